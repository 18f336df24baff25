"""nmarl_lstm_bptt_dial without a GPU: the kernel's resource budget as the compiler reports it, the `supported` predicate that
keeps every other case on the step-wise pair, and the argument struct against the C compiler's layout."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dial_instantiations_fit_the_register_budget():
    """The four lstm_dial instantiations of lstm_bptt_coupled_kernel (message rows of 64 / 128 floats x heads' gradient as a tensor /
    as dy8): no scratch and at most 256 VGPRs + AGPRs (512 threads per CU: two waves per SIMD)."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import resource_usage
    finally:
        sys.path.pop(0)
    def is_dial(name):               # lstm_bptt_coupled_kernel<NTM, RMAX, MASK, DY, DIAL = true>
        args = [x.strip() for x in name.rstrip('>').split('<', 1)[-1].split(',')]
        return name.startswith('lstm_bptt_coupled_kernel<') and len(args) == 5 and args[4] == 'true'
    rows = [r for r in resource_usage.usage(os.path.join(resource_usage.CSRC, 'lstm_bptt.hip')) if is_dial(r['name'])]
    assert len(rows) == 4, [r['name'] for r in rows]
    for r in rows:
        assert r['ScratchSize [bytes/lane]'] == 0, r
        assert r['VGPRs Spill'] == 0, r
        assert r['VGPRs'] + r['AGPRs'] <= 256, r


def _line(N):
    from deeprl_network_amd import ops
    nm = np.zeros((N, N), dtype=int)
    for i in range(N - 1):
        nm[i, i + 1] = nm[i + 1, i] = 1
    return ops.neighbor_table(nm, 'cpu')[0]


def test_supported_predicate():
    from deeprl_network_amd import ops
    assert ops.COUPLED_DIAL == 3
    idx = _line(8)
    rev = ops.reverse_neighbor_table(idx, ops.COUPLED_NC)
    assert rev['r_max'] == 2
    # the line table: inside the envelope -- on a GPU (the device is the only thing a CPU run lacks)
    assert ops.bptt_dial_supported(2, 64, rev=None, device='cuda')
    assert ops.bptt_dial_supported(2, 64, rev=dict(rev, rev_w=_Dev('cuda')))
    assert ops.bptt_dial_supported(1, 64, device='cuda')
    assert not ops.bptt_dial_supported(4, 64, device='cuda')                            # the 5x5 grid: stays on the step-wise pair
    assert not ops.bptt_dial_supported(2, 32, device='cuda')
    assert not ops.bptt_dial_supported(2, 128, device='cuda')
    assert not ops.bptt_dial_supported(2, 64, rev=dict(rev, r_max=3, rev_w=_Dev('cuda')))       # more than 2 sources per agent
    assert not ops.bptt_dial_supported(2, 64, rev=dict(rev, r_max=4), device='cuda')
    # CPU tensors (tests/cpu_emulation.py does not patch the op): the old path
    assert not ops.bptt_dial_supported(2, 64, rev=rev)
    assert not ops.bptt_dial_supported(2, 64, rev=rev, device='cpu')
    assert not ops.bptt_dial_supported(2, 64, device=torch.device('cpu'))


class _Dev:
    """Stands for a device tensor in the reverse table: the predicate only asks where it lives."""

    def __init__(self, kind):
        self.device = torch.device(kind)


def test_dial_policy_keeps_the_tensor_form_on_the_cpu():
    from deeprl_network_amd.agents import policies
    from test_sequence_cpu import _masks
    nb, n_feat, A = _masks('line')
    pol = policies.DIALMultiAgentPolicy(n_feat, A, nb, device='cpu')
    assert pol.bptt_takes_head_dy is False


def test_struct_layout_matches_c_compiler(tmp_path):
    from deeprl_network_amd import _lib
    header = os.path.join(ROOT, 'include', 'nmarl.h')
    fields = [n for n, _ in _lib.BpttDial._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu", sizeof(nmarl_bptt_dial_t));\n' % header
    for f in fields:
        src += 'printf(" %%zu", offsetof(nmarl_bptt_dial_t, %s));\n' % f
    src += 'return 0;}\n'
    c = tmp_path / 'off.c'
    c.write_text(src)
    exe = str(tmp_path / 'off')
    subprocess.check_call(['gcc', str(c), '-o', exe])
    nums = [int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert nums[0] == ctypes.sizeof(_lib.BpttDial)
    assert nums[1:] == [getattr(_lib.BpttDial, f).offset for f in fields]
    assert hasattr(_lib.lib, 'nmarl_lstm_bptt_dial')

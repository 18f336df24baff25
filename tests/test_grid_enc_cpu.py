"""The general-layout input encoders of the lock-step launch without a GPU: the `supported` predicates, the widened argument
struct against the header, and the register budget of the two new instantiations as the compiler reports it."""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_supported_predicates(monkeypatch):
    from deeprl_network_amd import ops
    monkeypatch.delenv('NMARL_INKERNEL_ENCODE', raising=False)
    # the ATSC grid: 12 own features, 5 actions, up to 4 neighbours, 25 agents
    assert ops.step_enc_supported(12, 5, 4, 64, 64, 25)
    assert ops.step_enc1_supported(12, 4, 64, 64, 25) and ops.step_enc1_supported(12, 0, 64, 64, 25)
    # CACC, as before
    assert ops.step_enc_supported(5, 4, 2, 64, 64, 8) and ops.step_enc_supported(5, 4, 2, 64, 64, 32)
    assert ops.step_enc1_supported(5, 2, 64, 64, 8) and ops.step_enc1_supported(5, 0, 64, 64, 8)
    assert not ops.step_enc_supported(5, 5, 2, 64, 64, 8) and not ops.step_enc_supported(5, 4, 1, 64, 64, 8)
    assert not ops.step_enc1_supported(5, 1, 64, 64, 8) and not ops.step_enc1_supported(5, 4, 64, 64, 8)
    # outside the envelope
    assert not ops.step_enc_supported(10, 5, 4, 64, 64, 25) and not ops.step_enc1_supported(10, 4, 64, 64, 25)      # F no multiple of 4
    assert not ops.step_enc_supported(8, 5, 5, 64, 64, 25) and not ops.step_enc1_supported(8, 5, 64, 64, 25)        # five slots
    assert not ops.step_enc_supported(12, 5, 4, 64, 64, 33) and not ops.step_enc1_supported(12, 4, 64, 64, 33)      # the by-value table
    assert not ops.step_enc_supported(16, 5, 4, 64, 64, 25)                    # 80 observation inputs
    assert not ops.step_enc_supported(12, 9, 4, 64, 64, 25)                    # 36 fingerprint inputs
    assert not ops.step_enc_supported(12, 5, 0, 64, 64, 25)                    # fingerprints need neighbours
    assert not ops.step_enc_supported(12, 5, 4, 32, 64, 25) and not ops.step_enc_supported(12, 5, 4, 64, 128, 25)
    assert ops.step_enc_cacc_layout(5) and not ops.step_enc_cacc_layout(12)   # (a coupled net's launch has the CACC forms only)
    monkeypatch.setenv('NMARL_INKERNEL_ENCODE', '0')
    assert not ops.step_enc_supported(12, 5, 4, 64, 64, 25) and not ops.step_enc1_supported(12, 4, 64, 64, 25)
    assert not ops.step_enc_supported(5, 4, 2, 64, 64, 8)


def test_cpu_emulation_keeps_the_grid_on_the_separate_encoders():
    from oracle import ops_ref
    assert not ops_ref.step_enc_supported(12, 5, 4, 64, 64, 25)


def test_step_enc_struct_holds_four_slots_for_32_agents():
    from deeprl_network_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'nmarl.h')).read()
    body = re.search(r'typedef struct nmarl_step_enc \{(.*?)\} nmarl_step_enc_t;', src, flags=re.S).group(1)
    n = int(re.search(r'int32_t nbr\[(\d+)\];', body).group(1))
    assert n == 32 * 4
    assert _lib.StepEnc.nbr.size == 4 * n and _lib.StepEnc.nbr.offset == _lib.StepEnc.pad_.offset + 4
    assert _lib.StepEnc.env.offset == _lib.StepEnc.nbr.offset + 4 * n
    assert _lib.StepEnc.relu_bits_sn.offset + 8 == ctypes.sizeof(_lib.StepEnc)
    assert _lib.ABI_VERSION == 4
    assert re.search(r'nmarl_abi_version\(void\) \{ return 4; \}', open(os.path.join(ROOT, 'deeprl_network_amd', 'csrc', 'cacc.hip')).read())


def test_general_layout_instantiations_fit_the_register_budget():
    """lstm_step_x_kernel<3,0,3> (both encoders) and <3,0,4> (the observation encoder alone): no scratch, no spills, at most 256
    VGPRs + AGPRs (512 threads per CU); the table goes to profiles/r10_resource_usage_grid_enc.txt when REGEN_PROFILES=1."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import resource_usage
    finally:
        sys.path.pop(0)
    want = {'lstm_step_x_kernel<3, 0, 3, 0, 0>', 'lstm_step_x_kernel<3, 0, 4, 0, 0>'}
    rows = [r for r in resource_usage.usage(os.path.join(resource_usage.CSRC, 'lstm_mfma.hip')) if r['name'] in want]
    assert {r['name'] for r in rows} == want, [r['name'] for r in rows]
    lines = ['%-40s VGPRs %3d  AGPRs %3d  SGPRs %3d  scratch %d B/lane  VGPR spill %d  waves/SIMD %d' % (
        r['name'], r['VGPRs'], r['AGPRs'], r['TotalSGPRs'], r['ScratchSize [bytes/lane]'], r['VGPRs Spill'], r['Occupancy [waves/SIMD]'])
        for r in sorted(rows, key=lambda r: r['name'])]
    print('\n'.join(lines))
    if os.environ.get('REGEN_PROFILES') == '1':
        path = os.path.join(ROOT, 'profiles', 'r10_resource_usage_grid_enc.txt')
        head = ('hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Rpass-analysis=kernel-resource-usage, csrc/lstm_mfma.hip: the lock-step\n'
                'launch with the input encoders on the general layout (tests/test_grid_enc_cpu.py)\n\n')
        open(path, 'w').write(head + '\n'.join(lines) + '\n')
    for r in rows:
        assert r['ScratchSize [bytes/lane]'] == 0, r
        assert r['VGPRs Spill'] == 0, r
        assert r['VGPRs'] + r['AGPRs'] <= 256, r

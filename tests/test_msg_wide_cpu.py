"""Host side of lstm_comm's in-kernel message term at three and four neighbour slots: which (kind, m_max) the step kernel's
pre-phase takes, and the resources of the two instantiations that carry the streamed form."""
import functools
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# lstm_step_x_kernel<HEAD, MSG, ENC, CARRY, PREC>: every instantiation the library carries (the streamed form adds none)
STEP_KERNELS = sorted(
    ['lstm_step_x_kernel<%d, %d, 0, 0, 0>' % (hd, ms) for hd in (0, 1, 2, 3) for ms in (0,)] +
    ['lstm_step_x_kernel<%d, %d, 0, 0, 0>' % (hd, ms) for hd in (1, 2) for ms in (1, 2, 3)] +
    ['lstm_step_x_kernel<4, %d, 0, %d, 0>' % (ms, cy) for ms in (1, 2) for cy in (0, 1, 2)] +
    ['lstm_step_x_kernel<4, 1, 1, %d, 0>' % cy for cy in (0, 1, 2)] +
    ['lstm_step_x_kernel<%d, 0, 0, 0, 1>' % hd for hd in (0, 1, 2, 3)] +
    ['lstm_step_x_kernel<3, 0, %d, 0, 0>' % en for en in (1, 2, 3, 4)] +
    ['lstm_step_x_kernel<3, 0, %d, 0, 1>' % en for en in (1, 2)])


@functools.lru_cache(maxsize=None)
def step_rows():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import resource_usage
    rows = resource_usage.usage(os.path.join(ROOT, 'deeprl_network_amd', 'csrc', 'lstm_mfma.hip'))
    return {r['name']: r for r in rows if r['name'].startswith('lstm_step_x_kernel<')}


def test_msg_supported_truth_table():
    from deeprl_network_amd import ops
    H = 64
    assert [ops.msg_supported(ops.MSG_GATHER_RELU, m, H) for m in (1, 2, 3, 4, 5)] == [True, True, True, True, False]
    assert [ops.msg_supported(ops.MSG_DIAL, m, H) for m in (1, 2, 3, 4)] == [True, True, False, False]
    # lstm_ic3 averages its neighbours: 64 floats whatever their number (up to the kernel's 8 slots)
    assert [ops.msg_supported(ops.MSG_MEAN_ADD, m, H) for m in (1, 2, 4, 8, 9)] == [True, True, True, True, False]
    assert not any(ops.msg_supported(k, 2, 32) for k in (ops.MSG_GATHER_RELU, ops.MSG_MEAN_ADD, ops.MSG_DIAL))
    # the one-launch lock-step (head kind 3) keeps the resident image: its bound is the name the tests of the narrow form read
    assert ops.MSG_MAX_K == 128 and ops.MSG_KIND_MAX_K[ops.MSG_GATHER_RELU] == 256


def test_one_launch_is_not_chosen_past_the_resident_image():
    """BatchedPolicy.pv_one_launch answers False for lstm_comm with K > 128 before it asks the device anything."""
    from deeprl_network_amd import ops
    from deeprl_network_amd.agents.policies import BatchedPolicy

    class P:
        fused_pv, fused_pv_coupled, msg_kind, n_h, N, device = False, True, ops.MSG_GATHER_RELU, 64, 25, 'cpu'

        def __init__(self, m_max):
            self.m_max = m_max
    asked = []
    orig = ops.step_handoff_supported
    ops.step_handoff_supported = lambda N, E, device, K=128: (asked.append(K), True)[1]
    try:
        assert BatchedPolicy.pv_one_launch(P(4), 130) is False and BatchedPolicy.pv_one_launch(P(3), 130) is False
        assert asked == []
        assert BatchedPolicy.pv_one_launch(P(2), 130) is True and asked == [128]
    finally:
        ops.step_handoff_supported = orig


@pytest.mark.parametrize('name', ['lstm_step_x_kernel<1, 1, 0, 0, 0>', 'lstm_step_x_kernel<2, 1, 0, 0, 0>'])
def test_streamed_forms_do_not_spill(name):
    r = step_rows()[name]
    assert r['ScratchSize [bytes/lane]'] == 0 and r['VGPRs Spill'] == 0 and r['VGPRs'] + r.get('AGPRs', 0) <= 256, r


def test_no_new_instantiation():
    assert sorted(step_rows()) == STEP_KERNELS

"""tests/sequence_tier_checks.py on the real kernels: the tier / kind pairs a configuration reaches (lstm_comm one-launch and
step-wise, lstm_ic3 one-launch, lstm_dial through nmarl_lstm_bptt_dial and through the step-wise pair with the adjoint kernel), the
torch tier of every kind, every buffer layout, and the uncoupled Functions.  E = 132: one full 128-row tile and a ragged tail, and
(T + 1) E a multiple of ops.WGRAD_SPLIT."""
import pytest

import sequence_tier_checks as stc

pytestmark = pytest.mark.gpu

E = 132


@pytest.mark.parametrize('kind,tier,layout,mask', stc.GPU_COUPLED_CASES)
def test_coupled_tiers(kind, tier, layout, mask):
    from deeprl_network_amd import ops
    from deeprl_network_amd.agents import sequence
    stc.check_coupled(ops, sequence, 'cuda', kind, tier, layout, mask, E)


@pytest.mark.parametrize('kind', stc.KINDS)
def test_coupled_separate_weights(kind):
    from deeprl_network_amd import ops
    from deeprl_network_amd.agents import sequence
    for tier in ('one', 'torch'):
        stc.check_coupled(ops, sequence, 'cuda', kind, tier, 'padded', 'first', E, flat_weights=False)


@pytest.mark.parametrize('fn,tier,layout,mask,form', stc.UNCOUPLED_CASES)
def test_uncoupled_tiers(fn, tier, layout, mask, form):
    from deeprl_network_amd import ops
    assert ((stc.T + 1) * E) % ops.WGRAD_SPLIT == 0
    stc.check_uncoupled(ops, 'cuda', fn, tier, layout, mask, form, E)

"""tests/sequence_tier_checks.py on the CPU, the ops patched by cpu_ops(): every tier and layout of the update's reverse recurrence
runs its host code here (cpu_emulation replaces ops.lstm_sequence* wholesale, so the Functions are called directly) -- and
ops.take_head_dy's hand-over of the heads' dy8."""
import pytest
import torch

import sequence_tier_checks as stc
from cpu_emulation import cpu_ops

E_COUPLED, E_UNCOUPLED, E_FALLBACK = 2, 4, 3


@pytest.mark.parametrize('kind,tier,layout,mask', stc.COUPLED_CASES)
def test_coupled_tiers(kind, tier, layout, mask):
    from deeprl_network_amd import ops
    from deeprl_network_amd.agents import sequence
    with cpu_ops():
        stc.check_coupled(ops, sequence, 'cpu', kind, tier, layout, mask, E_COUPLED)


@pytest.mark.parametrize('kind', stc.KINDS)
def test_coupled_separate_weights(kind):
    """wx and wh in buffers of their own: the torch tier's dgrad is two GEMMs, the fused tiers build their image from both."""
    from deeprl_network_amd import ops
    from deeprl_network_amd.agents import sequence
    with cpu_ops():
        for tier in ('one', 'torch'):
            stc.check_coupled(ops, sequence, 'cpu', kind, tier, 'padded', 'first', E_COUPLED, flat_weights=False)


@pytest.mark.parametrize('fn,tier,layout,mask,form', stc.UNCOUPLED_CASES)
def test_uncoupled_tiers(fn, tier, layout, mask, form):
    from deeprl_network_amd import ops
    assert ((stc.T + 1) * E_UNCOUPLED) % ops.WGRAD_SPLIT == 0
    with cpu_ops():
        stc.check_uncoupled(ops, 'cpu', fn, tier, layout, mask, form, E_UNCOUPLED)


@pytest.mark.parametrize('tier', stc.UNCOUPLED_TIERS)
def test_uncoupled_padded_layout_refused_by_the_row_split(tier):
    """(T + 1) E = 12 is no multiple of ops.WGRAD_SPLIT: the padded buffer is offered and the flat layout is taken."""
    from deeprl_network_amd import ops
    assert ((stc.T + 1) * E_FALLBACK) % ops.WGRAD_SPLIT != 0
    with cpu_ops():
        stc.check_uncoupled(ops, 'cpu', 'saved', tier, 'padded', 'first', 'dy8', E_FALLBACK)


# ------------------------------------------------------------------------------------------------------ ops.take_head_dy
def _saved_sequence(ops):
    c = stc.case('x', 'first', E_UNCOUPLED, 'dy8')
    sv, p, x = c['saved'], c['p'], c['x']
    prm = {k: p[k].clone().requires_grad_(True) for k in ('wx', 'wh', 'b')}
    s = x['enc'].clone().requires_grad_(True)
    Hs = ops._LstmSequenceSaved.apply(s, prm['wx'], prm['wh'], prm['b'], sv['G'].clone(), sv['H'].clone(), sv['C'].clone(), c['done'].clone(), (0,),
                                      None)
    return c, prm, s, Hs


def test_placeholder_hands_dy8_to_the_recurrence():
    from deeprl_network_amd import ops
    with cpu_ops(), stc.spied(ops) as calls:
        ops._pending_head_dy.clear()
        c, prm, s, Hs = _saved_sequence(ops)
        Hs.backward(gradient=ops.head_dy_placeholder(c['x']['dy8'], c['x']['hw'], Hs))
        assert calls['bptt_seq'] == [True] and not ops._pending_head_dy
    torch.testing.assert_close(prm['wh'].grad.double(), c['ref']['wh'], rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize('how', ['second consumer', 'contiguous copy'])
def test_gradient_that_is_not_the_placeholder_leaves_the_entry_pending(how):
    """Something else contributed to dL/dh, or the placeholder was materialised on the way: the recurrence gets a real tensor (all
    zero where it stands for the placeholder) and must NOT consume the dy8 entry -- the caller's check (models._loss_backward_fused:
    an entry still pending after backward) then raises instead of training on a wrong gradient."""
    from deeprl_network_amd import ops
    with cpu_ops(), stc.spied(ops) as calls:
        ops._pending_head_dy.clear()
        c, prm, s, Hs = _saved_sequence(ops)
        ph = ops.head_dy_placeholder(c['x']['dy8'], c['x']['hw'], Hs)
        if how == 'second consumer':
            torch.autograd.backward([Hs, (Hs * 2.0).sum()], [ph, None])
        else:
            Hs.backward(gradient=ph.contiguous())
        assert calls['bptt_seq'] == [False], 'the recurrence took dy8 although its gradient was not the placeholder'
        pend = ops._pending_head_dy.pop(Hs.device, None)
        assert pend is not None and pend[0] is ph, 'the pending entry is gone: the caller cannot notice'


def test_stale_entry_is_never_taken_by_a_later_backward():
    from deeprl_network_amd import ops
    with cpu_ops(), stc.spied(ops) as calls:
        ops._pending_head_dy.clear()
        c, prm, s, Hs = _saved_sequence(ops)
        ops.head_dy_placeholder(c['x']['dy8'], c['x']['hw'], Hs)          # handed to nobody: stays behind
        _, _, _, Hs2 = _saved_sequence(ops)
        Hs2.backward(gradient=torch.zeros_like(Hs2))
        assert calls['bptt_seq'] == [False], 'a backward with a tensor gradient took an earlier backward\'s dy8'
        ops._pending_head_dy.clear()

"""The edge checks of tests/fc_edge_checks.py are sharp: (a) the restatement oracle/ops_ref (fp32 on the CPU) stays within every
bound, (b) every named wrong variant of it -- mistakes the encoder / heads kernels of csrc/fc.hip, the neighbour kernels of
csrc/nbr.hip and the step kernels' transcendentals could make without the older tests noticing -- fails the assertion that targets
it (the tag in brackets that opens the assertion's message).

ops.heads_loss has no restatement (tests/helpers.py: the CPU emulation takes the autograd heads): `_heads_loss` below builds one
from ops_ref.heads + ops_ref.a2c_loss under fp32 autograd, and the wrong variants perturb that adapter.  Likewise ops.cell_fwd."""
import types

import pytest
import torch

import fc_edge_checks as fec
from oracle import ops_ref

_NAMES = ('fc_bwd', 'fc_fwd_multi', 'nbr_gather', 'nbr_mean', 'nbr_gather_bwd', 'nbr_mean_bwd', 'lstm_wimage', 'lstm_step_fused', 'cell_bwd',
          'bptt_step', 'bptt_seq', 'lstm_bptt_wimage', 'nbr_action_value', 'onehot_argmax_add_', 'thin_linear_bwd')


# ------------------------------------------------------------------------------------------------ adapters and variants
def _a2c_terms(logits, v, action, adv, R, v_coef, e_coef, variant):
    """ops_ref.a2c_loss (policies.py:20-30) with one mistake switched on."""
    if variant == 'no max subtraction':
        e = torch.exp(logits)
        pi = e / e.sum(-1, keepdim=True)
    else:
        pi = torch.softmax(logits, dim=-1)
    acts = action.t().long().unsqueeze(-1)
    if variant == 'log(p + 1e-10)':
        log_pi = torch.log(pi + 1e-10)
    else:
        log_pi = torch.log(torch.clamp(pi, 1e-8 if variant == 'clip at 1e-8' else 1e-10, 1.0))
    free = log_pi.detach() + (torch.log(pi) - torch.log(pi).detach())          # the clipped value with the unclipped gradient 1 / p
    entropy = -(pi * (free if variant == 'entropy gradient unclipped' else log_pi)).sum(-1)
    logp_a = (free if variant == 'policy gradient not blocked' else log_pi).gather(-1, acts).squeeze(-1)
    terms = torch.stack([-(logp_a * adv).mean(-1), (R - v).pow(2).mean(-1) * 0.5 * v_coef, -entropy.mean(-1) * e_coef], dim=1)
    return terms.sum(dim=1), terms.detach()


def _heads_loss(variant=None):
    """ops.heads_loss restated: ops_ref.heads -> ops_ref.a2c_loss -> backward, fp32, the same dict."""
    def f(h, pi_w, pi_b, v_w, v_b, action, nbr_idx, n_a, adv, R, v_coef, e_coef, want_dh=True):
        ts = [t.clone().requires_grad_(True) for t in (h, pi_w, pi_b, v_w, v_b)]
        logits, v = ops_ref.heads(*ts, action, nbr_idx, n_a)
        logits.retain_grad()
        v.retain_grad()
        if variant is None:
            tot, terms = ops_ref.a2c_loss(logits, v, action, adv, R, v_coef, e_coef)
        else:
            tot, terms = _a2c_terms(logits, v, action, adv, R, v_coef, e_coef, variant)
        tot.sum().backward()
        N, rows, _ = h.shape
        dy8 = torch.zeros(N, rows, 8)
        dy8[..., :n_a], dy8[..., n_a] = logits.grad, v.grad
        return dict(terms=terms, dh=ts[0].grad if want_dh else None, dy8=dy8, hw=None, pi_w=ts[1].grad, pi_b=ts[2].grad, v_w=ts[3].grad,
                    v_b=ts[4].grad)
    return f


def _cell(z, bias, c_prev, done, gates, c_new, h_new, sig=torch.sigmoid, tanh=torch.tanh):
    """agents/utils.py:102-113 with the gates kept (fp32)."""
    Hc = c_prev.shape[-1]
    zb = z + bias.unsqueeze(1)
    i, f, o, u = sig(zb[..., :Hc]), sig(zb[..., Hc:2 * Hc]), sig(zb[..., 2 * Hc:3 * Hc]), tanh(zb[..., 3 * Hc:])
    c = f * (c_prev * (1.0 - done).view(1, -1, 1)) + i * u
    if gates is not None:
        gates.copy_(torch.cat([i, f, o, u], dim=-1))
    c_new.copy_(c)
    h_new.copy_(o * tanh(c))


def _cell_fwd(z, bias, c_prev, done, gates, c_new, h_new, z2=None):
    _cell(z if z2 is None else z + z2, bias, c_prev, done, gates, c_new, h_new)


def _step_variant(kind):
    """The plain step (KX = 0, one addend) with a wrong transcendental."""
    sig, tanh = torch.sigmoid, torch.tanh
    if kind == 'tanh as (e^2x - 1) / (e^2x + 1)':
        tanh = lambda x: (torch.exp(2 * x) - 1) / (torch.exp(2 * x) + 1)                # noqa: E731
    if kind == 'sigmoid through fp16':
        sig = lambda x: torch.sigmoid(x.half().float()).half().float()                  # noqa: E731

    def f(h, wh, bias, zadd1, zadd2, c_prev, done, gates, c_out, h_out, xs=None):
        z = torch.bmm(h * (1.0 - done).view(1, -1, 1), wh) + zadd1
        _cell(z, bias, c_prev, done, gates, c_out, h_out, sig=sig, tanh=tanh)
        return h_out, c_out
    return f


def _impl(**replaced):
    ns = types.SimpleNamespace(**{k: getattr(ops_ref, k) for k in _NAMES})
    ns.heads_loss, ns.cell_fwd = _heads_loss(), _cell_fwd
    for k, v in replaced.items():
        setattr(ns, k, v)
    return ns


def _act_of(rows, F, layout):
    return (rows + F + len(layout)) % 3


# ------------------------------------------------------------------------------------------ (a) the restatement passes
@pytest.mark.parametrize('layout', fec.FC_BWD_LAYOUTS)
@pytest.mark.parametrize('F', fec.FC_BWD_F)
@pytest.mark.parametrize('rows', fec.FC_BWD_ROWS)
def test_restatement_fc_bwd_rows(rows, F, layout):
    for N in (2, 5):
        fec.check_fc_bwd_rows(_impl(), 'cpu', N, rows, F, layout, _act_of(rows, F, layout))
    fec.check_fc_bwd_rows(_impl(), 'cpu', 5, rows, F, layout, 1 + rows % 2, gather=True)


@pytest.mark.parametrize('case', fec.FC_MULTI_CASES)
@pytest.mark.parametrize('rows', fec.FC_MULTI_ROWS)
def test_restatement_fc_fwd_multi(rows, case):
    fec.check_fc_fwd_multi(_impl(), 'cpu', rows, case)


@pytest.mark.parametrize('F', fec.NBR_F)
@pytest.mark.parametrize('E', fec.NBR_E)
def test_restatement_nbr_ragged(E, F):
    fec.check_nbr_ragged(_impl(), 'cpu', E, F)


@pytest.mark.parametrize('want_dh', [True, False])
@pytest.mark.parametrize('A', fec.HEADS_LOSS_A)
@pytest.mark.parametrize('rows', fec.HEADS_LOSS_ROWS)
@pytest.mark.parametrize('N', fec.HEADS_LOSS_N)
def test_restatement_heads_loss_clip(N, rows, A, want_dh):
    fec.check_heads_loss_clip(_impl(), 'cpu', N, rows, A, want_dh)


@pytest.mark.parametrize('path', ['step', 'cell'])
def test_restatement_gate_sweep(path):
    fec.check_gate_sweep(_impl(), 'cpu', path)


@pytest.mark.parametrize('part', fec.BPTT_SAT_PARTS)
def test_restatement_bptt_saturated(part):
    fec.check_bptt_saturated(_impl(), 'cpu', part)


def test_restatement_small_things():
    for rows in (1, 300):
        fec.check_nbr_action_value_accumulate(_impl(), 'cpu', rows)
    fec.check_onehot_argmax_ties(_impl(), 'cpu')
    for rows in (63, 65):
        fec.check_thin_linear_bwd_o8(_impl(), 'cpu', rows)


# ------------------------------------------------------------------------------------------ (b) the wrong variants fail
HEADS_LOSS_MUTANTS = {
    'entropy gradient unclipped': 'entropy',         # -(log p + 1) everywhere
    'policy gradient not blocked': 'blocked',        # when the taken action is clipped
    'log(p + 1e-10)': 'blocked',                     # instead of log(max(p, 1e-10)): its gradient p / (p + 1e-10) is not 0
    'no max subtraction': 'finite',                  # exp(90 + ...) overflows
    'clip at 1e-8': 'terms',
}


def test_heads_loss_adapter_without_a_mistake_is_the_restatement():
    """_a2c_terms with no variant switched on == ops_ref.a2c_loss, gradients included: the variants differ from the restatement by
    their one mistake alone."""
    d = fec.heads_loss_inputs(2, 129, 4)
    outs = []
    for fn in (ops_ref.a2c_loss, lambda *a: _a2c_terms(*a, variant=None)):
        lg = (torch.randn(2, 129, 4, generator=torch.Generator().manual_seed(1)) * 3).requires_grad_(True)
        tot, terms = fn(lg, d['R'] * 0.5, d['action'], d['adv'], d['R'], 0.5, 0.01)
        tot.sum().backward()
        outs.append((terms, lg.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize('want_dh', [True, False])
@pytest.mark.parametrize('name', list(HEADS_LOSS_MUTANTS))
def test_heads_loss_mutant_fails_its_assertion(name, want_dh):
    for N, rows, A in ((5, 1003, 5), (2, 129, 4), (5, 129, 3), (2, 1003, 7)):
        with pytest.raises(AssertionError, match=r'^\[%s\]' % HEADS_LOSS_MUTANTS[name]):
            fec.check_heads_loss_clip(_impl(heads_loss=_heads_loss(name)), 'cpu', N, rows, A, want_dh)


def test_heads_loss_mutants_pass_on_well_behaved_logits():
    """On logits without the knocked-out columns and without the shifted agent -- what test_heads_loss_one_pass_vs_torch feeds --
    four of the five wrong variants are the restatement to within the tolerances: the regime is what pins them."""
    g = torch.Generator().manual_seed(7)
    N, rows, A = 3, 257, 4
    logits = torch.randn(N, rows, A, generator=g) * 1.5
    v, adv, R = (torch.randn(N, rows, generator=g) for _ in range(3))
    action = torch.randint(0, A, (rows, N), generator=g).to(torch.uint8)

    def grads(variant):
        lg = logits.clone().requires_grad_(True)
        tot, terms = _a2c_terms(lg, v, action, adv, R, 0.5, 0.01, variant)
        tot.sum().backward()
        return terms, lg.grad
    t0, g0 = grads(None)
    for name in HEADS_LOSS_MUTANTS:
        t1, g1 = grads(name)
        torch.testing.assert_close(t1, t0, rtol=2e-5, atol=1e-7)
        torch.testing.assert_close(g1, g0, rtol=2e-4, atol=2e-6 * float(g0.abs().max()))


GATE_MUTANTS = {'tanh as (e^2x - 1) / (e^2x + 1)': 'finite', 'sigmoid through fp16': 'sigmoid-rel'}


@pytest.mark.parametrize('name', list(GATE_MUTANTS))
def test_gate_sweep_mutant_fails_its_assertion(name):
    with pytest.raises(AssertionError, match=r'^\[%s\]' % GATE_MUTANTS[name]):
        fec.check_gate_sweep(_impl(lstm_step_fused=_step_variant(name)), 'cpu', 'step')


def test_gate_sweep_variant_without_a_mistake_passes():
    fec.check_gate_sweep(_impl(lstm_step_fused=_step_variant(None)), 'cpu', 'step')


def _fc_bwd_variant(kind):
    def f(x, y, dy, act, nbr_idx=None):
        rows = y.shape[1]
        if kind == 'last ragged tile dropped' and rows > 64:
            keep = rows // 64 * 64
            return ops_ref.fc_bwd(x[:, :keep], y[:, :keep], dy[:, :keep], act, nbr_idx=nbr_idx)
        if kind == 'padded slot reads agent 0' and nbr_idx is not None:
            nbr_idx = nbr_idx.clamp(min=0)
        if kind == 'tanh derivative from 1 - y':
            g = dy * (1.0 - y) if act == 2 else dy * (y > 0).to(dy.dtype) if act == 1 else dy
            xx = x if nbr_idx is None else ops_ref.nbr_gather(x, nbr_idx)
            return torch.bmm(xx.transpose(1, 2), g), g.sum(1)
        return ops_ref.fc_bwd(x, y, dy, act, nbr_idx=nbr_idx)
    return f


FC_BWD_MUTANTS = {
    'last ragged tile dropped': dict(rows=65, F=20, act=1, gather=False),
    'padded slot reads agent 0': dict(rows=63, F=15, act=1, gather=True),
    'tanh derivative from 1 - y': dict(rows=130, F=60, act=2, gather=False),
}


@pytest.mark.parametrize('name', list(FC_BWD_MUTANTS))
def test_fc_bwd_mutant_fails(name):
    kw = FC_BWD_MUTANTS[name]
    with pytest.raises(AssertionError):
        fec.check_fc_bwd_rows(_impl(fc_bwd=_fc_bwd_variant(name)), 'cpu', 5, kw['rows'], kw['F'], 'pitch66', kw['act'], gather=kw['gather'])


def _transposed(tab):
    """The table of the reversed graph (who lists me), -1 padded to the same width."""
    N, m = tab.shape
    out = -torch.ones(N, N, dtype=torch.int32)
    for j in range(N):
        src = [i for i in range(N) if j in tab[i].tolist()]
        out[j, :len(src)] = torch.tensor(src, dtype=torch.int32)
    return out[:, :m]


NBR_MUTANTS = {
    'mean divides by m_max': dict(nbr_mean=lambda x, tab: ops_ref.nbr_mean(x, tab) * ((tab >= 0).sum(1).float() / tab.shape[1]).view(-1, 1, 1)),
    'mean adjoint over the reversed graph': dict(nbr_mean_bwd=lambda dy, tab, add=None: ops_ref.nbr_mean_bwd(dy, _transposed(tab), add=add)),
    'add left out': dict(nbr_gather_bwd=lambda dy, tab, F, add=None: ops_ref.nbr_gather_bwd(dy, tab, F)),
    'a padded slot gathers agent 0': dict(nbr_gather=lambda x, tab: ops_ref.nbr_gather(x, tab.clamp(min=0))),
}


@pytest.mark.parametrize('name', list(NBR_MUTANTS))
def test_nbr_mutant_fails(name):
    with pytest.raises(AssertionError):
        fec.check_nbr_ragged(_impl(**NBR_MUTANTS[name]), 'cpu', 33, 12)


def test_fc_fwd_multi_mutant_fails():
    """A layer that writes all 64 + 64 columns from the first layer's block start (a wrong column offset) and one that runs past
    its block into the guard columns."""
    def shifted(parts, act, out=None):
        y = ops_ref.fc_fwd_multi(parts, act)
        out.copy_(torch.roll(y, 64, dims=-1))
        return out

    def overrun(parts, act, out=None):
        ops_ref.fc_fwd_multi(parts, act, out=out)
        wide = out._base if out._base is not None else out
        wide.view(-1)[-1] = 0.0
        return out
    for fn in (shifted, overrun):
        with pytest.raises(AssertionError):
            fec.check_fc_fwd_multi(_impl(fc_fwd_multi=fn), 'cpu', 65, 'pitch130')


def test_bptt_saturated_mutant_fails():
    """A cell backward that takes the sigmoid's derivative from a clamped gate (a guard against 0 * inf that a kernel might carry)
    leaves dz != 0 at the saturated gates."""
    def cell_bwd(gates, c_prev, c_new, done, dh, dc, dz, dc_prev, dh2=None):
        g = gates.clone()
        g[..., :3 * fec.H] = g[..., :3 * fec.H].clamp(1e-7, 1 - 1e-7)
        ops_ref.cell_bwd(g, c_prev, c_new, done, dh, dc, dz, dc_prev, dh2=dh2)
    with pytest.raises(AssertionError, match='exactly 0'):
        fec.check_bptt_saturated(_impl(cell_bwd=cell_bwd), 'cpu', 'cell_bwd')

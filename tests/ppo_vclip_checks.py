"""Shared by the tests of the opt-in value clipping and KL stop of the PPO epochs (MODEL_CONFIG ppo_vclip, ppo_target_kl): the
float64 torch restatement of the six terms with the clipped value loss and -- through autograd -- its gradients; an input generator
that extends ppo_checks.inputs with v_old; the wrong variants the checks must tell from the definition; torch stand-ins of the two
gate kernels and of a guarded optimiser step.

Definition, per agent over rows = T*E; policy, entropy, approx_kl, clip_frac as in ppo_checks:
    d = v - v_old;  inside = |d| <= ev;  v_c = v_old + clip(d, -ev, +ev);  e1 = (R - v)^2;  e2 = (R - v_c)^2
    e = inside ? e1 : max(e1, e2);  value = 0.5 v_coef mean(e);  d value / d v = -v_coef (R - v) / rows where inside or e1 >= e2, else 0
    vclip_frac = mean(|d| > ev)
"""
import numpy as np
import torch

import ppo_checks as pc

F32, F64 = torch.float32, torch.float64
VCLIP = 0.25
HUGE = 1e30


def restate(logits, v, action, adv, R, logp_old, clip, v_coef, e_coef, v_old, vclip, wrong=None):
    """-> (total [N] differentiable, terms [N,6] detached) in the dtype of logits.  wrong: the name of one mistake (WRONG)."""
    _, t5 = pc.restate(logits, v, action, adv, R, logp_old, clip, v_coef, e_coef)
    tot5, _ = pc.restate(logits, v.detach(), action, adv, R, logp_old, clip, v_coef, e_coef)       # the value term's gradient: below
    if wrong == 'v_old from the new weights':
        v_old = v.detach()
    d = v - v_old
    inside = d.abs() <= vclip
    v_c = v_old + torch.clamp(d, -vclip, vclip)
    if wrong == 'clip around R instead of v_old':
        v_c = R + torch.clamp(v - R, -vclip, vclip)
    e1, e2 = (R - v).pow(2), (R - v_c).pow(2)
    open_ = inside | (e1 >= e2)
    # the gradient of the definition: through e1 where the row is open, none elsewhere (v_c is constant in v outside the clip range)
    e = torch.where(open_, e1, e2.detach())
    if wrong == 'min instead of max':
        e = torch.where(inside, e1, torch.min(e1, e2))
    if wrong == 'gradient through the clipped branch':
        e = e1 + (e - e1).detach()
    value = e.mean(-1) * (v_coef if wrong == 'value term with the 0.5 missing' else 0.5 * v_coef)
    over = d.abs() >= vclip if wrong == 'vclip_frac with >=' else d.abs() > vclip
    vf = over.to(logits.dtype).mean(-1)
    total = (tot5 - t5[:, 1]) + value
    terms = torch.stack([t5[:, 0], value.detach(), t5[:, 2], t5[:, 3], t5[:, 4], vf], dim=1)
    return total, terms.detach()


# 'vclip_frac with >=' can differ from the definition only ON the boundary, which `inputs` keeps every row away from: it is told
# apart on `inputs(..., boundary=True)`, whose vclip is row (0, 2)'s own |d|
WRONG = ['min instead of max', 'gradient through the clipped branch', 'clip around R instead of v_old', 'v_old from the new weights',
         'vclip_frac with >=', 'value term with the 0.5 missing']


def literal(logits, v, action, adv, R, logp_old, clip, v_coef, e_coef, v_old, vclip):
    """An independently written PPO2 loss: the value term is the textbook max of the two squared errors, left to autograd."""
    pi = torch.softmax(logits, dim=-1)
    lp = torch.log(torch.clamp(pi, 1e-10, 1.0))
    lp_a = lp.gather(-1, action.t().long().unsqueeze(-1)).squeeze(-1)
    rho = torch.exp(lp_a - logp_old)
    policy = -torch.min(rho * adv, torch.clamp(rho, 1.0 - clip, 1.0 + clip) * adv).mean(-1)
    v_clipped = v_old + torch.clamp(v - v_old, -vclip, vclip)
    value = 0.5 * v_coef * torch.max((R - v) ** 2, (R - v_clipped) ** 2).mean(-1)
    entropy = e_coef * (pi * lp).sum(-1).mean(-1)
    kl = ((rho - 1.0) - (lp_a - logp_old)).mean(-1)
    cf = ((rho - 1.0).abs() > clip).to(logits.dtype).mean(-1)
    vf = ((v - v_old).abs() > vclip).to(logits.dtype).mean(-1)
    return policy + value + entropy, torch.stack([policy, value, entropy, kl, cf, vf], dim=1).detach()


def inputs(N, rows, A, vclip=VCLIP, seed=0, boundary=False):
    """ppo_checks.inputs plus v_old [N,rows] f32 and vclip.  By row index modulo 5: 0 -> v_old = v (d = 0); 1 -> inside, |d| in
    [0.1, 0.8] vclip; 2 -> clipped with e2 > e1 (v moved past v_old TOWARDS R: the clipped value is the worse one, the gradient is
    closed); 3 -> clipped with e1 > e2 (v moved AWAY from R); 4 -> inside.  Asserted in float64 on the fp32 data: no row has
    ||d| - vclip| < MARGIN, no clipped row has |e1 - e2| < MARGIN max(e1, e2, 1) -- conditions on the data, so fp32 and float64
    cannot disagree by a branch flip; for rows >= 256 the three kinds occur on every agent.
    boundary: vclip becomes row (0, 2)'s own |d| (float64 equality on that row; the margins hold for every other row)."""
    d = pc.inputs(N, rows, A, seed=seed)
    g = torch.Generator().manual_seed(77000 + 1000 * N + rows + A + seed)
    v, R = d['v'].double(), d['R'].double()
    u = torch.rand(N, rows, generator=g, dtype=F64)
    sgn = torch.where(torch.rand(N, rows, generator=g) < 0.5, -1.0, 1.0).double()
    toward = torch.where(R >= v, 1.0, -1.0).double()          # the direction from v to R
    gap = (R - v).abs()
    kind = torch.arange(rows) % 5
    off = torch.zeros(N, rows, dtype=F64)
    small = sgn * vclip * (0.1 + 0.7 * u)
    # clipped, e2 > e1: v_old lies behind v as seen from R, at distance (1.3 .. 2.3) vclip: v_c = v_old + vclip is farther from R than v
    behind = -toward * vclip * (1.3 + u)
    # clipped, e1 > e2: v_old lies between v and R (or beyond R by less than the gap), v_c is closer to R than v
    ahead = toward * vclip * (1.3 + u)
    off = torch.where((kind == 1) | (kind == 4), small, off)
    off = torch.where(kind == 2, behind, off)
    off = torch.where(kind == 3, ahead, off)
    v_old = (v + off).float()
    v_old[:, ::5] = d['v'][:, ::5]
    hold = None
    if boundary:
        assert rows > 2
        hold = (0, 2)
        vclip = abs(float(d['v'][hold].double() - v_old[hold].double()))
        assert vclip > 0.01
    dd = v - v_old.double()
    near = (dd.abs() - vclip).abs() < pc.MARGIN
    v_c = v_old.double() + torch.clamp(dd, -vclip, vclip)
    e1, e2 = (R - v).pow(2), (R - v_c).pow(2)
    clipped = dd.abs() > vclip
    tie = clipped & ((e1 - e2).abs() < pc.MARGIN * torch.maximum(torch.maximum(e1, e2), torch.ones_like(e1)))
    # rows that miss a margin are moved to v_old = v; then the conditions are asserted
    bad = near | tie
    if hold is not None:
        bad[hold] = False
    v_old = torch.where(bad, d['v'], v_old)
    dd = v - v_old.double()
    near = (dd.abs() - vclip).abs() < pc.MARGIN
    v_c = v_old.double() + torch.clamp(dd, -vclip, vclip)
    e1, e2 = (R - v).pow(2), (R - v_c).pow(2)
    clipped = dd.abs() > vclip
    tie = clipped & ((e1 - e2).abs() < pc.MARGIN * torch.maximum(torch.maximum(e1, e2), torch.ones_like(e1)))
    if hold is not None:
        assert float(dd[hold].abs()) == vclip
        near[hold] = False
        tie[hold] = False
    assert not bool(near.any()), 'a row lies within the margin of the value clip boundary'
    assert not bool(tie.any()), 'a clipped row has e1 ~ e2'
    if rows >= 5:
        assert bool((dd[:, ::5] == 0).all())
    if rows >= 256 and not boundary:
        assert bool((~clipped & (dd != 0)).any(dim=1).all()), 'no inside row on some agent'
        assert bool((clipped & (e2 > e1)).any(dim=1).all()), 'no clipped row with e2 > e1 on some agent'
        assert bool((clipped & (e1 > e2)).any(dim=1).all()), 'no clipped row with e1 > e2 on some agent'
    d['v_old'], d['vclip'] = v_old, vclip
    return d


def expect(d, dtype=F64, wrong=None, loss=None, vclip=None):
    """The restatement (or `loss`, called like ops.ppo_loss with v_old / vclip) on the generator's data in `dtype` on the CPU:
    -> dict(total, terms [N,6], dlogits [N,rows,A+1] (padding column: zero), dv) for the upstream factors d['w']."""
    A = d['A']
    vclip = d['vclip'] if vclip is None else vclip
    o = d['out'].to(dtype).requires_grad_()
    vv = d['v'].to(dtype).requires_grad_()
    args = (o[..., :A], vv, d['action'], d['adv'].to(dtype), d['R'].to(dtype), d['logp_old'].to(dtype), d['clip'], pc.V_COEF, pc.E_COEF)
    if loss is None:
        tot, terms = restate(*args, d['v_old'].to(dtype), vclip, wrong=wrong)
    else:
        tot, terms = loss(*args, v_old=d['v_old'].to(dtype), vclip=vclip)
    (tot * d['w'].to(dtype)).sum().backward()
    return dict(total=tot.detach(), terms=terms.detach(), dlogits=o.grad, dv=vv.grad)


differs = pc.differs


def restate_f32(logits, v, action, adv, R, logp_old, clip, v_coef, e_coef, v_old=None, vclip=None):
    """Stand-in for ops.ppo_loss with its optional value clipping (the torch chain on whatever device the tensors live on)."""
    if v_old is None:
        return pc.restate(logits, v, action, adv, R, logp_old, clip, v_coef, e_coef)
    return restate(logits, v, action, adv, R, logp_old, clip, v_coef, e_coef, v_old, vclip)


# ------------------------------------------------------------------------------------------------ the KL stop, restated on the host
def kl_sum(terms, tail):
    """ops.ppo_kl_sum: fp32, agents in index order."""
    s = np.float32(0.0)
    for x in terms[:, 3].detach().cpu().numpy().astype(np.float32):
        s = np.float32(s + x)
    tail.fill_(float(s))


def kl_gate(tail, count, kappa, gate):
    """ops.ppo_kl_gate: fp32 division, strict comparison with the fp32 target, sticky stop, epochs counted while it is down."""
    kl = np.float32(float(tail.reshape(-1)[0])) / np.float32(count)
    if not kl <= np.float32(kappa):
        gate[0] = 1
    if int(gate[0]) == 0:
        gate[2] += 1


def gate_sequence(kls, kappa, count=1):
    """(stop, epochs_done) after epochs 2.. with the given per-epoch KL SUMS (tail values): the definition, in plain Python."""
    stop, done = 0, 1
    for s in kls:
        kl = np.float32(s) / np.float32(count)
        if not kl <= np.float32(kappa):
            stop = 1
        if not stop:
            done += 1
    return stop, done

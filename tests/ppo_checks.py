"""Shared by the tests of the opt-in PPO epochs (MODEL_CONFIG ppo_epochs > 1): the float64 torch restatement of the behaviour
log-probability, the five terms of the clipped surrogate loss and -- through autograd -- its gradients; an input generator whose data
exercise both clip sides, both advantage signs, probabilities below the 1e-10 clamp, rho = 1 and Adv = 0; and the wrong variants the
checks must tell from the definition.

Definition, per agent n over rows = T*E:
    pi = softmax(logits);  lp = log(clip(pi, 1e-10, 1));  rho = exp(lp[a] - logp_old)
    policy = -mean(min(rho Adv, clip(rho, 1 - eps, 1 + eps) Adv));  value = 0.5 v_coef mean((R - v)^2);  entropy = -e_coef mean(H)
    approx_kl = mean((rho - 1) - (lp[a] - logp_old));  clip_frac = mean(|rho - 1| > eps);  total = policy + value + entropy
"""
import torch

F32, F64 = torch.float32, torch.float64

# tolerances of tests/test_gpu_ops.py::test_a2c_loss_fused, which the project already holds this arithmetic to
TERMS_TOL = dict(rtol=2e-5, atol=1e-6)
GRAD_TOL = dict(rtol=1e-4, atol=1e-9)
LOGP_TOL = dict(rtol=1e-5, atol=1e-6)
MARGIN = 1e-3            # no row's rho lies this close to 1 - eps or 1 + eps: a condition on the inputs, not a tolerance
V_COEF, E_COEF, CLIP = 0.5, 0.05, 0.2
SENTINEL = -12345.0

SHAPES = [(8, 4096, 4), (25, 1234, 5), (3, 1, 8), (1, 257, 2), (8, 70001, 4)]
# beside SHAPES, the smallest inputs at which the loss kernels' shared row, block-reduction and launcher code can go wrong: the widest
# action set over two chunks (rows * N > 4096) with a ragged last chunk and rows no multiple of 256; one row with one action (every
# padded lane of the row inactive).  LOSS_CASES: every shape with the logits contiguous (block False) and as a column block of pitch
# A + 1 (True), and the first edge shape once more at pitch A + 3 ('wide'), the strided form the heads hand over
EDGE_SHAPES = [(3, 1501, 8), (1, 1, 1)]
LOSS_CASES = [s + (block,) for s in SHAPES + EDGE_SHAPES for block in (False, True)] + [EDGE_SHAPES[0] + ('wide',)]


def column_block(out, A, block, fill=0.0):
    """out [N,rows,A+1] -> the tensor whose first A columns are handed over as logits: those columns alone, contiguous (block False),
    `out` itself (True: pitch A + 1) or `out` with two more padding columns of `fill` ('wide': pitch A + 3)."""
    if block == 'wide':
        return torch.nn.functional.pad(out, (0, 2), value=fill)
    return out if block else out[..., :A].contiguous()


def logp(logits, action):
    """log(clip(softmax(logits)[a], 1e-10, 1)) [N,rows] of the actions action [rows,N] u8, in the dtype of logits."""
    pi = torch.softmax(logits, dim=-1)
    lp = torch.log(torch.clamp(pi, 1e-10, 1.0))
    return lp.gather(-1, action.t().long().unsqueeze(-1)).squeeze(-1)


def restate(logits, v, action, adv, R, logp_old, clip, v_coef, e_coef, wrong=None):
    """-> (total [N] differentiable, terms [N,5] detached) in the dtype of logits.  wrong: the name of one mistake (WRONG)."""
    pi = torch.softmax(logits, dim=-1)
    lp = torch.log(torch.clamp(pi, 1e-10, 1.0))
    acts = action.t().long().unsqueeze(-1)
    lp_a = lp.gather(-1, acts).squeeze(-1)
    if wrong == 'ratio from unclamped probabilities':
        lp_a = torch.log(pi).gather(-1, acts).squeeze(-1)
    if wrong == 'logp_old taken from the new weights':
        logp_old = lp_a.detach()
    dlp = lp_a - logp_old
    rho = torch.exp(dlp)
    s1, s2 = rho * adv, torch.clamp(rho, 1.0 - clip, 1.0 + clip) * adv
    surr = torch.min(s1, s2)
    if wrong == 'max instead of min':
        surr = torch.max(s1, s2)
    if wrong == 'clip without the advantage sign':
        surr = s2
    if wrong == 'gradient through the clipped branch':
        surr = s1 + (surr - s1).detach()
    policy = -surr.mean(-1)
    if wrong == 'mean over N * rows':
        policy = -surr.sum(-1) / surr.numel()
    sq = (R - v).pow(2)
    if wrong == 'value term scaled by rho':
        sq = sq * rho.detach()
    value = sq.mean(-1) * 0.5 * v_coef
    H = -(pi * lp).sum(-1)
    if wrong == 'entropy gradient dropped':
        H = H.detach()
    entropy = -H.mean(-1) * e_coef
    kl = ((rho - 1.0) - dlp).mean(-1)
    if wrong == 'kl with the sign flipped':
        kl = -kl
    if wrong == 'kl as logp_old - lp':
        kl = (-dlp).mean(-1)
    cf = ((rho - 1.0).abs() > clip).to(logits.dtype).mean(-1)
    if wrong == 'clip_frac with >=':
        cf = ((rho - 1.0).abs() >= clip).to(logits.dtype).mean(-1)
    if wrong == 'clip_frac one-sided':
        cf = ((rho - 1.0) > clip).to(logits.dtype).mean(-1)
    if wrong == 'clamp of 1e-8':
        lp8 = torch.log(torch.clamp(pi, 1e-8, 1.0))
        return restate_from(lp8, pi, acts, v, adv, R, logp_old, clip, v_coef, e_coef)
    total = policy + value + entropy
    return total, torch.stack([policy, value, entropy, kl, cf], dim=1).detach()


def restate_from(lp, pi, acts, v, adv, R, logp_old, clip, v_coef, e_coef):
    """The definition from given clamped log-probabilities (the 'clamp of 1e-8' variant)."""
    dlp = lp.gather(-1, acts).squeeze(-1) - logp_old
    rho = torch.exp(dlp)
    policy = -torch.min(rho * adv, torch.clamp(rho, 1.0 - clip, 1.0 + clip) * adv).mean(-1)
    value = (R - v).pow(2).mean(-1) * 0.5 * v_coef
    entropy = (pi * lp).sum(-1).mean(-1) * e_coef
    kl = ((rho - 1.0) - dlp).mean(-1)
    cf = ((rho - 1.0).abs() > clip).to(lp.dtype).mean(-1)
    return policy + value + entropy, torch.stack([policy, value, entropy, kl, cf], dim=1).detach()


# every mistake the checks must see; 'clip_frac with >=' can differ from the definition only ON the boundary, which `inputs` keeps
# every row away from: it is told apart on `inputs(..., boundary=True)`, whose eps is row 0's own rho - 1
WRONG = ['max instead of min', 'clip without the advantage sign', 'gradient through the clipped branch',
         'ratio from unclamped probabilities', 'logp_old taken from the new weights', 'kl with the sign flipped', 'kl as logp_old - lp',
         'clip_frac with >=', 'clip_frac one-sided', 'entropy gradient dropped', 'value term scaled by rho', 'mean over N * rows',
         'clamp of 1e-8']


def inputs(N, rows, A, clip=CLIP, seed=0, boundary=False):
    """dict of CPU tensors: out [N,rows,A+1] f32 (logits = out[..., :A]: a column block of pitch A + 1; the last column is padding),
    action [rows,N] u8, v / adv / R / logp_old [N,rows] f32, w [N] upstream factors, clip.  Every 7th row has logit 0 = -60 and action
    0 (probability below the clamp); logp_old is the log-probability at perturbed logits (both clip sides, both advantage signs),
    on every 5th + 1 row lp_a itself (rho = 1 up to fp32 rounding); every 11th + 3 row has Adv = 0.  Asserted in float64: no row has
    |rho - (1 +- clip)| < MARGIN, so clip_frac and the gradient gate cannot differ between fp32 and float64 by a boundary flip.
    boundary: clip becomes row (0, 1)'s own rho - 1 instead (float64 equality on that row; the margin holds for every other row)."""
    g = torch.Generator().manual_seed(1000 * N + rows + A + seed)
    out = torch.randn(N, rows, A + 1, generator=g) * 2.0
    out[:, ::7, 0] = -60.0
    action = torch.randint(0, A, (rows, N), generator=g).to(torch.uint8)
    action[::7] = 0
    v, adv, R = (torch.randn(N, rows, generator=g) for _ in range(3))
    adv[:, 3::11] = 0.0
    w = torch.rand(N, generator=g) + 0.5
    noise = torch.randn(N, rows, A, generator=g) * 0.6
    l64 = out[..., :A].double()
    lp_a = logp(l64, action)
    logp_old = logp(l64 + noise.double(), action)
    logp_old[:, 1::5] = lp_a[:, 1::5]
    logp_old = logp_old.float()
    hold = None
    if boundary:
        assert rows > 2
        rho01 = torch.exp(lp_a[0, 2] - logp_old[0, 2].double())
        assert abs(float(rho01) - 1.0) > 0.01, 'boundary row has rho ~ 1'
        clip, hold = abs(float(rho01) - 1.0), (0, 2)
    # rows that fall within the margin are moved to rho = 1; then the condition is asserted
    rho = torch.exp(lp_a - logp_old.double())
    near = ((rho - (1.0 - clip)).abs() < 2 * MARGIN) | ((rho - (1.0 + clip)).abs() < 2 * MARGIN)
    if hold is not None:
        near[hold] = False
    logp_old = torch.where(near, lp_a.float(), logp_old)
    rho = torch.exp(lp_a - logp_old.double())
    near = ((rho - (1.0 - clip)).abs() < MARGIN) | ((rho - (1.0 + clip)).abs() < MARGIN)
    if hold is not None:
        assert float((rho[hold] - 1.0).abs()) == clip
        near[hold] = False
    assert not bool(near.any()), 'a row lies within the margin of the clip boundary'
    if rows >= 256 and not boundary:          # both clip sides and both advantage signs occur, on every agent
        for sgn in (1.0, -1.0):
            assert bool(((rho > 1.0 + clip) & (adv * sgn > 0)).any(dim=1).all())
            assert bool(((rho < 1.0 - clip) & (adv * sgn > 0)).any(dim=1).all())
    return dict(out=out, action=action, v=v, adv=adv, R=R, logp_old=logp_old, w=w, clip=clip, A=A)


def expect(d, dtype=F64, wrong=None, loss=None):
    """The restatement (or `loss`, called like ops.ppo_loss) on the generator's data in `dtype` on the CPU:
    -> dict(total, terms, dlogits [N,rows,A+1] (padding column: zero), dv) for the upstream factors d['w']."""
    A = d['A']
    o = d['out'].to(dtype).requires_grad_()
    vv = d['v'].to(dtype).requires_grad_()
    args = (o[..., :A], vv, d['action'], d['adv'].to(dtype), d['R'].to(dtype), d['logp_old'].to(dtype), d['clip'], V_COEF, E_COEF)
    tot, terms = restate(*args, wrong=wrong) if loss is None else loss(*args)
    (tot * d['w'].to(dtype)).sum().backward()
    return dict(total=tot.detach(), terms=terms.detach(), dlogits=o.grad, dv=vv.grad)


def differs(a, b):
    """Some term or gradient of two `expect` results lies outside the tolerances the device is held to."""
    for k, tol in (('terms', TERMS_TOL), ('dlogits', GRAD_TOL), ('dv', GRAD_TOL)):
        if not torch.allclose(a[k].double(), b[k].double(), **tol):
            return True
    return False


def restate_f32(logits, v, action, adv, R, logp_old, clip, v_coef, e_coef):
    """The restatement as a stand-in for ops.ppo_loss (fp32 torch chain on whatever device the tensors live on)."""
    return restate(logits, v, action, adv, R, logp_old, clip, v_coef, e_coef)

"""Checks of the opt-in clip + Adam optimiser step (csrc/a2c.hip: adam_sumsq_kernel, adam_kernel; nmarl_adam_clip[_guarded]), written
as functions of the implementation under test like update_edge_checks.check_rmsprop: `ops` on the GPU (tests/test_gpu_adam.py), the
fp32 restatement below or a deliberately wrong variant of it on the CPU (tests/test_adam_cpu.py, which proves the check sharp).

The definition (include/nmarl.h), per group, with t = step + 1:
    norm = ||g_grp|| |grad_scale|
    gc   = g grad_scale (max_norm min(1 / norm, 1 / max_norm))          (max_norm > 0; else gc = g grad_scale)
    m    = beta1 m + (1 - beta1) gc           v = beta2 v + (1 - beta2) gc^2
    w   -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)  (Kingma & Ba; eps outside the root)
    step = t
`adam_expect` restates it in float64, `Fp32Adam` in straight fp32 NumPy.  The C-ABI carries lr / betas / eps / max_norm / grad_scale
as `float`: they are rounded to fp32 before the float64 expectation uses them."""
import numpy as np
import torch

from update_edge_checks import RMSPROP_STEP_RTOL, _bits, _f32, _same_bits      # noqa: F401  (re-exported for the tests)

F32, F64 = torch.float32, torch.float64

ADAM_SHAPES = [(3, 77, -1.0, 1.0),               # no clip
               (8, 1000, 0.5, 0.125),            # clipped
               (2, 300, 40.0, 1.0),              # not clipped
               (1, 2 * 262144 + 5, 40.0, 0.5),   # above the 1024-block grid stride
               (5, 3, 0.5, 1.0),                 # odd P: unaligned group bases, a tail shorter than a vector
               (4, 1023, 40.0, 1.0),             # odd P
               (1, 1, -1.0, 1.0)]                # a single parameter
ADAM_T0 = [0, 999, 10_000_000]                   # the first step (m_hat = gc); mid-run; beta^t underflowed to 0
ADAM_BETAS = [(0.9, 0.999), (0.0, 0.999), (0.9, 0.0)]
ADAM_EPS = 1e-8
ADAM_RTOL = RMSPROP_STEP_RTOL      # the project's constant for "about a dozen fp32 roundings plus the fixed-order norm sum": here the
#                                    clip scale (norm, two reciprocals, three products), m and v (three each), root, correction,
#                                    eps, division, step size, subtraction


def adam_expect(w, g, m, v, t_prev, lr, beta1, beta2, eps, max_norm, grad_scale):
    """One step of the definition in float64 on [G,P] tensors -> dict(w, m, v, norm [G], gc, denom, bc1).  t_prev: steps applied so far."""
    w, g, m, v = (x.double() for x in (w, g, m, v))
    t = float(t_prev + 1)
    norm = g.pow(2).sum(dim=1, keepdim=True).sqrt() * abs(grad_scale)
    scale = torch.full_like(norm, grad_scale)
    if max_norm > 0:
        scale = grad_scale * (max_norm * torch.minimum(1.0 / norm, torch.full_like(norm, 1.0 / max_norm)))
    gc = g * scale
    m_new = beta1 * m + (1.0 - beta1) * gc
    v_new = beta2 * v + (1.0 - beta2) * gc * gc
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    denom = v_new.sqrt() / bc2 ** 0.5 + eps
    return dict(w=w - (lr / bc1) * m_new / denom, m=m_new, v=v_new, norm=norm.view(-1), gc=gc, denom=denom, bc1=bc1)


class Fp32Adam:
    """The definition in straight fp32 NumPy with the signature of ops.adam_clip (in place on CPU tensors); the bias corrections in
    float64, rounded once, as the kernel forms them.  The keyword switches turn on ONE mistake each (tests/test_adam_cpu.py)."""

    def __init__(self, eps_inside=False, no_correction=False, t_minus_one=False, unclipped_moments=False, swap_betas=False,
                 slots_from_one=False):
        self.eps_inside, self.no_correction, self.t_minus_one = eps_inside, no_correction, t_minus_one
        self.unclipped_moments, self.swap_betas, self.slots_from_one = unclipped_moments, swap_betas, slots_from_one

    def adam_clip(self, w, g, m, v, scratch, step, lr, beta1, beta2, eps, max_norm, grad_scale=1.0, norm_out=None, lr_dev=None,
                  guard=False):
        f = np.float32
        if lr_dev is not None:
            lr = float(lr_dev[0])
        lr, beta1, beta2, eps, mn, gs = f(lr), f(beta1), f(beta2), f(eps), f(max_norm), f(grad_scale)
        if self.swap_betas:
            beta1, beta2 = beta2, beta1
        t_prev = int(step[0])
        t = t_prev if self.t_minus_one else t_prev + 1
        wn, gn, m1, m2 = (x.numpy() for x in (w, g, m, v))                  # views: written in place
        if self.slots_from_one and t_prev == 0:
            m1[...] = 1.0
            m2[...] = 1.0
        with np.errstate(divide='ignore', invalid='ignore'):
            norm = np.sqrt((gn * gn).sum(axis=1, keepdims=True, dtype=f)) * abs(gs)
            scale = np.full_like(norm, gs)
            if mn > 0:
                scale = gs * (mn * np.minimum(f(1.0) / norm, f(1.0) / mn))
            gc = gn * scale
            gm = gn * gs if self.unclipped_moments else gc
            m1[...] = beta1 * m1 + (f(1.0) - beta1) * gm
            m2[...] = beta2 * m2 + (f(1.0) - beta2) * (gm * gm)
            bc1 = 1.0 if self.no_correction else 1.0 - float(beta1) ** t
            bc2 = 1.0 if self.no_correction else 1.0 - float(beta2) ** t
            step_size = f(float(lr) / bc1) if bc1 != 0 else f(np.inf)
            rs_bc2 = f(1.0 / bc2 ** 0.5) if bc2 != 0 else f(np.inf)
            denom = np.sqrt(m2 * rs_bc2 * rs_bc2 + eps) if self.eps_inside else np.sqrt(m2) * rs_bc2 + eps
            wn[...] = wn - step_size * m1 / denom
        step[0] = t_prev + 1
        if norm_out is not None:
            norm_out.copy_(torch.from_numpy(norm.reshape(-1)))


def adam_inputs(G, P, t0, eps):
    """-> w, m, v, g0 [G,P] fp32.  The groups' norms differ by x3; the last group's gradient (and, with it, its slots) is all zero
    when G > 1; every eighth weight starts at 0; every fifth gradient (from element 1) has |g| in eps x [0.5, 5], i.e. within a decade
    of eps, where eps inside or outside the root or a missing correction moves the step by percents.  t0 > 0: m = +-g0 x [0.5, 1.5]
    with the sign opposed to g on the odd elements (cancellation in beta1 m + (1 - beta1) gc), v = g0^2 x [0.5, 1.5].  t0 = 0: both
    slots are 0 -- the only state a run has before its first step (m_hat = gc there)."""
    gen = torch.Generator().manual_seed(G * 1009 + P)
    w = torch.randn(G, P, generator=gen)
    w[:, ::8] = 0.0
    g0 = torch.randn(G, P, generator=gen) * 0.05 * (3.0 ** (torch.arange(G) % 3).float()).view(G, 1)
    tiny = torch.sign(g0[:, 1::5]) * eps * (0.5 + 4.5 * torch.rand(g0[:, 1::5].shape, generator=gen))
    g0[:, 1::5] = tiny
    if G > 1:
        g0[G - 1] = 0.0
    um, uv = 0.5 + torch.rand(G, P, generator=gen), 0.5 + torch.rand(G, P, generator=gen)
    sign = torch.ones(P)
    sign[1::2] = -1.0
    m = g0 * um * sign
    m[g0 == 0] = 0.0                               # (not -0.0: the all-zero group's slots must be able to keep their bits)
    v = g0 * g0 * uv
    if t0 == 0:
        m, v = torch.zeros(G, P), torch.zeros(G, P)
    return w, m, v, g0


FP32_SUBNORMAL = 2.0 ** -148      # three roundings of a subnormal fp32 result, each off by at most half the spacing 2^-149


def assert_adam_step(prev, g, t_prev, got, lr, beta1, beta2, eps, max_norm, grad_scale, what='', underflow=0.0):
    """prev = (w, m, v) before a step [G,P], got = (w, m, v, norm_out) after it, g the gradient it saw, t_prev the step count before:
    the float64 expectation from `prev` and, with r = 4e-6, per element
        |m - m64| <= r (beta1 |m_prev| + (1 - beta1) |gc|)            |v - v64| <= r v64            norm_out to rtol r
        |w - w64| <= 2^-23 |w64| + r (lr / bc1) (beta1 |m_prev| + (1 - beta1) |gc|) / denom64
    (the terms of m by magnitude: cancellation between them is not allowed to hide behind |m|).  underflow: an absolute term added to
    the bounds of m and v -- 0 for check_adam, whose inputs stay in fp32's normal range; FP32_SUBNORMAL for a network's own gradient,
    whose smallest entries square to less than fp32 can hold (gc ~ 1e-23 -> gc^2 < 2^-149: the slot is 0 and no relative bound can
    hold; the step is not affected, eps dwarfs the root).  -> the share of each bound used (printed), and the float64 size of the
    step's bound term dw."""
    r = ADAM_RTOL
    w_prev, m_prev, v_prev = (x.detach().cpu() for x in prev)
    w_got, m_got, v_got, n_got = (x.detach().cpu().double() for x in got)
    e = adam_expect(w_prev, g.detach().cpu(), m_prev, v_prev, t_prev, lr, beta1, beta2, eps, max_norm, grad_scale)
    terms = beta1 * m_prev.double().abs() + (1.0 - beta1) * e['gc'].abs()
    dw = (lr / e['bc1']) * terms / e['denom']
    bounds = dict(w=2.0 ** -23 * e['w'].abs() + r * dw, m=r * terms + underflow, v=r * e['v'] + underflow, norm=r * e['norm'])
    errs = dict(w=(w_got - e['w']).abs(), m=(m_got - e['m']).abs(), v=(v_got - e['v']).abs(), norm=(n_got.view(-1) - e['norm']).abs())
    used = {}
    for k in ('w', 'm', 'v', 'norm'):
        err, bound = errs[k], bounds[k]
        ok = err <= bound                                    # (nan fails; 0 <= 0 passes: an all-zero group)
        share = torch.where(bound > 0, err / bound.clamp_min(1e-300),
                            torch.where(ok, torch.zeros_like(err), torch.full_like(err, float('inf'))))
        used[k] = float(share.max()) if bool((share == share).all()) else float('nan')
    print('adam %s: share of the bound used w %.3g, m %.3g, v %.3g, norm %.3g' % (what, used['w'], used['m'], used['v'], used['norm']))
    for k in ('norm', 'm', 'v', 'w'):
        assert bool((errs[k] <= bounds[k]).all()), '%s: %.3g of the bound (%s)' % (k, used[k], what)
    return used, dw


def check_adam(impl, dev, G, P, max_norm, grad_scale, use_lr_dev, t0, beta1=0.9, beta2=0.999, eps=ADAM_EPS):
    """Three consecutive steps from step count t0 with gradients growing x1, x2, x3 (inputs: `adam_inputs`), each held to the bounds
    of `assert_adam_step`: the float64 expectation restarts from the implementation's own fp32 state before each step (errors do not
    compound).  use_lr_dev: the host lr is wrong on purpose (1.0), the right one arrives in a device scalar that is rewritten before
    the third step.  After call k the counter is t0 + k; an all-zero group keeps the bits of w, m and v.  Returns the worst share of
    each bound used."""
    lr, b1, b2, ep = _f32(5e-4), _f32(beta1), _f32(beta2), _f32(eps)
    mn, gs = _f32(max_norm), _f32(grad_scale)
    w, m, v, g0 = adam_inputs(G, P, t0, ep)
    wd, md, vd = w.to(dev), m.to(dev), v.to(dev)
    step = torch.full((1,), t0, dtype=torch.int32, device=dev)
    scratch, norm_out = torch.zeros(G, 64, device=dev), torch.full((G,), -7.0, device=dev)
    lr_steps = [lr, lr, _f32(2.5e-4)] if use_lr_dev else [lr] * 3
    lr_dev = torch.zeros(1, device=dev) if use_lr_dev else None
    worst = dict(w=0.0, m=0.0, v=0.0, norm=0.0)
    any_small = False
    for it in range(3):
        g = g0 * float(it + 1)
        prev = tuple(x.cpu().clone() for x in (wd, md, vd))
        if use_lr_dev:
            lr_dev.fill_(lr_steps[it])
        impl.adam_clip(wd, g.to(dev), md, vd, scratch, step, 1.0 if use_lr_dev else lr, b1, b2, ep, mn, gs, norm_out, lr_dev=lr_dev)
        assert int(step.cpu()[0]) == t0 + it + 1, 'step counter %d after call %d from %d' % (int(step.cpu()[0]), it + 1, t0)
        what = 'G=%d P=%d max_norm=%g scale=%g lr_dev=%d t0=%d betas=(%g, %g) step %d' % (G, P, mn, gs, use_lr_dev, t0, b1, b2, it)
        used, dw = assert_adam_step(prev, g, t0 + it, (wd, md, vd, norm_out), lr_steps[it], b1, b2, ep, mn, gs, what)
        for k, x in used.items():
            worst[k] = max(worst[k], x) if x == x else float('nan')
        if G > 1:                                                # zero gradient, zero slots: nothing moves, bit for bit
            for name, got, before in zip('wmv', (wd, md, vd), prev):
                assert _same_bits(got[G - 1], before[G - 1]), 'the all-zero group changed %s (step %d)' % (name, it)
        any_small = any_small or bool(((prev[0].double().abs() <= 4 * dw) & (dw != 0)).any())
    assert any_small                             # some weight started at 0 in a group that moves: the step's error is not hidden
    return worst


def check_adam_guard(dev):
    """nmarl_adam_clip_guarded with a private status tensor (no global state): while word 0 is set the step changes neither w, m, v
    nor the counter and counts itself in word 1; with word 0 cleared it is the unguarded step bit for bit.  The word is set from the
    host: nothing faults."""
    from deeprl_network_amd import _lib
    lib, ptr = _lib.lib, _lib.ptr
    G, P, t0 = 3, 1000, 7
    w0, m0, v0, g = (x.to(dev) for x in adam_inputs(G, P, t0, _f32(ADAM_EPS)))
    s0 = torch.full((1,), t0, dtype=torch.int32, device=dev)
    scratch, norm = torch.zeros(G, 64, device=dev), torch.zeros(G, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    args = (None, _f32(5e-4), _f32(0.9), _f32(0.999), _f32(ADAM_EPS), _f32(0.5), _f32(0.5))

    def guarded(w, m, v, s):
        _lib.check(lib.nmarl_adam_clip_guarded(G, P, ptr(w, F32), ptr(g, F32), ptr(m, F32), ptr(v, F32), ptr(scratch, F32),
                                               ptr(s, torch.int32), *args, ptr(norm, F32), ptr(status, torch.int32), _lib.stream()),
                   'guarded')

    w, m, v, s = w0.clone(), m0.clone(), v0.clone(), s0.clone()
    status[0] = 1
    for n in (1, 2):
        guarded(w, m, v, s)
        assert status.tolist() == [1, n, 0, 0], status.tolist()
        assert _same_bits(w, w0) and _same_bits(m, m0) and _same_bits(v, v0) and _same_bits(s, s0)
    status[0] = 0
    guarded(w, m, v, s)
    assert status.tolist() == [0, 2, 0, 0], status.tolist()
    w2, m2, v2, s2 = w0.clone(), m0.clone(), v0.clone(), s0.clone()
    _lib.check(lib.nmarl_adam_clip(G, P, ptr(w2, F32), ptr(g, F32), ptr(m2, F32), ptr(v2, F32), ptr(scratch, F32), ptr(s2, torch.int32),
                                   *args, ptr(norm, F32), _lib.stream()), 'unguarded')
    assert _same_bits(w, w2) and _same_bits(m, m2) and _same_bits(v, v2) and _same_bits(s, s2)
    assert not _same_bits(w, w0) and not _same_bits(m, m0) and not _same_bits(v, v0) and s.tolist() == [t0 + 1]

"""Checks of the opt-in running return-based reward scaling (csrc/a2c.hip: reward_scale_scan_kernel / _merge_kernel / _apply_kernel),
written as functions of the implementation under test: `ops` on the GPU (tests/test_gpu_reward_scale.py), the float64 NumPy
restatement below or a deliberately wrong variant of it on the CPU (tests/test_reward_scale_cpu.py, which checks the restatement
against exact rational arithmetic and proves that the check is sharp).  Definition, everything in float64:

    for t = 0..T-1, every stream s (e = its replica):  carry[s] = gamma carry[s] + r_raw[t, s];  sample x = carry[s];
                                                       if done_post[t, e]: carry[s] = 0              (after the sample)
    (n, mean, M2) <- the population moments of every sample seen so far, this call's T S included
    sigma = sqrt(M2 / n);  scale = 1 / (sigma + eps) if sigma > 0 else 1;  r_out = fp32(double(r_raw) scale), then clamped to +-clip

Streams: s = e for the global reward [T,E] (N = 0), s = e N + i for per-agent rewards [T,E,N].

Acceptance.  carry, mean and sigma: 1e-12 relative (MOMENT_RTOL, the project's moment bound of tests/adv_norm_checks.py; absolute where
the expectation is 0); n exact.  r_out per element: |got - exp| <= 2^-23 |exp| + 1e-12 |exp| + 2^-149 -- one fp32 ulp of the single
rounding, the moment bound propagated (scale = 1 / (sigma + eps) moves by at most sigma's relative error), the smallest subnormal.
An element whose expectation lies beyond +-clip by more than that bound must be the fp32 clip exactly; inside by more than it, it is
held to the bound; in between either is accepted.  The restatement keeps every sample and takes its moments with math.fsum, so
it sits at a few 1e-16 (checked against fractions.Fraction to a tenth of the bound)."""
import math

import numpy as np

MOMENT_RTOL = 1e-12
EPS = 1e-8
GAMMA = 0.99
SENTINEL = -777.0
KINDS = ('plain', 'offset', 'tiny', 'zero', 'const')
DONES = ('none', 'last', 'first', 'random')
VARIANTS = ('carry_not_kept', 'reset_before_sample', 'no_reset', 'batch_moments_only', 'merged_after_scaling', 'sample_variance',
            'eps_inside_root', 'mean_subtracted', 'reward_norm_too', 'clip_before_scale', 'per_agent_moments', 'sigma_zero_unmapped')


def rewards(T, S, kind, call, seed=0):
    """[T, S] fp32 raw rewards of call number `call`:
      plain   N(0,1)
      offset  3e4 + 1e-2 N(0,1): the returns sit far from zero against the spread of the rewards
      tiny    1e-20 N(0,1): eps dominates the scale
      zero    all zero: sigma = 0, scale 1
      const   one non-zero value: the returns still spread (they grow from 0)"""
    rng = np.random.RandomState(1000003 * seed + 7919 * call + 31 * T + S + KINDS.index(kind))
    z = rng.standard_normal((T, S))
    if kind == 'plain':
        x = z
    elif kind == 'offset':
        x = 3e4 + 1e-2 * z
    elif kind == 'tiny':
        x = 1e-20 * z
    elif kind == 'zero':
        x = np.zeros((T, S))
    elif kind == 'const':
        x = np.full((T, S), -2.5)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def dones(T, E, pattern, call, seed=0):
    """[T, E] uint8 done_post flags: none; every replica at the last step; every replica at t = 0; random (one in four)."""
    d = np.zeros((T, E), dtype=np.uint8)
    if pattern == 'last':
        d[T - 1] = 1
    elif pattern == 'first':
        d[0] = 1
    elif pattern == 'random':
        d[:] = np.random.RandomState(77 + 13 * call + T + E + seed).rand(T, E) < 0.25
    elif pattern != 'none':
        raise ValueError(pattern)
    return d


class Restatement:
    """The definition in float64 NumPy.  `variant`: None = the definition, or one of VARIANTS = that mistake.  `call` advances the
    state and returns dict(r_out float64 [T,S] NOT rounded to fp32 (clamped), carry [S], n, mean, sigma)."""

    def __init__(self, E, N, gamma=GAMMA, eps=EPS, clip=0.0, reward_norm=0.0, variant=None):
        assert variant is None or variant in VARIANTS
        self.E, self.N, self.S = E, N, E * max(N, 1)
        self.gamma, self.eps, self.clip, self.reward_norm, self.variant = float(gamma), float(eps), float(clip), reward_norm, variant
        self.carry = np.zeros(self.S, dtype=np.float64)
        self.samples = np.zeros((0, self.S), dtype=np.float64)          # every sample seen so far, [calls * T, S]

    @staticmethod
    def moments(x, ddof=0):
        """(n, mean, sigma) of the float64 array x: math.fsum twice (the sums exact before their one rounding); beyond 200 000
        samples, where that loop takes seconds, two passes of NumPy's pairwise sums in extended precision."""
        x = np.asarray(x, dtype=np.float64).ravel()
        n = x.size
        if n == 0:
            return 0, 0.0, 0.0
        if n > 200000:
            xl = x.astype(np.longdouble)
            mean = xl.sum() / n
            return n, float(mean), float(np.sqrt(((xl - mean) ** 2).sum() / max(n - ddof, 1)))
        flat = x.tolist()
        mean = math.fsum(flat) / n
        m2 = math.fsum((v - mean) * (v - mean) for v in flat)
        return n, mean, math.sqrt(m2 / max(n - ddof, 1))

    def call(self, r_raw, done_post):
        v = self.variant
        r64 = np.asarray(r_raw, dtype=np.float64).reshape(r_raw.shape[0], self.S)
        T = r64.shape[0]
        d = np.asarray(done_post).reshape(T, self.E).astype(bool)
        d = np.repeat(d, max(self.N, 1), axis=1)                          # [T, S]: stream s = e N + i reads done[t, e]
        if v == 'carry_not_kept':
            self.carry[:] = 0.0
        x = np.empty((T, self.S), dtype=np.float64)
        for t in range(T):
            self.carry = self.gamma * self.carry + r64[t]
            if v == 'reset_before_sample':
                self.carry = np.where(d[t], 0.0, self.carry)
            x[t] = self.carry
            if v != 'no_reset':
                self.carry = np.where(d[t], 0.0, self.carry)
        before = self.samples
        self.samples = np.concatenate([self.samples, x], axis=0)
        pool = x if v == 'batch_moments_only' else self.samples
        n, mean, sigma = self.moments(pool, ddof=1 if v == 'sample_variance' else 0)
        used = (n, mean, sigma)
        if v == 'merged_after_scaling':
            used = self.moments(before)

        def scale_of(sig):
            if v == 'eps_inside_root':
                return 1.0 / math.sqrt(sig * sig + self.eps) if sig > 0 else 1.0
            if v == 'sigma_zero_unmapped':
                return 1.0 / (sig + self.eps)
            return 1.0 / (sig + self.eps) if sig > 0 else 1.0

        src = r64
        if v == 'clip_before_scale' and self.clip > 0:
            src = np.clip(src, -self.clip, self.clip)
        if v == 'reward_norm_too' and self.reward_norm > 0:
            src = src / self.reward_norm
        if v == 'mean_subtracted':
            src = src - used[1]
        if v == 'per_agent_moments' and self.N > 1:
            out = np.empty_like(src)
            for i in range(self.N):
                out[:, i::self.N] = src[:, i::self.N] * scale_of(self.moments(pool[:, i::self.N])[2])
        else:
            out = src * scale_of(used[2])
        if self.clip > 0 and v != 'clip_before_scale':
            c = float(np.float32(self.clip))
            out = np.clip(out, -c, c)
        return dict(r_out=out, carry=self.carry.copy(), n=n, mean=mean, sigma=sigma)


def _close(got, exp, rtol=MOMENT_RTOL):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    return np.abs(got - exp) <= rtol * np.where(exp != 0, np.abs(exp), 1.0)


def out_bound(exp):
    """The acceptance bound of r_out per element (module docstring)."""
    return (2.0 ** -23 + MOMENT_RTOL) * np.abs(exp) + 2.0 ** -149


def assert_call(got, r_raw, exp, eps, clip, what=''):
    """One call's results `got` = dict(r_out fp32-valued [T,S], carry [S], n, mean, sigma) of an implementation against the
    restatement's `exp` for the same call.  Returns the worst fraction of the bounds used."""
    S = exp['carry'].shape[0]
    T = np.asarray(r_raw).shape[0]
    assert int(got['n']) == int(exp['n']), '%s: n = %r, expected %r' % (what, got['n'], exp['n'])
    worst = 0.0
    for name in ('mean', 'sigma', 'carry'):
        g, e = np.asarray(got[name], dtype=np.float64), np.asarray(exp[name], dtype=np.float64)
        rel = np.abs(g - e) / np.where(e != 0, np.abs(e), 1.0)
        print('reward_scale %s: %s off by %.3g relative' % (what, name, rel.max()))
        assert bool(_close(g, e).all()), '%s: %s %r against %r' % (what, name, g, e)
        worst = max(worst, float(rel.max()) / MOMENT_RTOL)
    sigma = float(exp['sigma'])
    scale = 1.0 / (sigma + eps) if sigma > 0 else 1.0
    raw = np.asarray(r_raw, dtype=np.float64).reshape(T, S) * scale                # before the clamp
    g = np.asarray(got['r_out'], dtype=np.float64).reshape(T, S)
    b = out_bound(raw)
    err = np.abs(g - raw)
    if clip > 0:
        c = float(np.float32(clip))
        beyond, inside = np.abs(raw) > c + b, np.abs(raw) < c - b
        assert bool((g[beyond] == np.sign(raw[beyond]) * c).all()), '%s: clamped outputs must be the clip exactly' % what
        edge = ~beyond & ~inside
        assert bool(((err[edge] <= b[edge]) | (np.abs(g[edge]) == c)).all()), '%s: outputs at the clip' % what
        err, b = err[inside], b[inside]
    frac = float((err / b).max()) if err.size else 0.0
    print('reward_scale %s: r_out uses %.3g of the bound' % (what, frac))
    assert bool((err <= b).all()), '%s: r_out uses %.3g of the bound' % (what, frac)
    return max(worst, frac)


def run_case(make_impl, E, N, T, kind, pattern, clip=0.0, eps=EPS, gamma=GAMMA, calls=3, seed=0, reward_norm=0.0):
    """`calls` successive calls of make_impl(E, N, gamma, eps, clip).call(r_raw [T,S] fp32, done [T,E] u8) -> dict like
    Restatement.call's (r_out rounded to fp32) against the restatement, compared after every call."""
    S = E * max(N, 1)
    ref = Restatement(E, N, gamma, eps, clip, reward_norm=reward_norm)
    impl = make_impl(E, N, gamma, eps, clip)
    worst = 0.0
    for k in range(calls):
        r, d = rewards(T, S, kind, k, seed), dones(T, E, pattern, k, seed)
        exp = ref.call(r, d)
        got = impl.call(r, d)
        worst = max(worst, assert_call(got, r, exp, eps, clip, 'E=%d N=%d T=%d %s done=%s clip=%g call %d' % (E, N, T, kind, pattern, clip, k)))
    return worst

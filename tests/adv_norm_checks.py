"""Checks of the opt-in per-batch advantage standardisation (csrc/a2c.hip: standardize_moments_kernel / standardize_apply_kernel),
written as functions of the implementation under test: `ops` on the GPU (tests/test_gpu_adv_norm.py), a plain chunked loop or a
deliberately wrong variant of it on the CPU (tests/test_adv_norm_cpu.py, which proves that the check is sharp).  For a group of `rows`
fp32 values x, everything in float64, one rounding to fp32:

    mu    = (1 / rows) sum x
    sigma = sqrt((1 / rows) sum (x - mu)^2)          population variance
    y     = (x - mu) / (sigma + eps)                 eps outside the root

Acceptance bound per element:  |got - exp| <= 2^-23 |exp| + rows 2^-52 (1 + mean|x| / (sigma + eps)).  The first term is one fp32
ulp of the single final rounding; the second the worst-case effect of any float64 summation order on mu (rows 2^-52 mean|x|, divided
by sigma + eps), plus rows 2^-52 for the order of the sum under the root.  The restatement itself sits at 0.  The moments (mu, sigma)
an implementation reports are held to 1e-12 relative: |got - exp| <= 1e-12 |exp| (absolute 1e-12 where exp is 0)."""
import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
EPS = 1e-8
SENTINEL = -777.0
KINDS = ('adv', 'offset', 'offset_small', 'tiny', 'huge', 'const', 'one_nan')


def expect(x, eps=EPS):
    """Two-pass float64 restatement of the definition on x [G, rows] -> (y [G, rows], mu [G], sigma [G]), float64, not rounded."""
    x64 = np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64)
    with np.errstate(all='ignore'):
        mu = x64.sum(axis=1) / x64.shape[1]
        c = x64 - mu[:, None]
        sigma = np.sqrt((c * c).sum(axis=1) / x64.shape[1])
        y = c / (sigma + eps)[:, None]
    return y, mu, sigma


def nan_group(G):
    """The group that holds the NaN of kind `one_nan`."""
    return min(1, G - 1)


def inputs(G, rows, kind):
    """[G, rows] fp32.  Group g is the kind's base data scaled by g + 1 and shifted by g (in the kind's own unit for `tiny` and `huge`,
    where a shift by 1 would erase or vanish in the data): moments pooled or swapped across groups show.
      adv           0.3 N(0,1) - 0.05: what an update sees
      offset        3e4 + 1e-2 N(0,1): E[x^2] - mu^2 in float64 is thousands of fp32 ulps off, fp32 arithmetic tens of percent
      offset_small  1e3 + 1e-3 N(0,1): the same at another ratio
      tiny          1e-20 N(0,1): eps dominates, the outputs are ~1e-12 (eps inside the root: ~1e-16)
      huge          1e18 N(0,1): fp32 squares overflow
      const         one value per group: all zeros, exactly
      one_nan       `adv` with one NaN in group nan_group(G): that group all NaN, the others finite and correct"""
    gen = torch.Generator().manual_seed(G * 1000003 + rows * 7 + KINDS.index(kind))
    z = torch.randn(G, rows, generator=gen, dtype=F64)
    g = torch.arange(G, dtype=F64).unsqueeze(1)
    if kind in ('adv', 'one_nan'):
        x = (0.3 * z - 0.05) * (g + 1) + g
    elif kind == 'offset':
        x = (3e4 + 1e-2 * z) * (g + 1) + g
    elif kind == 'offset_small':
        x = (1e3 + 1e-3 * z) * (g + 1) + g
    elif kind == 'tiny':
        x = 1e-20 * (z * (g + 1) + g)
    elif kind == 'huge':
        x = 1e18 * (z * (g + 1) + g)
    elif kind == 'const':
        x = (1.5 * (g + 1) + g).expand(G, rows)
    else:
        raise ValueError(kind)
    x = x.to(F32).contiguous()
    if kind == 'one_nan':
        x[nan_group(G), rows // 2] = float('nan')
    return x


def bound(exp_y, x, sigma, eps):
    """The acceptance bound per element, [G, rows] float64."""
    rows = x.shape[1]
    x64 = x.detach().cpu().numpy().astype(np.float64)
    with np.errstate(all='ignore'):
        second = rows * 2.0 ** -52 * (1.0 + np.abs(x64).mean(axis=1) / (sigma + eps))
        return 2.0 ** -23 * np.abs(exp_y) + second[:, None]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def assert_standardized(out, moments, x, eps, what=''):
    """out [G, rows] fp32 and moments [G, 2] float64 (or None) against the restatement of x [G, rows]: the same NaN pattern, every
    other element inside the bound, (mu, sigma) within 1e-12 relative.  Returns the worst fraction of the bound used."""
    exp_y, exp_mu, exp_sigma = expect(x, eps)
    got = out.detach().cpu().numpy().astype(np.float64)
    assert got.shape == exp_y.shape
    nan_exp = np.isnan(exp_y)
    assert np.array_equal(np.isnan(got), nan_exp), '%s: NaN pattern differs (%d got, %d expected)' % (what, np.isnan(got).sum(), nan_exp.sum())
    ok = ~nan_exp
    b = bound(exp_y, x, exp_sigma, eps)
    with np.errstate(all='ignore'):
        err = np.abs(got - exp_y)
    worst = float((err[ok] / b[ok]).max()) if ok.any() else 0.0
    print('standardize %s: %.3g of the bound' % (what, worst))
    assert bool((err[ok] <= b[ok]).all()), '%s: %.3g of the bound' % (what, worst)
    if moments is not None:
        m = moments.detach().cpu().numpy()
        for col, name, e in ((0, 'mu', exp_mu), (1, 'sigma', exp_sigma)):
            fin = np.isfinite(e)
            assert np.array_equal(np.isfinite(m[:, col]), fin), '%s: %s finite pattern %r' % (what, name, m[:, col])
            rel = np.abs(m[fin, col] - e[fin]) / np.where(e[fin] != 0, np.abs(e[fin]), 1.0)
            print('standardize %s: %s off by %.3g relative' % (what, name, rel.max() if rel.size else 0.0))
            assert bool((rel <= 1e-12).all()), '%s: %s %r against %r' % (what, name, m[:, col], e)
    return worst


def check(impl, dev, G, rows, kind, pitch=None, inplace=False, eps=EPS):
    """impl.standardize(x, eps, out=, moments=) against `expect` on inputs(G, rows, kind).  pitch: None = dense [G, rows] buffers,
    (px, py) = group pitches in floats of x and out (>= rows); inplace: out is x.  The floats of a pitch behind `rows` and `moments`
    are pre-filled with a sentinel: the tail must keep its bits, the moments must be written and lie within 1e-12 relative of the
    restatement's.  A NaN input must make its group's outputs (and moments) NaN and leave the others finite.  Returns the worst
    fraction of the bound used."""
    x0 = inputs(G, rows, kind)
    px, py = (rows, rows) if pitch is None else pitch
    assert px >= rows and py >= rows
    xb = torch.full((G, px), SENTINEL, dtype=F32)
    xb[:, :rows] = x0
    xb = xb.to(dev)
    yb = xb if inplace else torch.full((G, py), SENTINEL, dtype=F32, device=dev)
    x, out = xb[:, :rows], yb[:, :rows]
    moments = torch.full((G, 2), SENTINEL, dtype=F64, device=dev)
    ret = impl.standardize(x, eps, out=out, moments=moments)
    assert ret is out, 'the caller\'s `out` must be what comes back'
    what = 'G=%d rows=%d %s pitch=%s inplace=%s' % (G, rows, kind, pitch, inplace)
    # the tails keep their bits, and x keeps all of its bits unless the call is in place
    for name, buf, p in (('x', xb, px), ('out', yb, px if inplace else py)):
        if p > rows:
            assert bool((_bits(buf[:, rows:]) == _bits(torch.full((1,), SENTINEL))).all()), '%s: %s tail overwritten' % (what, name)
    if not inplace:
        assert torch.equal(_bits(xb[:, :rows]), _bits(x0)), '%s: x changed' % what
    worst = assert_standardized(out, moments, x0, eps, what)
    got = out.detach().cpu().numpy()
    if kind == 'one_nan':
        assert np.isnan(got[nan_group(G)]).all() and np.isnan(got).sum() == rows
    if kind == 'const':
        assert not got.any(), '%s: a constant group must give exact zeros' % what
    return worst

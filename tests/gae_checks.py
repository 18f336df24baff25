"""Checks of the opt-in GAE(lambda) return scan (csrc/a2c.hip: gae_kernel), written as functions of the implementation under test:
`ops` on the GPU (tests/test_gpu_gae.py), the float64 restatement below or a deliberately wrong variant of it on the CPU
(tests/test_gae_cpu.py, which proves that the check is sharp).  Per agent n and replica e, backwards over the batch:

    rho[t] = r[t,e]                              global reward (alpha < 0)
           = sum_j alpha^dist(n,j) r[t,e,j]      spatial (alpha >= 0; dist < 0: weight 0)
    next = R_end[n,e];  A = 0
    for t = T-1 .. 0:
        keep  = 1 - d[t,e]
        delta = rho[t] + (gamma next) keep - v[t,n,e]
        A     = delta + ((gamma lambda) A) keep
        Adv[n,t,e] = A;  R[n,t,e] = A + v[t,n,e];  next = v[t,n,e]

Inputs are drawn the way update_edge_checks.check_nstep draws them; the bounds are the return scan's own."""
import numpy as np
import torch

from update_edge_checks import NSTEP_SPATIAL_ATOL, NSTEP_SPATIAL_RTOL, _same_bits, nstep_table

F32, F64 = torch.float32, torch.float64
GAE_GAMMA = 0.99


def gae_weights(alpha, dist):
    """alpha^dist [N,N] in float64, 0 for unreachable pairs (dist < 0); pow(0, 0) = 1."""
    d64 = dist.cpu().numpy().astype(np.float64)
    return torch.from_numpy(np.where(d64 < 0, 0.0, np.power(float(alpha), np.maximum(d64, 0.0))))


def gae_rho(r, alpha, dist, N):
    """The reward term of every step: [T,N,E] float64."""
    r64 = r.double().cpu()
    if alpha < 0:
        return r64.unsqueeze(1).expand(r64.shape[0], N, r64.shape[1])
    return torch.einsum('nj,tej->tne', gae_weights(alpha, dist), r64)


def gae_expect(r, v, done_post, R_end, gamma, lam, alpha, dist=None):
    """float64 restatement of the definition -> (R, Adv) [N,T,E] float64 (not rounded)."""
    T, N, E = v.shape
    v64, keep = v.double().cpu(), 1.0 - done_post.double().cpu()
    rho = gae_rho(r, alpha, dist, N)
    nxt, A = R_end.double().cpu().clone(), torch.zeros(N, E, dtype=F64)
    R, Adv = torch.zeros(N, T, E, dtype=F64), torch.zeros(N, T, E, dtype=F64)
    for t in range(T - 1, -1, -1):
        k = keep[t].unsqueeze(0)
        delta = rho[t] + (gamma * nxt) * k - v64[t]
        A = delta + ((gamma * lam) * A) * k
        Adv[:, t] = A
        R[:, t] = A + v64[t]
        nxt = v64[t]
    return R, Adv


def gae_inputs(N, E, T, alpha, table):
    """r, v, done, R_end, dist of update_edge_checks.check_nstep (same generator, same order of draws)."""
    gen = torch.Generator().manual_seed(N * 10007 + E * 101 + T)
    spatial = alpha >= 0
    r = torch.randn((T, E, N) if spatial else (T, E), generator=gen)
    v = torch.randn(T, N, E, generator=gen)
    done = (torch.rand(T, E, generator=gen) < 0.3).to(torch.uint8)
    e_idx = torch.arange(E)
    done[T - 1, e_idx % 4 == 1] = 1
    done[0, e_idx % 4 == 2] = 1
    R_end = torch.randn(N, E, generator=gen)
    dist = nstep_table(N, table, gen)
    if table == 'directed':
        assert bool((dist != dist.t()).any()) and bool((dist < 0).any())
    return r, v, done, R_end, dist


def within_one_ulp(got, exp64):
    """got (fp32) within one fp32 ulp of the float64 expectation rounded to fp32 -> (all ok, number of entries not equal)."""
    e32 = exp64.float()
    lo = torch.nextafter(e32, torch.full_like(e32, -float('inf')))
    hi = torch.nextafter(e32, torch.full_like(e32, float('inf')))
    got = got.detach().cpu()
    return bool(((got >= lo) & (got <= hi)).all()), int((got != e32).sum())


def assert_gae_close(got_R, got_A, exp_R, exp_A, spatial, what=''):
    """The return scan's bounds: global path one fp32 ulp of the rounded expectation; spatial path rtol 2e-7 + atol 1e-7 max|R|.
    Returns the worst figure (entries off the rounded expectation / fraction of the bound)."""
    worst = 0.0
    for name, got, exp in (('R', got_R, exp_R), ('Adv', got_A, exp_A)):
        if spatial:
            err = (got.detach().cpu().double() - exp).abs()
            bound = NSTEP_SPATIAL_RTOL * exp.abs() + NSTEP_SPATIAL_ATOL * float(exp_R.abs().max())
            rel = float((err / bound).max())
            print('gae spatial %s %s: %.3g of the bound' % (what, name, rel))
            worst = max(worst, rel) if rel == rel else float('nan')
            assert bool((err <= bound).all()), '%s %s: %.3g of the bound' % (what, name, rel)
        else:
            ok, n_off = within_one_ulp(got, exp)
            print('gae global %s %s: %d entries one ulp off' % (what, name, n_off))
            worst = max(worst, float(n_off))
            assert ok, '%s %s: entries more than one fp32 ulp off' % (what, name)
    return worst


def check_gae(impl, dev, N, E, T, alpha, table, lam):
    """impl.gae_return against gae_expect on check_nstep's inputs (done with probability 0.3, done[T-1] forced on e % 4 == 1 -- next
    and the A carry must both be masked there -- and done[0] on e % 4 == 2).  Shapes (N,T,E), fp32; a second call with
    caller-supplied outputs pre-filled with -777 must return those objects with the same bits."""
    r, v, done, R_end, dist = gae_inputs(N, E, T, alpha, table)
    spatial = alpha >= 0
    exp_R, exp_A = gae_expect(r, v, done, R_end, GAE_GAMMA, lam, alpha, dist)
    pass_dist = dist.to(dev) if (spatial or table == 'directed') else None        # ignored on the global path
    args = (r.to(dev), v.to(dev), done.to(dev), R_end.to(dev), GAE_GAMMA, lam, alpha, pass_dist)
    R1, A1 = impl.gae_return(*args)
    assert tuple(R1.shape) == (N, T, E) and tuple(A1.shape) == (N, T, E) and R1.dtype == F32 and A1.dtype == F32
    worst = assert_gae_close(R1, A1, exp_R, exp_A, spatial, 'N=%d E=%d T=%d alpha=%g %s lam=%g' % (N, E, T, alpha, table, lam))
    R_out, adv_out = torch.full((N, T, E), -777.0, device=dev), torch.full((N, T, E), -777.0, device=dev)
    R2, A2 = impl.gae_return(*args, R_out=R_out, adv_out=adv_out)
    assert R2 is R_out and A2 is adv_out
    assert _same_bits(R2, R1) and _same_bits(A2, A1)
    return worst

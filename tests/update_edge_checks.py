"""Edge checks of the update path's small kernels (csrc/a2c.hip: return scan, clip + RMSProp, action draw, batch epilogue,
multi-copy), written as functions of the implementation under test: `ops` on the GPU (tests/test_gpu_update_edges.py), the
restatement `oracle/ops_ref` or a deliberately wrong variant of it on the CPU (tests/test_update_edges_cpu.py, which proves that
every check is sharp).  Each check draws its inputs from a seeded generator, forms the expectation in float64 itself from the
reference's formulas (agents/utils.py:763-775, 800-816; policies.py:32-39; utils.py:135-141), asserts, and returns the worst
error it measured.  The C-ABI carries lr / rho / eps / max_norm / grad_scale as `float`: they are rounded to fp32 before the
float64 expectation uses them, so no check is about `1.0f - 0.99f`."""
import numpy as np
import torch

from oracle import philox

F32, F64 = torch.float32, torch.float64


def _f32(x):
    return float(np.float32(x))


def _bits(t):
    """Bit pattern of a tensor (float equality treats -0.0 == 0.0 and nan != nan)."""
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# --------------------------------------------------------------------------------------------------------- clip + RMSProp
RMSPROP_SHAPES = [(3, 77, -1.0, 1.0),              # no clip
                  (8, 1000, 0.5, 0.125),           # clipped (group 0 of the first step is just below max_norm: both branches)
                  (2, 300, 40.0, 1.0),             # not clipped
                  (1, 262144 * 2 + 5, 40.0, 0.5)]  # above the 1024-block grid stride
RMSPROP_STEP_RTOL = 4e-6       # of the step: its ~10 fp32 roundings and the fixed-order norm sum
RMSPROP_STATE_RTOL = 4e-6      # ms and the reported norm


def check_rmsprop(impl, dev, G, P, max_norm, grad_scale, use_lr_dev):
    """tf.clip_by_global_norm + TF-1.12 ApplyRMSProp (policies.py:32-39): three consecutive steps with growing gradients.  The
    float64 expectation restarts from the implementation's own fp32 state before each step (errors do not compound).  ms starts
    in [0, 1e-4], where eps = 1e-5 inside or outside the sqrt moves the step by percents; the groups' norms differ by x3; the last
    group's gradient is all zero (1/norm = inf in the clip); every eighth weight starts at 0, where the step's own error is not
    hidden below the rounding of the stored weight.  use_lr_dev: the host lr is wrong on purpose (1.0), the right one arrives in a
    device scalar that is rewritten before the third step.
    Per element |w - w64| <= 2^-23 |w64| + 4e-6 |dw64|; ms and norm_out to rtol 4e-6."""
    gen = torch.Generator().manual_seed(G * 1009 + P)
    lr, rho, eps = _f32(5e-4), _f32(0.99), _f32(1e-5)
    mn, gs = _f32(max_norm), _f32(grad_scale)
    w = torch.randn(G, P, generator=gen)
    w[:, ::8] = 0.0
    ms = torch.rand(G, P, generator=gen) * 1e-4
    g0 = torch.randn(G, P, generator=gen) * 0.05 * (3.0 ** (torch.arange(G) % 3).float()).view(G, 1)
    if G > 1:
        g0[G - 1] = 0.0
    wd, msd = w.to(dev), ms.to(dev)
    scratch, norm_out = torch.zeros(G, 64, device=dev), torch.full((G,), -7.0, device=dev)
    lr_steps = [lr, lr, _f32(2.5e-4)] if use_lr_dev else [lr] * 3
    lr_dev = torch.zeros(1, device=dev) if use_lr_dev else None
    worst = dict(step=0.0, bound_used=0.0, ms=0.0, norm=0.0)
    for it in range(3):
        g = g0 * float(it + 1)
        w64, m64, g64 = wd.cpu().double(), msd.cpu().double(), g.double()
        norm64 = g64.pow(2).sum(dim=1, keepdim=True).sqrt() * abs(gs)
        scale = torch.full_like(norm64, gs)
        if mn > 0:
            scale = gs * (mn * torch.minimum(1.0 / norm64, torch.full_like(norm64, 1.0 / mn)))
        gc = g64 * scale
        m_exp = m64 + (gc * gc - m64) * (1.0 - rho)
        dw = lr_steps[it] * gc / torch.sqrt(m_exp + eps)
        w_exp = w64 - dw
        if use_lr_dev:
            lr_dev.fill_(lr_steps[it])
        impl.rmsprop_tf_clip(wd, g.to(dev), msd, scratch, 1.0 if use_lr_dev else lr, rho, eps, mn, gs, norm_out, lr_dev=lr_dev)
        w_got, m_got, n_got = wd.cpu().double(), msd.cpu().double(), norm_out.cpu().double()
        err = (w_got - w_exp).abs()
        bound = 2.0 ** -23 * w_exp.abs() + RMSPROP_STEP_RTOL * dw.abs()
        small = (w64.abs() <= 4 * dw.abs()) & (dw != 0)            # the weights that started at 0: the step's error shows
        step_err = float((err[small] / dw.abs()[small]).max()) if bool(small.any()) else 0.0
        used = float((err / bound.clamp_min(1e-300)).max())
        m_err = float(((m_got - m_exp).abs() / m_exp.abs().clamp_min(1e-300)).max())
        n_exp = norm64.view(-1)
        n_err = float(((n_got - n_exp).abs() / n_exp.clamp_min(1e-300)).max())
        print('rmsprop G=%d P=%d max_norm=%g scale=%g lr_dev=%d step %d: step %.3g, bound used %.3g, ms %.3g, norm %.3g'
              % (G, P, mn, gs, use_lr_dev, it, step_err, used, m_err, n_err))
        for k, v in (('step', step_err), ('bound_used', used), ('ms', m_err), ('norm', n_err)):
            worst[k] = max(worst[k], v) if v == v else float('nan')
        assert bool((err <= bound).all()), 'w: %.3g of the bound (step %d)' % (used, it)
        assert bool(((m_got - m_exp).abs() <= RMSPROP_STATE_RTOL * m_exp.abs()).all()), 'ms: rel %.3g (step %d)' % (m_err, it)
        assert bool(((n_got - n_exp).abs() <= RMSPROP_STATE_RTOL * n_exp).all()), 'norm: rel %.3g (step %d)' % (n_err, it)
        assert bool(small.any())
    return worst


def check_rmsprop_guard(dev):
    """nmarl_rmsprop_tf_clip_guarded with a private status tensor (no global state): while word 0 is set the step changes
    neither w nor ms and counts itself in word 1; with word 0 cleared it is the unguarded step bit for bit.  The word is set from
    the host: nothing faults."""
    from deeprl_network_amd import _lib
    lib, ptr = _lib.lib, _lib.ptr
    G, P = 3, 1000
    gen = torch.Generator().manual_seed(5)
    w0, g = torch.randn(G, P, generator=gen).to(dev), (torch.randn(G, P, generator=gen) * 0.05).to(dev)
    ms0 = (torch.rand(G, P, generator=gen) * 1e-4).to(dev)
    scratch, norm = torch.zeros(G, 64, device=dev), torch.zeros(G, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    args = (None, _f32(5e-4), _f32(0.99), _f32(1e-5), _f32(0.5), _f32(0.5))

    def guarded(w, ms):
        _lib.check(lib.nmarl_rmsprop_tf_clip_guarded(G, P, ptr(w, F32), ptr(g, F32), ptr(ms, F32), ptr(scratch, F32), *args,
                                                     ptr(norm, F32), ptr(status, torch.int32), _lib.stream()), 'guarded')

    w, ms = w0.clone(), ms0.clone()
    status[0] = 1
    for n in (1, 2):
        guarded(w, ms)
        assert status.tolist() == [1, n, 0, 0], status.tolist()
        assert _same_bits(w, w0) and _same_bits(ms, ms0)
    status[0] = 0
    guarded(w, ms)
    assert status.tolist() == [0, 2, 0, 0], status.tolist()
    w2, ms2 = w0.clone(), ms0.clone()
    _lib.check(lib.nmarl_rmsprop_tf_clip(G, P, ptr(w2, F32), ptr(g, F32), ptr(ms2, F32), ptr(scratch, F32), *args, ptr(norm, F32),
                                         _lib.stream()), 'unguarded')
    assert _same_bits(w, w2) and _same_bits(ms, ms2)
    assert not _same_bits(w, w0) and not _same_bits(ms, ms0)


# ------------------------------------------------------------------------------------------------------------ return scan
NSTEP_SHAPES = [(3, 5, 13), (28, 37, 21), (64, 3, 11), (8, 300, 10), (2, 1, 1)]
NSTEP_ALPHAS = [-1.0, 0.9, 0.0, 1.0]
NSTEP_TABLES = ['line', 'directed']
NSTEP_SPATIAL_RTOL, NSTEP_SPATIAL_ATOL = 2e-7, 1e-7      # atol in units of max |R|


def nstep_table(N, table, gen):
    idx = torch.arange(N)
    if table == 'line':
        return (idx[:, None] - idx[None, :]).abs().to(torch.int32)
    d = torch.randint(0, 6, (N, N), generator=gen, dtype=torch.int32)
    d[torch.rand(N, N, generator=gen) < 0.15] = -1                   # unreachable pairs of a directed graph
    d[idx, idx] = 0
    d[0, 1], d[1, 0] = -1, 2                                         # at the smallest N too: one-way reachability
    return d


def check_nstep(impl, dev, N, E, T, alpha, table):
    """n-step return and advantage (agents/utils.py:763-775 global, 800-816 spatially discounted) against the float64 recurrence.
    done has probability 0.3, done[T-1] is forced on the replicas e % 4 == 1 (R_end must be masked) and done[0] on e % 4 == 2.
    Global path: the float64 operation order is the expectation's, so R and Adv are the expectation rounded to fp32, to within
    one fp32 ulp.  Spatial path: rtol 2e-7, atol 1e-7 max|R| (the sum over j in another order, both in float64).  A second call
    with caller-supplied outputs must return those tensors with the same bits."""
    gen = torch.Generator().manual_seed(N * 10007 + E * 101 + T)
    spatial = alpha >= 0
    gamma = 0.99
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
    # float64 expectation
    keep = 1.0 - done.double()
    R = R_end.double().clone()
    Rs = torch.zeros(N, T, E, dtype=F64)
    if spatial:
        d64 = dist.numpy().astype(np.float64)
        wt = torch.from_numpy(np.where(d64 < 0, 0.0, np.power(float(alpha), np.maximum(d64, 0.0))))     # pow(0, 0) = 1
    for t in range(T - 1, -1, -1):
        if spatial:
            R = (gamma * R) * keep[t].unsqueeze(0) + wt @ r[t].double().t()
        else:
            R = r[t].double().unsqueeze(0) + (gamma * R) * keep[t].unsqueeze(0)
        Rs[:, t] = R
    adv = Rs - v.double().permute(1, 0, 2)
    pass_dist = dist.to(dev) if (spatial or table == 'directed') else None        # ignored on the global path
    args = (r.to(dev), v.to(dev), done.to(dev), R_end.to(dev), gamma, alpha, pass_dist)
    R1, A1 = impl.nstep_return(*args)
    assert tuple(R1.shape) == (N, T, E) and tuple(A1.shape) == (N, T, E) and R1.dtype == F32 and A1.dtype == F32
    worst = 0.0
    for name, got, exp in (('R', R1, Rs), ('Adv', A1, adv)):
        got = got.cpu()
        if spatial:
            err = (got.double() - exp).abs()
            bound = NSTEP_SPATIAL_RTOL * exp.abs() + NSTEP_SPATIAL_ATOL * float(Rs.abs().max())
            rel = float((err / bound).max())
            print('nstep spatial N=%d E=%d T=%d alpha=%g %s %s: %.3g of the bound' % (N, E, T, alpha, table, name, rel))
            worst = max(worst, rel) if rel == rel else float('nan')
            assert bool((err <= bound).all()), '%s: %.3g of the bound' % (name, rel)
        else:
            e32 = exp.float()
            lo = torch.nextafter(e32, torch.full_like(e32, -float('inf')))
            hi = torch.nextafter(e32, torch.full_like(e32, float('inf')))
            ok = (got >= lo) & (got <= hi)
            n_off = int((got != e32).sum())
            worst = max(worst, float(n_off))
            assert bool(ok.all()), '%s: %d entries more than one fp32 ulp off' % (name, int((~ok).sum()))
    R_out, adv_out = torch.full((N, T, E), -777.0, device=dev), torch.full((N, T, E), -777.0, device=dev)
    R2, A2 = impl.nstep_return(*args, R_out=R_out, adv_out=adv_out)
    assert R2 is R_out and A2 is adv_out
    assert _same_bits(R2, R1) and _same_bits(A2, A1)
    return worst


def check_nstep_abi_refusals(dev):
    """N = 65 (the LDS table holds 64 x 64 weights) and alpha >= 0 without a distance table: NMARL_EINVAL, nothing written."""
    from deeprl_network_amd import _lib
    lib, ptr = _lib.lib, _lib.ptr
    for N, alpha, with_dist in ((65, -1.0, True), (65, 0.9, True), (4, 0.9, False), (4, 0.0, False)):
        E, T = 2, 3
        r = torch.zeros(T, E, N, device=dev)
        v, done, R_end = torch.zeros(T, N, E, device=dev), torch.zeros(T, E, dtype=torch.uint8, device=dev), torch.zeros(N, E, device=dev)
        dist = torch.zeros(N, N, dtype=torch.int32, device=dev) if with_dist else None
        R_out, adv_out = torch.full((N, T, E), -777.0, device=dev), torch.full((N, T, E), -777.0, device=dev)
        rc = lib.nmarl_nstep_return(E, N, T, ptr(r, F32), ptr(v, F32), ptr(done, torch.uint8), ptr(R_end, F32), 0.99, alpha,
                                    ptr(dist, torch.int32), ptr(R_out), ptr(adv_out), _lib.stream())
        assert rc == -1, (N, alpha, with_dist, rc)                    # NMARL_EINVAL
        torch.cuda.synchronize()
        assert bool((R_out == -777.0).all()) and bool((adv_out == -777.0).all())


# ------------------------------------------------------------------------------------------------------------ action draw
SAMPLE_E = 33
SAMPLE_SHAPES = [(3, 4), (5, 1), (7, 9), (28, 37), (6, 255)]       # (N, A)
SAMPLE_MODES = ['philox', 'uniform', 'argmax']
SAMPLE_SEED, SAMPLE_ENV_BASE, SAMPLE_STEP, SAMPLE_STEP_DEV = (0x9E37 << 32) + 12345, 777, 5, 37


def _inverse_cdf(p, u):
    """np.random.choice(arange(A), p=pi) with the uniform u (utils.py:138): searchsorted(cumsum(p) / sum, u, side='right')."""
    cdf = np.cumsum(p.astype(np.float64), axis=-1)
    cdf = cdf / cdf[..., -1:]
    return np.minimum((cdf <= u.astype(np.float64)[..., None]).sum(-1), p.shape[-1] - 1)


def check_sample(impl, dev, N, E, A, mode):
    """The action draw (utils.py:135-141) == the float64 inverse CDF, entry for entry.
    philox: a seed above 2^32, env_id_base 777, host step 5 + device step 37, N not a multiple of 4 (word n & 3 of counter n >> 2).
    uniform: rows built in turn as pi x 3.7 (renormalised) | exact zeros at the front, the middle and the end | dyadic pi with u on the
    cumulative boundaries 0, 1/4, 1/2 (the next bin: side='right') | u = 1 - 2^-24 | u = 1 (the clamp to A - 1) | plain.
    argmax: rows with two and with three equal maxima (the first wins)."""
    gen = np.random.RandomState(N * 1000 + A)
    p = gen.dirichlet(np.ones(A), size=(E, N)).astype(np.float32) if A > 1 else np.ones((E, N, 1), np.float32)
    row = np.arange(E * N).reshape(E, N)
    kw = {}
    if mode == 'philox':
        u = philox.action_uniform(SAMPLE_SEED, SAMPLE_ENV_BASE + np.arange(E), N, SAMPLE_STEP + SAMPLE_STEP_DEV)
        want = _inverse_cdf(p, u)
        kw = dict(seed=SAMPLE_SEED, env_id_base=SAMPLE_ENV_BASE, step=SAMPLE_STEP,
                  step_dev=torch.tensor(SAMPLE_STEP_DEV, dtype=torch.int64).to(dev))
        code = 1
    elif mode == 'uniform':
        u = gen.random_sample((E, N)).astype(np.float32)
        kind = row % 6
        p[kind == 0] *= np.float32(3.7)
        if A >= 4:
            for k in (0, A // 2, A - 1):
                p[kind == 1, k] = 0.0
        dy = np.zeros(A, np.float32)
        dy[:min(A, 4)] = 1.0 / min(A, 4) if A < 4 else 0.25
        p[kind == 2] = dy
        u[kind == 2] = (np.array([0.0, 0.25, 0.5], np.float32)[(row // 6) % 3])[kind == 2]
        u[kind == 3] = np.float32(1.0 - 2.0 ** -24)
        u[kind == 4] = np.float32(1.0)
        want = _inverse_cdf(p, u)
        if A >= 4:
            assert (want[kind == 2] == ((row // 6) % 3)[kind == 2]).all()          # the boundary falls into the NEXT bin
            assert (want[kind == 1] != 0).all() and (want[kind == 1] != A - 1).all()
        assert (want[kind == 4] == A - 1).all()
        kw = dict(u=torch.from_numpy(u).to(dev))
        code = 0
    else:
        for m, k in ((2, 1), (3, 2)):
            for e, n in zip(*np.nonzero(row % 3 == k)):
                pos = gen.permutation(A)[:min(m, A)]
                p[e, n, pos] = p[e, n].max() + np.float32(0.125)
        want = p.argmax(-1)                                                        # np.argmax: the first maximum
        code = 2
    pi = torch.from_numpy(np.ascontiguousarray(p.transpose(1, 0, 2)))             # [N,E,A]
    out = torch.full((E, N), 255, dtype=torch.uint8, device=dev)
    got = impl.sample_actions(pi.to(dev), out, code, **kw)
    got = (out if got is None else got).cpu().numpy()
    bad = int((got != want.astype(np.uint8)).sum())
    assert bad == 0, '%d of %d draws differ (N=%d A=%d %s)' % (bad, E * N, N, A, mode)
    return bad


# --------------------------------------------------------------------------------------------------------- batch epilogue
EPILOGUE_SHAPES = [(3, 70, 8, 3, 4, 13), (2, 5, 4, 1, 1, 25), (1, 256 * 1024 + 3, 4, 1, 1, 2)]    # (N, E, H, A, F, T)
EPILOGUE_STATE = ('ep_sum', 'ep_sq', 'ep_len', 'h_fw', 'c_fw', 'h_bw', 'c_bw', 'fp_0', 'x_0', 'done_pre', 'fin')
EPILOGUE_HISTORY = 997.0


def epilogue_const_rewards(E):
    """The constant reward of replica e (used where e % 3 == 0): seven fp32 values in [-0.175, -0.1]."""
    return torch.from_numpy(np.float32(-0.1 * (1.0 + (np.arange(E) % 7) / 8.0)))


def check_epilogue(impl, dev, N, E, H, A, F, T, n_batches=4, skip_pattern=False):
    """nmarl_batch_epilogue over n_batches batches with done probability 0.3 (episodes span 1..n_batches batches; T_env = 3 T, so
    some close early = collisions, some exactly at T_env, some later) against oracle/ops_ref.batch_epilogue run on float64 state.
    A third of the replicas (e % 3 == 0) has a constant reward c (one of seven fp32 values) and an episode of 997 such steps behind
    it, whose rounded sum of squares puts var = sq/len - mean^2 within a few 2^-53 c^2 of zero on either side: without the clamp
    fin[2] is nan.
    skip_pattern: a device int32 word, non-zero on batches 1 and 2 -- every state tensor and fin keeps its bits there, and batch 3
    continues from batch 0's state.
    The fp32 state must be equal; the float64 statistics to rtol 1e-12, atol 1e-9 (sums in another order); fin[2] gets, per closed
    constant-reward episode, sqrt(k 2^-53) |c| more with k = n_batches + 2: its var carries at most k roundings of sq (the history,
    one add per batch, the division), each <= 2^-53 c^2, mean and mean^2 being exact (c has 24 bits), so its std lies in
    [0, sqrt(k 2^-53) |c|] whatever the order (1e-8 per episode; the other episodes' std is ~29)."""
    from oracle import ops_ref
    gen = torch.Generator().manual_seed(N * 31 + E + T)
    T_env = 3 * T
    c32 = epilogue_const_rewards(E)
    c, c_max = c32.double(), float(c32.abs().max())
    const = torch.arange(E) % 3 == 0
    z64 = torch.zeros(E, dtype=F64)
    host = dict(ep_sum=torch.where(const, EPILOGUE_HISTORY * c, z64), ep_sq=torch.where(const, EPILOGUE_HISTORY * c * c, z64),
                ep_len=torch.where(const, z64 + EPILOGUE_HISTORY, z64), fin=torch.zeros(4, dtype=F64),
                h_fw=torch.randn(N, E, H, generator=gen).double(), c_fw=torch.randn(N, E, H, generator=gen).double(),
                h_bw=torch.zeros(N, E, H, dtype=F64), c_bw=torch.zeros(N, E, H, dtype=F64), fp_0=torch.zeros(N, E, A, dtype=F64),
                x_0=torch.zeros(E, N, F, dtype=F64), done_pre=torch.zeros(E, dtype=F64))
    stats = ('ep_sum', 'ep_sq', 'ep_len', 'fin')
    prod = {k: (v.clone() if k in stats else v.float()).to(dev) for k, v in host.items()}
    fp_uniform = torch.rand(N, 1, A, generator=gen)
    word = torch.zeros(1, dtype=torch.int32, device=dev) if skip_pattern else None
    n_const_closed, worst = 0, 0.0
    for b in range(n_batches):
        g = -torch.rand(T, E, generator=gen) * 100
        g[:, const] = c32[const]
        done = (torch.rand(E, generator=gen) < 0.3).to(torch.uint8)
        fp_T, x_T = torch.rand(N, E, A, generator=gen), torch.randn(E, N, F, generator=gen)
        skipped = skip_pattern and b in (1, 2)
        if skip_pattern:
            word.fill_(3 if skipped else 0)
        before = {k: prod[k].clone() for k in EPILOGUE_STATE}
        ops_ref.batch_epilogue(g, done, host['ep_sum'], host['ep_sq'], host['ep_len'], host['fin'], T_env, host['h_fw'], host['c_fw'],
                               host['h_bw'], host['c_bw'], fp_T.double(), host['fp_0'], fp_uniform.double(), x_T.double(), host['x_0'],
                               host['done_pre'], skip_if=None if word is None else word.cpu())
        impl.batch_epilogue(g.to(dev), done.to(dev), prod['ep_sum'], prod['ep_sq'], prod['ep_len'], prod['fin'], T_env, prod['h_fw'],
                            prod['c_fw'], prod['h_bw'], prod['c_bw'], fp_T.to(dev), prod['fp_0'], fp_uniform.to(dev), x_T.to(dev),
                            prod['x_0'], prod['done_pre'], skip_if=word)
        if skipped:
            for k in EPILOGUE_STATE:
                assert _same_bits(prod[k], before[k]), 'batch %d is skipped, %s changed' % (b, k)
        else:
            n_const_closed += int((done.bool() & const).sum())
        for k in ('h_fw', 'c_fw', 'h_bw', 'c_bw', 'fp_0', 'x_0', 'done_pre'):
            assert torch.equal(prod[k].cpu().double(), host[k]), 'batch %d: %s' % (b, k)
        for k in stats:
            got, exp = prod[k].cpu(), host[k]
            atol = torch.full_like(exp, 1e-9)
            if k == 'fin':
                atol[2] += n_const_closed * ((n_batches + 2) * 2.0 ** -53) ** 0.5 * c_max
            err = (got - exp).abs()
            bound = atol + 1e-12 * exp.abs()
            rel = float((err / bound).max())
            worst = max(worst, rel) if rel == rel else float('nan')
            assert bool((err <= bound).all()), 'batch %d: %s at %.3g of its bound (%s vs %s)' % (b, k, rel, got[:4].tolist(), exp[:4].tolist())
    fin = host['fin']
    assert fin[0] > 0 and (E < 50 or (fin[3] > 0 and fin[0] > fin[3])) and n_const_closed > 0
    return worst


# ------------------------------------------------------------------------------------------------------------- multi-copy
def check_copy_multi_skip(dev):
    """nmarl_copy_multi with its skip word: 18 pairs (two launches) of odd byte counts, one source and one destination off the
    16-byte grid, one empty pair.  Word set: nothing is copied; word cleared: everything is."""
    from deeprl_network_amd import ops
    gen = torch.Generator().manual_seed(18)
    sizes = [1, 3, 17, 255, 4099, 0, 16, 31, 33, 1000, 4096, 7, 65, 129, 513, 2049, 5, 70001]
    assert len(sizes) == 18 > ops.COPY_MAX
    pool = torch.randint(0, 255, (sum(sizes) + 64,), generator=gen, dtype=torch.uint8).to(dev)
    pairs, o = [], 3                                                     # sources packed from byte 3 on: most are unaligned
    for i, n in enumerate(sizes):
        src = pool[o:o + n]
        o += n
        if i == 4:                                                       # a destination off the grid as well
            dst = torch.full((n + 5,), 0xAB, dtype=torch.uint8, device=dev)[5:]
        elif i in (6, 10):                                               # float tensors, both ends aligned (the 16-byte path)
            src = torch.randn(n // 4, generator=gen).to(dev)
            dst = torch.full((n // 4,), -777.0, device=dev)
        else:
            dst = torch.full((n,), 0xAB, dtype=torch.uint8, device=dev)
        pairs.append((dst, src))
    assert pairs[0][1].data_ptr() % 16 != 0 and pairs[4][0].data_ptr() % 16 != 0
    sentinels = [d.clone() for d, _ in pairs]
    word = torch.ones(1, dtype=torch.int32, device=dev)
    ops.copy_multi(pairs, skip_if=word)
    for (d, _), s0 in zip(pairs, sentinels):
        assert _same_bits(d, s0)
    word.zero_()
    ops.copy_multi(pairs, skip_if=word)
    for i, (d, s) in enumerate(pairs):
        assert _same_bits(d, s), i

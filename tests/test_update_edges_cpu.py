"""The edge checks of tests/update_edge_checks.py are sharp: (a) the restatement oracle/ops_ref alone (fp32 on the CPU) stays within
every bound, (b) every named wrong variant of it -- the mistakes the small update kernels of csrc/a2c.hip could make without the
older tests noticing -- makes its check raise."""
import types

import numpy as np
import pytest
import torch

import update_edge_checks as uec
from oracle import ops_ref, philox


def _impl(**replaced):
    ns = types.SimpleNamespace(**{k: getattr(ops_ref, k) for k in ('rmsprop_tf_clip', 'nstep_return', 'sample_actions', 'batch_epilogue')})
    for k, v in replaced.items():
        setattr(ns, k, v)
    return ns


# ------------------------------------------------------------------------------------------ (a) the restatement passes
@pytest.mark.parametrize('use_lr_dev', [False, True])
@pytest.mark.parametrize('G,P,max_norm,grad_scale', uec.RMSPROP_SHAPES)
def test_restatement_rmsprop(G, P, max_norm, grad_scale, use_lr_dev):
    uec.check_rmsprop(ops_ref, 'cpu', G, P, max_norm, grad_scale, use_lr_dev)


@pytest.mark.parametrize('table', uec.NSTEP_TABLES)
@pytest.mark.parametrize('alpha', uec.NSTEP_ALPHAS)
@pytest.mark.parametrize('N,E,T', uec.NSTEP_SHAPES)
def test_restatement_nstep(N, E, T, alpha, table):
    uec.check_nstep(ops_ref, 'cpu', N, E, T, alpha, table)


@pytest.mark.parametrize('mode', uec.SAMPLE_MODES)
@pytest.mark.parametrize('N,A', uec.SAMPLE_SHAPES)
def test_restatement_sample(N, A, mode):
    uec.check_sample(ops_ref, 'cpu', N, uec.SAMPLE_E, A, mode)


@pytest.mark.parametrize('skip_pattern', [False, True])
@pytest.mark.parametrize('N,E,H,A,F,T', uec.EPILOGUE_SHAPES)
def test_restatement_epilogue(N, E, H, A, F, T, skip_pattern):
    uec.check_epilogue(ops_ref, 'cpu', N, E, H, A, F, T, 4, skip_pattern)


# ------------------------------------------------------------------------------------------ (b) the wrong variants fail
def _rmsprop_variant(eps_outside=False, ms_unclipped=False, no_min=False, scale_out_of_norm=False, group0=False, step_factor=1.0):
    """ops_ref.rmsprop_tf_clip in fp32 with one mistake switched on (none: the restatement itself)."""
    def f(w, g, ms, scratch, lr, rho, eps, max_norm, grad_scale=1.0, norm_out=None, lr_dev=None, guard=False):
        if lr_dev is not None:
            lr = lr_dev.reshape(-1)[0]
        gs = g * grad_scale
        norm = gs.pow(2).sum(dim=1, keepdim=True).sqrt()
        clip_norm = g.pow(2).sum(dim=1, keepdim=True).sqrt() if scale_out_of_norm else norm
        if group0:
            clip_norm = clip_norm[:1].expand_as(clip_norm)       # norm_out stays right: only the clip reads the wrong group
        gc = gs
        if max_norm > 0:
            gc = gs * (max_norm / clip_norm) if no_min else \
                gs * (max_norm * torch.minimum(1.0 / clip_norm, torch.full_like(clip_norm, 1.0 / max_norm)))
        gm = gs if ms_unclipped else gc
        ms.add_((gm * gm - ms) * (1.0 - rho))
        w.sub_(step_factor * lr * gc / (torch.sqrt(ms) + eps if eps_outside else torch.sqrt(ms + eps)))
        if norm_out is not None:
            norm_out.copy_(norm.view(-1))
    return f


def _rmsprop_no_lr_dev(w, g, ms, scratch, lr, rho, eps, max_norm, grad_scale=1.0, norm_out=None, lr_dev=None, guard=False):
    ops_ref.rmsprop_tf_clip(w, g, ms, scratch, float(np.float32(5e-4)), rho, eps, max_norm, grad_scale, norm_out)   # the right lr, once and for all


CLIPPED, UNCLIPPED = (8, 1000, 0.5, 0.125), (2, 300, 40.0, 1.0)
RMSPROP_MUTANTS = {
    'sqrt(m) + eps': (_rmsprop_variant(eps_outside=True), CLIPPED, False),
    'ms fed the unclipped gradient': (_rmsprop_variant(ms_unclipped=True), CLIPPED, False),
    'clip without the min': (_rmsprop_variant(no_min=True), UNCLIPPED, False),
    'grad_scale left out of the norm': (_rmsprop_variant(scale_out_of_norm=True), CLIPPED, False),
    'lr_dev ignored': (_rmsprop_no_lr_dev, CLIPPED, True),
    "every group uses group 0's norm": (_rmsprop_variant(group0=True), CLIPPED, False),
    'step x 1.02': (_rmsprop_variant(step_factor=1.02), CLIPPED, False),
}


def test_rmsprop_variant_without_a_mistake_passes():
    for shape in uec.RMSPROP_SHAPES[:3]:
        uec.check_rmsprop(_impl(rmsprop_tf_clip=_rmsprop_variant()), 'cpu', *shape, True)


@pytest.mark.parametrize('name', list(RMSPROP_MUTANTS))
def test_rmsprop_mutant_fails(name):
    fn, shape, use_lr_dev = RMSPROP_MUTANTS[name]
    with pytest.raises(AssertionError):
        uec.check_rmsprop(_impl(rmsprop_tf_clip=fn), 'cpu', *shape, use_lr_dev)


def test_rmsprop_eps_placement_is_pinned_at_every_shape():
    for shape in uec.RMSPROP_SHAPES[:3]:
        with pytest.raises(AssertionError):
            uec.check_rmsprop(_impl(rmsprop_tf_clip=_rmsprop_variant(eps_outside=True)), 'cpu', *shape, False)


def _nstep_wrap(kind):
    def f(r, v, done_post, R_end, gamma, alpha, dist=None, R_out=None, adv_out=None):
        T = v.shape[0]
        if kind == 'transposed' and dist is not None:
            dist = dist.t().contiguous()
        if kind == 'minus one is one hop' and dist is not None:
            dist = torch.where(dist < 0, torch.ones_like(dist), dist)
        if kind == 'done of t + 1':
            done_post = torch.cat([done_post[1:], done_post[-1:]])
        if kind == 'R_end not masked':
            done_post = done_post.clone()
            done_post[T - 1] = 0                                  # done[T-1] is read nowhere else
        R, A = ops_ref.nstep_return(r, v, done_post, R_end, gamma, alpha, dist, R_out, adv_out)
        if kind == 'tail unwritten':
            R[:, :T % 10] = -777.0                                # what the caller's buffer held
            A[:, :T % 10] = -777.0
        return R, A
    return f


NSTEP_MUTANTS = {
    'weight table transposed': ('transposed', (28, 37, 21, 0.9, 'directed')),
    '-1 treated as hop count 1': ('minus one is one hop', (28, 37, 21, 0.9, 'directed')),
    'done taken from step t + 1': ('done of t + 1', (3, 5, 13, -1.0, 'line')),
    'R_end not masked by done[T-1]': ('R_end not masked', (8, 300, 10, -1.0, 'line')),
    'the last T % 10 steps left unwritten': ('tail unwritten', (3, 5, 13, -1.0, 'line')),
}


@pytest.mark.parametrize('name', list(NSTEP_MUTANTS))
def test_nstep_mutant_fails(name):
    kind, case = NSTEP_MUTANTS[name]
    with pytest.raises(AssertionError):
        uec.check_nstep(_impl(nstep_return=_nstep_wrap(kind)), 'cpu', *case)


def test_nstep_mutants_on_the_other_path_and_the_old_table():
    """The mistakes that exist on both paths fail on both; the transposed table passes the old symmetric one (which is why it was
    invisible) and fails every directed one."""
    for kind in ('done of t + 1', 'R_end not masked'):
        with pytest.raises(AssertionError):
            uec.check_nstep(_impl(nstep_return=_nstep_wrap(kind)), 'cpu', 28, 37, 21, 0.9, 'directed')
    uec.check_nstep(_impl(nstep_return=_nstep_wrap('transposed')), 'cpu', 28, 37, 21, 0.9, 'line')
    for N, E, T in uec.NSTEP_SHAPES[:4]:
        for alpha in (0.9, 1.0):
            with pytest.raises(AssertionError):
                uec.check_nstep(_impl(nstep_return=_nstep_wrap('transposed')), 'cpu', N, E, T, alpha, 'directed')
    with pytest.raises(AssertionError):
        uec.check_nstep(_impl(nstep_return=_nstep_wrap('minus one is one hop')), 'cpu', 3, 5, 13, 1.0, 'directed')


def _sample_variant(side_left=False, no_division=False, last_max=False, counter_n=False):
    """ops_ref.sample_actions with one mistake switched on."""
    def f(pi, out, mode, u=None, seed=0, env_id_base=0, step=0, step_dev=None):
        N, E, A = pi.shape
        if step_dev is not None:
            step = int(step) + int(step_dev.item())
        p = pi.numpy().astype(np.float64).transpose(1, 0, 2)
        if mode == ops_ref.SAMPLE_ARGMAX:
            a = A - 1 - p[..., ::-1].argmax(-1) if last_max else p.argmax(-1)
        else:
            if mode == ops_ref.SAMPLE_UNIFORM:
                uu = u.numpy().astype(np.float64).reshape(E, N)
            elif counter_n:
                agents = np.arange(N, dtype=np.uint64)[None, :]
                w = philox.philox4x32(np.asarray(env_id_base + np.arange(E), dtype=np.uint64)[:, None], agents, step, philox.STREAM_ACTION,
                                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
                w = np.stack(w, axis=-1)
                sel = np.broadcast_to((agents & np.uint64(3)).astype(np.int64), w.shape[:2])
                uu = philox.u01(np.take_along_axis(w, sel[..., None], axis=-1)[..., 0]).astype(np.float64)
            else:
                uu = philox.action_uniform(seed, env_id_base + np.arange(E), N, step).astype(np.float64)
            cdf = np.cumsum(p, axis=-1)
            if not no_division:
                cdf = cdf / cdf[..., -1:]
            a = ((cdf < uu[..., None]) if side_left else (cdf <= uu[..., None])).sum(-1)
            a = np.minimum(a, A - 1)
        out.copy_(torch.from_numpy(a.astype(np.uint8)))
        return out
    return f


def _sample_no_step_dev(pi, out, mode, u=None, seed=0, env_id_base=0, step=0, step_dev=None):
    return ops_ref.sample_actions(pi, out, mode, u=u, seed=seed, env_id_base=env_id_base, step=step)


SAMPLE_MUTANTS = {
    "cdf < u (side='left')": (_sample_variant(side_left=True), (3, 4, 'uniform')),
    'no division by the total': (_sample_variant(no_division=True), (7, 9, 'uniform')),
    'last maximum wins': (_sample_variant(last_max=True), (3, 4, 'argmax')),
    'Philox counter n instead of n >> 2': (_sample_variant(counter_n=True), (3, 4, 'philox')),
    'step_dev ignored': (_sample_no_step_dev, (7, 9, 'philox')),
}


def test_sample_variant_without_a_mistake_passes():
    for N, A in uec.SAMPLE_SHAPES:
        for mode in uec.SAMPLE_MODES:
            uec.check_sample(_impl(sample_actions=_sample_variant()), 'cpu', N, uec.SAMPLE_E, A, mode)


@pytest.mark.parametrize('name', list(SAMPLE_MUTANTS))
def test_sample_mutant_fails(name):
    fn, (N, A, mode) = SAMPLE_MUTANTS[name]
    with pytest.raises(AssertionError):
        uec.check_sample(_impl(sample_actions=fn), 'cpu', N, uec.SAMPLE_E, A, mode)


def test_sample_boundary_rows_alone_catch_the_left_side():
    """Without the rows whose uniform sits exactly on a cumulative boundary, side='left' draws the same actions: the rows are what
    pins it."""
    N, E, A = 28, uec.SAMPLE_E, 37
    rs = np.random.RandomState(1)
    p = rs.dirichlet(np.ones(A), size=(N, E)).astype(np.float32)
    u = rs.random_sample((E, N)).astype(np.float32)
    a, b = torch.zeros(E, N, dtype=torch.uint8), torch.zeros(E, N, dtype=torch.uint8)
    _sample_variant(side_left=True)(torch.from_numpy(p), a, ops_ref.SAMPLE_UNIFORM, u=torch.from_numpy(u))
    ops_ref.sample_actions(torch.from_numpy(p), b, ops_ref.SAMPLE_UNIFORM, u=torch.from_numpy(u))
    assert torch.equal(a, b)


def _epilogue_wrap(kind):
    def f(g, done, ep_sum, ep_sq, ep_len, fin, T_env, h_fw, c_fw, h_bw, c_bw, fp_T, fp_0, fp_uniform, x_T, x_0, done_pre, skip_if=None):
        if kind == 'collision with <=':
            T_env = T_env + 1                                      # len < T_env + 1 == len <= T_env (whole numbers)
        if kind == 'fp_uniform row 0':
            fp_uniform = fp_uniform[:1].expand_as(fp_uniform).contiguous()
        if kind == 'skip_if ignored':
            skip_if = None
        fin2 = None
        if kind == 'no clamp' and not (skip_if is not None and int(skip_if.reshape(-1)[0]) != 0):
            gd = g.double()
            s, q, n = ep_sum + gd.sum(0), ep_sq + (gd * gd).sum(0), ep_len + g.shape[0]
            mean = s / n
            fin2 = fin[2] + ((q / n - mean * mean).sqrt() * done.bool().double()).sum()
        ops_ref.batch_epilogue(g, done, ep_sum, ep_sq, ep_len, fin, T_env, h_fw, c_fw, h_bw, c_bw, fp_T, fp_0, fp_uniform, x_T, x_0, done_pre,
                               skip_if=skip_if)
        if fin2 is not None:
            fin[2] = fin2
    return f


EPILOGUE_MUTANTS = {
    'collision counted with <=': ('collision with <=', False),
    'no clamp on var': ('no clamp', False),
    'fp_uniform row 0 for every agent': ('fp_uniform row 0', False),
    'skip_if ignored': ('skip_if ignored', True),
}


@pytest.mark.parametrize('name', list(EPILOGUE_MUTANTS))
def test_epilogue_mutant_fails(name):
    kind, skip_pattern = EPILOGUE_MUTANTS[name]
    with pytest.raises(AssertionError):
        uec.check_epilogue(_impl(batch_epilogue=_epilogue_wrap(kind)), 'cpu', *uec.EPILOGUE_SHAPES[0], 4, skip_pattern)

"""The opt-in replica minibatches of the PPO epochs on the device: the kernels of csrc/minibatch.hip (permutation, count, gather)
against the restatement of tests/ppo_minibatch_checks.py, bit for bit, and the ABI's refusals; and MODEL_CONFIG ppo_minibatches
through BatchedTrainer, eager and captured."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import ppo_minibatch_checks as mc
from helpers import cacc_config, grid_config

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

SEED = 12 + (77 << 32)          # both words of the Philox key in use


# ------------------------------------------------------------------------------------------------------------------ the kernels
def _device_perm(E, epoch, count, seed=SEED, base=0):
    from deeprl_network_amd import ops
    cnt = torch.tensor([count], dtype=torch.int32, device='cuda')
    keys = torch.full((E,), -1, dtype=torch.int32, device='cuda')
    out = torch.full((E,), -1, dtype=torch.int32, device='cuda')
    ops.minibatch_perm(seed, base, epoch, cnt, keys, out)
    return out.cpu().numpy(), keys.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('E', [1, 2, 63, 64, 65, 77, 1000, 4096])
def test_permutation_equals_the_restatement(E):
    for epoch, count, base in ((2, 0, 0), (3, 0, 0), (2, 41, 0), (5, 7, 3 * E), (2, 2 ** 31 - 1, 10 ** 9)):
        got, keys = _device_perm(E, epoch, count, base=base)
        assert np.array_equal(keys, mc.keys(E, epoch, count, SEED, base)), (epoch, count, base)
        assert np.array_equal(got, mc.perm(E, epoch, count, SEED, base)), (epoch, count, base)
    a, b = _device_perm(E, 2, 5)[0], _device_perm(E, 2, 5)[0]
    assert np.array_equal(a, b) and sorted(a.tolist()) == list(range(E))


def test_count_advance_and_a_draw_that_follows_the_device_word():
    from deeprl_network_amd import ops
    E = 77
    cnt = torch.tensor([6], dtype=torch.int32, device='cuda')
    keys, out = torch.zeros(E, dtype=torch.int32, device='cuda'), torch.zeros(E, dtype=torch.int32, device='cuda')
    ops.minibatch_count_advance(cnt)
    ops.minibatch_perm(SEED, 0, 2, cnt, keys, out)
    assert int(cnt) == 7 and np.array_equal(out.cpu().numpy(), mc.perm(E, 2, 7, SEED))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                     # a replayed graph draws a fresh permutation and counts
        ops.minibatch_perm(SEED, 0, 2, cnt, keys, out)
        ops.minibatch_count_advance(cnt)
    for n in (7, 8, 9):
        g.replay()
        torch.cuda.synchronize()
        assert int(cnt) == n + 1 and np.array_equal(out.cpu().numpy(), mc.perm(E, 2, n, SEED))


INNER = [1, 4, 8, 25, 100, 160, 256]
OUTER = [1, 3, 480]


def _bytes(n, offset, gen):
    """n random bytes on the device whose base address is `offset` past an allocation's (256-byte aligned) start."""
    buf = torch.randint(0, 256, (n + offset,), dtype=torch.uint8, generator=gen, device='cuda')
    return buf[offset:]


@pytest.mark.parametrize('E,Em', [(1, 1), (2, 1), (77, 11), (128, 64), (1000, 500)])
@pytest.mark.parametrize('offset', [0, 4, 1])
def test_gather_equals_fancy_indexing(E, Em, offset):
    """Every (outer, inner) of the specification per (E, Em); offset 4 sends the 16-byte shapes down the 4-byte path, offset 1
    everything down the byte path.  The index holds repeats and is no prefix of anything."""
    from deeprl_network_amd import ops
    gen = torch.Generator(device='cuda').manual_seed(E * 131 + Em + offset)
    idx_d = torch.randint(0, E, (Em,), generator=gen, dtype=torch.int32, device='cuda')
    for outer in OUTER:
        pairs, want = [], []
        for inner in INNER:
            src = _bytes(outer * E * inner, offset, gen).view(outer, E, inner)
            dst = torch.full((outer * Em * inner + offset,), 0xA5, dtype=torch.uint8, device='cuda')[offset:].view(outer, Em, inner)
            pairs.append((dst, src))
            want.append(src[:, idx_d.long()])
        ops.minibatch_gather(pairs, idx_d, outer_of=[outer] * len(pairs))
        torch.cuda.synchronize()
        for (dst, _), w, inner in zip(pairs, want, INNER):
            assert torch.equal(dst, w), (outer, inner)


@pytest.mark.parametrize('n', [1, 16, 17])
def test_gather_of_many_pairs_and_typed_tensors(n):
    """1, 16 and 17 pairs (17: two launches), float and byte tensors of the update's own shapes [T, E, N, F], [N, T * E], [N, E, H]."""
    from deeprl_network_amd import ops
    T, E, N, F, H, Em = 3, 12, 8, 5, 64, 6
    gen = torch.Generator().manual_seed(n)
    idx = torch.from_numpy(mc.perm(E, 2, 0, SEED)[:Em].copy())
    shapes = [((T, E, N, F), (T, Em, N, F), T, torch.float32), ((N, T * E), (N, T * Em), N * T, torch.float32),
              ((N, E, H), (N, Em, H), N, torch.float32), ((T, E, N), (T, Em, N), T, torch.uint8)]
    pairs, outer, want = [], [], []
    for i in range(n):
        s_shape, d_shape, o, dt = shapes[i % len(shapes)]
        src = torch.randint(0, 200, s_shape, generator=gen).to(dt).cuda()
        pairs.append((torch.zeros(d_shape, dtype=dt, device='cuda'), src))
        outer.append(o)
        want.append(mc.gather_rows(src.cpu(), idx.tolist(), o, E).reshape(d_shape))
    ops.minibatch_gather(pairs, idx.cuda(), outer_of=outer)
    torch.cuda.synchronize()
    for (dst, _), w in zip(pairs, want):
        assert torch.equal(dst.cpu(), w)


def test_gather_leaves_the_rows_of_an_index_outside_the_range_untouched():
    from deeprl_network_amd import ops
    E, Em, outer = 9, 6, 11
    idx = torch.tensor([3, -1, 9, 0, 2 ** 31 - 1, 8], dtype=torch.int32)
    for inner in (16, 4, 3):
        src = torch.arange(outer * E * inner, dtype=torch.int32).to(torch.uint8).view(outer, E, inner).cuda()
        dst = torch.full((outer, Em, inner), 0xA5, dtype=torch.uint8, device='cuda')
        ops.minibatch_gather([(dst, src)], idx.cuda(), outer_of=[outer])
        got = dst.cpu()
        for i, e in enumerate(idx.tolist()):
            if 0 <= e < E:
                assert torch.equal(got[:, i], src.cpu()[:, e])
            else:
                assert bool((got[:, i] == 0xA5).all()), (inner, i)


def test_abi_refusals_launch_nothing():
    from deeprl_network_amd import _lib
    lib, ptr, st = _lib.lib, _lib.ptr, _lib.stream
    E, Em, outer, inner = 8, 4, 3, 16
    S = 0x5A
    src = torch.zeros(outer, E, inner, dtype=torch.uint8, device='cuda')
    dst = torch.full((outer, Em, inner), S, dtype=torch.uint8, device='cuda')
    idx = torch.arange(Em, dtype=torch.int32, device='cuda')
    cnt = torch.full((1,), S, dtype=torch.int32, device='cuda')
    keys, out = torch.full((E,), S, dtype=torch.int32, device='cuda'), torch.full((E,), S, dtype=torch.int32, device='cuda')

    def gather(n=1, idx=ptr(idx), Em=Em, E=E, src=ptr(src), dst=ptr(dst), outer=outer, inner=inner, desc=True):
        arr = (_lib.GatherDesc * 17)(*[_lib.GatherDesc(src, dst, outer, inner) for _ in range(17)])
        return lib.nmarl_minibatch_gather(n, arr if desc else None, idx, Em, E, st())

    for kw in (dict(n=0), dict(n=-1), dict(n=17), dict(Em=0), dict(Em=-3), dict(E=0), dict(E=-1), dict(idx=None), dict(desc=False),
               dict(src=None), dict(dst=None), dict(outer=0), dict(outer=-1), dict(inner=0), dict(inner=-16)):
        assert gather(**kw) == -1, kw

    def perm(E=E, cnt=ptr(cnt), keys=ptr(keys), out=ptr(out)):
        return lib.nmarl_minibatch_perm(E, SEED, 0, 2, cnt, keys, out, st())

    for kw in (dict(E=0), dict(E=-1), dict(E=65537), dict(cnt=None), dict(keys=None), dict(out=None)):
        assert perm(**kw) == -1, kw
    assert lib.nmarl_minibatch_count_advance(None, st()) == -1
    torch.cuda.synchronize()
    for t in (dst, cnt, keys, out):
        assert bool((t == S).all())
    cnt.zero_()
    assert gather() == 0 and perm() == 0 and lib.nmarl_minibatch_count_advance(ptr(cnt), st()) == 0
    torch.cuda.synchronize()
    assert not bool((dst == S).any()) and int(cnt) == 1 and sorted(out.tolist()) == list(range(E))
    big = torch.zeros(65536, dtype=torch.int32, device='cuda')                     # the largest E is accepted
    assert lib.nmarl_minibatch_perm(65536, SEED, 0, 2, ptr(cnt), ptr(big), ptr(torch.zeros_like(big)), st()) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ the engine
CONFIGS = [('ia2c_fp', 'cacc', 8), ('ia2c_fp', 'cacc', 12), ('ia2c', 'cacc', 8), ('ia2c', 'cacc', 12), ('ma2c_cu', 'cacc', 8),
           ('ma2c_cu', 'cacc', 12), ('ia2c_fp', 'grid', 4)]
IDS = ['%s-%s-E%d' % c for c in CONFIGS]
# the weight and gradient tolerances of tests/test_gpu_ppo.py (native == restated)
W_TOL = dict(rtol=1e-3, atol=1e-5)
G_RTOL, G_ATOL_SCALE = 1e-4, 2e-6
MODEL_SEED = 12


def _build(cfg, use_graph, extra=None, **trainer_kw):
    from deeprl_network_amd.envs import make_batch_env
    from deeprl_network_amd.main import init_agent
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    agent, scen, E = cfg
    if scen == 'cacc':                      # the ini's n_step: 60 on CACC, 120 on the grid
        cp = cacc_config(agent=agent, scenario='catchup', coop_gamma=-1, reward_norm=800.0 if agent.startswith('ia2c') else 5000.0)
    else:
        cp = grid_config(agent=agent)
    for k, v in (extra or {}).items():
        cp['MODEL_CONFIG'][k] = v
    env = make_batch_env(cp['ENV_CONFIG'], num_envs=E)
    np.random.seed(12)
    model = init_agent(env, cp['MODEL_CONFIG'], 10 ** 9, MODEL_SEED, num_envs=E)
    return env, model, BatchedTrainer(env, model, Counter(10 ** 12, 10 ** 12, 10 ** 12), use_graph=use_graph, **trainer_kw)


def _slots(model):
    ps = model.policy.params
    return [ps.adam_m, ps.adam_v, ps.adam_t] if model.optimizer == 'adam' else [ps.ms]


@functools.lru_cache(maxsize=None)
def _run(cfg, use_graph, batches, extra=(), identity=False):
    """One fresh run -> what the tests compare, on the host.  Cached: the tests share their runs and leave them unchanged."""
    import graph_nodes as G
    if identity:
        os.environ['NMARL_TEST_MINIBATCH_IDENTITY'] = '1'
    try:
        env, model, tr = _build(cfg, use_graph, extra=dict(extra), **(dict(keep_graphs=True) if use_graph else {}))
    finally:
        os.environ.pop('NMARL_TEST_MINIBATCH_IDENTITY', None)
    perms, adam_t = [], []
    for _ in range(batches):
        tr.run_batch()
        if hasattr(model, 'mb_perm'):
            perms.append(model.mb_perm.cpu().numpy().copy())
        if model.optimizer == 'adam':
            adam_t.append(int(model.policy.params.adam_t))
    torch.cuda.synchronize()
    r = dict(flat=model.policy.params.flat.detach().cpu().clone(), slots=[s.detach().cpu().clone() for s in _slots(model)],
             stats=model.ppo_stats.cpu().clone() if hasattr(model, 'ppo_stats') else None, perms=perms, adam_t=adam_t,
             vstats=model.ppo_vclip_stats.cpu().clone() if hasattr(model, 'ppo_vclip_stats') else None,
             steps_done=model.ppo_steps_done, count=int(model.mb_count) if hasattr(model, 'mb_count') else None,
             env_id_base=int(env.env_id_base), census=None, upd_keys=None, error=tr.update_capture_error)
    if use_graph:
        assert tr._upd is not None and tr.update_capture_error is None and tr._upd['apply'] is None
        r['census'] = G.census(tr._upd['grads'])
        r['upd_keys'] = sorted(tr._upd)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        model.save(d + '/', 1)
        r['ckpt_keys'] = sorted(torch.load(d + '/checkpoint-1.pt', weights_only=True))
    return r


def _same(a, b, what=('flat', 'slots', 'stats')):
    for k in what:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        assert len(xs) == len(ys)
        for x, y in zip(xs, ys):
            assert torch.equal(x, y), k


@pytest.mark.parametrize('cfg', CONFIGS, ids=IDS)
def test_absent_is_one_is_the_model_without_the_key(cfg):
    base = _run(cfg, True, 2, (('ppo_epochs', '2'),))
    one = _run(cfg, True, 2, (('ppo_epochs', '2'), ('ppo_minibatches', '1')))
    _same(base, one)
    assert base['ckpt_keys'] == one['ckpt_keys'] and 'ppo_minibatch_count' not in one['ckpt_keys']
    assert base['census'] == one['census'] and set(one['census']) == {'kernel'} and base['upd_keys'] == one['upd_keys']
    assert one['count'] is None and one['perms'] == []
    plain, plain1 = _run(cfg, True, 2), _run(cfg, True, 2, (('ppo_minibatches', '1'),))       # without ppo_epochs as well
    _same(plain, plain1, what=('flat', 'slots'))
    assert plain['census'] == plain1['census'] and plain['ckpt_keys'] == plain1['ckpt_keys']


@pytest.mark.parametrize('cfg', CONFIGS, ids=IDS)
def test_the_gather_with_the_identity_permutation_is_lossless(cfg):
    base = _run(cfg, True, 2, (('ppo_epochs', '2'),))
    ident = _run(cfg, True, 2, (('ppo_epochs', '2'),), identity=True)
    _same(base, ident)
    assert sum(ident['census'].values()) > sum(base['census'].values()) and set(ident['census']) == {'kernel'}     # it did gather


def _spy(model):
    """The flat gradient and the weights every update_apply of the model starts from."""
    seen = []
    inner = model.update_apply

    def apply(lr, rotate=True, lr_dev=None):
        seen.append((model.policy.params.grad.clone(), model.policy.params.flat.detach().clone()))
        return inner(lr, rotate=rotate, lr_dev=lr_dev)
    model.update_apply = apply
    return seen


def _literal_update(tr, K, M, at_weights=None):
    """'PPO with replica minibatches', written out on index-selected tensors with the project's torch loss chain (_loss_torch) and
    autograd, on a trainer whose rollout is done: -> the flat gradient of every step.  at_weights: per step the weights another run
    took its gradient at -- the step's gradient is ALSO formed there (returned in place of the own one); the trajectory stays the
    literal run's own."""
    m = tr.model
    N, T, E, A = m.n_agent, m.n_step, m.E, m.n_a
    p, ps = m.policy, m.policy.params
    Em = E // M
    m.load_rewards(tr.buf_rraw)
    lr = m.update_begin()
    m.update_grads(tr.R_end)
    grads = [ps.grad.clone()]
    m.update_reduce()
    m.update_apply(lr, rotate=False)
    adv_all, R_all = m._loss_adv().view(N, T, E), m.R.view(N, T, E)
    lo_all = m.ppo_logp_old.view(N, T, E)
    vo_all = m.ppo_v_old.view(N, T, E) if m.ppo_vclip is not None else None
    count = 0

    def grad_of_group(idx):
        ps.begin_backward()
        X = m.buf_x[:T].index_select(1, idx)
        FP = m.buf_fp[:T].index_select(2, idx).permute(1, 0, 2, 3).reshape(N, T * Em, A)
        Hs = p.unroll(X, FP, m.buf_done_pre.index_select(1, idx), m.h_bw.index_select(1, idx), m.c_bw.index_select(1, idx),
                      masked_steps=m.masked_steps)
        action = m.buf_act.index_select(1, idx).reshape(T * Em, N)
        logits, v = p.heads(Hs, action)
        sel = lambda z: None if z is None else z.index_select(2, idx).reshape(N, T * Em)      # noqa: E731
        per_agent, _ = m._loss_torch(logits, v, action, sel(adv_all), sel(R_all), sel(lo_all), sel(vo_all))
        per_agent.sum().backward()
        m._end_grads()
        return ps.grad.clone()

    step = 0
    for k in range(2, K + 1):
        pi = torch.from_numpy(mc.perm(E, k, count, MODEL_SEED, int(tr.env.env_id_base))).long().cuda()
        for j in range(M):
            idx = pi[j * Em:(j + 1) * Em]
            step += 1
            if at_weights is not None:
                own = ps.flat.detach().clone()
                with torch.no_grad():
                    ps.flat.copy_(at_weights[step])
                grads.append(grad_of_group(idx))
                with torch.no_grad():
                    ps.flat.copy_(own)
            g = grad_of_group(idx)
            if at_weights is None:
                grads.append(g)
            m.update_reduce()
            m.update_apply(lr, rotate=False)
    m.update_end()
    return grads


@pytest.mark.parametrize('cfg', CONFIGS, ids=IDS)
def test_step_gradients_and_weights_equal_the_literal_update(cfg):
    """K = 2, M = 2, one update: every step's flat gradient against autograd over _loss_torch on index-selected tensors, formed at
    the weights the native step started from; the weights after the update against the literal run's own trajectory."""
    K, M = 2, 2
    extra = dict(ppo_epochs=str(K), ppo_minibatches=str(M))
    env, model, tr = _build(cfg, False, extra=extra)
    seen = _spy(model)
    tr.run_batch()
    torch.cuda.synchronize()
    assert len(seen) == 1 + (K - 1) * M
    w_native = model.policy.params.flat.detach().clone()
    perm_native = model.mb_perm.cpu().numpy().copy()
    del env, model, tr
    env, twin, tr2 = _build(cfg, False, extra=dict(ppo_epochs=str(K)))           # (no minibatch key: the loop is the test's own)
    tr2.rollout()
    grads = _literal_update(tr2, K, M, at_weights=[w for _, w in seen])
    torch.cuda.synchronize()
    assert np.array_equal(perm_native, mc.perm(cfg[2], K, 0, MODEL_SEED, 0))
    assert torch.equal(seen[0][0], grads[0]) and float(grads[0].abs().max()) > 0          # epoch 1 is the A2C step of before
    for s in range(1, len(seen)):
        g, g0 = seen[s][0], grads[s]
        err = float((g - g0).abs().max())
        print('step %d: max |g| %.3e, max |g - literal| %.3e' % (s, float(g0.abs().max()), err))
        torch.testing.assert_close(g, g0, rtol=G_RTOL, atol=G_ATOL_SCALE * float(g0.abs().max()))
    assert not torch.equal(seen[1][0], seen[2][0])
    torch.testing.assert_close(w_native, twin.policy.params.flat.detach(), **W_TOL)


@pytest.mark.parametrize('cfg', CONFIGS, ids=IDS)
def test_adam_counts_every_step(cfg):
    K, M = 3, 2
    r = _run(cfg, False, 2, (('optimizer', 'adam'), ('ppo_epochs', str(K)), ('ppo_minibatches', str(M))))
    assert r['adam_t'] == [1 + (K - 1) * M, 2 * (1 + (K - 1) * M)] and r['count'] == 2


@pytest.mark.parametrize('cfg', CONFIGS, ids=IDS)
def test_zero_lr_leaves_the_weights_and_the_groups_average_to_the_batch(cfg):
    """lr_init = 0: the optimiser moves nothing through 1 + (K - 1) M steps -- the weights keep their bits, every ratio is 1
    (clip_frac 0, approx_kl in the 1e-6 class of two forward paths) and, groups of equal size that partition the replicas, the mean of
    an epoch's M group gradients is the full-batch gradient within the gradient tolerance.  ConseNet's consensus pass behind every
    step moves the weights whatever the lr: there the weights have the bits of the run without minibatches that makes as many steps
    (ppo_epochs = 1 + (K - 1) M), which holds for the other nets too.  Weights and optimiser slots have the bits of the captured twin's."""
    K, M = 2, 2
    consensus = cfg[0] == 'ma2c_cu'
    extra = dict(ppo_epochs=str(K), ppo_minibatches=str(M), lr_init='0')
    env, model, tr = _build(cfg, False, extra=extra)
    w0 = model.policy.params.flat.detach().clone()
    seen = _spy(model)
    for _ in range(2):
        tr.run_batch()
    torch.cuda.synchronize()
    flat = model.policy.params.flat.detach().cpu().clone()
    assert len(seen) == 6 and torch.equal(flat, w0.cpu()) != consensus
    same_steps = _run(cfg, False, 2, (('lr_init', '0'), ('ppo_epochs', str(1 + (K - 1) * M))))
    assert torch.equal(flat, same_steps['flat'])
    if not consensus:
        st = model.ppo_stats
        print('max approx_kl at lr 0: %.3e' % float(st[1:, :, 0].max()))
        assert not st[:, :, 1].any() and float(st[1:, :, 0].max()) < 1e-6 and bool((st[1:, :, 0] >= 0).all())
        g1, mean = seen[0][0], (seen[1][0] + seen[2][0]) / 2
        torch.testing.assert_close(mean, g1, rtol=G_RTOL, atol=G_ATOL_SCALE * float(g1.abs().max()))
    slots = [s.detach().cpu().clone() for s in _slots(model)]
    del env, model, tr
    cap = _run(cfg, True, 2, tuple(sorted(extra.items())))          # (two batches: the second update is the replayed one)
    assert torch.equal(cap['flat'], flat) and all(torch.equal(a, b) for a, b in zip(cap['slots'], slots))


@pytest.mark.parametrize('cfg', CONFIGS, ids=IDS)
def test_captured_equals_eager_and_two_runs_are_identical(cfg):
    K, M = 3, 2
    extra = (('ppo_epochs', str(K)), ('ppo_minibatches', str(M)))
    cap, eager = _run(cfg, True, 3, extra), _run(cfg, False, 3, extra)
    _same(cap, eager)
    assert set(cap['census']) == {'kernel'} and cap['census']['kernel'] > 0, cap['census']
    assert cap['upd_keys'] == ['apply', 'chain', 'epilogue_inside', 'grads']
    for r in (cap, eager):
        assert r['count'] == 3 and bool(torch.isfinite(r['flat']).all())
        for b, p in enumerate(r['perms']):         # what stands in mb_perm behind update b is the last epoch's draw under count b
            assert np.array_equal(p, mc.perm(cfg[2], K, b, MODEL_SEED, r['env_id_base']))
        st = r['stats']
        assert not st[0].any() and bool(torch.isfinite(st).all()) and bool((st[1:, :, 0] >= 0).all()) and float(st[1:, :, 0].max()) > 0
        assert bool((st[1:, :, 1] >= 0).all()) and bool((st[1:, :, 1] <= 1).all())
    _run.cache_clear()
    again = _run(cfg, True, 3, extra)
    _same(cap, again)
    assert all(np.array_equal(a, b) for a, b in zip(cap['perms'], again['perms']))
    one = _run(cfg, True, 3, (('ppo_epochs', str(K)),))
    assert float((one['flat'] - cap['flat']).abs().max()) > 1e-5               # the groups' steps are not the full-batch steps


@pytest.mark.parametrize('cfg', CONFIGS, ids=IDS)
def test_save_load_continues_the_permutations(cfg, tmp_path):
    K, M = 2, 2
    extra = dict(ppo_epochs=str(K), ppo_minibatches=str(M))
    straight = _run(cfg, False, 3, tuple(sorted(extra.items())))
    env, model, tr = _build(cfg, False, extra=extra)
    for _ in range(2):
        tr.run_batch()
    d = str(tmp_path) + '/'
    model.save(d, 5)
    assert int(torch.load(d + 'checkpoint-5.pt', weights_only=True)['ppo_minibatch_count']) == 2
    del env, model, tr
    env, model, tr = _build(cfg, False, extra=extra)
    assert model.load(d) and int(model.mb_count) == 2
    tr.run_batch()
    torch.cuda.synchronize()
    assert np.array_equal(model.mb_perm.cpu().numpy(), straight['perms'][2]) and int(model.mb_count) == 3
    assert np.array_equal(straight['perms'][2], mc.perm(cfg[2], K, 2, MODEL_SEED, 0))


@pytest.mark.parametrize('cfg', CONFIGS, ids=IDS)
def test_kl_stop_decides_per_step(cfg):
    """kappa = 1e30 is the run without the key; a kappa between two observed step KLs stops the update at that step: the weights are
    those the unstopped update had behind its last applied step, bit for bit, and ppo_steps_done says so."""
    K, M = 3, 2
    keys = (('ppo_epochs', str(K)), ('ppo_minibatches', str(M)))
    off, huge = _run(cfg, False, 1, keys), _run(cfg, False, 1, keys + (('ppo_target_kl', '1e30'),))
    _same(off, huge)
    assert huge['steps_done'] == 1 + (K - 1) * M and off['steps_done'] is None
    env, model, tr = _build(cfg, False, extra=dict(keys + (('ppo_target_kl', '1e30'),)))
    seen, kls = _spy(model), []
    inner = model._end_grads
    model._end_grads = lambda kl_terms=None: (kls.append(None if kl_terms is None else float(kl_terms[:, 3].sum()) / model.n_agent),
                                              inner(kl_terms=kl_terms))[1]
    tr.run_batch()
    torch.cuda.synchronize()
    kls = kls[1:]
    after = [w for _, w in seen[1:]] + [model.policy.params.flat.detach().clone()]        # after[s]: the weights behind 1 + s steps
    print('step KLs:', kls)
    assert len(kls) == (K - 1) * M and all(k is not None and k >= 0 for k in kls)
    # the first step whose KL exceeds every one before it (kappa halfway between the two); if the first step's is the largest, it
    # stops the update itself (kappa halfway down to the next largest)
    s = next((i for i in range(1, len(kls)) if kls[i] > max(kls[:i])), 0)
    kappa = 0.5 * (max(kls[:s]) + kls[s]) if s else 0.5 * (kls[0] + max(kls[1:]))
    assert 0 < kappa < kls[s] and all(k < kappa for k in kls[:s])
    del env, model, tr
    env, model, tr = _build(cfg, False, extra=dict(keys + (('ppo_target_kl', repr(kappa)),)))
    tr.run_batch()
    torch.cuda.synchronize()
    assert model.ppo_steps_done == 1 + s and model.ppo_epochs_done == 1 + s // M
    assert torch.equal(model.policy.params.flat, after[s])


@pytest.mark.parametrize('cfg', CONFIGS, ids=IDS)
@pytest.mark.parametrize('key,value', [('gae_lambda', '0.9'), ('adv_norm', 'agent'), ('reward_scale', 'return'), ('optimizer', 'adam'),
                                       ('ppo_vclip', '0.2')])
def test_composition_with_the_other_opt_in_keys(cfg, key, value):
    extra = tuple(sorted(dict([('ppo_epochs', '2'), ('ppo_minibatches', '2'), (key, value)]).items()))
    cap, eager = _run(cfg, True, 2, extra), _run(cfg, False, 2, extra)       # (two batches: the second update is the replayed one)
    _same(cap, eager)
    assert bool(torch.isfinite(cap['flat']).all()) and float(cap['stats'][1, :, 0].max()) > 0
    if key == 'ppo_vclip':
        assert torch.equal(cap['vstats'], eager['vstats']) and bool((cap['vstats'] >= 0).all()) and bool((cap['vstats'] <= 1).all())


def test_refusals_on_the_device_path():
    for extra, match in ((dict(ppo_epochs='2', ppo_minibatches='3'), 'does not divide'), (dict(ppo_minibatches='2'), 'ppo_epochs = 1'),
                         (dict(ppo_epochs='2', ppo_minibatches='16'), 'does not divide')):
        with pytest.raises(ValueError, match=match):
            _build(('ia2c_fp', 'cacc', 8), False, extra=extra)
    with pytest.raises(ValueError, match='ppo_epochs'):
        _build(('ma2c_nc', 'cacc', 8), False, extra=dict(ppo_epochs='2', ppo_minibatches='2'))

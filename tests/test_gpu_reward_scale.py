"""The opt-in running return-based reward scaling on the device (csrc/a2c.hip: reward_scale_scan_kernel, reward_scale_merge_kernel,
reward_scale_apply_kernel, nmarl_reward_scale) and in the engine: three successive calls against the float64 restatement of
tests/reward_scale_checks.py at the smallest shapes where each piece can go wrong (one stream, the lane, wave and block edges, one
stream count past 256 x the chunk cap, the per-agent layout with a ragged block), every done pattern and data class, sentinels behind
every buffer, determinism, graph capture, the ABI's refusals, and MODEL_CONFIG reward_scale through BatchedTrainer (eager, captured,
checkpointed) and the one-replica path."""
import configparser
import os
import sys

import numpy as np
import pytest
import torch

import reward_scale_checks as rc
from helpers import GOLDEN, cacc_config, drive_scripted, load_npz

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
F32, F64 = torch.float32, torch.float64
PAD = 37


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64 if t.dtype == F64 else torch.int32)


def _sentinel_tail(t, n, what):
    assert bool((t[n:] == rc.SENTINEL).all()), '%s: the words behind %d were overwritten' % (what, n)


class Device:
    """The implementation under test with the interface of rc.Restatement: through the C-ABI (raw pointers into buffers that are PAD
    words longer than needed and pre-filled with a sentinel) or through ops.reward_scale (views of such buffers)."""

    def __init__(self, E, N, gamma, eps, clip, via='abi'):
        from deeprl_network_amd import ops
        self.E, self.N, self.S = E, N, E * max(N, 1)
        self.gamma, self.eps, self.clip, self.via = gamma, eps, clip, via
        self.C = ops.reward_scale_chunks(self.S)
        self.carry = torch.full((self.S + PAD,), rc.SENTINEL, dtype=F64, device='cuda')
        self.carry[:self.S] = 0
        self.state = torch.zeros(ops.REWARD_SCALE_STATE, dtype=F64, device='cuda')
        self.partial = torch.full((self.C * 4 + PAD,), rc.SENTINEL, dtype=F64, device='cuda')
        self.out = None

    def call(self, r, d):
        from deeprl_network_amd import _lib, ops
        T, S, E, N = r.shape[0], self.S, self.E, self.N
        r_dev = torch.from_numpy(np.ascontiguousarray(r)).cuda().view((T, E, N) if N else (T, E))
        d_dev = torch.from_numpy(np.ascontiguousarray(d)).cuda()
        self.out = out = torch.full((T * S + PAD,), rc.SENTINEL, dtype=F32, device='cuda')
        if self.via == 'abi':
            rcode = _lib.lib.nmarl_reward_scale(E, N, T, _lib.ptr(r_dev), _lib.ptr(d_dev), self.gamma, self.eps, self.clip,
                                                _lib.ptr(self.carry), _lib.ptr(self.state), _lib.ptr(self.partial), _lib.ptr(out),
                                                _lib.stream())
            assert rcode == 0
        else:
            ops.reward_scale(r_dev, d_dev, self.gamma, self.eps, self.clip, self.carry[:S], self.state, self.partial[:self.C * 4],
                             out[:T * S].view(r_dev.shape))
        torch.cuda.synchronize()
        assert torch.equal(r_dev.cpu().view(T, S), torch.from_numpy(r)), 'r_raw changed'
        _sentinel_tail(out, T * S, 'r_out')
        _sentinel_tail(self.carry, S, 'carry')
        _sentinel_tail(self.partial, self.C * 4, 'partial')
        st = self.state.cpu().numpy()
        return dict(r_out=out[:T * S].cpu().numpy().reshape(T, S), carry=self.carry[:S].cpu().numpy(), n=st[0], mean=st[5], sigma=st[6])

    def words(self):
        return [_bits(self.out), _bits(self.carry), _bits(self.state), _bits(self.partial)]


def _cap_streams():
    from deeprl_network_amd import ops
    cap = ops.reward_scale_chunks(10 ** 9)
    assert ops.reward_scale_chunks(256 * cap) == cap == ops.reward_scale_chunks(256 * cap + 1)
    return 256 * cap + 1                  # one stream past what one lane per stream covers: the grid-stride order is exercised


# (E, N, T): N = 0 the global reward [T,E], N >= 1 per-agent rewards [T,E,N]; S = E max(N, 1)
EDGES = [(1, 0, 1), (1, 2, 3),
         (63, 0, 2), (64, 0, 2), (65, 0, 2), (255, 0, 2), (256, 0, 2), (257, 0, 2),
         (21, 3, 2), (16, 4, 2), (13, 5, 2), (51, 5, 2), (64, 4, 2), (257, 1, 2),
         (7, 25, 120), (175, 0, 120)]


# ------------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize('pattern', rc.DONES)
@pytest.mark.parametrize('kind', rc.KINDS)
@pytest.mark.parametrize('E,N,T', EDGES)
def test_three_calls_equal_the_restatement(E, N, T, kind, pattern):
    rc.run_case(lambda *a: Device(*a), E, N, T, kind, pattern)


@pytest.mark.parametrize('pattern', ['none', 'random'])
@pytest.mark.parametrize('kind', ['plain', 'offset'])
@pytest.mark.parametrize('per_agent', [False, True])
def test_streams_past_the_chunk_cap(per_agent, kind, pattern):
    S = _cap_streams()
    if per_agent:
        assert S % 3 == 0
        rc.run_case(lambda *a: Device(*a), S // 3, 3, 2, kind, pattern)
    else:
        rc.run_case(lambda *a: Device(*a), S, 0, 2, kind, pattern)


@pytest.mark.parametrize('kind', ['plain', 'const', 'offset'])
@pytest.mark.parametrize('E,N,T', [(1, 2, 3), (65, 0, 2), (7, 25, 120)])
def test_clamped_outputs_are_the_clip_exactly(E, N, T, kind):
    clip = {'plain': 0.7, 'const': 0.25, 'offset': 1.5}[kind]
    rc.run_case(lambda *a: Device(*a), E, N, T, kind, 'random', clip=clip)


@pytest.mark.parametrize('E,N,T', [(1, 0, 1), (13, 5, 2), (7, 25, 120)])
def test_through_ops_with_another_gamma_and_epsilon(E, N, T):
    for gamma, eps in ((0.0, 0.0), (1.0, 1e-3), (0.9, 1e-8)):
        rc.run_case(lambda *a: Device(*a, via='ops'), E, N, T, 'plain', 'random', eps=eps, gamma=gamma, clip=1.0)


@pytest.mark.parametrize('E,N,T', [(7, 25, 120), (257, 0, 2), (1, 0, 1)])
def test_two_runs_from_the_same_state_give_the_same_bits(E, N, T):
    S = E * max(N, 1)
    a, b = Device(E, N, rc.GAMMA, rc.EPS, 0.5), Device(E, N, rc.GAMMA, rc.EPS, 0.5)
    for k in range(3):
        r, d = rc.rewards(T, S, 'plain', k), rc.dones(T, E, 'random', k)
        a.call(r, d)
        b.call(r, d)
        for x, y in zip(a.words(), b.words()):
            assert torch.equal(x, y), 'call %d: two runs differ' % k


def test_one_captured_call_replayed_equals_three_eager_calls():
    import graph_nodes as G
    from deeprl_network_amd import ops
    E, N, T = 7, 25, 12
    S = E * N
    eager = Device(E, N, rc.GAMMA, rc.EPS, 0.5, via='ops')
    r_st, d_st = torch.zeros(T, E, N, device='cuda'), torch.zeros(T, E, dtype=torch.uint8, device='cuda')
    out = torch.full((T, E, N), rc.SENTINEL, device='cuda')
    carry, state = torch.zeros(S, dtype=F64, device='cuda'), torch.zeros(ops.REWARD_SCALE_STATE, dtype=F64, device='cuda')
    partial = torch.full((ops.reward_scale_chunks(S), 4), rc.SENTINEL, dtype=F64, device='cuda')
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        ops.reward_scale(r_st, d_st, rc.GAMMA, rc.EPS, 0.5, carry, state, partial, out)
    c = G.census(g)
    assert set(c) == {'kernel'} and c['kernel'] == 3, c
    torch.cuda.synchronize()
    assert not state.any() and not carry.any() and bool((out == rc.SENTINEL).all())         # (capturing ran nothing)
    for k in range(3):
        r, d = rc.rewards(T, S, 'plain', k), rc.dones(T, E, 'random', k)
        eager.call(r, d)
        r_st.copy_(torch.from_numpy(r).view(T, E, N))
        d_st.copy_(torch.from_numpy(d))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out).view(-1), _bits(eager.out[:T * S])), 'replay %d: r_out' % k
        assert torch.equal(_bits(carry), _bits(eager.carry[:S])) and torch.equal(_bits(state), _bits(eager.state))


def test_abi_refusals_write_nothing():
    """A null required pointer, T < 1, E < 1, a negative or NaN eps, gamma outside [0, 1] or NaN, N outside 0..64, a NaN clip:
    NMARL_EINVAL, and r_out, carry, state and partial keep their bits."""
    from deeprl_network_amd import _lib
    lib, ptr = _lib.lib, _lib.ptr
    E, N, T = 5, 3, 4
    S = E * N
    r = torch.from_numpy(rc.rewards(T, S, 'plain', 0)).cuda()
    d = torch.zeros(T, E, dtype=torch.uint8, device='cuda')
    out = torch.full((T * S,), rc.SENTINEL, device='cuda')
    carry, state = (torch.full((n,), rc.SENTINEL, dtype=F64, device='cuda') for n in (S, 8))
    partial = torch.full((4 * lib.nmarl_reward_scale_chunks(S),), rc.SENTINEL, dtype=F64, device='cuda')
    pr, pd, pc, ps, pp, po = ptr(r), ptr(d), ptr(carry), ptr(state), ptr(partial), ptr(out)
    nan = float('nan')
    good = dict(E=E, N=N, T=T, r=pr, d=pd, gamma=0.99, eps=1e-8, clip=0.0, carry=pc, state=ps, partial=pp, out=po)
    bad = {'null r_raw': dict(r=None), 'null done_post': dict(d=None), 'null carry': dict(carry=None), 'null state': dict(state=None),
           'null partial': dict(partial=None), 'null r_out': dict(out=None), 'T 0': dict(T=0), 'T -1': dict(T=-1), 'E 0': dict(E=0),
           'E -1': dict(E=-1), 'eps -1': dict(eps=-1.0), 'eps NaN': dict(eps=nan), 'gamma -0.1': dict(gamma=-0.1),
           'gamma 1.01': dict(gamma=1.01), 'gamma NaN': dict(gamma=nan), 'N -1': dict(N=-1), 'N 65': dict(N=65), 'clip NaN': dict(clip=nan)}
    for name, change in bad.items():
        a = dict(good, **change)
        assert lib.nmarl_reward_scale(*a.values(), _lib.stream()) == -1, name            # NMARL_EINVAL
    torch.cuda.synchronize()
    for t in (out, carry, state, partial):
        assert bool((t == rc.SENTINEL).all())


def test_chunk_count_is_capped():
    from deeprl_network_amd import _lib
    f = _lib.lib.nmarl_reward_scale_chunks
    assert [f(s) for s in (-5, 0, 1, 256, 257, 131072, 131073, 2 ** 40)] == [1, 1, 1, 1, 2, 512, 512, 512]


# ------------------------------------------------------------------------------------------------------------------ the engine
E_ENGINE = 16
ENGINE_INIS = ['config_ia2c_fp_catchup.ini', 'config_ma2c_nc_catchup.ini']


def _build(ini, use_graph, reward_scale, coop_gamma=None, E=E_ENGINE, **trainer_kw):
    from deeprl_network_amd.envs import make_batch_env
    from deeprl_network_amd.main import init_agent
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    cp = configparser.ConfigParser()
    assert cp.read(os.path.join(ROOT, 'config', ini))
    if reward_scale is not None:
        cp['MODEL_CONFIG']['reward_scale'] = reward_scale
    if coop_gamma is not None:
        cp['ENV_CONFIG']['coop_gamma'] = str(coop_gamma)
    env = make_batch_env(cp['ENV_CONFIG'], num_envs=E)
    np.random.seed(12)
    model = init_agent(env, cp['MODEL_CONFIG'], 10 ** 9, 12, num_envs=E)
    return env, model, BatchedTrainer(env, model, Counter(10 ** 12, 10 ** 12, 10 ** 12), use_graph=use_graph, **trainer_kw)


def _ref_of(model):
    N = model.n_agent if model.buf_r.dim() == 3 else 0
    return rc.Restatement(model.E, N, model.gamma, model.reward_scale_epsilon, max(model.reward_clip, 0.0))


def _assert_batch(model, tr, ref, what):
    """model.buf_r, carry and moments against the restatement fed with this batch's raw rewards and done flags."""
    T = model.n_step
    r = tr.buf_rraw.cpu().numpy().reshape(T, -1)
    exp = ref.call(r, model.buf_done_post.cpu().numpy())
    st = model.rs_state.cpu().numpy()
    got = dict(r_out=model.buf_r.cpu().numpy().reshape(T, -1), carry=model.rs_carry.cpu().numpy(), n=st[0], mean=st[5], sigma=st[6])
    rc.assert_call(got, r, exp, model.reward_scale_epsilon, max(model.reward_clip, 0.0), what)
    assert float(np.abs(r).max()) > 0 and exp['sigma'] > 0
    assert model.reward_scale_std == st[6]


@pytest.mark.parametrize('ini,coop_gamma', [(ENGINE_INIS[0], None), (ENGINE_INIS[1], None), (ENGINE_INIS[1], 0.9)])
def test_buf_r_is_the_restatement_of_the_batchs_raw_rewards(ini, coop_gamma):
    """Three batches with the key on: after each, buf_r is raw / (running std of the discounted return + eps) -- not raw /
    reward_norm.  (Without the feature the key is ignored and buf_r is raw / reward_norm: this test fails.)"""
    env, model, tr = _build(ini, True, 'return', coop_gamma)
    assert model.reward_scale == 'return' and tuple(model.rs_carry.shape) == (model.buf_r[0].numel(),)
    assert (model.buf_r.dim() == 3) == (coop_gamma is not None)
    ref = _ref_of(model)
    for k in range(3):
        tr.run_batch()
        torch.cuda.synchronize()
        _assert_batch(model, tr, ref, '%s batch %d' % (ini, k))
        assert not torch.equal(model.buf_r, (tr.buf_rraw / model.reward_norm))
    assert tr.handoff_fallbacks == 0 and torch.isfinite(model.policy.params.flat).all()


@pytest.mark.parametrize('ini', ENGINE_INIS)
def test_captured_update_equals_eager_with_reward_scale(ini):
    import graph_nodes as G
    runs = []
    for use_graph in (True, False):
        env, model, tr = _build(ini, use_graph, 'return', **(dict(keep_graphs=True) if use_graph else {}))
        w0 = model.policy.params.flat.clone()
        for _ in range(3):
            tr.run_batch()
        torch.cuda.synchronize()
        assert tr.handoff_fallbacks == 0
        if use_graph:
            assert tr._upd is not None and tr.update_capture_error is None
            c = G.census(tr._upd['grads'])
            assert c.get('kernel', 0) > 0 and set(c) == {'kernel'}, c
        runs.append((model.policy.params.flat.clone(), model.buf_r.clone(), model.rs_carry.clone(), model.rs_state.clone()))
        assert torch.isfinite(runs[-1][0]).all() and not torch.equal(runs[-1][0], w0)
        del env, model, tr
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b)), 'captured update with reward_scale differs from the eager one'


@pytest.mark.parametrize('ini', ENGINE_INIS)
def test_key_absent_is_the_untouched_default_path(ini, monkeypatch):
    """Key absent and an explicit `none`: no call, none of the new tensors, buf_r = raw / reward_norm clamped, and update graphs with
    the same nodes; `return` adds three kernel nodes in place of the division (reward_clip is off in these inis)."""
    import graph_nodes as G
    from deeprl_network_amd import ops
    n_calls = []
    inner = ops.reward_scale
    monkeypatch.setattr(ops, 'reward_scale', lambda *a, **kw: n_calls.append(1) or inner(*a, **kw))
    runs, nodes = [], []
    for value in (None, 'none', 'return'):
        env, model, tr = _build(ini, True, value, keep_graphs=True)
        n_env = len(env.state_tensors())
        on = value == 'return'
        assert hasattr(model, 'rs_carry') == on and hasattr(model, 'rs_state') == on and hasattr(model, '_rs_partial') == on
        assert len(tr._shadow_tensors()) == n_env + 3 + 2 * on and len(tr._state_tensors()) == n_env + 6 + 2 * on
        for _ in range(2):
            tr.run_batch()
        torch.cuda.synchronize()
        assert tr._upd is not None and tr.update_capture_error is None
        nodes.append(G.census(tr._upd['grads']))
        if not on:
            assert not n_calls
            exp = tr.buf_rraw / model.reward_norm
            if model.reward_clip > 0:
                exp = exp.clamp(-model.reward_clip, model.reward_clip)
            assert torch.equal(_bits(model.buf_r), _bits(exp))
        runs.append((model.policy.params.flat.clone(), model.R.clone(), model.buf_r.clone()))
        del env, model, tr
    assert n_calls
    assert nodes[0] == nodes[1] and set(nodes[2]) == {'kernel'} and nodes[2]['kernel'] == nodes[0]['kernel'] + 2, nodes
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(_bits(a), _bits(b))
    assert not torch.equal(runs[0][0], runs[2][0]), 'reward_scale = return left the weights of the default run'


@pytest.mark.parametrize('ini', ENGINE_INIS)
def test_save_after_batch_two_and_load_give_the_uninterrupted_third_batch(ini, tmp_path):
    """The checkpoint carries the running moments and the carried returns: batch 3 of a fresh trainer that loaded it (and was handed
    the simulator and recurrent state, which no checkpoint holds) has the bits of batch 3 of the uninterrupted run."""
    d = str(tmp_path) + os.sep
    env, model, tr = _build(ini, False, 'return')
    for _ in range(2):
        tr.run_batch()
    torch.cuda.synchronize()
    model.save(d, 120)
    snap = tr._snapshot()
    tr.run_batch()
    torch.cuda.synchronize()
    want = [t.clone() for t in (model.buf_r, model.rs_carry, model.rs_state, model.policy.params.flat)]
    env2, model2, tr2 = _build(ini, False, 'return')
    tr2._restore(snap)
    model2.h_bw.copy_(model2.h_fw)
    model2.c_bw.copy_(model2.c_fw)
    model2.policy.invalidate_cached_msg()
    model2.rs_carry.zero_()
    model2.rs_state.zero_()                       # (the statistics come from the checkpoint alone)
    assert model2.load(d, 120)
    tr2.run_batch()
    torch.cuda.synchronize()
    got = [model2.buf_r, model2.rs_carry, model2.rs_state, model2.policy.params.flat]
    for name, a, b in zip(('buf_r', 'carry', 'state', 'weights'), want, got):
        assert torch.equal(_bits(a), _bits(b)), name


def test_coupled_trainer_snapshots_carry_and_state():
    """The coupled agent's hand-off guard: carry and state are part of what a refused batch is rewound to (list membership, and a
    hand-made snapshot put back through _restore; no time-out is provoked)."""
    env, model, tr = _build(ENGINE_INIS[1], True, 'return')
    for lst in (tr._shadow_tensors(), tr._state_tensors()):
        assert any(t is model.rs_carry for t in lst) and any(t is model.rs_state for t in lst)
    if tr._shadow is not None:
        assert len(tr._shadow) == len(tr._shadow_tensors())
        assert [tuple(s.shape) for s in tr._shadow[-2:]] == [tuple(model.rs_carry.shape), tuple(model.rs_state.shape)]
    tr.run_batch()
    torch.cuda.synchronize()
    snap = tr._snapshot()
    tensors = tr._state_tensors()
    ic, is_ = [i for i, t in enumerate(tensors) if t is model.rs_carry][0], [i for i, t in enumerate(tensors) if t is model.rs_state][0]
    snap[ic] = torch.arange(model.rs_carry.numel(), dtype=F64, device='cuda') / 3
    snap[is_] = torch.arange(model.rs_state.numel(), dtype=F64, device='cuda') / 7
    tr.run_batch()
    tr._restore(snap)
    torch.cuda.synchronize()
    assert torch.equal(model.rs_carry, snap[ic]) and torch.equal(model.rs_state, snap[is_])


def test_one_replica_path_gives_the_bits_of_the_batched_path():
    """The reference-API path (model.forward / add_transition / backward, one replica) on the scripted three-batch run of the IA2C-FP
    golden: `record` keeps the raw rewards and the update makes the one call -- buf_r, carry and state equal, bit for bit, what
    load_rewards gives a second model for the same rewards and flags; and they are the restatement's."""
    from deeprl_network_amd.agents import models
    z = load_npz(os.path.join(GOLDEN, 'nn_ia2c_fp_line.npz'))
    cp = cacc_config(agent='ia2c_fp', n_step=int(z['n_step']), reward_norm=float(z['reward_norm']), coop_gamma=-1)
    cp['MODEL_CONFIG']['reward_scale'] = 'return'
    nb = z['nb']
    N = nb.shape[0]

    def make():
        np.random.seed(int(z['seed']))
        return models.IA2C_FP([5 * (1 + int(nb[i].sum())) for i in range(N)], [4] * N, nb, z['dist'], -1.0, 10000, cp['MODEL_CONFIG'],
                              seed=int(z['seed']), num_envs=1, device='cuda')
    a, b = make(), make()
    seen = []
    inner = a._scale_rewards

    def spy(raw):
        inner(raw)
        seen.append([t.clone() for t in (raw, a.buf_done_post, a.buf_r, a.rs_carry, a.rs_state)])
    a._scale_rewards = spy
    drive_scripted(a, z)
    assert len(seen) >= 3 and torch.isfinite(a.policy.params.flat).all()
    ref = _ref_of(b)
    for k, (raw, done, buf_r, carry, state) in enumerate(seen):
        b.buf_done_post.copy_(done)
        b.load_rewards(raw)
        b.t = 0
        torch.cuda.synchronize()
        for name, x, y in (('buf_r', buf_r, b.buf_r), ('carry', carry, b.rs_carry), ('state', state, b.rs_state)):
            assert torch.equal(_bits(x), _bits(y)), 'batch %d: %s' % (k, name)
        r = raw.cpu().numpy().reshape(b.n_step, -1)
        st = state.cpu().numpy()
        rc.assert_call(dict(r_out=buf_r.cpu().numpy().reshape(b.n_step, -1), carry=carry.cpu().numpy(), n=st[0], mean=st[5], sigma=st[6]),
                       r, ref.call(r, done.cpu().numpy()), b.reward_scale_epsilon, max(b.reward_clip, 0.0), 'one replica, batch %d' % k)

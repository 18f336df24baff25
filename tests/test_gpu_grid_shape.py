"""GPU: the synthetic ATSC grid on a rows x cols lattice of 2..32 intersections (ENV_CONFIG grid_rows / grid_cols; csrc/grid.hip's
runtime-shape kernels through nmarl_grid_step_rc / nmarl_grid_reset_rc) against its restatement tests/grid_shape_ref.py, the
5x5 grid through the runtime-shape kernels against the 5x5 kernels bit for bit, and the shape through every layer above:
reference duck-type, traffic record, batched engine, CLI.  Tolerances: those of tests/test_gpu_grid.py for the same quantities
(tests/test_grid_shape_cpu.py shows the float32 reference itself stays inside them on these inputs)."""
import ctypes

import numpy as np
import pytest
import torch

import grid_shape_ref as S
from helpers import grid_config
from oracle import grid_ref as G

pytestmark = pytest.mark.gpu


def shape_config(rows, cols, agent='ma2c_ic3', coop_gamma=-1, seed=12, n_step=120, objective=None):
    cp = grid_config(agent=agent, coop_gamma=coop_gamma, seed=seed, n_step=n_step)
    cp['ENV_CONFIG']['grid_rows'] = str(rows)
    cp['ENV_CONFIG']['grid_cols'] = str(cols)
    if objective is not None:
        cp['ENV_CONFIG']['objective'] = objective
        cp['ENV_CONFIG']['coef_wait'] = '0.2'
    return cp


def make(rows, cols, E, coop_gamma=-1, env_id_base=0, seed=12, objective=None, agent='ma2c_ic3'):
    from deeprl_network_amd.envs.large_grid_env import LargeGridBatchEnv
    env = LargeGridBatchEnv(shape_config(rows, cols, agent, coop_gamma, seed, objective=objective)['ENV_CONFIG'], num_envs=E,
                            env_id_base=env_id_base)
    N = rows * cols
    assert env.n_agent == N and env.q.shape == (E, N, 6) and env.obs.shape == (E, N, 60) and env.prev_action.shape == (E, N)
    assert env.fixed_shape == ((rows, cols) == (5, 5))
    return env


def ref_for(env, dtype=np.float32):
    return S.ShapeBatchRef(G.GridParams(config=env.config), env.rows, env.cols, E=env.E, dtype=dtype)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('E', [1, 7, 8, 9, 77])
@pytest.mark.parametrize('coop_gamma', [-1, 0.9])
@pytest.mark.parametrize('rows,cols', [(1, 2), (2, 2), (3, 3), (6, 5), (5, 6), (4, 8), (2, 16)])
def test_trajectory_vs_restatement(rows, cols, coop_gamma, E):
    env = make(rows, cols, E, coop_gamma)
    rng = np.random.RandomState(E)
    U = rng.rand(E, 4).astype(np.float32)
    env.reset(u0=cuda(U))
    ref = ref_for(env)
    ref.reset(np.float32(0.8) + np.float32(0.4) * U)
    np.testing.assert_array_equal(env.xi.cpu().numpy(), ref.xi)
    for t in range(150):
        a = S.actions(rng, ref, t)
        obs, r, d, g = env.step(cuda(a))
        ro, rr, rd, rg = ref.step(a)
        np.testing.assert_allclose(env.q.cpu().numpy(), ref.q, rtol=2e-4, atol=2e-3, err_msg='q t=%d' % t)
        np.testing.assert_allclose(env.transit.cpu().numpy(), ref.tr, rtol=2e-4, atol=2e-3, err_msg='tr t=%d' % t)
        np.testing.assert_allclose(obs.cpu().numpy(), ref.gather(ro), rtol=2e-4, atol=1e-3)
        np.testing.assert_allclose(g.cpu().numpy(), rg, rtol=2e-4, atol=2e-2)
        np.testing.assert_allclose(r.cpu().numpy(), rr, rtol=2e-4, atol=2e-2)
        assert np.array_equal(d.cpu().numpy().astype(bool), rd)
        assert np.array_equal(env.prev_action.cpu().numpy(), a)
    assert float(ref.q.max()) > 1.0


@pytest.mark.parametrize('rows,cols', [(3, 3), (5, 6), (1, 32)])
def test_single_step_tight_from_random_state(rows, cols):
    """One step from identical random states (no accumulated drift): rtol 1e-5."""
    E, N = 64, rows * cols
    env = make(rows, cols, E)
    rng = np.random.RandomState(3)
    env.reset(u0=cuda(rng.rand(E, 4).astype(np.float32)))
    ref = ref_for(env)
    ref.reset(env.xi.cpu().numpy())
    ref.q = rng.uniform(0, 30, size=(E, N, 6)).astype(np.float32) * (rng.rand(E, N, 6) < 0.8)
    ref.tr = rng.uniform(0, 3, size=(E, N, 6)).astype(np.float32)
    ref.prev = rng.randint(0, 5, size=(E, N))
    ref.t = rng.randint(0, 700, size=E)
    env.q.copy_(cuda(ref.q)); env.transit.copy_(cuda(ref.tr))
    env.prev_action.copy_(cuda(ref.prev.astype(np.uint8))); env.t.copy_(cuda(ref.t.astype(np.int32)))
    a = rng.randint(0, 5, size=(E, N)).astype(np.uint8)
    obs, r, d, g = env.step(cuda(a))
    ro, rr, rd, rg = ref.step(a)
    np.testing.assert_allclose(env.q.cpu().numpy(), ref.q, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(env.transit.cpu().numpy(), ref.tr, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(obs.cpu().numpy(), ref.gather(ro), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(g.cpu().numpy(), rg, rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize('E', [8, 9])
@pytest.mark.parametrize('objective,coop_gamma', [('wait', -1), ('hybrid', 0.9)])
@pytest.mark.parametrize('rows,cols', [(3, 3), (4, 8)])
def test_wait_and_hybrid_objectives_vs_restatement(rows, cols, objective, coop_gamma, E):
    """As tests/test_gpu_grid.py's test of the two objectives: head_wait handed over from the restatement before every step and
    compared exactly, a lane within rounding of the threshold excepted (< 2e-3 of the lanes); rewards on the replicas without
    one; the fused auto-reset clears the state."""
    N = rows * cols
    env = make(rows, cols, E, coop_gamma, objective=objective)
    assert env.head_wait is not None and env.head_wait.shape == (E, N, 6)
    rng = np.random.RandomState(E)
    U = rng.rand(E, 4).astype(np.float32)
    env.reset(u0=cuda(U))
    ref = ref_for(env)
    assert ref.p.objective == objective and ref.p.coef_wait == pytest.approx(0.2)
    ref.reset(np.float32(0.8) + np.float32(0.4) * U)
    seen_wait = 0.0
    for t in range(120):
        a = S.actions(rng, ref, t, hold=0.7)
        env.head_wait.copy_(cuda(ref.hw))
        obs, r, d, g = env.step(cuda(a))
        ro, rr, rd, rg = ref.step(a)
        bad = env.head_wait.cpu().numpy() != ref.hw
        assert bad.mean() < 2e-3, 'head_wait differs in %d lanes at t=%d' % (bad.sum(), t)
        np.testing.assert_allclose(env.q.cpu().numpy(), ref.q, rtol=2e-4, atol=2e-3)
        ok = ~bad.any(axis=(1, 2))
        np.testing.assert_allclose(g.cpu().numpy()[ok], rg[ok], rtol=2e-4, atol=5e-2)
        np.testing.assert_allclose(r.cpu().numpy()[ok], rr[ok], rtol=2e-4, atol=5e-2)
        seen_wait = max(seen_wait, float(ref.hw.max()))
    assert seen_wait >= 10.0
    env.t.fill_(env.T - 1)
    env.step(torch.zeros(E, N, dtype=torch.uint8, device='cuda'), auto_reset=True)
    assert torch.all(env.head_wait == 0) and torch.all(env.q == 0) and torch.all(env.transit == 0) and torch.all(env.t == 0)


@pytest.mark.parametrize('E', [7, 8, 300])
@pytest.mark.parametrize('compact', [True, False])
@pytest.mark.parametrize('objective', ['queue', 'wait', 'hybrid'])
def test_5x5_through_the_rc_entries_is_bit_identical(objective, compact, E):
    """rows = cols = 5 handed to nmarl_grid_reset_rc / nmarl_grid_step_rc (the runtime-shape kernels) against nmarl_grid_reset /
    nmarl_grid_step (the 5x5 kernels): 40 steps, auto-reset on the last, every state array and every output bit for bit."""
    envs = []
    for rc in (False, True):
        env = make(5, 5, E, coop_gamma=0.9, env_id_base=70, objective=objective)
        if compact:
            env.set_compact_obs(True)
        env.params.T = 40
        env.fixed_shape = not rc                        # the host's dispatch rule, overridden: 5x5 on the `_rc` entries
        env.reset()
        envs.append(env)
    a_env, b_env = envs
    assert torch.equal(a_env.xi, b_env.xi) and torch.equal(a_env.episode, b_env.episode) and int(b_env.episode.min()) == 1
    rng = np.random.RandomState(E)
    for t in range(40):
        a = cuda(rng.randint(0, 5, size=(E, 25)).astype(np.uint8))
        oa, ra, da, ga = a_env.step(a, auto_reset=True)
        ob, rb, db, gb = b_env.step(a, auto_reset=True)
        for x, y in zip(a_env.state_tensors() + [oa, ra, da, ga], b_env.state_tensors() + [ob, rb, db, gb]):
            assert torch.equal(x, y), t
        assert bool(da.all()) == (t == 39)
    assert float(ga.min()) < 0 and torch.all(b_env.episode == 2) and torch.all(b_env.t == 0) and torch.all(b_env.q == 0)
    assert not torch.equal(b_env.xi, torch.ones_like(b_env.xi))


SENT_F, SENT_B, SENT_I, TAIL = -12345.0, 0xAB, -77, 96


@pytest.mark.parametrize('E', [7, 9])
@pytest.mark.parametrize('compact', [True, False])
@pytest.mark.parametrize('rows,cols', [(1, 2), (3, 3), (5, 6)])
def test_idle_and_tail_lanes_write_nothing(rows, cols, compact, E):
    """Every state and output array with a sentinel-filled tail behind its E * N rows, through the C-ABI: the tails are intact
    after reset, a step, and a step with the fused auto-reset (lanes >= N of a half wave hold no node; E = 7, 9: the partial
    group of replicas of a block)."""
    from deeprl_network_amd import _lib
    N, W = rows * cols, 12 if compact else 60
    sizes = dict(q=(E * N * 6, torch.float32), transit=(E * N * 6, torch.float32), head_wait=(E * N * 6, torch.float32),
                 prev=(E * N, torch.uint8), t=(E, torch.int32), xi=(E * 4, torch.float32), obs=(E * N * W, torch.float32),
                 reward=(E * N, torch.float32), done=(E, torch.uint8), greward=(E, torch.float32), episode=(E, torch.int32),
                 action=(E * N, torch.uint8))
    sent = {torch.float32: SENT_F, torch.uint8: SENT_B, torch.int32: SENT_I}
    buf = {k: torch.full((n + TAIL,), sent[dt], dtype=dt, device='cuda') for k, (n, dt) in sizes.items()}
    buf['episode'][:E] = 0
    buf['action'][:E * N] = cuda(np.random.RandomState(E).randint(0, 5, size=E * N).astype(np.uint8))
    p = _lib.GridParams()
    p.norm_wave, p.clip_wave, p.peak1, p.peak2, p.T, p.per_agent_reward = 5.0, 2.0, 1100.0, 925.0, 3, 1
    p.compact_obs, p.objective, p.coef_wait, p.head_wait = int(compact), 2, 0.2, buf['head_wait'].data_ptr()
    P, st = _lib.ptr, _lib.stream()

    def tails_intact(what):
        torch.cuda.synchronize()
        for k, (n, dt) in sizes.items():
            assert bool((buf[k][n:] == sent[dt]).all()), '%s wrote behind %s' % (what, k)

    rc = _lib.lib.nmarl_grid_reset_rc(ctypes.byref(p), E, None, None, 12, 0, P(buf['episode']), P(buf['q']), P(buf['transit']),
                                      P(buf['prev']), P(buf['t']), P(buf['xi']), P(buf['obs']), st, rows, cols)
    assert rc == 0
    tails_intact('reset')
    for k in ('q', 'transit', 'head_wait', 'prev', 't', 'obs'):
        assert bool((buf[k][:sizes[k][0]] == 0).all()), k
    assert bool((buf['xi'][:E * 4] >= 0.8).all()) and bool((buf['episode'][:E] == 1).all())
    for step in range(3):
        rc = _lib.lib.nmarl_grid_step_rc(ctypes.byref(p), E, P(buf['action']), P(buf['q']), P(buf['transit']), P(buf['prev']),
                                         P(buf['t']), P(buf['xi']), P(buf['obs']), P(buf['reward']), P(buf['done']),
                                         P(buf['greward']), 1, 12, 0, P(buf['episode']), st, rows, cols)
        assert rc == 0
        tails_intact('step %d' % step)
        for k in ('reward', 'done', 'greward'):
            assert not bool((buf[k][:sizes[k][0]] == sent[sizes[k][1]]).any()), k
        if step == 0:
            assert bool((buf['transit'][:E * N * 6] > 0).any()) and bool((buf['prev'][:E * N] == buf['action'][:E * N]).all())
    assert bool((buf['done'][:E] == 1).all()) and bool((buf['episode'][:E] == 2).all()) and bool((buf['t'][:E] == 0).all())
    assert bool((buf['q'][:E * N * 6] == 0).all()) and bool((buf['obs'][:E * N * W] == 0).all())


def test_invalid_shapes_are_refused_without_a_launch():
    from deeprl_network_amd import _lib
    env = make(3, 3, 4)
    env.reset()
    before = [x.clone() for x in env.state_tensors()]
    P, st = _lib.ptr, _lib.stream()
    a = torch.zeros(4, 9, dtype=torch.uint8, device='cuda')
    for rows, cols in ((0, 3), (3, 0), (1, 1), (6, 6), (1, 33), (33, 1), (-1, -9), (65536, 65536)):
        assert _lib.lib.nmarl_grid_step_rc(ctypes.byref(env.params), 4, P(a), P(env.q), P(env.transit), P(env.prev_action), P(env.t),
                                           P(env.xi), P(env.obs), P(env.reward), P(env.done), P(env.global_reward), 0, 12, 0,
                                           P(env.episode), st, rows, cols) == -1
        assert _lib.lib.nmarl_grid_reset_rc(ctypes.byref(env.params), 4, None, None, 12, 0, P(env.episode), P(env.q), P(env.transit),
                                            P(env.prev_action), P(env.t), P(env.xi), P(env.obs), st, rows, cols) == -1
    torch.cuda.synchronize()
    for x, y in zip(before, env.state_tensors()):
        assert torch.equal(x, y)


@pytest.mark.parametrize('rows,cols', [(3, 3), (2, 16)])
def test_episode_end_auto_reset_and_philox(rows, cols):
    from oracle import philox
    E, base, seed, N = 64, 500, 12, rows * cols
    env = make(rows, cols, E, env_id_base=base, seed=seed)
    env.params.T = 6
    env.reset()
    U0 = np.stack(philox.philox4x32(base + np.arange(E), 0, 0, 0, seed, 0), axis=-1)
    np.testing.assert_array_equal(env.xi.cpu().numpy(), np.float32(0.8) + np.float32(0.4) * philox.u01(U0))
    assert torch.all(env.episode == 1)
    a = torch.zeros(E, N, dtype=torch.uint8, device='cuda')
    for t in range(6):
        obs, r, d, g = env.step(a, auto_reset=True)
        assert bool(d.all()) == (t == 5)
    assert torch.all(env.t == 0) and torch.all(env.q == 0) and torch.all(env.obs == 0) and torch.all(env.episode == 2)
    U1 = np.stack(philox.philox4x32(base + np.arange(E), 0, 1, 0, seed, 0), axis=-1)
    np.testing.assert_array_equal(env.xi.cpu().numpy(), np.float32(0.8) + np.float32(0.4) * philox.u01(U1))


def test_batch_invariance_on_4x8():
    E = 1024
    env = make(4, 8, E)
    env.reset()
    small = make(4, 8, 8, env_id_base=400)
    small.reset()
    assert torch.equal(env.xi[400:408], small.xi)
    rng = np.random.RandomState(5)
    for t in range(40):
        a = cuda(rng.randint(0, 5, size=(E, 32)).astype(np.uint8))
        env.step(a)
        small.step(a[400:408].contiguous())
        assert torch.equal(env.q[400:408], small.q) and torch.equal(env.transit[400:408], small.transit)
        assert torch.equal(env.obs[400:408], small.obs) and torch.equal(env.global_reward[400:408], small.global_reward)
    assert torch.isfinite(env.obs).all() and float(env.global_reward.max()) <= 0 and float(env.global_reward.min()) < 0


@pytest.mark.parametrize('rows,cols', [(3, 4), (1, 6)])
def test_reference_duck_type(rows, cols):
    """LargeGridEnv (one replica): IA2C / IA2C-FP observations list the neighbours north, east, south, west; an MA2C agent gets
    its own vector; neighbour actions come in ascending index."""
    from deeprl_network_amd.envs.large_grid_env import LargeGridEnv
    N = rows * cols
    order = S.neighbor_order(rows, cols)
    nb, dist = S.masks(rows, cols)
    rng = np.random.RandomState(0)
    for agent in ('ia2c', 'ia2c_fp', 'ma2c_nc'):
        env = LargeGridEnv(shape_config(rows, cols, agent=agent, coop_gamma=0.9)['ENV_CONFIG'])
        assert env.n_agent == N and env.node_names == ['nt%d' % (i + 1) for i in range(N)] and env.n_a_ls == [5] * N
        np.testing.assert_array_equal(env.neighbor_mask, nb)
        np.testing.assert_array_equal(env.distance_mask, dist)
        env.train_mode = True
        ob = env.reset()
        fp_w = 5 if agent == 'ia2c_fp' else 0
        want_len = [12 * (1 + len(order[i])) + fp_w * len(order[i]) if agent.startswith('ia2c') else 12 for i in range(N)]
        assert [len(o) for o in ob] == want_len
        assert env.n_s_ls == [12 * (1 + len(order[i])) if agent.startswith('ia2c') else 12 for i in range(N)]
        for _ in range(30):
            act = rng.randint(0, 5, size=N)
            ob, r, d, g = env.step(act)
        assert np.asarray(r).shape == (N,) and g <= 0
        env.update_fingerprint([rng.dirichlet(np.ones(5)) for _ in range(N)])
        ob = env._state_list()
        own = env.batch.obs[0, :, :12].cpu().numpy()
        assert own.max() > 0
        for i in range(N):
            parts = [own[i]]
            if agent.startswith('ia2c'):
                parts += [own[j] for j in order[i]]
            if agent == 'ia2c_fp':
                parts += [env.fp[j] for j in order[i]]
            np.testing.assert_allclose(ob[i], np.concatenate(parts), rtol=0, atol=0)
        na = env.get_neighbor_action(act)
        for i in range(N):
            assert list(na[i]) == [act[j] for j in sorted(order[i])]


@pytest.mark.parametrize('rows,cols', [(3, 4), (1, 6)])
def test_traffic_rows_and_greedy_evaluate(rows, cols, tmp_path):
    """The traffic record on the shape against tests/traffic_record_ref.py driven with the shape's demand table (entries per
    group x the per-entry rate), at the tolerances of tests/test_gpu_traffic_record.py; and `main.py evaluate` with the greedy
    agent writes the reference's three tables."""
    import pandas as pd
    from deeprl_network_amd.envs.traffic_record import GRID_MULT, TrafficRecorder
    from deeprl_network_amd.main import main
    from traffic_record_ref import COLUMNS, TrafficRecordRef
    E, N, steps = 5, rows * cols, 40
    env = make(rows, cols, E)
    rng = np.random.RandomState(100 + E)
    env.reset(u0=cuda(rng.rand(E, 4).astype(np.float32)))
    rec = TrafficRecorder(env, steps)
    demand = S.demand_table(rows, cols, 1100.0, 925.0)
    np.testing.assert_allclose(rec.demand_host, demand, rtol=1e-15, atol=0)
    ref = TrafficRecordRef(np.tile(np.array(GRID_MULT, dtype=np.int32), (N, 1)), demand, E)
    rec.begin()
    for k in range(steps):
        env.step(cuda(rng.randint(0, 5, size=(E, N)).astype(np.uint8)))
        rec.step(k)
        want = ref.step(env.q.cpu().numpy(), env.transit.cpu().numpy(), env.t.cpu().numpy(), env.xi.cpu().numpy())
        got = rec.rec[k].cpu().numpy()
        for c, name in enumerate(COLUMNS):
            np.testing.assert_allclose(got[:, c], want[:, c], rtol=1e-6, atol=1e-6, err_msg='%s, step %d' % (name, k))
        assert np.array_equal(rec.stand.cpu().numpy(), ref.stand)
    assert rec.rows()[-1, :, 0].min() > 1
    # greedy evaluation through the CLI
    cp = shape_config(rows, cols, agent='greedy', coop_gamma=0.75)
    cp['ENV_CONFIG']['episode_length_sec'] = '100'
    base = tmp_path / 'greedy'
    (base / 'data').mkdir(parents=True)
    (base / 'model').mkdir()
    with open(base / 'data' / 'config_greedy.ini', 'w') as f:
        cp.write(f)
    main(['--base-dir', str(base), 'evaluate', '--evaluation-seeds', '10000,20000'])
    stem = str(base / 'eva_data') + '/atsc_large_grid_greedy_'
    control, traffic, trip = (pd.read_csv(stem + name + '.csv', index_col=0) for name in ('control', 'traffic', 'trip'))
    assert set(control.columns) == {'episode', 'time_sec', 'step', 'action', 'reward'}
    assert set(traffic.columns) == {'episode', 'time_sec', 'number_total_car', 'number_departed_car', 'number_arrived_car',
                                    'avg_wait_sec', 'avg_speed_mps', 'std_queue', 'avg_queue'}
    assert set(trip.columns) == {'episode', 'id', 'depart_sec', 'arrival_sec', 'duration_sec', 'wait_step', 'wait_sec'}
    assert len(control) == len(traffic) == 2 * 20 and len(trip) == 2
    assert all(len(str(a).split(',')) == N for a in control['action'])
    assert (traffic['number_total_car'] > 0).all() and np.isfinite(traffic.to_numpy(dtype=np.float64)).all()


AGENTS = ['ia2c', 'ia2c_fp', 'ma2c_cu', 'ma2c_nc', 'ma2c_ic3', 'ma2c_dial']


def build_trainer(rows, cols, agent, E, use_graph, n_step=20):
    from deeprl_network_amd.envs import make_batch_env
    from deeprl_network_amd.main import init_agent
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    cp = shape_config(rows, cols, agent=agent, n_step=n_step)
    env = make_batch_env(cp['ENV_CONFIG'], num_envs=E)
    np.random.seed(12)
    model = init_agent(env, cp['MODEL_CONFIG'], 10 ** 9, 12, num_envs=E)
    return env, model, BatchedTrainer(env, model, Counter(10 ** 12, 10 ** 12, 10 ** 12), use_graph=use_graph)


@pytest.mark.parametrize('rows,cols,agent', [(3, 3, a) for a in AGENTS] + [(4, 8, 'ma2c_ic3'), (4, 8, 'ia2c_fp'), (1, 5, 'ma2c_ic3'),
                                                                          (1, 5, 'ia2c_fp')])
def test_batched_engine_any_shape(rows, cols, agent):
    """BatchedTrainer for two batches of n_step = 20 at E = 64, eager and with hipGraphs: actions, rewards and post-update weights
    bit-identical, finite, no hand-off fall-back; off 5x5 a lock-step is the lock-step launch plus one env launch."""
    from deeprl_network_amd import ops
    E, N = 64, rows * cols
    runs = []
    for use_graph in (False, True):
        env, model, tr = build_trainer(rows, cols, agent, E, use_graph)
        assert tr.N == N and not tr.env_in_kernel and not env.inkernel_step_supported()
        w0 = model.policy.params.flat.clone()
        rec = []
        for b in range(2):
            tr.run_batch()
            torch.cuda.synchronize()
            rec += [model.buf_act.clone(), tr.buf_rraw.clone(), tr.buf_g.clone(), model.policy.params.flat.clone()]
            assert all(bool(torch.isfinite(x).all()) for x in model.last_loss if torch.is_tensor(x))
        assert tr.handoff_fallbacks == 0 and int(ops.handoff_status(env.device)[0].item()) == 0
        assert bool(torch.isfinite(rec[-1]).all()) and not torch.equal(rec[-1], w0) and not torch.equal(rec[3], rec[-1])
        assert int(model.buf_act.max()) <= 4 and model.buf_act.shape == (20, E, N) and float(tr.buf_g.min()) < 0
        runs.append(rec)
        del env, model, tr
    for k, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), 'hipGraph replay differs from eager launches (record %d)' % k


def test_commnet_on_5x5_keeps_the_env_step_inside_the_launch():
    env, model, tr = build_trainer(5, 5, 'ma2c_ic3', 1024, True)
    assert env.fixed_shape and env.inkernel_step_supported() and tr.env_in_kernel
    env, model, tr = build_trainer(3, 3, 'ma2c_ic3', 1024, True)
    assert not env.inkernel_step_supported() and not tr.env_in_kernel
    with pytest.raises(Exception, match='5x5'):
        env.inkernel_step()


def test_cli_train_and_evaluate_a_3x4_grid(tmp_path):
    """main.py train on an ini with grid_rows = 3, grid_cols = 4 (the batched loop, --num-envs 16) writes train_reward.csv and a
    checkpoint; main.py evaluate loads it and writes the three tables with twelve actions per control row."""
    import os

    import pandas as pd
    from deeprl_network_amd.main import main
    cp = shape_config(3, 4, agent='ma2c_nc', coop_gamma=0.9, n_step=20)
    cp['ENV_CONFIG']['episode_length_sec'] = '100'
    cp['ENV_CONFIG']['num_envs'] = '16'
    cp['TRAIN_CONFIG']['total_step'] = '60'
    ini = tmp_path / 'config_ma2c_nc_grid34.ini'
    with open(ini, 'w') as f:
        cp.write(f)
    base = str(tmp_path / 'run')
    main(['--base-dir', base, 'train', '--config-dir', str(ini), '--num-envs', '16'])
    df = pd.read_csv(base + '/data/train_reward.csv')
    assert {'agent', 'step', 'avg_reward', 'std_reward'} <= set(df.columns) and len(df) >= 1 and np.isfinite(df['avg_reward']).all()
    assert len([f for f in os.listdir(base + '/model') if f.startswith('checkpoint-')]) == 1
    main(['--base-dir', base, 'evaluate', '--evaluation-seeds', '2000'])
    control = pd.read_csv(base + '/eva_data/atsc_large_grid_ma2c_nc_control.csv')
    traffic = pd.read_csv(base + '/eva_data/atsc_large_grid_ma2c_nc_traffic.csv')
    trip = pd.read_csv(base + '/eva_data/atsc_large_grid_ma2c_nc_trip.csv')
    assert len(control) == len(traffic) == 20 and len(trip) == 1
    assert all(len(str(a).split(',')) == 12 for a in control['action']) and (control['reward'] <= 0).all()

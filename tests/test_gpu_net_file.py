"""GPU: the signalised network read from a file (ENV_CONFIG net_file): nmarl_net_step_dem -- the step kernel with the demand's
activity table as data -- bit for bit against nmarl_net_step on Monaco, and on the fixture networks of tests/net_file_fixtures.py
against the restatement; the objectives, the rule agents, the traffic record, the learned agents and the CLI on such a network."""
import os

import numpy as np
import pytest
import torch

import net_file_fixtures as F

pytestmark = pytest.mark.gpu

MONACO = os.path.join(F.ROOT, 'config', 'networks', 'monaco.json')
COEF = 0.2
TRAFFIC_CSV = {'episode', 'time_sec', 'number_total_car', 'number_departed_car', 'number_arrived_car', 'avg_wait_sec',
               'avg_speed_mps', 'std_queue', 'avg_queue'}                                   # atsc_env.py:490-498
TRIP_CSV = {'episode', 'id', 'depart_sec', 'arrival_sec', 'duration_sec', 'wait_step', 'wait_sec'}     # atsc_env.py:113-120
CONTROL_CSV = {'episode', 'time_sec', 'step', 'action', 'reward'}


@pytest.fixture(scope='module')
def nets(tmp_path_factory):
    d = tmp_path_factory.mktemp('nets')
    return {'small': F.write(d, F.SMALL, 'small.json'), 'limits': F.write(d, F.LIMITS, 'limits.json'),
            'uniform': F.write(d, F.UNIFORM, 'uniform.json')}


@pytest.fixture(scope='module')
def topos():
    return {'small': F.Topo(F.SMALL), 'limits': F.Topo(F.LIMITS), 'uniform': F.Topo(F.UNIFORM)}


def make(path, E, **kw):
    from deeprl_network_amd.envs.real_net_env import RealNetBatchEnv
    env_kw = {k: kw.pop(k) for k in ('env_id_base',) if k in kw}
    return RealNetBatchEnv(F.config(path, **kw)['ENV_CONFIG'], num_envs=E, **env_kw)


def make_ref(env, tp, objective=None):
    from oracle import realnet_ref as R
    if objective is None:
        return F.with_activity(R.NetBatchRef)(R.NetParams(config=env.config), E=env.E, dtype=np.float32, topo=tp)
    from realnet_wait_ref import NetWaitRef
    return F.with_activity(NetWaitRef)(R.NetParams(config=env.config), E=env.E, dtype=np.float32, topo=tp, objective=objective,
                                       coef_wait=COEF)


def random_state(ref, rng, t_max=720):
    """A random mid-episode state of the oracle (tests/test_gpu_realnet.py::test_single_step_tight_from_random_state)."""
    E, tp = ref.E, ref.tp
    ref.q = (rng.uniform(0, 30, size=(E, tp.N, tp.L)) * (rng.rand(E, tp.N, tp.L) < 0.8) * ref.valid).astype(np.float32)
    ref.q = np.minimum(ref.q, np.float32(26.0))
    ref.tr = (rng.uniform(0, 3, size=(E, tp.N, tp.L)) * ref.valid).astype(np.float32)
    ref.prev = F.rand_actions(rng, E, tp)
    ref.t = rng.randint(0, t_max, size=E)
    if hasattr(ref, 'hw'):
        ref.hw = (5.0 * rng.randint(0, 40, size=(E, tp.N, tp.L)) * ref.valid).astype(np.float32)


def hand_over(env, ref):
    env.q.copy_(torch.from_numpy(ref.q))
    env.transit.copy_(torch.from_numpy(ref.tr))
    env.prev_action.copy_(torch.from_numpy(ref.prev.astype(np.uint8)))
    env.t.copy_(torch.from_numpy(ref.t.astype(np.int32)))
    if env.head_wait is not None:
        env.head_wait.copy_(torch.from_numpy(ref.hw))


# ------------------------------------------------------------------ Monaco through both entries
@pytest.mark.parametrize('objective', ['queue', 'hybrid'])
@pytest.mark.parametrize('t0', [59, 659])
@pytest.mark.parametrize('E', [1, 7, 9, 2051])
def test_monaco_table_gives_monaco_bits(monkeypatch, E, t0, objective):
    """The built-in network through nmarl_net_step and the same network read from config/networks/monaco.json through
    nmarl_net_step_dem, 4 steps from one random state across a piece boundary (t = 59 -> 60) and into the last piece (659 -> 660):
    every output and every state array bit for bit.  E: both replicas-per-block forms (4 up to 2048, 8 above), partial last blocks."""
    from oracle import realnet_ref as R
    from deeprl_network_amd import _lib
    envs = [make(None, E, objective=objective, coef_wait=COEF), make(MONACO, E, objective=objective, coef_wait=COEF)]
    assert envs[0].topo.dem is None and envs[1].topo.dem is not None
    rng = np.random.RandomState(1000 * E + t0)
    U = torch.from_numpy(rng.rand(E, 4).astype(np.float32)).cuda()
    ref = R.NetBatchRef(R.NetParams(config=envs[0].config), E=E, dtype=np.float32)      # (only its random state is used)
    ref.reset(np.float32(0.8) + np.float32(0.4) * U.cpu().numpy())
    random_state(ref, rng)
    ref.t[:] = t0
    ref.hw = (5.0 * rng.randint(0, 40, size=ref.q.shape) * ref.valid).astype(np.float32)
    for env in envs:
        env.reset(u0=U)
        hand_over(env, ref)
    entries, check = [], _lib.check
    monkeypatch.setattr(_lib, 'check', lambda rc, what: entries.append(what) or check(rc, what))      # which entry each env calls
    for step in range(4):
        a = torch.from_numpy(F.rand_actions(rng, E, R.TOPO).astype(np.uint8)).cuda()
        outs = [[x.clone() for x in env.step(a)] for env in envs]
        for x, y, what in zip(outs[0], outs[1], ('obs', 'reward', 'done', 'global reward')):
            assert torch.equal(x, y), '%s differs at step %d' % (what, step)
        for x, y in zip(envs[0].state_tensors(), envs[1].state_tensors()):
            assert x.shape == y.shape and torch.equal(x, y), 'a state array differs at step %d' % step
    assert entries == ['nmarl_net_step', 'nmarl_net_step_dem'] * 4
    assert float(envs[0].transit.max()) > 0 and int(envs[0].t[0]) == t0 + 4
    if objective == 'hybrid':
        assert len(envs[0].state_tensors()) == 9 and float(envs[0].head_wait.max()) > 0


def test_dem_entry_refuses_a_bad_table():
    """NMARL_EINVAL for a NULL table and for a negative or non-finite entry, before any launch."""
    import ctypes
    from deeprl_network_amd import _lib
    env = make(MONACO, 3)
    env.reset(u0=torch.full((3, 4), 0.5, device='cuda'))
    before = [x.clone() for x in env.state_tensors()]
    P = _lib.ptr
    act = torch.zeros(3, env.n_agent, dtype=torch.uint8, device='cuda')

    def call(dem):
        return _lib.lib.nmarl_net_step_dem(ctypes.byref(env.params), ctypes.byref(env.topo.c), 3, P(act), P(env.q), P(env.transit),
                                           P(env.prev_action), P(env.t), P(env.xi), P(env.obs), P(env.reward), P(env.done),
                                           P(env.global_reward), 0, 12, 0, P(env.episode), _lib.stream(), dem)
    assert call(None) == -1
    for bad in (-1.0, float('nan'), float('inf')):
        dem = _lib.NetDemand()
        dem.act[3][11] = bad
        assert call(ctypes.byref(dem)) == -1, bad
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, env.state_tensors()))
    assert call(ctypes.byref(_lib.NetDemand())) == 0               # an all-zero table is a valid one: no demand
    torch.cuda.synchronize()
    assert int(env.t[0]) == 1 and float(env.transit.max()) == 0


# ------------------------------------------------------------------ the fixtures against the restatement
def run_trajectory(path, tp, E, coop_gamma, steps):
    from oracle import realnet_ref as R
    env = make(path, E, coop_gamma=coop_gamma)
    assert env.n_agent == tp.N and tuple(env.obs.shape) == (E, tp.N, tp.L * (1 + tp.m_max))
    rng = np.random.RandomState(E)
    U = rng.rand(E, 4).astype(np.float32)
    env.reset(u0=torch.from_numpy(U).cuda())
    ref = make_ref(env, tp)
    ref.reset(np.float32(0.8) + np.float32(0.4) * U)
    np.testing.assert_array_equal(env.xi.cpu().numpy(), ref.xi)
    for t in range(steps):
        hold = rng.rand(E, tp.N) < 0.6                    # keep the phase most of the time
        a = np.where(hold & (t > 0), ref.prev, F.rand_actions(rng, E, tp)).astype(np.uint8)
        obs, r, d, g = env.step(torch.from_numpy(a).cuda())
        ro, rr, rd, rg = ref.step(a)
        np.testing.assert_allclose(env.q.cpu().numpy(), ref.q, rtol=2e-4, atol=2e-3, err_msg='q t=%d' % t)
        np.testing.assert_allclose(env.transit.cpu().numpy(), ref.tr, rtol=2e-4, atol=2e-3, err_msg='tr t=%d' % t)
        np.testing.assert_allclose(obs.cpu().numpy(), R.gather_net(ro, tp), rtol=2e-4, atol=1e-3)
        np.testing.assert_allclose(g.cpu().numpy(), rg, rtol=2e-4, atol=5e-2)
        np.testing.assert_allclose(r.cpu().numpy(), rr, rtol=2e-4, atol=5e-2)
        assert np.array_equal(d.cpu().numpy().astype(bool), rd)
        assert np.array_equal(env.prev_action.cpu().numpy(), a)
    return env, ref


@pytest.mark.parametrize('E', [1, 9])
@pytest.mark.parametrize('coop_gamma', [-1, 0.9])
def test_small_trajectory_vs_restatement(nets, topos, E, coop_gamma):
    """200 steps (pieces 0..3 of the fixture's non-integer activity table) at the tolerances of test_trajectory_vs_oracle."""
    env, ref = run_trajectory(nets['small'], topos['small'], E, coop_gamma, 200)
    assert float(ref.q.max()) > 1 and float(ref.tr[:, 4, 0].max()) > 0        # traffic; the node without neighbours has its entry


def test_limits_trajectory_vs_restatement(nets, topos):
    """32 nodes, 24 links and 8 phases in one node, 4 neighbours in another: 20 steps at E = 9, the same tolerances."""
    env, ref = run_trajectory(nets['limits'], topos['limits'], 9, 0.9, 20)
    assert (env.topo.N, env.topo.L, env.topo.A, env.topo.m_max) == (32, 24, 8, 4) and float(ref.q.max()) > 0


def test_small_single_step_tight_from_random_state(nets, topos):
    """One step from identical random states, t anywhere in the episode (piece 11 and the step behind it included): the
    tolerances of tests/test_gpu_realnet.py::test_single_step_tight_from_random_state."""
    from oracle import realnet_ref as R
    E, tp = 512, topos['small']
    env = make(nets['small'], E)
    rng = np.random.RandomState(3)
    env.reset(u0=torch.from_numpy(rng.rand(E, 4).astype(np.float32)).cuda())
    ref = make_ref(env, tp)
    ref.reset(env.xi.cpu().numpy())
    random_state(ref, rng)
    ref.t[:8] = [0, 59, 60, 659, 660, 718, 719, 300]
    hand_over(env, ref)
    a = F.rand_actions(rng, E, tp).astype(np.uint8)
    obs, r, d, g = env.step(torch.from_numpy(a).cuda())
    ro, rr, rd, rg = ref.step(a)
    np.testing.assert_allclose(env.q.cpu().numpy(), ref.q, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(env.transit.cpu().numpy(), ref.tr, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(obs.cpu().numpy(), R.gather_net(ro, tp), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r.cpu().numpy(), rr, rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(g.cpu().numpy(), rg, rtol=1e-5, atol=2e-3)
    assert np.array_equal(d.cpu().numpy().astype(bool), rd) and rd[6] and not rd[5]
    last = ref.tr[3][tp.group >= 0]                                # t = 659 -> piece 10; replica 4: t = 660 -> piece 11, non-zero
    assert (ref.tr[4][tp.group >= 0] > 0).all() and (last > 0).any()


def test_small_episode_end_auto_reset_and_philox(nets):
    from oracle import philox
    E, base, seed = 40, 1000, 77
    env = make(nets['small'], E, env_id_base=base, seed=seed)
    env.reset()
    U0 = np.stack(philox.philox4x32(base + np.arange(E), 0, 0, 0, seed, 0), axis=-1)
    np.testing.assert_array_equal(env.xi.cpu().numpy(), np.float32(0.8) + np.float32(0.4) * philox.u01(U0))
    env.t.fill_(env.T - 1)
    a = torch.zeros(E, env.n_agent, dtype=torch.uint8, device='cuda')
    obs, r, d, g = env.step(a, auto_reset=True)
    assert d.all() and (env.t == 0).all() and (env.q == 0).all() and (env.transit == 0).all() and (obs == 0).all()
    assert (env.episode == 2).all()
    U1 = np.stack(philox.philox4x32(base + np.arange(E), 0, 1, 0, seed, 0), axis=-1)
    np.testing.assert_array_equal(env.xi.cpu().numpy(), np.float32(0.8) + np.float32(0.4) * philox.u01(U1))


# ------------------------------------------------------------------ objectives
@pytest.mark.parametrize('objective,coop_gamma,E', [('wait', -1, 9), ('hybrid', 0.9, 9), ('hybrid', -1, 1)])
def test_small_objectives_vs_the_wait_model(nets, topos, objective, coop_gamma, E):
    """tests/realnet_wait_ref.py's model on the fixture's topology and activity, 120 handed-over steps, at the tolerances of
    tests/test_gpu_realnet_objectives.py::test_handed_over_steps_vs_oracle: head_wait exactly but for links within 1e-5 of the
    threshold (at most 1e-3 of the valid entries), the rest at the single-step tolerances."""
    from oracle import realnet_ref as R
    tp = topos['small']
    env = make(nets['small'], E, objective=objective, coop_gamma=coop_gamma, coef_wait=COEF, flow_rate=500)
    assert env.head_wait is not None and env.params.objective == {'wait': 1, 'hybrid': 2}[objective]
    rng = np.random.RandomState(E)
    U = rng.rand(E, 4).astype(np.float32)
    env.reset(u0=torch.from_numpy(U).cuda())
    ref = make_ref(env, tp, objective)
    assert ref.p.flow_rate == 500
    ref.reset(np.float32(0.8) + np.float32(0.4) * U)
    n_excl = n_valid = 0
    hw_max = 0.0
    for t in range(120):
        hold = rng.rand(E, tp.N) < 0.6
        a = np.where(hold & (t > 0), ref.prev, F.rand_actions(rng, E, tp)).astype(np.uint8)
        hand_over(env, ref)
        obs, r, d, g = env.step(torch.from_numpy(a).cuda())
        ro, rr, rd, rg = ref.step(a)
        valid = np.broadcast_to(ref.valid, ref.hw.shape)
        excl = ref.near_threshold(1e-5) & valid
        hw, cmp = env.head_wait.cpu().numpy(), valid & ~excl
        assert np.array_equal(hw[cmp], ref.hw[cmp]), 't=%d: head_wait differs' % t
        assert np.all(hw[~valid] == 0)
        np.testing.assert_allclose(env.q.cpu().numpy(), ref.q, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(env.transit.cpu().numpy(), ref.tr, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(obs.cpu().numpy(), R.gather_net(ro, tp), rtol=1e-5, atol=1e-6)
        ok = ~excl.any(axis=(1, 2))
        np.testing.assert_allclose(g.cpu().numpy()[ok], rg[ok], rtol=2e-4, atol=5e-2)
        np.testing.assert_allclose(r.cpu().numpy()[ok], rr[ok], rtol=2e-4, atol=5e-2)
        n_excl += int(excl.sum()); n_valid += int(valid.sum())
        hw_max = max(hw_max, float(ref.hw.max()))
    assert n_excl <= 1e-3 * n_valid
    assert hw_max >= 20                                            # queues stood through red steps: not vacuous


# ------------------------------------------------------------------ rule agents and the recorder
def _rule_observations(rng, E, tp, row):
    """[E,N,row] f32: own vectors quantised to quarters (ties for the maximum are frequent) in the even replicas, continuous in the
    odd ones; other numbers behind the own vector."""
    x = rng.rand(E, tp.N, row).astype(np.float32) * 7.0
    x[0::2] = np.round(x[0::2] * 0.5) * 2.0
    return x


@pytest.mark.parametrize('agent', ['greedy', 'maxpressure'])
def test_batch_rule_controllers_equal_their_host_controllers(nets, topos, agent):
    from deeprl_network_amd.envs.greedy import GreedyBatchController
    from deeprl_network_amd.envs.maxpressure import MaxPressureBatchController
    E, tp = 67, topos['small']
    env = make(nets['small'], E, agent=agent)
    assert env.n_s_ls == tp.n_s_ls                                  # a rule agent reads its own links
    ctl = (GreedyBatchController if agent == 'greedy' else MaxPressureBatchController)(env)
    host = env.host_controller()
    x = _rule_observations(np.random.RandomState(5), E, tp, env.obs.shape[2])
    env.obs.copy_(torch.from_numpy(x))
    out = torch.full((E, tp.N), 255, dtype=torch.uint8, device='cuda')
    ctl.forward_batch(env.obs, out)
    got = out.cpu().numpy()
    ties = 0
    for e in range(E):
        own = [x[e, i, :tp.n_s_ls[i]].astype(np.float64) for i in range(tp.N)]
        assert host.forward(own) == got[e].tolist(), e
        if agent == 'greedy':                                       # and the rule itself, from the description
            for i in range(tp.N):
                flows = [sum(own[i][k] for k, ch in enumerate(ph) if ch == 'G') for ph in tp.phases[i]]
                assert got[e, i] == flows.index(max(flows))
                ties += flows.count(max(flows)) > 1
    assert agent != 'greedy' or ties > 20
    assert len(np.unique(got[:, 0])) == 3 and len(np.unique(got[:, 1])) == 2


def test_traffic_record_on_the_small_network(nets, topos):
    """TrafficRecorder rows == tests/traffic_record_ref.py given the fixture's own `mult` and demand (flow_rate x its activity)."""
    from traffic_record_ref import COLUMNS, TrafficRecordRef
    from deeprl_network_amd.envs.traffic_record import TrafficRecorder
    E, steps, tp = 5, 40, topos['small']
    env = make(nets['small'], E, flow_rate=411)
    rng = np.random.RandomState(100 + E)
    env.reset(u0=torch.from_numpy(rng.rand(E, 4).astype(np.float32)).cuda())
    env.t.fill_(640)                                               # pieces 10 and 11 of the table
    rec = TrafficRecorder(env, steps)
    mult = (np.arange(tp.L)[None, :] < np.array(tp.n_s_ls)[:, None]).astype(np.int32)
    demand = 411.0 * tp.activity
    assert np.array_equal(rec.mult_host, mult) and np.array_equal(rec.demand_host, demand)
    ref = TrafficRecordRef(mult, demand, E)
    rec.begin()
    for k in range(steps):
        env.step(torch.from_numpy(F.rand_actions(rng, E, tp).astype(np.uint8)).cuda())
        rec.step(k)
        want = ref.step(env.q.cpu().numpy(), env.transit.cpu().numpy(), env.t.cpu().numpy(), env.xi.cpu().numpy())
        got = rec.rec[k].cpu().numpy()
        for c, name in enumerate(COLUMNS):
            np.testing.assert_allclose(got[:, c], want[:, c], rtol=1e-6, atol=1e-6, err_msg='%s, step %d' % (name, k))
        assert np.array_equal(rec.stand.cpu().numpy(), ref.stand)
    rows = rec.rows()
    assert rows[-1, :, 0].min() > 1 and rows[:, :, 1].min() > 0 and rows[:, :, 5].max() > 0
    trip, want = rec.trip(), ref.trip(steps)
    for key in want:
        np.testing.assert_allclose(trip[key], want[key], rtol=1e-9, atol=1e-9, err_msg=key)


# ------------------------------------------------------------------ learned agents
@pytest.mark.parametrize('agent', ['ma2c_nc', 'ia2c_fp', 'ma2c_ic3'])
@pytest.mark.parametrize('name', ['small', 'uniform'])
def test_heterogeneous_nets_train_on_the_fixture_networks(nets, topos, name, agent):
    """The assertions of tests/test_gpu_realnet.py::test_heterogeneous_nets_train_on_the_network on the small network and on the
    uniform one (equal phase counts over unequal link counts: heterogeneous by the observation widths alone): E = 16, n_step 8,
    3 batches, captured graph: finite, identical across two runs, actions inside every agent's own set, padded parameters
    untouched."""
    from deeprl_network_amd.main import AGENTS
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    tp, outs = topos[name], []
    for rep in range(2):
        cp = F.config(nets[name], agent=agent, n_step=8)
        env = make(nets[name], 16, agent=agent)
        assert env.n_agent == tp.N and env.n_a_ls == tp.n_a_ls and env.n_feat_ls == tp.n_s_ls
        np.random.seed(5)
        model = AGENTS[agent](env.n_s_ls, env.n_a_ls, env.neighbor_mask, env.distance_mask, env.coop_gamma, 10 ** 9,
                              cp['MODEL_CONFIG'], seed=5, num_envs=16, device='cuda', n_feat_ls=env.n_feat_ls)
        assert not model.identical_agent and model.policy.hetero and model.policy.n_obs == env.obs.shape[2]
        pad0 = model.policy.params['pi_b'].detach().clone()
        tr = BatchedTrainer(env, model, Counter(10 ** 9, 10 ** 9, 10 ** 9), use_graph=True)
        for _ in range(3):
            tr.run_batch()
        torch.cuda.synchronize()
        acts = model.buf_act.cpu().numpy()
        for i, n in enumerate(env.n_a_ls):
            assert acts[:, :, i].max() < n
        flat = model.policy.params.flat
        assert torch.isfinite(flat).all()
        pb = model.policy.params['pi_b'].detach()
        for i, n in enumerate(env.n_a_ls):
            assert torch.equal(pb[i, n:], pad0[i, n:]) and (pb[i, n:] < -1e29).all()
        if model.policy.params.mask is not None:
            frozen = model.policy.params.mask == 0
            assert (model.policy.params.grad[frozen] == 0).all()
        outs.append(flat.clone())
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------ the CLI
def test_cli_greedy_on_the_corridor_batched_and_one_replica(tmp_path):
    """`main.py train` on config_greedy_netfile.ini sets the run directory up (the ini, the corridor's file beside it); `main.py
    evaluate` on it, 3 seeds, 200-s episodes, with and without --batched: the three CSVs with the reference's columns, and the
    same `_control.csv` rows."""
    import configparser
    import pandas as pd
    from deeprl_network_amd.main import main
    cp = configparser.ConfigParser()
    cp.read(os.path.join(F.ROOT, 'config', 'config_greedy_netfile.ini'))
    cp['ENV_CONFIG']['episode_length_sec'] = '200'
    cp['ENV_CONFIG']['net_file'] = os.path.join(F.ROOT, 'config', cp['ENV_CONFIG']['net_file'])
    ini = tmp_path / 'config_greedy_netfile.ini'
    with open(ini, 'w') as f:
        cp.write(f)
    tables = {}
    for mode in ('one', 'batched'):
        base = str(tmp_path / mode)
        main(['--base-dir', base, 'train', '--config-dir', str(ini)])
        assert os.path.isfile(os.path.join(base, 'data', 'corridor.json'))
        main(['--base-dir', base, 'evaluate', '--evaluation-seeds', '2000,2010,2020'] + (['--batched'] if mode == 'batched' else []))
        stem = os.path.join(base, 'eva_data', 'atsc_real_net_greedy_')
        tables[mode] = {n: pd.read_csv(stem + n + '.csv', index_col=0) for n in ('control', 'traffic', 'trip')}
        t = tables[mode]
        assert set(t['control'].columns) == CONTROL_CSV and set(t['traffic'].columns) == TRAFFIC_CSV and set(t['trip'].columns) == TRIP_CSV
        assert len(t['control']) == len(t['traffic']) == 3 * 40 and len(t['trip']) == 3
        assert all(len(a.split(',')) == 6 for a in t['control']['action'])           # the corridor's six nodes
    pd.testing.assert_frame_equal(tables['batched']['control'].reset_index(drop=True), tables['one']['control'].reset_index(drop=True),
                                  check_exact=True)
    assert len(set(tables['one']['control']['action'])) > 3 and (tables['one']['traffic']['number_departed_car'] > 0).all()

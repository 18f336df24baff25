"""CPU: the network description file of `scenario = atsc_real_net` (ENV_CONFIG net_file, envs/net_file.py): every rejection, the
built-in network written out as a file, the topology of the fixture networks against tests/net_file_fixtures.py, the rule agents'
tables against their host controllers, the learned agents' construction, and the run directory `main.py train` leaves."""
import copy
import os

import numpy as np
import pytest

import net_file_fixtures as F

ROOT = F.ROOT
NETWORKS = os.path.join(ROOT, 'config', 'networks')


def _topology(obj):
    from deeprl_network_amd.envs import net_file
    from deeprl_network_amd.envs.real_net_env import NetTopology
    return NetTopology('cpu', net_file.parse(obj))


def _edit(path, value, base=None):
    """A deep copy of the small fixture with the entry at `path` replaced (or removed: value = KeyError)."""
    obj = copy.deepcopy(F.SMALL if base is None else base)
    cur = obj
    for key in path[:-1]:
        cur = cur[key]
    if value is KeyError:
        del cur[path[-1]]
    else:
        cur[path[-1]] = value
    return obj


def _many_nodes(n):
    return {'nodes': {'k%02d' % i: {'phases': ['Gr', 'rG'], 'neighbors': ['k%02d' % ((i + 1) % n)] if n > 1 else []} for i in range(n)}}


NO_GROUP_3 = _edit(('nodes', 'n2', 'links'), ['n0', 2, 'n0'])         # group 3 keeps its positive activity and loses its only entry

REJECTED = [
    ('one node', _many_nodes(1), 'nodes'),
    ('33 nodes', _many_nodes(33), 'nodes'),
    ('unknown neighbour', _edit(('nodes', 'n2', 'neighbors'), ['nope']), "'n2'"),
    ('repeated neighbour', _edit(('nodes', 'n0', 'neighbors'), ['n1', 'n1']), "'n0'"),
    ('self neighbour', _edit(('nodes', 'n3', 'neighbors'), ['n1', 'n3']), "'n3'"),
    ('five neighbours', {'nodes': dict(_many_nodes(6)['nodes'], k00={'phases': ['Gr', 'rG'], 'neighbors': ['k01', 'k02', 'k03', 'k04', 'k05']})},
     "'k00'"),
    ('unequal phase strings', _edit(('nodes', 'n4', 'phases'), ['G', 'rr']), "'n4'"),
    ('other characters', _edit(('nodes', 'n4', 'phases'), ['G', 'y']), "'n4'"),
    ('one phase', _edit(('nodes', 'n4', 'phases'), ['G']), "'n4'"),
    ('nine phases', _edit(('nodes', 'n4', 'phases'), ['G'] * 9), "'n4'"),
    ('no link', _edit(('nodes', 'n4', 'phases'), ['', '']), "'n4'"),
    ('25 links', _edit(('nodes', 'n4', 'links'), KeyError, _edit(('nodes', 'n4', 'phases'), ['G' * 25, 'r' * 25])), "'n4'"),
    ('links of the wrong length', _edit(('nodes', 'n2', 'links'), ['n0', 3]), "'n2'"),
    ('feeder not listed', _edit(('nodes', 'n2', 'links'), ['n1', 3, 'n0']), "'n2'"),
    ('group 4', _edit(('nodes', 'n2', 'links'), ['n0', 4, 'n0']), "'n2'"),
    ('group -1', _edit(('nodes', 'n2', 'links'), ['n0', -1, 'n0']), "'n2'"),
    ('activity 3 x 12', _edit(('activity',), F.SMALL['activity'][:3]), 'activity'),
    ('activity 4 x 11', _edit(('activity',), [row[:11] for row in F.SMALL['activity']]), 'activity'),
    ('negative activity', _edit(('activity', 1, 5), -0.5), 'activity'),
    ('infinite activity', _edit(('activity', 1, 5), float('inf')), 'activity'),
    ('NaN activity', _edit(('activity', 1, 5), float('nan')), 'activity'),
    ('activity beyond float32', _edit(('activity', 1, 5), 1e39), 'activity'),
    ('activity without an entry', NO_GROUP_3, 'group 3'),
    ('nobody lists a neighbour', {'nodes': {n: {'phases': ['Gr', 'rG'], 'neighbors': []} for n in 'ab'}}, 'neighbour'),
]


@pytest.mark.parametrize('what,obj,names', REJECTED, ids=[r[0] for r in REJECTED])
def test_rejections_name_the_node_or_field(what, obj, names):
    from deeprl_network_amd.envs import net_file
    with pytest.raises(ValueError) as e:
        net_file.parse(obj)
    assert names in str(e.value), str(e.value)


def test_rejections_survive_the_file(tmp_path):
    """Through JSON text (which can spell NaN and Infinity), and a file that is no JSON at all."""
    from deeprl_network_amd.envs import net_file
    for bad in ('NaN', 'Infinity', '-1'):
        p = tmp_path / 'bad.json'
        p.write_text('{"nodes": {"a": {"phases": ["G", "r"], "neighbors": ["b"]}, "b": {"phases": ["G", "r"], "neighbors": []}},'
                     ' "activity": [[%s,0,0,0,0,0,0,0,0,0,0,0],[0,0,0,0,0,0,0,0,0,0,0,0],[0,0,0,0,0,0,0,0,0,0,0,0],'
                     '[0,0,0,0,0,0,0,0,0,0,0,0]]}' % bad)
        with pytest.raises(ValueError, match='activity'):
            net_file.load(str(p))
    p = tmp_path / 'text.json'
    p.write_text('not json')
    with pytest.raises(ValueError, match='text.json'):
        net_file.load(str(p))


def test_net_file_with_another_scenario_is_refused(tmp_path):
    from deeprl_network_amd.envs import init_env, make_batch_env, net_file
    path = F.write(tmp_path, F.SMALL)
    cp = F.config(path)
    cp['ENV_CONFIG']['scenario'] = 'atsc_large_grid'
    for build in (lambda: make_batch_env(cp['ENV_CONFIG'], num_envs=2), lambda: init_env(cp['ENV_CONFIG'])):
        with pytest.raises(ValueError, match='net_file'):
            build()
    with open(tmp_path / 'grid.ini', 'w') as f:
        cp.write(f)
    with pytest.raises(ValueError, match='net_file'):
        net_file.read_ini(str(tmp_path / 'grid.ini'))


def test_zero_activity_group_with_entries_is_fine_and_divides_by_nothing():
    """A group with external links and zero activity keeps its share; a group without an entry and without activity has none."""
    obj = _edit(('activity', 3), [0.0] * 12)
    with np.errstate(all='raise'):
        tp = _topology(obj)
        assert tp.host['ext_share'][F.Topo(obj).group == 3].tolist() == [1.0]
        obj = _edit(('activity', 3), [0.0] * 12, NO_GROUP_3)
        tp = _topology(obj)
    assert not (tp.host['group'] == 3).any() and np.isfinite(tp.host['ext_share']).all()


def test_monaco_file_is_the_built_in_network():
    """config/networks/monaco.json -- `links` and `activity` written out -- gives the built-in topology byte for byte."""
    import json
    from deeprl_network_amd.envs import net_file
    from deeprl_network_amd.envs.real_net_env import NetTopology
    from deeprl_network_amd.envs.traffic_record import net_demand
    path = os.path.join(NETWORKS, 'monaco.json')
    raw = json.load(open(path))
    assert len(raw['nodes']) == 28 and all('links' in nd for nd in raw['nodes'].values()) and 'activity' in raw
    a, b = NetTopology('cpu', net_file.load(path)), NetTopology('cpu')
    assert b.builtin and b.dem is None and not a.builtin and a.dem is not None
    assert a.node_names == b.node_names and a.phases == b.phases and a.nbrs == b.nbrs
    assert (a.N, a.L, a.A, a.m_max, a.n_a_ls, a.n_s_ls) == (b.N, b.L, b.A, b.m_max, b.n_a_ls, b.n_s_ls)
    assert set(a.host) == set(b.host)
    for key in b.host:
        assert a.host[key].dtype == b.host[key].dtype and a.host[key].tobytes() == b.host[key].tobytes(), key
    assert np.array_equal(a.neighbor_mask, b.neighbor_mask) and np.array_equal(a.distance_mask, b.distance_mask)
    assert a.dev['image'].numpy().tobytes() == b.dev['image'].numpy().tobytes()
    for flow_rate in (325.0, 411.7):
        assert (flow_rate * a.activity).tobytes() == net_demand(flow_rate).tobytes()
        assert (flow_rate * b.activity).tobytes() == net_demand(flow_rate).tobytes()
    assert [[a.dem.act[g][p] for p in range(12)] for g in range(4)] == a.activity.tolist()


def test_shipped_and_fixture_networks_parse():
    from deeprl_network_amd.envs import net_file
    c = net_file.load(os.path.join(NETWORKS, 'corridor.json'))
    assert 5 <= len(c.names) <= 6
    raw = __import__('json').load(open(os.path.join(NETWORKS, 'corridor.json')))
    nodes = raw['nodes'].values()       # every feature of the format: explicit and absent links, no neighbour, g, 2 and 3 phases, activity
    assert any('links' in nd for nd in nodes) and any('links' not in nd for nd in nodes) and any(not nd['neighbors'] for nd in nodes)
    assert any('g' in s for nd in nodes for s in nd['phases']) and {len(nd['phases']) for nd in nodes} >= {2, 3} and 'activity' in raw
    for ini in ('config_ma2c_nc_netfile.ini', 'config_greedy_netfile.ini'):
        cp = net_file.read_ini(os.path.join(ROOT, 'config', ini))
        assert cp['ENV_CONFIG']['net_file'] == os.path.join(NETWORKS, 'corridor.json')
    s, lim = _topology(F.SMALL), _topology(F.LIMITS)
    assert (s.N, s.m_max, sorted(s.n_s_ls), sorted(set(s.n_a_ls))) == (5, 2, [1, 2, 3, 5, 6], [2, 3])
    assert (lim.N, lim.L, lim.A, lim.m_max) == (32, 24, 8, 4) and lim.n_s_ls[1] == 24 and lim.n_a_ls[1] == 8 and len(lim.nbrs[0]) == 4


@pytest.mark.parametrize('name', ['small', 'limits'])
def test_topology_equals_the_independent_restatement(name):
    obj = {'small': F.SMALL, 'limits': F.LIMITS}[name]
    tp, ref = _topology(obj), F.Topo(obj)
    h = tp.host
    assert tp.node_names == ref.names and tp.n_s_ls == ref.n_s_ls and tp.n_a_ls == ref.n_a_ls and tp.nbrs == ref.nbrs
    assert np.array_equal(h['src'], ref.src) and np.array_equal(h['group'], ref.group) and np.array_equal(h['green'], ref.green)
    assert np.array_equal(h['fan'], ref.fan) and h['ext_share'].tobytes() == ref.ext_share.astype(np.float32).tobytes()
    assert np.array_equal(tp.neighbor_mask, ref.neighbor_mask) and np.array_equal(tp.distance_mask, ref.distance_mask)
    assert np.array_equal(tp.activity, ref.activity)
    for j in range(tp.N):
        pairs = [(int(v) >> 8, int(v) & 255) for v in h['dn_pair'][h['dn_ptr'][j]:h['dn_ptr'][j + 1]]]
        assert pairs == ref.dn[j], j
    if name == 'small':
        assert ref.fan.tolist() == [4, 5, 0, 2, 1] and not ref.nbrs[4] and {int(g) for g in ref.group[ref.group >= 0]} == {0, 1, 2, 3}
        assert (ref.green == 2).any() and ref.activity[:, 11].min() > 0 and (ref.activity != np.round(ref.activity)).any()
        rule = F.Topo({'nodes': {n: {k: v for k, v in nd.items() if k != 'links'} for n, nd in F.SMALL['nodes'].items()}})
        assert all((rule.src[i] != ref.src[i]).any() or (rule.group[i] != ref.group[i]).any() for i in range(ref.N))    # every `links` differs from the rule


def _observations(rng, tp, n):
    """n observation lists of small integers (ties for the maximum are frequent) and of continuous values."""
    for r in range(n):
        if r % 2:
            yield [rng.randint(0, 3, size=w).astype(np.float64) for w in tp.n_s_ls]
        else:
            yield [rng.rand(w) * 7 for w in tp.n_s_ls]


def test_rule_tables_equal_the_host_controllers_on_the_small_network():
    from deeprl_network_amd.envs.maxpressure import MaxPressureController, net_pressure_table
    from deeprl_network_amd.envs.real_net_env import RealNetController, net_greedy_table
    tp, ref = _topology(F.SMALL), F.Topo(F.SMALL)
    n_a, mask = net_greedy_table(tp.node_names, tp.phases)
    greedy = RealNetController(tp.node_names, tp.phases)
    table = net_pressure_table(tp)
    assert np.array_equal(table.n_a, n_a) and np.array_equal(table.mask, mask) and n_a.tolist() == ref.n_a_ls
    pressure = MaxPressureController(table)
    rng = np.random.RandomState(0)
    ties = 0
    for obs in _observations(rng, tp, 400):
        want_g, want_p = [], []
        for i in range(tp.N):
            counted = [[k for k, ch in enumerate(ph) if ch == 'G'] for ph in ref.phases[i]]
            assert [[k for k in range(tp.L) if (int(mask[i, a]) >> k) & 1] for a in range(n_a[i])] == counted
            flows = [sum(obs[i][k] for k in ks) for ks in counted]
            ties += flows.count(max(flows)) > 1
            want_g.append(flows.index(max(flows)))
            down = sum(obs[a][b] for a, b in ref.dn[i]) / len(ref.dn[i]) if ref.dn[i] else 0.0
            scores = [sum(obs[i][k] - down for k in ks) if ref.dn[i] else sum(obs[i][k] for k in ks) for ks in counted]
            want_p.append(scores.index(max(scores)))
        assert greedy.forward(obs) == want_g
        assert pressure.forward(obs) == want_p
    assert ties > 100


LEARNED = ('ia2c', 'ia2c_fp', 'ma2c_nc', 'ma2c_ic3', 'ma2c_cu', 'ma2c_dial')
BUILDS = [(a, 'small') for a in LEARNED] + [('ia2c_fp', 'limits'), ('ma2c_nc', 'limits')] + [(a, 'uniform') for a in LEARNED]


@pytest.mark.parametrize('agent,name', BUILDS, ids=['%s-%s' % b for b in BUILDS])
def test_learned_agents_build_on_the_fixture_networks(agent, name):
    """Every learned agent that builds on Monaco builds on the small network (two of them on the limits network too):
    heterogeneous, padded to the widest node, the most phases and the most neighbours.  On the uniform network -- equal phase
    counts over unequal link counts -- the agents are heterogeneous by their observation widths alone."""
    from cpu_emulation import cpu_ops
    from deeprl_network_amd.main import AGENTS
    tp = _topology({'small': F.SMALL, 'limits': F.LIMITS, 'uniform': F.UNIFORM}[name])
    cp = F.config(None, agent=agent, n_step=8)
    n_s_ls = list(tp.n_s_ls) if agent.startswith('ma2c') else [tp.n_s_ls[i] + sum(tp.n_s_ls[j] for j in tp.nbrs[i]) for i in range(tp.N)]
    with cpu_ops():
        np.random.seed(3)
        model = AGENTS[agent](n_s_ls, list(tp.n_a_ls), tp.neighbor_mask, tp.distance_mask, 0.9, 10 ** 6, cp['MODEL_CONFIG'], seed=3,
                              num_envs=2, device='cpu', n_feat_ls=list(tp.n_s_ls))
    p = model.policy
    assert p.hetero and not model.identical_agent
    assert (model.n_agent, model.n_a, p.n_feat, p.m_max) == {'small': (5, 3, 6, 2), 'limits': (32, 8, 24, 4), 'uniform': (3, 2, 6, 2)}[name]
    assert p.n_own == tp.n_s_ls
    assert p.n_obs == p.n_feat * (1 + p.m_max) and list(model.n_a_ls) == tp.n_a_ls
    pb = p.params['pi_b'].detach()
    for i, n in enumerate(tp.n_a_ls):
        assert bool((pb[i, n:] < -1e29).all()) and bool((pb[i, :n] > -1e29).all())


@pytest.mark.parametrize('agent', ['ma2c_nc', 'ia2c_fp', 'ia2c', 'ma2c_dial'])
@pytest.mark.parametrize('name', ['uniform', 'small'])
def test_batched_engine_on_file_networks_cpu(name, agent):
    """The batched engine's host logic on the CPU emulation (tests/test_trainer_cpu.py::test_heterogeneous_agents_on_the_network_cpu) on
    the small network and on the uniform one, whose env slab is 6 x (1 + 2) = 18 wide while agent 0 has 4 links: the rollout
    buffer takes the env's observation as it is, actions stay inside every agent's set, the padding is untouched."""
    import torch
    from cpu_emulation import cpu_ops
    from deeprl_network_amd.main import AGENTS
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    with cpu_ops():
        cp = F.config(None, agent=agent, n_step=6, episode_length_sec=60)        # T = 12 = 2 batches
        env = F.CpuFileNetBatchEnv({'uniform': F.UNIFORM, 'small': F.SMALL}[name], cp['ENV_CONFIG'], num_envs=3)
        np.random.seed(4)
        model = AGENTS[agent](env.n_s_ls, env.n_a_ls, env.neighbor_mask, env.distance_mask, env.coop_gamma, 10 ** 6,
                              cp['MODEL_CONFIG'], seed=4, num_envs=3, device='cpu', n_feat_ls=env.n_feat_ls)
        ps = model.policy.params
        assert model.policy.hetero and model.policy.n_obs == env.obs.shape[2]
        w0, pad0 = ps.flat.clone(), ps['pi_b'].detach().clone()
        tr = BatchedTrainer(env, model, Counter(10 ** 6, 10 ** 7, 10 ** 4), use_graph=False)
        for _ in range(5):
            tr.run_batch()
        acts, fp = model.buf_act.numpy(), model.buf_fp.numpy()
        for i, n in enumerate(env.n_a_ls):
            assert acts[:, :, i].max() < n and (fp[:, i, :, n:] == 0).all()
            np.testing.assert_allclose(fp[:, i, :, :n].sum(-1), 1.0, rtol=1e-5)
            assert torch.equal(ps['pi_b'].detach()[i, n:], pad0[i, n:])
        assert torch.isfinite(ps.flat).all() and not torch.equal(w0, ps.flat)
        if ps.mask is not None:
            assert torch.equal(ps.flat[ps.mask == 0], w0[ps.mask == 0])
        assert tr.stats()['episodes'] == 3 * 2
        # the one-replica API scatters an observation list into the same slab
        ob = [np.arange(1, w + 1, dtype=np.float64) for w in env.n_s_ls]
        if agent == 'ia2c_fp':
            ob = [np.concatenate([np.arange(1, w + 1, dtype=np.float64), np.zeros(w_fp)]) for w, w_fp in
                  zip(env.n_s_ls, [sum(env.n_a_ls[j] for j in env.topo.nbrs[i]) for i in range(env.n_agent)])]
        slab = model._obs_to_slab(ob)[0][0].numpy()
        assert slab.shape == (env.n_agent, env.obs.shape[2])


def test_default_phases_are_the_built_in_network_s_only():
    """RealNetController / net_greedy_table without `phases` serve the built-in network; other names are refused, not guessed."""
    from deeprl_network_amd.envs.real_net_env import RealNetController, net_greedy_table
    for build in (RealNetController, net_greedy_table):
        with pytest.raises(ValueError, match="'n0'"):
            build(['n0', 'n1'])
    with pytest.raises(ValueError, match='phases'):
        net_greedy_table(['n0', 'n1'], [('G', 'r')])


def test_train_leaves_a_run_directory_that_evaluate_can_open(tmp_path):
    """`main.py train` copies the network's file into <run>/data and names the copy in the run's ini (host code: a rule agent's
    `train` stops behind the set-up); the ini read back from the run resolves to the copy, which parses to the same network."""
    from deeprl_network_amd import main
    from deeprl_network_amd.envs import net_file
    src = tmp_path / 'cfg'
    (src / 'nets').mkdir(parents=True)
    F.write(src / 'nets', F.SMALL, 'small.json')
    cp = F.config('nets/small.json', agent='greedy')               # relative: against the ini's directory, not the working one
    with open(src / 'config_small.ini', 'w') as f:
        cp.write(f)
    base = tmp_path / 'run'
    main.main(['--base-dir', str(base), 'train', '--config-dir', str(src / 'config_small.ini')])
    copied = base / 'data' / 'small.json'
    assert copied.is_file() and copied.read_bytes() == (src / 'nets' / 'small.json').read_bytes()
    moved = tmp_path / 'elsewhere'
    os.rename(base, moved)                                         # the run names its copy relative to its own ini
    cfg = main._open_run(str(moved))
    assert cfg['ENV_CONFIG']['net_file'] == str(moved / 'data' / 'small.json')
    assert cfg['ENV_CONFIG']['agent'] == 'greedy' and cfg['ENV_CONFIG']['flow_rate'] == '325'
    got, want = net_file.load(cfg['ENV_CONFIG']['net_file']), net_file.parse(F.SMALL)
    assert got[:5] == want[:5] and np.array_equal(got.activity, want.activity)

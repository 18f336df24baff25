"""The `maxpressure` ATSC agent, the parts that need no GPU: the table builders and the host controller against the brute-force
restatement (tests/maxpressure_ref.py), its relation to the greedy controllers, the agent name in the envs' observation choice
and in `main.py train`."""
import configparser
import logging
import os

import numpy as np
import pytest

import maxpressure_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (groups, pairs) the issue pins: 4x8 has one group per directed edge of the lattice, 2 (4*7 + 8*3) = 104, a north / south approach
# one lane (48 pairs), an east / west approach two (112); the network 26 feeding nodes over 177 fed links, the longest group 13
COUNTS = {'grid4x8': (104, 160), 'net': (26, 177)}


def _net_topology():
    from deeprl_network_amd.envs.real_net_env import NetTopology
    return NetTopology('cpu')


@pytest.fixture(scope='module')
def tables():
    from deeprl_network_amd.envs.maxpressure import grid_pressure_table, net_pressure_table
    out = {'grid%dx%d' % rc: grid_pressure_table(*rc) for rc in ref.GRID_SHAPES}
    out['net'] = net_pressure_table(_net_topology())
    return out


def _spec(name):
    return ref.net_spec() if name == 'net' else ref.grid_spec(*(int(v) for v in name[4:].split('x')))


NAMES = ['grid%dx%d' % rc for rc in ref.GRID_SHAPES] + ['net']


def test_link_constants_are_the_oracle_s():
    from oracle import grid_ref as G
    from deeprl_network_amd.envs import maxpressure as M
    assert list(M.LINK_LANE) == list(G.LINK_LANE) and list(M.LINK_DEST) == list(G.LINK_DEST)
    assert [float(v) for v in M.LINK_SHARE] == [float(v) for v in G.LINK_SHARE]
    assert [M._LANE_FIRST_LINK[ln] for ln in range(6)] == [ref._first_link(ln) for ln in range(6)]


@pytest.mark.parametrize('name', NAMES)
def test_table_builders_equal_the_restatement(tables, name):
    """n_a / mask, every group's pairs in order, every (node, feature)'s terms in order with the float32 share: the host table,
    expanded, is the restatement's description; groups are numbered in ascending 4 j + approach (grid) / feeding node (network)."""
    from deeprl_network_amd.envs.maxpressure import check_pressure_table
    t, spec = tables[name], _spec(name)
    assert check_pressure_table(t) is t and t.n_feat == spec['F'] and len(t.n_a) == spec['N']
    phases, groups, terms = ref.expand(t)
    assert phases == spec['phases']
    order = sorted(spec['groups'], key=lambda key: 4 * key[0] + key[1] if isinstance(key, tuple) else key)
    index = {key: g for g, key in enumerate(order)}
    assert groups == {index[key]: pairs for key, pairs in spec['groups'].items()}
    want = {at: [(index[key], share) for key, share in cur] for at, cur in spec['terms'].items() if cur}
    assert set(terms) == set(want)
    for at, cur in want.items():
        assert [g for g, _ in terms[at]] == [g for g, _ in cur], at
        assert [w.tobytes() for _, w in terms[at]] == [np.float32(w).tobytes() for _, w in cur], at
    assert t.tgrp.dtype == np.int16 and t.tw.dtype == np.float32 and t.gptr.dtype == np.int32 and t.gpair.dtype == np.int16
    assert max(len(cur) for cur in want.values()) <= 3 and all(len(p) >= 1 for p in groups.values())
    if name in COUNTS:
        assert (len(groups), len(t.gpair)) == COUNTS[name]
    if name == 'grid4x8':
        assert max(len(cur) for cur in want.values()) == 3
    if name == 'net':
        assert max(len(p) for p in groups.values()) == 13
        assert all(len(cur) == 1 and cur[0][1] == np.float32(1.0) for cur in want.values())


def _own(name, row):
    """One row [N, F] f32 -> the list of own vectors the one-replica envs hand a controller (float64 copies)."""
    from oracle import realnet_ref as R
    x = row.astype(np.float64)
    return [x[i, :R.TOPO.n_s_ls[i]] for i in range(len(x))] if name == 'net' else list(x)


@pytest.mark.parametrize('name', ['grid1x2', 'grid3x3', 'grid5x5', 'grid4x8', 'net'])
def test_host_controller_equals_the_restatement(tables, name):
    from deeprl_network_amd.envs.maxpressure import MaxPressureController
    spec, obs, want = ref.case(name)
    ctl = MaxPressureController(tables[name])
    assert ctl.name == 'maxpressure' and ctl.n_step == 1 and ctl.reset() is None and ctl.load('anywhere/') is True
    for kind, rows in (('quantised', 120), ('uniform', 80), ('zero', 2)):
        for r in range(rows):
            assert ctl.forward(_own(name, obs[kind][r])) == want[kind][r].tolist(), (name, kind, r)
    assert not want['zero'].any()
    # the quantised rows do hold ties for the maximum (the first one must win), and the scores are the restatement's to the bit
    sc = ref.scores(spec, obs['quantised'][:120])
    tied = sum(int(((s == s.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum()) for s in sc)
    assert tied >= 1
    got = ctl.scores(_own(name, obs['uniform'][0]))
    for i, s in enumerate(ref.scores(spec, obs['uniform'][:1])):
        assert np.array(got[i]).tobytes() == s[0].tobytes(), (name, i)


def _greedy(name):
    from deeprl_network_amd.envs.large_grid_env import LargeGridController
    from deeprl_network_amd.envs.real_net_env import RealNetController
    from oracle import realnet_ref as R
    return RealNetController(R.TOPO.names) if name == 'net' else LargeGridController()


@pytest.mark.parametrize('name', ['grid3x3', 'grid5x5', 'net'])
def test_without_downstream_occupancy_it_is_the_greedy_controller(tables, name):
    from deeprl_network_amd.envs.maxpressure import MaxPressureController
    spec, obs, _ = ref.case(name)
    x = obs['quantised'][:150].copy()
    for pairs in spec['groups'].values():
        for j, f in pairs:
            x[:, j, f] = 0.0
    assert x.any()                                         # the links no node feeds keep their counts
    ctl, greedy = MaxPressureController(tables[name]), _greedy(name)
    assert len({tuple(greedy.forward(_own(name, row))) for row in x}) > 10
    for row in x:
        assert ctl.forward(_own(name, row)) == greedy.forward(_own(name, row))


@pytest.mark.parametrize('name', ['grid5x5', 'net'])
def test_it_is_another_controller_than_greedy_on_the_oracle(tables, name):
    """60 steps of the float32 oracle under max-pressure: greedy would have acted differently at least once (a condition; the
    prototype of the issue measured 27-36 % of all decisions over full episodes)."""
    from oracle import grid_ref as G
    from oracle import realnet_ref as R
    from deeprl_network_amd.envs.maxpressure import MaxPressureController
    if name == 'net':
        env = R.NetBatchRef(R.NetParams(norm_wave=1.0, clip_wave=-1, coop_gamma=-1), E=1, dtype=np.float32)
    else:
        env = G.GridBatchRef(G.GridParams(norm_wave=1.0, clip_wave=-1, coop_gamma=-1), E=1, dtype=np.float32)
    ctl, greedy = MaxPressureController(tables[name]), _greedy(name)
    ob = env.reset(np.ones((1, 4)))
    differ = total = 0
    for t in range(60):
        a = ctl.forward(_own(name, ob[0]))
        assert a == ref.rule(_spec(name), ob)[0].tolist()
        differ += sum(int(u != v) for u, v in zip(a, greedy.forward(_own(name, ob[0]))))
        total += len(a)
        ob, _, _, _ = env.step(np.array(a)[None, :])
    print('%s: max-pressure differs from greedy in %d of %d decisions' % (name, differ, total))
    assert differ >= 1


def test_bad_tables_are_refused(tables):
    from deeprl_network_amd import _lib
    from deeprl_network_amd.envs.maxpressure import check_pressure_table
    t = tables['grid3x3']
    bad_pair = t.gpair.copy()
    bad_pair[0, 0] = 9                                      # a node outside the grid
    bad_grp = t.tgrp.copy()
    bad_grp[0, 0, 0] = len(t.gptr) - 1                      # a group that does not exist
    empty = t.gptr.copy()
    empty[1] = 0                                            # an empty group
    for bad in (t._replace(gpair=bad_pair), t._replace(tgrp=bad_grp), t._replace(gptr=empty), t._replace(n_feat=11)):
        with pytest.raises(_lib.NmarlError):
            check_pressure_table(bad)


def test_agent_name_selects_own_row_observations():
    from deeprl_network_amd.envs import large_grid_env as L
    from deeprl_network_amd.envs import real_net_env as N
    assert 'maxpressure' in L.RULE_AGENTS and 'maxpressure' in N.RULE_AGENTS and 'greedy' in L.RULE_AGENTS
    for rows, cols in ((5, 5), (4, 8)):
        assert L.grid_n_s_ls('maxpressure', L.grid_masks(rows, cols)[0]) == [12] * (rows * cols)
    for name in ('config_maxpressure.ini', 'config_maxpressure_net.ini'):
        cp = configparser.ConfigParser()
        assert cp.read(os.path.join(ROOT, 'config', name))
        assert cp['ENV_CONFIG']['agent'] == 'maxpressure' and not cp.has_section('MODEL_CONFIG')
    # the grid ini is config_greedy.ini, the network ini config_ia2c_fp_net.ini's ENV_CONFIG, with the agent changed
    for name, base in (('config_maxpressure.ini', 'config_greedy.ini'), ('config_maxpressure_net.ini', 'config_ia2c_fp_net.ini')):
        a, b = configparser.ConfigParser(), configparser.ConfigParser()
        a.read(os.path.join(ROOT, 'config', name))
        b.read(os.path.join(ROOT, 'config', base))
        want = dict(b['ENV_CONFIG'])
        want['agent'] = 'maxpressure'
        assert dict(a['ENV_CONFIG']) == want


@pytest.mark.parametrize('ini', ['config_maxpressure.ini', 'config_maxpressure_net.ini'])
def test_train_refuses_the_rule_based_agent(tmp_path, caplog, ini):
    """`main.py train` on a max-pressure ini logs that there is nothing to train and returns."""
    from deeprl_network_amd.main import main
    with caplog.at_level(logging.ERROR):
        main(['--base-dir', str(tmp_path / 'run'), 'train', '--config-dir', os.path.join(ROOT, 'config', ini)])
    assert any('maxpressure' in r.getMessage() and 'rule-based controller' in r.getMessage() for r in caplog.records)
    assert not os.listdir(str(tmp_path / 'run' / 'model'))


def test_kernel_needs_no_scratch():
    """The compiler's own report for csrc/maxpressure.hip (gfx950): no scratch, no spills, within the static LDS limit -- the
    figures quoted in profiles/r17_maxpressure.txt."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import resource_usage
    finally:
        sys.path.pop(0)
    rows = {r['name']: r for r in resource_usage.usage(os.path.join(resource_usage.CSRC, 'maxpressure.hip'))}
    assert list(rows) == ['atsc_maxpressure_kernel'], sorted(rows)
    r = rows['atsc_maxpressure_kernel']
    print(r)
    assert r['ScratchSize [bytes/lane]'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0
    # 128 registers: four waves per SIMD, so four 256-thread blocks fit a compute unit beside their 4 x 34 KB of LDS
    assert r['VGPRs'] <= 128 and r['LDS Size [bytes/block]'] <= 65536

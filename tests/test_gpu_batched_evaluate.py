"""Batched evaluation on the device: nmarl_atsc_greedy against the host controllers, `main.py evaluate --batched` against the
one-replica evaluation (greedy: every cell of the three CSVs), replica independence of a learned policy, CACC early termination."""
import configparser
import os

import numpy as np
import pandas as pd
import pytest

import batched_eval_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [2000, 2010, 2020]


def _ini(name, **env):
    cp = configparser.ConfigParser()
    assert cp.read(os.path.join(ROOT, 'config', name))
    for k, v in env.items():
        cp['ENV_CONFIG'][k] = str(v)
    return cp


def _run_dir(base, cp, ini_name, with_model=False):
    """A finished run on disk: its ini under data/, and (with_model) a checkpoint of randomly initialised weights under model/."""
    os.makedirs(os.path.join(base, 'data'))
    os.makedirs(os.path.join(base, 'model'))
    with open(os.path.join(base, 'data', ini_name), 'w') as f:
        cp.write(f)
    if with_model:
        from deeprl_network_amd.envs import make_batch_env
        from deeprl_network_amd.main import init_agent
        np.random.seed(cp['ENV_CONFIG'].getint('seed'))
        env = make_batch_env(cp['ENV_CONFIG'], num_envs=1)
        init_agent(env, cp['MODEL_CONFIG'], 0, 0, num_envs=1).save(os.path.join(base, 'model') + '/', 0)
    return base


def _evaluate(base, seeds, batched):
    from deeprl_network_amd.main import main
    main(['--base-dir', base, 'evaluate', '--evaluation-seeds', ','.join(str(s) for s in seeds)] + (['--batched'] if batched else []))


def _tables(base, stem, names):
    return {n: pd.read_csv(os.path.join(base, 'eva_data', '%s_%s.csv' % (stem, n)), index_col=0) for n in names}


def _assert_same_tables(got, want, what):
    for name in want:
        assert list(got[name].columns) == list(want[name].columns), (what, name)
        assert len(got[name]) == len(want[name]), (what, name, len(got[name]), len(want[name]))
        pd.testing.assert_frame_equal(got[name].reset_index(drop=True), want[name].reset_index(drop=True), check_exact=True,
                                      obj='%s %s' % (what, name))


# ------------------------------------------------------------------ 5. the kernel
LAYOUTS = [('grid5x5', 12), ('grid5x5', 60), ('grid1x2', 12), ('grid4x8', 12), ('net', 24), ('net', 120)]


@pytest.mark.parametrize('name,row', LAYOUTS, ids=['%s-row%d' % lr for lr in LAYOUTS])
def test_greedy_kernel_equals_the_host_controller(name, row):
    """Every action of nmarl_atsc_greedy == LargeGridController.greedy / RealNetController.greedy, for E = 1, 5, 67 (and all
    2 000 drawn rows as one batch: more than one block).  row: 12 = compact grid observation, 60 = grid slab (the neighbours'
    vectors behind the own one hold other numbers), 24 = the network's own vectors as GreedyBatchController stages them, 120 = a
    network row of 24-float slots [own | 4 neighbours]."""
    import torch
    from deeprl_network_amd import ops
    n_a, mask, obs, want = ref.case(name)
    R, N, F = obs.shape
    full = np.random.RandomState(11).rand(R, N, row).astype(np.float32) * 7.0       # what lies behind the own vector is not read
    full[:, :, :F] = obs
    n_a_d = torch.from_numpy(n_a).cuda()
    mask_d = torch.from_numpy(mask.view(np.int32)).cuda()
    start = 0
    for E in (1, 5, 67, R):
        lo = 0 if E == R else start
        x = torch.from_numpy(full[lo:lo + E]).cuda()
        out = torch.full((E, N), 255, dtype=torch.uint8, device='cuda')
        ops.atsc_greedy(n_a_d, mask_d, x, out, a_max=int(n_a.max()))
        np.testing.assert_array_equal(out.cpu().numpy(), want[lo:lo + E], err_msg='%s row %d E %d' % (name, row, E))
        out.fill_(255)
        ops.atsc_greedy(n_a_d, mask_d, x, out)                                    # a_max = 8: the same actions
        np.testing.assert_array_equal(out.cpu().numpy(), want[lo:lo + E])
        start += E


def test_greedy_controller_on_the_network_env_s_own_observation_buffer():
    """The Monaco env's observation rows are 22 (1 + m_max) = 110 floats, no multiple of 4: GreedyBatchController stages the own
    vectors and still gives RealNetController's actions; on the grid env's slab it hands the buffer over as it is."""
    import torch
    from deeprl_network_amd.envs import make_batch_env
    from deeprl_network_amd.envs.greedy import GreedyBatchController
    for name, ini, kw in (('net', 'config_ia2c_fp_net.ini', dict(agent='greedy')), ('grid5x5', 'config_greedy.ini', {})):
        n_a, mask, obs, want = ref.case(name)
        E = 67
        env = make_batch_env(_ini(ini, **kw)['ENV_CONFIG'], num_envs=E)
        N, row = env.obs.shape[1:]
        assert row == (110 if name == 'net' else 60)
        F = min(obs.shape[2], row if name == 'grid5x5' else env.topo.L)
        full = np.random.RandomState(3).rand(E, N, row).astype(np.float32) * 7.0
        full[:, :, :F] = obs[:E, :, :F]
        env.obs.copy_(torch.from_numpy(full))
        ctl = GreedyBatchController(env)
        out = torch.full((E, N), 255, dtype=torch.uint8, device='cuda')
        ctl.forward_batch(env.obs, out)
        np.testing.assert_array_equal(out.cpu().numpy(), want[:E])
        assert ctl.forward([o[:w] for o, w in zip(obs[0].astype(np.float64), ref.net_widths())] if name == 'net'
                           else list(obs[0].astype(np.float64))) == want[0].tolist()


def test_greedy_kernel_rejects_bad_arguments():
    import torch
    from deeprl_network_amd import _lib
    n_a, mask, obs, _ = ref.case('grid5x5')
    n_a_d, mask_d = torch.from_numpy(n_a).cuda(), torch.from_numpy(mask.view(np.int32)).cuda()
    x = torch.from_numpy(obs[:4]).cuda()
    out = torch.full((4, 25), 255, dtype=torch.uint8, device='cuda')
    f = _lib.lib.nmarl_atsc_greedy
    P, s = (lambda t: t.data_ptr()), _lib.stream()
    assert f(4, 25, 5, P(n_a_d), P(mask_d), P(x), 12, P(out), s) == 0
    for E, N, A, na, m, o, row, act in ((4, 0, 5, P(n_a_d), P(mask_d), P(x), 12, P(out)),
                                        (4, 33, 5, P(n_a_d), P(mask_d), P(x), 12, P(out)),
                                        (4, 25, 5, P(n_a_d), P(mask_d), P(x), 6, P(out)),
                                        (4, 25, 5, P(n_a_d), P(mask_d), P(x), 12, None),
                                        (4, 25, 0, P(n_a_d), P(mask_d), P(x), 12, P(out)),
                                        (4, 25, 9, P(n_a_d), P(mask_d), P(x), 12, P(out)),
                                        (4, 25, 5, None, P(mask_d), P(x), 12, P(out)),
                                        (4, 25, 5, P(n_a_d), None, P(x), 12, P(out)),
                                        (4, 25, 5, P(n_a_d), P(mask_d), None, 12, P(out)),
                                        (4, 25, 5, P(n_a_d), P(mask_d), P(x), 0, P(out)),
                                        (0, 25, 5, P(n_a_d), P(mask_d), P(x), 12, P(out))):
        assert f(E, N, A, na, m, o, row, act, s) == -1, (E, N, A, row)
    torch.cuda.synchronize()
    out.fill_(255)
    for args in ((4, 0), (4, 33)):
        f(args[0], args[1], 5, P(n_a_d), P(mask_d), P(x), 12, P(out), s)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 255).all()                                       # nothing was launched


# ------------------------------------------------------------------ 6. greedy through the CLI
@pytest.mark.parametrize('scenario', ['grid', 'net'])
def test_cli_greedy_batched_equals_one_replica(tmp_path, scenario):
    """`main.py evaluate` with and without --batched on a greedy run directory, three seeds, T = 60: the three CSVs are equal
    cell for cell (both sides run the same env and recorder kernels on the same actions)."""
    if scenario == 'grid':
        cp, ini, stem = _ini('config_greedy.ini', episode_length_sec=300), 'config_greedy.ini', 'atsc_large_grid_greedy'
    else:
        cp, ini, stem = _ini('config_ia2c_fp_net.ini', agent='greedy', episode_length_sec=300), 'config_ia2c_fp_net.ini', \
            'atsc_real_net_greedy'
    one = _run_dir(str(tmp_path / 'one'), cp, ini)
    bat = _run_dir(str(tmp_path / 'bat'), cp, ini)
    _evaluate(one, SEEDS, batched=False)
    _evaluate(bat, SEEDS, batched=True)
    names = ('control', 'traffic', 'trip')
    want, got = _tables(one, stem, names), _tables(bat, stem, names)
    assert len(want['control']) == len(want['traffic']) == 3 * 60 and len(want['trip']) == 3
    _assert_same_tables(got, want, scenario)
    for n in names:                                                               # and as files
        f = os.path.join('eva_data', '%s_%s.csv' % (stem, n))
        assert open(os.path.join(bat, f)).read() == open(os.path.join(one, f)).read(), n
    # the seeds differ, and the controller acts on what it sees
    assert list(want['control']['reward'][:60]) != list(want['control']['reward'][60:120])
    assert len(set(want['control']['action'])) > 3


def test_one_captured_graph_writes_the_eager_tables(tmp_path):
    """BatchedEvaluator(use_graph=True) -- the T lock-steps as one hipGraph, replayed -- writes what the eager form writes, twice in
    a row (greedy on the grid, T = 60: library launches only inside)."""
    from deeprl_network_amd.envs import make_batch_env
    from deeprl_network_amd.envs.greedy import GreedyBatchController
    from deeprl_network_amd.utils import BatchedEvaluator
    cp = _ini('config_greedy.ini', episode_length_sec=300)
    text = {}
    for tag, use_graph in (('eager', False), ('graph', True)):
        env = make_batch_env(cp['ENV_CONFIG'], num_envs=3)
        out = tmp_path / tag
        out.mkdir()
        ev = BatchedEvaluator(env, GreedyBatchController(env), SEEDS, str(out) + '/', use_graph=use_graph)
        for _ in range(2):
            means = ev.run()
            cur = {n: open(str(out / ('atsc_large_grid_greedy_%s.csv' % n))).read() for n in ('control', 'traffic', 'trip')}
            assert text.setdefault('first', cur) == cur, tag
        assert len(means) == 3


# ------------------------------------------------------------------ 7. a learned policy
def _learned(kind):
    if kind == 'cacc':
        return _ini('config_ia2c_fp_catchup.ini', episode_length_sec=6), 'config_ia2c_fp_catchup.ini', 'catchup_ia2c_fp', \
            ('control', 'traffic')
    return _ini('config_ma2c_cnet_grid.ini', episode_length_sec=300), 'config_ma2c_cnet_grid.ini', 'atsc_large_grid_ma2c_ic3', \
        ('control', 'traffic', 'trip')


@pytest.mark.parametrize('kind', ['cacc', 'grid'])
def test_learned_policy_replicas_are_independent(tmp_path, kind):
    """IA2C-FP on CACC catch-up / CommNet on the 5x5 grid, random weights, T = 60: --batched over three seeds == three --batched
    runs of one seed each, cell for cell (a replica's episode depends on its seed alone, not on its position or on E)."""
    import shutil
    cp, ini, stem, names = _learned(kind)
    three = _run_dir(str(tmp_path / 'three'), cp, ini, with_model=True)
    _evaluate(three, SEEDS, batched=True)
    got = _tables(three, stem, names)
    T = 60
    assert len(got['control']) == 3 * T
    for k, seed in enumerate(SEEDS):
        single = str(tmp_path / ('single%d' % k))
        shutil.copytree(three, single, ignore=shutil.ignore_patterns('eva_data', 'eva_log'))
        _evaluate(single, [seed], batched=True)
        want = _tables(single, stem, names)
        part = {}
        for n in names:
            sel = got[n][got[n]['episode'] == k + 1].copy()
            sel['episode'] = sel['episode'] * 0 + 1
            part[n] = sel.astype(want[n].dtypes.to_dict())
        _assert_same_tables(part, want, '%s seed %d' % (kind, seed))
    # the three episodes differ (seeds reach the initial state and, on the grid, the action draws)
    c = got['control']
    assert list(c['reward'][c['episode'] == 1]) != list(c['reward'][c['episode'] == 2])


@pytest.mark.parametrize('kind', ['cacc', 'grid'])
def test_reset_state_is_the_one_replica_path_s(tmp_path, kind):
    """Replica e after BatchedEvaluator.reset == the one-replica env after reset(test_ind=e) in evaluation mode, bit for bit."""
    import torch
    from deeprl_network_amd.envs import init_env, make_batch_env
    from deeprl_network_amd.main import init_agent
    from deeprl_network_amd.utils import BatchedEvaluator
    cp, _, _, _ = _learned(kind)
    env = make_batch_env(cp['ENV_CONFIG'], num_envs=3)
    model = init_agent(env, cp['MODEL_CONFIG'], 0, 0, num_envs=3)
    ev = BatchedEvaluator(env, model, SEEDS, str(tmp_path) + '/')
    ev.reset()
    one = init_env(cp['ENV_CONFIG'], port=1)
    one.init_test_seeds(SEEDS)
    one.train_mode = False
    keys = ('h', 'v', 'u', 'v0_init', 't') if kind == 'cacc' else ('q', 'transit', 'xi', 't', 'prev_action')
    for e in range(3):
        one.reset(test_ind=e)
        for k in keys:
            a, b = getattr(env, k)[e].cpu().numpy(), getattr(one.batch, k)[0].cpu().numpy()
            assert a.tobytes() == b.tobytes(), (kind, e, k)
        assert env.obs[e].cpu().numpy().tobytes() == one.batch.obs[0].cpu().numpy().tobytes()
    if kind == 'grid':
        assert not torch.equal(env.xi[0], env.xi[1])                               # (the seeds reach the state)
    else:
        assert not torch.equal(env.h[0], env.h[1])


def test_cacc_first_reward_agrees_with_the_one_replica_evaluator(tmp_path):
    """CACC, IA2C-FP, random weights: the first control row of every episode of --batched agrees with the one-replica Evaluator's
    to rtol 1e-4 (the project's NN-forward tolerance; the policies go through different launches, so later rows may differ after
    an arg-max flip and are not compared).  Same rows, clock and episode numbers on both sides."""
    import shutil
    cp, ini, stem, names = _learned('cacc')
    bat = _run_dir(str(tmp_path / 'bat'), cp, ini, with_model=True)
    one = str(tmp_path / 'one')
    shutil.copytree(bat, one)
    _evaluate(bat, SEEDS, batched=True)
    _evaluate(one, SEEDS, batched=False)
    got, want = _tables(bat, stem, names), _tables(one, stem, names)
    for n in names:
        assert list(got[n].columns) == list(want[n].columns)
    g1, w1 = got['control'][got['control']['step'] == 1], want['control'][want['control']['step'] == 1]
    assert list(g1['episode']) == list(w1['episode']) == [1, 2, 3]
    print('first rewards: batched %r one-replica %r' % (list(g1['reward']), list(w1['reward'])))
    np.testing.assert_allclose(g1['reward'].to_numpy(), w1['reward'].to_numpy(), rtol=1e-4)
    assert list(got['control']['time_sec'][:60]) == list(want['control']['time_sec'][:60])
    # row 0 of the traffic table is the state after the reset: bit-identical
    t0g, t0w = got['traffic'][got['traffic']['time_sec'] == 0], want['traffic'][want['traffic']['time_sec'] == 0]
    pd.testing.assert_frame_equal(t0g.reset_index(drop=True), t0w.reset_index(drop=True), check_exact=True)


# ------------------------------------------------------------------ 8. CACC early termination
def test_cacc_collision_stops_that_replica_s_tables(tmp_path):
    """T = 120, batch_size 60: replica 1 of 3 is given a headway under the collision threshold before the first step.  It
    collides at step 1 and is done at the batch boundary, step 60: 60 control rows, 61 traffic rows.  The other two replicas'
    tables equal those of a run without it."""
    from deeprl_network_amd.envs import make_batch_env
    from deeprl_network_amd.main import init_agent
    from deeprl_network_amd.utils import BatchedEvaluator
    cp, _, stem, names = _learned('cacc')
    cp['ENV_CONFIG']['episode_length_sec'] = '12'
    res = {}
    for tag in ('plain', 'hit'):
        np.random.seed(12)
        env = make_batch_env(cp['ENV_CONFIG'], num_envs=3)
        assert env.T == 120 and env.batch_size == 60
        model = init_agent(env, cp['MODEL_CONFIG'], 0, 0, num_envs=3)
        out = tmp_path / tag
        out.mkdir()
        ev = BatchedEvaluator(env, model, SEEDS, str(out) + '/')
        ev.reset()
        if tag == 'hit':
            env.h[1, 3] = 0.5                                                      # headway_min = 1
        means = ev.run_episode()
        assert len(means) == 3
        res[tag] = {n: pd.read_csv(str(out / ('%s_%s.csv' % (stem, n))), index_col=0) for n in names}
    plain, hit = res['plain'], res['hit']
    assert [int((plain['control']['episode'] == e).sum()) for e in (1, 2, 3)] == [120, 120, 120]
    assert [int((hit['control']['episode'] == e).sum()) for e in (1, 2, 3)] == [120, 60, 120]
    assert [int((hit['traffic']['episode'] == e).sum()) for e in (1, 2, 3)] == [121, 61, 121]
    c1 = hit['control'][hit['control']['episode'] == 2]
    assert list(c1['step']) == list(range(1, 61)) and (c1['reward'] == -8000.0).all()      # -G for each of the 8 vehicles
    for n in names:
        for e in (1, 3):
            a, b = hit[n][hit[n]['episode'] == e], plain[n][plain[n]['episode'] == e]
            pd.testing.assert_frame_equal(a.reset_index(drop=True), b.reset_index(drop=True), check_exact=True)

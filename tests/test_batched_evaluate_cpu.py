"""Batched evaluation, the parts that need no GPU: the greedy tables against the host controllers, the seed -> uniform maps, the
assembly of the CSV tables from per-step buffers, the CLI flag."""
import types

import numpy as np
import pandas as pd
import pytest

import batched_eval_ref as ref


# ------------------------------------------------------------------ 1. the (n_a, mask) tables
@pytest.mark.parametrize('name', ['grid5x5', 'grid1x2', 'grid4x8', 'net'])
def test_greedy_table_restates_the_host_controller(name):
    """The rule of nmarl_atsc_greedy, restated in NumPy on the table, gives exactly LargeGridController.greedy /
    RealNetController.greedy on 2 000 rows per node; ties for the maximum are frequent in them (measured when the generator was
    chosen: 19 % of the rows on the grid, 6.6 % on the network), so the first-maximum rule is exercised."""
    n_a, mask, obs, want = ref.case(name)
    assert obs.shape[0] == 2000 and mask.shape == (obs.shape[1], 8) and mask.dtype == np.uint32 and n_a.dtype == np.int32
    assert set(np.unique(obs * 4)) <= set(range(9))
    share = ref.tie_share(n_a, mask, obs)
    print('%s: tie share %.4f' % (name, share))
    assert share >= 0.05
    np.testing.assert_array_equal(ref.greedy_rule(n_a, mask, obs), want)


def test_grid_table_is_the_five_first_link_pairs():
    from deeprl_network_amd.envs.large_grid_env import grid_greedy_table
    want = [sum(1 << k for k in s) for s in ((0, 6), (5, 11), (3, 9), (3, 5), (9, 11))] + [0, 0, 0]
    for rows, cols in ref.GRID_SHAPES:
        n_a, mask = grid_greedy_table(rows, cols)
        assert n_a.tolist() == [5] * (rows * cols)
        assert all(row.tolist() == want for row in mask)


def test_net_table_counts_capital_g_only():
    from deeprl_network_amd.envs.real_net_env import NODE_DEFS, PHASE_SETS, net_greedy_table
    names = ref.net_names()
    n_a, mask = net_greedy_table(names)
    key = {name: k for name, k, _ in NODE_DEFS}
    for i, name in enumerate(names):
        phases = PHASE_SETS[key[name]]
        assert n_a[i] == len(phases) and not mask[i, len(phases):].any()
        for a, phase in enumerate(phases):
            assert [(int(mask[i, a]) >> k) & 1 for k in range(24)] == [int(ch == 'G') for ch in phase.ljust(24, 'r')]
    assert any('g' in ph for p in PHASE_SETS.values() for ph in p)          # (a permitted green exists, and is not counted)


# ------------------------------------------------------------------ 2. seeds -> uniforms
def test_eval_uniforms_depend_on_the_seed_alone():
    from deeprl_network_amd.utils import cacc_eval_u0, eval_uniforms
    seeds = [2000, 2010, 2020, 2030]
    T, N = 7, 5
    u = eval_uniforms(seeds, T, N)
    assert u.shape == (T, 4, N) and u.dtype == np.float32
    for e, s in enumerate(seeds):
        np.testing.assert_array_equal(u[:, e], np.random.RandomState(s).random_sample((T, N)).astype(np.float32))
    perm = [2, 0, 3, 1]
    up = eval_uniforms([seeds[k] for k in perm], T, N)
    for pos, k in enumerate(perm):
        np.testing.assert_array_equal(up[:, pos], u[:, k])
    ux = eval_uniforms(seeds + [5, 6, 7], T, N)
    np.testing.assert_array_equal(ux[:, :4], u)

    u0 = cacc_eval_u0(seeds, run_seed=12)
    assert u0.tolist() == [np.random.RandomState(s).rand() for s in seeds]
    assert cacc_eval_u0([seeds[k] for k in perm], run_seed=12).tolist() == [u0[k] for k in perm]
    assert cacc_eval_u0(seeds + [1, 2], run_seed=12)[:4].tolist() == u0.tolist()
    # the one-replica reset draws only while its running seed is not 0 (CACCEnv.reset): episode 2 of a run seeded -2 takes 0.5
    assert cacc_eval_u0(seeds, run_seed=-2).tolist() == [u0[0], 0.5, u0[2], u0[3]]


# ------------------------------------------------------------------ 3. table assembly
def _buffers(T, E, N, n_a, seed=3):
    rng = np.random.RandomState(seed)
    acts = rng.randint(0, n_a, size=(T, E, N)).astype(np.uint8)
    G = (-rng.rand(T, E) * 100).astype(np.float32)
    return acts, G


def test_row_counts_stop_at_the_first_done():
    from deeprl_network_amd.utils import eval_row_counts
    D = np.zeros((6, 4), dtype=np.uint8)
    D[5, 0] = 1
    D[2, 1] = D[4, 1] = D[5, 1] = 1
    D[0, 2] = 1
    rows, finished = eval_row_counts(D)
    assert rows.tolist() == [6, 3, 1, 6] and finished.tolist() == [True, True, True, False]


def test_atsc_tables_equal_the_one_replica_writers(tmp_path):
    """Synthetic buffers of 3 replicas x 4 steps through the batched assembly == the same episodes, one after another, through
    the statements of LargeGridEnv.step, EpisodeRecord.collect and write_tables: columns, row order, every cell."""
    from deeprl_network_amd.envs.traffic_record import EpisodeRecord, write_tables
    from deeprl_network_amd.utils import eval_atsc_tables, eval_control_rows, eval_row_counts
    T, E, N = 4, 3, 25
    acts, G = _buffers(T, E, N, 5)
    D = np.zeros((T, E), dtype=np.uint8)
    D[T - 1] = 1
    rng = np.random.RandomState(5)
    rec = rng.rand(T, E, 8).astype(np.float32)
    rec[:, :, 7] = (5 * np.arange(1, T + 1))[:, None]
    trip = {'depart_sec': np.zeros(E, dtype=np.int64), 'arrival_sec': 5 * np.full(E, T), 'duration_sec': rng.rand(E),
            'wait_step': rng.rand(E), 'wait_sec': rng.rand(E)}
    rows, _ = eval_row_counts(D)
    control = eval_control_rows(acts, G, rows, True, 5)
    traffic, trips = eval_atsc_tables(rec, trip, rows)

    env = types.SimpleNamespace(control_data=[], traffic_data=[], trip_data=[], cur_episode=0, control_interval_sec=5,
                                output_path=str(tmp_path) + '/', name='atsc_large_grid', agent='greedy')
    for e in range(E):
        env.cur_episode += 1
        for k in range(T):
            action, global_reward, t = acts[k, e], float(G[k, e]), k + 1
            sec = int(t) * env.control_interval_sec                                       # LargeGridEnv.step
            env.control_data.append({'episode': env.cur_episode, 'time_sec': sec, 'step': sec / env.control_interval_sec,
                                     'action': ','.join('%d' % x for x in action), 'reward': global_reward})
        er = EpisodeRecord.__new__(EpisodeRecord)
        er.env, er.slot = env, T
        er.recorder = types.SimpleNamespace(rows=lambda e=e: rec[:, e:e + 1], trip=lambda e=e: {k: v[e:e + 1] for k, v in trip.items()})
        er.collect(env.traffic_data, env.trip_data)
    write_tables(env)
    stem = env.output_path + 'atsc_large_grid_greedy_'
    for name, got in (('control', control), ('traffic', traffic), ('trip', trips)):
        pd.DataFrame(got).to_csv(str(tmp_path / 'b.csv'))
        assert open(str(tmp_path / 'b.csv')).read() == open(stem + name + '.csv').read(), name
    assert list(pd.DataFrame(control).columns) == ['episode', 'time_sec', 'step', 'action', 'reward']
    assert [r['episode'] for r in control] == [1] * T + [2] * T + [3] * T


def _todays_cacc_traffic(hist, rewards, cur_episode, dt, n_agent):
    """A literal copy of CACCEnv._log_traffic_data's statements as they stood before the function was shared."""
    hist = np.array(hist)
    hs, vs, us = hist[:, 0], hist[:, 1], hist[:, 2]
    df = pd.DataFrame()
    df['episode'] = np.ones(len(hs)) * cur_episode
    df['time_sec'] = np.arange(len(hs)) * dt
    df['reward'] = np.array(rewards)
    df['lead_headway_m'] = hs[:, 0]
    df['avg_headway_m'] = np.mean(hs[:, 1:], axis=1)
    df['std_headway_m'] = np.std(hs[:, 1:], axis=1)
    df['avg_speed_mps'] = np.mean(vs, axis=1)
    df['std_speed_mps'] = np.std(vs, axis=1)
    df['avg_accel_mps2'] = np.mean(us, axis=1)
    df['std_accel_mps2'] = np.std(us, axis=1)
    for i in range(n_agent):
        df['headway_%d_m' % (i + 1)] = hs[:, i]
        df['velocity_%d_mps' % (i + 1)] = vs[:, i]
        df['accel_%d_mps2' % (i + 1)] = us[:, i]
    return df


def test_cacc_tables_equal_the_one_replica_writers():
    """CACC: 3 replicas x 6 steps, replica 1 done at step 3 (a collision at a batch boundary): its control rows and its traffic
    table stop there; the shared traffic function equals a literal copy of today's statements; CACCEnv._log_traffic_data goes
    through it."""
    from deeprl_network_amd.envs.cacc_env import CACCEnv, cacc_traffic_table
    from deeprl_network_amd.utils import eval_cacc_traffic, eval_control_rows, eval_row_counts
    T, E, N, dt = 6, 3, 8, 0.1
    acts, G = _buffers(T, E, N, 4)
    D = np.zeros((T, E), dtype=np.uint8)
    D[T - 1] = 1
    D[2, 1] = 1
    hist = np.random.RandomState(9).rand(T + 1, E, 3, N).astype(np.float32)
    rows, finished = eval_row_counts(D)
    assert rows.tolist() == [6, 3, 6]
    control = eval_control_rows(acts, G, rows, False, dt)
    tables = eval_cacc_traffic(hist, G, rows, finished, dt)
    assert len(tables) == E and [len(t) for t in tables] == [7, 4, 7]

    want_control = []
    for e in range(E):
        n = int(rows[e])
        h64 = [hist[k, e].astype(np.float64) for k in range(n + 1)]                       # CACCEnv._phys per step
        rewards = [0] + [float(G[k, e]) for k in range(n)]
        want = _todays_cacc_traffic(h64, rewards, e + 1, dt, N)
        pd.testing.assert_frame_equal(tables[e], want, check_exact=True)
        pd.testing.assert_frame_equal(cacc_traffic_table(h64, rewards, e + 1, dt, N), want, check_exact=True)
        env = CACCEnv.__new__(CACCEnv)                                                     # the one-replica writer itself
        env._hist, env._rewards, env.cur_episode, env.dt, env.n_agent, env.traffic_data = h64, rewards, e + 1, dt, N, []
        env._log_traffic_data()
        pd.testing.assert_frame_equal(env.traffic_data[0], want, check_exact=True)
        for k in range(n):
            t = k + 1                                                                      # CACCEnv.step
            want_control.append({'episode': e + 1, 'time_sec': int(t) * dt, 'step': int(t),
                                 'action': ','.join('%d' % x for x in acts[k, e]), 'reward': float(G[k, e])})
    assert control == want_control
    assert list(pd.DataFrame(control).columns) == ['episode', 'time_sec', 'step', 'action', 'reward']
    # a replica without a done writes no traffic table (the one-replica env logs it `if done`)
    assert len(eval_cacc_traffic(hist, G, rows, np.array([True, False, True]), dt)) == 2


# ------------------------------------------------------------------ 4. the CLI flag
def test_parse_args_batched_flag():
    from deeprl_network_amd.main import parse_args
    args = parse_args(['evaluate', '--batched'])
    assert args.option == 'evaluate' and args.batched is True
    assert parse_args(['evaluate']).batched is False
    assert parse_args(['evaluate', '--batched', '--evaluation-seeds', '1,2']).evaluation_seeds == '1,2'

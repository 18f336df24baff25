"""Shared by tests/test_batched_evaluate_cpu.py and tests/test_gpu_batched_evaluate.py: the greedy rule of nmarl_atsc_greedy
restated in NumPy on the (n_a, mask) table, the observation generator of its tests, and the host controllers' answers."""
import functools

import numpy as np

GRID_SHAPES = ((5, 5), (1, 2), (4, 8))
ROWS = 2000                      # observation rows drawn per node


def greedy_rule(n_a, mask, obs):
    """obs [R, N, F] f32 (node i's own wave vector leads obs[r, i]) -> actions [R, N]: score_a = sum of (double) obs_k over the
    set bits k of mask[i][a], k ascending from 0; the smallest a < n_a[i] with the largest score."""
    R, N, F = obs.shape
    x = obs.astype(np.float64)
    out = np.zeros((R, N), dtype=np.uint8)
    for i in range(N):
        score = np.zeros((R, int(n_a[i])))
        for a in range(int(n_a[i])):
            s = np.zeros(R)
            for k in range(min(F, 24)):
                if (int(mask[i, a]) >> k) & 1:
                    s = s + x[:, i, k]
            score[:, a] = s
        out[:, i] = np.argmax(score, axis=1)              # the first maximum
    return out


def tie_share(n_a, mask, obs):
    """Share of the (row, node) pairs whose maximal score is reached by more than one phase."""
    R, N, F = obs.shape
    x = obs.astype(np.float64)
    ties = 0
    for i in range(N):
        bits = np.array([[(int(mask[i, a]) >> k) & 1 for k in range(F)] for a in range(int(n_a[i]))], dtype=np.float64)
        score = x[:, i, :] @ bits.T                        # (exact: multiples of 0.25, small sums)
        ties += int(((score == score.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    return ties / float(R * N)


def draw_obs(n_node, n_feat, rows=ROWS, seed=0):
    """[rows, N, n_feat] f32 with entries in multiples of 0.25 in [0, 2]: ties for the maximum are frequent."""
    rng = np.random.RandomState(1234 + seed)
    return (rng.randint(0, 9, size=(rows, n_node, n_feat)) * 0.25).astype(np.float32)


def net_names():
    from deeprl_network_amd.envs.real_net_env import NODE_DEFS
    return sorted(name for name, _, _ in NODE_DEFS)


def net_widths():
    from deeprl_network_amd.envs.real_net_env import NODE_DEFS, PHASE_SETS
    key = {name: k for name, k, _ in NODE_DEFS}
    return [len(PHASE_SETS[key[name]][0]) for name in net_names()]


@functools.lru_cache(maxsize=None)
def case(name):
    """name: 'grid5x5' | 'grid1x2' | 'grid4x8' | 'net' -> (n_a, mask, obs [ROWS, N, F], host controller's actions [ROWS, N]);
    computed once and shared (callers do not modify it).  F = 12 on the grid, 24 on the network, where the entries past a node's
    own links are 0 as in the env's padded observation."""
    if name.startswith('grid'):
        from deeprl_network_amd.envs.large_grid_env import LargeGridController, grid_greedy_table
        rows, cols = (int(v) for v in name[4:].split('x'))
        n_a, mask = grid_greedy_table(rows, cols)
        obs = draw_obs(rows * cols, 12, seed=rows * 100 + cols)
        host = LargeGridController()
        want = np.array([host.forward(list(ob)) for ob in obs.astype(np.float64)], dtype=np.uint8)
    else:
        from deeprl_network_amd.envs.real_net_env import RealNetController, net_greedy_table
        names, widths = net_names(), net_widths()
        n_a, mask = net_greedy_table(names)
        obs = draw_obs(len(names), 24, seed=7)
        for i, w in enumerate(widths):
            obs[:, i, w:] = 0.0
        host = RealNetController(names)
        x = obs.astype(np.float64)                         # (the env hands the controller float64 copies of its float32 rows)
        want = np.array([host.forward([ob[i, :widths[i]] for i in range(len(names))]) for ob in x], dtype=np.uint8)
    return n_a, mask, obs, want

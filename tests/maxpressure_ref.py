"""Shared by tests/test_maxpressure_cpu.py and tests/test_gpu_maxpressure.py: the max-pressure rule of DESIGN.md 6 restated by brute
force in NumPy, straight from the constants of oracle/grid_ref.py (LINK_DEST / LINK_LANE / LINK_SHARE / LANE_APPROACH) and from
oracle/realnet_ref.py's Topology (src, phases).  It does NOT use the host's table builders (envs/maxpressure.py): a scenario is
described here by names -- a downstream group is named (node, approach) on the grid and the feeding node on the network --, and
the tests expand the host's tables into the same form to compare them.

    spec = {'N', 'F', 'phases': per node, per phase: its counted features, ascending,
            'groups': {name: [(node, feature), ...]},                       # the order of the sum
            'terms':  {(node, feature): [(group name, float32 share), ...]}}   # the order of the subtractions
"""
import functools

import numpy as np

from oracle import grid_ref as G
from oracle import realnet_ref as R

# the five phases of the grid's rule-based agents as sets of lanes [N, E lane 0, E lane 1, S, W lane 0, W lane 1]
# (large_grid_env.py:25-26 of the reference: N+S through, E+W left, E+W through, E approach, W approach)
GRID_PHASE_LANES = ((0, 3), (2, 5), (1, 4), (1, 2), (4, 5))
GRID_SHAPES = ((1, 2), (2, 2), (3, 3), (5, 5), (4, 8), (1, 32))


def _first_link(lane):
    return int(np.where(G.LINK_LANE == lane)[0][0])


def grid_spec(rows, cols):
    N = rows * cols
    phases = [[sorted(_first_link(lane) for lane in lanes) for lanes in GRID_PHASE_LANES] for _ in range(N)]
    groups, terms = {}, {}
    for i in range(N):
        r, c = divmod(i, cols)
        for lane in range(G.N_LANE):
            cur = []
            for k in range(G.N_LINK):                                  # the lane's links, ascending
                if G.LINK_LANE[k] != lane:
                    continue
                dr, dc, ap = G.LINK_DEST[k]
                rr, cc = r + dr, c + dc
                if not (0 <= rr < rows and 0 <= cc < cols):
                    continue                                           # leaves the lattice: contributes nothing
                j = rr * cols + cc
                cur.append(((j, ap), np.float32(G.LINK_SHARE[k])))
                groups[(j, ap)] = [(j, _first_link(ln)) for ln in range(G.N_LANE) if G.LANE_APPROACH[ln] == ap]
            terms[(i, _first_link(lane))] = cur
    return dict(N=N, F=G.N_LINK, phases=phases, groups=groups, terms=terms)


def net_spec(topo=R.TOPO):
    N = topo.N
    phases = [[[k for k, ch in enumerate(s) if ch == 'G'] for s in topo.phases[i]] for i in range(N)]
    groups, terms = {}, {}
    for j in range(N):
        fed = [(i, k) for i in range(N) for k in range(topo.n_s_ls[i]) if topo.src[i, k] == j]
        if fed:
            groups[j] = fed
            for k in range(topo.n_s_ls[j]):
                terms[(j, k)] = [(j, np.float32(1.0))]
    return dict(N=N, F=topo.L, phases=phases, groups=groups, terms=terms)


def scores(spec, obs):
    """obs [R, N, >= F] f32 -> per node the [R, n_a] float64 scores, every operation in the order of the specification."""
    x = np.asarray(obs, dtype=np.float32).astype(np.float64)
    rows = x.shape[0]
    occ = {}
    for name, pairs in spec['groups'].items():
        s = np.zeros(rows)
        for j, f in pairs:
            s = s + x[:, j, f]
        occ[name] = s / np.float64(len(pairs))
    out = []
    for i in range(spec['N']):
        sc = np.zeros((rows, len(spec['phases'][i])))
        for a, feats in enumerate(spec['phases'][i]):
            s = np.zeros(rows)
            for k in feats:
                press = x[:, i, k]
                for name, share in spec['terms'].get((i, k), []):
                    press = press - np.float64(share) * occ[name]
                s = s + press
            sc[:, a] = s
        out.append(sc)
    return out


def rule(spec, obs):
    """-> actions [R, N] u8: the smallest phase with the largest score."""
    return np.stack([np.argmax(sc, axis=1) for sc in scores(spec, obs)], axis=1).astype(np.uint8)


def expand(table):
    """A host PressureTable in the named form of a spec, groups named by their index -> (phases, groups, terms)."""
    N = len(table.n_a)
    phases = [[[k for k in range(32) if (int(table.mask[i, a]) >> k) & 1] for a in range(int(table.n_a[i]))] for i in range(N)]
    groups = {g: [tuple(int(v) for v in p) for p in table.gpair[table.gptr[g]:table.gptr[g + 1]]] for g in range(len(table.gptr) - 1)}
    terms = {}
    for i in range(N):
        for k in range(24):
            cur = [(int(table.tgrp[i, k, r]), table.tw[i, k, r]) for r in range(3) if table.tgrp[i, k, r] >= 0]
            if cur:
                terms[(i, k)] = cur
    return phases, groups, terms


# ------------------------------------------------------------------ observations of the kernel tests
KINDS = ('quantised', 'uniform', 'zero')
ROWS = {'quantised': 4200, 'uniform': 80, 'zero': 80}      # 4200 > 4 x 1024: more replicas than one pass of the launch grid holds


def draw_obs(kind, n_node, n_feat, seed):
    rng = np.random.RandomState(4321 + seed)
    shape = (ROWS[kind], n_node, n_feat)
    if kind == 'quantised':                                 # multiples of 0.2 in [0, 1.4]: many ties for the maximum
        return (rng.randint(0, 8, size=shape) * 0.2).astype(np.float32)
    if kind == 'uniform':
        return (rng.rand(*shape) * 1.4).astype(np.float32)
    return np.zeros(shape, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """name: 'grid<rows>x<cols>' | 'net' -> (spec, {kind: obs [ROWS, N, F] f32}, {kind: actions [ROWS, N] u8}); computed once and
    shared (callers do not modify it).  Every entry of an own vector is drawn, also the ones no phase counts."""
    if name == 'net':
        spec, seed = net_spec(), 7
    else:
        rows, cols = (int(v) for v in name[4:].split('x'))
        spec, seed = grid_spec(rows, cols), rows * 100 + cols
    obs = {kind: draw_obs(kind, spec['N'], spec['F'], seed + n) for n, kind in enumerate(KINDS)}
    if name == 'net':                                       # the env's rows are zero past a node's own links
        for o in obs.values():
            for i, w in enumerate(R.TOPO.n_s_ls):
                o[:, i, w:] = 0.0
    return spec, obs, {kind: rule(spec, o) for kind, o in obs.items()}

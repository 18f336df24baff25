"""NumPy restatement of the synthetic ATSC grid for a rows x cols lattice on the constants of oracle/grid_ref.py.
TEST INFRASTRUCTURE: at 5x5 it is oracle.grid_ref.GridBatchRef operation for operation (tests/test_grid_shape_cpu.py compares
the two bit for bit); for every other shape it is what csrc/grid.hip's runtime-shape kernels are checked against.

  node i = row * cols + col, row 0 at the bottom; neighbours N = i + cols, E = i + 1, S = i - cols, W = i - 1;
  per-node model: oracle/grid_ref.py steps 1-6 unchanged; a link whose destination is outside the lattice leaves the grid;
  external entries: `entries(rows, cols)`, one xi factor per flow group.
"""
import numpy as np

from oracle import grid_ref as G


def entries(rows, cols):
    """(node, approach, group) of every external entry, in the order of oracle.grid_ref.ENTRIES at 5x5."""
    out = []
    for c in range(cols - 2, 0, -1):                 # group 0: from the north, top row, interior columns
        out.append(((rows - 1) * cols + c, 0, 0))
    for r in range(rows - 1, -1, -1):                # group 1: from the west, first column, even rows
        if r % 2 == 0:
            out.append((r * cols, 3, 1))
    for c in range(1, cols - 1):                     # group 2: from the south, bottom row, interior columns
        out.append((c, 2, 2))
    for r in range(rows):                            # group 3: from the east, last column, even rows
        if r % 2 == 0:
            out.append((r * cols + cols - 1, 1, 3))
    return out


def masks(rows, cols):
    n = rows * cols
    dist = np.zeros((n, n), dtype=int)
    for i in range(n):
        for j in range(n):
            dist[i, j] = abs(i // cols - j // cols) + abs(i % cols - j % cols)
    return (dist == 1).astype(int), dist


def neighbor_order(rows, cols):
    """north, east, south, west, the absent ones skipped."""
    out = []
    for i in range(rows * cols):
        r, c = divmod(i, cols)
        cur = []
        if r + 1 < rows:
            cur.append(i + cols)
        if c + 1 < cols:
            cur.append(i + 1)
        if r > 0:
            cur.append(i - cols)
        if c > 0:
            cur.append(i - 1)
        out.append(cur)
    return out


def demand_table(rows, cols, peak1, peak2):
    """[4,12] veh/h of every flow group in every 5-minute piece: entries of the group x the per-entry rate."""
    ent = entries(rows, cols)
    return np.array([[sum(1 for e in ent if e[2] == g) * G.demand_rate(g, 300 * p, peak1, peak2) for p in range(12)]
                     for g in range(4)], dtype=np.float64)


class ShapeBatchRef:
    def __init__(self, params, rows, cols, E=1, dtype=np.float64):
        self.p, self.E, self.f = params, E, dtype
        self.rows, self.cols, self.N = rows, cols, rows * cols
        self.green = G.green_table()
        self.nb, self.dist = masks(rows, cols)
        self.entries = entries(rows, cols)

    def reset(self, xi, mask=None):
        f, N = self.f, self.N
        xi = np.asarray(xi, dtype=f).reshape(self.E, 4)
        if mask is None:
            self.q = np.zeros((self.E, N, G.N_LANE), dtype=f)
            self.tr = np.zeros((self.E, N, G.N_LANE), dtype=f)
            self.prev = np.zeros((self.E, N), dtype=np.int64)
            self.t = np.zeros(self.E, dtype=np.int64)
            self.xi = xi.copy()
            self.hw = np.zeros((self.E, N, G.N_LANE), dtype=f)
        else:
            m = np.asarray(mask, dtype=bool)
            self.q[m] = 0; self.tr[m] = 0; self.prev[m] = 0; self.t[m] = 0; self.hw[m] = 0
            self.xi[m] = xi[m]
        return self.obs()

    def _eff_green(self, prev, cur):
        gp = self.green[prev] != 0
        gc = self.green[cur] != 0
        same = (prev == cur)[..., None]
        g = np.where(gc & gp, G.DT, np.where(gc & ~gp, G.DT - G.YELLOW, np.where(~gc & gp, G.YELLOW_EFF, 0.0)))
        g = np.where(same, np.where(gc, G.DT, 0.0), g)
        fac = np.where(self.green[cur] == 2, 0.5, 1.0)
        return (g * fac).astype(self.f)

    def _inside(self, rr, cc):
        return 0 <= rr < self.rows and 0 <= cc < self.cols

    def step(self, action):
        f, E, N, cols = self.f, self.E, self.N, self.cols
        a = np.asarray(action).reshape(E, N).astype(np.int64)
        geff = self._eff_green(self.prev, a)
        share = G.LINK_SHARE.astype(f)
        qk = self.q[:, :, G.LINK_LANE]
        D = np.minimum(qk * share, f(G.SAT) * geff * share)
        space = np.zeros((E, N, 4), dtype=f)
        free = np.maximum(f(G.Q_MAX) - self.q - self.tr, f(0))
        for lane in range(G.N_LANE):
            space[:, :, G.LANE_APPROACH[lane]] += free[:, :, lane]
        insum = np.zeros((E, N, 4), dtype=f)
        for n in range(N):
            r0, c0 = divmod(n, cols)
            for ap in range(4):
                dr, dc = G.APPROACH_FROM[ap]
                rr, cc = r0 + dr, c0 + dc
                if self._inside(rr, cc):
                    m = rr * cols + cc
                    k0, k1, k2 = G.APPROACH_FEED[ap]
                    insum[:, n, ap] = D[:, m, k0] + D[:, m, k1] + D[:, m, k2]
        scale = np.minimum(f(1), space / np.maximum(insum, f(1e-6)))
        flow = np.zeros_like(D)
        for n in range(N):
            r0, c0 = divmod(n, cols)
            for k in range(G.N_LINK):
                dr, dc, ap = G.LINK_DEST[k]
                rr, cc = r0 + dr, c0 + dc
                if self._inside(rr, cc):
                    flow[:, n, k] = D[:, n, k] * scale[:, rr * cols + cc, ap]
                else:
                    flow[:, n, k] = D[:, n, k]                                      # leaves the grid
        served = np.zeros_like(self.q)
        for k in range(G.N_LINK):
            served[:, :, G.LINK_LANE[k]] += flow[:, :, k]
        inflow = insum * scale
        sec = self.t * self.p.control
        for (node, ap, grp) in self.entries:
            rate = np.array([G.demand_rate(grp, s, self.p.peak1, self.p.peak2) for s in sec], dtype=f)
            inflow[:, node, ap] += rate / f(3600) * f(G.DT) * self.xi[:, grp]
        split = G.APPROACH_SPLIT.astype(f)
        moved = (served > f(G.WAIT_EPS)) | (self.q <= f(G.WAIT_EPS))
        self.hw = np.where(moved, f(0), self.hw + f(G.DT)).astype(f)
        self.q = (self.q - served + self.tr).astype(f)
        self.tr = (inflow[:, :, G.LANE_APPROACH] * split).astype(f)
        self.prev = a
        self.t = self.t + 1
        c = np.minimum(self.q, f(G.DET_CAP))[:, :, G.LINK_LANE]
        reward = -c.sum(axis=2)
        if self.p.objective != 'queue':
            wait = self.hw[:, :, G.LINK_LANE].sum(axis=2)
            reward = -wait if self.p.objective == 'wait' else reward - f(self.p.coef_wait) * wait
        g = reward.sum(axis=1)
        done = self.t >= self.p.T
        r_out = g if self.p.coop_gamma < 0 else reward
        return self.obs(), r_out.astype(f), done, g.astype(f)

    def obs(self):
        f = self.f
        c = np.minimum(self.q, f(G.DET_CAP))[:, :, G.LINK_LANE] / f(self.p.norm_wave)
        if self.p.clip_wave >= 0:
            c = np.clip(c, 0, f(self.p.clip_wave))
        return c.astype(f)

    def gather(self, x):
        """[E,N,F] -> [E,N,5F]: own, then the neighbours in ascending node index, left packed, zero padded."""
        return G.gather_grid(x, self.nb)


def actions(rng, ref, t, hold=0.6):
    """The action pattern of the trajectory tests: keep the phase with probability `hold`, else a random one."""
    keep = rng.rand(ref.E, ref.N) < hold
    return np.where(keep & (t > 0), ref.prev, rng.randint(0, 5, size=(ref.E, ref.N))).astype(np.uint8)

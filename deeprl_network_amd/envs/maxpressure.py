"""The rule-based `maxpressure` ATSC agent (Varaiya 2013): per intersection the phase whose served movements hold the largest
incoming-minus-downstream occupancy.  The tables of both synthetic scenarios, the host rule for one replica, and
csrc/maxpressure.hip behind the duck-type of the host controllers for a batch of replicas.  The rule is DESIGN.md 6."""
import collections

import numpy as np
import torch

from .. import _lib, ops
from .atsc import RuleController, described

N_MAX, A_MAX, F_MAX, T_MAX, G_MAX, P_MAX = 32, 8, 24, 3, 128, 768       # the limits of nmarl_atsc_maxpressure

# the signal links of a grid node: physical lane, turning share within the lane, destination as
# (neighbour offset (drow, dcol), receiving approach)
LINK_LANE = (0, 0, 0, 1, 1, 2, 3, 3, 3, 4, 4, 5)
LINK_SHARE = (.2, .6, .2, .15 / .85, .7 / .85, 1.0) * 2
LINK_DEST = ((0, -1, 1), (-1, 0, 0), (0, 1, 3), (1, 0, 2), (0, -1, 1), (-1, 0, 0),
             (0, 1, 3), (1, 0, 2), (0, -1, 1), (-1, 0, 0), (0, 1, 3), (1, 0, 2))
_LANE_FIRST_LINK = (0, 3, 5, 6, 9, 11)
_APPROACH_FIRST_LINKS = ((0,), (3, 5), (6,), (9, 11))                   # the distinct lanes of an approach at their first links

PressureTable = collections.namedtuple('PressureTable', 'n_a mask gptr gpair tgrp tw n_feat')
PressureTable.__doc__ = """The tables of nmarl_atsc_maxpressure (host NumPy): n_a [N] i32, mask [N,8] u32 (the greedy agent's), gptr [G+1] i32,
gpair [P,2] i16 (node, feature), tgrp [N,24,3] i16 (-1 = none, left packed), tw [N,24,3] f32, n_feat = the widest own vector."""


def _pack(n_a, mask, groups, terms, n_feat):
    """groups: list of pair lists [(node, feature)]; terms: {(node, feature): [(group, share)]} -> PressureTable."""
    N = len(n_a)
    gptr = np.zeros(len(groups) + 1, dtype=np.int32)
    gptr[1:] = np.cumsum([len(g) for g in groups])
    gpair = np.array([p for g in groups for p in g], dtype=np.int16).reshape(-1, 2)
    tgrp = -np.ones((N, F_MAX, T_MAX), dtype=np.int16)
    tw = np.zeros((N, F_MAX, T_MAX), dtype=np.float32)
    for (i, k), cur in terms.items():
        for r, (g, share) in enumerate(cur):
            tgrp[i, k, r], tw[i, k, r] = g, np.float32(share)
    return check_pressure_table(PressureTable(n_a, mask, gptr, gpair, tgrp, tw, int(n_feat)))


def check_pressure_table(t):
    """The kernel reads the tables without checks: every bound it relies on is verified here.  -> t"""
    N = len(t.n_a)
    G, P = len(t.gptr) - 1, len(t.gpair)
    ok = (1 <= N <= N_MAX and 1 <= t.n_feat <= F_MAX and 0 <= G <= G_MAX and 0 <= P <= P_MAX and
          t.mask.shape == (N, A_MAX) and t.tgrp.shape == (N, F_MAX, T_MAX) and t.tw.shape == (N, F_MAX, T_MAX) and
          t.gpair.shape == (P, 2) and int(t.n_a.min()) >= 1 and int(t.n_a.max()) <= A_MAX and
          int(t.gptr[0]) == 0 and int(t.gptr[-1]) == P and bool((np.diff(t.gptr) >= 1).all()) and
          int(t.tgrp.min()) >= -1 and int(t.tgrp.max()) < G and bool(np.isfinite(t.tw).all()) and
          not int((t.mask >> np.uint32(t.n_feat)).max()))
    if ok and P:
        ok = 0 <= int(t.gpair[:, 0].min()) and int(t.gpair[:, 0].max()) < N and 0 <= int(t.gpair[:, 1].min()) and \
            int(t.gpair[:, 1].max()) < t.n_feat
    if ok:                                                 # left packed: no term behind an empty slot
        present = t.tgrp >= 0
        ok = bool((present[:, :, :-1] | ~present[:, :, 1:]).all())
    if not ok:
        raise _lib.NmarlError('max-pressure table outside the limits of nmarl_atsc_maxpressure (N <= %d, F <= %d, G <= %d, P <= %d)'
                              % (N_MAX, F_MAX, G_MAX, P_MAX))
    return t


def grid_pressure_table(rows=5, cols=5):
    """PressureTable of a rows x cols grid.  Lane l of a node is read at its first link, as the greedy agent reads it; its terms
    are the lane's links, ascending, whose destination node j lies inside the lattice: (group of (j, receiving approach),
    float32 turning share).  A link that leaves the lattice contributes nothing.  The group of (j, approach) lists the distinct
    lanes of that approach at their first links; only referenced groups exist, numbered in ascending 4 j + approach."""
    from .large_grid_env import N_FEAT, grid_greedy_table
    n_a, mask = grid_greedy_table(rows, cols)
    raw = {}
    for i in range(rows * cols):
        r, c = divmod(i, cols)
        for k, lane in enumerate(LINK_LANE):
            dr, dc, ap = LINK_DEST[k]
            rr, cc = r + dr, c + dc
            if 0 <= rr < rows and 0 <= cc < cols:
                raw.setdefault((i, _LANE_FIRST_LINK[lane]), []).append((4 * (rr * cols + cc) + ap, LINK_SHARE[k]))
    keys = sorted({key for cur in raw.values() for key, _ in cur})
    index = {key: g for g, key in enumerate(keys)}
    groups = [[(key // 4, k0) for k0 in _APPROACH_FIRST_LINKS[key % 4]] for key in keys]
    terms = {at: [(index[key], share) for key, share in cur] for at, cur in raw.items()}
    return _pack(n_a, mask, groups, terms, N_FEAT)


def net_pressure_table(topo):
    """PressureTable of the network `topo` (NetTopology).  Every node j that feeds a link gets one group: the links (i, k) with
    src[i, k] = j in the order of `dn_pair`; every link of such a node carries the one term (that group, 1.0).  A node that feeds
    nothing has no terms."""
    from .real_net_env import net_greedy_table
    n_a, mask = net_greedy_table(topo.node_names, topo.phases)
    h = topo.host
    groups, terms = [], {}
    for j in range(topo.N):
        if int(h['fan'][j]) > 0:
            pairs = h['dn_pair'][int(h['dn_ptr'][j]):int(h['dn_ptr'][j + 1])]
            for k in range(topo.n_s_ls[j]):
                terms[(j, k)] = [(len(groups), 1.0)]
            groups.append([(int(v) >> 8, int(v) & 255) for v in pairs])
    return _pack(n_a, mask, groups, terms, topo.L)


class MaxPressureController(RuleController):
    """The rule on the host for ONE replica, in float64 on the list of the nodes' own wave vectors (Python floats: every sum and
    product in the order DESIGN.md 6 writes it).  Same `forward(obs) -> actions` duck-type as the greedy controllers."""
    name = 'maxpressure'

    def __init__(self, table, node_names=None):
        self.table = t = check_pressure_table(table)
        self.node_names = node_names
        self._groups = [[(int(i), int(k)) for i, k in t.gpair[t.gptr[g]:t.gptr[g + 1]]] for g in range(len(t.gptr) - 1)]
        self._phases = []                                 # per node, per phase: its counted features, ascending
        self._terms = {}                                  # (node, feature) -> [(group, float64 of the float32 share)]
        for i in range(len(t.n_a)):
            self._phases.append([[k for k in range(t.n_feat) if (int(t.mask[i, a]) >> k) & 1] for a in range(int(t.n_a[i]))])
            for k in range(t.n_feat):
                cur = []
                for r in range(T_MAX):
                    if t.tgrp[i, k, r] < 0:
                        break
                    cur.append((int(t.tgrp[i, k, r]), float(t.tw[i, k, r])))
                self._terms[(i, k)] = cur

    @classmethod
    def for_env(cls, env):
        """For a batch env or a one-replica env (which wraps one): the scenario's table is the batch env's `pressure_table`."""
        return cls(described(getattr(env, 'batch', env), 'pressure_table', 'maxpressure agent'), getattr(env, 'node_names', None))

    def scores(self, obs):
        """-> per node the list of its phases' scores."""
        x = [[float(v) for v in np.asarray(ob).reshape(-1)] for ob in obs]
        occ = []
        for pairs in self._groups:
            s = 0.0
            for i, k in pairs:
                s = s + x[i][k]
            occ.append(s / float(len(pairs)))
        out = []
        for i, phases in enumerate(self._phases):
            cur = []
            for feats in phases:
                s = 0.0
                for k in feats:
                    press = x[i][k]
                    for g, w in self._terms[(i, k)]:
                        press = press - w * occ[g]
                    s = s + press
                cur.append(s)
            out.append(cur)
        return out

    def forward(self, obs):
        return [int(np.argmax(np.array(s))) for s in self.scores(obs)]          # the first maximum


class MaxPressureBatchController(RuleController):
    """`MaxPressureController` for E lock-stepped replicas.  `forward_batch(obs, out)` decides every (replica, node) with one
    launch of nmarl_atsc_maxpressure on the env's observation buffer as it is -- no staging copy, nothing read back --; `forward`
    is the host controller's, so the object also drives the one-replica loops."""
    name = 'maxpressure'

    def __init__(self, batch_env):
        self.host = MaxPressureController.for_env(batch_env)
        t = self.table = self.host.table
        self.node_names = self.host.node_names
        self.n_own, self.a_max = t.n_feat, int(t.n_a.max())
        dev = torch.device(batch_env.device)
        self.n_a = torch.from_numpy(t.n_a).to(dev)
        self.mask = torch.from_numpy(t.mask.view('int32')).to(dev)
        self.gptr, self.gpair = torch.from_numpy(t.gptr).to(dev), torch.from_numpy(t.gpair).to(dev)
        self.tgrp, self.tw = torch.from_numpy(t.tgrp).to(dev), torch.from_numpy(t.tw).to(dev)

    def forward_batch(self, obs_tensor, out_actions):
        """obs_tensor [E,N,row] f32 (rows lead with the node's own wave vector) -> out_actions [E,N] u8."""
        return ops.atsc_maxpressure(self.n_a, self.mask, self.gptr, self.gpair, self.tgrp, self.tw, obs_tensor, out_actions,
                                    n_feat=self.n_own, a_max=self.a_max)

    def forward(self, obs):
        return self.host.forward(obs)

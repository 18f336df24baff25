"""Synthetic (SUMO-free) ATSC grid on MI355X -- host mirror of the reference's
envs/large_grid_env.py + envs/atsc_env.py for the `atsc_large_grid` scenario.

The reference drives an external SUMO process over TraCI; this path keeps the reference's
*contract* (25 agents, 5 phases, 12-wide `wave` observation, queue reward, 5 s control / 2 s
yellow, 720-step episodes, the peak_flow demand schedule, neighbour / distance masks) and
replaces the microsimulation by the store-and-forward model specified in
oracle/grid_ref.py, stepped by csrc/grid.hip for E lock-stepped replicas.

ENV_CONFIG's optional keys `grid_rows` / `grid_cols` (absent: 5) give the lattice any shape of 2..32 intersections -- the same
per-node model, the external entries placed by the rule of `grid_entries`; 5x5 is the reference's grid.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from .atsc import N_GROUP, OBJECTIVES, RULE_AGENTS, AtscBatchEnv, AtscEnv, RuleController, atsc_params_from_config  # noqa: F401
from .traffic_record import grid_demand, grid_mult

N_NODE, N_FEAT, N_OBS, N_PHASE = 25, 12, 60, 5
N_NODE_MAX = 32                   # one replica per 32-lane half wave, lane = intersection (csrc/grid_tile.h)


def grid_shape_from_config(config):
    """(rows, cols) from ENV_CONFIG's optional `grid_rows` / `grid_cols` (absent: 5)."""
    rows, cols = config.getint('grid_rows', fallback=5), config.getint('grid_cols', fallback=5)
    if rows < 1 or cols < 1 or not 2 <= rows * cols <= N_NODE_MAX:
        raise _lib.NmarlError('grid_rows x grid_cols must be at least 1 x 1 with 2 <= grid_rows * grid_cols <= %d intersections, '
                              'got %d x %d' % (N_NODE_MAX, rows, cols))
    return rows, cols


def grid_masks(rows=5, cols=5):
    """neighbor_mask / distance_mask of large_grid_env.py:58-105 (node i = row * cols + col = nt{i+1}): Manhattan distance 1 /
    Manhattan distance."""
    idx = np.arange(rows * cols)
    r, c = idx // cols, idx % cols
    dist = (np.abs(r[:, None] - r[None, :]) + np.abs(c[:, None] - c[None, :])).astype(int)
    return (dist == 1).astype(int), dist


def grid_neighbor_order(rows=5, cols=5):
    """For every node its neighbours in the order the reference's `neighbor_map` lists them (large_grid_env.py:58-85: north,
    east, south, west, the absent ones skipped; node i = row * cols + col = nt{i+1}, north = i + cols).  This -- not the ascending
    index -- is the order in which an IA2C / IA2C-FP agent's observation concatenates the neighbours' wave vectors and
    fingerprints (atsc_env.py:263-271); neighbour ACTIONS and the MA2C nets' gathers use the mask order (ascending)."""
    out = []
    for i in range(rows * cols):
        r, c = divmod(i, cols)
        cand = [(r + 1, c), (r, c + 1), (r - 1, c), (r, c - 1)]
        out.append([rr * cols + cc for rr, cc in cand if 0 <= rr < rows and 0 <= cc < cols])
    return out


def grid_n_s_ls(agent, neighbor_mask):
    """Observation width per node: an `ia2c*` agent sees its own and its neighbours' wave vectors, every other its own."""
    return [N_FEAT * (1 + int(row.sum())) if agent.startswith('ia2c') else N_FEAT for row in np.asarray(neighbor_mask)]


def grid_entries(rows=5, cols=5):
    """The external entries (node, approach, flow group) of a rows x cols lattice, by the rule that yields the reference's twelve
    at 5x5 (large_grid_data/build_file.py:285-295), in its order: group 0 from the north into approach 0 of the top-row nodes at
    the interior columns 1..cols-2, group 1 from the west into approach 3 of the first-column nodes at even rows, group 2 from
    the south into approach 2 of the bottom-row nodes at the interior columns, group 3 from the east into approach 1 of the
    last-column nodes at even rows.  (What csrc/grid_tile.h evaluates per (node, approach).)"""
    top, even = (rows - 1) * cols, range(0, rows, 2)
    return ([(top + c, 0, 0) for c in range(cols - 2, 0, -1)] + [(r * cols, 3, 1) for r in reversed(even)] +
            [(c, 2, 2) for c in range(1, cols - 1)] + [(r * cols + cols - 1, 1, 3) for r in even])


# link -> physical lane (oracle/grid_ref.py LINK_LANE): the 12-wide wave vector counts duplicated lanes
_LANE_FIRST_LINK = (0, 3, 5, 6, 9, 11)


class LargeGridController(RuleController):
    """The reference's rule-based `greedy` agent (large_grid_env.py:30-45): per node the phase whose served lanes hold the
    most vehicles.  The reference indexes a 6-lane observation [N, E lane 0, E lane 1, S, W lane 0, W lane 1]; this env's
    wave vector has one entry per signal LINK (12, duplicated lanes), so the six lanes are read at their first links.
    Same `forward(obs) -> actions` duck-type."""
    name = 'greedy'

    def __init__(self, node_names=None):
        self.node_names = node_names

    @staticmethod
    def lane_counts(ob):
        ob = np.asarray(ob, dtype=np.float64).reshape(-1)
        return ob if len(ob) == 6 else ob[list(_LANE_FIRST_LINK)]

    def greedy(self, ob, node_name=None):
        q = self.lane_counts(ob)
        # phases of large_grid_env.py:25-26: N+S through, E+W left, E+W through, E approach, W approach
        return int(np.argmax([q[0] + q[3], q[2] + q[5], q[1] + q[4], q[1] + q[2], q[4] + q[5]]))

    def forward(self, obs):
        return [self.greedy(ob) for ob in obs]


# the five phases of LargeGridController.greedy as sets of lanes [N, E lane 0, E lane 1, S, W lane 0, W lane 1] (large_grid_env.py:25-26)
_GREEDY_PHASE_LANES = ((0, 3), (2, 5), (1, 4), (1, 2), (4, 5))


def grid_greedy_table(rows=5, cols=5):
    """(n_a [N] i32, mask [N,8] u32) of nmarl_atsc_greedy for a rows x cols grid: bit k of mask[i][a] = feature k of the node's
    wave vector counts for phase a.  The lanes are read at their first links, so the five bit sets are {0,6}, {5,11}, {3,9},
    {3,5}, {9,11} -- what LargeGridController.greedy adds -- and every node of any shape has the same."""
    N = rows * cols
    mask = np.zeros((N, 8), dtype=np.uint32)
    for a, lanes in enumerate(_GREEDY_PHASE_LANES):
        mask[:, a] = sum(1 << _LANE_FIRST_LINK[lane] for lane in lanes)
    return np.full(N, N_PHASE, dtype=np.int32), mask


def grid_params_from_config(config):
    """ENV_CONFIG section -> nmarl_grid_params_t; keys of atsc_env.py:79-99 + large_grid_env.py:50-52."""
    p = atsc_params_from_config(config, _lib.GridParams(), 'grid', config.get('objective', fallback='queue'), _lib.NmarlError)
    p.peak1 = config.getfloat('peak_flow1')
    p.peak2 = config.getfloat('peak_flow2')
    return p


class LargeGridBatchEnv(AtscBatchEnv):
    rows, cols = 5, 5                 # the reference's lattice unless ENV_CONFIG's grid_rows / grid_cols say otherwise

    @property
    def entries(self):
        return grid_entries(self.rows, self.cols)

    def _scenario(self, config):
        if self.name == 'large_grid':        # (config_greedy.ini's spelling): ONE name for the scenario -- Trainer / perform branch on 'atsc*'
            self.name = 'atsc_large_grid'
        self.params = grid_params_from_config(config)
        self.rows, self.cols = grid_shape_from_config(config)
        self.fixed_shape = (self.rows, self.cols) == (5, 5)       # the 5x5 kernels; any other shape: the `_rc` entries
        N = self.rows * self.cols
        self.n_agent = N
        self.n_a = N_PHASE
        self.n_a_ls = [N_PHASE] * N
        self.neighbor_mask, self.distance_mask = grid_masks(self.rows, self.cols)
        self.neighbor_order = grid_neighbor_order(self.rows, self.cols)
        self.n_s_ls = grid_n_s_ls(self.agent, self.neighbor_mask)
        return 6, N_OBS

    def traffic_model(self):
        """(mult [N,6] i32, demand [4,12] f64) of the traffic record (envs/traffic_record.py)."""
        n_entry = [sum(1 for e in self.entries if e[2] == g) for g in range(N_GROUP)]
        return grid_mult(self.n_agent), grid_demand(float(self.params.peak1), float(self.params.peak2), n_entry)

    def greedy_rule(self):
        """(host controller, own observation width, n_a, mask) of the batched greedy agent (envs/greedy.py)."""
        return (LargeGridController(), N_FEAT) + grid_greedy_table(self.rows, self.cols)

    def pressure_table(self):
        from .maxpressure import grid_pressure_table
        return grid_pressure_table(self.rows, self.cols)

    compact_obs = False

    def set_compact_obs(self, flag=True):
        """Compact observation [E,N,12]: every node's OWN wave vector -- what the reference hands an MA2C agent
        (atsc_env.py:253-262) -- instead of the gathered [E,N,60] slab; the consumer gathers the neighbours
        (agents/policies.py `_enc_parts`).  Batched engine only: the E = 1 reference duck-type keeps the slab."""
        self.compact_obs = bool(flag)
        self.params.compact_obs = 1 if flag else 0
        self.obs = torch.zeros(self.E, self.n_agent, N_FEAT if flag else N_OBS, dtype=torch.float32, device=self.device)
        return True

    def _reset_call(self, params, args):
        if self.fixed_shape:
            rc = _lib.lib.nmarl_grid_reset(ctypes.byref(params), *args)
        else:
            rc = _lib.lib.nmarl_grid_reset_rc(ctypes.byref(params), *args, self.rows, self.cols)
        _lib.check(rc, 'nmarl_grid_reset')

    def _step_call(self, args):
        if self.fixed_shape:
            rc = _lib.lib.nmarl_grid_step(ctypes.byref(self.params), *args)
        else:
            rc = _lib.lib.nmarl_grid_step_rc(ctypes.byref(self.params), *args, self.rows, self.cols)
        _lib.check(rc, 'nmarl_grid_step')

    _words = None

    def inkernel_step_supported(self):
        """CommNet's one-launch lock-step can run this env's step as a role of the same launch (csrc/lstm_mfma.hip GENV): compact
        observation, queue objective, the 5x5 lattice (the hand-off words pack 13 + 12 actions), and compute units left idle by
        the LSTM blocks."""
        from .. import ops
        return (self.fixed_shape and self.compact_obs and not self.params.objective and
                ops.step_grid_env_blocks(self.n_agent, self.E) > 0)

    def inkernel_step(self, auto_reset=False, obs_out=None, reward_out=None, done_out=None, greward_out=None):
        """Arguments of `step` for the policy's lock-step launch to run the env step itself, on the actions it draws
        (ops._step_x msg['genv'], nmarl_lstm_step_x with genv): same state tensors, same outputs."""
        if not self.fixed_shape or not self.compact_obs or self.params.objective:
            raise _lib.NmarlError('the in-launch grid env step writes the compact observation and knows the queue objective on '
                                  'the 5x5 lattice')
        if self._words is None:          # hand-off words of the launch ([E][2] u64): zeroed once, every launch leaves them zero
            self._words = torch.zeros(_lib.lib.nmarl_lstm_step_grid_words(self.E), dtype=torch.int64, device=self.device)
        obs, reward, done, greward = self._outputs(obs_out, reward_out, done_out, greward_out)
        return dict(params=self.params, q=self.q, transit=self.transit, prev_action=self.prev_action, t=self.t, xi=self.xi,
                    obs_out=obs, reward=reward, done=done, global_reward=greward, auto_reset=bool(auto_reset),
                    seed=self.seed, env_id_base=self.env_id_base, episode=self.episode, words=self._words)

    def clear_inkernel_words(self):
        """After a hand-off time-out (the launch gave up waiting and may have left arrivals in the words)."""
        if self._words is not None:
            self._words.zero_()


class LargeGridEnv(AtscEnv):
    """Reference duck-type (atsc_env.py:77-524 / large_grid_env.py:48-137) for ONE replica.
    Observation lists: `ma2c*` / `greedy` / `maxpressure` 12 wave features; `ia2c*` own + neighbours' in the reference's `neighbor_map` list
    order (north, east, south, west: atsc_env.py:263-269, `neighbor_order`) (+ the neighbours' fingerprints in the same order
    for ia2c_fp); neighbour actions in mask order (ascending, atsc_env.py:132-136)."""
    batch_class = LargeGridBatchEnv

    def __init__(self, config, port=0, device='cuda', **_):
        super().__init__(config, port, device)
        self.rows, self.cols, self.neighbor_order = self.batch.rows, self.batch.cols, self.batch.neighbor_order
        self.node_names = ['nt%d' % (i + 1) for i in range(self.n_agent)]
        self._nbr = [np.where(self.neighbor_mask[i] == 1)[0] for i in range(self.n_agent)]

    def _state_list(self):
        own = self.batch.obs[0, :, :N_FEAT].cpu().numpy().astype(np.float64)      # every node's own wave vector leads its row
        out = []
        for i in range(self.n_agent):
            cur = [own[i]]
            if self.agent.startswith('ia2c'):
                cur += [own[j] for j in self.neighbor_order[i]]
            if self.agent == 'ia2c_fp':
                cur += [np.asarray(self.fp[j]) for j in self.neighbor_order[i]]
            out.append(np.concatenate(cur))
        return out

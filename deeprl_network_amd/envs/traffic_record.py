"""Traffic and trip tables of an ATSC evaluation -- the reference's `_traffic.csv` / `_trip.csv` (envs/atsc_env.py:107-124,
155-163, 464-499) measured on the synthetic grid / network envs by csrc/traffic.hip (specification: its header).

The reference reads individual SUMO vehicles over TraCI once per simulated second; the synthetic envs are fluid models with one
state per 5-s control step, so there is one row per control step, measured by one launch behind the env step for all E replicas
and kept on the device until `rows()` copies the whole record to the host once.  A batched user records every replica with

    rec = TrafficRecorder(batch_env, max_steps); rec.begin()
    batch_env.step(actions); rec.step(k)              # k = 0, 1, ...: the row's slot; no host synchronisation
    table, trips = rec.rows(), rec.trip()
"""
import numpy as np
import torch

from .. import _lib
from .atsc import described
from .net_file import MONACO_ACTIVITY

TRAFFIC_COLUMNS = ('number_total_car', 'number_departed_car', 'number_arrived_car', 'avg_wait_sec', 'avg_speed_mps', 'std_queue',
                   'avg_queue', 'time_sec')                       # the 8 floats of a row, in the kernel's order
TRIP_COLUMNS = ('episode', 'id', 'depart_sec', 'arrival_sec', 'duration_sec', 'wait_step', 'wait_sec')      # atsc_env.py:113-120
N_GROUP, N_PIECE = 4, 12
DT, WAIT_EPS = 5.0, 1e-3

GRID_MULT = (3, 2, 1, 3, 2, 1)                                    # signal links per lane (oracle/grid_ref.py LINK_LANE)
_GRID_RATIOS1 = (0.4, 0.7, 0.9, 1.0, 0.75, 0.5, 0.25)             # large_grid_data/build_file.py:298
_GRID_RATIOS2 = (0.3, 0.8, 0.9, 1.0, 0.8, 0.6, 0.2)               # large_grid_data/build_file.py:299


def grid_mult(n_node=25):
    """[N,6] i32: every lane of every node counts once per signal link it carries, the way the reward counts it."""
    return np.tile(np.array(GRID_MULT, dtype=np.int32), (n_node, 1))


def net_mult(n_s_ls, L):
    """[N,L] i32: 1 for the node's own links, 0 for the padding up to the widest node."""
    return (np.arange(L)[None, :] < np.asarray(n_s_ls)[:, None]).astype(np.int32)


def grid_demand(peak1, peak2, n_entry=(3, 3, 3, 3)):
    """[4,12] f64 veh/h: the flow group's entries (3 each on the 5x5 grid; `n_entry` per group for another shape) x the
    per-entry rate of large_grid_data/build_file.py:296-321 (what csrc/grid_tile.h demand_rate evaluates): first wave in pieces
    0..6, second wave, from 900 s, in pieces 3..9."""
    d = np.zeros((N_GROUP, N_PIECE))
    for g in range(N_GROUP):
        for p in range(N_PIECE):
            if g < 2 and p < 7:
                d[g, p] = float(n_entry[g]) * (peak1 * (0.6 if g == 0 else 1.0) * _GRID_RATIOS1[p])
            elif g >= 2 and 3 <= p < 10:
                d[g, p] = float(n_entry[g]) * (peak2 * (0.6 if g == 2 else 1.0) * _GRID_RATIOS2[p - 3])
    return d


def net_demand(flow_rate):
    """[4,12] f64 veh/h: flow_rate x the number of active flows of the group (real_net_data/build_file.py:70-96)."""
    return float(flow_rate) * np.array(MONACO_ACTIVITY, dtype=np.float64)


class TrafficRecorder:
    """Recorder state + the record rec[max_steps][E][8] of an ATSC batch env (envs/atsc.py AtscBatchEnv, which says what its lanes
    or links count for and what its demand is: `traffic_model`), all on the env's device."""

    def __init__(self, batch_env, max_steps):
        mult, demand = described(batch_env, 'traffic_model', 'traffic record')
        dev = torch.device(batch_env.device)
        if dev.type != 'cuda':
            raise _lib.NmarlError('TrafficRecorder needs a HIP device; there is no CPU path')
        if int(max_steps) < 1:
            raise _lib.NmarlError('max_steps must be at least 1')
        self.env, self.E, self.max_steps = batch_env, batch_env.E, int(max_steps)
        self.N, self.S = mult.shape
        self.mult_host, self.demand_host = mult, demand
        self.mult = torch.from_numpy(mult).to(dev)
        self.demand = torch.from_numpy(demand).to(dev)
        self.stand = torch.zeros(self.E, self.N, self.S, dtype=torch.float32, device=dev)
        self.prev_total = torch.zeros(self.E, dtype=torch.float64, device=dev)
        self.cum = torch.zeros(self.E, 4, dtype=torch.float64, device=dev)
        self.rec = torch.zeros(self.max_steps, self.E, 8, dtype=torch.float32, device=dev)
        self.n_calls = 0                                                     # `step` calls so far (host)
        self.first_call = torch.zeros(self.E, dtype=torch.int64, device=dev)  # n_calls at the replica's last `begin`

    def begin(self, mask=None):
        """Clears stand / prev_total / cum of the replicas selected by mask ([E] u8 on the device; None = all)."""
        P = _lib.ptr
        rc = _lib.lib.nmarl_atsc_traffic_begin(self.E, self.N, self.S, P(mask, torch.uint8), P(self.stand), P(self.prev_total),
                                               P(self.cum), _lib.stream())
        _lib.check(rc, 'nmarl_atsc_traffic_begin')
        if mask is None:
            self.first_call.fill_(self.n_calls)
        else:
            self.first_call.masked_fill_(mask.bool(), self.n_calls)

    def step(self, slot):
        """Measures the state the env's last `step` (without auto-reset) left, for every replica, into rec[slot]."""
        if not 0 <= slot < self.max_steps:
            raise _lib.NmarlError('record slot %d outside 0..%d' % (slot, self.max_steps - 1))
        P, b = _lib.ptr, self.env
        rc = _lib.lib.nmarl_atsc_traffic_step(self.E, self.N, self.S, P(self.mult), P(self.demand), P(b.q, torch.float32),
                                              P(b.transit, torch.float32), P(b.t, torch.int32), P(b.xi, torch.float32),
                                              P(self.stand), P(self.prev_total), P(self.cum), P(self.rec[slot]), _lib.stream())
        _lib.check(rc, 'nmarl_atsc_traffic_step')
        self.n_calls += 1

    def rows(self):
        """The whole record on the host, [max_steps, E, 8] f32 (columns: TRAFFIC_COLUMNS): one copy."""
        return self.rec.cpu().numpy()

    def trip(self):
        """Per replica, the one `trip` a fluid has since its last `begin`: the mean time in the network per completed vehicle
        (Little's law) and the mean time spent in a queue.  -> dict of [E] arrays keyed by the reference's column names."""
        cum = self.cum.cpu().numpy()
        steps = self.n_calls - self.first_call.cpu().numpy()
        done = np.maximum(cum[:, 1], WAIT_EPS)
        return {'depart_sec': np.zeros(self.E, dtype=np.int64), 'arrival_sec': 5 * steps, 'duration_sec': cum[:, 2] / done,
                'wait_step': cum[:, 3] / DT / done, 'wait_sec': cum[:, 3] / done}


def traffic_rows(rec, episode):
    """One replica's record rec [steps, 8] f32 -> its rows of `_traffic.csv` (atsc_env.py:490-499), in step order."""
    out = []
    for row in np.asarray(rec).astype(np.float64):
        cur = dict(zip(TRAFFIC_COLUMNS, row.tolist()))
        out.append({'episode': episode, 'time_sec': int(cur.pop('time_sec')), **cur})
    return out


def trip_row(trip, e, episode):
    """Replica e of `TrafficRecorder.trip()` -> its row of `_trip.csv` (atsc_env.py:113-120)."""
    return {'episode': episode, 'id': 'fluid', **{k: trip[k][e].item() for k in TRIP_COLUMNS[2:]}}


class EpisodeRecord:
    """The one-replica env's (envs/atsc.py AtscEnv) recorder next to `control_data`, and the two tables."""

    def __init__(self, env):
        self.env = env
        self.recorder = TrafficRecorder(env.batch, env.T)
        self.slot = 0

    def begin(self):
        self.recorder.begin()
        self.slot = 0

    def step(self):
        self.recorder.step(self.slot)
        self.slot += 1

    def collect(self, traffic_data, trip_data):
        """The episode's rows (atsc_env.py:490-499) and its trip row (113-120), appended to the env's lists."""
        if self.slot == 0:
            return
        episode = self.env.cur_episode
        traffic_data.extend(traffic_rows(self.recorder.rows()[:self.slot, 0], episode))
        trip_data.append(trip_row(self.recorder.trip(), 0, episode))
        self.slot = 0


def write_tables(env):
    """atsc_env.py:155-163: the three CSVs of an evaluation."""
    import pandas as pd
    stem = env.output_path + '%s_%s_' % (env.name, env.agent)
    pd.DataFrame(env.control_data).to_csv(stem + 'control.csv')
    pd.DataFrame(env.traffic_data).to_csv(stem + 'traffic.csv')
    pd.DataFrame(env.trip_data).to_csv(stem + 'trip.csv')

"""The traffic record of an ATSC evaluation (csrc/traffic.hip): NumPy float64 restatement of its eight steps.
TEST INFRASTRUCTURE.  PARITY UNPINNED: the reference measures these quantities on individual SUMO vehicles over TraCI
(envs/atsc_env.py:464-499); the synthetic envs are fluid store-and-forward models without vehicles, so this file IS the
specification of the measurement.  File names, column names, row cadence and column meanings are the reference's.

Static inputs: mult [N,S] int (detector entries of `ilds_in` per state slot; a slot is valid where mult > 0; M = sum mult) and
demand [4,12] float64 (veh/h of flow group g in 5-minute piece p; pieces >= 12 count 0)."""
import numpy as np

DT = 5.0
V_FREE = 13.89          # m/s: 50 km/h, one speed for every link
WAIT_EPS = 1e-3         # veh, the constant of the `wait` objective
COLUMNS = ('number_total_car', 'number_departed_car', 'number_arrived_car', 'avg_wait_sec', 'avg_speed_mps', 'std_queue',
           'avg_queue', 'time_sec')


class TrafficRecordRef:
    def __init__(self, mult, demand, E):
        self.mult = np.asarray(mult, dtype=np.int64)
        self.demand = np.asarray(demand, dtype=np.float64)
        assert self.demand.shape == (4, 12) and self.mult.ndim == 2
        self.valid = self.mult > 0
        self.M = float(self.mult[self.valid].sum())
        self.E = E
        self.stand = np.zeros((E,) + self.mult.shape, dtype=np.float32)
        self.prev_total = np.zeros(E)
        self.cum = np.zeros((E, 4))
        self.arrived_raw = np.zeros(E)

    def begin(self, mask=None):
        m = np.ones(self.E, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        self.stand[m] = 0
        self.prev_total[m] = 0
        self.cum[m] = 0

    def step(self, q, transit, t, xi):
        """q, transit [E,N,S], t [E] (>= 1), xi [E,4]: the state an env step without auto-reset left.  -> rows [E,8] float64
        (COLUMNS); `arrived_raw` keeps step 3's value before the clamp."""
        q = np.asarray(q).astype(np.float64)
        tr = np.asarray(transit).astype(np.float64)
        t = np.asarray(t).astype(np.int64)
        xi = np.asarray(xi).astype(np.float64)
        assert (t >= 1).all()
        v, w = self.valid[None], self.mult[None].astype(np.float64)
        piece = ((t - 1) * 5) // 300                                                           # 1
        rate = np.where((piece < 12)[:, None], self.demand[:, np.minimum(piece, 11)].T, 0.0)   # [E,4]
        departed = (rate / 3600.0 * DT * xi).sum(axis=1)
        halting = np.where(v, q, 0.0).sum(axis=(1, 2))                                         # 2
        moving = np.where(v, tr, 0.0).sum(axis=(1, 2))
        total = halting + moving
        self.arrived_raw = self.prev_total + departed - total                                  # 3
        arrived = np.maximum(self.arrived_raw, 0.0)
        self.stand = np.where(v & ~(q <= WAIT_EPS), self.stand + np.float32(DT), np.float32(0)).astype(np.float32)   # 4
        some = total > WAIT_EPS
        safe = np.where(some, total, 1.0)
        avg_wait = np.where(some, np.where(v, q * self.stand.astype(np.float64), 0.0).sum(axis=(1, 2)) / 2.0 / safe, 0.0)   # 5
        avg_speed = np.where(some, V_FREE * moving / safe, 0.0)                                # 6
        avg_queue = (w * np.where(v, q, 0.0)).sum(axis=(1, 2)) / self.M                         # 7
        dev = np.where(v, q - avg_queue[:, None, None], 0.0)
        std_queue = np.sqrt((w * dev * dev).sum(axis=(1, 2)) / self.M)
        self.prev_total = total                                                                # 8
        self.cum = self.cum + np.stack([departed, arrived, total * DT, halting * DT], axis=1)
        return np.stack([total, departed, arrived, avg_wait, avg_speed, std_queue, avg_queue, 5.0 * t], axis=1)

    def trip(self, steps):
        """The episode's one trip row per replica (without `episode`, `id`): dict of [E] arrays."""
        done = np.maximum(self.cum[:, 1], WAIT_EPS)
        return {'depart_sec': np.zeros(self.E), 'arrival_sec': 5.0 * np.broadcast_to(steps, (self.E,)),
                'duration_sec': self.cum[:, 2] / done, 'wait_step': self.cum[:, 3] / DT / done, 'wait_sec': self.cum[:, 3] / done}

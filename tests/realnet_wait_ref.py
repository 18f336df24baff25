"""The `wait` / `hybrid` objectives of the synthetic network (atsc_env.py:87-96, 383-418) as a NumPy reference: the
specification in the header of csrc/realnet.hip / DESIGN.md 6, on top of oracle/realnet_ref.py.  TEST HELPER, not a test.

It is the grid's step 6 (oracle/grid_ref.py:42-48) carried to links.  One more state array hw [E,N,L] holds the seconds the
front vehicle of a link has been standing.  With q the queue at the START of the step and served = D * scale the quantity of
oracle/realnet_ref.py step 3:
    moved    = served > WAIT_EPS  or  q <= WAIT_EPS
    hw'      = 0 if moved else hw + 5                      (links k >= n_s_i stay 0)
    wait_i   = sum over the node's links of hw'
    reward_i = -wait_i (`wait`)  or  -queue_i - coef_wait * wait_i (`hybrid`)
The objective changes rewards only; every reset clears the replica's hw."""
import numpy as np

from oracle import realnet_ref as R
from oracle.grid_ref import WAIT_EPS

OBJECTIVES = ('queue', 'wait', 'hybrid')


class NetWaitRef(R.NetBatchRef):
    def __init__(self, params, E=1, dtype=np.float64, topo=R.TOPO, objective='queue', coef_wait=0.0):
        super().__init__(params, E=E, dtype=dtype, topo=topo)
        assert objective in OBJECTIVES
        self.objective, self.coef_wait = objective, float(coef_wait)

    def reset(self, xi, mask=None):
        if mask is None:
            self.hw = np.zeros((self.E, self.tp.N, self.tp.L), dtype=self.f)
        else:
            self.hw[np.asarray(mask, dtype=bool)] = 0
        return super().reset(xi, mask)

    def served(self, action):
        """served [E,N,L] of the step `action` would take from the current state: steps 1-3 of oracle/realnet_ref.py, in
        NetBatchRef.step's own arithmetic and summation order."""
        f, E, tp = self.f, self.E, self.tp
        a = np.asarray(action).reshape(E, tp.N).astype(np.int64)
        geff = self._eff_green(self.prev, a) * self.valid
        D = np.minimum(self.q, f(R.SAT) * geff)
        out = D.sum(axis=2)
        space = np.maximum(f(R.Q_MAX) - self.q - self.tr, f(0))
        fed = tp.src >= 0
        srcc = np.maximum(tp.src, 0)
        offer = np.where(fed[None], out[:, srcc] / np.maximum(tp.fan[srcc], 1).astype(f)[None], f(0))
        acc = np.minimum(offer, space) * fed[None]
        delivered = np.zeros((E, tp.N), dtype=f)
        for i in range(tp.N):
            for k in range(tp.n_s_ls[i]):
                if fed[i, k]:
                    delivered[:, tp.src[i, k]] += acc[:, i, k]
        delivered = np.where(tp.fan[None] == 0, out, delivered)
        scale = np.where(out > f(1e-6), delivered / np.maximum(out, f(1e-6)), f(0))
        return (D * scale[:, :, None]).astype(f)

    def step(self, action):
        f = self.f
        self.last_q0 = self.q.copy()                       # the queue at the start of the step
        self.last_served = self.served(action)
        moved = (self.last_served > f(WAIT_EPS)) | (self.last_q0 <= f(WAIT_EPS))
        self.hw = (np.where(moved, f(0), self.hw + f(R.DT)) * self.valid).astype(f)
        ob, _, done, _ = super().step(action)
        c = np.minimum(self.q, f(R.DET_CAP)) * self.valid
        reward = -c.sum(axis=2)                            # queue_i, as NetBatchRef.step forms it
        if self.objective != 'queue':
            wait = self.hw.sum(axis=2)
            reward = -wait if self.objective == 'wait' else reward - f(self.coef_wait) * wait
        g = reward.sum(axis=1)
        r_out = g if self.p.coop_gamma < 0 else reward
        return ob, r_out.astype(f), done, g.astype(f)

    def near_threshold(self, margin=1e-5):
        """[E,N,L] links whose decision of the LAST step sits within `margin` of WAIT_EPS (served or the start-of-step queue):
        a comparison against another precision may leave them out."""
        return (np.abs(self.last_served - WAIT_EPS) <= margin) | (np.abs(self.last_q0 - WAIT_EPS) <= margin)

"""NumPy / torch restatement of the opt-in replica minibatches of the PPO epochs (MODEL_CONFIG ppo_minibatches): the
permutation (oracle/philox.py + np.lexsort), the gather (fancy indexing) and a literal "PPO with replica minibatches" update on torch
tensors, with the wrong variants the tests tell apart.  TEST INFRASTRUCTURE: nothing here calls the library."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import philox  # noqa: E402

STREAM_MINIBATCH = 3
F64 = torch.float64


# ------------------------------------------------------------------------------------------------------------------ permutation
def keys(E, epoch, count, seed, env_id_base=0):
    """key(e) = word x of Philox4x32-10(counter (env_id_base + e, epoch, count, 3), key seed), [E] uint32."""
    e = np.arange(E, dtype=np.uint64) + np.uint64(env_id_base)
    return philox.philox4x32(e, epoch, count, STREAM_MINIBATCH, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]


def perm_of_keys(k):
    """perm[rank(e)] = e with rank(e) = #{e' : (k[e'], e') < (k[e], e)}: ascending keys, equal keys in index order."""
    k = np.asarray(k)
    return np.lexsort((np.arange(len(k)), k)).astype(np.int32)


def perm(E, epoch, count, seed, env_id_base=0):
    return perm_of_keys(keys(E, epoch, count, seed, env_id_base))


def rank_literal(k):
    """The definition, pair by pair (small E only)."""
    E = len(k)
    out = np.zeros(E, dtype=np.int32)
    for e in range(E):
        rank = sum(1 for f in range(E) if (int(k[f]), f) < (int(k[e]), e))
        out[rank] = e
    return out


# ------------------------------------------------------------------------------------------------------------------ gather
def gather_rows(src, idx, outer, E):
    """dst[o, i] = src[o, idx[i]] for src [outer, E, inner...] given as any contiguous tensor with outer * E * inner elements."""
    v = src.reshape(outer, E, -1)
    return v[:, torch.as_tensor(np.asarray(idx), dtype=torch.long, device=src.device)].contiguous()


# ------------------------------------------------------------------------------------------------------------------ literal update
class Toy:
    """A small recurrent actor-critic in float64 (one 'agent'): h_t = tanh((1 - done_t) h_{t-1} Wh + x_t Wx), logits = h Wp, v = h wv.
    Its update is the specification's, written out: epoch 1 a full-batch A2C step on the forward pass under the weights that
    produced the batch; every epoch k >= 2 a permutation of the replicas, M steps on E / M whole sequences each, every step's
    means over its own T * E / M rows, logp_old / v_old / R / Adv those of the whole update.  Plain SGD (the optimiser is not what
    the variants are about)."""
    T, E, F, H, A = 6, 8, 3, 5, 4

    def __init__(self, seed=5):
        g = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=g, dtype=F64)      # noqa: E731
        T, E, F, H, A = self.T, self.E, self.F, self.H, self.A
        self.w0 = [0.5 * r(H, H), 0.5 * r(F, H), 0.7 * r(H, A), 0.7 * r(H)]
        self.x = r(T, E, F)
        self.done = torch.zeros(T, E, dtype=F64)
        self.done[0, ::3] = 1.0
        self.h0 = r(E, H)
        self.action = torch.randint(0, A, (T, E), generator=g)
        self.R = r(T, E)
        self.adv = r(T, E)
        self.lr, self.clip, self.v_coef, self.e_coef = 0.3, 0.2, 0.5, 0.01

    def forward(self, w, idx, t0=0, t1=None, h0=None):
        """Replicas idx, steps t0..t1 from h0 (default: the state the batch started from) -> logits [t, len(idx), A], v [t, len(idx)]."""
        Wh, Wx, Wp, wv = w
        h = self.h0[idx] if h0 is None else h0
        out = []
        for t in range(t0, self.T if t1 is None else t1):
            h = torch.tanh(((1.0 - self.done[t, idx]).unsqueeze(-1) * h) @ Wh + self.x[t, idx] @ Wx)
            out.append(h)
        hs = torch.stack(out)
        return hs @ Wp, hs @ wv

    def logp(self, logits, action):
        lp = torch.log(torch.clamp(torch.softmax(logits, -1), 1e-10, 1.0))
        return lp.gather(-1, action.unsqueeze(-1)).squeeze(-1), lp

    def step(self, w, grads):
        return [a - self.lr * g for a, g in zip(w, grads)]

    def update(self, K, M, perm_fn, wrong=None):
        """-> the weights after one update; perm_fn(k) -> the permutation of epoch k.  wrong: one of WRONG."""
        T, E = self.T, self.E
        every = torch.arange(E)
        w = [a.clone().requires_grad_() for a in self.w0]
        logits, v = self.forward(w, every)
        lpa, lp = self.logp(logits, self.action)
        logp_old, v_old = lpa.detach(), v.detach()
        ent = -(lp.exp() * lp).sum(-1)
        loss = -(lpa * self.adv).mean() + 0.5 * self.v_coef * (self.R - v).pow(2).mean() - self.e_coef * ent.mean()
        w = self.step(w, torch.autograd.grad(loss, w))
        Em = E // M
        for k in range(2, K + 1):
            pi = torch.as_tensor(np.asarray(perm_fn(2 if wrong == 'same grouping every epoch' else k)), dtype=torch.long)
            for j in range(M):
                w = [a.detach().requires_grad_() for a in w]
                if wrong == 'groups split a sequence':
                    # the group is a time slice of every replica, restarted from the batch's initial state
                    idx, t0, t1 = every, j * T // M, (j + 1) * T // M
                else:
                    idx, t0, t1 = pi[j * Em:(j + 1) * Em], 0, T
                logits, v = self.forward(w, idx, t0, t1)
                act, adv, R, lo = (z[t0:t1][:, idx] for z in (self.action, self.adv, self.R, logp_old))
                lpa, lp = self.logp(logits, act)
                if wrong == 'logp_old recomputed per group':
                    lo = lpa.detach()
                rho = torch.exp(lpa - lo)
                surr = torch.min(rho * adv, torch.clamp(rho, 1 - self.clip, 1 + self.clip) * adv)
                ent = -(lp.exp() * lp).sum(-1)
                rows = T * E if wrong == 'means over the whole batch' else surr.numel()
                loss = (-surr.sum() + 0.5 * self.v_coef * (R - v).pow(2).sum() - self.e_coef * ent.sum()) / rows
                w = self.step(w, torch.autograd.grad(loss, w))
        return [a.detach() for a in w]


WRONG = ('same grouping every epoch', 'groups split a sequence', 'means over the whole batch', 'logp_old recomputed per group')


def differs(a, b, tol=1e-6):
    return max(float((x - y).abs().max()) for x, y in zip(a, b)) > tol

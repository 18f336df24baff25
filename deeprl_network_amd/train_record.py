"""Training record -- the reference's per-update TensorBoard scalars (agents/policies.py:40-48, 265-273, written from
models.py:34-42 / policies.py:201-213: policy / value / entropy / total loss, lr, gradnorm) and critic diagnostics of every
update of the batched engine, measured by csrc/train_record.hip (specification: its header).

The batched update is a captured hipGraph that is replayed with no host code in between and the engine never synchronises per
batch, so nothing is read per update.  `TrainRecorder.record` is two small launches behind the optimiser step (inside the
captured graph: two kernel nodes) that append one row per agent to a device-resident ring; `rows()` copies the ring to the host
ONCE, where the trainer synchronises anyway (a row of train_reward.csv is due), and the writers below emit the reference's tags
and `train_summary.csv`:

    rec = TrainRecorder(model)                        # K = 64 updates fit between two drains
    ... update_apply(...); rec.record(lr); ...        # every update, no host synchronisation
    rec.note(global_step)                             # host side: the step the row is logged at
    steps, rows = rec.rows()                          # [n], [n,N,24] in commit order

Under data parallelism every rank records its OWN replicas' loss terms and statistics (`gradnorm` is the norm of the reduced
gradient, the same on all ranks) and rank 0 writes its own rows: there is no collective for the record.
"""
import numpy as np
import torch

from . import _lib, ops

COLUMNS = ('policy_loss', 'value_loss', 'entropy_loss', 'total_loss', 'lr', 'gradnorm', 'ret_mean', 'ret_std', 'value_mean',
           'explained_var', 'adv_mean', 'adv_std', 'entropy', 'rows')        # columns 0..13 of a row, in the kernel's order
N_COLS, SHARE0 = ops.TRAIN_RECORD_COLS, 16                                   # columns 14, 15 are reserved; 16 + a: action shares
CSV_NAMED = COLUMNS[:13]
# the reference's six tags in the order it creates them, each with its column
REFERENCE_TAGS = (('loss/%s_entropy_loss', 2), ('loss/%s_policy_loss', 0), ('loss/%s_value_loss', 1), ('loss/%s_total_loss', 3),
                  ('train/%s_lr', 4), ('train/%s_gradnorm', 5))
EXTRA_TAGS = (('train/%s_explained_var', 9), ('train/%s_entropy', 12), ('train/%s_value_mean', 8))


class TrainRecorder:
    """Ring [K,N,24] f32 + the committed-row counter (one buffer, so a drain is one copy) + the kernel's workspace, on the
    model's device, and the host-side list of the global steps of the updates recorded since the last drain."""

    def __init__(self, model, K=64):
        dev = torch.device(model.device)
        if dev.type != 'cuda':
            raise _lib.NmarlError('TrainRecorder needs a HIP device; there is no CPU path')
        if int(K) < 1:
            raise _lib.NmarlError('K must be at least 1')
        N, A = model.n_agent, model.n_a
        if N > ops.TRAIN_RECORD_MAX_N or A > ops.TRAIN_RECORD_MAX_A:
            raise _lib.NmarlError('the training record holds up to %d agents with up to %d actions (got %d, %d)'
                                  % (ops.TRAIN_RECORD_MAX_N, ops.TRAIN_RECORD_MAX_A, N, A))
        self.model, self.K, self.N, self.A = model, int(K), N, A
        self.rows_per_agent = model.n_step * model.E
        n = self.K * N * N_COLS
        self._buf = torch.zeros(n + 2, dtype=torch.float32, device=dev)      # (persistent addresses: captured graphs hold them)
        self.ring = self._buf[:n].view(self.K, N, N_COLS)
        self.count = self._buf[n:].view(torch.int64)                         # one int64: rows committed so far
        self.ws = ops.train_record_ws(N, self.rows_per_agent, dev)
        self.n_a = None if model.identical_agent else torch.tensor(model.n_a_ls, dtype=torch.int32, device=dev)
        self.steps = []                                                      # global step of every update not drained yet
        self.drained = 0                                                     # rows handed out by `rows()` so far

    def record(self, lr, lr_dev=None, skip_if=None):
        """The launch, directly behind `model.update_apply` (grad_norm is final there).  lr_dev: device scalar that overrides
        lr (captured updates); skip_if: the int32 device word of the batch epilogue -- while != 0 no row is written."""
        m, N, n = self.model, self.N, self.rows_per_agent
        ops.train_record(m.loss_terms(), m.grad_norm if m.per_agent_optimizer else m.grad_norm[:1], lr, m.e_coef,
                         m.R.view(N, n), m.Adv.view(N, n), m.buf_act.view(n, N), self.ring, self.count, self.ws, n_a=self.n_a,
                         lr_dev=lr_dev, skip_if=skip_if, A=self.A)

    def note(self, step):
        """Host side of an update: the global step its row is logged at."""
        self.steps.append(int(step))

    def drop(self, n):
        """Forget the last n noted updates (batches the device refused and the trainer rewinds: they left no row)."""
        if n > 0:
            del self.steps[-n:]

    def rows(self):
        """-> (steps [n], rows [n,N,24] f32) of the updates committed since the last call, in commit order.  One device-to-host
        copy, which synchronises: call it where the trainer synchronises anyway."""
        host = self._buf.cpu()
        count = int(host[-2:].view(torch.int64)[0])
        n = count - self.drained
        if n > self.K:
            raise _lib.NmarlError('training record overrun: %d updates since the last drain, the ring holds %d' % (n, self.K))
        if n != len(self.steps):
            raise _lib.NmarlError('training record out of step: the device committed %d rows, the host noted %d updates'
                                  % (n, len(self.steps)))
        ring = host[:-2].view(self.K, self.N, N_COLS).numpy()
        out = ring[[(self.drained + j) % self.K for j in range(n)]] if n else np.zeros((0, self.N, N_COLS), dtype=np.float32)
        steps, self.steps, self.drained = self.steps, [], count
        return steps, out


def scalars(name, per_agent, row, extras=True):
    """One update's row [N,24] -> [(tag, value)].  name: the reference policy's scope name (policies.py:7-11), this project's
    `policy.summary_name`.  The reference's six tags with its aggregation -- a per-agent optimiser
    (IA2C, IA2C-FP) logs agent 0's row only; a single policy sums the four loss terms over the agents (policies.py:252-255)
    and takes lr / gradnorm from row 0 -- and (extras) the mean over agents of explained_var, entropy and value_mean."""
    row = np.asarray(row, dtype=np.float64)
    out = []
    for tag, col in REFERENCE_TAGS:
        v = row[0, col] if per_agent or col >= 4 else row[:, col].sum()
        out.append((tag % name, float(v)))
    if extras:
        out += [(tag % name, float(row[:, col].mean())) for tag, col in EXTRA_TAGS]
    return out


def write_scalars(writer, name, per_agent, steps, rows, extras=True):
    """One set of scalars per update, at that update's step."""
    for step, row in zip(steps, rows):
        for tag, v in scalars(name, per_agent, row, extras):
            writer.add_scalar(tag, v, step)


def csv_columns(A):
    return ['step', 'agent_id'] + list(CSV_NAMED) + ['share_%d' % a for a in range(A)]


def csv_rows(steps, rows, A):
    """[n] steps, [n,N,24] rows -> one dict per (update, agent) with the columns of train_summary.csv."""
    cols = csv_columns(A)
    out = []
    for step, upd in zip(steps, np.asarray(rows, dtype=np.float64)):
        for i, r in enumerate(upd):
            out.append(dict(zip(cols, [int(step), i] + r[:13].tolist() + r[SHARE0:SHARE0 + A].tolist())))
    return out


def write_csv(path, data, A):
    import pandas as pd
    pd.DataFrame(data, columns=csv_columns(A)).to_csv(path, index=False)


def host_row(model):
    """The E = 1 reference path (A2CModel.backward synchronises every step anyway): columns 0..5 of the row from plain host
    reads of the last update's loss terms, learning rate and gradient norm; the other columns stay 0."""
    terms = model.loss_terms().detach().cpu().numpy().astype(np.float32)
    gn = model.grad_norm.detach().cpu().numpy().astype(np.float32)
    row = np.zeros((model.n_agent, N_COLS), dtype=np.float32)
    row[:, :3] = terms
    row[:, 3] = ((terms[:, 0].astype(np.float64) + terms[:, 1]) + terms[:, 2]).astype(np.float32)
    row[:, 4] = np.float32(model.cur_lr)
    row[:, 5] = gn if model.per_agent_optimizer else gn[0]
    return row

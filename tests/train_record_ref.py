"""TEST-ONLY restatement of the training record's row (csrc/train_record.hip) in NumPy float64, written from the
specification and not from the kernel."""
import numpy as np

N_COLS = 24


def train_record_ref(terms, grad_norm, lr, e_coef, R, Adv, action, n_a=None):
    """terms [N,3] f32, grad_norm [G] f32 (agent i reads entry min(i, G - 1)), lr, e_coef scalars, R / Adv [N,rows] f32,
    action [rows,N] u8, n_a [N] own action counts or None (then: as many as there are share columns, 8) -> [N,24] float64."""
    terms = np.asarray(terms, dtype=np.float32)
    grad_norm = np.asarray(grad_norm, dtype=np.float32).reshape(-1)
    R = np.asarray(R, dtype=np.float32).astype(np.float64)
    Adv = np.asarray(Adv, dtype=np.float32).astype(np.float64)
    action = np.asarray(action)
    N, n = R.shape
    assert terms.shape == (N, 3) and Adv.shape == (N, n) and action.shape == (n, N)
    V = R - Adv                                              # the value the return scan used
    out = np.zeros((N, N_COLS), dtype=np.float64)
    for i in range(N):
        c0, c1, c2 = (float(x) for x in terms[i])
        ret_mean = R[i].sum() / n
        var_r = (R[i] ** 2).sum() / n - ret_mean ** 2
        adv_mean = Adv[i].sum() / n
        var_a = (Adv[i] ** 2).sum() / n - adv_mean ** 2
        out[i, 0], out[i, 1], out[i, 2] = c0, c1, c2
        out[i, 3] = c0 + c1 + c2
        out[i, 4] = np.float32(lr)
        out[i, 5] = grad_norm[min(i, len(grad_norm) - 1)]
        out[i, 6] = ret_mean
        out[i, 7] = np.sqrt(max(var_r, 0.0))
        out[i, 8] = V[i].sum() / n
        out[i, 9] = 1.0 - var_a / var_r if var_r > 0 else 0.0
        out[i, 10] = adv_mean
        out[i, 11] = np.sqrt(max(var_a, 0.0))
        out[i, 12] = -c2 / float(e_coef) if e_coef != 0 else 0.0
        out[i, 13] = n
        own = N_COLS - 16 if n_a is None else int(n_a[i])
        for a in range(own):
            out[i, 16 + a] = np.count_nonzero(action[:, i] == a) / n
    return out

"""Same-box, same-process A/B of lstm_dial's reverse recurrence: nmarl_lstm_bptt_dial (one launch) against the step-wise pair
nmarl_lstm_bptt_step + nmarl_dial_msg_adjoint it replaces, on config_ma2c_dial_catchup.ini at 8 x 4096, n_step 60.
The 'pair' arm is this tree with ops.bptt_dial_supported patched to False: the engine then runs the previous commit's path, whose
code and kernels this commit does not touch (the previous commit's library cannot be loaded next to this binding through
tools/ab_build.sh: its C-ABI lacks the new entry point).  Arms alternate, RUNS runs each.  'recurrence stamped' is the DURATION of the
reverse recurrence inside the captured update: two nmarl_timestamp launches (device wall clock), one in front of the arm's first
recurrence launch and one behind its last (one launch: around nmarl_lstm_bptt_dial; pair: in front of the first nmarl_lstm_bptt_step,
behind the T-th nmarl_dial_msg_adjoint), median of 5 replays.  The shader-clock account of one step: tools/bptt_timeline.py dial.
    python tools/ab_dial_bptt.py [RUNS=3] [BATCHES=20]"""
import configparser
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import graph_nodes as GN  # noqa: E402
from deeprl_network_amd import _lib, ops  # noqa: E402
from deeprl_network_amd.envs import make_batch_env  # noqa: E402
from deeprl_network_amd.main import AGENTS  # noqa: E402
from deeprl_network_amd.utils import BatchedTrainer, Counter  # noqa: E402

RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
B = int(sys.argv[2]) if len(sys.argv) > 2 else 20
E = 4096
real_supported = ops.bptt_dial_supported


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def stamped_recurrence(tr, first, last, n_last):
    """Re-captures the update with a time stamp in front of the first call of entry point `first` and one behind call number `n_last`
    of `last`; replays it 5 times on a snapshot of the trainer's state -> median stamp difference in us."""
    stamps = torch.zeros(2, dtype=torch.int64, device='cuda')
    f_first, f_last = getattr(_lib.lib, first), getattr(_lib.lib, last)
    seen = [0, 0]

    def w_first(*a, **k):
        if seen[0] == 0:
            ops.timestamp(stamps[0:1])
        seen[0] += 1
        return (w_last if first == last else f_first)(*a, **k)

    def w_last(*a, **k):
        rc = f_last(*a, **k)
        seen[1] += 1
        if seen[1] == n_last:
            ops.timestamp(stamps[1:2])
        return rc
    keep = tr._upd
    try:
        setattr(_lib.lib, last, w_last)
        setattr(_lib.lib, first, w_first)
        tr._upd = None
        tr._capture_update()
        g = tr._upd
    finally:
        setattr(_lib.lib, first, f_first)
        setattr(_lib.lib, last, f_last)
        tr._upd = keep
    assert seen[1] == n_last, (first, last, seen)
    snap = tr._snapshot()
    ticks = []
    for _ in range(6):
        g['grads'].replay()
        if g['apply'] is not None:
            g['apply'].replay()
        ticks.append(int((stamps[1] - stamps[0]).item()))
    tr._restore(snap)
    return sorted(ticks[1:])[2] / ops.timestamp_rate_khz(torch.device('cuda')) * 1e3


def trainer_run(arm):
    ops.bptt_dial_supported = real_supported if arm == 'one launch' else (lambda *a, **k: False)
    cp = configparser.ConfigParser()
    cp.read(os.path.join(ROOT, 'config', 'config_ma2c_dial_catchup.ini'))
    env = make_batch_env(cp['ENV_CONFIG'], num_envs=E)
    np.random.seed(12)
    model = AGENTS[env.agent](env.n_s_ls, env.n_a_ls, env.neighbor_mask, env.distance_mask, env.coop_gamma, 10 ** 9, cp['MODEL_CONFIG'],
                              seed=12, num_envs=E)
    tr = BatchedTrainer(env, model, Counter(10 ** 12, 10 ** 12, 10 ** 12), use_graph=True, keep_graphs=True)
    for _ in range(3):
        tr.run_batch()
    ms = timed(tr.run_batch, B)
    tr.flush()
    ops.check_coupled_status()
    assert tr.handoff_fallbacks == 0 and tr._upd is not None
    N, T = model.n_agent, model.n_step
    snap = tr._snapshot()
    upd = timed(tr._upd['grads'].replay, 10)
    tr._restore(snap)
    k_roll, k_upd = GN.census(tr.graph)['kernel'], GN.census(tr._upd['grads'])['kernel']
    k_apply = GN.census(tr._upd['apply'])['kernel'] if tr._upd['apply'] is not None else 0
    if arm == 'one launch':
        us = stamped_recurrence(tr, 'nmarl_lstm_bptt_dial', 'nmarl_lstm_bptt_dial', 1)
    else:
        us = stamped_recurrence(tr, 'nmarl_lstm_bptt_step', 'nmarl_dial_msg_adjoint', T)
    tb = N * E * T * 4640 / us / 1e6
    print('%-10s batch %.3f ms  %.1f M env-steps/s (agents x replicas x n_step / batch)  update graph alone %.3f ms  recurrence stamped '
          'inside the update %.1f us%s  kernels per batch %d (rollout %d + update %d)  dy8 %s'
          % (arm, ms, N * E * T / ms / 1e3, upd, us, ' (%.2f TB/s algorithmic = %.2f of the 8 TB/s HBM peak)' % (tb, tb / 8.0)
             if arm == 'one launch' else '', k_roll + k_upd + k_apply, k_roll, k_upd + k_apply, model.policy.bptt_takes_head_dy), flush=True)
    ops.bptt_dial_supported = real_supported


def op_run():
    """The recurrence alone at the same shape on random operands: the one launch (dy8 form, as the update uses it; includes its
    flag-clearing launch) against the 60 launch pairs (tensor form of the heads' gradient, as the update hands it to them)."""
    N, T, H = 8, 60, 64
    rd = lambda *s: torch.randn(*s, device='cuda')            # noqa: E731
    nm = np.zeros((N, N), dtype=int)
    for i in range(N - 1):
        nm[i, i + 1] = nm[i + 1, i] = 1
    idx, _ = ops.neighbor_table(nm, 'cuda')
    G = torch.cat([torch.sigmoid(rd(N, T, E, 3 * H)), torch.tanh(rd(N, T, E, H))], dim=-1)
    Cc, done = rd(N, T + 1, E, H) * 0.5, torch.zeros(T, E, device='cuda')
    dy8, hw = torch.zeros(N, T * E, 8, device='cuda'), rd(N, H, 5) * 0.3
    dy8[:, :, :5] = rd(N, T * E, 5)
    dHs = ops.head_dy_to_dh(dy8, hw, (N, T, E, H))
    wx, wh, w_msg, mfc_w = rd(N, H, 4 * H) * 0.1, rd(N, H, 4 * H) * 0.1, rd(N, 2 * H, H) * 0.15, rd(N, H, H) * 0.2
    hm, msg = torch.relu(rd(N, T, E, H)), torch.relu(rd(N, T + 1, E, H))
    dZ, DS, D1, D2 = torch.empty_like(G), rd(N, T, E, H), rd(N, T + 1, E, H), rd(N, T + 1, E, H)
    rev = ops.reverse_neighbor_table(idx, ops.COUPLED_NC)
    ws = (wx, wh, ops.lstm_bptt_wimage(wx, wh))
    wm = (w_msg, ops.lstm_bptt_msg_wimage(w_msg))
    img_f = ops.lstm_bptt_msg_wimage(mfc_w)
    imgs = ops.dial_adjoint_images(w_msg, mfc_w)
    dhd, dh, dc, dc2 = rd(N, E, H), rd(N, E, H), torch.zeros(N, E, H, device='cuda'), torch.zeros(N, E, H, device='cuda')
    dbp, parts = ops.bptt_step_db_parts(N, E, H, 'cuda'), ops.dial_adjoint_bias_parts(N, E, 'cuda')

    def new(mode=0):
        ops.bptt_dial(rev, 2, G, Cc, done, None, ws, wm, img_f, hm, msg, dZ, DS, D1[:, :T], D2[:, :T], head_dy=(dy8, hw), mode=mode)

    def pair():
        rec = None
        a, b = dc, dc2
        for t in range(T - 1, -1, -1):
            ops.bptt_step(G[:, t], Cc[:, t], Cc[:, t + 1], done[t], dHs[:, t], rec, a, ws, dZ[:, t], b, dhd, t == 0, dx=DS[:, t], db_part=dbp)
            a, b = b, a
            rec = ops.dial_msg_adjoint(DS[:, t], hm[:, t], msg[:, t], dhd, w_msg, mfc_w, idx, imgs, rev, D1[:, t], D2[:, t], dh, bias_parts=parts)
    for _ in range(RUNS):
        t_new, t_pair, t_sw = timed(new, 5), timed(pair, 5), timed(lambda: new(2), 3)
        ops.check_coupled_status()
        # algorithmic bytes per (agent, replica, step), dy8 form: read gates 1024 + c 256 + dy8 32 + hm 256 + msg 256 + ring 2 x 256 (interior
        # agents; ends 256), written dz 1024 + ds, d1, d2 3 x 256 + ring 512
        byt = N * E * T * (1024 + 256 + 32 + 256 + 256 + 512 + 1024 + 768 + 512)
        print('recurrence alone: one launch %.3f ms (%.2f TB/s algorithmic, 4640 B per row-step)   60 launch pairs %.3f ms   '
              'step-wise form of the new kernel (61 launches) %.3f ms' % (t_new, byt / t_new / 1e9, t_pair, t_sw), flush=True)


if __name__ == '__main__':
    print(torch.cuda.get_device_name(0))
    op_run()
    for _ in range(RUNS):
        for arm in ('pair', 'one launch'):
            trainer_run(arm)

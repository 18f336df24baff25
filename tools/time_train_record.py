"""The training record's cost (nmarl_train_record, csrc/train_record.hip: two launches behind the optimiser step).
1. The call alone at the headline shape (N = 8, rows = 60 x 4096) and the grid shape (N = 25, rows = 120 x 1024): median of 200
   calls, each between its own pair of events, after a warm-up.
2. Same-box, same-process A/B of ms per batch with record=True against record=False for config_ia2c_fp_catchup.ini at 8 x 4096:
   the two trainers are built once and their timed windows alternate.
    python tools/time_train_record.py [RUNS=5] [BATCHES=20]"""
import configparser
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from deeprl_network_amd import ops  # noqa: E402
from deeprl_network_amd.envs import make_batch_env  # noqa: E402
from deeprl_network_amd.main import init_agent  # noqa: E402
from deeprl_network_amd.utils import BatchedTrainer, Counter, SummaryWriter  # noqa: E402

RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
BATCHES = int(sys.argv[2]) if len(sys.argv) > 2 else 20
N_CALL, WARM = 200, 20


def median_us(fn):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(N_CALL)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) * 1e3 for a, b in ev]))


print('1. the call alone (two launches), median of %d calls between event pairs' % N_CALL)
for label, N, rows, A in (('headline (8 x 60 x 4096)', 8, 60 * 4096, 4), ('grid (25 x 120 x 1024)', 25, 120 * 1024, 5)):
    g = torch.Generator(device='cuda').manual_seed(1)
    R = torch.randn(N, rows, device='cuda', generator=g) * 2 - 3
    Adv = torch.randn(N, rows, device='cuda', generator=g)
    act = torch.randint(0, A, (rows, N), device='cuda', generator=g).to(torch.uint8)
    terms, gn = torch.randn(N, 3, device='cuda', generator=g), torch.ones(N, device='cuda')
    ring, count = torch.zeros(64, N, 24, device='cuda'), torch.zeros(1, dtype=torch.int64, device='cuda')
    ws = ops.train_record_ws(N, rows, 'cuda')

    def call():
        ops.train_record(terms, gn, 5e-4, 0.01, R, Adv, act, ring, count, ws, A=A)
    for _ in range(WARM):
        call()
    torch.cuda.synchronize()
    t = median_us(call)
    nbytes = 9 * N * rows
    print('   %-26s %7.2f us per call; %.1f MB read (R, Adv, actions) -> %.3f TB/s algorithmic' % (label, t, nbytes / 1e6, nbytes / t / 1e6))

print('2. ms per batch, config_ia2c_fp_catchup.ini at 8 x 4096, hipGraph rollout + update, %d batches per window, windows alternate' % BATCHES)
cp = configparser.ConfigParser()
cp.read(os.path.join(ROOT, 'config', 'config_ia2c_fp_catchup.ini'))
arms = {}
for arm in ('record', 'no record'):
    env = make_batch_env(cp['ENV_CONFIG'], num_envs=4096)
    np.random.seed(12)
    model = init_agent(env, cp['MODEL_CONFIG'], 10 ** 9, 12, num_envs=4096)
    tr = BatchedTrainer(env, model, Counter(10 ** 12, 10 ** 12, 10 ** 12), use_graph=True,
                        summary_writer=SummaryWriter(None) if arm == 'record' else None, record=(arm == 'record'), record_slots=64)
    for _ in range(5):
        tr.run_batch()
    torch.cuda.synchronize()
    assert tr._upd is not None and tr.update_capture_error is None
    arms[arm] = tr
ms = {arm: [] for arm in arms}
for _ in range(RUNS):
    for arm, tr in arms.items():
        if tr.recorder is not None:
            tr.recorder.rows()                 # (the drain a logged row makes, outside the window)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(BATCHES):
            tr.run_batch()
        torch.cuda.synchronize()
        ms[arm].append((time.perf_counter() - t0) * 1e3 / BATCHES)
for arm, v in ms.items():
    print('   %-10s ms per batch: %s  median %.3f' % (arm, ' '.join('%.3f' % x for x in v), float(np.median(v))))
a, b = float(np.median(ms['record'])), float(np.median(ms['no record']))
print('   record / no record = %.4f (%+.2f %%)' % (a / b, (a / b - 1) * 100))

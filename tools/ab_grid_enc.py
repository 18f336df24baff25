"""Same-box, same-process A/B of the uncoupled nets' lock-step on the 5 x 5 ATSC grid: the input encoders INSIDE the policy + value
launch (lstm_step_x_kernel<3,0,3> / <3,0,4>, the default) against the separate encoder launch in front of it (NMARL_INKERNEL_ENCODE=0:
the previous commit's path, whose code and kernels this commit does not touch; the previous commit's library cannot be loaded next
to this binding through tools/ab_build.sh, its C-ABI version differs).  config_ia2c_fp_grid's settings (the grid config with agent =
ia2c_fp, coop_gamma = 0.95, reward_norm = 100) at 25 x 1024 replicas, n_step 120.  Arms alternate, RUNS runs each; per run: ms per batch
(rollout graph + update graph) and the kernel nodes of the captured graphs.
    python tools/ab_grid_enc.py [RUNS=3] [BATCHES=10] [AGENT=ia2c_fp]"""
import configparser
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import graph_nodes as GN  # noqa: E402
from deeprl_network_amd.envs import make_batch_env  # noqa: E402
from deeprl_network_amd.main import init_agent  # noqa: E402
from deeprl_network_amd.utils import BatchedTrainer, Counter  # noqa: E402

RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
B = int(sys.argv[2]) if len(sys.argv) > 2 else 10
AGENT = sys.argv[3] if len(sys.argv) > 3 else 'ia2c_fp'
E = 1024
SETTINGS = {'ia2c_fp': ('0.95', '100.0'), 'ia2c': ('0.9', '100.0'), 'ma2c_cu': ('0.9', '100.0')}      # coop_gamma, reward_norm


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


def trainer_run(arm):
    os.environ['NMARL_INKERNEL_ENCODE'] = '1' if arm == 'in-kernel' else '0'
    cp = configparser.ConfigParser()
    cp.read(os.path.join(ROOT, 'config', 'config_ma2c_cnet_grid.ini'))
    cp['ENV_CONFIG']['agent'] = AGENT
    cp['ENV_CONFIG']['coop_gamma'], cp['MODEL_CONFIG']['reward_norm'] = SETTINGS[AGENT]
    env = make_batch_env(cp['ENV_CONFIG'], num_envs=E)
    np.random.seed(12)
    model = init_agent(env, cp['MODEL_CONFIG'], 10 ** 9, 12, num_envs=E)
    tr = BatchedTrainer(env, model, Counter(10 ** 12, 10 ** 12, 10 ** 12), use_graph=True, keep_graphs=True)
    assert tr.enc_in_kernel == (arm == 'in-kernel')
    for _ in range(3):
        tr.run_batch()
    ms = timed(tr.run_batch, B)
    tr.flush()
    assert tr._upd is not None and tr.update_capture_error is None
    snap = tr._snapshot()
    roll = timed(tr.graph.replay, 5)
    tr._restore(snap)
    N, T = model.n_agent, model.n_step
    k_roll, k_upd = GN.census(tr.graph)['kernel'], GN.census(tr._upd['grads'])['kernel']
    k_apply = GN.census(tr._upd['apply'])['kernel'] if tr._upd['apply'] is not None else 0
    print('%-9s batch %.3f ms  %.1f M env-steps/s (agents x replicas x n_step / batch)  rollout graph alone %.3f ms  kernels per batch %d '
          '(rollout %d = %.2f per lock-step + update %d)' % (arm, ms, N * E * T / ms / 1e3, roll, k_roll + k_upd + k_apply, k_roll,
                                                            k_roll / (T + 1), k_upd + k_apply), flush=True)
    del tr, model, env
    torch.cuda.empty_cache()


if __name__ == '__main__':
    print('%s on the 5 x 5 grid, 25 x %d replicas, n_step 120, %s' % (AGENT, E, torch.cuda.get_device_name(0)), flush=True)
    for r in range(RUNS):
        for arm in ('separate', 'in-kernel'):
            trainer_run(arm)

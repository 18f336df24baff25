"""`main.py evaluate` with and without --batched: wall time of the whole evaluation, and the greedy launch alone.
    python tools/time_batched_evaluate.py [--seeds N=50] [--graph] > profiles/r15_batched_evaluate.txt

Per scenario (config_greedy.ini: the rule-based agent on the 5x5 grid; config_ia2c_fp_catchup.ini: IA2C-FP on CACC, randomly
initialised weights -- the time does not depend on them) at the ini's full episode length, the default evaluation seeds
2000, 2010, ...: wall time around `Evaluator.run` (one replica, seed after seed) and around `BatchedEvaluator.run` (all seeds
as one batch), each after one warm-up (the one-replica warm-up runs 2 seeds: its steps are all alike), each ending in a device
synchronise or a read-back.  Both write their CSVs, as the CLI does.  --graph also times `use_graph=True`.
Then nmarl_atsc_greedy alone between two events, E = 64 and 1024, on the grid (compact and slab rows) and on the network's
own vectors staged in rows of 24 floats, as GreedyBatchController hands them over."""
import argparse
import configparser
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from deeprl_network_amd import ops  # noqa: E402
from deeprl_network_amd.envs import init_env, make_batch_env  # noqa: E402
from deeprl_network_amd.envs.greedy import GreedyBatchController  # noqa: E402
from deeprl_network_amd.main import model_config, init_agent  # noqa: E402
from deeprl_network_amd.utils import BatchedEvaluator, Evaluator  # noqa: E402


def config(name):
    cp = configparser.ConfigParser()
    cp.read(os.path.join(ROOT, 'config', name))
    return cp


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def one_replica(cp, seeds, out):
    env = init_env(cp['ENV_CONFIG'], port=1)
    model = init_agent(env, model_config(cp), 0, 0)
    env.init_test_seeds(seeds[:2])
    Evaluator(env, model, out, gui=False).run()                 # warm-up
    env.init_test_seeds(seeds)
    sec, means = timed(Evaluator(env, model, out, gui=False).run)
    return sec, means, env.T


def batched(cp, seeds, out, use_graph):
    env = make_batch_env(cp['ENV_CONFIG'], num_envs=len(seeds))
    np.random.seed(cp['ENV_CONFIG'].getint('seed'))             # the initial weights init_env's seeding gives the one-replica model
    model = GreedyBatchController(env) if env.agent == 'greedy' else init_agent(env, model_config(cp), 0, 0, num_envs=len(seeds))
    ev = BatchedEvaluator(env, model, seeds, out, use_graph=use_graph)
    ev.run()                                                    # warm-up (and, with use_graph, the capture)
    sec, means = timed(ev.run)
    return sec, means


def greedy_alone(name, obs_row, E, reps=200):
    from deeprl_network_amd.envs.large_grid_env import grid_greedy_table
    from deeprl_network_amd.envs.real_net_env import NODE_DEFS, net_greedy_table
    n_a, mask = grid_greedy_table(5, 5) if name == 'grid' else net_greedy_table(sorted(n for n, _, _ in NODE_DEFS))
    N = len(n_a)
    n_a_d, mask_d = torch.from_numpy(n_a).cuda(), torch.from_numpy(mask.view(np.int32)).cuda()
    obs = torch.rand(E, N, obs_row, device='cuda')
    out = torch.zeros(E, N, dtype=torch.uint8, device='cuda')
    for _ in range(20):
        ops.atsc_greedy(n_a_d, mask_d, obs, out, a_max=int(n_a.max()))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        ops.atsc_greedy(n_a_d, mask_d, obs, out, a_max=int(n_a.max()))
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) * 1e3 / reps
    nbytes = E * N * (16 * min(6, obs_row // 4) + 1)
    return us, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seeds', type=int, default=50)
    ap.add_argument('--graph', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X'
    seeds = list(range(2000, 2000 + 10 * args.seeds, 10))
    print('batched evaluation vs the one-replica evaluation, %d seeds, %s' % (len(seeds), torch.cuda.get_device_name(0)))
    for ini in ('config_greedy.ini', 'config_ia2c_fp_catchup.ini'):
        cp = config(ini)
        with tempfile.TemporaryDirectory() as tmp:
            dirs = {k: os.path.join(tmp, k) + '/' for k in ('one', 'batched', 'graph')}
            for d in dirs.values():
                os.makedirs(d)
            s1, m1, T = one_replica(cp, seeds, dirs['one'])
            sb, mb = batched(cp, seeds, dirs['batched'], use_graph=False)
            line = ('%s (agent %s, T = %d): one replica %.3f s = %.3f ms per lock-step; batched (eager) %.3f s = %.3f ms per '
                    'lock-step of %d replicas; ratio %.1fx' % (ini, cp['ENV_CONFIG']['agent'], T, s1, s1 / (len(seeds) * T) * 1e3,
                                                               sb, sb / T * 1e3, len(seeds), s1 / sb))
            if args.graph:
                sg, _ = batched(cp, seeds, dirs['graph'], use_graph=True)
                line += '; batched (one hipGraph) %.3f s, ratio %.1fx' % (sg, s1 / sg)
            print(line)
            print('    mean reward over the seeds: one replica %.3f, batched %.3f' % (float(np.mean(m1)), float(np.mean(mb))))
    print('nmarl_atsc_greedy alone (between two events, 200 launches back to back):')
    for name, row in (('grid', 12), ('grid', 60), ('net', 24)):
        for E in (64, 1024):
            us, nbytes = greedy_alone(name, row, E)
            print('    %-4s row %3d floats, E = %4d: %.2f us per launch, %d algorithmic bytes (%.1f GB/s)'
                  % (name, row, E, us, nbytes, nbytes / us * 1e-3))


if __name__ == '__main__':
    main()

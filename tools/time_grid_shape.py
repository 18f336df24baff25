"""The synthetic-grid step kernel on other lattices (nmarl_grid_step_rc: 3x3, 5x5, 4x8) next to the fixed 5x5 kernel
(nmarl_grid_step) of the same build, auto-reset on, at E = 1024 and 2^17: us per launch between two events and the fraction of the
8 TB/s peak on the algorithmic bytes of a replica-step,

    compact observation: 147 N + 33     slab: 339 N + 33

(q and transit read and written 2 x 2 x 24 N, the observation 48 N or 240 N, action N, prev_action read and written 2 N; t read and
written 8, xi 16, reward + global reward + done 9 -- 3 708 B at N = 25, the formula of bench.py).  python tools/time_grid_shape.py"""
import os
import sys
import configparser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from deeprl_network_amd.envs.large_grid_env import LargeGridBatchEnv

CASES = [('5x5 fixed', 5, 5, False), ('5x5 _rc', 5, 5, True), ('3x3 _rc', 3, 3, True), ('4x8 _rc', 4, 8, True)]


def time_case(rows, cols, rc, E, compact):
    cp = configparser.ConfigParser()
    cp.read(os.path.join(ROOT, 'config', 'config_ma2c_cnet_grid.ini'))
    cp['ENV_CONFIG']['grid_rows'], cp['ENV_CONFIG']['grid_cols'] = str(rows), str(cols)
    env = LargeGridBatchEnv(cp['ENV_CONFIG'], num_envs=E)
    env.fixed_shape = not rc
    env.set_compact_obs(compact)
    env.reset()
    e = torch.arange(E, device='cuda')[:, None]
    a = torch.arange(env.n_agent, device='cuda')[None, :]
    acts = [((e + 3 * a + s) % 5).to(torch.uint8).contiguous() for s in range(4)]
    for s in range(10):
        env.step(acts[s % 4], auto_reset=True)
    torch.cuda.synchronize()
    n = 200 if E <= (1 << 15) else 60
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = None
    for rep in range(3):
        t0.record()
        for s in range(n):
            env.step(acts[s % 4], auto_reset=True)
        t1.record()
        torch.cuda.synchronize()
        us = t0.elapsed_time(t1) * 1e3 / n
        best = us if best is None else min(best, us)
    return best, (147 if compact else 339) * env.n_agent + 33


def main():
    print('nmarl_grid_step (5x5 fixed) and nmarl_grid_step_rc, queue objective, auto-reset on; best of 3 runs of 200 (60 at 2^17) '
          'launches between two events; bytes per replica-step: 147 N + 33 (compact), 339 N + 33 (slab)')
    for E in (1024, 1 << 17):
        for compact in (True, False):
            base = None
            for name, rows, cols, rc in CASES:
                us, nbytes = time_case(rows, cols, rc, E, compact)
                if base is None:
                    base = us
                rel = '' if (rows, cols) != (5, 5) or not rc else '   (%.3f x the fixed 5x5 kernel)' % (us / base)
                print('E = %7d  %-7s  %-9s  N = %2d: %9.2f us per step = %.3f of 8 TB/s on %5d B per replica-step%s' % (
                    E, 'compact' if compact else 'slab', name, rows * cols, us, E * nbytes / us / 8e6, nbytes, rel))


if __name__ == '__main__':
    main()

"""The CACC env step ALONE for platoons of several lengths, one process, compact observation, E * N = 2^24 vehicles per arm.

    python tools/platoon_env_bench.py [--steps 20] [--runs 3] [--lanes 16777216]

Arms: N = 4, 16, 32 through the any-length kernel (cacc_step_nv_kernel: one lane per vehicle, groups of G = 4 / 16 / 32 lanes);
N = 8 through the any-length kernel, through cacc_step4_kernel (four vehicles per lane, what nmarl_cacc_step launches at this size)
and through cacc_step_kernel (lane per vehicle, NMARL_CACC_QUAD=0).  The arms alternate, `--runs` timed runs each, every run
`--steps` launches between two HIP events after a warm-up.  Reported: microseconds per launch (median of the runs, and each run)
and the fraction of the 8 TB/s HBM peak on the ALGORITHMIC bytes (41 N + 23) E per step (351 B at N = 8).
No threshold: this tool records where the lane-per-vehicle mapping of the new sizes stands against the N = 8 quad mapping."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))

HBM_PEAK = 8.0e12


def make_arm(name, N, lanes, form):
    from helpers import cacc_config
    from deeprl_network_amd import _lib
    from deeprl_network_amd.envs.cacc_env import CACCBatchEnv
    cp = cacc_config('ma2c_nc', 'catchup')
    cp['ENV_CONFIG']['n_vehicle'] = str(N)
    E = lanes // N
    env = CACCBatchEnv(cp['ENV_CONFIG'], num_envs=E)
    env.set_compact_obs(True)
    env.reset()
    act = torch.randint(0, 4, (E, N), dtype=torch.uint8, device='cuda')
    P = _lib.ptr

    def step():
        if form == 'nv':        # the any-length entry, also for N = 8 (CACCBatchEnv.step would take the 8-vehicle kernels there)
            rc = _lib.lib.nmarl_cacc_step_nv(
                ctypes.byref(env.params), env.E, P(act), P(env.h), P(env.v), P(env.u), P(env.t), P(env.collided), P(env.v0_init),
                P(env.obs), P(env.reward), P(env.done), P(env.global_reward), 1, env.seed, env.env_id_base, P(env.episode), N,
                _lib.stream())
            _lib.check(rc, 'nmarl_cacc_step_nv')
        else:
            os.environ['NMARL_CACC_QUAD'] = '1' if form == 'quad' else '0'
            env.step(act, auto_reset=True)
    return dict(name=name, N=N, E=E, step=step, us=[])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--lanes', type=int, default=1 << 24)
    args = ap.parse_args()
    arms = [make_arm('nv   N=4  (G=4)', 4, args.lanes, 'nv'), make_arm('nv   N=8  (G=8)', 8, args.lanes, 'nv'),
            make_arm('quad N=8  (cacc_step4_kernel)', 8, args.lanes, 'quad'), make_arm('lane N=8  (cacc_step_kernel)', 8, args.lanes, 'lane'),
            make_arm('nv   N=16 (G=16)', 16, args.lanes, 'nv'), make_arm('nv   N=32 (G=32)', 32, args.lanes, 'nv')]
    for arm in arms:
        for _ in range(5):
            arm['step']()
    torch.cuda.synchronize()
    for _ in range(args.runs):
        for arm in arms:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            arm['step']()
            t0.record()
            for _ in range(args.steps):
                arm['step']()
            t1.record()
            t1.synchronize()
            arm['us'].append(t0.elapsed_time(t1) * 1000.0 / args.steps)
    print('CACC env step alone, compact observation, E * N = %d vehicles per arm, %d launches per run, %d alternating runs'
          % (args.lanes, args.steps, args.runs))
    print('device: %s' % torch.cuda.get_device_name())
    print('%-34s %3s %9s %10s %12s %9s   runs (us)' % ('arm', 'N', 'E', 'us/launch', 'B_alg/step', 'of 8 TB/s'))
    for arm in arms:
        us = statistics.median(arm['us'])
        b = (41 * arm['N'] + 23) * arm['E']
        print('%-34s %3d %9d %10.1f %12d %9.3f   %s' % (arm['name'], arm['N'], arm['E'], us, b, b / (us * 1e-6) / HBM_PEAK,
                                                          ' '.join('%.1f' % x for x in arm['us'])))


if __name__ == '__main__':
    main()

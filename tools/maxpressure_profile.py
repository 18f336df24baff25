"""First measurements of the `maxpressure` ATSC agent next to `greedy`, one box, one run:
    python tools/maxpressure_profile.py [--seeds N=50] > profiles/r17_maxpressure.txt

Every GPU step is a child process of its own under its own time limit; the first step that fails, faults or runs out of time
ends the run (nothing more is started on the device behind it).
  launch     nmarl_atsc_maxpressure and nmarl_atsc_greedy between two events, 200 launches back to back, E = 64 and 1024, on the
             observation buffers of the two batch envs as they are (greedy on the network: its staged rows of 24 floats).  The
             figure is the floor of an eager launch, not a kernel duration.
  evaluate   BatchedEvaluator over the default evaluation seeds 2000, 2010, ... at the ini's full episode length, both scenarios,
             both rule-based agents: mean global reward per lock-step and mean of the traffic table's avg_queue, over the seed set.
The kernel's registers, LDS and scratch are the compiler's (-Rpass-analysis=kernel-resource-usage) and are quoted by hand."""
import argparse
import configparser
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = [('launch', 240)] + [('evaluate:%s:%s' % (s, a), 300) for s in ('grid', 'net') for a in ('maxpressure', 'greedy')]
INIS = {'grid': 'config_maxpressure.ini', 'net': 'config_maxpressure_net.ini'}


def config(scenario, agent):
    cp = configparser.ConfigParser()
    assert cp.read(os.path.join(ROOT, 'config', INIS[scenario]))
    cp['ENV_CONFIG']['agent'] = agent
    return cp


def controller(env):
    from deeprl_network_amd.envs.greedy import GreedyBatchController
    from deeprl_network_amd.envs.maxpressure import MaxPressureBatchController
    return MaxPressureBatchController(env) if env.agent == 'maxpressure' else GreedyBatchController(env)


def launch(reps=200):
    import torch
    from deeprl_network_amd.envs import make_batch_env
    print('one controller launch between two events, %d launches back to back, %s' % (reps, torch.cuda.get_device_name(0)))
    for scenario in ('grid', 'net'):
        for E in (64, 1024):
            for agent in ('maxpressure', 'greedy'):
                env = make_batch_env(config(scenario, agent)['ENV_CONFIG'], num_envs=E)
                env.reset()
                env.obs.copy_(torch.rand_like(env.obs))
                ctl = controller(env)
                out = torch.zeros(E, env.n_agent, dtype=torch.uint8, device='cuda')
                if agent == 'greedy':
                    ctl.forward_batch(env.obs, out)        # (the network's staging copy is made once, outside the window)
                    obs = env.obs if ctl._own is None else ctl._own
                else:
                    obs = env.obs
                for _ in range(20):
                    ctl.forward_batch(obs, out)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                for _ in range(reps):
                    ctl.forward_batch(obs, out)
                b.record()
                torch.cuda.synchronize()
                print('    %-4s %-11s row %3d floats, E = %4d: %6.2f us per launch'
                      % (scenario, agent, obs.shape[2], E, a.elapsed_time(b) * 1e3 / reps))


def evaluate(scenario, agent, n_seeds):
    import numpy as np
    from deeprl_network_amd.envs import make_batch_env
    from deeprl_network_amd.utils import BatchedEvaluator
    seeds = list(range(2000, 2000 + 10 * n_seeds, 10))
    cp = config(scenario, agent)
    env = make_batch_env(cp['ENV_CONFIG'], num_envs=len(seeds))
    with tempfile.TemporaryDirectory() as tmp:
        ev = BatchedEvaluator(env, controller(env), seeds, tmp + '/')
        means = ev.run()
        queue = [row['avg_queue'] for row in ev.traffic_data]
    print('    %-4s %-11s %d seeds x %d lock-steps: mean global reward per lock-step %.3f (per-seed min %.3f, max %.3f), '
          'mean avg_queue %.4f' % (scenario, agent, len(seeds), env.T, float(np.mean(means)), min(means), max(means),
                                   float(np.mean(queue))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seeds', type=int, default=50)
    ap.add_argument('--step', default=None, help='run this step in this process (the parent starts one child per step)')
    args = ap.parse_args()
    if args.step is not None:
        import torch
        assert torch.cuda.is_available(), 'needs the MI355X'
        if args.step == 'launch':
            launch()
        else:
            _, scenario, agent = args.step.split(':')
            evaluate(scenario, agent, args.seeds)
        return 0
    print('max-pressure next to greedy (tools/maxpressure_profile.py --seeds %d)' % args.seeds)
    for step, limit in STEPS:
        if step.startswith('evaluate:grid:maxpressure'):
            print('`evaluate --batched` at full episode length, default evaluation seeds:')
        sys.stdout.flush()
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--seeds', str(args.seeds), '--step', step],
                                timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print('step %s ended with status %d: stopping here' % (step, rc))
            return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())

"""Same-box A/B of the lock-step's LSTM product arithmetic, fp32 against the opt-in bf16x3 (MODEL_CONFIG lstm_precision): for
BASELINE configs[1] (IA2C-FP catch-up, 8 x 4096) and IA2C on CACC catch-up, per precision
  - the rollout graph alone (one n_step batch of lock-steps, replayed), median of `reps` replays;
  - the lock-step by graph difference: (rollout graph) / n_step -- the same graph with only the step kernel's precision changed,
    so the difference of the two per-lock-step times is the step kernel's;
  - the whole batch (rollout graph + captured update + epilogue: BatchedTrainer.run_batch), median ms and env-steps/s.
The two precisions alternate (A B A B ...) so that clock drift hits both.  python tools/precision_ab.py [E=4096] [reps=30]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def build(agent, E, precision, n_step=60):
    from helpers import cacc_config
    from deeprl_network_amd.envs import make_batch_env
    from deeprl_network_amd.main import init_agent
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    cp = cacc_config(agent=agent, scenario='catchup', n_step=n_step, reward_norm=800.0)
    cp['MODEL_CONFIG']['lstm_precision'] = precision
    env = make_batch_env(cp['ENV_CONFIG'], num_envs=E)
    np.random.seed(12)
    model = init_agent(env, cp['MODEL_CONFIG'], 10 ** 9, 12, num_envs=E)
    return BatchedTrainer(env, model, Counter(10 ** 12, 10 ** 12, 10 ** 12), use_graph=True)


def timed(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def main():
    E = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    n_step = 60
    print('precision A/B on %s, E = %d, n_step = %d, %d reps per point (medians; alternating A/B rounds)'
          % (torch.cuda.get_device_name(0), E, n_step, reps))
    for agent in ('ia2c_fp', 'ia2c'):
        trs = {p: build(agent, E, p, n_step) for p in ('fp32', 'bf16x3')}
        for tr in trs.values():
            for _ in range(3):
                tr.run_batch()
        torch.cuda.synchronize()
        roll = {p: [] for p in trs}
        batch = {p: [] for p in trs}
        for _ in range(3):
            for p, tr in trs.items():
                roll[p] += timed(tr.graph.replay, reps // 3)
                batch[p] += timed(tr.run_batch, reps // 3)
        med = {p: (float(np.median(roll[p])), float(np.median(batch[p]))) for p in trs}
        r32, r3 = med['fp32'][0], med['bf16x3'][0]
        print('\n%s catch-up (lock-step kernel: %s)' % (agent, 'lstm_step_x_kernel<3,0,1>' if agent == 'ia2c_fp' else 'lstm_step_x_kernel<3,0,2>'))
        for p in trs:
            rg, bt = med[p]
            print('  %-7s rollout graph %8.3f ms (%6.2f us / lock-step)   whole batch %8.3f ms  %7.1f M env-steps/s'
                  % (p, rg, rg * 1e3 / n_step, bt, trs[p].model.n_agent * E * n_step / (bt * 1e-3) / 1e6))
        print('  lock-step by graph difference: %.2f us saved per lock-step (rollout graph %.1f %% shorter); whole batch %.1f %% shorter'
              % ((r32 - r3) * 1e3 / n_step, 100 * (1 - r3 / r32), 100 * (1 - med['bf16x3'][1] / med['fp32'][1])))
        del trs
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

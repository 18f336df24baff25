"""The traffic recorder's launch (nmarl_atsc_traffic_step, csrc/traffic.hip) next to the env step launch it follows, on both ATSC
scenarios at E = 64 and 1024: median of 200 launches, each between its own pair of events, after a warm-up.  The env step kernels
are the parent's (the record reads their state and edits neither).  Prints one line per scenario and size."""
import configparser
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from deeprl_network_amd.envs import make_batch_env
from deeprl_network_amd.envs.traffic_record import TrafficRecorder

N_LAUNCH, WARM = 200, 20


def median_us(fn):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(N_LAUNCH)]
    for k, (a, b) in enumerate(ev):
        a.record()
        fn(k)
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) * 1e3 for a, b in ev]))


for ini, label in (('config_ma2c_cnet_grid.ini', 'grid (25 x 6 slots)'), ('config_ma2c_nc_net.ini', 'network (28 x 22 slots)')):
    cp = configparser.ConfigParser()
    cp.read(os.path.join(ROOT, 'config', ini))
    for E in (64, 1024):
        env = make_batch_env(cp['ENV_CONFIG'], num_envs=E)
        env.reset()
        rec = TrafficRecorder(env, 8)
        rec.begin()
        e = torch.arange(E, device='cuda')[:, None]
        a = torch.arange(env.n_agent, device='cuda')[None, :]
        n_a = torch.tensor(env.n_a_ls, device='cuda')[None, :]
        acts = [((e + 3 * a + s) % n_a).to(torch.uint8).contiguous() for s in range(4)]
        for s in range(WARM):
            env.step(acts[s % 4])
            rec.step(s % 8)
        torch.cuda.synchronize()
        t_env = median_us(lambda k: env.step(acts[k % 4]))
        t_rec = median_us(lambda k: rec.step(k % 8))
        nbytes = 20 * rec.N * rec.S + 120
        print('%-24s E = %5d: recorder %6.2f us per launch, env step %6.2f us per launch, recorder / step = %.3f; '
              '%d B per replica -> %.3f TB/s algorithmic' % (label, E, t_rec, t_env, t_rec / t_env, nbytes, E * nbytes / t_rec / 1e6))
        del env, rec

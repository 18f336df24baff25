"""Time nmarl_net_step (hipGraph of 20 launches) at several E; NMARL_NET_REPS picks replicas per block.
  python tools/time_net.py [E ...]                              the `queue` step (default E = 1024 8192 65536)
  python tools/time_net.py --objectives [E ...]                 `queue`, `wait`, `hybrid` of this tree side by side
  python tools/time_net.py --ab tools/dbg/libnmarl_prev.so [E ...]
      same-box A/B of the `queue` step: this tree's library against another build's nmarl_net_step (tools/ab_build.sh <rev>;
      only that one symbol is taken from it and the other build sees the leading fields of nmarl_net_params_t alone, so an older
      C-ABI will do), the two alternating --rounds times on the same state tensors; prints the median ratio."""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np, torch
from helpers import net_config
from deeprl_network_amd import _lib
from deeprl_network_amd.envs.real_net_env import RealNetBatchEnv


class _StepFrom:
    """_lib.lib with nmarl_net_step taken from another library."""
    def __init__(self, base, other):
        self._base, self._step = base, other.nmarl_net_step
        self._step.argtypes, self._step.restype = _lib.SIGNATURES['nmarl_net_step'], ctypes.c_int

    def __getattr__(self, k):
        return self._step if k == 'nmarl_net_step' else getattr(self._base, k)


def make(E, objective='queue'):
    cp = net_config()
    cp['ENV_CONFIG']['objective'] = objective
    cp['ENV_CONFIG']['coef_wait'] = '0.2'
    env = RealNetBatchEnv(cp['ENV_CONFIG'], num_envs=E)
    env.reset()
    return env


def actions(env):
    tp, rng = env.topo, np.random.RandomState(0)
    return [torch.from_numpy(np.stack([rng.randint(0, tp.n_a_ls[i], size=env.E) for i in range(tp.N)], 1).astype(np.uint8)).cuda()
            for _ in range(4)]


def capture(env, acts):
    """-> a hipGraph of 20 steps, warmed up (40 eager steps, one replay)."""
    for k in range(40): env.step(acts[k % 4], auto_reset=True)
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s): env.step(acts[0], auto_reset=True)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for k in range(20): env.step(acts[k % 4], auto_reset=True)
    g.replay(); torch.cuda.synchronize()
    return g


def time_us(g, replays=5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays): g.replay()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (20 * replays)


def kb(env):
    """Algorithmic KB per replica-step: the state arrays in and out, actions, the slab (csrc/realnet.hip header)."""
    return 16.652 + (2 * 4 * sum(env.topo.n_s_ls) / 1e3 if env.head_wait is not None else 0.0)


def main():
    argv = sys.argv[1:]
    ab = argv[argv.index('--ab') + 1] if '--ab' in argv else None
    rounds = int(argv[argv.index('--rounds') + 1]) if '--rounds' in argv else 15
    skip = {argv.index(f) + 1 for f in ('--ab', '--rounds') if f in argv}
    sizes = [int(x) for i, x in enumerate(argv) if not x.startswith('--') and i not in skip] or [1024, 8192, 65536]
    reps = os.environ.get('NMARL_NET_REPS', 'auto')
    for E in sizes:
        if ab:
            env = make(E)
            acts = actions(env)
            mine = _lib.lib
            theirs = _StepFrom(mine, ctypes.CDLL(os.path.abspath(ab)))
            graphs = {}
            for tag, lib in (('tree', mine), ('other', theirs)):
                _lib.lib = lib
                try:
                    graphs[tag] = capture(env, acts)
                finally:
                    _lib.lib = mine
            t = {'tree': [], 'other': []}
            for r in range(rounds):                      # alternating, the order swapped every round
                for tag in (('tree', 'other') if r % 2 == 0 else ('other', 'tree')):
                    t[tag].append(time_us(graphs[tag]))
            med = {k: float(np.median(v)) for k, v in t.items()}
            ratios = np.array(t['tree']) / np.array(t['other'])
            print('A/B queue reps=%s E=%d: tree %.1f us, other %.1f us per launch (medians of %d alternating rounds); '
                  'tree / other = %.4f (median of the per-round ratios %.4f, min %.4f, max %.4f)'
                  % (reps, E, med['tree'], med['other'], rounds, med['tree'] / med['other'], float(np.median(ratios)),
                     ratios.min(), ratios.max()))
            del graphs, env
        else:
            base = None
            for objective in (('queue', 'wait', 'hybrid') if '--objectives' in argv else ('queue',)):
                env = make(E, objective)
                g = capture(env, actions(env))
                us = float(np.median([time_us(g) for _ in range(5)]))
                base = us if base is None else base
                print('%s reps=%s E=%d: %.1f us per launch, %.2f TB/s algorithmic (%.1f KB/replica)%s'
                      % (objective, reps, E, us, kb(env) * 1e3 * E / us / 1e6, kb(env),
                         '' if objective == 'queue' else ', %.3f x the queue step' % (us / base)))
                del g, env
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

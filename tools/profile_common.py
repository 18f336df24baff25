"""What the tools/*_profile.py scripts share: the compiler's resource lines of csrc/a2c.hip, a captured BatchedTrainer of
config_ia2c_fp_catchup.ini with some MODEL_CONFIG keys set, the alternating timing of several such trainers, and the bench.py A/B
against a built checkout of the parent commit.  Each script keeps its own `measure` and the wording of its report."""
import configparser
import gc
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tools'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def resources(width, names=None, prefixes=(), title='compiler resource report, gfx950:'):
    """Print the register / scratch / LDS / occupancy line of the kernels of a2c.hip called `names` (in that order) or, without names,
    of those whose name starts with one of `prefixes` (in the file's order).  -> {kernel name: the compiler's figures}."""
    import resource_usage
    rows = {r['name']: r for r in resource_usage.usage(os.path.join(ROOT, 'deeprl_network_amd', 'csrc', 'a2c.hip'))}
    print(title)
    if names is None:
        names = [n for n in rows if n.startswith(tuple(prefixes))]
    for k in names:
        r = rows[k]
        print('    %-*s VGPRs %3d, AGPRs %d, SGPRs %3d, scratch %d bytes/lane, LDS %d bytes/block, occupancy %d waves/SIMD'
              % (width, k, r['VGPRs'], r.get('AGPRs', 0), r['TotalSGPRs'], r['ScratchSize [bytes/lane]'], r['LDS Size [bytes/block]'],
                 r['Occupancy [waves/SIMD]']))
    return rows


def trainer(keys, E):
    """-> (env, model, captured BatchedTrainer) of config_ia2c_fp_catchup.ini at E replicas with the MODEL_CONFIG `keys` set."""
    import numpy as np
    from deeprl_network_amd.envs import make_batch_env
    from deeprl_network_amd.main import init_agent
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    cp = configparser.ConfigParser()
    cp.read(os.path.join(ROOT, 'config', 'config_ia2c_fp_catchup.ini'))
    for k, v in keys.items():
        cp['MODEL_CONFIG'][k] = str(v)
    env = make_batch_env(cp['ENV_CONFIG'], num_envs=E)
    np.random.seed(env.seed)
    model = init_agent(env, cp['MODEL_CONFIG'], int(1e9), env.seed, num_envs=E)
    return env, model, BatchedTrainer(env, model, Counter(int(1e18), int(1e18), int(1e18)), use_graph=True)


PER_BLOCK = 20          # batches per timed block of `training_ab`


def training_ab(order, E=4096, per_block=PER_BLOCK, blocks=8):
    """order: {arm name: MODEL_CONFIG keys}.  The arms' trainers are built and warmed in that order, then timed in blocks of per_block
    batches, alternating.  -> ({name: (env, model, trainer)}, {name: [ms per batch of every block]}); `close_arms` when done."""
    import torch
    arms = {name: trainer(keys, E) for name, keys in order.items()}
    for _, _, tr in arms.values():
        for _ in range(5):
            tr.run_batch()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(blocks):
        for k, (_, _, tr) in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(per_block):
                tr.run_batch()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / per_block * 1e3)
    return arms, ms


def report_arms(ms, width):
    """Print every arm's line; -> {name: median ms per batch}."""
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, v in ms.items():
        print('    %-*s median %7.3f ms per batch (min %7.3f, max %7.3f; spread of the blocks %.2f %%)'
              % (width, k, med[k], min(v), max(v), (max(v) - min(v)) / med[k] * 100))
    return med


def close_arms(arms, captured_update=False):
    """Every arm trained on finite weights without a fallback (captured_update: and its update was captured); then free the trainers."""
    import torch
    for k, (_, model, tr) in arms.items():
        assert torch.isfinite(model.policy.params.flat).all() and tr.handoff_fallbacks == 0, k
        assert not captured_update or tr.update_capture_error is None, k
    arms.clear()
    gc.collect()
    torch.cuda.empty_cache()


def bench_ab(parent, runs=4):
    """`bench.py --gpus 1 --steps 20 --warmup 3` of the built checkout `parent` and of this tree, each run a fresh child process,
    alternating."""
    trees = {'parent': os.path.abspath(parent), 'this tree': ROOT}
    ms = {k: [] for k in trees}
    for _ in range(runs):
        for k, d in trees.items():
            out = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', '20', '--warmup', '3'], cwd=d, check=True,
                                 stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300).stdout.decode()
            ms[k].append(json.loads([l for l in out.splitlines() if l.startswith('{')][-1])['ms_per_step'])
            print('bench.py of %s: %.3f ms per batch' % (k, ms[k][-1]), file=sys.stderr, flush=True)
    print('bench.py --gpus 1 --steps 20 --warmup 3 (key absent), the parent commit\'s tree and this one, %d runs each, alternating:' % runs)
    for k in trees:
        print('    %-10s ms per batch: %s; median %.3f' % (k, ', '.join('%.3f' % v for v in ms[k]), statistics.median(ms[k])))
    r = statistics.median(ms['this tree']) / statistics.median(ms['parent'])
    print('    this tree / parent: %.4f (%+.2f %%; the documented run-to-run spread of the batch time is +-1.5 %%)' % (r, (r - 1) * 100))


def parent_tree_arg():
    """The scripts' one option."""
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-tree', default=None, help='a built checkout of the parent commit: adds the bench.py A/B against it')
    return ap.parse_args().parent_tree

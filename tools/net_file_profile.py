"""Measurements of the network-from-a-file feature (profiles/r29_net_file.txt).
  python tools/net_file_profile.py --resources [REV]     no GPU: registers / scratch / LDS of every net_step_kernel instantiation of
                                                         this tree as compiled for gfx950, next to revision REV's (default HEAD~1)
  python tools/net_file_profile.py --time [E ...]        one nmarl_net_step_dem launch next to one nmarl_net_step launch on Monaco
                                                         (the built-in network / config/networks/monaco.json), each between two
                                                         events, alternating, `--rounds` times (default 200); default E = 64 1024 131072
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

REALNET = 'deeprl_network_amd/csrc/realnet.hip'
COLS = (('SGPR', 'TotalSGPRs'), ('VGPR', 'VGPRs'), ('AGPR', 'AGPRs'), ('scratch B/lane', 'ScratchSize [bytes/lane]'),
        ('SGPR spill', 'SGPRs Spill'), ('VGPR spill', 'VGPRs Spill'), ('LDS B', 'LDS Size [bytes/block]'), ('waves/SIMD', 'Occupancy [waves/SIMD]'))


def _rows(src):
    import resource_usage
    return {r['name']: r for r in resource_usage.usage(src) if r['name'].startswith('net_step_kernel')}


def resources(rev):
    """The tree's instantiations and revision `rev`'s, whose sources are extracted with `git show` into a scratch directory of
    the same layout (csrc/common.h includes ../../include/nmarl.h)."""
    mine = _rows(os.path.join(ROOT, REALNET))
    with tempfile.TemporaryDirectory() as d:
        for f in (REALNET, 'deeprl_network_amd/csrc/common.h', 'include/nmarl.h'):
            os.makedirs(os.path.dirname(os.path.join(d, f)), exist_ok=True)
            with open(os.path.join(d, f), 'wb') as out:
                out.write(subprocess.run(['git', 'show', '%s:%s' % (rev, f)], cwd=ROOT, capture_output=True, check=True).stdout)
        theirs = _rows(os.path.join(d, REALNET))
    print('net_step_kernel<REPS, WAIT, DEM> of this tree / net_step_kernel<REPS, WAIT> of %s, gfx950 (hipcc -O3 -ffp-contract=off,' % rev)
    print('-Rpass-analysis=kernel-resource-usage)')
    print('%-42s ' % 'kernel' + ' '.join('%14s' % c for c, _ in COLS))
    same = True
    for name in sorted(theirs):
        print('%-42s ' % (name + '  [' + rev + ']') + ' '.join('%14d' % theirs[name][k] for _, k in COLS))
        for dem in ('false', 'true'):
            cur = mine[name[:-1] + ', ' + dem + '>']
            print('%-42s ' % cur['name'] + ' '.join('%14d' % cur[k] for _, k in COLS))
            if dem == 'false':
                same = same and all(cur[k] == theirs[name][k] for _, k in COLS)
            else:
                for _, k in (COLS[3], COLS[6]):
                    assert cur[k] <= theirs[name][k], 'a DEM form adds %s' % k
    print('DEM = false: every figure equals %s\'s: %s' % (rev, 'yes' if same else 'NO'))
    print('DEM = true: no LDS and no scratch added (asserted above); replicas per block unchanged (2 / 4 / 8)')
    return same


def time_launches(sizes, rounds):
    import numpy as np
    import torch
    from helpers import net_config
    from deeprl_network_amd.envs.real_net_env import RealNetBatchEnv
    for E in sizes:
        envs, acts = {}, None
        for tag, path in (('nmarl_net_step', None), ('nmarl_net_step_dem', os.path.join(ROOT, 'config', 'networks', 'monaco.json'))):
            cp = net_config()
            if path:
                cp['ENV_CONFIG']['net_file'] = path
            env = envs[tag] = RealNetBatchEnv(cp['ENV_CONFIG'], num_envs=E)
            env.reset()
            if acts is None:
                tp, rng = env.topo, np.random.RandomState(0)
                acts = [torch.from_numpy(np.stack([rng.randint(0, tp.n_a_ls[i], size=E) for i in range(tp.N)], 1).astype(np.uint8)).cuda()
                        for _ in range(4)]
            for k in range(40):                                  # warm-up: the queues fill, the code objects are loaded
                env.step(acts[k % 4], auto_reset=True)
        torch.cuda.synchronize()
        t = {tag: [] for tag in envs}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for r in range(rounds):                                  # alternating, the order swapped every round
            for tag in (list(envs) if r % 2 == 0 else list(envs)[::-1]):
                e0.record()
                envs[tag].step(acts[r % 4], auto_reset=True)
                e1.record()
                e1.synchronize()
                t[tag].append(e0.elapsed_time(e1) * 1e3)
        med = {tag: float(np.median(v)) for tag, v in t.items()}
        ratios = np.array(t['nmarl_net_step_dem']) / np.array(t['nmarl_net_step'])
        print('E=%d: nmarl_net_step %.2f us, nmarl_net_step_dem %.2f us per launch (medians of %d alternating launches, each between '
              'two events); dem / plain = %.4f (median of the per-round ratios %.4f, quartiles %.4f .. %.4f)'
              % (E, med['nmarl_net_step'], med['nmarl_net_step_dem'], rounds, med['nmarl_net_step_dem'] / med['nmarl_net_step'],
                 float(np.median(ratios)), float(np.percentile(ratios, 25)), float(np.percentile(ratios, 75))), flush=True)
        del envs
        torch.cuda.empty_cache()


def main():
    argv = sys.argv[1:]
    if '--resources' in argv:
        rest = [a for a in argv if not a.startswith('--')]
        raise SystemExit(0 if resources(rest[0] if rest else 'HEAD~1') else 1)
    rounds = int(argv[argv.index('--rounds') + 1]) if '--rounds' in argv else 200
    skip = {argv.index('--rounds') + 1} if '--rounds' in argv else set()
    sizes = [int(x) for i, x in enumerate(argv) if not x.startswith('--') and i not in skip] or [64, 1024, 1 << 17]
    time_launches(sizes, rounds)


if __name__ == '__main__':
    main()

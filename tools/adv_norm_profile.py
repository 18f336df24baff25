"""First measurement of the opt-in advantage standardisation, one box, one process:
    python tools/adv_norm_profile.py > profiles/r20_adv_norm.txt

(1) ops.standardize (standardize_moments_kernel + standardize_apply_kernel) next to ops.nstep_return, the return scan it follows in the
update, on the same [N, T, E] advantage buffer at the two update shapes -- N = 8, E = 4096, T = 60 (groups of 245 760 rows) and
N = 25, E = 1024, T = 120 (groups of 122 880 rows) -- in `agent` mode (G = N) and pooled in `all` mode (G = 1, rows = N T E):
  single   one eager call between two events, the two ops alternating, 300 pairs: median and minimum.  An eager call between two
           events carries the launches' own floor; the yardstick is nstep_return measured the same way, not a fixed time.
  block    100 calls back to back between two events, the two ops alternating block by block, 10 blocks each: median per call.
The data (7.9 and 12.3 MB, read twice and written once) fit the last-level cache: times only, no share of the HBM bandwidth.  Each
shape's first call is held to the bound of tests/adv_norm_checks.py before anything is timed.
(2) config_ia2c_fp_catchup.ini at 8 x 4096 through BatchedTrainer (captured), without the key -- the code path of before -- and with
adv_norm = agent, two trainers in one process, blocks of 20 batches alternating, 8 blocks each: median ms per batch, to be read
against the +-1.5 % run-to-run spread of the batch time.  Done twice with fresh trainers, built and timed in either order, so
that an effect of the order on a trainer's batch time shows next to the effect of the key.
(3) with --parent-tree DIR (a built checkout of the parent commit; tools/ab_build.sh does not serve here, the C-ABI grew): `bench.py
--gpus 1 --steps 20 --warmup 3` of that tree and of this one, each run a fresh child process, alternating, 4 runs each: the key is
absent in bench.py, so this is the parent's batch time against this tree's on one box.
The kernels' registers, LDS, scratch and occupancy are the compiler's resource report for gfx950 (tools/resource_usage.py)."""
import contextlib
import io
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import profile_common as common  # noqa: E402  (puts the repository, tools/ and tests/ on sys.path)

SHAPES = [(8, 4096, 60), (25, 1024, 120)]
GAMMA, EPS = 0.99, 1e-8


def measure(N, E, T, mode):
    import torch
    import adv_norm_checks as ac
    from deeprl_network_amd import ops
    gen = torch.Generator().manual_seed(N * 10007 + E * 101 + T)
    r = torch.randn(T, E, generator=gen).cuda()
    v = torch.randn(T, N, E, generator=gen).cuda()
    done = (torch.rand(T, E, generator=gen) < 0.02).to(torch.uint8).cuda()
    R_end = torch.randn(N, E, generator=gen).cuda()
    R, Adv, Adv_n = (torch.zeros(N, T, E, device='cuda') for _ in range(3))
    G = N if mode == 'agent' else 1
    rows = N * T * E // G
    C = ops.standardize_chunks(rows, G)
    partial = torch.zeros(G, C, 3, dtype=torch.float64, device='cuda')
    moments = torch.zeros(G, 2, dtype=torch.float64, device='cuda')
    run = {'nstep_return': lambda: ops.nstep_return(r, v, done, R_end, GAMMA, -1.0, None, R, Adv),
           'standardize': lambda: ops.standardize(Adv.view(G, rows), EPS, out=Adv_n.view(G, rows), partial=partial, moments=moments)}
    for f in run.values():
        f()
    torch.cuda.synchronize()
    # the timed call is the call the tests pin (a timing of a kernel that computes something else is worthless)
    with contextlib.redirect_stdout(io.StringIO()):
        worst = ac.assert_standardized(Adv_n.view(G, rows), moments, Adv.view(G, rows), EPS, 'the timed call')
    for _ in range(30):
        for f in run.values():
            f()
    torch.cuda.synchronize()
    single = {k: [] for k in run}
    for _ in range(300):
        for k, f in run.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            single[k].append(a.elapsed_time(b) * 1e3)
    block, reps = {k: [] for k in run}, 100
    for _ in range(10):
        for k, f in run.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                f()
            b.record()
            b.synchronize()
            block[k].append(a.elapsed_time(b) * 1e3 / reps)
    print('N = %d, E = %d, T = %d, adv_norm = %s: G = %d groups of %d rows, %d chunks of %d rows per group (%d blocks per launch), '
          '%.1f MB of advantages; the timed call uses %.2g of the bound:'
          % (N, E, T, mode, G, rows, C, -(-rows // C), G * C, 4 * N * T * E / 1e6, worst))
    med = {}
    for k in run:
        med[k] = (statistics.median(single[k]), statistics.median(block[k]))
        print('    %-13s single call: median %7.2f us, min %7.2f us;  back to back: median %7.2f us per call (min %7.2f, max %7.2f)'
              % (k, med[k][0], min(single[k]), med[k][1], min(block[k]), max(block[k])))
    print('    standardize / nstep_return: %.2f (single call), %.2f (back to back)'
          % tuple(med['standardize'][i] / med['nstep_return'][i] for i in (0, 1)))


def training_ab(first):
    keys = {'key absent': {}, 'adv_norm = agent': dict(adv_norm='agent')}
    arms, ms = common.training_ab({k: keys[k] for k in sorted(keys, key=lambda k: k != first)})      # `first` is built and timed first
    env, model, _ = arms['key absent']
    print('config_ia2c_fp_catchup.ini, %d agents x %d replicas, n_step %d, captured, %d blocks of %d batches per arm, alternating, '
          '"%s" built and timed first:' % (env.n_agent, model.E, model.n_step, len(ms[first]), common.PER_BLOCK, first))
    med = common.report_arms(ms, 17)
    print('    adv_norm = agent / key absent: %.4f (%+.2f %%; the documented run-to-run spread of the batch time is +-1.5 %%)'
          % (med['adv_norm = agent'] / med['key absent'], (med['adv_norm = agent'] / med['key absent'] - 1) * 100))
    del env, model
    common.close_arms(arms)


def main():
    parent = common.parent_tree_arg()
    import torch
    assert torch.cuda.is_available(), 'needs the MI355X'
    print('advantage standardisation next to the n-step return scan (tools/adv_norm_profile.py), %s' % torch.cuda.get_device_name(0))
    common.resources(27, names=('nstep_kernel', 'standardize_moments_kernel', 'standardize_apply_kernel'))
    for N, E, T in SHAPES:
        for mode in ('agent', 'all'):
            measure(N, E, T, mode)
    for first in ('key absent', 'adv_norm = agent'):      # two fresh pairs of trainers, built in either order
        training_ab(first)
    if parent:
        common.bench_ab(parent)
    return 0


if __name__ == '__main__':
    sys.exit(main())

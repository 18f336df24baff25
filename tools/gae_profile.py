"""First measurement of the opt-in GAE(lambda) return scan next to the n-step scan it stands beside, one box, one process:
    python tools/gae_profile.py > profiles/r18_gae.txt

ops.gae_return (gae_kernel, lambda = 0.95) and ops.nstep_return (nstep_kernel) on the same inputs at the two update shapes
(N = 8, E = 4096, T = 60 and N = 25, E = 1024, T = 120), on the global path and on the spatial path at alpha = 0.9 (line distances).
  single   one launch between two events, the two ops alternating, 300 pairs: median and minimum.  An eager launch between two
           events carries the launch's own floor; the yardstick is nstep_return measured the same way, not a fixed time.
  block    100 launches back to back between two events, the two ops alternating block by block, 10 blocks each: median per launch.
The bytes moved are the same; the dependent chain has two multiply-adds per step instead of one.  The kernels' registers, LDS,
scratch and occupancy are the compiler's resource report for gfx950 (tools/resource_usage.py), printed first."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import profile_common as common  # noqa: E402  (puts the repository, tools/ and tests/ on sys.path)

SHAPES = [(8, 4096, 60), (25, 1024, 120)]
GAMMA, LAMBDA = 0.99, 0.95


def bytes_moved(N, E, T, spatial):
    """Bytes the threads of either scan request per launch (one thread per (agent, replica), per step: done u8, r -- N floats on the
    spatial path --, v, R, Adv).  The agents' threads of a replica read the same done / r lines: HBM sees fewer."""
    per_thread_step = 1 + 4 * (N if spatial else 1) + 3 * 4
    return N * E * T * per_thread_step


def measure(N, E, T, alpha):
    import torch
    from deeprl_network_amd import ops
    gen = torch.Generator().manual_seed(N * 10007 + E * 101 + T)
    spatial = alpha >= 0
    r = torch.randn((T, E, N) if spatial else (T, E), generator=gen).cuda()
    v = torch.randn(T, N, E, generator=gen).cuda()
    done = (torch.rand(T, E, generator=gen) < 0.02).to(torch.uint8).cuda()
    R_end = torch.randn(N, E, generator=gen).cuda()
    idx = torch.arange(N)
    dist = (idx[:, None] - idx[None, :]).abs().to(torch.int32).cuda()
    out = [torch.zeros(N, T, E, device='cuda') for _ in range(4)]
    run = {'nstep_return': lambda: ops.nstep_return(r, v, done, R_end, GAMMA, alpha, dist, out[0], out[1]),
           'gae_return': lambda: ops.gae_return(r, v, done, R_end, GAMMA, LAMBDA, alpha, dist, out[2], out[3])}
    for _ in range(30):
        for f in run.values():
            f()
    torch.cuda.synchronize()
    # lambda = 1 on these inputs is the n-step scan (a timing of a kernel that computes something else is worthless)
    ops.gae_return(r, v, done, R_end, GAMMA, 1.0, alpha, dist, out[2], out[3])
    torch.cuda.synchronize()
    scale = float(out[0].abs().max())
    assert float((out[2] - out[0]).abs().max()) <= 4e-7 * scale and float((out[3] - out[1]).abs().max()) <= 4e-7 * scale
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
    print('N = %d, E = %d, T = %d, %s (%.1f MB issued per launch):'
          % (N, E, T, 'spatial alpha = %g' % alpha if spatial else 'global reward', bytes_moved(N, E, T, spatial) / 1e6))
    med = {}
    for k in run:
        med[k] = (statistics.median(single[k]), statistics.median(block[k]))
        print('    %-13s single launch: median %7.2f us, min %7.2f us;  back to back: median %7.2f us per launch (min %7.2f, max %7.2f)'
              % (k, med[k][0], min(single[k]), med[k][1], min(block[k]), max(block[k])))
    ratios = tuple(med['gae_return'][i] / med['nstep_return'][i] for i in (0, 1))
    print('    gae_return / nstep_return: %.2f (single launch), %.2f (back to back)' % ratios)
    return ratios


def main():
    import torch
    assert torch.cuda.is_available(), 'needs the MI355X'
    print('GAE(lambda) return scan next to the n-step scan (tools/gae_profile.py), %s' % torch.cuda.get_device_name(0))
    common.resources(17, names=('nstep_kernel', 'gae_kernel<false>', 'gae_kernel<true>'))
    worst = 0.0
    for N, E, T in SHAPES:
        for alpha in (-1.0, 0.9):
            worst = max(worst, *measure(N, E, T, alpha))
    print('largest ratio: %.2f' % worst)
    return 0


if __name__ == '__main__':
    sys.exit(main())

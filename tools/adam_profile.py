"""First measurement of the opt-in clip + Adam optimiser step next to the clip + RMSProp step it stands beside, one box, one process:
    python tools/adam_profile.py > profiles/r19_adam.txt

ops.adam_clip (adam_sumsq_kernel + adam_kernel) and ops.rmsprop_tf_clip (sumsq_kernel + rmsprop_kernel) on the same flat buffers at
the two update shapes: the headline's (G = 8 optimisers x P = 409 568 / 8 parameters) and the grid CommNet's (G = 1, P = 1 021 990).
  single   one eager call (two launches) between two events, the two ops alternating, 300 pairs: median and minimum.  An eager call
           between two events carries the launches' own floor; the yardstick is rmsprop_tf_clip measured the same way, not a fixed time.
  block    100 calls back to back between two events, the two ops alternating block by block, 10 blocks each: median per call.
Adam moves 28 bytes per parameter (g; w, m, v read and written -- the second launch's read of g counted as cached), RMSProp 20.
The kernels' registers, LDS, scratch and occupancy are the compiler's resource report for gfx950 (tools/resource_usage.py), printed
first; each shape's first call is held to the bounds of tests/adam_checks.py before anything is timed."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import profile_common as common  # noqa: E402  (puts the repository, tools/ and tests/ on sys.path)

SHAPES = [(8, 409568 // 8), (1, 1021990)]
LR, MAX_NORM = 5e-4, 40.0


def measure(G, P):
    import torch
    from deeprl_network_amd import ops
    gen = torch.Generator().manual_seed(G * 1009 + P)
    w0 = torch.randn(G, P, generator=gen).cuda()
    g = (torch.randn(G, P, generator=gen) * 0.05).cuda()
    scratch, norm = torch.zeros(G, 64, device='cuda'), torch.zeros(G, device='cuda')
    a = dict(w=w0.clone(), m=torch.zeros_like(w0), v=torch.zeros_like(w0), t=torch.zeros(1, dtype=torch.int32, device='cuda'))
    r = dict(w=w0.clone(), ms=torch.ones_like(w0))
    # the timed step is the step the tests pin (a timing of a kernel that computes something else is worthless): one call, checked
    import adam_checks as ac
    prev = (a['w'].clone(), a['m'].clone(), a['v'].clone())
    ops.adam_clip(a['w'], g, a['m'], a['v'], scratch, a['t'], LR, 0.9, 0.999, 1e-8, MAX_NORM, 1.0, norm)
    f32 = ac._f32
    ac.assert_adam_step(prev, g, 0, (a['w'], a['m'], a['v'], norm), f32(LR), f32(0.9), f32(0.999), f32(1e-8), f32(MAX_NORM), 1.0,
                        'G=%d P=%d, the timed call' % (G, P))
    run = {'rmsprop_tf_clip': lambda: ops.rmsprop_tf_clip(r['w'], g, r['ms'], scratch, LR, 0.99, 1e-5, MAX_NORM, 1.0, norm),
           'adam_clip': lambda: ops.adam_clip(a['w'], g, a['m'], a['v'], scratch, a['t'], LR, 0.9, 0.999, 1e-8, MAX_NORM, 1.0, norm)}
    for _ in range(30):
        for f in run.values():
            f()
    torch.cuda.synchronize()
    single = {k: [] for k in run}
    for _ in range(300):
        for k, f in run.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            single[k].append(e0.elapsed_time(e1) * 1e3)
    block, reps = {k: [] for k in run}, 100
    for _ in range(10):
        for k, f in run.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            e1.synchronize()
            block[k].append(e0.elapsed_time(e1) * 1e3 / reps)
    assert torch.isfinite(a['w']).all() and torch.isfinite(r['w']).all()
    print('G = %d, P = %d (%d parameters; Adam moves %.1f MB per call, RMSProp %.1f MB):' % (G, P, G * P, 28 * G * P / 1e6, 20 * G * P / 1e6))
    med = {}
    for k in run:
        med[k] = (statistics.median(single[k]), statistics.median(block[k]))
        print('    %-16s single call: median %7.2f us, min %7.2f us;  back to back: median %7.2f us per call (min %7.2f, max %7.2f)'
              % (k, med[k][0], min(single[k]), med[k][1], min(block[k]), max(block[k])))
    ratios = tuple(med['adam_clip'][i] / med['rmsprop_tf_clip'][i] for i in (0, 1))
    print('    adam_clip / rmsprop_tf_clip: %.2f (single call), %.2f (back to back)' % ratios)
    return ratios


def main():
    import torch
    assert torch.cuda.is_available(), 'needs the MI355X'
    print('clip + Adam step next to the clip + RMSProp step (tools/adam_profile.py), %s' % torch.cuda.get_device_name(0))
    common.resources(17, names=('sumsq_kernel', 'rmsprop_kernel', 'adam_sumsq_kernel', 'adam_kernel'))
    worst = 0.0
    for G, P in SHAPES:
        worst = max(worst, *measure(G, P))
    print('largest ratio: %.2f' % worst)
    return 0


if __name__ == '__main__':
    sys.exit(main())

"""First measurement of the opt-in replica minibatches of the PPO epochs (MODEL_CONFIG ppo_minibatches), one box, one process:
    python tools/ppo_minibatch_profile.py [--parent-tree DIR] > profiles/r28_ppo_minibatch.txt

  (a) one ops.minibatch_gather call for the operand list of one step (buf_x, buf_fp, buf_act, buf_done_pre, the policy advantage, R,
      ppo_logp_old, ppo_v_old, h_bw, c_bw) at 8 agents x 4096 replicas x 60 steps and 25 x 1024 x 120 for M = 2 and 8, between two
      events, 200 calls: median and minimum, next to the bytes it moves (read + written) and the rate that is;
  (b) the two launches of ops.minibatch_perm at E = 1024 and 4096, the same way;
  (c) config_ia2c_fp_catchup.ini at 8 x 4096 with ppo_epochs = 2: ms per batch with ppo_minibatches absent, 1, 2, 4 and 8, the arms
      alternating in blocks (tools/profile_common.py);
  (d) with --parent-tree: bench.py (key absent) of a built checkout of the parent commit against this tree, four alternating runs.
The kernels' registers, LDS and scratch are the compiler's resource report for gfx950 (tools/resource_usage.py), printed first; each
timed gather is held to fancy indexing before anything is timed."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import profile_common as common  # noqa: E402  (puts the repository, tools/ and tests/ on sys.path)

HBM_ACHIEVABLE_TBS = 6.3          # what a streaming copy reaches of the MI355X's 8 TB/s HBM3E peak (measured, float4 copy: 79 %)


def resources():
    import resource_usage
    rows = resource_usage.usage(os.path.join(common.ROOT, 'deeprl_network_amd', 'csrc', 'minibatch.hip'))
    print('compiler resource report, gfx950 (csrc/minibatch.hip):')
    for r in rows:
        name = r['name'].split('(')[0].split('::')[-1]
        print('    %-32s VGPRs %3d, SGPRs %3d, scratch %d bytes/lane, LDS %d bytes/block, occupancy %d waves/SIMD'
              % (name, r['VGPRs'], r['TotalSGPRs'], r['ScratchSize [bytes/lane]'], r['LDS Size [bytes/block]'], r['Occupancy [waves/SIMD]']))


def timed(f, n=200, warm=20):
    import torch
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    us = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(us), min(us)


def gather_case(N, E, T, M, F=5, A=4, H=64):
    import torch
    from deeprl_network_amd import ops
    import ppo_minibatch_checks as mc
    Em = E // M
    f32 = lambda *s: torch.randn(*s, device='cuda')      # noqa: E731
    src = [(f32(T, E, N, F), T), (f32(T, N, E, A), T * N), (torch.randint(0, A, (T, E, N), dtype=torch.uint8, device='cuda'), T),
           (f32(T, E), T)] + [(f32(N, T * E), N * T) for _ in range(4)] + [(f32(N, E, H), N), (f32(N, E, H), N)]
    pairs = [(torch.zeros(s.numel() // M, dtype=s.dtype, device='cuda'), s) for s, _ in src]
    outer = [o for _, o in src]
    idx = torch.from_numpy(mc.perm(E, 2, 0, 12)[:Em].copy()).cuda()
    ops.minibatch_gather(pairs, idx, outer_of=outer)
    for (d, s), o in zip(pairs, outer):
        assert torch.equal(d, mc.gather_rows(s, idx.cpu().tolist(), o, E).reshape(-1)), 'the timed gather is not fancy indexing'
    nbytes = 2 * sum(d.numel() * d.element_size() for d, _ in pairs)
    med, lo = timed(lambda: ops.minibatch_gather(pairs, idx, outer_of=outer))
    print('    N = %2d, E = %4d, T = %3d, M = %d: %6.2f MB read + written; median %7.2f us, min %7.2f us = %.2f TB/s at the median '
          '(%.0f %% of the %.1f TB/s a streaming kernel reaches)' % (N, E, T, M, nbytes / 1e6, med, lo, nbytes / med / 1e6,
                                                                     nbytes / med / 1e6 / HBM_ACHIEVABLE_TBS * 100, HBM_ACHIEVABLE_TBS))


def perm_case(E):
    import torch
    from deeprl_network_amd import ops
    import ppo_minibatch_checks as mc
    cnt = torch.zeros(1, dtype=torch.int32, device='cuda')
    keys, out = torch.zeros(E, dtype=torch.int32, device='cuda'), torch.zeros(E, dtype=torch.int32, device='cuda')
    ops.minibatch_perm(12, 0, 2, cnt, keys, out)
    assert (out.cpu().numpy() == mc.perm(E, 2, 0, 12)).all()
    med, lo = timed(lambda: ops.minibatch_perm(12, 0, 2, cnt, keys, out))
    print('    E = %4d: median %7.2f us, min %7.2f us (two launches, %d key compares)' % (E, med, lo, E * E))


def main():
    import torch
    parent = common.parent_tree_arg()
    assert torch.cuda.is_available(), 'needs the MI355X'
    print('replica minibatches of the PPO epochs (tools/ppo_minibatch_profile.py), %s' % torch.cuda.get_device_name(0))
    resources()
    print('(a) one gather call for a full step\'s operand list (10 pairs, one launch), an eager call between two events:')
    for N, E, T in ((8, 4096, 60), (25, 1024, 120)):
        for M in (2, 8):
            gather_case(N, E, T, M)
    print('(b) the permutation of an epoch (keys, then rank-and-scatter), an eager call between two events:')
    for E in (1024, 4096):
        perm_case(E)
    print('(c) config_ia2c_fp_catchup.ini at 8 x 4096, ppo_epochs = 2, captured update, blocks of %d batches, arms alternating:' % common.PER_BLOCK)
    order = {'M absent': dict(ppo_epochs=2)}
    order.update({'M = %d' % M: dict(ppo_epochs=2, ppo_minibatches=M) for M in (1, 2, 4, 8)})
    arms, ms = common.training_ab(order, blocks=6)
    med = common.report_arms(ms, 9)
    for k in list(order)[1:]:
        print('    %-9s / M absent: %.3f' % (k, med[k] / med['M absent']))
    common.close_arms(arms, captured_update=True)
    if parent:
        print('(d)', end=' ')
        common.bench_ab(parent)
    return 0


if __name__ == '__main__':
    sys.exit(main())

"""First measurement of the opt-in running return-based reward scaling, one box, one process:
    python tools/reward_scale_profile.py > profiles/r21_reward_scale.txt

(1) ops.reward_scale (reward_scale_scan_kernel + reward_scale_merge_kernel + reward_scale_apply_kernel) next to the two torch launches
it replaces in load_rewards (`torch.div(raw, reward_norm, out=buf_r)` + `buf_r.clamp_`), on the same reward buffers: 8 agents x 4096
replicas x 60 steps with the global reward [T, E], and 25 x 1024 x 120 with the global [T, E] and the per-agent [T, E, N] reward:
  single   one eager call between two events, the two alternating, 300 pairs: median and minimum.  An eager call between two events
           carries the launches' own floor; the yardstick is div + clamp_ measured the same way, not a fixed time.
  block    100 calls back to back between two events, alternating block by block, 10 blocks each: median per call.
Each shape's first call is held to the bound of tests/reward_scale_checks.py before anything is timed.
(2) config_ia2c_fp_catchup.ini at 8 x 4096 through BatchedTrainer (captured), without the key -- the code path of before -- and with
reward_scale = return, two trainers in one process, blocks of 20 batches alternating, 8 blocks each: median ms per batch, to be read
against the +-1.5 % run-to-run spread of the batch time.  Done twice with fresh trainers, built and timed in either order.
(3) with --parent-tree DIR (a built checkout of the parent commit): `bench.py --gpus 1 --steps 20 --warmup 3` of that tree and of this
one, each run a fresh child process, alternating, 4 runs each: the key is absent in bench.py, so this is the parent's batch time
against this tree's on one box.
The kernels' registers, LDS, scratch and occupancy are the compiler's resource report for gfx950 (tools/resource_usage.py)."""
import contextlib
import io
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import profile_common as common  # noqa: E402  (puts the repository, tools/ and tests/ on sys.path)

SHAPES = [(8, 4096, 60, False), (25, 1024, 120, False), (25, 1024, 120, True)]       # (agents, replicas, steps, per-agent reward)
GAMMA, EPS, CLIP = 0.99, 1e-8, 2.0


def measure(N, E, T, per_agent):
    import numpy as np
    import torch
    import reward_scale_checks as rc
    from deeprl_network_amd import ops
    gen = torch.Generator().manual_seed(N * 10007 + E * 101 + T + per_agent)
    raw = (torch.randn((T, E, N) if per_agent else (T, E), generator=gen) * 300 - 100).cuda()
    done = (torch.rand(T, E, generator=gen) < 0.02).to(torch.uint8).cuda()
    buf_r, out = torch.zeros_like(raw), torch.zeros_like(raw)
    S = raw[0].numel()
    C = ops.reward_scale_chunks(S)
    carry = torch.zeros(S, dtype=torch.float64, device='cuda')
    state = torch.zeros(ops.REWARD_SCALE_STATE, dtype=torch.float64, device='cuda')
    partial = torch.zeros(C, 4, dtype=torch.float64, device='cuda')

    def div_clamp():
        torch.div(raw, 800.0, out=buf_r)
        buf_r.clamp_(-CLIP, CLIP)
    run = {'div + clamp_': div_clamp,
           'reward_scale': lambda: ops.reward_scale(raw, done, GAMMA, EPS, CLIP, carry, state, partial, out)}
    # the timed call is the call the tests pin (a timing of a kernel that computes something else is worthless)
    run['reward_scale']()
    torch.cuda.synchronize()
    ref = rc.Restatement(E, N if per_agent else 0, GAMMA, EPS, CLIP)
    r_np = raw.cpu().numpy().reshape(T, S)
    st = state.cpu().numpy()
    with contextlib.redirect_stdout(io.StringIO()):
        worst = rc.assert_call(dict(r_out=out.cpu().numpy().reshape(T, S), carry=carry.cpu().numpy(), n=st[0], mean=st[5], sigma=st[6]),
                               r_np, ref.call(r_np, done.cpu().numpy()), EPS, CLIP, 'the timed call')
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
    assert bool(np.isfinite(state.cpu().numpy()).all())
    print('N = %d, E = %d, T = %d, %s reward: %d streams, %d scan blocks, %.1f MB of rewards; the checked call uses %.2g of the bound:'
          % (N, E, T, 'per-agent' if per_agent else 'global', S, C, 4 * T * S / 1e6, worst))
    med = {}
    for k in run:
        med[k] = (statistics.median(single[k]), statistics.median(block[k]))
        print('    %-13s single call: median %7.2f us, min %7.2f us;  back to back: median %7.2f us per call (min %7.2f, max %7.2f)'
              % (k, med[k][0], min(single[k]), med[k][1], min(block[k]), max(block[k])))
    print('    reward_scale / (div + clamp_): %.2f (single call), %.2f (back to back)'
          % tuple(med['reward_scale'][i] / med['div + clamp_'][i] for i in (0, 1)))


def training_ab(first):
    keys = {'key absent': {}, 'reward_scale = return': dict(reward_scale='return')}
    arms, ms = common.training_ab({k: keys[k] for k in sorted(keys, key=lambda k: k != first)})      # `first` is built and timed first
    env, model, _ = arms['key absent']
    print('config_ia2c_fp_catchup.ini, %d agents x %d replicas, n_step %d, captured, %d blocks of %d batches per arm, alternating, '
          '"%s" built and timed first:' % (env.n_agent, model.E, model.n_step, len(ms[first]), common.PER_BLOCK, first))
    med = common.report_arms(ms, 22)
    print('    reward_scale = return / key absent: %.4f (%+.2f %%; the documented run-to-run spread of the batch time is +-1.5 %%)'
          % (med['reward_scale = return'] / med['key absent'], (med['reward_scale = return'] / med['key absent'] - 1) * 100))
    print('    running std of the discounted return after these batches: %.6g (raw reward units)' % arms['reward_scale = return'][1].reward_scale_std)
    del env, model
    common.close_arms(arms)


def main():
    parent = common.parent_tree_arg()
    import torch
    assert torch.cuda.is_available(), 'needs the MI355X'
    print('running return-based reward scaling next to the division and clamp it replaces (tools/reward_scale_profile.py), %s'
          % torch.cuda.get_device_name(0))
    common.resources(27, names=('reward_scale_scan_kernel', 'reward_scale_merge_kernel', 'reward_scale_apply_kernel'))
    for shape in SHAPES:
        measure(*shape)
    for first in ('key absent', 'reward_scale = return'):      # two fresh pairs of trainers, built in either order
        training_ab(first)
    if parent:
        common.bench_ab(parent)
    return 0


if __name__ == '__main__':
    sys.exit(main())

"""First measurement of the opt-in PPO epochs, one box, one process:
    python tools/ppo_profile.py [--parent-tree DIR] > profiles/r22_ppo.txt

(1) ops.ppo_loss forward + backward (ppo_loss_kernel<fwd> + loss_reduce_kernel<5>, ppo_loss_kernel<bwd>) next to ops.a2c_loss forward +
backward on the same logits, values, actions, advantages and returns, and ops.ppo_logp alone, at 8 agents x 245 760 rows x 4 actions and
25 x 122 880 x 5: 50 calls back to back between two events, the arms alternating block by block, 10 blocks each: median us per call.
The timed ppo_loss call is first held to the float64 restatement of tests/ppo_checks.py at the tests' tolerances.
(2) config_ia2c_fp_catchup.ini at 8 x 4096 through BatchedTrainer (captured), the key absent against ppo_epochs = 2 and = 4, three
trainers in one process, blocks of 20 batches alternating, 8 blocks each: median ms per batch and ms per extra epoch, to be read against
the +-1.5 % run-to-run spread of the batch time.  Done twice with fresh trainers, built and timed in either order.
(3) with --parent-tree DIR (a built checkout of the parent commit): `bench.py --gpus 1 --steps 20 --warmup 3` of that tree and of this
one, each run a fresh child process, alternating, 4 runs each: the key is absent in bench.py, so this is the parent's batch time
against this tree's on one box.
The kernels' registers, LDS, scratch and occupancy are the compiler's resource report for gfx950 (tools/resource_usage.py)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import profile_common as common  # noqa: E402  (puts the repository, tools/ and tests/ on sys.path)

SHAPES = [(8, 245760, 4), (25, 122880, 5)]


def measure(N, rows, A):
    import torch
    import ppo_checks as pc
    from deeprl_network_amd import ops
    d = pc.inputs(N, rows, A)
    e = pc.expect(d)
    out = d['out'].cuda()
    v, adv, R, lo, act, w = (d[k].cuda() for k in ('v', 'adv', 'R', 'logp_old', 'action', 'w'))

    def ppo():
        o, vv = out.detach().requires_grad_(), v.detach().requires_grad_()
        tot, terms = ops.ppo_loss(o[..., :A], vv, act, adv, R, lo, d['clip'], pc.V_COEF, pc.E_COEF)
        (tot * w).sum().backward()
        return terms, o.grad, vv.grad

    def a2c():
        o, vv = out.detach().requires_grad_(), v.detach().requires_grad_()
        tot, terms = ops.a2c_loss(o[..., :A], vv, act, adv, R, pc.V_COEF, pc.E_COEF)
        (tot * w).sum().backward()
        return terms, o.grad, vv.grad
    logp_out = torch.empty(N, rows, device='cuda')
    run = {'a2c_loss fwd + bwd': a2c, 'ppo_loss fwd + bwd': ppo, 'ppo_logp': lambda: ops.ppo_logp(out[..., :A], act, out=logp_out)}
    # the timed call is the call the tests pin
    terms, dl, dv = ppo()
    torch.testing.assert_close(terms.cpu().double(), e['terms'], **pc.TERMS_TOL)
    torch.testing.assert_close(dl.cpu().double(), e['dlogits'], **pc.GRAD_TOL)
    torch.testing.assert_close(dv.cpu().double(), e['dv'], **pc.GRAD_TOL)
    for _ in range(10):
        for f in run.values():
            f()
    torch.cuda.synchronize()
    block, reps = {k: [] for k in run}, 50
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
    print('N = %d, rows = %d, A = %d (logits a column block of pitch %d; %.1f MB of logits), the autograd wrapper included:'
          % (N, rows, A, A + 1, 4 * N * rows * (A + 1) / 1e6))
    med = {k: statistics.median(block[k]) for k in run}
    for k in run:
        print('    %-19s back to back: median %8.2f us per call (min %8.2f, max %8.2f)' % (k, med[k], min(block[k]), max(block[k])))
    print('    ppo_loss / a2c_loss: %.2f' % (med['ppo_loss fwd + bwd'] / med['a2c_loss fwd + bwd']))


def training_ab(order):
    names = {None: 'key absent', 2: 'ppo_epochs = 2', 4: 'ppo_epochs = 4'}
    arms, ms = common.training_ab({names[K]: {} if K is None else dict(ppo_epochs=K) for K in order})
    env, model, _ = arms['key absent']
    print('config_ia2c_fp_catchup.ini, %d agents x %d replicas, n_step %d, captured, %d blocks of %d batches per arm, alternating, '
          'built and timed in the order %s:' % (env.n_agent, model.E, model.n_step, len(ms['key absent']), common.PER_BLOCK, ', '.join(arms)))
    med = common.report_arms(ms, 15)
    for K in (2, 4):
        print('    %s: %+.3f ms per batch over the key absent = %.3f ms per extra epoch; approx_kl %.3g, clip_frac %.3g in the last epoch'
              % (names[K], med[names[K]] - med['key absent'], (med[names[K]] - med['key absent']) / (K - 1), arms[names[K]][1].ppo_kl,
                 arms[names[K]][1].ppo_clip_frac))
    del env, model
    common.close_arms(arms, captured_update=True)


def main():
    parent = common.parent_tree_arg()
    import torch
    assert torch.cuda.is_available(), 'needs the MI355X'
    print('PPO epochs: the clipped-surrogate loss next to the A2C loss, and K optimiser steps per batch (tools/ppo_profile.py), %s'
          % torch.cuda.get_device_name(0))
    common.resources(30, prefixes=('ppo_', 'a2c_loss_', 'loss_reduce_'))
    for shape in SHAPES:
        measure(*shape)
    for order in ((None, 2, 4), (4, 2, None)):      # two fresh sets of trainers, built in either order
        training_ab(order)
    if parent:
        common.bench_ab(parent)
    return 0


if __name__ == '__main__':
    sys.exit(main())

"""First measurement of the opt-in value clipping and KL stop of the PPO epochs, one box, one process:
    python tools/ppo_vclip_kl_profile.py [--parent-tree DIR] > profiles/r23_ppo_vclip_kl.txt

(1) ops.ppo_loss forward + backward with v_old / vclip (ppo_loss_kernel<fwd, vclip> + loss_reduce_kernel<6>,
ppo_loss_kernel<bwd, vclip>) next to the same call without them, on the same data, at 8 agents x 245 760 rows x 4 actions and
25 x 122 880 x 5: 50 calls back to back between two events, the arms alternating block by block, 10 blocks each: median us per call.
The timed value-clip call is first held to the float64 restatement of tests/ppo_vclip_checks.py at the tests' tolerances.
(2) the two gate launches (ops.ppo_kl_sum, ops.ppo_kl_gate), 200 pairs back to back, 10 blocks: median us per launch.
(3) config_ia2c_fp_catchup.ini at 8 x 4096 with ppo_epochs = 2 through BatchedTrainer (captured), both keys absent against both keys
on (ppo_vclip = 0.2, ppo_target_kl = 0.02), blocks of 20 batches alternating, 8 blocks each, done twice with fresh trainers built and
timed in either order: median ms per batch, to be read against the +-1.5 % run-to-run spread of the batch time.
(4) with --parent-tree DIR (a built checkout of the parent commit): the bench.py A/B of tools/profile_common.py -- the keys are absent in
bench.py, so this is the parent's batch time against this tree's on one box.
The kernels' registers, LDS, scratch and occupancy are the compiler's resource report for gfx950 (tools/resource_usage.py)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import profile_common as common  # noqa: E402  (puts the repository, tools/ and tests/ on sys.path)

import ppo_profile as base  # noqa: E402

KEYS = dict(ppo_vclip='0.2', ppo_target_kl='0.02')


def _blocks(run, reps, blocks=10):
    import torch
    for _ in range(10):
        for f in run.values():
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in run}
    for _ in range(blocks):
        for k, f in run.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                f()
            b.record()
            b.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3 / reps)
    return us


def measure(N, rows, A):
    import torch
    import ppo_checks as pc
    import ppo_vclip_checks as vc
    from deeprl_network_amd import ops
    d = vc.inputs(N, rows, A)
    e = vc.expect(d)
    out = d['out'].cuda()
    v, adv, R, lo, vo, act, w = (d[k].cuda() for k in ('v', 'adv', 'R', 'logp_old', 'v_old', 'action', 'w'))

    def loss(**kw):
        o, vv = out.detach().requires_grad_(), v.detach().requires_grad_()
        tot, terms = ops.ppo_loss(o[..., :A], vv, act, adv, R, lo, d['clip'], pc.V_COEF, pc.E_COEF, **kw)
        (tot * w).sum().backward()
        return terms, o.grad, vv.grad
    run = {'ppo_loss fwd + bwd': loss, 'value-clip loss fwd + bwd': lambda: loss(v_old=vo, vclip=d['vclip'])}
    terms, dl, dv = run['value-clip loss fwd + bwd']()          # the timed call is the call the tests pin
    torch.testing.assert_close(terms.cpu().double(), e['terms'], **pc.TERMS_TOL)
    torch.testing.assert_close(dl.cpu().double(), e['dlogits'], **pc.GRAD_TOL)
    torch.testing.assert_close(dv.cpu().double(), e['dv'], **pc.GRAD_TOL)
    us = _blocks(run, 50)
    print('N = %d, rows = %d, A = %d (logits a column block of pitch %d; v_old one more %.1f MB read per pass), the autograd wrapper '
          'included:' % (N, rows, A, A + 1, 4 * N * rows / 1e6))
    med = {k: statistics.median(us[k]) for k in run}
    for k in run:
        print('    %-26s back to back: median %8.2f us per call (min %8.2f, max %8.2f)' % (k, med[k], min(us[k]), max(us[k])))
    print('    value-clip / ppo_loss: %.3f (vclip_frac %.3f)' % (med['value-clip loss fwd + bwd'] / med['ppo_loss fwd + bwd'],
                                                                float(terms[:, 5].mean())))


def gate(N=8):
    import torch
    from deeprl_network_amd import ops
    terms = torch.rand(N, 6, device='cuda') * 0.01
    tail = torch.zeros(1, device='cuda')
    g = torch.tensor(ops.PPO_GATE_RESET, dtype=torch.int32, device='cuda')
    us = _blocks({'kl_sum': lambda: ops.ppo_kl_sum(terms, tail), 'kl_gate': lambda: ops.ppo_kl_gate(tail, N, 1.0, g)}, 200)
    print('the KL stop\'s two launches per epoch, N = %d, one thread each, back to back:' % N)
    for k, v in us.items():
        print('    ops.ppo_%-8s median %6.2f us per launch (min %6.2f, max %6.2f)' % (k, statistics.median(v), min(v), max(v)))


def training_ab(order):
    arms, ms = common.training_ab({name: dict(KEYS if name == 'both keys on' else {}, ppo_epochs=2) for name in order})
    env, model, _ = arms['keys absent']
    print('config_ia2c_fp_catchup.ini, ppo_epochs = 2, %d agents x %d replicas, n_step %d, captured, %d blocks of %d batches per arm, '
          'alternating, built and timed in the order %s:' % (env.n_agent, model.E, model.n_step, len(ms['keys absent']), common.PER_BLOCK, ', '.join(arms)))
    med = common.report_arms(ms, 13)
    on = arms['both keys on'][1]
    print('    both keys on (%s): %+.3f ms per batch (%+.2f %%); approx_kl %.3g, vclip_frac %.3g, ppo_epochs_done %d in the last update'
          % (', '.join('%s = %s' % kv for kv in KEYS.items()), med['both keys on'] - med['keys absent'],
             (med['both keys on'] / med['keys absent'] - 1) * 100, on.ppo_kl, on.ppo_vclip_frac, on.ppo_epochs_done))
    del env, model, on
    common.close_arms(arms, captured_update=True)


def main():
    parent = common.parent_tree_arg()
    import torch
    assert torch.cuda.is_available(), 'needs the MI355X'
    print('PPO epochs: the clipped value loss next to the unclipped one, the KL stop\'s launches, and both keys through the trainer '
          '(tools/ppo_vclip_kl_profile.py), %s' % torch.cuda.get_device_name(0))
    common.resources(36, prefixes=('ppo_', 'loss_reduce_'), title='compiler resource report, gfx950 (ppo_loss_kernel<BWD, VCLIP>):')
    for shape in base.SHAPES:
        measure(*shape)
    gate()
    for order in (('keys absent', 'both keys on'), ('both keys on', 'keys absent')):
        training_ab(order)
    if parent:
        common.bench_ab(parent)
    return 0


if __name__ == '__main__':
    sys.exit(main())

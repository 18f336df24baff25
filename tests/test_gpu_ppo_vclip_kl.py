"""The opt-in value clipping and KL stop of the PPO epochs on the device: the value-clip instantiation of ppo_loss_kernel and the two
gate kernels of csrc/a2c.hip against the float64 restatement of tests/ppo_vclip_checks.py, their bit-equality with nmarl_ppo_loss_*
where every row is inside, determinism, the ABI's refusals; and MODEL_CONFIG ppo_vclip / ppo_target_kl through BatchedTrainer (eager
and captured) and the one-replica path."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import ppo_checks as pc
import ppo_vclip_checks as vc
from helpers import GOLDEN, cacc_config, drive_scripted, load_npz

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

S = pc.SENTINEL
_EXPECT = {}


def _case(N, rows, A):
    """The generator's data and its float64 expectation, computed once per shape and left unchanged."""
    key = (N, rows, A)
    if key not in _EXPECT:
        d = vc.inputs(N, rows, A)
        _EXPECT[key] = (d, vc.expect(d))
    return _EXPECT[key]


def _raw(d, block, vclip):
    """The C entries themselves, forward and backward with g_up = d['w'], every output filled with the sentinel beforehand.
    vclip None: nmarl_ppo_loss_*; block: logits contiguous or as a column block (pc.column_block)."""
    from deeprl_network_amd import _lib
    lib, ptr, st = _lib.lib, _lib.ptr, _lib.stream
    A = d['A']
    N, rows = d['v'].shape
    lg = pc.column_block(d['out'], A, block).cuda()
    pitch = lg.shape[-1]
    v, adv, R, lo, vo, act, w = (d[k].cuda() for k in ('v', 'adv', 'R', 'logp_old', 'v_old', 'action', 'w'))
    C = lib.nmarl_ppo_loss_chunks(rows, N)
    cols = 5 if vclip is None else 6
    partial, out = torch.full((N, C, cols), S, device='cuda'), torch.full((N, cols), S, device='cuda')
    dl, dv = torch.full((N, rows, A), S, device='cuda'), torch.full((N, rows), S, device='cuda')
    head = (rows, N, A, ptr(lg), rows * pitch, pitch, ptr(v), ptr(act), ptr(adv), ptr(R), ptr(lo))
    if vclip is None:
        rc = (lib.nmarl_ppo_loss_fwd(*head, d['clip'], pc.V_COEF, pc.E_COEF, ptr(partial), ptr(out), st()),
              lib.nmarl_ppo_loss_bwd(*head, d['clip'], pc.V_COEF, pc.E_COEF, ptr(w), ptr(dl), ptr(dv), st()))
    else:
        rc = (lib.nmarl_ppo_loss_vclip_fwd(*head, ptr(vo), d['clip'], vclip, pc.V_COEF, pc.E_COEF, ptr(partial), ptr(out), st()),
              lib.nmarl_ppo_loss_vclip_bwd(*head, ptr(vo), d['clip'], vclip, pc.V_COEF, pc.E_COEF, ptr(w), ptr(dl), ptr(dv), st()))
    assert rc == (0, 0), rc
    torch.cuda.synchronize()
    return dict(terms=out, dlogits=dl, dv=dv, partial=partial)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize('N,rows,A,block', pc.LOSS_CASES)
def test_vclip_loss_equals_the_restatement(N, rows, A, block):
    d, e = _case(N, rows, A)
    g = _raw(d, block, d['vclip'])
    names = ('policy', 'value', 'entropy', 'approx_kl', 'clip_frac', 'vclip_frac')
    dev = (g['terms'].cpu().double() - e['terms']).abs().max(dim=0).values
    print('max |term error|:', dict(zip(names, dev.tolist())))
    print('max |dv error|: %.3e' % float((g['dv'].cpu().double() - e['dv']).abs().max()))
    for k in g:                                                   # sentinel-filled outputs are fully overwritten
        assert not bool((g[k] == S).any()), k
    torch.testing.assert_close(g['terms'].cpu().double(), e['terms'], **pc.TERMS_TOL)
    torch.testing.assert_close(g['dlogits'].cpu().double(), e['dlogits'][..., :A], **pc.GRAD_TOL)
    torch.testing.assert_close(g['dv'].cpu().double(), e['dv'], **pc.GRAD_TOL)
    # vclip_frac is a count over rows: exact, and the closed gradients are exact zeros
    assert torch.equal((g['terms'][:, 5].cpu().double() * rows).round(), (e['terms'][:, 5] * rows).round())
    assert torch.equal(g['dv'].cpu() == 0, e['dv'] == 0)


@pytest.mark.parametrize('N,rows,A,block', pc.LOSS_CASES)
def test_where_every_row_is_inside_the_bits_are_those_of_the_unclipped_loss(N, rows, A, block):
    d, _ = _case(N, rows, A)
    g, p = _raw(d, block, vc.HUGE), _raw(d, block, None)
    assert torch.equal(_bits(g['terms'][:, :5]), _bits(p['terms']))
    assert torch.equal(_bits(g['dlogits']), _bits(p['dlogits'])) and torch.equal(_bits(g['dv']), _bits(p['dv']))
    assert not g['terms'][:, 5].any()
    # and with the clip active the other four terms and dlogits still are
    c = _raw(d, block, d['vclip'])
    for j in (0, 2, 3, 4):
        assert torch.equal(_bits(c['terms'][:, j]), _bits(p['terms'][:, j])), j
    assert torch.equal(_bits(c['dlogits']), _bits(p['dlogits']))
    if rows >= 256:
        assert not torch.equal(c['terms'][:, 1], p['terms'][:, 1]) and not torch.equal(c['dv'], p['dv'])


@pytest.mark.parametrize('N,rows,A', [(8, 70001, 4), (3, 1, 8), (25, 1234, 5)])
def test_two_calls_give_the_same_bits(N, rows, A):
    d, _ = _case(N, rows, A)
    a, b = _raw(d, True, d['vclip']), _raw(d, True, d['vclip'])
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


@pytest.mark.parametrize('N,rows,A', [(8, 4096, 4), (3, 1, 8)])
def test_ops_ppo_loss_with_v_old_through_autograd(N, rows, A):
    from deeprl_network_amd import ops
    d, e = _case(N, rows, A)
    o = d['out'].cuda().requires_grad_()
    vv = d['v'].cuda().requires_grad_()
    tot, terms = ops.ppo_loss(o[..., :A], vv, d['action'].cuda(), d['adv'].cuda(), d['R'].cuda(), d['logp_old'].cuda(), d['clip'],
                              pc.V_COEF, pc.E_COEF, v_old=d['v_old'].cuda(), vclip=d['vclip'])
    (tot * d['w'].cuda()).sum().backward()
    assert tuple(terms.shape) == (N, 6) and not terms.requires_grad
    torch.testing.assert_close(tot.detach().cpu().double(), e['total'], **pc.TERMS_TOL)
    torch.testing.assert_close(terms.cpu().double(), e['terms'], **pc.TERMS_TOL)
    torch.testing.assert_close(o.grad.cpu().double(), e['dlogits'], **pc.GRAD_TOL)
    torch.testing.assert_close(vv.grad.cpu().double(), e['dv'], **pc.GRAD_TOL)
    assert torch.all(o.grad[..., A] == 0)


def test_abi_refusals_write_nothing():
    """The refusals of nmarl_ppo_loss_*, a null v_old and vclip 0 / -0.2 / NaN / inf: NMARL_EINVAL, every output keeps its bits."""
    from deeprl_network_amd import _lib
    lib, ptr, st = _lib.lib, _lib.ptr, _lib.stream
    N, rows, A = 3, 70, 4
    d = vc.inputs(N, rows, A)
    C = lib.nmarl_ppo_loss_chunks(rows, N)
    lg = d['out'][..., :A].contiguous().cuda()
    v, adv, R, lo, vo, act, w = (d[k].cuda() for k in ('v', 'adv', 'R', 'logp_old', 'v_old', 'action', 'w'))
    partial, loss_out = torch.full((N, C, 6), S, device='cuda'), torch.full((N, 6), S, device='cuda')
    dl, dv = torch.full((N, rows, A), S, device='cuda'), torch.full((N, rows), S, device='cuda')
    nan, inf = float('nan'), float('inf')

    def fwd(rows=rows, N=N, A=A, lg=ptr(lg), pitch=A, v=ptr(v), act=ptr(act), adv=ptr(adv), R=ptr(R), lo=ptr(lo), vo=ptr(vo), clip=0.2,
            vclip=0.25, partial=ptr(partial), out=ptr(loss_out)):
        return lib.nmarl_ppo_loss_vclip_fwd(rows, N, A, lg, rows * A, pitch, v, act, adv, R, lo, vo, clip, vclip, 0.5, 0.05, partial, out,
                                            st())

    def bwd(rows=rows, N=N, A=A, lg=ptr(lg), pitch=A, v=ptr(v), act=ptr(act), adv=ptr(adv), R=ptr(R), lo=ptr(lo), vo=ptr(vo), clip=0.2,
            vclip=0.25, g=ptr(w), dl=ptr(dl), dv=ptr(dv)):
        return lib.nmarl_ppo_loss_vclip_bwd(rows, N, A, lg, rows * A, pitch, v, act, adv, R, lo, vo, clip, vclip, 0.5, 0.05, g, dl, dv,
                                            st())

    common = [dict(rows=0), dict(rows=-1), dict(N=0), dict(N=-1), dict(A=0), dict(A=9), dict(pitch=A - 1), dict(lg=None), dict(act=None),
              dict(v=None), dict(adv=None), dict(R=None), dict(lo=None), dict(clip=0.0), dict(clip=-0.2), dict(clip=nan), dict(clip=inf),
              dict(vo=None), dict(vclip=0.0), dict(vclip=-0.2), dict(vclip=nan), dict(vclip=inf), dict(vclip=-inf)]
    for kw in common + [dict(partial=None), dict(out=None)]:
        assert fwd(**kw) == -1, ('fwd', kw)
    for kw in common + [dict(g=None), dict(dl=None), dict(dv=None)]:
        assert bwd(**kw) == -1, ('bwd', kw)
    torch.cuda.synchronize()
    for t in (partial, loss_out, dl, dv):
        assert bool((t == S).all())
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    for t in (partial, loss_out, dl, dv):
        assert not bool((t == S).any())


# ---------------------------------------------------------------------------------------------------------------- the gate kernels
def _gate():
    from deeprl_network_amd import ops
    return torch.tensor(ops.PPO_GATE_RESET, dtype=torch.int32, device='cuda')


@pytest.mark.parametrize('cols', [5, 6])
@pytest.mark.parametrize('N', [1, 8, 25])
def test_gate_kernels(N, cols):
    from deeprl_network_amd import ops
    g = torch.Generator().manual_seed(40 + N)
    terms = torch.rand(N, cols, generator=g) * 0.05
    terms[:, [0, 1, 2, 4]] = 1e6                                  # only column 3 may be read
    want = torch.zeros(1)
    vc.kl_sum(terms, want)
    tail = torch.full((2,), S, device='cuda')
    t_dev = terms.cuda()
    ops.ppo_kl_sum(t_dev, tail[:1])
    first = tail.clone()
    ops.ppo_kl_sum(t_dev, tail[:1])
    assert torch.equal(_bits(tail), _bits(first)) and float(tail[1]) == S          # bit-stable, one float written
    assert torch.equal(_bits(tail[:1].cpu()), _bits(want))                          # the agents in index order, fp32
    world = 2
    kl = float(np.float32(float(want)) / np.float32(world * N))
    up, down = float(np.nextafter(np.float32(kl), np.float32(1))), float(np.nextafter(np.float32(kl), np.float32(0)))
    for kappa, stop, done in ((up, 0, 2), (kl, 0, 2), (down, 1, 1), (kl * 1.5, 0, 2), (kl / 1.5, 1, 1)):
        gate = _gate()
        ops.ppo_kl_gate(tail[:1], world * N, kappa, gate)
        assert gate.tolist() == [stop, 0, done, 0], (kappa, kl, gate.tolist())
        assert (stop, done) == vc.gate_sequence([float(want)], kappa, world * N)
    # sticky: once raised, a small KL does not lower it and the counter stands; while down, the counter goes on
    gate = _gate()
    small = torch.zeros(1, device='cuda')
    ops.ppo_kl_gate(small, N, kl, gate)
    ops.ppo_kl_gate(tail[:1], world * N, down, gate)
    ops.ppo_kl_gate(small, N, kl, gate)
    ops.ppo_kl_gate(small, N, kl, gate)
    assert gate.tolist() == [1, 0, 2, 0]
    gate = _gate()
    for _ in range(3):
        ops.ppo_kl_gate(small, N, kl, gate)
    assert gate.tolist() == [0, 0, 4, 0]
    gate = _gate()
    ops.ppo_kl_gate(torch.full((1,), float('nan'), device='cuda'), N, kl, gate)     # a NaN fails closed
    assert gate.tolist() == [1, 0, 1, 0]


def test_gate_refusals_write_nothing():
    from deeprl_network_amd import _lib
    lib, ptr, st = _lib.lib, _lib.ptr, _lib.stream
    terms = torch.rand(4, 5, device='cuda')
    tail = torch.full((1,), S, device='cuda')
    gate = torch.full((4,), 7, dtype=torch.int32, device='cuda')
    nan, inf = float('nan'), float('inf')
    for a in ((0, ptr(terms), 5, ptr(tail)), (-1, ptr(terms), 5, ptr(tail)), (4, None, 5, ptr(tail)), (4, ptr(terms), 3, ptr(tail)),
              (4, ptr(terms), 5, None)):
        assert lib.nmarl_ppo_kl_sum(*a, st()) == -1, a
    for a in ((None, 4, 0.1, ptr(gate)), (ptr(tail), 0, 0.1, ptr(gate)), (ptr(tail), -2, 0.1, ptr(gate)), (ptr(tail), 4, 0.0, ptr(gate)),
              (ptr(tail), 4, -0.1, ptr(gate)), (ptr(tail), 4, nan, ptr(gate)), (ptr(tail), 4, inf, ptr(gate)), (ptr(tail), 4, 0.1, None),
              (ptr(tail), 4, 0.1, ptr(gate) + 2)):
        assert lib.nmarl_ppo_kl_gate(*a, st()) == -1, a
    torch.cuda.synchronize()
    assert float(tail) == S and gate.tolist() == [7, 7, 7, 7]
    assert lib.nmarl_ppo_kl_sum(4, ptr(terms), 5, ptr(tail), st()) == 0
    torch.cuda.synchronize()
    assert float(tail) != S


@pytest.mark.parametrize('optimizer', ['rmsprop', 'adam'])
def test_a_raised_stop_refuses_the_optimiser_step(optimizer):
    from deeprl_network_amd import ops
    g = torch.Generator().manual_seed(5)
    G, P = 3, 1000
    w, grad, s1, s2 = (torch.randn(G, P, generator=g).cuda() for _ in range(4))
    s1, s2 = s1.abs(), s2.abs()
    scratch = torch.zeros(G * 64 + 64, device='cuda')
    step = torch.full((1,), 5, dtype=torch.int32, device='cuda')
    norm = torch.full((G,), S, device='cuda')

    def apply(stop):
        if optimizer == 'adam':
            ops.adam_clip(w, grad, s1, s2, scratch, step, 1e-2, 0.9, 0.999, 1e-8, 40.0, norm_out=norm, stop=stop)
        else:
            ops.rmsprop_tf_clip(w, grad, s1, scratch, 1e-2, 0.99, 1e-5, 40.0, norm_out=norm, stop=stop)
    keep = [t.clone() for t in (w, s1, s2, step, norm)]
    gate = torch.tensor([1, 0, 3, 0], dtype=torch.int32, device='cuda')
    apply(gate)
    apply(gate)
    for a, b in zip((w, s1, s2, step, norm), keep):
        assert torch.equal(a, b)
    assert gate.tolist() == [1, 2, 3, 0]                           # the refused steps count themselves
    gate = _gate()
    apply(gate)
    assert not torch.equal(w, keep[0]) and not torch.equal(s1, keep[1]) and gate.tolist() == [0, 0, 1, 0]
    assert int(step) == (6 if optimizer == 'adam' else 5)
    with pytest.raises(ValueError, match='exclude'):
        ops.rmsprop_tf_clip(w, grad, s1, scratch, 1e-2, 0.99, 1e-5, 40.0, guard=True, stop=gate)


# ------------------------------------------------------------------------------------------------------------------ the engine
E_ENGINE, T_ENGINE = 16, 5
HUGE_KEYS = dict(ppo_vclip='1e30', ppo_target_kl='1e30')


def _build(agent, use_graph, extra=None, **trainer_kw):
    from deeprl_network_amd.envs import make_batch_env
    from deeprl_network_amd.main import init_agent
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    cp = cacc_config(agent=agent, scenario='catchup', n_step=T_ENGINE, coop_gamma=-1,
                     reward_norm=800.0 if agent.startswith('ia2c') else 5000.0)
    for k, v in (extra or {}).items():
        cp['MODEL_CONFIG'][k] = v
    env = make_batch_env(cp['ENV_CONFIG'], num_envs=E_ENGINE)
    np.random.seed(12)
    model = init_agent(env, cp['MODEL_CONFIG'], 10 ** 9, 12, num_envs=E_ENGINE)
    return env, model, BatchedTrainer(env, model, Counter(10 ** 12, 10 ** 12, 10 ** 12), use_graph=use_graph, **trainer_kw)


def _state(model):
    """Weights, optimiser slots and (Adam) the device counter."""
    ps = model.policy.params
    if model.optimizer == 'adam':
        return dict(flat=ps.flat.clone(), m=ps.adam_m.clone(), v=ps.adam_v.clone(), t=ps.adam_t.clone())
    return dict(flat=ps.flat.clone(), ms=ps.ms.clone())


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _run(agent, use_graph, extra, batches, **kw):
    env, model, tr = _build(agent, use_graph, extra=extra, **kw)
    per_batch = []
    for _ in range(batches):
        tr.run_batch()
        per_batch.append((model.ppo_stats.clone() if hasattr(model, 'ppo_stats') else None, model.ppo_epochs_done))
    torch.cuda.synchronize()
    assert tr.handoff_fallbacks == 0 and (not use_graph or tr.update_capture_error is None)
    return model, tr, per_batch


def _tails(stats):
    """The KL sums of epochs 2..K of an update as the gate sees them: fp32, the agents in index order."""
    out = []
    for k in range(1, stats.shape[0]):
        tail = torch.zeros(1)
        vc.kl_sum(torch.cat([torch.zeros(stats.shape[1], 3), stats[k, :, :1].cpu()], dim=1), tail)
        out.append(float(tail))
    return out


def _pooled(stats):
    """kl_2..kl_K: the sums over the number of agents, in fp32."""
    return [float(np.float32(s) / np.float32(stats.shape[1])) for s in _tails(stats)]


@pytest.mark.parametrize('agent,optimizer', [('ia2c_fp', 'rmsprop'), ('ia2c_fp', 'adam'), ('ia2c', 'rmsprop'), ('ma2c_cu', 'rmsprop')])
def test_huge_keys_are_the_keys_absent_bit_for_bit(agent, optimizer):
    base = dict(ppo_epochs='3', optimizer=optimizer)
    off, _, st_off = _run(agent, True, base, 2)
    on, tr, st_on = _run(agent, True, dict(base, **HUGE_KEYS), 2)
    _same(_state(off), _state(on))
    for (a, _), (b, done) in zip(st_off, st_on):
        assert torch.equal(a, b) and done == 3
    assert not on.ppo_vclip_stats.any() and on.ppo_vclip_frac == 0.0 and off.ppo_epochs_done is None
    assert float(st_on[-1][0][1:, :, 0].max()) > 0


def test_zero_lr_applies_every_epoch_under_the_smallest_target():
    """lr_init = 0: the weights stay; where the update's first forward pass is the one epochs >= 2 recompute (the rollout's saved
    activations off) approx_kl is exactly 0 and even a target of 1e-30 lets every step through.
    With the saved activations on (the trainer's default) epoch 1's forward pass is the rollout's, which differs from the recomputed
    one by fp32 rounding: measured on an MI355X at these sizes, pooled approx_kl 7.8e-17, 5.8e-16 and 7.8e-16 in the first three
    updates, eager and captured alike -- above 1e-30, so the stop comes down at k = 2 and one step is applied.  That arrangement
    is held to the definition on its own KL, and to round 22's bound of 1e-6 on it."""
    keys = dict(ppo_epochs='3', lr_init='0', ppo_target_kl='1e-30', ppo_vclip='1e-30')
    model, _, per = _run('ia2c_fp', False, keys, 2, save_activations=False)
    for st, done in per:
        print('max approx_kl at lr 0: %.3e' % float(st[1:, :, 0].max()))
        assert done == 3
    assert not model.ppo_vclip_stats.any()                         # v = v_old to the bit as well
    model, _, per = _run('ia2c_fp', False, keys, 2)
    assert model.save_acts
    for st, done in per:
        print('saved activations: pooled approx_kl at lr 0:', _pooled(st))
        assert float(st[1:, :, 0].max()) < 1e-6 and done == vc.gate_sequence(_tails(st), 1e-30, model.n_agent)[1]


@pytest.mark.parametrize('optimizer', ['rmsprop', 'adam'])
def test_the_smallest_target_leaves_the_a2c_step_alone(optimizer):
    one, _, _ = _run('ia2c_fp', True, dict(optimizer=optimizer), 2)
    stop, _, per = _run('ia2c_fp', True, dict(ppo_epochs='3', ppo_target_kl='1e-30', optimizer=optimizer), 2)
    assert [d for _, d in per] == [1, 1] and stop.ppo_gate.tolist() == [1, 2, 1, 0]
    _same(_state(one), _state(stop))
    if optimizer == 'adam':
        assert int(stop.policy.params.adam_t) == 2


MID = dict(lr_init='5e-4')        # the shipped learning rate of config_ia2c_fp_catchup.ini


@pytest.mark.parametrize('optimizer', ['rmsprop', 'adam'])
def test_a_stop_in_the_middle_of_an_update(optimizer):
    """The target-off run with K = 4 gives the pooled kl_2..kl_4 of the first update; the target is put between kl_k* and the largest
    KL in front of it: the run with the target applies k* - 1 steps and ends in the state of ppo_epochs = k* - 1, eager and
    captured (the captured run's first update is eager; its second, replayed, is held to the eager run's and to the definition)."""
    base = dict(MID, optimizer=optimizer)
    _, _, per = _run('ia2c_fp', False, dict(base, ppo_epochs='4'), 1)
    kls = _pooled(per[0][0])
    print('pooled kl_2..kl_4:', kls)
    ks = [k for k in (3, 4) if kls[k - 2] > 1.5 * max(kls[:k - 2])]
    assert ks, 'precondition: some k* >= 3 with kl_k* > 1.5 max(kl_2..kl_{k*-1}); got %r' % (kls,)
    k_star = ks[0]
    kappa = math.sqrt(kls[k_star - 2] * max(kls[:k_star - 2]))
    want, _, _ = _run('ia2c_fp', False, dict(base, ppo_epochs=str(k_star - 1)), 1)
    keyed = dict(base, ppo_epochs='4', ppo_target_kl=repr(kappa))
    got, _, per1 = _run('ia2c_fp', False, keyed, 1)
    assert per1[0][1] == k_star - 1 and got.ppo_gate.tolist() == [1, 4 - (k_star - 1), k_star - 1, 0]
    _same(_state(want), _state(got))
    # after the stop the weights stand: the remaining epochs recompute the same forward pass and report the same KL bits
    st = per1[0][0]
    for k in range(k_star, 4):
        assert torch.equal(st[k], st[k_star - 1])
    runs = []
    for use_graph in (False, True):
        m, tr, per3 = _run('ia2c_fp', use_graph, keyed, 3, **(dict(keep_graphs=True) if use_graph else {}))
        for stats, done in per3:
            stop, want_done = vc.gate_sequence(_tails(stats), kappa, m.n_agent)
            assert done == want_done and int(m.ppo_gate[0]) in (0, 1)
        runs.append((_state(m), [d for _, d in per3], per3[-1][0]))
    print('epochs done per update:', runs[0][1])
    _same(runs[0][0], runs[1][0])
    assert runs[0][1] == runs[1][1] and torch.equal(runs[0][2], runs[1][2]) and runs[0][1][0] == k_star - 1


@pytest.mark.parametrize('agent', ['ia2c_fp', 'ma2c_cu'])
def test_captured_update_with_both_keys_holds_kernel_nodes_only(agent):
    import graph_nodes as G
    runs = []
    for use_graph in (True, False):
        extra = dict(ppo_epochs='3', ppo_vclip='0.05', ppo_target_kl='1e-30' if agent == 'ma2c_cu' else '10')
        model, tr, per = _run(agent, use_graph, extra, 3, **(dict(keep_graphs=True) if use_graph else {}))
        if use_graph:
            assert tr._upd is not None and tr._upd['apply'] is None and tr._upd['chain'] == []
            c = G.census(tr._upd['grads'])
            assert c.get('kernel', 0) > 0 and set(c) == {'kernel'}, c
        vs = model.ppo_vclip_stats
        assert not vs[0].any() and bool((vs >= 0).all()) and bool((vs <= 1).all())
        runs.append((_state(model), vs.clone(), model.ppo_stats.clone(), model.ppo_v_old.clone(), [d for _, d in per]))
    _same(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1:4], runs[1][1:4]):
        assert torch.equal(a, b)
    assert runs[0][4] == runs[1][4] == ([1, 1, 1] if agent == 'ma2c_cu' else [3, 3, 3])


def test_consensus_pass_stands_still_after_a_refused_step():
    """ConseNet averages the LSTM weights behind every optimiser step: under the smallest target the state is that of one step."""
    one, _, _ = _run('ma2c_cu', True, {}, 2)
    stop, _, per = _run('ma2c_cu', True, dict(ppo_epochs='3', ppo_target_kl='1e-30'), 2)
    assert [d for _, d in per] == [1, 1]
    _same(_state(one), _state(stop))


def test_value_clip_changes_the_critic_step_only_where_it_clips():
    """A clip range the critic leaves within two steps (vclip_frac > 0) moves the weights away from the unclipped run's."""
    off, _, _ = _run('ia2c_fp', False, dict(MID, ppo_epochs='3'), 2)
    on, _, _ = _run('ia2c_fp', False, dict(MID, ppo_epochs='3', ppo_vclip='1e-4'), 2)
    assert on.ppo_vclip_frac > 0 and float(on.ppo_vclip_stats[1:].max()) <= 1
    assert not torch.equal(off.policy.params.flat, on.policy.params.flat)
    assert torch.isfinite(on.policy.params.flat).all()


@pytest.mark.parametrize('optimizer', ['rmsprop', 'adam'])
def test_one_replica_path(optimizer):
    """model.backward of the reference API (E = 1, update(rotate=True)): under the smallest target the run equals the one-step run
    and the states are still handed over by the last, refused step; with lr 0 every epoch is applied (no saved activations here)."""
    from deeprl_network_amd.agents import models
    z = load_npz(os.path.join(GOLDEN, 'nn_ia2c_fp_line.npz'))
    nb = z['nb']
    N = nb.shape[0]

    def run(**keys):
        cp = cacc_config(agent='ia2c_fp', n_step=int(z['n_step']), reward_norm=float(z['reward_norm']), coop_gamma=-1)
        cp['MODEL_CONFIG']['optimizer'] = optimizer
        for k, v in keys.items():
            cp['MODEL_CONFIG'][k] = v
        np.random.seed(int(z['seed']))
        model = models.IA2C_FP([5 * (1 + int(nb[i].sum())) for i in range(N)], [4] * N, nb, z['dist'], -1.0, 10000, cp['MODEL_CONFIG'],
                               seed=int(z['seed']), num_envs=1, device='cuda')
        rotations, done = [], []
        inner = model.update_apply
        model.update_apply = lambda lr, rotate=True, lr_dev=None: rotations.append(rotate) or inner(lr, rotate=rotate, lr_dev=lr_dev)
        inner_b = model.backward
        model.backward = lambda *a, **kw: (inner_b(*a, **kw), done.append(model.ppo_epochs_done))
        drive_scripted(model, z)
        return model, rotations, done
    one, _, _ = run()
    stop, rotations, done = run(ppo_epochs='3', ppo_target_kl='1e-30', ppo_vclip='0.2')
    assert len(done) >= 1 and done == [1] * len(done) and rotations == [False, False, True] * len(done)
    _same(_state(one), _state(stop))
    assert torch.equal(one.h_bw, stop.h_bw) and torch.equal(one.c_bw, stop.c_bw)
    still, _, done = run(ppo_epochs='3', ppo_target_kl='1e-30', lr_init='0')
    assert done == [3] * len(done)

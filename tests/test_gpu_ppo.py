"""The opt-in PPO epochs on the device: the kernels of csrc/a2c.hip (ppo_logp_kernel, ppo_loss_kernel, loss_reduce_kernel) against
the float64 restatement of tests/ppo_checks.py, their bit-equality with the A2C loss at rho = 1, determinism and the ABI's refusals;
and MODEL_CONFIG ppo_epochs through BatchedTrainer (eager and captured) and the one-replica path."""
import os
import sys

import numpy as np
import pytest
import torch

import ppo_checks as pc
from helpers import GOLDEN, cacc_config, drive_scripted, load_npz

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

_EXPECT = {}


def _case(N, rows, A):
    """The generator's data and its float64 expectation, computed once per shape and left unchanged."""
    key = (N, rows, A)
    if key not in _EXPECT:
        d = pc.inputs(N, rows, A)
        _EXPECT[key] = (d, pc.expect(d), pc.logp(d['out'][..., :A].double(), d['action']))
    return _EXPECT[key]


def _native(d, block, loss=None, logp_old=None):
    """ops.ppo_loss forward + backward on the device: logits contiguous or as a column block (`block`, pc.column_block)."""
    from deeprl_network_amd import ops
    A = d['A']
    o = pc.column_block(d['out'], A, block).cuda().requires_grad_()
    logits = o[..., :A]
    vv = d['v'].cuda().requires_grad_()
    lo = d['logp_old'].cuda() if logp_old is None else logp_old
    tot, terms = (loss or ops.ppo_loss)(logits, vv, d['action'].cuda(), d['adv'].cuda(), d['R'].cuda(), lo, d['clip'], pc.V_COEF,
                                        pc.E_COEF)
    (tot * d['w'].cuda()).sum().backward()
    return dict(total=tot.detach(), terms=terms, dlogits=o.grad, dv=vv.grad)


# ------------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize('N,rows,A,block', pc.LOSS_CASES)
def test_ppo_loss_equals_the_restatement(N, rows, A, block):
    d, e, _ = _case(N, rows, A)
    g = _native(d, block)
    names = ('policy', 'value', 'entropy', 'approx_kl', 'clip_frac')
    dev = (g['terms'].cpu().double() - e['terms']).abs().max(dim=0).values
    print('max |term error|:', dict(zip(names, dev.tolist())))
    torch.testing.assert_close(g['terms'].cpu().double(), e['terms'], **pc.TERMS_TOL)
    torch.testing.assert_close(g['total'].cpu().double(), e['total'], **pc.TERMS_TOL)
    torch.testing.assert_close(g['dlogits'].cpu().double(), pc.column_block(e['dlogits'], A, block), **pc.GRAD_TOL)
    torch.testing.assert_close(g['dv'].cpu().double(), e['dv'], **pc.GRAD_TOL)
    if block:
        assert torch.all(g['dlogits'][..., A:] == 0)               # the padding columns receive no gradient


@pytest.mark.parametrize('N,rows,A,block', pc.LOSS_CASES)
def test_ppo_logp_equals_the_restatement(N, rows, A, block):
    from deeprl_network_amd import ops
    d, _, lp = _case(N, rows, A)
    out = d['out'].clone()
    out[..., A] = pc.SENTINEL
    out = pc.column_block(out, A, block or True, fill=pc.SENTINEL).cuda()
    logits = out[..., :A] if block else out[..., :A].contiguous()
    got = ops.ppo_logp(logits, d['action'].cuda())
    assert tuple(got.shape) == (N, rows) and got.dtype == torch.float32
    torch.testing.assert_close(got.cpu().double(), lp, **pc.LOGP_TOL)
    assert bool((out[..., A:] == pc.SENTINEL).all())               # the padding columns of the column block are not written
    dst = torch.full((N, rows), pc.SENTINEL, device='cuda')
    assert ops.ppo_logp(logits, d['action'].cuda(), out=dst) is dst and torch.equal(dst, got)
    # the probability below the clamp: log(1e-10)
    if rows >= 8:
        assert float((got[:, ::7] - float(np.log(np.float32(1e-10)))).abs().max()) < 1e-5


@pytest.mark.parametrize('N,rows,A,block', pc.LOSS_CASES)
def test_at_the_behaviour_policy_the_gradient_has_the_bits_of_the_a2c_loss(N, rows, A, block):
    from deeprl_network_amd import ops
    d, _, _ = _case(N, rows, A)
    src = pc.column_block(d['out'], A, block or True).cuda()
    logits = src[..., :A] if block else src[..., :A].contiguous()
    lo = ops.ppo_logp(logits, d['action'].cuda())
    g = _native(d, block, logp_old=lo)
    a = _native(d, block, loss=lambda lg, v, act, adv, R, lo_, clip, vc, ec: ops.a2c_loss(lg, v, act, adv, R, vc, ec))
    assert torch.equal(g['dlogits'].view(torch.int32), a['dlogits'].view(torch.int32))
    assert torch.equal(g['dv'].view(torch.int32), a['dv'].view(torch.int32))
    assert bool((g['terms'][:, 4] == 0).all()) and bool((g['terms'][:, 3] == 0).all())


@pytest.mark.parametrize('N,rows,A', [(8, 70001, 4), (3, 1, 8), (25, 1234, 5)])
def test_two_calls_give_the_same_bits(N, rows, A):
    from deeprl_network_amd import ops
    d, _, _ = _case(N, rows, A)
    a, b = _native(d, True), _native(d, True)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    lg = d['out'].cuda()[..., :A]
    assert torch.equal(ops.ppo_logp(lg, d['action'].cuda()).view(torch.int32), ops.ppo_logp(lg, d['action'].cuda()).view(torch.int32))


def test_support_and_chunk_count():
    from deeprl_network_amd import _lib, ops
    assert ops.ppo_loss_supported(8) and ops.ppo_loss_supported(1) and not ops.ppo_loss_supported(9)
    f = _lib.lib.nmarl_ppo_loss_chunks
    for N, rows in ((8, 245760), (25, 122880), (1, 1), (3, 70001)):
        assert f(rows, N) == _lib.lib.nmarl_a2c_loss_chunks(rows, N) >= 1
    assert f(0, 3) == 0 and f(5, 0) == 0


def test_abi_refusals_write_nothing():
    """rows 0, N 0, A 0 / 9, a row pitch below A, a null pointer, clip 0 / -0.2 / NaN / inf: NMARL_EINVAL, and every output keeps its
    bits."""
    from deeprl_network_amd import _lib
    lib, ptr, st = _lib.lib, _lib.ptr, _lib.stream
    N, rows, A = 3, 70, 4
    d = pc.inputs(N, rows, A)
    C = lib.nmarl_ppo_loss_chunks(rows, N)
    lg = d['out'][..., :A].contiguous().cuda()
    v, adv, R, lo, act, w = (d[k].cuda() for k in ('v', 'adv', 'R', 'logp_old', 'action', 'w'))
    S = pc.SENTINEL
    logp_out = torch.full((N, rows), S, device='cuda')
    partial, loss_out = torch.full((N, C, 5), S, device='cuda'), torch.full((N, 5), S, device='cuda')
    dl, dv = torch.full((N, rows, A), S, device='cuda'), torch.full((N, rows), S, device='cuda')
    nan, inf = float('nan'), float('inf')

    def logp(rows=rows, N=N, A=A, lg=ptr(lg), pitch=A, act=ptr(act), out=ptr(logp_out)):
        return lib.nmarl_ppo_logp(rows, N, A, lg, rows * A, pitch, act, out, st())

    def fwd(rows=rows, N=N, A=A, lg=ptr(lg), pitch=A, v=ptr(v), act=ptr(act), adv=ptr(adv), R=ptr(R), lo=ptr(lo), clip=0.2,
            partial=ptr(partial), out=ptr(loss_out)):
        return lib.nmarl_ppo_loss_fwd(rows, N, A, lg, rows * A, pitch, v, act, adv, R, lo, clip, 0.5, 0.05, partial, out, st())

    def bwd(rows=rows, N=N, A=A, lg=ptr(lg), pitch=A, v=ptr(v), act=ptr(act), adv=ptr(adv), R=ptr(R), lo=ptr(lo), clip=0.2,
            g=ptr(w), dl=ptr(dl), dv=ptr(dv)):
        return lib.nmarl_ppo_loss_bwd(rows, N, A, lg, rows * A, pitch, v, act, adv, R, lo, clip, 0.5, 0.05, g, dl, dv, st())

    common = [dict(rows=0), dict(rows=-1), dict(N=0), dict(N=-1), dict(A=0), dict(A=9), dict(pitch=A - 1), dict(lg=None), dict(act=None)]
    for kw in common + [dict(out=None)]:
        assert logp(**kw) == -1, ('logp', kw)
    loss_only = [dict(v=None), dict(adv=None), dict(R=None), dict(lo=None), dict(clip=0.0), dict(clip=-0.2), dict(clip=nan),
                 dict(clip=inf), dict(clip=-inf)]
    for kw in common + loss_only + [dict(partial=None), dict(out=None)]:
        assert fwd(**kw) == -1, ('fwd', kw)
    for kw in common + loss_only + [dict(g=None), dict(dl=None), dict(dv=None)]:
        assert bwd(**kw) == -1, ('bwd', kw)
    torch.cuda.synchronize()
    for t in (logp_out, partial, loss_out, dl, dv):
        assert bool((t == S).all())
    assert logp() == 0 and fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    for t in (logp_out, loss_out, dl, dv):
        assert not bool((t == S).any())


# ------------------------------------------------------------------------------------------------------------------ the engine
E_ENGINE, T_ENGINE = 8, 5
AGENTS = ['ia2c_fp', 'ia2c', 'ma2c_cu']
# the weight and gradient tolerances of tests/test_gpu_trainer.py's fused-vs-autograd heads comparison
W_TOL = dict(rtol=1e-3, atol=1e-5)
G_RTOL, G_ATOL_SCALE = 1e-4, 2e-6


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


def _spy_applies(model):
    """The flat gradient every update_apply of the model sees."""
    grads = []
    inner = model.update_apply

    def apply(lr, rotate=True, lr_dev=None):
        grads.append(model.policy.params.grad.clone())
        return inner(lr, rotate=rotate, lr_dev=lr_dev)
    model.update_apply = apply
    return grads


def _close_grads(g, g0):
    torch.testing.assert_close(g, g0, rtol=G_RTOL, atol=G_ATOL_SCALE * float(g0.abs().max()))


@pytest.mark.parametrize('agent', AGENTS)
def test_the_first_epoch_is_the_a2c_step(agent):
    seen = []
    for K in (None, '2'):
        env, model, tr = _build(agent, False, extra={} if K is None else dict(ppo_epochs=K))
        grads = _spy_applies(model)
        tr.run_batch()
        torch.cuda.synchronize()
        assert len(grads) == (1 if K is None else 2)
        seen.append(grads)
        del env, model, tr
    assert torch.equal(seen[0][0], seen[1][0]) and float(seen[0][0].abs().max()) > 0
    assert not torch.equal(seen[1][0], seen[1][1])


@pytest.mark.parametrize('agent', AGENTS)
def test_saved_start_state_is_the_state_the_batch_started_from(agent):
    """What epochs >= 2 unroll from (h_bw / c_bw) is slot 0 of the state sequences the rollout saved."""
    env, model, tr = _build(agent, True, extra=dict(ppo_epochs='2'))
    assert model.save_acts
    for _ in range(2):
        tr.run_batch()
    tr.rollout()
    torch.cuda.synchronize()
    assert torch.equal(model.H_all[:, 0], model.h_bw) and torch.equal(model.C_all[:, 0], model.c_bw)
    assert float(model.h_bw.abs().max()) > 0


@pytest.mark.parametrize('agent', AGENTS)
def test_native_loss_equals_the_restated_loss_in_the_engine(agent, monkeypatch):
    from deeprl_network_amd import ops
    runs = {}
    for name in ('native', 'restated', 'one'):
        if name == 'restated':
            monkeypatch.setattr(ops, 'ppo_loss', pc.restate_f32)
        env, model, tr = _build(agent, False, extra=dict(ppo_epochs='1' if name == 'one' else '3'))
        for _ in range(2):
            tr.run_batch()
        torch.cuda.synchronize()
        runs[name] = model.policy.params.flat.clone()
        assert torch.isfinite(runs[name]).all()
        del env, model, tr
    torch.testing.assert_close(runs['native'], runs['restated'], **W_TOL)
    for name in ('native', 'restated'):
        assert float((runs[name] - runs['one']).abs().max()) > 1e-4, name


@pytest.mark.parametrize('agent', AGENTS)
def test_captured_update_equals_eager(agent):
    import graph_nodes as G
    runs = []
    for use_graph in (True, False):
        env, model, tr = _build(agent, use_graph, extra=dict(ppo_epochs='3'), **(dict(keep_graphs=True) if use_graph else {}))
        for _ in range(3):
            tr.run_batch()
        torch.cuda.synchronize()
        assert tr.handoff_fallbacks == 0
        if use_graph:
            assert tr._upd is not None and tr.update_capture_error is None and tr._upd['apply'] is None and tr._upd['chain'] == []
            c = G.census(tr._upd['grads'])
            assert c.get('kernel', 0) > 0 and set(c) == {'kernel'}, c
        st = model.ppo_stats
        assert not st[0].any() and bool(torch.isfinite(st).all()) and bool((st[1:, :, 0] >= 0).all())
        assert bool((st[1:, :, 1] >= 0).all()) and bool((st[1:, :, 1] <= 1).all()) and float(st[1:, :, 0].max()) > 0
        assert model.ppo_kl == pytest.approx(float(st[-1, :, 0].mean())) and 0 <= model.ppo_clip_frac <= 1
        runs.append((model.policy.params.flat.clone(), st.clone(), model.ppo_logp_old.clone()))
        assert torch.isfinite(runs[-1][0]).all()
        del env, model, tr
    for a, b in zip(*runs):
        assert torch.equal(a, b), 'captured update with ppo_epochs differs from the eager one'


def test_a_huge_clip_never_clips():
    env, model, tr = _build('ia2c_fp', True, extra=dict(ppo_epochs='3', ppo_clip='1e9'))
    for _ in range(3):
        tr.run_batch()
    torch.cuda.synchronize()
    assert not model.ppo_stats[:, :, 1].any() and float(model.ppo_stats[1:, :, 0].max()) > 0


def test_zero_lr_saved_forward_equals_recomputed_forward():
    """lr_init = 0: the weights stay, so every epoch sees the behaviour policy -- clip_frac is 0, approx_kl below 1e-6 (the k3
    estimate at a log-probability difference of 1.4e-3, the 1e-3 class between two forward paths) and every epoch's gradient is
    epoch 1's within the weight-gradient tolerance: the forward pass epochs >= 2 recompute is the one the rollout saved.
    Measured on an MI355X: the largest approx_kl over agents and epochs is 7.1e-16 in the first batch and 4.6e-15 in the second."""
    env, model, tr = _build('ia2c_fp', False, extra=dict(ppo_epochs='3', lr_init='0'))
    assert model.save_acts
    grads = _spy_applies(model)
    w0 = model.policy.params.flat.clone()
    kl = []
    for _ in range(2):
        tr.run_batch()
        kl.append(model.ppo_stats.clone())
    torch.cuda.synchronize()
    assert torch.equal(model.policy.params.flat, w0) and len(grads) == 6
    for st in kl:
        print('max approx_kl at lr 0: %.3e' % float(st[1:, :, 0].max()))
        assert not st[:, :, 1].any() and float(st[1:, :, 0].max()) < 1e-6 and bool((st[1:, :, 0] >= 0).all())
    for b in range(2):
        assert float(grads[3 * b].abs().max()) > 0
        for k in (1, 2):
            _close_grads(grads[3 * b + k], grads[3 * b])


def test_ppo_with_the_other_opt_in_keys():
    extra = dict(ppo_epochs='2', gae_lambda='0.9', optimizer='adam', adv_norm='agent', reward_scale='return')
    runs = []
    for use_graph in (True, False):
        env, model, tr = _build('ia2c_fp', use_graph, extra=extra)
        for b in range(3):
            tr.run_batch()
            assert int(model.policy.params.adam_t) == 2 * (b + 1)
        torch.cuda.synchronize()
        runs.append((model.policy.params.flat.clone(), model.ppo_stats.clone(), model.Adv_n.clone()))
        assert torch.isfinite(runs[-1][0]).all() and float(runs[-1][1][1, :, 0].max()) > 0
        del env, model, tr
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_one_replica_backward_makes_two_steps():
    from deeprl_network_amd.agents import models
    z = load_npz(os.path.join(GOLDEN, 'nn_ia2c_fp_line.npz'))
    cp = cacc_config(agent='ia2c_fp', n_step=int(z['n_step']), reward_norm=float(z['reward_norm']), coop_gamma=-1)
    cp['MODEL_CONFIG']['ppo_epochs'] = '2'
    nb = z['nb']
    N = nb.shape[0]
    np.random.seed(int(z['seed']))
    model = models.IA2C_FP([5 * (1 + int(nb[i].sum())) for i in range(N)], [4] * N, nb, z['dist'], -1.0, 10000, cp['MODEL_CONFIG'],
                           seed=int(z['seed']), num_envs=1, device='cuda')
    rotations = []
    inner = model.update_apply
    model.update_apply = lambda lr, rotate=True, lr_dev=None: rotations.append(rotate) or inner(lr, rotate=rotate, lr_dev=lr_dev)
    n_back = []
    inner_b = model.backward
    model.backward = lambda *a, **kw: n_back.append(1) or inner_b(*a, **kw)
    drive_scripted(model, z)
    assert len(n_back) >= 1 and rotations == [False, True] * len(n_back)
    assert torch.isfinite(model.policy.params.flat).all() and bool(torch.isfinite(model.ppo_stats).all())
    assert bool((model.ppo_stats[1, :, 0] >= 0).all())


@pytest.mark.parametrize('agent', AGENTS)
def test_an_explicit_one_is_the_untouched_default_path(agent, monkeypatch):
    from deeprl_network_amd import ops
    n_ppo = []
    for name in ('ppo_logp', 'ppo_loss'):
        inner = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _f=inner, **kw: n_ppo.append(1) or _f(*a, **kw))
    runs = []
    for K in ('1', None):
        env, model, tr = _build(agent, True, extra={} if K is None else dict(ppo_epochs=K))
        assert model.ppo_epochs == 1 and not hasattr(model, 'ppo_logp_old') and not hasattr(model, 'ppo_stats')
        for _ in range(2):
            tr.run_batch()
        torch.cuda.synchronize()
        assert sorted(tr._upd) == ['apply', 'epilogue_inside', 'grads'] and not n_ppo
        runs.append(model.policy.params.flat.clone())
        del env, model, tr
    assert torch.equal(runs[0], runs[1])


@pytest.mark.parametrize('agent,extra', [('ma2c_nc', {}), ('ma2c_ic3', {}), ('ma2c_dial', {}), ('ia2c_fp', dict(lstm_precision='bf16x3'))])
def test_refusals(agent, extra):
    with pytest.raises(ValueError, match='ppo_epochs'):
        _build(agent, False, extra=dict(ppo_epochs='2', **extra))

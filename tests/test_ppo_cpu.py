"""The opt-in PPO epochs without a GPU: the float64 restatement of tests/ppo_checks.py is pinned to a literal per-agent PPO, every wrong
variant is told from it on the generator's data, and the host layers are followed from the ini keys and the CLI flags down to the
order of the calls one update makes (ops.ppo_logp / ops.ppo_loss replaced by recording restatements)."""
import configparser
import contextlib
import os

import numpy as np
import pytest
import torch

import ppo_checks as pc
from cpu_emulation import CpuCaccBatchEnv, cpu_ops
from helpers import cacc_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64


# -------------------------------------------------------------------------------------------- the restatement is the definition
def _literal(d):
    """PPO as one would write it for one agent at a time, float64."""
    A = d['A']
    tot, terms = [], []
    for n in range(d['out'].shape[0]):
        logits = d['out'][n, :, :A].double()
        a = d['action'][:, n].long()
        probs = torch.softmax(logits, dim=1)
        logp_all = torch.log(probs.clamp(1e-10, 1.0))
        new_logp = logp_all[torch.arange(len(a)), a]
        ratio = torch.exp(new_logp - d['logp_old'][n].double())
        adv = d['adv'][n].double()
        surr1 = ratio * adv
        surr2 = torch.clamp(ratio, 1.0 - d['clip'], 1.0 + d['clip']) * adv
        policy = -torch.min(surr1, surr2).mean()
        value = 0.5 * pc.V_COEF * ((d['R'][n].double() - d['v'][n].double()) ** 2).mean()
        entropy = -pc.E_COEF * (-(probs * logp_all).sum(dim=1)).mean()
        log_ratio = new_logp - d['logp_old'][n].double()
        kl = ((ratio - 1.0) - log_ratio).mean()
        cf = ((ratio - 1.0).abs() > d['clip']).double().mean()
        tot.append(policy + value + entropy)
        terms.append(torch.stack([policy, value, entropy, kl, cf]))
    return torch.stack(tot), torch.stack(terms)


@pytest.mark.parametrize('N,rows,A', [(8, 4096, 4), (25, 1234, 5), (3, 1, 8), (1, 257, 2)])
def test_restatement_equals_a_literal_ppo(N, rows, A):
    d = pc.inputs(N, rows, A)
    e = pc.expect(d)
    tot, terms = _literal(d)
    torch.testing.assert_close(e['total'], tot, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(e['terms'], terms, rtol=1e-12, atol=1e-14)
    assert bool((e['terms'][:, 3] >= 0).all()) and bool((e['dlogits'][..., A] == 0).all())
    if rows >= 256:
        assert bool((e['terms'][:, 4] > 0).all()) and bool((e['terms'][:, 4] < 1).all())


def test_gradient_is_the_closed_form_with_the_gate():
    """autograd of the restatement == -Adv rho gate c_a (delta - pi) / rows + the value and entropy parts of the A2C loss."""
    from oracle import ops_ref
    N, rows, A = 4, 700, 4
    d = pc.inputs(N, rows, A)
    e = pc.expect(d)
    l64 = d['out'][..., :A].double()
    pi = torch.softmax(l64, -1)
    acts = d['action'].t().long().unsqueeze(-1)
    pa = pi.gather(-1, acts).squeeze(-1)
    adv = d['adv'].double()
    rho = torch.exp(pc.logp(l64, d['action']) - d['logp_old'].double())
    gate = 1.0 - (((adv > 0) & (rho > 1 + d['clip'])) | ((adv < 0) & (rho < 1 - d['clip']))).double()
    assert 0 < float(gate.mean()) < 1
    onehot = torch.zeros_like(pi).scatter_(-1, acts, 1.0)
    d_pol = -(adv * rho * gate * (pa >= 1e-10).double()).unsqueeze(-1) * (onehot - pi) / rows
    # value and entropy parts: the A2C loss with a zero advantage
    o = d['out'].double().requires_grad_()
    vv = d['v'].double().requires_grad_()
    tot, _ = ops_ref.a2c_loss(o[..., :A], vv, d['action'], torch.zeros_like(adv), d['R'].double(), pc.V_COEF, pc.E_COEF)
    (tot * d['w'].double()).sum().backward()
    want = o.grad[..., :A] + d_pol * d['w'].double().view(-1, 1, 1)
    torch.testing.assert_close(e['dlogits'][..., :A], want, rtol=1e-10, atol=1e-15)
    torch.testing.assert_close(e['dv'], vv.grad, rtol=1e-12, atol=0)


def test_at_rho_one_the_gradient_is_the_a2c_gradient():
    from oracle import ops_ref
    d = pc.inputs(5, 300, 4)
    d['logp_old'] = pc.logp(d['out'][..., :4].double(), d['action'])          # float64: rho = 1 exactly
    e = pc.expect(d)
    o = d['out'].double().requires_grad_()
    vv = d['v'].double().requires_grad_()
    tot, _ = ops_ref.a2c_loss(o[..., :4], vv, d['action'], d['adv'].double(), d['R'].double(), pc.V_COEF, pc.E_COEF)
    (tot * d['w'].double()).sum().backward()
    torch.testing.assert_close(e['dlogits'], o.grad, rtol=1e-12, atol=1e-18)
    assert torch.equal(e['dv'], vv.grad) and not e['terms'][:, 3:].any()


@pytest.mark.parametrize('name', pc.WRONG)
def test_wrong_variant_is_told_apart(name):
    d = pc.inputs(8, 4096, 4, boundary=(name == 'clip_frac with >='))
    good = pc.expect(d)
    assert not pc.differs(good, pc.expect(d)), 'the restatement differs from itself'
    assert not pc.differs(good, pc.expect(d, dtype=F64, loss=pc.restate_f32))
    assert pc.differs(good, pc.expect(d, wrong=name)), name


def test_fp32_restatement_meets_the_device_tolerances():
    """The fp32 torch chain of the same formula lies inside the tolerances the kernels are held to (so a native loss and the
    restatement standing in for it can be compared at them)."""
    for N, rows, A in pc.SHAPES[:4]:
        d = pc.inputs(N, rows, A)
        a, b = pc.expect(d), pc.expect(d, dtype=F32)
        torch.testing.assert_close(b['terms'].double(), a['terms'], **pc.TERMS_TOL)


# --------------------------------------------------------------------------------------------------------------- host layers
@contextlib.contextmanager
def spied_ops():
    """cpu_ops() with ops.ppo_logp / ops.ppo_loss replaced by recording restatements, ops.a2c_loss, ops.rmsprop_tf_clip,
    ops.nstep_return and the policy's unroll recording their calls: -> the call lists."""
    from deeprl_network_amd import ops
    import adam_checks
    calls = dict(order=[], logp=[], loss=[], flat_at=[])
    with cpu_ops():
        saved = {k: getattr(ops, k) for k in ('ppo_logp', 'ppo_loss', 'a2c_loss', 'rmsprop_tf_clip', 'nstep_return', 'adam_clip')}
        inner = dict(saved)

        def ppo_logp(logits, action, out=None):
            calls['order'].append('logp')
            calls['logp'].append(dict(logits=logits.detach().clone(), out=out))
            r = pc.logp(logits.detach(), action)
            if out is None:
                return r
            out.copy_(r)
            return out

        def ppo_loss(logits, v, action, adv, R, logp_old, clip, v_coef, e_coef):
            calls['order'].append('ppo_loss')
            calls['loss'].append(dict(adv=adv, R=R, logp_old=logp_old, clip=clip, logits=logits.detach().clone()))
            return pc.restate(logits, v, action, adv, R, logp_old, clip, v_coef, e_coef)

        def a2c_loss(logits, *a, **kw):
            calls['order'].append('a2c_loss')
            calls['a2c_logits'] = logits.detach().clone()
            return inner['a2c_loss'](logits, *a, **kw)

        def rmsprop(w, *a, **kw):
            calls['order'].append('apply')
            calls['flat_at'].append(w.detach().clone())
            return inner['rmsprop_tf_clip'](w, *a, **kw)

        def adam(w, g, m, v, scratch, step, *a, guard=False, **kw):
            calls['order'].append('apply')
            return adam_checks.Fp32Adam().adam_clip(w, g, m, v, scratch, step, *a, **kw)

        def scan(*a, **kw):
            calls['order'].append('scan')
            return inner['nstep_return'](*a, **kw)

        ops.ppo_logp, ops.ppo_loss, ops.a2c_loss, ops.rmsprop_tf_clip, ops.nstep_return, ops.adam_clip = \
            ppo_logp, ppo_loss, a2c_loss, rmsprop, scan, adam
        try:
            yield calls
        finally:
            for k, f in saved.items():
                setattr(ops, k, f)


def _build(agent='ia2c_fp', E=3, n_step=5, trainer=True, **keys):
    from deeprl_network_amd.agents import models
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    cp = cacc_config(agent=agent, n_step=n_step, reward_norm=800.0, coop_gamma=-1, total_step=1200)
    cp['MODEL_CONFIG']['lr_decay'] = 'linear'
    cp['MODEL_CONFIG']['lr_min'] = '1e-5'
    for k, v in keys.items():
        if v is not None:
            cp['MODEL_CONFIG'][k] = v
    env = CpuCaccBatchEnv(cp['ENV_CONFIG'], num_envs=E)
    cls = {'ia2c': models.IA2C, 'ia2c_fp': models.IA2C_FP, 'ma2c_nc': models.MA2C_NC, 'ma2c_ic3': models.MA2C_IC3,
           'ma2c_cu': models.IA2C_CU, 'ma2c_dial': models.MA2C_DIAL}[agent]
    np.random.seed(12)
    model = cls(env.n_s_ls, env.n_a_ls, env.neighbor_mask, env.distance_mask, env.coop_gamma, 1200, cp['MODEL_CONFIG'], seed=12,
                num_envs=E, device='cpu')
    if not trainer:
        return env, model, None
    return env, model, BatchedTrainer(env, model, Counter(10 ** 6, 10 ** 7, 10 ** 4), use_graph=False)


@pytest.mark.parametrize('K', [2, 4])
def test_call_order_of_one_update(K):
    with spied_ops() as calls:
        _, model, tr = _build(ppo_epochs=str(K), ppo_clip='0.3')
        N, T, E = model.n_agent, model.n_step, model.E
        assert model.ppo_epochs == K and model.ppo_clip == 0.3
        assert tuple(model.ppo_logp_old.shape) == (N, T * E) and model.ppo_logp_old.dtype == F32
        assert tuple(model.ppo_stats.shape) == (K, N, 2) and model.ppo_stats.dtype == F32
        rotations = []
        inner_apply = model.update_apply
        model.update_apply = lambda lr, rotate=True, lr_dev=None: rotations.append((lr, rotate)) or inner_apply(lr, rotate=rotate, lr_dev=lr_dev)
        lrs, n_sched = [], model.lr_scheduler.n
        for b in range(2):
            tr.run_batch()
            lrs.append(model.cur_lr)
        per_update = ['scan', 'logp', 'a2c_loss', 'apply'] + ['ppo_loss', 'apply'] * (K - 1)
        assert calls['order'] == per_update * 2, calls['order']
        # the schedule advanced once per update; every epoch of an update used that update's lr
        assert model.lr_scheduler.n == n_sched + 2 * T and lrs[0] != lrs[1]
        assert [lr for lr, _ in rotations] == [lrs[0]] * K + [lrs[1]] * K
        assert not any(r for _, r in rotations)                  # (the batched trainer hands the states over itself)
        for b in range(2):
            # logp_old: before the first apply, from the logits of the first epoch's hidden states
            lp = calls['logp'][b]
            assert lp['out'] is model.ppo_logp_old
            for c in calls['loss'][b * (K - 1):(b + 1) * (K - 1)]:
                assert c['clip'] == 0.3 and c['logp_old'] is model.ppo_logp_old
                assert c['adv'].data_ptr() == model.Adv.data_ptr() and c['R'].data_ptr() == model.R.data_ptr()
                assert not torch.equal(c['logits'], lp['logits'])          # the forward was recomputed with stepped weights
        assert torch.equal(calls['logp'][1]['logits'], calls['a2c_logits'])
        # the weights moved in every step
        fl = calls['flat_at']
        assert len(fl) == 2 * K and all(not torch.equal(fl[i], fl[i + 1]) for i in range(len(fl) - 1))
        st = model.ppo_stats
        assert not st[0].any() and bool(torch.isfinite(st).all()) and bool((st[1:, :, 0] >= 0).all())
        assert bool((st[1:, :, 1] >= 0).all()) and bool((st[1:, :, 1] <= 1).all()) and float(st[1:, :, 0].max()) > 0
        assert model.ppo_kl == pytest.approx(float(st[-1, :, 0].mean())) and model.ppo_clip_frac == pytest.approx(float(st[-1, :, 1].mean()))
        assert tuple(model.loss_terms().shape) == (N, 3) and model.loss_terms().is_contiguous()
        assert torch.isfinite(model.policy.params.flat).all()


def test_rotate_only_on_the_last_epoch_and_adam_counts_every_step():
    """model.update(rotate=True) (the one-replica path's call): the states are handed over by the last step alone."""
    with spied_ops() as calls:
        _, model, tr = _build(ppo_epochs='3', optimizer='adam')
        tr.rollout()
        model.load_rewards(tr.buf_rraw)
        rotations = []
        inner_apply = model.update_apply
        model.update_apply = lambda lr, rotate=True, lr_dev=None: rotations.append(rotate) or inner_apply(lr, rotate=rotate, lr_dev=lr_dev)
        h_fw = model.h_fw.clone()
        assert not torch.equal(model.h_bw, h_fw)
        model.update(tr.R_end)
        assert rotations == [False, False, True] and torch.equal(model.h_bw, h_fw)
        assert calls['order'] == ['scan', 'logp', 'a2c_loss', 'apply', 'ppo_loss', 'apply', 'ppo_loss', 'apply']
        assert int(model.policy.params.adam_t) == 3 and model.t == 0


def test_saved_start_state_is_the_state_the_batch_started_from():
    """At update time h_bw / c_bw (what epochs >= 2 unroll from) equal slot 0 of the saved state sequences."""
    with spied_ops():
        _, model, tr = _build(ppo_epochs='2')
        for _ in range(2):
            tr.run_batch()
        tr.rollout()
        if model.save_acts:
            assert torch.equal(model.H_all[:, 0], model.h_bw) and torch.equal(model.C_all[:, 0], model.c_bw)
            assert float(model.h_bw.abs().max()) > 0


@pytest.mark.parametrize('agent', ['ia2c_fp', 'ia2c', 'ma2c_cu'])
def test_one_epoch_is_the_untouched_default_path(agent):
    runs = []
    for value in (None, '1', ' 1 '):
        with spied_ops() as calls:
            _, model, tr = _build(agent, ppo_epochs=value, ppo_clip=None if value is None else '0.1')
            assert model.ppo_epochs == 1 and not hasattr(model, 'ppo_logp_old') and not hasattr(model, 'ppo_stats')
            assert model.ppo_kl is None and model.ppo_clip_frac is None
            for _ in range(2):
                tr.run_batch()
            assert calls['order'] == ['scan', 'a2c_loss', 'apply'] * 2 and not calls['logp'] and not calls['loss']
            runs.append(model.policy.params.flat.clone())
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    with spied_ops():
        _, model, tr = _build(agent, ppo_epochs='2')
        for _ in range(2):
            tr.run_batch()
        assert not torch.equal(runs[0], model.policy.params.flat)


@pytest.mark.parametrize('keys,match', [(dict(ppo_epochs='0'), 'ppo_epochs'), (dict(ppo_epochs='-2'), 'ppo_epochs'),
                                        (dict(ppo_epochs='1.5'), 'ppo_epochs'), (dict(ppo_epochs='two'), 'ppo_epochs'),
                                        (dict(ppo_clip='0'), 'ppo_clip'), (dict(ppo_clip='-0.2'), 'ppo_clip'),
                                        (dict(ppo_clip='nan'), 'ppo_clip'), (dict(ppo_clip='inf'), 'ppo_clip'),
                                        (dict(ppo_epochs='2', ppo_clip='nan'), 'ppo_clip'),
                                        (dict(ppo_epochs='2', lstm_precision='bf16x3'), 'ppo_epochs')])
def test_config_refusals_name_the_key(keys, match):
    with cpu_ops():
        with pytest.raises(ValueError, match=match):
            _build(trainer=False, **keys)


@pytest.mark.parametrize('agent', ['ma2c_nc', 'ma2c_ic3', 'ma2c_dial'])
def test_coupled_nets_refuse_more_than_one_epoch(agent):
    with cpu_ops():
        with pytest.raises(ValueError, match='ppo_epochs'):
            _build(agent, trainer=False, ppo_epochs='2')
        _, model, _ = _build(agent, trainer=False, ppo_epochs='1')
        assert model.ppo_epochs == 1


def test_cli_flags_reach_the_run_ini_and_the_model_rebuilt_from_it(tmp_path):
    from deeprl_network_amd.main import apply_overrides, parse_args
    a0 = parse_args(['train'])
    assert a0.ppo_epochs is None and a0.ppo_clip is None
    args = parse_args(['train', '--ppo-epochs', '3', '--ppo-clip', '0.15'])
    assert args.ppo_epochs == 3 and args.ppo_clip == 0.15
    with pytest.raises(SystemExit):
        parse_args(['train', '--ppo-epochs', 'many'])
    cp = cacc_config(agent='ia2c_fp', n_step=5)
    run_ini = tmp_path / 'config.ini'
    with open(run_ini, 'w') as f:
        cp.write(f)
    before = open(run_ini, 'rb').read()
    assert not apply_overrides(cp, a0, str(run_ini)) and open(run_ini, 'rb').read() == before
    assert apply_overrides(cp, args, str(run_ini))
    back = configparser.ConfigParser()
    back.read(str(run_ini))
    assert back['MODEL_CONFIG'].getint('ppo_epochs') == 3 and back['MODEL_CONFIG'].getfloat('ppo_clip') == 0.15
    assert not back.has_option('MODEL_CONFIG', 'adv_norm') and back.has_section('ENV_CONFIG')
    # what `evaluate` does: the policy rebuilt from the run's ini (an evaluation-only model: total_step = 0, nothing allocated)
    from deeprl_network_amd.agents import models
    with cpu_ops():
        env = CpuCaccBatchEnv(back['ENV_CONFIG'], num_envs=2)
        model = models.IA2C_FP(env.n_s_ls, env.n_a_ls, env.neighbor_mask, env.distance_mask, env.coop_gamma, 0, back['MODEL_CONFIG'],
                               seed=12, num_envs=2, device='cpu')
    assert model.ppo_epochs == 3 and model.ppo_clip == 0.15 and not hasattr(model, 'ppo_stats') and model.ppo_kl is None


def test_every_reference_ini_has_no_ppo_key():
    import glob
    inis = sorted(glob.glob(os.path.join(ROOT, 'config', '*.ini')))
    assert inis
    for path in inis:
        cp = configparser.ConfigParser()
        cp.read(path)
        for key in ('ppo_epochs', 'ppo_clip'):
            assert not (cp.has_section('MODEL_CONFIG') and cp.has_option('MODEL_CONFIG', key)), (path, key)


def test_scalars_are_written_only_with_the_key_on():
    from deeprl_network_amd.utils import SummaryWriter, _write_ppo_scalars
    with spied_ops():
        for K, n in (('2', 2), (None, 0)):
            _, model, tr = _build(ppo_epochs=K)
            tr.run_batch()
            w = SummaryWriter()
            _write_ppo_scalars(w, model, 7)
            assert len(w._rows) == n
            if n:
                assert 'train/%s_ppo_kl' % model.policy.summary_name in w._rows[0] and '_ppo_clipfrac' in w._rows[1]


def test_new_kernels_use_no_scratch():
    """The four new kernels as compiled for gfx950: no scratch, no spills; the loss kernel's LDS is its four wave sums of five terms."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import resource_usage
    rows = {r['name']: r for r in resource_usage.usage(os.path.join(ROOT, 'deeprl_network_amd', 'csrc', 'a2c.hip'))}
    ppo = {n: r for n, r in rows.items() if n.startswith('ppo_') or n == 'loss_reduce_kernel<5>'}
    assert len(ppo) >= 3 and any('logp' in n for n in ppo) and any('reduce' in n for n in ppo), sorted(rows)
    for n, g in ppo.items():
        assert g['ScratchSize [bytes/lane]'] == 0 and g['VGPRs Spill'] == 0 and g['SGPRs Spill'] == 0, (n, g)
        print(n, {k: g[k] for k in g if 'GPR' in k or 'LDS' in k or 'Scratch' in k})

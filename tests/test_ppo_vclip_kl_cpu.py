"""Opt-in value clipping and KL stop of the PPO epochs (MODEL_CONFIG ppo_vclip, ppo_target_kl), without a GPU: the definition against
a literal PPO2 value loss, the wrong variants, the config / CLI layers and the call order of an update with a stop on the torch path
(the HIP-op wrappers replaced by the restatements of tests/ppo_vclip_checks.py)."""
import configparser
import contextlib
import glob
import os

import numpy as np
import pytest
import torch

import ppo_checks as pc
import ppo_vclip_checks as vc
from cpu_emulation import CpuCaccBatchEnv, cpu_ops
from helpers import cacc_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64


# ---------------------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize('N,rows,A', pc.SHAPES)
def test_generator_conditions_hold_at_every_shape(N, rows, A):
    d = vc.inputs(N, rows, A)             # (asserts its own margins and, for rows >= 256, the three kinds of rows on every agent)
    assert tuple(d['v_old'].shape) == (N, rows) and d['v_old'].dtype == F32 and d['vclip'] == vc.VCLIP
    assert torch.equal(d['v_old'][:, ::5], d['v'][:, ::5])
    base = pc.inputs(N, rows, A)
    for k in ('out', 'action', 'v', 'adv', 'R', 'logp_old', 'w'):
        assert torch.equal(d[k], base[k]), k


@pytest.mark.parametrize('N,rows,A', pc.SHAPES[:4])
def test_restatement_equals_a_literal_ppo2_value_loss(N, rows, A):
    d = vc.inputs(N, rows, A)
    a, b = vc.expect(d), vc.expect(d, loss=vc.literal)
    tight = dict(rtol=1e-12, atol=1e-14)
    for k in ('total', 'terms', 'dlogits', 'dv'):
        torch.testing.assert_close(a[k], b[k], **tight)
    if rows >= 256:
        assert float(a['terms'][:, 5].min()) > 0.2 and float(a['terms'][:, 5].max()) < 0.5
        # some gradients are closed (clipped rows with e2 > e1) and some clipped rows keep theirs
        dd = (d['v'] - d['v_old']).double().abs() > d['vclip']
        assert bool(((a['dv'] == 0) & dd).any()) and bool(((a['dv'] != 0) & dd).any())


def test_the_first_five_terms_and_dlogits_do_not_see_the_value_clip():
    d = vc.inputs(8, 4096, 4)
    a, b = vc.expect(d), pc.expect(d)
    for j in (0, 2, 3, 4):
        assert torch.equal(a['terms'][:, j], b['terms'][:, j])
    torch.testing.assert_close(a['dlogits'], b['dlogits'], rtol=1e-12, atol=1e-15)
    assert not torch.allclose(a['terms'][:, 1], b['terms'][:, 1], **pc.TERMS_TOL)
    # every row inside: the value term and its gradient are the unclipped ones
    c = vc.expect(d, vclip=vc.HUGE)
    assert torch.equal(c['terms'][:, :5], b['terms']) and torch.equal(c['dv'], b['dv']) and not c['terms'][:, 5].any()


@pytest.mark.parametrize('name', vc.WRONG)
def test_wrong_variant_is_told_apart(name):
    d = vc.inputs(8, 4096, 4, boundary=(name == 'vclip_frac with >='))
    good = vc.expect(d)
    assert not vc.differs(good, vc.expect(d)), 'the restatement differs from itself'
    assert not vc.differs(good, vc.expect(d, loss=vc.restate_f32))
    assert vc.differs(good, vc.expect(d, wrong=name)), name


def test_fp32_restatement_meets_the_device_tolerances():
    for N, rows, A in pc.SHAPES[:4]:
        d = vc.inputs(N, rows, A)
        a, b = vc.expect(d), vc.expect(d, dtype=F32)
        torch.testing.assert_close(b['terms'].double(), a['terms'], **pc.TERMS_TOL)
        torch.testing.assert_close(b['dv'].double(), a['dv'], **pc.GRAD_TOL)


def test_gate_sequence_is_strict_and_sticky():
    assert vc.gate_sequence([0.1, 0.5, 0.1], 0.3) == (1, 2)
    assert vc.gate_sequence([0.1, 0.3, 0.1], 0.3) == (0, 4)          # equal does not stop
    assert vc.gate_sequence([0.5, 0.0, 0.0], 0.3) == (1, 1)
    assert vc.gate_sequence([0.8, 0.8], 0.3, count=4) == (0, 3)      # the mean over ranks x agents is what is compared
    assert vc.gate_sequence([float('nan')], 0.3) == (1, 1)


# --------------------------------------------------------------------------------------------------------------- host layers
@contextlib.contextmanager
def spied_ops(kl_script=None):
    """cpu_ops() with the PPO ops, the optimiser steps, copy_multi and the two gate ops replaced by recording stand-ins.
    kl_script: per PPO epoch of the run (in call order) the approx_kl every agent reports in place of the computed one."""
    from deeprl_network_amd import ops
    import adam_checks
    calls = dict(order=[], loss=[], applied=[], gate=[], copies=[])
    names = ('ppo_logp', 'ppo_loss', 'rmsprop_tf_clip', 'adam_clip', 'copy_multi', 'ppo_kl_sum', 'ppo_kl_gate')
    with cpu_ops():
        saved = {k: getattr(ops, k) for k in names}
        inner = dict(saved)
        script = list(kl_script or [])

        def ppo_logp(logits, action, out=None):
            calls['order'].append('logp')
            out.copy_(pc.logp(logits.detach(), action))
            return out

        def ppo_loss(logits, v, action, adv, R, logp_old, clip, v_coef, e_coef, **kw):
            calls['order'].append('ppo_loss')
            calls['loss'].append(dict(kw))
            tot, terms = vc.restate_f32(logits, v, action, adv, R, logp_old, clip, v_coef, e_coef, **kw)
            if script:
                terms = terms.clone()
                terms[:, 3] = script.pop(0)
            return tot, terms

        def stopped(stop):
            if stop is not None and int(stop[0]) != 0:
                stop[1] += 1
                calls['order'].append('refused')
                return True
            calls['order'].append('apply')
            return False

        def rmsprop(w, *a, stop=None, **kw):
            if not stopped(stop):
                inner['rmsprop_tf_clip'](w, *a, **kw)
                calls['applied'].append(w.detach().clone())

        def adam(w, g, m, v, scratch, step, *a, guard=False, stop=None, **kw):
            if not stopped(stop):
                adam_checks.Fp32Adam().adam_clip(w, g, m, v, scratch, step, *a, **kw)

        def copy_multi(pairs, skip_if=None):
            calls['copies'].append(skip_if)
            if skip_if is None or int(skip_if.reshape(-1)[0]) == 0:
                for dst, src in pairs:
                    dst.copy_(src)

        def ppo_kl_sum(terms, tail):
            calls['order'].append('kl_sum')
            vc.kl_sum(terms, tail)

        def ppo_kl_gate(tail, count, kappa, gate):
            calls['order'].append('kl_gate')
            calls['gate'].append((float(tail[0]), count, kappa))
            vc.kl_gate(tail, count, kappa, gate)

        ops.ppo_logp, ops.ppo_loss, ops.rmsprop_tf_clip, ops.adam_clip = ppo_logp, ppo_loss, rmsprop, adam
        ops.copy_multi, ops.ppo_kl_sum, ops.ppo_kl_gate = copy_multi, ppo_kl_sum, ppo_kl_gate
        try:
            yield calls
        finally:
            for k, f in saved.items():
                setattr(ops, k, f)


def _build(agent='ia2c_fp', E=3, n_step=5, trainer=True, **keys):
    from deeprl_network_amd.agents import models
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    cp = cacc_config(agent=agent, n_step=n_step, reward_norm=800.0, coop_gamma=-1, total_step=1200)
    for k, v in keys.items():
        if v is not None:
            cp['MODEL_CONFIG'][k] = v
    env = CpuCaccBatchEnv(cp['ENV_CONFIG'], num_envs=E)
    cls = {'ia2c': models.IA2C, 'ia2c_fp': models.IA2C_FP, 'ma2c_nc': models.MA2C_NC, 'ma2c_cu': models.IA2C_CU}[agent]
    np.random.seed(12)
    model = cls(env.n_s_ls, env.n_a_ls, env.neighbor_mask, env.distance_mask, env.coop_gamma, 1200, cp['MODEL_CONFIG'], seed=12,
                num_envs=E, device='cpu')
    if not trainer:
        return env, model, None
    return env, model, BatchedTrainer(env, model, Counter(10 ** 6, 10 ** 7, 10 ** 4), use_graph=False)


@pytest.mark.parametrize('keys,match', [(dict(ppo_epochs='2', ppo_vclip='0'), 'ppo_vclip'), (dict(ppo_epochs='2', ppo_vclip='-0.2'), 'ppo_vclip'),
                                        (dict(ppo_epochs='2', ppo_vclip='nan'), 'ppo_vclip'), (dict(ppo_epochs='2', ppo_vclip='inf'), 'ppo_vclip'),
                                        (dict(ppo_epochs='2', ppo_vclip='wide'), 'ppo_vclip'), (dict(ppo_vclip='0.2'), 'ppo_vclip'),
                                        (dict(ppo_epochs='1', ppo_vclip='0.2'), 'ppo_epochs = 1'),
                                        (dict(ppo_epochs='2', ppo_target_kl='0'), 'ppo_target_kl'),
                                        (dict(ppo_epochs='2', ppo_target_kl='-1e-3'), 'ppo_target_kl'),
                                        (dict(ppo_epochs='2', ppo_target_kl='nan'), 'ppo_target_kl'),
                                        (dict(ppo_epochs='2', ppo_target_kl='inf'), 'ppo_target_kl'),
                                        (dict(ppo_target_kl='0.02'), 'ppo_target_kl'),
                                        (dict(ppo_epochs='1', ppo_target_kl='0.02'), 'ppo_epochs = 1')])
def test_config_refusals_name_the_key(keys, match):
    with cpu_ops():
        with pytest.raises(ValueError, match=match):
            _build(trainer=False, **keys)


@pytest.mark.parametrize('agent', ['ia2c_fp', 'ia2c', 'ma2c_cu'])
def test_keys_absent_allocate_nothing_and_run_the_path_of_before(agent):
    with spied_ops() as calls:
        _, model, tr = _build(agent, ppo_epochs='2')
        assert model.ppo_vclip is None and model.ppo_target_kl is None
        for name in ('ppo_v_old', 'ppo_vclip_stats', 'ppo_gate', '_ppo_gate_reset'):
            assert not hasattr(model, name), name
        assert model.ppo_vclip_frac is None and model.ppo_epochs_done is None
        tr.run_batch()
        assert calls['order'] == ['logp', 'apply', 'ppo_loss', 'apply'] and calls['loss'] == [{}] and not calls['gate']
        assert all(c is None for c in calls['copies'])
    with cpu_ops():
        _, model, _ = _build(agent, trainer=False)
        assert model.ppo_vclip is None and model.ppo_target_kl is None and model.ppo_epochs_done is None


def test_keys_on_allocate_their_state():
    with spied_ops():
        _, model, _ = _build(ppo_epochs='3', ppo_vclip='0.5', ppo_target_kl=' 0.02 ')
        N, T, E = model.n_agent, model.n_step, model.E
        assert model.ppo_vclip == 0.5 and model.ppo_target_kl == 0.02
        assert tuple(model.ppo_v_old.shape) == (N, T * E) and model.ppo_v_old.dtype == F32
        assert tuple(model.ppo_vclip_stats.shape) == (3, N) and tuple(model.ppo_stats.shape) == (3, N, 2)
        assert model.ppo_gate.dtype == torch.int32 and model.ppo_gate.tolist() == [0, 0, 1, 0]


def test_v_old_is_taken_with_logp_old_and_reaches_the_loss():
    with spied_ops() as calls:
        _, model, tr = _build(ppo_epochs='3', ppo_vclip='0.05')
        seen = []
        inner_heads = model.policy.heads

        def heads(Hs, action):
            r = inner_heads(Hs, action)
            seen.append(r[1].detach().clone())
            return r
        model.policy.heads = heads
        tr.run_batch()
        # the second result of the heads call in front of the first optimiser step
        first_apply = calls['order'].index('apply')
        assert calls['order'][:first_apply].count('logp') == 1
        assert any(torch.equal(model.ppo_v_old, s) for s in seen[:2])
        assert len(calls['loss']) == 2
        for kw in calls['loss']:
            assert kw['v_old'] is model.ppo_v_old and kw['vclip'] == 0.05
        st = model.ppo_vclip_stats
        assert not st[0].any() and bool((st >= 0).all()) and bool((st <= 1).all())
        assert model.ppo_vclip_frac == pytest.approx(float(st[-1].mean()))
        assert tuple(model.ppo_stats.shape) == (3, model.n_agent, 2)


@pytest.mark.parametrize('optimizer', [None, 'adam'])
def test_call_order_of_an_update_with_a_stop(optimizer):
    """K = 4, target 0.03; the epochs report 0.01, 0.05, 0.02: the step of epoch 3 and -- the stop is sticky -- of epoch 4 are refused,
    the rotation of the last step is done all the same."""
    with spied_ops(kl_script=[0.01, 0.05, 0.02, 0.01, 0.02, 0.03]) as calls:
        _, model, tr = _build(ppo_epochs='4', ppo_target_kl='0.03', optimizer=optimizer)
        N = model.n_agent
        tr.rollout()
        model.load_rewards(tr.buf_rraw)
        rotations = []
        inner_apply = model.update_apply
        model.update_apply = lambda lr, rotate=True, lr_dev=None: rotations.append(rotate) or inner_apply(lr, rotate=rotate, lr_dev=lr_dev)
        h_fw, flat0 = model.h_fw.clone(), model.policy.params.flat.clone()
        assert not torch.equal(model.h_bw, h_fw)
        model.update(tr.R_end)
        assert calls['order'] == ['logp', 'apply', 'ppo_loss', 'kl_sum', 'kl_gate', 'apply', 'ppo_loss', 'kl_sum', 'kl_gate', 'refused',
                                  'ppo_loss', 'kl_sum', 'kl_gate', 'refused'], calls['order']
        assert rotations == [False, False, False, True] and torch.equal(model.h_bw, h_fw)
        assert model.ppo_epochs_done == 2 and model.ppo_gate.tolist()[:3] == [1, 2, 2]
        assert [g[1:] for g in calls['gate']] == [(N, 0.03)] * 3
        assert [g[0] for g in calls['gate']] == [pytest.approx(N * k, rel=1e-6) for k in (0.01, 0.05, 0.02)]
        if optimizer is None:
            assert len(calls['applied']) == 2 and torch.equal(model.policy.params.flat, calls['applied'][-1])
            assert not torch.equal(calls['applied'][0], flat0) and not torch.equal(calls['applied'][0], calls['applied'][1])
        else:
            assert int(model.policy.params.adam_t) == 2          # the counter stands still on refused steps
        # the next update starts with the stop down; its epochs stay at or below the target: all four steps are applied
        del calls['order'][:]
        tr.rollout()
        model.load_rewards(tr.buf_rraw)
        model.update(tr.R_end)
        assert calls['order'].count('apply') == 4 and 'refused' not in calls['order']
        assert model.ppo_epochs_done == 4 and model.ppo_gate.tolist()[:3] == [0, 0, 4]


def test_a_kl_equal_to_the_target_does_not_stop():
    """Per-agent KL 2^-5 exactly: sum and mean are exact in fp32, the target is the same number."""
    with spied_ops(kl_script=[0.03125, 0.03125]) as calls:
        _, model, tr = _build(ppo_epochs='3', ppo_target_kl='0.03125')
        tr.run_batch()
        assert calls['order'].count('apply') == 3 and model.ppo_epochs_done == 3
    with spied_ops(kl_script=[0.03125, float(np.nextafter(np.float32(0.03125), np.float32(1)))]) as calls:
        _, model, tr = _build(ppo_epochs='3', ppo_target_kl='0.03125')
        tr.run_batch()
        assert calls['order'].count('apply') == 2 and calls['order'][-1] == 'refused' and model.ppo_epochs_done == 2


def test_consensus_pass_does_not_move_the_weights_after_a_refused_step():
    with spied_ops(kl_script=[0.5, 0.0]):
        _, model, tr = _build('ma2c_cu', ppo_epochs='3', ppo_target_kl='0.1')
        flats = []
        inner = model._after_apply
        model._after_apply = lambda: (inner(), flats.append(model.policy.params.flat.clone()))
        tr.run_batch()
        assert model.ppo_epochs_done == 1 and len(flats) == 3
        assert torch.equal(flats[0], flats[1]) and torch.equal(flats[1], flats[2])
    with spied_ops():
        _, model, tr = _build('ma2c_cu', ppo_epochs='3')
        flats = []
        inner = model._after_apply
        model._after_apply = lambda: (inner(), flats.append(model.policy.params.flat.clone()))
        tr.run_batch()
        assert not torch.equal(flats[0], flats[1]) and not torch.equal(flats[1], flats[2])


def test_coupled_nets_never_see_both_words():
    from deeprl_network_amd import ops
    w = torch.zeros(1, 4)
    with pytest.raises(ValueError, match='exclude'):
        ops._status_word(w, True, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match='two words'):
        ops._status_word(w, False, torch.zeros(1, dtype=torch.int32))
    with cpu_ops():
        with pytest.raises(ValueError, match='ppo_epochs'):
            _build('ma2c_nc', trainer=False, ppo_epochs='2', ppo_target_kl='0.02')


def test_ops_ppo_loss_wants_v_old_and_vclip_together():
    from deeprl_network_amd import ops
    d = vc.inputs(3, 1, 8)
    a = (d['out'][..., :8], d['v'], d['action'], d['adv'], d['R'], d['logp_old'], 0.2, 0.5, 0.05)
    with pytest.raises(ValueError, match='together'):
        ops.ppo_loss(*a, v_old=d['v_old'])
    with pytest.raises(ValueError, match='together'):
        ops.ppo_loss(*a, vclip=0.2)
    with pytest.raises(ValueError, match='shape of v'):
        ops.ppo_loss(*a, v_old=d['v_old'][:2], vclip=0.2)


def test_cli_flags_reach_the_run_ini_and_the_model_rebuilt_from_it(tmp_path):
    from deeprl_network_amd.main import apply_overrides, parse_args
    a0 = parse_args(['train'])
    assert a0.ppo_vclip is None and a0.ppo_target_kl is None
    args = parse_args(['train', '--ppo-epochs', '3', '--ppo-vclip', '0.4', '--ppo-target-kl', '0.015'])
    assert args.ppo_vclip == 0.4 and args.ppo_target_kl == 0.015
    with pytest.raises(SystemExit):
        parse_args(['train', '--ppo-target-kl', 'small'])
    cp = cacc_config(agent='ia2c_fp', n_step=5)
    run_ini = tmp_path / 'config.ini'
    with open(run_ini, 'w') as f:
        cp.write(f)
    before = open(run_ini, 'rb').read()
    assert not apply_overrides(cp, a0, str(run_ini)) and open(run_ini, 'rb').read() == before
    assert apply_overrides(cp, args, str(run_ini))
    back = configparser.ConfigParser()
    back.read(str(run_ini))
    mc = back['MODEL_CONFIG']
    assert mc.getint('ppo_epochs') == 3 and mc.getfloat('ppo_vclip') == 0.4 and mc.getfloat('ppo_target_kl') == 0.015
    assert not back.has_option('MODEL_CONFIG', 'ppo_clip')
    from deeprl_network_amd.agents import models
    with cpu_ops():
        env = CpuCaccBatchEnv(back['ENV_CONFIG'], num_envs=2)
        model = models.IA2C_FP(env.n_s_ls, env.n_a_ls, env.neighbor_mask, env.distance_mask, env.coop_gamma, 0, mc, seed=12,
                               num_envs=2, device='cpu')
    assert model.ppo_vclip == 0.4 and model.ppo_target_kl == 0.015
    assert not hasattr(model, 'ppo_gate') and model.ppo_epochs_done is None and model.ppo_vclip_frac is None


def test_help_names_both_flags(capsys):
    from deeprl_network_amd.main import parse_args
    with pytest.raises(SystemExit):
        parse_args(['train', '--help'])
    out = capsys.readouterr().out
    assert '--ppo-vclip' in out and '--ppo-target-kl' in out


def test_every_reference_ini_has_neither_key():
    inis = sorted(glob.glob(os.path.join(ROOT, 'config', '*.ini')))
    assert inis
    for path in inis:
        cp = configparser.ConfigParser()
        cp.read(path)
        for key in ('ppo_vclip', 'ppo_target_kl'):
            assert not (cp.has_section('MODEL_CONFIG') and cp.has_option('MODEL_CONFIG', key)), (path, key)


def test_scalars_are_written_only_with_the_keys_on():
    from deeprl_network_amd.utils import SummaryWriter, _write_ppo_scalars
    with spied_ops():
        for keys, n in ((dict(ppo_vclip='0.3', ppo_target_kl='10'), 4), (dict(ppo_vclip='0.3'), 3), (dict(ppo_target_kl='10'), 3), ({}, 2)):
            _, model, tr = _build(ppo_epochs='2', **keys)
            tr.run_batch()
            w = SummaryWriter()
            _write_ppo_scalars(w, model, 7)
            rows = ' '.join(str(r) for r in w._rows)
            assert len(w._rows) == n
            name = model.policy.summary_name
            assert ('train/%s_ppo_vclipfrac' % name in rows) == ('ppo_vclip' in keys)
            assert ('train/%s_ppo_epochs_done' % name in rows) == ('ppo_target_kl' in keys)


def test_new_kernels_use_no_scratch():
    """The value-clip instantiations and the two gate kernels as compiled for gfx950: no scratch, no spills."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import resource_usage
    rows = {r['name']: r for r in resource_usage.usage(os.path.join(ROOT, 'deeprl_network_amd', 'csrc', 'a2c.hip'))}
    loss = [n for n in rows if 'ppo_loss_kernel' in n]
    assert len(loss) == 4, sorted(rows)                                   # <BWD, VCLIP>: the two of before and the two new ones
    for want in ('loss_reduce_kernel<6>', 'ppo_kl_sum_kernel', 'ppo_kl_gate_kernel'):
        assert any(want in n for n in rows), (want, sorted(rows))
    for n, g in rows.items():
        if 'ppo_' in n or 'loss_reduce_kernel' in n:
            assert g['ScratchSize [bytes/lane]'] == 0 and g['VGPRs Spill'] == 0 and g['SGPRs Spill'] == 0, (n, g)
            print(n, {k: g[k] for k in g if 'GPR' in k or 'LDS' in k or 'Scratch' in k})

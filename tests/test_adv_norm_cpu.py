"""The opt-in per-batch advantage standardisation without a GPU: the float64 restatement of tests/adv_norm_checks.py is pinned, a
plain chunked (count, mean, M2) loop passes `check` at every shape and kind, `check` is shown to fail on every mistake it is meant to
see, and the host layers are followed from the ini keys and the CLI flag down to the op the update calls and the advantage the loss
reads."""
import contextlib
import os
import sys
import types

import numpy as np
import pytest
import torch

import adv_norm_checks as ac
from cpu_emulation import CpuCaccBatchEnv, cpu_ops
from helpers import cacc_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64


# -------------------------------------------------------------------------------------------- the restatement is the definition
@pytest.mark.parametrize('G,rows', [(1, 4096), (8, 40), (25, 600)])
def test_restatement_has_zero_mean_and_unit_std(G, rows):
    y, mu, sigma = ac.expect(ac.inputs(G, rows, 'adv'))
    assert float(np.abs(y.mean(axis=1)).max()) < 1e-6
    assert float(np.abs(y.std(axis=1) - 1.0).max()) < 1e-6                      # (numpy's std is the population one)
    x = ac.inputs(G, rows, 'adv').double().numpy()
    assert np.allclose(mu, x.mean(axis=1), rtol=1e-13, atol=0) and np.allclose(sigma, x.std(axis=1), rtol=1e-13, atol=0)


def test_restatement_edges():
    y, mu, sigma = ac.expect(ac.inputs(3, 1, 'adv'))                            # rows = 1: sigma = 0, y = 0
    assert not sigma.any() and not y.any()
    y, mu, sigma = ac.expect(ac.inputs(4, 257, 'const'))
    assert not sigma.any() and not y.any()
    y, _, _ = ac.expect(ac.inputs(2, 64, 'tiny'))                               # eps outside the root: ~1e-12, not ~1e-16
    assert 1e-13 < float(np.abs(y).max()) < 1e-10
    y, _, _ = ac.expect(ac.inputs(3, 65, 'one_nan'))
    assert np.isnan(y[1]).all() and np.isfinite(y[[0, 2]]).all()
    y, _, _ = ac.expect(ac.inputs(2, 255, 'huge'))
    assert np.isfinite(y).all() and float(np.abs(y.std(axis=1) - 1.0).max()) < 1e-6


# ------------------------------------------------------------------------------------------------- the check sees what it must
def _merge(a, b, guard=True):
    """Chan's formula for the moments (count, mean, M2) of a followed by b; an empty side is a no-op."""
    if guard and b[0] == 0:
        return a
    if guard and a[0] == 0:
        return b
    n = a[0] + b[0]
    with np.errstate(all='ignore'):
        d = b[1] - a[1]
        return (n, a[1] + d * (np.float64(b[0]) / n), a[2] + b[2] + d * d * (np.float64(a[0]) * (np.float64(b[0]) / n)))


def _impl(chunks=7, ddof=0, eps_inside=False, shortcut=False, acc32=False, final32=False, pooled=False, ignore_pitch=False,
          write_tail=False, ignore_out=False, guard=True, shift=True):
    """standardize as a plain loop over groups and chunks -- per chunk (count, mean, M2) from two passes, merged in chunk order, the
    means relative to the group's first element and mu from the chunks' plain sums as in the kernel -- with one mistake switched on."""
    def f(x, eps, out=None, partial=None, moments=None):
        G, rows = x.shape
        src = x.as_strided((G, rows), (rows, 1)) if ignore_pitch else x
        acc = np.float32 if acc32 else np.float64
        per = -(-rows // chunks)
        mom = []
        for g in range(G):
            xs = src[g].numpy().astype(acc)
            with np.errstate(all='ignore'):
                K = xs[0] if shift else acc(0)
                raw, xs = xs, xs - K
            tot, plain = (0, acc(0), acc(0)), acc(0)
            for c in range(chunks):
                piece = xs[c * per:(c + 1) * per]
                n = len(piece)
                with np.errstate(all='ignore'):
                    if shortcut:
                        mean = piece.sum() / acc(n) if n else acc(0)
                        m2 = (piece * piece).sum() - acc(n) * mean * mean
                    else:
                        mean = piece.sum() / acc(n) if (n or not guard) else acc(0)
                        m2 = ((piece - mean) * (piece - mean)).sum()
                    plain = plain + raw[c * per:(c + 1) * per].sum()
                tot = _merge(tot, (n, mean, m2), guard)
            with np.errstate(all='ignore'):
                mom.append((tot[0], plain / acc(rows), tot[2]))
        if pooled:
            tot = (0, 0.0, 0.0)
            for m in mom:
                tot = _merge(tot, m)
            mom = [tot] * G
        y = torch.empty(G, rows, dtype=F32) if (out is None or ignore_out) else out
        if write_tail and y.stride(0) > rows:
            y.as_strided((G, y.stride(0)), (y.stride(0), 1)).zero_()
        for g, (n, mean, m2) in enumerate(mom):
            with np.errstate(all='ignore'):
                var = np.float64(m2) / (n - ddof) if n - ddof > 0 else np.float64(0.0)
                sigma = np.sqrt(var + eps) if eps_inside else np.sqrt(var)
                den = sigma if eps_inside else sigma + eps
                xg = src[g].numpy()
                if final32:
                    yg = (xg - np.float32(mean)) / np.float32(den)
                else:
                    yg = ((xg.astype(np.float64) - np.float64(mean)) / den).astype(np.float32)
            y[g] = torch.from_numpy(yg)
            if moments is not None:
                moments[g, 0], moments[g, 1] = float(mean), float(np.sqrt(var))
        return y
    return types.SimpleNamespace(standardize=f)


# the shapes of the device test with the chunk counts a plain loop affords: fewer rows than chunks (empty chunks), the wave and block
# edges, odd rows, rows around a multiple of the chunk count, the engine's shapes
SHAPES = [(1, 1), (1, 2), (3, 1), (2, 63), (2, 64), (2, 65), (3, 255), (3, 256), (3, 257), (5, 1023), (2, 34), (2, 35), (2, 36),
          (8, 40), (25, 600), (4, 12289)]
FORMS = [(None, False), ('padded', False), (None, True), ('padded', True)]


def _pitch(form, rows):
    return None if form is None else (rows + 3, rows + 5)


@pytest.mark.parametrize('kind', ac.KINDS)
@pytest.mark.parametrize('form,inplace', FORMS)
@pytest.mark.parametrize('G,rows', SHAPES)
def test_plain_loop_passes(G, rows, form, inplace, kind):
    ac.check(_impl(), 'cpu', G, rows, kind, _pitch(form, rows), inplace)


@pytest.mark.parametrize('kind', ac.KINDS)
@pytest.mark.parametrize('chunks', [1, 256, 512])
def test_plain_loop_passes_with_other_chunk_counts(chunks, kind):
    """One chunk is the two-pass form itself; 256 and 512 chunks of a short group are mostly empty."""
    ac.check(_impl(chunks=chunks), 'cpu', 3, 257, kind)
    ac.check(_impl(chunks=chunks), 'cpu', 1, 100003, kind)


MUTANTS = {
    '(rows - 1) variance': (dict(ddof=1), (3, 257, 'adv', None, False)),
    'eps inside the root': (dict(eps_inside=True), (2, 64, 'tiny', None, False)),
    'sum-of-squares shortcut': (dict(shortcut=True, shift=False, chunks=1), (5, 1023, 'offset', None, False)),
    'sum-of-squares shortcut, small offset': (dict(shortcut=True, shift=False, chunks=1), (5, 1023, 'offset_small', None, False)),
    'sum-of-squares shortcut per chunk': (dict(shortcut=True, shift=False), (4, 12289, 'offset', None, False)),
    'fp32 accumulation': (dict(acc32=True, shift=False), (5, 1023, 'offset', None, False)),
    'fp32 accumulation overflows': (dict(acc32=True), (2, 65, 'huge', None, False)),
    # Chan's formula on plain means: the outputs pass, sigma is ~1e-11 off where the data sit far from zero (why the kernel keeps its
    # means relative to the group's first element)
    'chunk means not relative to the first element': (dict(shift=False), (2, 63, 'offset', None, False)),
    'final arithmetic in fp32': (dict(final32=True), (5, 1023, 'offset', None, False)),
    'moments pooled across groups': (dict(pooled=True), (3, 257, 'adv', None, False)),
    'pitch ignored': (dict(ignore_pitch=True), (3, 257, 'adv', (260, 262), False)),
    'pitch ignored in place': (dict(ignore_pitch=True), (3, 257, 'adv', (260, 260), True)),
    'tail overwritten': (dict(write_tail=True), (3, 257, 'adv', (260, 262), False)),
    'tail overwritten in place': (dict(write_tail=True), (3, 257, 'adv', (260, 260), True)),
    'caller\'s out ignored': (dict(ignore_out=True), (3, 257, 'adv', None, False)),
    'empty chunk merged as 0 / 0': (dict(guard=False), (1, 2, 'adv', None, False)),
    'empty chunk merged as 0 / 0, one row': (dict(guard=False), (3, 1, 'adv', None, False)),
}


@pytest.mark.parametrize('name', list(MUTANTS))
def test_mutant_fails(name):
    kw, case = MUTANTS[name]
    with pytest.raises(AssertionError):
        ac.check(_impl(**kw), 'cpu', *case)


# --------------------------------------------------------------------------------------------------------------- host layers
@contextlib.contextmanager
def spied_ops():
    """cpu_ops() with ops.standardize replaced by a recording stand-in (the restatement) and ops.a2c_loss -- the loss of the CPU
    path's `_loss` -- recording the advantage it is handed: -> the call lists."""
    from deeprl_network_amd import ops
    calls = dict(std=[], loss_adv=[], order=[])

    def standardize(x, eps, out=None, partial=None, moments=None):
        calls['std'].append(dict(x=x, eps=eps, out=out, partial=partial, moments=moments))
        calls['order'].append('standardize')
        y, mu, sigma = ac.expect(x, eps)
        out.copy_(torch.from_numpy(y).float())
        if moments is not None:
            moments.copy_(torch.from_numpy(np.stack([mu, sigma], axis=1)))
        return out

    with cpu_ops():
        saved = ops.standardize, ops.a2c_loss, ops.nstep_return      # (without the feature: AttributeError)
        inner_loss, inner_scan = ops.a2c_loss, ops.nstep_return

        def a2c_loss(logits, v, action, adv, R, v_coef, e_coef):
            calls['loss_adv'].append(adv)
            calls['order'].append('loss')
            return inner_loss(logits, v, action, adv, R, v_coef, e_coef)

        def nstep_return(*a, **kw):
            calls['order'].append('scan')
            return inner_scan(*a, **kw)

        ops.standardize, ops.a2c_loss, ops.nstep_return = standardize, a2c_loss, nstep_return
        try:
            yield calls
        finally:
            ops.standardize, ops.a2c_loss, ops.nstep_return = saved


def _build(agent, adv_norm=None, eps=None, gae_lambda=None, E=3, n_step=5, coop_gamma=-1):
    from deeprl_network_amd.agents import models
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    cp = cacc_config(agent=agent, n_step=n_step, reward_norm=800.0, coop_gamma=coop_gamma)
    for key, value in (('adv_norm', adv_norm), ('adv_norm_epsilon', eps), ('gae_lambda', gae_lambda)):
        if value is not None:
            cp['MODEL_CONFIG'][key] = value
    env = CpuCaccBatchEnv(cp['ENV_CONFIG'], num_envs=E)
    cls = {'ia2c_fp': models.IA2C_FP, 'ma2c_nc': models.MA2C_NC}[agent]
    np.random.seed(12)
    model = cls(env.n_s_ls, env.n_a_ls, env.neighbor_mask, env.distance_mask, env.coop_gamma, 10 ** 6, cp['MODEL_CONFIG'], seed=12,
                num_envs=E, device='cpu')
    return env, model, BatchedTrainer(env, model, Counter(10 ** 6, 10 ** 7, 10 ** 4), use_graph=False)


@pytest.mark.parametrize('agent', ['ia2c_fp', 'ma2c_nc'])
@pytest.mark.parametrize('value', [None, 'none', ' None '])
def test_default_update_never_standardises(agent, value):
    with spied_ops() as calls:
        _, model, tr = _build(agent, value)
        assert model.adv_norm == 'none'
        for _ in range(2):
            tr.run_batch()
        assert calls['std'] == [] and not hasattr(model, 'Adv_n') and not hasattr(model, 'adv_moments')
        assert len(calls['loss_adv']) == 2
        for adv in calls['loss_adv']:
            assert adv.data_ptr() == model.Adv.data_ptr()
        assert torch.isfinite(model.policy.params.flat).all()


@pytest.mark.parametrize('gae_lambda', [None, '0.9'])
@pytest.mark.parametrize('mode', ['agent', 'all'])
@pytest.mark.parametrize('agent,coop_gamma', [('ia2c_fp', -1), ('ma2c_nc', 0.9)])
def test_adv_norm_standardises_once_per_update_and_the_loss_reads_it(agent, coop_gamma, mode, gae_lambda):
    from deeprl_network_amd import ops
    with spied_ops() as calls:
        if gae_lambda is not None:          # (cpu_ops has no GAE scan: the restatement of tests/gae_checks.py stands in)
            import gae_checks as gc

            def gae(r, v, done_post, R_end, gamma, lam, alpha, dist=None, R_out=None, adv_out=None):
                calls['order'].append('scan')
                R, A = gc.gae_expect(r, v, done_post, R_end, gamma, lam, alpha, dist)
                R_out.copy_(R.float())
                adv_out.copy_(A.float())
                return R_out, adv_out
            saved_gae, ops.gae_return = ops.gae_return, gae
        try:
            _, model, tr = _build(agent, mode, '1e-6', gae_lambda, coop_gamma=coop_gamma)
            N, T, E = model.n_agent, model.n_step, model.E
            G = N if mode == 'agent' else 1
            assert model.adv_norm == mode and model.adv_norm_epsilon == 1e-6
            assert tuple(model.Adv_n.shape) == (N, T, E) and model.Adv_n.dtype == F32
            assert tuple(model.adv_moments.shape) == (G, 2) and model.adv_moments.dtype == F64
            w0 = model.policy.params.flat.clone()
            for _ in range(2):
                tr.run_batch()
        finally:
            if gae_lambda is not None:
                ops.gae_return = saved_gae
        assert len(calls['std']) == 2 and len(calls['loss_adv']) == 2                 # once per update
        assert calls['order'] == ['scan', 'standardize', 'loss'] * 2                  # directly behind the return scan
        for c in calls['std']:
            assert c['eps'] == 1e-6
            assert tuple(c['x'].shape) == (G, N * T * E // G) and c['x'].data_ptr() == model.Adv.data_ptr() and c['x'].is_contiguous()
            assert tuple(c['out'].shape) == (G, N * T * E // G) and c['out'].data_ptr() == model.Adv_n.data_ptr()
            assert c['moments'] is model.adv_moments and c['partial'] is not None and c['partial'].dtype == F64
        for adv in calls['loss_adv']:
            assert adv.data_ptr() == model.Adv_n.data_ptr() and tuple(adv.shape) == (N, T * E)
        # Adv stays raw, Adv_n is its standardised copy
        y, mu, sigma = ac.expect(model.Adv.view(G, -1), 1e-6)
        assert torch.equal(model.Adv_n.view(G, -1), torch.from_numpy(y).float())
        assert float(model.Adv.view(G, -1).double().std(dim=1, unbiased=False).sub(1.0).abs().min()) > 1e-3
        assert torch.isfinite(model.policy.params.flat).all() and not torch.equal(w0, model.policy.params.flat)


@pytest.mark.parametrize('key,value', [('adv_norm', 'batch'), ('adv_norm', 'true'), ('adv_norm', ''), ('adv_norm_epsilon', '-1e-8'),
                                       ('adv_norm_epsilon', 'nan')])
def test_bad_mode_and_bad_epsilon_are_refused(key, value):
    with cpu_ops():
        with pytest.raises(ValueError, match=key):
            _build('ia2c_fp', **({'adv_norm': value} if key == 'adv_norm' else {'adv_norm': 'agent', 'eps': value}))


def test_epsilon_is_checked_with_the_mode_off_and_zero_is_allowed():
    with cpu_ops():
        with pytest.raises(ValueError, match='adv_norm_epsilon'):
            _build('ia2c_fp', None, '-1')
        _, model, _ = _build('ia2c_fp', 'all', '0')
        assert model.adv_norm_epsilon == 0.0


def test_cli_flag_parses_and_reaches_the_run_ini(tmp_path):
    import configparser
    from deeprl_network_amd.main import apply_overrides, parse_args
    assert parse_args(['train']).adv_norm is None
    args = parse_args(['train', '--adv-norm', 'agent'])
    assert args.adv_norm == 'agent'
    with pytest.raises(SystemExit):
        parse_args(['train', '--adv-norm', 'batch'])
    cp = cacc_config(agent='ia2c_fp')
    run_ini = tmp_path / 'config.ini'
    with open(run_ini, 'w') as f:
        cp.write(f)
    other = cacc_config(agent='ia2c_fp')
    assert apply_overrides(other, args) and other['MODEL_CONFIG']['adv_norm'] == 'agent'          # (a rank that writes nothing)
    assert apply_overrides(cp, args, str(run_ini))
    back = configparser.ConfigParser()
    back.read(str(run_ini))
    assert back['MODEL_CONFIG']['adv_norm'] == 'agent'
    assert not back.has_option('MODEL_CONFIG', 'gae_lambda') and not back.has_option('MODEL_CONFIG', 'optimizer')
    assert back['MODEL_CONFIG']['batch_size'] == cp['MODEL_CONFIG']['batch_size'] and back.has_section('ENV_CONFIG')
    # no flag: the ini keeps its bytes
    before = open(run_ini, 'rb').read()
    assert not apply_overrides(cp, parse_args(['train']), str(run_ini))
    assert open(run_ini, 'rb').read() == before
    both = parse_args(['train', '--adv-norm', 'all', '--gae-lambda', '0.5'])
    apply_overrides(cp, both, str(run_ini))
    back.read(str(run_ini))
    assert back['MODEL_CONFIG']['adv_norm'] == 'all' and back['MODEL_CONFIG'].getfloat('gae_lambda') == 0.5


def test_every_reference_ini_has_no_adv_norm():
    import configparser
    import glob
    inis = sorted(glob.glob(os.path.join(ROOT, 'config', '*.ini')))
    assert inis
    for path in inis:
        cp = configparser.ConfigParser()
        cp.read(path)
        for key in ('adv_norm', 'adv_norm_epsilon'):
            assert not (cp.has_section('MODEL_CONFIG') and cp.has_option('MODEL_CONFIG', key)), (path, key)


def test_chunk_count_is_a_function_of_its_arguments():
    """>= 1, at most a few hundred, G x chunks fills a 256-CU device at both workload shapes."""
    from deeprl_network_amd import ops
    for G, rows in ((8, 245760), (1, 3072000), (25, 122880)):
        C = ops.standardize_chunks(rows, G)
        assert 1 <= C <= 512 and G * C >= 512, (G, rows, C)
    for G, rows in ((1, 1), (3, 1), (65535, 7), (0, 5), (4, 0)):
        assert 1 <= ops.standardize_chunks(rows, G) <= 512
    assert ops.standardize_chunks(40, 8) == ops.standardize_chunks(40, 8)


def test_standardize_kernel_resources():
    """Both kernels as compiled for gfx950: no scratch, no spills; the moments kernel's LDS is its three sets of four wave sums, the
    apply kernel's the 256 (count, sum, mean, M2) slots of the merge tree."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import resource_usage
    rows = {r['name']: r for r in resource_usage.usage(os.path.join(ROOT, 'deeprl_network_amd', 'csrc', 'a2c.hip'))}
    std = {n: r for n, r in rows.items() if n.startswith('standardize_')}
    assert sorted(std) == ['standardize_apply_kernel', 'standardize_moments_kernel'], sorted(rows)
    for n, g in std.items():
        assert g['ScratchSize [bytes/lane]'] == 0 and g['VGPRs Spill'] == 0 and g['SGPRs Spill'] == 0, (n, g)
    assert std['standardize_moments_kernel']['LDS Size [bytes/block]'] == 3 * 4 * 8
    assert std['standardize_apply_kernel']['LDS Size [bytes/block]'] == 256 * 4 * 8

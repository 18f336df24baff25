"""The opt-in GAE(lambda) return scan without a GPU: the float64 restatement of tests/gae_checks.py is pinned (lambda = 1 against the
reference's buffers as restated in oracle/ops_ref.nstep_return, lambda = 0 in closed form, general lambda against the brute-force sum),
check_gae is shown to fail on every mistake it is meant to see, and the host layers are followed from the ini key and the CLI flag down
to the op the update calls."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

import gae_checks as gc
import update_edge_checks as uec
from cpu_emulation import CpuCaccBatchEnv, cpu_ops
from helpers import cacc_config
from oracle import ops_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


# -------------------------------------------------------------------------------------------- the restatement is the definition
@pytest.mark.parametrize('table', uec.NSTEP_TABLES)
@pytest.mark.parametrize('alpha', uec.NSTEP_ALPHAS)
@pytest.mark.parametrize('N,E,T', uec.NSTEP_SHAPES)
def test_lambda_one_is_the_reference_nstep_return(N, E, T, alpha, table):
    r, v, done, R_end, dist = gc.gae_inputs(N, E, T, alpha, table)
    R, A = gc.gae_expect(r, v, done, R_end, gc.GAE_GAMMA, 1.0, alpha, dist)
    R_ref, A_ref = ops_ref.nstep_return(r, v, done, R_end, gc.GAE_GAMMA, alpha, dist)
    for name, got, exp in (('R', R_ref, R), ('Adv', A_ref, A)):
        ok, n_off = gc.within_one_ulp(got, exp)
        assert ok, '%s: lambda = 1 is more than one fp32 ulp off the n-step return' % name
    # and inside the spatial bound of the return scan
    gc.assert_gae_close(R_ref, A_ref, R, A, True, 'lambda=1')


@pytest.mark.parametrize('alpha,table', [(-1.0, 'line'), (0.9, 'directed')])
@pytest.mark.parametrize('N,E,T', uec.NSTEP_SHAPES)
def test_lambda_zero_is_the_one_step_td_error(N, E, T, alpha, table):
    r, v, done, R_end, dist = gc.gae_inputs(N, E, T, alpha, table)
    R, A = gc.gae_expect(r, v, done, R_end, gc.GAE_GAMMA, 0.0, alpha, dist)
    v64, keep, rho = v.double(), 1.0 - done.double(), gc.gae_rho(r, alpha, dist, N)
    nxt = torch.cat([v64[1:], R_end.double().unsqueeze(0)])                         # [T,N,E]: v[t+1], R_end behind the last step
    td = rho + (gc.GAE_GAMMA * nxt) * keep.unsqueeze(1) - v64
    assert torch.equal(A, td.permute(1, 0, 2))
    assert torch.equal(R, (td + v64).permute(1, 0, 2))


@pytest.mark.parametrize('alpha,table', [(-1.0, 'line'), (0.9, 'directed')])
@pytest.mark.parametrize('lam', [0.5, 0.95])
def test_general_lambda_is_the_brute_force_sum(lam, alpha, table):
    """A_t = sum_k (gamma lambda)^k (prod_{i<k} keep_{t+i}) delta_{t+k}, every term formed on its own."""
    N, E, T = 3, 5, 13
    r, v, done, R_end, dist = gc.gae_inputs(N, E, T, alpha, table)
    R, A = gc.gae_expect(r, v, done, R_end, gc.GAE_GAMMA, lam, alpha, dist)
    v64, keep, rho = v.double().numpy(), 1.0 - done.double().numpy(), gc.gae_rho(r, alpha, dist, N).numpy()
    Re = R_end.double().numpy()
    delta = np.zeros((T, N, E))
    for t in range(T):
        nxt = Re if t == T - 1 else v64[t + 1]
        delta[t] = rho[t] + gc.GAE_GAMMA * nxt * keep[t][None, :] - v64[t]
    brute = np.zeros((N, T, E))
    for t in range(T):
        for k in range(T - t):
            w = (gc.GAE_GAMMA * lam) ** k * np.prod(keep[t:t + k], axis=0)          # empty product = 1
            brute[:, t] += w[None, :] * delta[t + k]
    tol = 1e-12 * float(R.abs().max())
    assert float(np.abs(A.numpy() - brute).max()) <= tol
    assert float(np.abs(R.numpy() - (brute + v64.transpose(1, 0, 2))).max()) <= tol


# ------------------------------------------------------------------------------------------------- the check sees what it must
def _scan(carry_keep=True, next_keep=True, add_v=True, next_before=False, ignore_lambda=False, unreachable_one=False,
          ignore_outputs=False):
    """An implementation of gae_return as a plain loop over the steps, with one mistake switched on."""
    def f(r, v, done_post, R_end, gamma, lam, alpha, dist=None, R_out=None, adv_out=None):
        T, N, E = v.shape
        if ignore_lambda:
            lam = 1.0
        v64, keep = v.double(), 1.0 - done_post.double()
        if alpha >= 0:
            d = dist.double()
            w = torch.pow(torch.tensor(float(alpha), dtype=F64), d.clamp_min(0.0))
            w = torch.where(dist < 0, torch.full_like(w, 1.0 if unreachable_one else 0.0), w)
        nxt, A = R_end.double().clone(), torch.zeros(N, E, dtype=F64)
        R, Adv = torch.zeros(N, T, E, dtype=F64), torch.zeros(N, T, E, dtype=F64)
        for t in range(T - 1, -1, -1):
            k = keep[t].unsqueeze(0)
            rho = r[t].double().unsqueeze(0) if alpha < 0 else w @ r[t].double().t()
            if next_before:
                nxt = v64[t]
            delta = rho + gamma * nxt * (k if next_keep else 1.0) - v64[t]
            A = delta + gamma * lam * A * (k if carry_keep else 1.0)
            Adv[:, t] = A
            R[:, t] = A + v64[t] if add_v else A
            nxt = v64[t]
        R32, A32 = R.float(), Adv.float()
        if R_out is not None and not ignore_outputs:
            R_out.copy_(R32)
            adv_out.copy_(A32)
            return R_out, adv_out
        return R32, A32
    import types
    return types.SimpleNamespace(gae_return=f)


GAE_CASES = [(N, E, T, alpha, table, lam) for (N, E, T) in uec.NSTEP_SHAPES for lam in (0.0, 0.95, 1.0)
             for alpha, table in ((-1.0, 'line'), (0.9, 'line'), (0.9, 'directed'), (0.0, 'directed'), (1.0, 'directed'))]


@pytest.mark.parametrize('N,E,T,alpha,table,lam', GAE_CASES)
def test_plain_loop_passes(N, E, T, alpha, table, lam):
    gc.check_gae(_scan(), 'cpu', N, E, T, alpha, table, lam)


GAE_MUTANTS = {
    'keep missing on the A carry': (dict(carry_keep=False), (3, 5, 13, -1.0, 'line', 0.95)),
    'keep missing on next': (dict(next_keep=False), (3, 5, 13, -1.0, 'line', 0.95)),
    'R = A without + v': (dict(add_v=False), (3, 5, 13, -1.0, 'line', 0.95)),
    'next taken from v[t] before the step': (dict(next_before=True), (3, 5, 13, -1.0, 'line', 0.95)),
    'lambda ignored (plain n-step)': (dict(ignore_lambda=True), (3, 5, 13, -1.0, 'line', 0.95)),
    'dist < 0 weighted 1': (dict(unreachable_one=True), (28, 37, 21, 0.9, 'directed', 0.95)),
    'caller-supplied outputs ignored': (dict(ignore_outputs=True), (3, 5, 13, -1.0, 'line', 0.95)),
}


@pytest.mark.parametrize('name', list(GAE_MUTANTS))
def test_gae_mutant_fails(name):
    kw, case = GAE_MUTANTS[name]
    with pytest.raises(AssertionError):
        gc.check_gae(_scan(**kw), 'cpu', *case)


def test_gae_mutants_on_the_other_path_and_edge_shapes():
    """The mistakes that exist on both paths fail on the spatial one too; the masks are seen at lambda = 0 / 1 where only one of them
    acts, and at the one-step shape (2, 1, 1) nothing but R_end can be carried."""
    for kw in (dict(carry_keep=False), dict(next_keep=False), dict(add_v=False), dict(next_before=True), dict(ignore_lambda=True)):
        with pytest.raises(AssertionError):
            gc.check_gae(_scan(**kw), 'cpu', 28, 37, 21, 0.9, 'directed', 0.95)
    with pytest.raises(AssertionError):
        gc.check_gae(_scan(next_keep=False), 'cpu', 8, 300, 10, -1.0, 'line', 0.0)
    with pytest.raises(AssertionError):
        gc.check_gae(_scan(carry_keep=False), 'cpu', 8, 300, 10, -1.0, 'line', 1.0)
    with pytest.raises(AssertionError):
        gc.check_gae(_scan(unreachable_one=True), 'cpu', 2, 1, 1, 1.0, 'directed', 0.95)


# --------------------------------------------------------------------------------------------------------------- host layers
@contextlib.contextmanager
def spied_ops():
    """cpu_ops() with both return scans replaced by recording stand-ins (the n-step one is the oracle's, the GAE one the restatement
    of gae_checks): -> the two call lists."""
    from deeprl_network_amd import ops
    calls = dict(nstep=[], gae=[])

    def nstep(*a, **kw):
        calls['nstep'].append((a, kw))
        return ops_ref.nstep_return(*a, **kw)

    def gae(r, v, done_post, R_end, gamma, lam, alpha, dist=None, R_out=None, adv_out=None):
        calls['gae'].append(dict(r=r, v=v, done_post=done_post, R_end=R_end, gamma=gamma, lam=lam, alpha=alpha, dist=dist, R_out=R_out,
                                 adv_out=adv_out))
        R, A = gc.gae_expect(r, v, done_post, R_end, gamma, lam, alpha, dist)
        R_out.copy_(R.float())
        adv_out.copy_(A.float())
        return R_out, adv_out

    with cpu_ops():
        saved = ops.nstep_return, ops.gae_return               # (without the feature: AttributeError)
        ops.nstep_return, ops.gae_return = nstep, gae
        try:
            yield calls
        finally:
            ops.nstep_return, ops.gae_return = saved


def _build(agent, gae_lambda=None, E=3, n_step=5, coop_gamma=-1):
    from deeprl_network_amd.agents import models
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    cp = cacc_config(agent=agent, n_step=n_step, reward_norm=800.0, coop_gamma=coop_gamma)
    if gae_lambda is not None:
        cp['MODEL_CONFIG']['gae_lambda'] = gae_lambda
    env = CpuCaccBatchEnv(cp['ENV_CONFIG'], num_envs=E)
    cls = {'ia2c_fp': models.IA2C_FP, 'ma2c_nc': models.MA2C_NC}[agent]
    np.random.seed(12)
    model = cls(env.n_s_ls, env.n_a_ls, env.neighbor_mask, env.distance_mask, env.coop_gamma, 10 ** 6, cp['MODEL_CONFIG'], seed=12,
                num_envs=E, device='cpu')
    return env, model, BatchedTrainer(env, model, Counter(10 ** 6, 10 ** 7, 10 ** 4), use_graph=False)


@pytest.mark.parametrize('agent', ['ia2c_fp', 'ma2c_nc'])
@pytest.mark.parametrize('value', [None, '1.0', ' 1 '])
def test_default_update_calls_nstep_return_only(agent, value):
    with spied_ops() as calls:
        _, model, tr = _build(agent, value)
        assert model.gae_lambda == 1.0
        for _ in range(2):
            tr.run_batch()
        assert len(calls['nstep']) == 2 and calls['gae'] == []
        assert torch.isfinite(model.policy.params.flat).all()


@pytest.mark.parametrize('agent,coop_gamma', [('ia2c_fp', -1), ('ma2c_nc', 0.9)])
def test_gae_lambda_sends_the_update_through_gae_return(agent, coop_gamma):
    with spied_ops() as calls:
        _, model, tr = _build(agent, '0.9', coop_gamma=coop_gamma)
        assert model.gae_lambda == 0.9
        w0 = model.policy.params.flat.clone()
        for _ in range(2):
            tr.run_batch()
        assert calls['nstep'] == [] and len(calls['gae']) == 2                     # once per update
        for c in calls['gae']:
            assert c['lam'] == 0.9 and c['gamma'] == model.gamma and c['alpha'] == (coop_gamma if coop_gamma >= 0 else -1.0)
            assert c['r'] is model.buf_r and c['v'] is model.buf_v and c['done_post'] is model.buf_done_post
            assert c['R_out'] is model.R and c['adv_out'] is model.Adv and c['dist'] is model.dist_dev
            assert c['R_end'].data_ptr() == tr.R_end.data_ptr()
        assert torch.isfinite(model.policy.params.flat).all() and not torch.equal(w0, model.policy.params.flat)


@pytest.mark.parametrize('value', ['-0.1', '1.5', 'nan'])
def test_gae_lambda_outside_the_unit_interval_is_refused(value):
    with cpu_ops():
        with pytest.raises(ValueError, match='gae_lambda'):
            _build('ia2c_fp', value)


def test_cli_flag_parses_and_reaches_the_run_ini(tmp_path):
    import configparser
    from deeprl_network_amd.main import apply_overrides, parse_args
    assert parse_args(['train']).gae_lambda is None
    args = parse_args(['train', '--gae-lambda', '0.9'])
    assert args.gae_lambda == 0.9
    # the ini handling of `train`: every rank sets the key, rank 0 rewrites the run's copy of the ini with it
    cp = cacc_config(agent='ia2c_fp')
    run_ini = tmp_path / 'config.ini'
    with open(run_ini, 'w') as f:
        cp.write(f)
    other = cacc_config(agent='ia2c_fp')
    assert apply_overrides(other, args) and other['MODEL_CONFIG'].getfloat('gae_lambda') == 0.9      # (a rank that writes nothing)
    assert apply_overrides(cp, args, str(run_ini))
    back = configparser.ConfigParser()
    back.read(str(run_ini))
    assert back['MODEL_CONFIG'].getfloat('gae_lambda') == 0.9
    assert not back.has_option('MODEL_CONFIG', 'lstm_precision')
    assert back['MODEL_CONFIG']['batch_size'] == cp['MODEL_CONFIG']['batch_size'] and back.has_section('ENV_CONFIG')
    # no flag: the ini keeps its bytes
    before = open(run_ini).read()
    assert not apply_overrides(cp, parse_args(['train']), str(run_ini))
    assert open(run_ini).read() == before
    both = parse_args(['train', '--gae-lambda', '0.5', '--lstm-precision', 'bf16x3'])
    apply_overrides(cp, both, str(run_ini))
    back.read(str(run_ini))
    assert back['MODEL_CONFIG'].getfloat('gae_lambda') == 0.5 and back['MODEL_CONFIG']['lstm_precision'] == 'bf16x3'


def test_every_reference_ini_has_no_gae_lambda():
    import configparser
    import glob
    inis = sorted(glob.glob(os.path.join(ROOT, 'config', '*.ini')))
    assert inis
    for path in inis:
        cp = configparser.ConfigParser()
        cp.read(path)
        assert not (cp.has_section('MODEL_CONFIG') and cp.has_option('MODEL_CONFIG', 'gae_lambda')), path


def test_gae_kernel_resources():
    """Both instantiations of gae_kernel as compiled for gfx950: the ten steps' operands live in registers -- no scratch, no spill;
    the 64 x 64 float64 weight table is the spatial one's only LDS, the global one has none."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import resource_usage
    rows = {r['name']: r for r in resource_usage.usage(os.path.join(ROOT, 'deeprl_network_amd', 'csrc', 'a2c.hip'))}
    gae = {n: r for n, r in rows.items() if n.startswith('gae_kernel<')}
    assert sorted(gae) == ['gae_kernel<false>', 'gae_kernel<true>'], sorted(rows)
    for n, g in gae.items():
        assert g['ScratchSize [bytes/lane]'] == 0 and g['VGPRs Spill'] == 0 and g['SGPRs Spill'] == 0, (n, g)
        assert g['LDS Size [bytes/block]'] == (64 * 64 * 8 if n == 'gae_kernel<true>' else 0), (n, g)

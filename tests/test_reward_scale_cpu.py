"""Opt-in running return-based reward scaling (MODEL_CONFIG reward_scale = return), the CPU side: the float64 restatement of
tests/reward_scale_checks.py against exact rational arithmetic, the checker against a catalogue of wrong implementations, and the
host layers (ini keys, the flag, the one call per update, checkpoints, the key-absent path)."""
import configparser
import contextlib
import glob
import logging
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import reward_scale_checks as rc
from cpu_emulation import CpuCaccBatchEnv, cpu_ops
from helpers import cacc_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64


# ------------------------------------------------------------------------------------------- the restatement against exact arithmetic
def _exact(calls, E, N, gamma, eps):
    """The definition in fractions.Fraction (gamma, eps and the fp32 rewards are exact rationals): per call the exact carry, n, mean,
    variance and -- the root taken of the correctly rounded variance, 2e-16 -- sigma and the unrounded r_out."""
    S = E * max(N, 1)
    g, carry, seen, out = Fraction(gamma), [Fraction(0)] * S, [], []
    for r, d in calls:
        T = r.shape[0]
        for t in range(T):
            for s in range(S):
                carry[s] = g * carry[s] + Fraction(float(r[t, s]))
                seen.append(carry[s])
                if d[t, s // max(N, 1)]:
                    carry[s] = Fraction(0)
        n = len(seen)
        mean = sum(seen) / n
        var = sum((x - mean) ** 2 for x in seen) / n
        sigma = math.sqrt(var)
        scale = Fraction(1) / (Fraction(sigma) + Fraction(eps)) if var > 0 else Fraction(1)
        out.append(dict(carry=[float(c) for c in carry], n=n, mean=float(mean), sigma=sigma if var > 0 else 0.0,
                        r_out=np.array([[float(Fraction(float(r[t, s])) * scale) for s in range(S)] for t in range(T)])))
    return out


@pytest.mark.parametrize('pattern', ['none', 'random'])
@pytest.mark.parametrize('kind', rc.KINDS)
@pytest.mark.parametrize('E,N,T', [(4, 0, 4), (2, 4, 8), (1, 0, 1), (1, 2, 3)])
def test_restatement_sits_within_a_tenth_of_the_bound_of_exact_arithmetic(E, N, T, kind, pattern):
    S = E * max(N, 1)
    assert T * S <= 64
    calls = [(rc.rewards(T, S, kind, k), rc.dones(T, E, pattern, k)) for k in range(3)]
    ref = rc.Restatement(E, N, rc.GAMMA, rc.EPS, 0.0)
    for k, ((r, d), ex) in enumerate(zip(calls, _exact(calls, E, N, rc.GAMMA, rc.EPS))):
        got = ref.call(r, d)
        assert got['n'] == ex['n'] == (k + 1) * T * S
        for name in ('carry', 'mean', 'sigma', 'r_out'):
            g, e = np.asarray(got[name], dtype=np.float64), np.asarray(ex[name], dtype=np.float64)
            rel = np.abs(g - e) / np.where(e != 0, np.abs(e), 1.0)
            # (the mean of centred data is ill-conditioned by mean|x| / |mean| in any float64 arithmetic: a few units here)
            assert float(rel.max()) <= 0.1 * rc.MOMENT_RTOL, (name, k, float(rel.max()))
        if kind == 'zero':
            assert got['sigma'] == 0.0 and not got['r_out'].any()


def test_restatement_edges():
    """sigma = 0 gives scale 1 (one sample; all-zero rewards); the moments include the current batch from the first call on; the mean
    is not subtracted; one pooled scale; the clamp comes last and is the fp32 clip."""
    one = rc.Restatement(1, 0).call(np.array([[3.0]], dtype=np.float32), np.zeros((1, 1), dtype=np.uint8))
    assert one['sigma'] == 0.0 and one['r_out'][0, 0] == 3.0 and one['n'] == 1 and one['mean'] == 3.0
    ref = rc.Restatement(1, 0, gamma=0.5, eps=0.0)
    a = ref.call(np.array([[1.0], [1.0]], dtype=np.float32), np.array([[0], [1]], dtype=np.uint8))
    assert a['n'] == 2 and a['mean'] == 1.25 and a['sigma'] == 0.25 and a['carry'][0] == 0.0        # samples 1, 1.5; reset after
    assert np.array_equal(a['r_out'], [[4.0], [4.0]])                                               # raw / sigma, mean kept
    b = ref.call(np.array([[2.0]], dtype=np.float32), np.zeros((1, 1), dtype=np.uint8))
    assert b['n'] == 3 and b['carry'][0] == 2.0 and b['mean'] == 1.5                                # samples 1, 1.5, 2
    assert abs(b['sigma'] - math.sqrt(1.0 / 6.0)) < 1e-15
    c = rc.Restatement(1, 0, gamma=0.5, eps=0.0, clip=0.3).call(np.array([[1.0], [-1.0]], dtype=np.float32), np.zeros((2, 1), dtype=np.uint8))
    assert np.array_equal(c['r_out'], np.array([[1.0], [-1.0]]) * float(np.float32(0.3)))


# ------------------------------------------------------------------------------------------- the checker rejects wrong implementations
class _Rounded:
    """A Restatement (or a wrong variant of it) as an implementation under test: r_out rounded to fp32 once."""

    def __init__(self, E, N, gamma, eps, clip, variant=None, reward_norm=0.0):
        self.inner = rc.Restatement(E, N, gamma, eps, clip, reward_norm=reward_norm, variant=variant)

    def call(self, r, d):
        got = self.inner.call(r, d)
        got['r_out'] = got['r_out'].astype(np.float32)
        return got


SMALL = [dict(E=3, N=2, T=4, kind='plain', pattern='random'),
         dict(E=3, N=2, T=4, kind='plain', pattern='random', clip=0.5),
         dict(E=3, N=0, T=5, kind='plain', pattern='last'),
         dict(E=2, N=0, T=3, kind='tiny', pattern='none'),
         dict(E=1, N=0, T=1, kind='plain', pattern='none'),
         dict(E=2, N=3, T=4, kind='offset', pattern='first'),
         dict(E=2, N=0, T=2, kind='const', pattern='none')]


@pytest.mark.parametrize('case', SMALL, ids=lambda c: '-'.join(str(v) for v in c.values()))
def test_the_restatement_passes_the_check(case):
    assert rc.run_case(lambda *a: _Rounded(*a), **case) <= 1.0


@pytest.mark.parametrize('variant', rc.VARIANTS)
def test_wrong_implementation_fails(variant):
    failed = []
    for case in SMALL:
        try:
            rc.run_case(lambda *a: _Rounded(*a, variant=variant, reward_norm=10.0), **case)
        except AssertionError:
            failed.append(case)
    assert failed, '%s passes every small case: the check is not sharp' % variant


# --------------------------------------------------------------------------------------------------------------- host layers
@contextlib.contextmanager
def spied_ops(forbid=False):
    """cpu_ops() with ops.reward_scale replaced by the restatement (one Restatement per `state` tensor), recording its calls; with
    `forbid` the stand-in raises instead."""
    from deeprl_network_amd import ops
    calls, refs = [], {}

    def reward_scale(r_raw, done_post, gamma, eps, clip, carry, state, partial, out):
        if forbid:
            raise AssertionError('ops.reward_scale called with the key absent')
        T, E = done_post.shape
        N = 0 if r_raw.dim() == 2 else r_raw.shape[2]
        ref = refs.setdefault(state.data_ptr(), rc.Restatement(E, N, gamma, eps, clip))
        got = ref.call(r_raw.numpy().reshape(T, -1), done_post.numpy())
        calls.append(dict(r_raw=r_raw.clone(), done=done_post.clone(), gamma=gamma, eps=eps, clip=clip, carry=carry, state=state,
                          partial=partial, out=out, exp=got))
        out.copy_(torch.from_numpy(got['r_out'].astype(np.float32)).view(out.shape))
        carry.copy_(torch.from_numpy(got['carry']))
        state[0], state[5], state[6] = got['n'], got['mean'], got['sigma']
        return out

    with cpu_ops():
        saved = ops.reward_scale                                       # (without the feature: AttributeError)
        ops.reward_scale = reward_scale
        try:
            yield calls
        finally:
            ops.reward_scale = saved


def _build(agent='ia2c_fp', reward_scale=None, eps=None, E=3, n_step=5, coop_gamma=-1, reward_clip=None, trainer=True):
    from deeprl_network_amd.agents import models
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    cp = cacc_config(agent=agent, n_step=n_step, reward_norm=800.0, coop_gamma=coop_gamma)
    for key, value in (('reward_scale', reward_scale), ('reward_scale_epsilon', eps), ('reward_clip', reward_clip)):
        if value is not None:
            cp['MODEL_CONFIG'][key] = value
    env = CpuCaccBatchEnv(cp['ENV_CONFIG'], num_envs=E)
    cls = {'ia2c_fp': models.IA2C_FP, 'ma2c_nc': models.MA2C_NC}[agent]
    np.random.seed(12)
    model = cls(env.n_s_ls, env.n_a_ls, env.neighbor_mask, env.distance_mask, env.coop_gamma, 10 ** 6, cp['MODEL_CONFIG'], seed=12,
                num_envs=E, device='cpu')
    return env, model, (BatchedTrainer(env, model, Counter(10 ** 6, 10 ** 7, 10 ** 4), use_graph=False) if trainer else None)


NEW_ATTRS = ('rs_carry', 'rs_state', '_rs_partial', '_rs_raw', '_rs_pending')


@pytest.mark.parametrize('agent', ['ia2c_fp', 'ma2c_nc'])
@pytest.mark.parametrize('value', [None, 'none', ' None '])
def test_key_absent_allocates_nothing_and_never_calls(agent, value):
    with spied_ops(forbid=True):
        _, model, tr = _build(agent, value)
        assert model.reward_scale == 'none' and model.reward_scale_std is None
        for _ in range(2):
            tr.run_batch()
        for name in NEW_ATTRS:
            assert not hasattr(model, name), name
        assert tr._reward_scale_tensors() == []          # (what joins _shadow_tensors() / _state_tensors(): nothing)
        # buf_r = raw / reward_norm, clamped, as before
        exp = tr.buf_rraw / model.reward_norm
        if model.reward_clip > 0:
            exp = exp.clamp(-model.reward_clip, model.reward_clip)
        assert torch.equal(model.buf_r, exp)
        assert torch.isfinite(model.policy.params.flat).all()


@pytest.mark.parametrize('agent,coop_gamma', [('ia2c_fp', -1), ('ma2c_nc', 0.9)])
def test_key_on_makes_the_one_call_per_update_in_place_of_reward_norm(agent, coop_gamma, caplog):
    with spied_ops() as calls:
        with caplog.at_level(logging.INFO):
            _, model, tr = _build(agent, ' Return ', '1e-6', coop_gamma=coop_gamma, reward_clip='2.0')
        assert sum('reward_norm' in r.getMessage() and 'not applied' in r.getMessage() for r in caplog.records) == 1
        N, T, E = model.n_agent, model.n_step, model.E
        S = E * N if coop_gamma >= 0 else E
        assert model.reward_scale == 'return' and model.reward_scale_epsilon == 1e-6
        assert tuple(model.rs_carry.shape) == (S,) and model.rs_carry.dtype == F64 and not model.rs_carry.any()
        assert model.rs_state.dtype == F64 and not model.rs_state.any() and model._rs_partial.dtype == F64
        joined = tr._reward_scale_tensors()              # (what joins _shadow_tensors() / _state_tensors())
        assert len(joined) == 2 and joined[0] is model.rs_carry and joined[1] is model.rs_state
        w0 = model.policy.params.flat.clone()
        for k in range(3):
            tr.run_batch()
            assert len(calls) == k + 1
            c = calls[-1]
            assert c['out'].data_ptr() == model.buf_r.data_ptr() and c['carry'] is model.rs_carry and c['state'] is model.rs_state
            assert c['partial'] is model._rs_partial and c['gamma'] == model.gamma and c['eps'] == 1e-6 and c['clip'] == 2.0
            assert torch.equal(c['r_raw'], tr.buf_rraw) and torch.equal(c['done'], model.buf_done_post)
            assert tuple(c['r_raw'].shape) == ((T, E, N) if coop_gamma >= 0 else (T, E))
            # buf_r is the raw reward over the running std, clamped: reward_norm (800) plays no part
            assert torch.equal(model.buf_r, torch.from_numpy(c['exp']['r_out'].astype(np.float32)).view(model.buf_r.shape))
            assert model.reward_scale_std == c['exp']['sigma'] > 0
        assert calls[-1]['exp']['n'] == 3 * T * S
        assert torch.isfinite(model.policy.params.flat).all() and not torch.equal(w0, model.policy.params.flat)


def test_record_per_step_makes_the_same_one_call_before_the_scan():
    """The one-replica path: `record` keeps the raw rewards, the update scales the batch once -- the bits of load_rewards."""
    with spied_ops() as calls:
        _, a, _ = _build('ia2c_fp', 'return', E=1, n_step=4, trainer=False)
        _, b, _ = _build('ia2c_fp', 'return', E=1, n_step=4, trainer=False)
        for k in range(2):
            raw = torch.from_numpy(rc.rewards(4, 1, 'plain', k))
            done = torch.from_numpy(rc.dones(4, 1, 'last', k))
            for t in range(4):
                a.record(raw[t], done[t])
            assert len(calls) == 2 * k and a._rs_pending
            a.update_grads(torch.zeros(a.n_agent, 1))
            assert len(calls) == 2 * k + 1 and not a._rs_pending
            a.update_end()
            b.buf_done_post.copy_(done)
            b.load_rewards(raw)
            assert len(calls) == 2 * k + 2
            assert torch.equal(a.buf_r, b.buf_r) and torch.equal(a.rs_carry, b.rs_carry) and torch.equal(a.rs_state, b.rs_state)
            assert torch.equal(calls[-2]['r_raw'], calls[-1]['r_raw']) and torch.equal(calls[-2]['done'], calls[-1]['done'])
            b.t = 0


@pytest.mark.parametrize('key,value', [('reward_scale', 'std'), ('reward_scale', 'true'), ('reward_scale', ''),
                                       ('reward_scale_epsilon', '-1e-8'), ('reward_scale_epsilon', 'nan')])
def test_bad_mode_and_bad_epsilon_are_refused(key, value):
    with cpu_ops():
        with pytest.raises(ValueError, match=key):
            _build(**({'reward_scale': value} if key == 'reward_scale' else {'reward_scale': 'return', 'eps': value}), trainer=False)
        with pytest.raises(ValueError, match='reward_scale_epsilon'):
            _build(reward_scale=None, eps='-1', trainer=False)
        _, model, _ = _build(reward_scale='return', eps='0', trainer=False)
        assert model.reward_scale_epsilon == 0.0


def test_cli_flag_parses_and_reaches_the_run_ini(tmp_path):
    from deeprl_network_amd.main import apply_overrides, parse_args
    assert parse_args(['train']).reward_scale is None
    args = parse_args(['train', '--reward-scale', 'return'])
    assert args.reward_scale == 'return'
    with pytest.raises(SystemExit):
        parse_args(['train', '--reward-scale', 'std'])
    cp = cacc_config(agent='ia2c_fp')
    run_ini = tmp_path / 'config.ini'
    with open(run_ini, 'w') as f:
        cp.write(f)
    other = cacc_config(agent='ia2c_fp')
    assert apply_overrides(other, args) and other['MODEL_CONFIG']['reward_scale'] == 'return'
    assert apply_overrides(cp, args, str(run_ini))
    back = configparser.ConfigParser()
    back.read(str(run_ini))
    assert back['MODEL_CONFIG']['reward_scale'] == 'return'
    assert not back.has_option('MODEL_CONFIG', 'adv_norm') and not back.has_option('MODEL_CONFIG', 'optimizer')
    assert back['MODEL_CONFIG']['reward_norm'] == cp['MODEL_CONFIG']['reward_norm'] and back.has_section('ENV_CONFIG')
    before = open(run_ini, 'rb').read()
    assert not apply_overrides(cp, parse_args(['train']), str(run_ini))          # no flag: the ini keeps its bytes
    assert open(run_ini, 'rb').read() == before
    both = parse_args(['train', '--reward-scale', 'none', '--adv-norm', 'agent'])
    apply_overrides(cp, both, str(run_ini))
    back.read(str(run_ini))
    assert back['MODEL_CONFIG']['reward_scale'] == 'none' and back['MODEL_CONFIG']['adv_norm'] == 'agent'


def test_every_reference_ini_has_no_reward_scale():
    inis = sorted(glob.glob(os.path.join(ROOT, 'config', '*.ini')))
    assert inis
    for path in inis:
        cp = configparser.ConfigParser()
        cp.read(path)
        for key in ('reward_scale', 'reward_scale_epsilon'):
            assert not (cp.has_section('MODEL_CONFIG') and cp.has_option('MODEL_CONFIG', key)), (path, key)


def _fill(model):
    model.rs_state.copy_(torch.arange(1, model.rs_state.numel() + 1, dtype=F64) / 7)
    model.rs_carry.copy_(torch.arange(model.rs_carry.numel(), dtype=F64) / 3 - 1)


def test_checkpoint_round_trip_and_the_three_mismatches(tmp_path, caplog):
    with cpu_ops():
        d = str(tmp_path) + os.sep
        _, on, _ = _build(reward_scale='return', trainer=False)
        _fill(on)
        on.save(d, 100)
        blob = torch.load(d + 'checkpoint-100.pt', weights_only=True)
        assert blob['reward_scale'] == 'return' and blob['reward_scale_state'].dtype == F64 and blob['reward_scale_carry'].dtype == F64
        # the round trip: bits
        _, fresh, _ = _build(reward_scale='return', trainer=False)
        with caplog.at_level(logging.WARNING):
            assert fresh.load(d, 100)
        assert not [r for r in caplog.records if r.levelno >= logging.WARNING]
        assert torch.equal(fresh.rs_state, on.rs_state) and torch.equal(fresh.rs_carry, on.rs_carry)
        assert torch.equal(fresh.policy.params.flat, on.policy.params.flat)
        # (1) written with the key on, loaded with the key absent: variables, a warning, no new attribute
        _, off, _ = _build(trainer=False)
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            assert off.load(d, 100)
        assert sum('reward_scale' in r.getMessage() for r in caplog.records) == 1 and not hasattr(off, 'rs_state')
        assert torch.equal(off.policy.params.flat, on.policy.params.flat)
        # (2) a blob without the keys (key absent, or an earlier version) into a model with the key on: state left fresh, a warning
        off.policy.params.flat.mul_(0.5)
        off.save(d, 200)
        assert not any(k.startswith('reward_scale') for k in torch.load(d + 'checkpoint-200.pt', weights_only=True))
        _, on2, _ = _build(reward_scale='return', trainer=False)
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            assert on2.load(d, 200)
        assert sum('left fresh' in r.getMessage() for r in caplog.records) == 1
        assert not on2.rs_state.any() and not on2.rs_carry.any() and torch.equal(on2.policy.params.flat, off.policy.params.flat)
        # (3) another num_envs: the moments load, the carry stays fresh, a warning
        _, wide, _ = _build(reward_scale='return', E=5, trainer=False)
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            assert wide.load(d, 100)
        assert sum('num_envs' in r.getMessage() for r in caplog.records) == 1
        assert torch.equal(wide.rs_state, on.rs_state) and not wide.rs_carry.any()
        # the key-absent checkpoint keeps the keys of before
        assert sorted(torch.load(d + 'checkpoint-200.pt', weights_only=True)) == sorted(
            ['variables', 'optimizer', 'rmsprop_ms', 'name', 'global_step', 'lr_n'])


def test_chunk_count_is_a_function_of_the_streams_alone():
    from deeprl_network_amd import ops
    for S, C in ((1, 1), (256, 1), (257, 2), (4096, 16), (25600, 100), (131072, 512), (131073, 512), (10 ** 9, 512), (0, 1)):
        assert ops.reward_scale_chunks(S) == C, S


def test_reward_scale_kernel_resources():
    """The three kernels as compiled for gfx950: no scratch, no spills; LDS = the four wave triples of the scan, the 256 slots of the
    merge tree, none in the apply pass."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import resource_usage
    rows = {r['name']: r for r in resource_usage.usage(os.path.join(ROOT, 'deeprl_network_amd', 'csrc', 'a2c.hip'))}
    rs = {n: r for n, r in rows.items() if n.startswith('reward_scale_')}
    assert sorted(rs) == ['reward_scale_apply_kernel', 'reward_scale_merge_kernel', 'reward_scale_scan_kernel'], sorted(rows)
    for n, g in rs.items():
        assert g['ScratchSize [bytes/lane]'] == 0 and g['VGPRs Spill'] == 0 and g['SGPRs Spill'] == 0, (n, g)
    assert rs['reward_scale_scan_kernel']['LDS Size [bytes/block]'] == 4 * 4 * 8
    assert rs['reward_scale_merge_kernel']['LDS Size [bytes/block]'] == 256 * 4 * 8
    assert rs['reward_scale_apply_kernel']['LDS Size [bytes/block]'] == 0


def test_reward_scale_std_scalar_is_written_with_the_train_reward_row():
    """Where a train_reward row is logged and a writer exists: `train/reward_scale_std` with the key on, the tags of before without."""
    import types
    from deeprl_network_amd.utils import Trainer

    class Writer:
        def __init__(self):
            self.rows = []

        def add_scalar(self, tag, value, step):
            self.rows.append((tag, value, step))

        def flush(self):
            pass
    for model, tags in ((types.SimpleNamespace(reward_scale='return', reward_scale_std=2.5), ['train_reward', 'train/reward_scale_std']),
                        (types.SimpleNamespace(reward_scale='none', reward_scale_std=None), ['train_reward']),
                        (types.SimpleNamespace(), ['train_reward'])):
        me = types.SimpleNamespace(data=[], agent='ia2c_fp', summary_writer=Writer(), model=model)
        Trainer._record(me, 60, -3.0, 1.0)
        assert [r[0] for r in me.summary_writer.rows] == tags and me.summary_writer.rows[-1][2] == 60
        assert list(me.data[0]) == ['agent', 'step', 'test_id', 'avg_reward', 'std_reward']          # the CSV columns of before
    assert me.summary_writer.rows == [('train_reward', -3.0, 60)]

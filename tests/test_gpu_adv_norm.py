"""The opt-in per-batch advantage standardisation on the device (csrc/a2c.hip: standardize_moments_kernel, standardize_apply_kernel,
nmarl_standardize) and in the engine: the kernels against the float64 restatement of tests/adv_norm_checks.py at the smallest shapes
where they can go wrong (fewer rows than chunks, the wave and block edges, odd rows on a dense pitch, rows around a multiple of the
chunk count, the engine's group shapes, many chunks of many rows), with dense, padded and in-place buffers and every kind of data;
determinism, the ABI's refusals, and MODEL_CONFIG adv_norm through BatchedTrainer (eager and captured) and the one-replica path."""
import os
import sys

import numpy as np
import pytest
import torch

import adv_norm_checks as ac
import gae_checks as gc
from helpers import GOLDEN, cacc_config, drive_scripted, load_npz

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

SHAPES = [(1, 1), (1, 2), (3, 1),                       # fewer rows than chunks: empty chunks
          (2, 63), (2, 64), (2, 65),                    # the wave edge
          (3, 255), (3, 256), (3, 257),                 # the block edge
          (5, 1023),                                    # odd rows on a dense pitch: group bases off 16 bytes
          (8, 40), (25, 600), (32, 12289), (1, 100003)]
FORMS = ['dense', 'padded', 'inplace']


def _run(G, rows, form, kind):
    from deeprl_network_amd import ops
    return ac.check(ops, 'cuda', G, rows, kind, (rows + 3, rows + 5) if form == 'padded' else None, form == 'inplace')


# ------------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize('kind', ac.KINDS)
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('G,rows', SHAPES)
def test_standardize_equals_the_restatement(G, rows, form, kind):
    _run(G, rows, form, kind)


@pytest.mark.parametrize('kind', ac.KINDS)
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('around', [-1, 0, 1])
def test_rows_around_a_multiple_of_the_chunk_count(around, form, kind):
    """rows = 3 C - 1, 3 C, 3 C + 1 for the C of G = 2: chunks of 3 rows with a short last one, all full, chunks of 4 with the last
    quarter of them empty."""
    from deeprl_network_amd import ops
    C = ops.standardize_chunks(1000, 2)
    assert C > 1 and ops.standardize_chunks(3 * C + around, 2) == C
    _run(2, 3 * C + around, form, kind)


@pytest.mark.parametrize('form', ['padded', 'inplace'])
def test_padded_pitch_in_place_and_equal_padded_pitches(form):
    """The two forms the three above leave out: in place on a padded pitch, and x and out on the same padded pitch (the 16-byte path
    with the group bases off 16 bytes and a tail to keep)."""
    from deeprl_network_amd import ops
    for G, rows in ((5, 1023), (3, 257), (32, 12289)):
        for kind in ('adv', 'offset'):
            ac.check(ops, 'cuda', G, rows, kind, (rows + 6, rows + 6), form == 'inplace')


def test_chunk_count():
    from deeprl_network_amd import _lib
    f = _lib.lib.nmarl_standardize_chunks
    for G, rows in ((8, 245760), (1, 3072000), (25, 122880)):          # G x chunks fills the device at the workload shapes
        assert 1 <= f(rows, G) <= 512 and G * f(rows, G) >= torch.cuda.get_device_properties(0).multi_processor_count
    for G, rows in ((1, 1), (3, 1), (65535, 7), (0, 5), (-1, 5), (4, 0)):
        assert 1 <= f(rows, G) <= 512


@pytest.mark.parametrize('G,rows', [(32, 12289), (1, 100003), (3, 1)])
def test_two_calls_give_the_same_bits(G, rows):
    from deeprl_network_amd import ops
    x = ac.inputs(G, rows, 'adv').cuda()
    m1, m2 = torch.zeros(G, 2, dtype=torch.float64, device='cuda'), torch.zeros(G, 2, dtype=torch.float64, device='cuda')
    y1 = ops.standardize(x, ac.EPS, moments=m1)
    y2 = ops.standardize(x, ac.EPS, moments=m2)
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32)) and torch.equal(m1.view(torch.int64), m2.view(torch.int64))
    # and in place, from a buffer at another address
    z = x.clone()
    assert ops.standardize(z, ac.EPS, out=z) is z and torch.equal(z.view(torch.int32), y1.view(torch.int32))


def test_abi_refusals_write_nothing():
    """rows 0, G -1, G 65536, a null x / y / partial, a pitch below rows, eps -1, eps NaN: NMARL_EINVAL and y, partial and moments keep
    their bits; G = 0: OK without a launch."""
    from deeprl_network_amd import _lib
    lib, ptr = _lib.lib, _lib.ptr
    G, rows = 3, 70
    C = lib.nmarl_standardize_chunks(rows, G)
    x = ac.inputs(G, rows, 'adv').cuda()
    y = torch.full((G, rows), ac.SENTINEL, device='cuda')
    partial = torch.full((G, C, 3), ac.SENTINEL, dtype=torch.float64, device='cuda')
    moments = torch.full((G, 2), ac.SENTINEL, dtype=torch.float64, device='cuda')
    px, py, pp, pm = ptr(x), ptr(y), ptr(partial), ptr(moments)
    nan = float('nan')
    cases = {'rows 0': (G, 0, px, rows, py, rows, 1e-8, pp, pm), 'rows -1': (G, -1, px, rows, py, rows, 1e-8, pp, pm),
             'G -1': (-1, rows, px, rows, py, rows, 1e-8, pp, pm), 'G 65536': (65536, rows, px, rows, py, rows, 1e-8, pp, pm),
             'null x': (G, rows, None, rows, py, rows, 1e-8, pp, pm), 'null y': (G, rows, px, rows, None, rows, 1e-8, pp, pm),
             'null partial': (G, rows, px, rows, py, rows, 1e-8, None, pm),
             'x pitch below rows': (G, rows, px, rows - 1, py, rows, 1e-8, pp, pm),
             'y pitch below rows': (G, rows, px, rows, py, rows - 1, 1e-8, pp, pm),
             'eps -1': (G, rows, px, rows, py, rows, -1.0, pp, pm), 'eps NaN': (G, rows, px, rows, py, rows, nan, pp, pm)}
    for name, a in cases.items():
        assert lib.nmarl_standardize(*a, _lib.stream()) == -1, name            # NMARL_EINVAL
    torch.cuda.synchronize()
    for t in (y, partial, moments):
        assert bool((t == ac.SENTINEL).all())
    assert lib.nmarl_standardize(0, rows, px, rows, py, rows, 1e-8, pp, pm, _lib.stream()) == 0
    assert lib.nmarl_standardize(0, rows, None, rows, None, rows, 1e-8, None, None, _lib.stream()) == 0
    torch.cuda.synchronize()
    for t in (y, partial, moments):
        assert bool((t == ac.SENTINEL).all())
    # moments may be NULL, eps may be 0
    assert lib.nmarl_standardize(G, rows, px, rows, py, rows, 0.0, pp, None, _lib.stream()) == 0
    torch.cuda.synchronize()
    assert bool((moments == ac.SENTINEL).all())
    ac.assert_standardized(y, None, x, 0.0, 'eps = 0, no moments')


# ------------------------------------------------------------------------------------------------------------------ the engine
E_ENGINE, T_ENGINE = 8, 5
ENGINE_CASES = [('ia2c_fp', 'catchup', -1), ('ma2c_nc', 'slowdown', 0.9)]


def _build(agent, use_graph, adv_norm, scenario='catchup', coop_gamma=-1, extra=None, **trainer_kw):
    from deeprl_network_amd.envs import make_batch_env
    from deeprl_network_amd.main import init_agent
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    cp = cacc_config(agent=agent, scenario=scenario, n_step=T_ENGINE, coop_gamma=coop_gamma,
                     reward_norm=800.0 if agent.startswith('ia2c') else 5000.0)
    if adv_norm is not None:
        cp['MODEL_CONFIG']['adv_norm'] = adv_norm
    for k, v in (extra or {}).items():
        cp['MODEL_CONFIG'][k] = v
    env = make_batch_env(cp['ENV_CONFIG'], num_envs=E_ENGINE)
    np.random.seed(12)
    model = init_agent(env, cp['MODEL_CONFIG'], 10 ** 9, 12, num_envs=E_ENGINE)
    return env, model, BatchedTrainer(env, model, Counter(10 ** 12, 10 ** 12, 10 ** 12), use_graph=use_graph, **trainer_kw)


def _assert_model_advantages(model, R_end, lam=1.0):
    """model.Adv / model.R == the scan restatement of the model's own rollout buffers (raw, as without the key), and model.Adv_n,
    model.adv_moments == the standardisation restatement of model.Adv."""
    alpha = model.coop_gamma if model.coop_gamma >= 0 else -1.0
    exp_R, exp_A = gc.gae_expect(model.buf_r, model.buf_v, model.buf_done_post, R_end, model.gamma, lam, alpha, model.dist_dev)
    gc.assert_gae_close(model.R, model.Adv, exp_R, exp_A, alpha >= 0, '%s raw' % model.name)
    G = model.n_agent if model.adv_norm == 'agent' else 1
    assert tuple(model.Adv_n.shape) == tuple(model.Adv.shape) and tuple(model.adv_moments.shape) == (G, 2)
    ac.assert_standardized(model.Adv_n.view(G, -1), model.adv_moments, model.Adv.view(G, -1), model.adv_norm_epsilon,
                           '%s %s' % (model.name, model.adv_norm))
    assert float(model.Adv_n.abs().max()) > 0 and not torch.equal(model.Adv_n, model.Adv)


@pytest.mark.parametrize('mode', ['agent', 'all'])
@pytest.mark.parametrize('agent,scenario,coop_gamma', ENGINE_CASES)
def test_adv_n_is_the_restatement_of_the_models_adv(agent, scenario, coop_gamma, mode):
    env, model, tr = _build(agent, False, mode, scenario, coop_gamma)
    assert model.adv_norm == mode and model.adv_norm_epsilon == 1e-8
    tr.run_batch()
    torch.cuda.synchronize()
    _assert_model_advantages(model, tr.R_end)


@pytest.mark.parametrize('mode', ['agent', 'all'])
@pytest.mark.parametrize('agent,scenario,coop_gamma', ENGINE_CASES)
def test_captured_update_equals_eager_with_adv_norm(agent, scenario, coop_gamma, mode):
    import graph_nodes as G
    runs = []
    for use_graph in (True, False):
        env, model, tr = _build(agent, use_graph, mode, scenario, coop_gamma, **(dict(keep_graphs=True) if use_graph else {}))
        w0 = model.policy.params.flat.clone()
        for _ in range(3):
            tr.run_batch()
        torch.cuda.synchronize()
        assert tr.handoff_fallbacks == 0
        if use_graph:
            assert tr._upd is not None and tr.update_capture_error is None
            c = G.census(tr._upd['grads'])
            assert c.get('kernel', 0) > 0 and set(c) == {'kernel'}, c
        _assert_model_advantages(model, tr.R_end)
        runs.append((model.policy.params.flat.clone(), model.Adv_n.clone(), model.adv_moments.clone()))
        assert torch.isfinite(runs[-1][0]).all() and not torch.equal(runs[-1][0], w0)
        del env, model, tr
    for a, b in zip(*runs):
        assert torch.equal(a, b), 'captured update with adv_norm differs from the eager one'


@pytest.mark.parametrize('agent,scenario,coop_gamma', ENGINE_CASES)
def test_explicit_none_is_the_untouched_default_path(agent, scenario, coop_gamma, monkeypatch):
    from deeprl_network_amd import ops
    n_std = []
    inner = ops.standardize
    monkeypatch.setattr(ops, 'standardize', lambda *a, **kw: n_std.append(1) or inner(*a, **kw))
    runs = []
    for value in ('none', None, 'agent'):
        env, model, tr = _build(agent, True, value, scenario, coop_gamma)
        assert model.adv_norm == (value or 'none') and hasattr(model, 'Adv_n') == (value == 'agent')
        for _ in range(2):
            tr.run_batch()
        torch.cuda.synchronize()
        if value != 'agent':
            assert not n_std
        runs.append((model.policy.params.flat.clone(), model.R.clone(), model.Adv.clone()))
        del env, model, tr
    assert n_std
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    assert not torch.equal(runs[0][0], runs[2][0]), 'adv_norm = agent left the weights of the none run'


def test_adv_norm_with_the_other_opt_in_keys():
    """lstm_precision = bf16x3, gae_lambda < 1 and optimizer = adam together with adv_norm = agent: captured equals eager, the
    advantages are the restatements (the scan's at lambda = 0.9)."""
    extra = dict(lstm_precision='bf16x3', gae_lambda='0.9', optimizer='adam')
    runs = []
    for use_graph in (True, False):
        env, model, tr = _build('ia2c_fp', use_graph, 'agent', extra=extra)
        for _ in range(3):
            tr.run_batch()
        torch.cuda.synchronize()
        _assert_model_advantages(model, tr.R_end, 0.9)
        runs.append(model.policy.params.flat.clone())
        assert torch.isfinite(runs[-1]).all()
        del env, model, tr
    assert torch.equal(runs[0], runs[1])


def test_one_replica_backward_with_adv_norm():
    """The reference-API path (model.forward / add_transition / backward, one replica): the scripted three-batch run of the
    IA2C-FP golden with adv_norm = agent; the last update's Adv_n is the restatement of its Adv, the weights are finite."""
    from deeprl_network_amd.agents import models
    z = load_npz(os.path.join(GOLDEN, 'nn_ia2c_fp_line.npz'))
    assert str(z['agent']) == 'ia2c_fp' and str(z['topo']) == 'line' and float(z['coop_gamma']) < 0
    cp = cacc_config(agent='ia2c_fp', n_step=int(z['n_step']), reward_norm=float(z['reward_norm']), coop_gamma=-1)
    cp['MODEL_CONFIG']['adv_norm'] = 'agent'
    nb = z['nb']
    N = nb.shape[0]
    np.random.seed(int(z['seed']))
    model = models.IA2C_FP([5 * (1 + int(nb[i].sum())) for i in range(N)], [4] * N, nb, z['dist'], -1.0, 10000, cp['MODEL_CONFIG'],
                           seed=int(z['seed']), num_envs=1, device='cuda')
    out = drive_scripted(model, z)
    R_end = torch.from_numpy(np.asarray(out['RB'][-1], dtype=np.float32).reshape(N, 1))
    _assert_model_advantages(model, R_end)
    assert torch.isfinite(model.policy.params.flat).all()

"""The opt-in GAE(lambda) return scan on the device (csrc/a2c.hip: gae_kernel, nmarl_gae_return) and in the engine: the kernel against
the float64 restatement of tests/gae_checks.py at the return scan's edge shapes (T = 1, T below and off the unroll of ten, the full
64 x 64 weight table, one-way reachability at N = 2, more replicas than one block, one replica), lambda = 1 against nstep_kernel on
the device, the ABI's refusals, and MODEL_CONFIG gae_lambda through BatchedTrainer (eager and captured) and the one-replica path."""
import os
import sys

import numpy as np
import pytest
import torch

import gae_checks as gc
import update_edge_checks as uec
from helpers import GOLDEN, cacc_config, drive_scripted, load_npz

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

# alpha x table: both tables on the spatial path, `line` only on the global one
PATHS = [(-1.0, 'line')] + [(a, t) for a in (0.9, 0.0, 1.0) for t in uec.NSTEP_TABLES]
LAMBDAS = [0.0, 0.95, 1.0]


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('lam', LAMBDAS)
@pytest.mark.parametrize('alpha,table', PATHS)
@pytest.mark.parametrize('N,E,T', uec.NSTEP_SHAPES)
def test_gae_kernel_equals_the_restatement(N, E, T, alpha, table, lam):
    from deeprl_network_amd import ops
    gc.check_gae(ops, 'cuda', N, E, T, alpha, table, lam)


@pytest.mark.parametrize('lam', LAMBDAS)
@pytest.mark.parametrize('table', uec.NSTEP_TABLES)
@pytest.mark.parametrize('N,E,T', [(7, 70, 23), (25, 9, 30)])
def test_spatial_sum_in_blocks_of_four_with_a_remainder(N, E, T, table, lam):
    """The spatial sum takes j four at a time and the last N % 4 one by one: the return scan's five shapes have N = 28, 64, 8 (blocks
    only) and 3, 2 (remainder only); these have both (7 = 4 + 3; 25 = 6 x 4 + 1, the grid's agent count), T off and on the unroll."""
    from deeprl_network_amd import ops
    gc.check_gae(ops, 'cuda', N, E, T, 0.9, table, lam)


@pytest.mark.parametrize('alpha,table', PATHS)
@pytest.mark.parametrize('N,E,T', uec.NSTEP_SHAPES)
def test_lambda_one_equals_nstep_return_on_the_device(N, E, T, alpha, table):
    from deeprl_network_amd import ops
    r, v, done, R_end, dist = (x.cuda() for x in gc.gae_inputs(N, E, T, alpha, table))
    R_n, A_n = ops.nstep_return(r, v, done, R_end, gc.GAE_GAMMA, alpha, dist)
    R_g, A_g = ops.gae_return(r, v, done, R_end, gc.GAE_GAMMA, 1.0, alpha, dist)
    # (the n-step kernel's fp32 results, read as exact numbers, are the expectation of the return scan's bound)
    gc.assert_gae_close(R_g, A_g, R_n.cpu().double(), A_n.cpu().double(), alpha >= 0, 'lambda=1 vs nstep_kernel')


def test_abi_refusals_write_nothing():
    """N = 65, alpha >= 0 without a distance table, lambda outside [0, 1] or NaN: NMARL_EINVAL and the outputs keep their bits;
    E = 0: OK without a launch."""
    from deeprl_network_amd import _lib
    lib, ptr = _lib.lib, _lib.ptr
    F32 = torch.float32
    cases = [(65, -1.0, True, 0.9), (65, 0.9, True, 0.9), (4, 0.9, False, 0.9), (4, 0.0, False, 0.9),
             (4, -1.0, True, -0.01), (4, -1.0, True, 1.01), (4, -1.0, True, float('nan')), (4, 0.9, True, float('nan'))]
    for N, alpha, with_dist, lam in cases:
        E, T = 2, 3
        r = torch.zeros(T, E, N, device='cuda')
        v, done, R_end = torch.zeros(T, N, E, device='cuda'), torch.zeros(T, E, dtype=torch.uint8, device='cuda'), torch.zeros(N, E, device='cuda')
        dist = torch.zeros(N, N, dtype=torch.int32, device='cuda') if with_dist else None
        R_out, adv_out = torch.full((N, T, E), -777.0, device='cuda'), torch.full((N, T, E), -777.0, device='cuda')
        rc = lib.nmarl_gae_return(E, N, T, ptr(r, F32), ptr(v, F32), ptr(done, torch.uint8), ptr(R_end, F32), 0.99, lam, alpha,
                                  ptr(dist, torch.int32), ptr(R_out), ptr(adv_out), _lib.stream())
        assert rc == -1, (N, alpha, with_dist, lam, rc)                # NMARL_EINVAL
        torch.cuda.synchronize()
        assert bool((R_out == -777.0).all()) and bool((adv_out == -777.0).all())
    # T = 0 and a null input are refused as well (the last case's tensors, a lambda that is fine)
    for T_bad, null_v in ((0, False), (T, True)):
        rc = lib.nmarl_gae_return(E, N, T_bad, ptr(r, F32), None if null_v else ptr(v, F32), ptr(done, torch.uint8), ptr(R_end, F32),
                                  0.99, 0.9, alpha, ptr(dist, torch.int32), ptr(R_out), ptr(adv_out), _lib.stream())
        assert rc == -1, (T_bad, null_v, rc)
    torch.cuda.synchronize()
    assert bool((R_out == -777.0).all()) and bool((adv_out == -777.0).all())
    assert lib.nmarl_gae_return(0, 4, 3, None, None, None, None, 0.99, 0.9, -1.0, None, None, None, _lib.stream()) == 0


# ------------------------------------------------------------------------------------------------------------------ the engine
E_ENGINE, T_ENGINE = 8, 5


def _build(agent, use_graph, gae_lambda, scenario='catchup', coop_gamma=-1, **trainer_kw):
    from deeprl_network_amd.envs import make_batch_env
    from deeprl_network_amd.main import init_agent
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    cp = cacc_config(agent=agent, scenario=scenario, n_step=T_ENGINE, coop_gamma=coop_gamma,
                     reward_norm=800.0 if agent.startswith('ia2c') else 5000.0)
    if gae_lambda is not None:
        cp['MODEL_CONFIG']['gae_lambda'] = gae_lambda
    env = make_batch_env(cp['ENV_CONFIG'], num_envs=E_ENGINE)
    np.random.seed(12)
    model = init_agent(env, cp['MODEL_CONFIG'], 10 ** 9, 12, num_envs=E_ENGINE)
    return env, model, BatchedTrainer(env, model, Counter(10 ** 12, 10 ** 12, 10 ** 12), use_graph=use_graph, **trainer_kw)


def _assert_model_scan(model, R_end, lam):
    """model.R / model.Adv == the restatement on the model's own rollout buffers."""
    alpha = model.coop_gamma if model.coop_gamma >= 0 else -1.0
    assert tuple(model.buf_r.shape) == ((model.n_step, model.E, model.n_agent) if alpha >= 0 else (model.n_step, model.E))
    exp_R, exp_A = gc.gae_expect(model.buf_r, model.buf_v, model.buf_done_post, R_end, model.gamma, lam, alpha, model.dist_dev)
    gc.assert_gae_close(model.R, model.Adv, exp_R, exp_A, alpha >= 0, '%s lam=%g' % (model.name, lam))
    assert float(exp_A.abs().max()) > 0


ENGINE_CASES = [('ia2c_fp', 'catchup', -1), ('ma2c_nc', 'slowdown', 0.9)]


@pytest.mark.parametrize('agent,scenario,coop_gamma', ENGINE_CASES)
def test_update_scan_is_the_restatement_of_the_models_buffers(agent, scenario, coop_gamma):
    env, model, tr = _build(agent, False, '0.9', scenario, coop_gamma)
    assert model.gae_lambda == 0.9
    tr.run_batch()
    torch.cuda.synchronize()
    _assert_model_scan(model, tr.R_end, 0.9)
    # lambda < 1 is not the n-step scan of the same buffers
    from deeprl_network_amd import ops
    alpha = coop_gamma if coop_gamma >= 0 else -1.0
    R_n, _ = ops.nstep_return(model.buf_r, model.buf_v, model.buf_done_post, tr.R_end, model.gamma, alpha, model.dist_dev)
    assert not torch.equal(R_n, model.R)


@pytest.mark.parametrize('agent,scenario,coop_gamma', ENGINE_CASES)
def test_captured_update_equals_eager_with_gae(agent, scenario, coop_gamma):
    import graph_nodes as G
    runs = []
    for use_graph in (True, False):
        env, model, tr = _build(agent, use_graph, '0.9', scenario, coop_gamma, **(dict(keep_graphs=True) if use_graph else {}))
        w0 = model.policy.params.flat.clone()
        for _ in range(3):
            tr.run_batch()
        torch.cuda.synchronize()
        assert tr.handoff_fallbacks == 0
        if use_graph:
            assert tr._upd is not None and tr.update_capture_error is None
            c = G.census(tr._upd['grads'])
            assert c.get('kernel', 0) > 0 and set(c) == {'kernel'}, c
        _assert_model_scan(model, tr.R_end, 0.9)
        runs.append(model.policy.params.flat.clone())
        assert torch.isfinite(runs[-1]).all() and not torch.equal(runs[-1], w0)
        del env, model, tr
    assert torch.equal(runs[0], runs[1]), 'captured update with gae_lambda differs from the eager one'


@pytest.mark.parametrize('agent,scenario,coop_gamma', ENGINE_CASES)
def test_explicit_lambda_one_is_the_untouched_default_path(agent, scenario, coop_gamma, monkeypatch):
    from deeprl_network_amd import ops
    n_gae = []
    inner = ops.gae_return
    monkeypatch.setattr(ops, 'gae_return', lambda *a, **kw: n_gae.append(1) or inner(*a, **kw))
    runs = []
    for value in ('1.0', None):
        env, model, tr = _build(agent, True, value, scenario, coop_gamma)
        assert model.gae_lambda == 1.0
        for _ in range(2):
            tr.run_batch()
        torch.cuda.synchronize()
        runs.append((model.policy.params.flat.clone(), model.R.clone(), model.Adv.clone()))
        del env, model, tr
    assert not n_gae
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_one_replica_backward_with_gae():
    """The reference-API path (model.forward / add_transition / backward, one replica): the scripted three-batch run of the
    IA2C-FP golden with gae_lambda = 0.9; the last update's R / Adv are the restatement of its buffers."""
    from deeprl_network_amd.agents import models
    z = load_npz(os.path.join(GOLDEN, 'nn_ia2c_fp_line.npz'))
    assert str(z['agent']) == 'ia2c_fp' and str(z['topo']) == 'line' and float(z['coop_gamma']) < 0
    cp = cacc_config(agent='ia2c_fp', n_step=int(z['n_step']), reward_norm=float(z['reward_norm']), coop_gamma=-1)
    cp['MODEL_CONFIG']['gae_lambda'] = '0.9'
    nb = z['nb']
    N = nb.shape[0]
    np.random.seed(int(z['seed']))
    model = models.IA2C_FP([5 * (1 + int(nb[i].sum())) for i in range(N)], [4] * N, nb, z['dist'], -1.0, 10000, cp['MODEL_CONFIG'],
                           seed=int(z['seed']), num_envs=1, device='cuda')
    out = drive_scripted(model, z)
    R_end = torch.from_numpy(np.asarray(out['RB'][-1], dtype=np.float32).reshape(N, 1))
    _assert_model_scan(model, R_end, 0.9)
    assert torch.isfinite(model.policy.params.flat).all()

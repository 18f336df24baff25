"""The opt-in clip + Adam optimiser step on the device (csrc/a2c.hip: adam_sumsq_kernel + adam_kernel, nmarl_adam_clip[_guarded]) and
in the engine: the kernel against the float64 restatement of tests/adam_checks.py at the optimiser's edge shapes (no clip / clipped /
not clipped, above the grid stride, odd P with unaligned group bases, one parameter) crossed with the step counts 0 / 999 / 1e7, the
device lr and the degenerate betas; the reported norm against the RMSProp entry's; the guard, the ABI's refusals and a replayed graph;
then MODEL_CONFIG optimizer = adam through BatchedTrainer (eager and captured), the one-replica path, the config's refusals and the
checkpoints."""
import logging
import os

import numpy as np
import pytest
import torch

import adam_checks as ac
from adam_checks import _f32, _same_bits
from helpers import GOLDEN, cacc_config, drive_scripted, load_npz

pytestmark = pytest.mark.gpu

F32 = torch.float32


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('beta1,beta2', ac.ADAM_BETAS)
@pytest.mark.parametrize('use_lr_dev', [False, True])
@pytest.mark.parametrize('t0', ac.ADAM_T0)
@pytest.mark.parametrize('G,P,max_norm,grad_scale', ac.ADAM_SHAPES)
def test_adam_kernel_equals_the_restatement(G, P, max_norm, grad_scale, t0, use_lr_dev, beta1, beta2):
    from deeprl_network_amd import ops
    ac.check_adam(ops, 'cuda', G, P, max_norm, grad_scale, use_lr_dev, t0, beta1, beta2)


@pytest.mark.parametrize('G,P,max_norm,grad_scale', ac.ADAM_SHAPES)
def test_reported_norm_has_the_bits_of_the_rmsprop_entry(G, P, max_norm, grad_scale):
    from deeprl_network_amd import ops
    w, m, v, g = (x.cuda() for x in ac.adam_inputs(G, P, 5, _f32(ac.ADAM_EPS)))
    g = g * 3.0
    scratch = torch.zeros(G, 64, device='cuda')
    n_adam, n_rms = torch.full((G,), -7.0, device='cuda'), torch.full((G,), -9.0, device='cuda')
    ops.adam_clip(w.clone(), g, m, v, scratch, torch.zeros(1, dtype=torch.int32, device='cuda'), 5e-4, 0.9, 0.999, ac.ADAM_EPS,
                  max_norm, grad_scale, n_adam)
    ops.rmsprop_tf_clip(w.clone(), g, torch.ones_like(w), scratch, 5e-4, 0.99, 1e-5, max_norm, grad_scale, n_rms)
    assert _same_bits(n_adam, n_rms)
    assert bool((n_adam[:1] > 0).all())


def test_guarded_step_changes_nothing_while_the_status_word_is_set():
    ac.check_adam_guard('cuda')


def _abi_call(lib, ptr, t, G, P, beta1=0.9, beta2=0.999, eps=1e-8, null=None):
    from deeprl_network_amd import _lib
    p = {k: (None if k == null else ptr(x, torch.int32 if k == 'step' else F32)) for k, x in t.items()}
    return lib.nmarl_adam_clip_guarded(G, P, p['w'], p['g'], p['m'], p['v'], p['scratch'], p['step'], None, 5e-4, beta1, beta2, eps, 0.5,
                                       1.0, p['norm'], None, _lib.stream())


def test_abi_refusals_write_nothing():
    """A null w / g / m / v / scratch / step, G = 0, P < 0, beta1 = 1, beta2 = -0.1, eps = 0 and a NaN in each of the three:
    NMARL_EINVAL, and the sentinel-filled w, m, v, step keep their bits.  P = 0: OK without a launch."""
    from deeprl_network_amd import _lib
    lib, ptr = _lib.lib, _lib.ptr
    G, P = 2, 37
    nan = float('nan')
    t = dict(w=torch.full((G, P), -777.0, device='cuda'), g=torch.ones(G, P, device='cuda'), m=torch.full((G, P), -778.0, device='cuda'),
             v=torch.full((G, P), 779.0, device='cuda'), scratch=torch.zeros(G, 64, device='cuda'),
             step=torch.full((1,), 41, dtype=torch.int32, device='cuda'), norm=torch.full((G,), -7.0, device='cuda'))
    before = {k: x.clone() for k, x in t.items()}
    cases = [dict(null=k) for k in ('w', 'g', 'm', 'v', 'scratch', 'step')]
    cases += [dict(G=0), dict(G=-1), dict(P=-1), dict(beta1=1.0), dict(beta2=-0.1), dict(eps=0.0), dict(eps=-1e-8), dict(beta1=-0.1),
              dict(beta2=1.0), dict(beta1=nan), dict(beta2=nan), dict(eps=nan)]
    for kw in cases:
        rc = _abi_call(lib, ptr, t, kw.pop('G', G), kw.pop('P', P), **kw)
        assert rc == -1, (kw, rc)                                         # NMARL_EINVAL
    assert _abi_call(lib, ptr, t, G, 0) == 0
    torch.cuda.synchronize()
    for k in t:
        assert _same_bits(t[k], before[k]), k
    # (the same arguments without a mistake are accepted: the refusals above are the mistakes')
    assert _abi_call(lib, ptr, t, G, P) == 0
    torch.cuda.synchronize()
    assert t['step'].tolist() == [42] and not _same_bits(t['w'], before['w'])


def test_replayed_graph_counts_its_steps_on_the_device():
    """One captured call (a single stream, no parallel branches) replayed three times with g and the device lr rewritten in place ==
    three eager calls, bit for bit in w, m, v and the counter: t advances on the device although every replay re-sends the same
    host arguments."""
    from deeprl_network_amd import ops
    G, P, t0 = 3, 1000, 0
    w0, m0, v0, g0 = (x.cuda() for x in ac.adam_inputs(G, P, t0, _f32(ac.ADAM_EPS)))
    lrs = [5e-4, 5e-4, 2.5e-4]

    def state():
        return dict(w=w0.clone(), m=m0.clone(), v=v0.clone(), step=torch.full((1,), t0, dtype=torch.int32, device='cuda'),
                    g=g0.clone(), lr=torch.zeros(1, device='cuda'), scratch=torch.zeros(G, 64, device='cuda'),
                    norm=torch.zeros(G, device='cuda'))

    def call(s):
        ops.adam_clip(s['w'], s['g'], s['m'], s['v'], s['scratch'], s['step'], 1.0, 0.9, 0.999, ac.ADAM_EPS, 0.5, 0.5, s['norm'],
                      lr_dev=s['lr'])

    eager, norms = state(), []
    for k in range(3):
        eager['g'].copy_(g0 * float(k + 1))
        eager['lr'].fill_(lrs[k])
        call(eager)
        norms.append(eager['norm'].clone())
    torch.cuda.synchronize()
    cap = state()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(cap)
    torch.cuda.synchronize()
    assert cap['step'].tolist() == [t0] and _same_bits(cap['w'], w0)            # capturing launches nothing
    for k in range(3):
        cap['g'].copy_(g0 * float(k + 1))
        cap['lr'].fill_(lrs[k])
        graph.replay()
        assert _same_bits(cap['norm'], norms[k])
    torch.cuda.synchronize()
    assert cap['step'].tolist() == [t0 + 3]
    for k in ('w', 'm', 'v', 'step'):
        assert _same_bits(cap[k], eager[k]), k
    assert not _same_bits(cap['w'], w0)


# ------------------------------------------------------------------------------------------------------------------ the engine
E_ENGINE, T_ENGINE = 8, 5
AGENTS = ['ia2c', 'ia2c_fp', 'ma2c_cu', 'ma2c_nc', 'ma2c_ic3', 'ma2c_dial']


def _config(agent, optimizer, scenario='catchup', **keys):
    """optimizer: the value of the ini key, None = key absent; keys: further MODEL_CONFIG keys."""
    cp = cacc_config(agent=agent, scenario=scenario, n_step=T_ENGINE, reward_norm=800.0 if agent.startswith('ia2c') else 5000.0)
    if optimizer is not None:
        cp['MODEL_CONFIG']['optimizer'] = optimizer
    for k, v in keys.items():
        cp['MODEL_CONFIG'][k] = v
    return cp


def _build(agent, use_graph, optimizer, scenario='catchup', total_step=10 ** 9, **trainer_kw):
    from deeprl_network_amd.envs import make_batch_env
    from deeprl_network_amd.main import init_agent
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    cp = _config(agent, optimizer, scenario)
    env = make_batch_env(cp['ENV_CONFIG'], num_envs=E_ENGINE)
    np.random.seed(12)
    model = init_agent(env, cp['MODEL_CONFIG'], total_step, 12, num_envs=E_ENGINE)
    return env, model, BatchedTrainer(env, model, Counter(10 ** 12, 10 ** 12, 10 ** 12), use_graph=use_graph, **trainer_kw)


def _watch_apply(model):
    """Wrap model.update_apply: -> the list that receives, per call, what the step saw (the weights, slots and counter before it, the
    model's own flat gradient as update_grads left it, the lr) and what it left."""
    log, inner, ps = [], model.update_apply, model.policy.params

    def update_apply(lr, rotate=True, lr_dev=None):
        assert lr_dev is None                                       # (the eager update passes the host lr)
        rec = dict(prev=(ps.flat.detach().clone(), ps.adam_m.clone(), ps.adam_v.clone()), t=int(ps.adam_t.item()), g=ps.grad.clone(), lr=lr)
        inner(lr, rotate=rotate, lr_dev=lr_dev)
        rec['got'] = (ps.flat.detach().clone(), ps.adam_m.clone(), ps.adam_v.clone(), model.grad_norm.clone())
        log.append(rec)
    model.update_apply = update_apply
    return log


def _assert_logged_steps(model, log):
    """Every logged optimiser step == the float64 restatement of the state and the gradient it saw, within check_adam's bounds, on the
    model's [G,P] views (per agent, or joint)."""
    N, P = model.policy.params.flat.shape
    shape, G = ((N, P), N) if model.per_agent_optimizer else ((1, N * P), 1)
    for k, rec in enumerate(log):
        assert rec['t'] == k
        prev = tuple(x.reshape(shape) for x in rec['prev'])
        got = tuple(x.reshape(shape) for x in rec['got'][:3]) + (rec['got'][3][:G],)
        used, dw = ac.assert_adam_step(prev, rec['g'].reshape(shape), rec['t'], got, _f32(rec['lr']), _f32(model.adam_beta1),
                                       _f32(model.adam_beta2), _f32(model.adam_epsilon), _f32(model.max_grad_norm), 1.0,
                                       '%s update %d' % (model.name, k), underflow=ac.FP32_SUBNORMAL)
        assert float(dw.max()) > 0 and float(rec['g'].abs().max()) > 0
        assert not _same_bits(rec['prev'][0], rec['got'][0])


@pytest.mark.parametrize('agent,scenario', [('ia2c_fp', 'catchup'), ('ma2c_nc', 'slowdown')])
def test_engine_step_is_the_restatement_of_the_models_gradient(agent, scenario):
    """One eager batch of BatchedTrainer under adam: IA2C-FP steps one optimiser per agent (G = N), NeurComm one joint, guarded one."""
    env, model, tr = _build(agent, False, 'adam', scenario)
    ps = model.policy.params
    assert model.optimizer == 'adam' and model.per_agent_optimizer == (agent == 'ia2c_fp')
    assert model.handoff_guarded == (agent == 'ma2c_nc')
    assert ps.adam_t.dtype == torch.int32 and ps.adam_t.numel() == 1 and ps.adam_m.shape == ps.flat.shape == ps.adam_v.shape
    assert not ps.adam_m.any() and not ps.adam_v.any() and ps.adam_t.item() == 0
    log = _watch_apply(model)
    tr.run_batch()
    torch.cuda.synchronize()
    assert len(log) == 1 and tr.handoff_fallbacks == 0
    _assert_logged_steps(model, log)
    assert ps.adam_t.item() == 1 and bool(ps.ms.eq(1.0).all())                # the RMSProp slot is not touched


@pytest.mark.parametrize('agent,scenario', [('ia2c_fp', 'catchup'), ('ma2c_nc', 'slowdown')])
def test_captured_update_equals_eager_with_adam(agent, scenario):
    runs = []
    for use_graph in (True, False):
        env, model, tr = _build(agent, use_graph, 'adam', scenario)
        ps = model.policy.params
        w0 = ps.flat.clone()
        for _ in range(3):
            tr.run_batch()
        torch.cuda.synchronize()
        assert tr.handoff_fallbacks == 0
        if use_graph:
            assert tr._upd is not None and tr.update_capture_error is None
        assert ps.adam_t.tolist() == [3]
        runs.append((ps.flat.clone(), ps.adam_m.clone(), ps.adam_v.clone(), ps.adam_t.clone(), model.grad_norm.clone()))
        assert torch.isfinite(runs[-1][0]).all() and not torch.equal(runs[-1][0], w0)
        del env, model, tr
    for a, b in zip(*runs):
        assert _same_bits(a, b), 'captured update under adam differs from the eager one'


@pytest.mark.parametrize('agent', AGENTS)
def test_every_agent_trains_two_batches_with_adam(agent):
    """All six agents; ConseNet's consensus averaging runs behind the Adam step as it does behind RMSProp: after each update the
    agents' LSTM blocks are the neighbourhood averages of what the optimiser step left."""
    env, model, tr = _build(agent, False, 'adam')
    ps, p = model.policy.params, model.policy
    w0 = ps.flat.clone()
    seen = []
    if agent == 'ma2c_cu':
        inner = p.consensus_update
        o0, o1 = ps.index['lstm_wx'][0], ps.index['lstm_b'][0] + ps.index['lstm_b'][1]

        def consensus_update():
            t, before = int(ps.adam_t.item()), ps.flat[:, o0:o1].detach().clone()
            inner()
            seen.append((t, before, ps.flat[:, o0:o1].detach().clone()))
        p.consensus_update = consensus_update
    for _ in range(2):
        tr.run_batch()
    torch.cuda.synchronize()
    assert ps.adam_t.tolist() == [2] and tr.handoff_fallbacks == 0
    assert torch.isfinite(ps.flat).all() and torch.isfinite(ps.adam_m).all() and torch.isfinite(ps.adam_v).all()
    assert not torch.equal(ps.flat, w0) and bool(ps.adam_v.any())
    if agent == 'ma2c_cu':
        assert [t for t, _, _ in seen] == [1, 2]                      # behind the step: the counter has advanced
        for _, before, after in seen:
            torch.testing.assert_close(after, p._avg @ before, rtol=1e-6, atol=1e-7)
            assert not torch.equal(after, before)


def test_one_replica_backward_with_adam():
    """The reference-API path (model.forward / add_transition / backward, one replica): the scripted three-batch run of the IA2C-FP
    golden under adam; every model.backward moves the weights as the restatement says."""
    from deeprl_network_amd.agents import models
    z = load_npz(os.path.join(GOLDEN, 'nn_ia2c_fp_line.npz'))
    assert str(z['agent']) == 'ia2c_fp' and str(z['topo']) == 'line'
    cp = cacc_config(agent='ia2c_fp', n_step=int(z['n_step']), reward_norm=float(z['reward_norm']), coop_gamma=-1)
    cp['MODEL_CONFIG']['optimizer'] = 'adam'
    nb = z['nb']
    N = nb.shape[0]
    np.random.seed(int(z['seed']))
    model = models.IA2C_FP([5 * (1 + int(nb[i].sum())) for i in range(N)], [4] * N, nb, z['dist'], -1.0, 10000, cp['MODEL_CONFIG'],
                           seed=int(z['seed']), num_envs=1, device='cuda')
    log = _watch_apply(model)
    drive_scripted(model, z)
    assert len(log) == z['X'].shape[0] == model.policy.params.adam_t.item()
    _assert_logged_steps(model, log)
    assert torch.isfinite(model.policy.params.flat).all()


@pytest.mark.parametrize('agent,scenario', [('ia2c_fp', 'catchup'), ('ma2c_nc', 'slowdown')])
def test_explicit_rmsprop_is_the_untouched_default_path(agent, scenario, monkeypatch):
    from deeprl_network_amd import ops
    n_adam = []
    inner = ops.adam_clip
    monkeypatch.setattr(ops, 'adam_clip', lambda *a, **kw: n_adam.append(1) or inner(*a, **kw))
    runs = []
    for value in ('rmsprop', None):
        env, model, tr = _build(agent, True, value, scenario)
        ps = model.policy.params
        assert model.optimizer == 'rmsprop' and ps.adam_m is None and ps.adam_v is None and ps.adam_t is None
        for _ in range(2):
            tr.run_batch()
        torch.cuda.synchronize()
        runs.append((ps.flat.clone(), ps.ms.clone(), model.grad_norm.clone()))
        del env, model, tr
    assert not n_adam
    for a, b in zip(*runs):
        assert _same_bits(a, b)


@pytest.mark.parametrize('optimizer,keys', [('sgd', {}), ('adam', dict(adam_beta2='1')), ('adam', dict(adam_epsilon='0')),
                                            ('adam', dict(adam_beta1='-0.1')), ('adam', dict(adam_beta1='nan')),
                                            (None, dict(adam_epsilon='nan'))])
def test_config_refusals(optimizer, keys):
    from deeprl_network_amd.envs import make_batch_env
    from deeprl_network_amd.main import init_agent
    cp = _config('ia2c_fp', optimizer, **keys)
    env = make_batch_env(cp['ENV_CONFIG'], num_envs=E_ENGINE)
    with pytest.raises(ValueError, match='optimizer|adam_'):
        init_agent(env, cp['MODEL_CONFIG'], 10 ** 9, 12, num_envs=E_ENGINE)


def test_config_keys_reach_the_step():
    env, model, tr = _build('ia2c_fp', False, 'adam')
    assert (model.adam_beta1, model.adam_beta2, model.adam_epsilon) == (0.9, 0.999, 1e-8)
    from deeprl_network_amd.envs import make_batch_env
    from deeprl_network_amd.main import init_agent
    cp = _config('ia2c_fp', ' Adam ', adam_beta1='0.5', adam_beta2='0.75', adam_epsilon='1e-6')
    model = init_agent(make_batch_env(cp['ENV_CONFIG'], num_envs=E_ENGINE), cp['MODEL_CONFIG'], 10 ** 9, 12, num_envs=E_ENGINE)
    assert model.optimizer == 'adam' and (model.adam_beta1, model.adam_beta2, model.adam_epsilon) == (0.5, 0.75, 1e-6)


# ----------------------------------------------------------------------------------------------------------------- checkpoints
def _synthetic_step(model, seed=7):
    ps = model.policy.params
    g = torch.randn(ps.grad.shape, generator=torch.Generator().manual_seed(seed)) * 0.05
    ps.grad.copy_(g)
    model.update_apply(2.5e-4, rotate=False)
    torch.cuda.synchronize()


def test_checkpoint_round_trip_restores_the_adam_state(tmp_path):
    env, model, tr = _build('ia2c_fp', False, 'adam')
    for _ in range(2):
        tr.run_batch()
    d = str(tmp_path) + '/'
    model.save(d, 10)
    blob = torch.load(d + 'checkpoint-10.pt', weights_only=True)
    assert blob['optimizer'] == 'adam' and 'rmsprop_ms' not in blob and blob['adam_t'].tolist() == [2]
    assert blob['adam_m'].shape == blob['adam_v'].shape == model.policy.params.flat.shape
    env2, model2, _ = _build('ia2c_fp', False, 'adam')
    assert model2.load(d)
    a, b = model.policy.params, model2.policy.params
    for k in ('flat', 'adam_m', 'adam_v', 'adam_t'):
        assert _same_bits(getattr(a, k), getattr(b, k)), k
    assert b.adam_t.dtype == torch.int32 and b.adam_t.is_cuda
    for m_ in (model, model2):
        _synthetic_step(m_)
    for k in ('flat', 'adam_m', 'adam_v', 'adam_t'):
        assert _same_bits(getattr(a, k), getattr(b, k)), k
    assert a.adam_t.tolist() == [3]


@pytest.mark.parametrize('saved,loading', [('rmsprop', 'adam'), ('adam', 'rmsprop')])
def test_checkpoint_of_the_other_optimizer_loads_the_variables_only(tmp_path, caplog, saved, loading):
    env, model, tr = _build('ia2c_fp', False, saved)
    for _ in range(2):
        tr.run_batch()
    d = str(tmp_path) + '/'
    model.save(d, 10)
    env2, model2, _ = _build('ia2c_fp', False, loading)
    with caplog.at_level(logging.WARNING):
        assert model2.load(d)
    assert any(r.levelno == logging.WARNING and 'optimizer' in r.getMessage() for r in caplog.records)
    a, b = model.policy.params, model2.policy.params
    assert _same_bits(a.flat, b.flat)
    assert bool(b.ms.eq(1.0).all())                                            # fresh either way
    if loading == 'adam':
        assert not b.adam_m.any() and not b.adam_v.any() and b.adam_t.tolist() == [0]
    else:
        assert b.adam_m is None and bool(a.adam_v.any())


def test_old_format_checkpoint_without_the_optimizer_key_loads(tmp_path, caplog):
    env, model, tr = _build('ia2c_fp', False, None)
    for _ in range(2):
        tr.run_batch()
    d = str(tmp_path) + '/'
    model.save(d, 10)
    blob = torch.load(d + 'checkpoint-10.pt', weights_only=True)
    assert blob.pop('optimizer') == 'rmsprop' and 'rmsprop_ms' in blob and not any(k.startswith('adam') for k in blob)
    torch.save(blob, d + 'checkpoint-10.pt')
    env2, model2, _ = _build('ia2c_fp', False, None)
    with caplog.at_level(logging.WARNING):
        assert model2.load(d)
    assert not [r for r in caplog.records if r.levelno >= logging.WARNING]
    a, b = model.policy.params, model2.policy.params
    assert _same_bits(a.flat, b.flat) and _same_bits(a.ms, b.ms) and not bool(b.ms.eq(1.0).all())
    # and it is an RMSProp checkpoint to an adam model: variables only, with the warning
    env3, model3, _ = _build('ia2c_fp', False, 'adam')
    with caplog.at_level(logging.WARNING):
        assert model3.load(d)
    assert any(r.levelno == logging.WARNING and 'optimizer' in r.getMessage() for r in caplog.records)
    assert _same_bits(a.flat, model3.policy.params.flat) and model3.policy.params.adam_t.tolist() == [0]

"""GPU: the `wait` / `hybrid` objectives of the synthetic network (net_step_kernel<REPS, WAIT = true>, through the C-ABI)
against their specification tests/realnet_wait_ref.py, the resets, the untouched `queue` form, the trainer on a `hybrid`
env, and the rule-based `greedy` agent through the reference duck-type and `main.py evaluate`."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import net_config

pytestmark = pytest.mark.gpu

COEF = 0.2


def config(objective='queue', coop_gamma=0.9, seed=12, agent='ma2c_nc', coef_wait=COEF, n_step=120):
    cp = net_config(agent=agent, coop_gamma=coop_gamma, seed=seed, n_step=n_step)
    cp['ENV_CONFIG']['objective'] = objective
    cp['ENV_CONFIG']['coef_wait'] = str(coef_wait)
    cp['ENV_CONFIG']['flow_rate'] = '325'
    return cp


def make(E, objective='queue', coop_gamma=0.9, **kw):
    from deeprl_network_amd.envs.real_net_env import RealNetBatchEnv
    return RealNetBatchEnv(config(objective, coop_gamma, **kw)['ENV_CONFIG'], num_envs=E)


def make_ref(env, objective, coef_wait=COEF):
    from oracle import realnet_ref as R
    from realnet_wait_ref import NetWaitRef
    return NetWaitRef(R.NetParams(config=env.config), E=env.E, dtype=np.float32, objective=objective, coef_wait=coef_wait)


def rand_actions(rng, E, tp):
    return np.stack([rng.randint(0, tp.n_a_ls[i], size=E) for i in range(tp.N)], axis=1)


def hand_over(env, ref):
    """The oracle's state into the env: the two sides are then one step apart and a threshold decision cannot drift."""
    env.q.copy_(torch.from_numpy(ref.q))
    env.transit.copy_(torch.from_numpy(ref.tr))
    env.prev_action.copy_(torch.from_numpy(ref.prev.astype(np.uint8)))
    env.t.copy_(torch.from_numpy(ref.t.astype(np.int32)))
    env.head_wait.copy_(torch.from_numpy(ref.hw))


def handed_over_step(env, ref, a, what=''):
    """One step of both sides from the oracle's state; every assertion of the comparison.  -> (excluded links, hw of the oracle)."""
    from oracle import realnet_ref as R
    hand_over(env, ref)
    obs, r, d, g = env.step(torch.from_numpy(a).cuda())
    ro, rr, rd, rg = ref.step(a)
    valid = np.broadcast_to(ref.valid, ref.hw.shape)
    excl = ref.near_threshold(1e-5) & valid                # the decision sits within 1e-5 of WAIT_EPS: left out
    hw = env.head_wait.cpu().numpy()
    cmp = valid & ~excl
    assert np.array_equal(hw[cmp], ref.hw[cmp]), '%s: head_wait differs in %d links' % (what, (hw[cmp] != ref.hw[cmp]).sum())
    assert np.all(hw[~valid] == 0), '%s: head_wait on padding links' % what
    np.testing.assert_allclose(env.q.cpu().numpy(), ref.q, rtol=1e-5, atol=1e-5, err_msg=what)
    np.testing.assert_allclose(env.transit.cpu().numpy(), ref.tr, rtol=1e-5, atol=1e-5, err_msg=what)
    np.testing.assert_allclose(obs.cpu().numpy(), R.gather_net(ro), rtol=1e-5, atol=1e-6, err_msg=what)
    ok = ~excl.any(axis=(1, 2))                            # replicas with no excluded link: rewards
    np.testing.assert_allclose(g.cpu().numpy()[ok], rg[ok], rtol=2e-4, atol=5e-2, err_msg=what)
    np.testing.assert_allclose(r.cpu().numpy()[ok], rr[ok], rtol=2e-4, atol=5e-2, err_msg=what)
    assert np.array_equal(d.cpu().numpy().astype(bool), rd)
    return excl, valid


@pytest.mark.parametrize('objective,coop_gamma,E', [('wait', -1, 9), ('hybrid', 0.9, 300), ('hybrid', -1, 8), ('wait', 0.9, 1)])
def test_handed_over_steps_vs_oracle(objective, coop_gamma, E):
    """200 steps, each from the fp32 oracle's own state (q, transit, prev, t, head_wait copied in before the step): head_wait
    exactly, a link within 1e-5 of the threshold excepted (at most 1e-3 of all valid entries; fp32 against float64 gave 2e-4
    on the CPU), q / transit / observation at the single-step tolerances, rewards where no link is excepted."""
    from oracle import realnet_ref as R
    env = make(E, objective, coop_gamma)
    assert env.head_wait is not None and any(t is env.head_wait for t in env.state_tensors())
    assert env.params.objective == {'wait': 1, 'hybrid': 2}[objective] and env.params.coef_wait == pytest.approx(COEF)
    tp = R.TOPO
    rng = np.random.RandomState(E)
    U = rng.rand(E, 4).astype(np.float32)
    env.reset(u0=torch.from_numpy(U).cuda())
    ref = make_ref(env, objective)
    assert ref.p.flow_rate == 325 and ref.p.coop_gamma == coop_gamma
    ref.reset(np.float32(0.8) + np.float32(0.4) * U)
    np.testing.assert_array_equal(env.xi.cpu().numpy(), ref.xi)
    n_excl = n_valid = n_wait = n_node = 0
    hw_max = 0.0
    for t in range(200):
        hold = rng.rand(E, tp.N) < 0.6                     # keep the phase most of the time
        a = np.where(hold & (t > 0), ref.prev, rand_actions(rng, E, tp)).astype(np.uint8)
        excl, valid = handed_over_step(env, ref, a, 't=%d' % t)
        n_excl += int(excl.sum()); n_valid += int(valid.sum())
        n_wait += int((ref.hw.sum(axis=2) > 0).sum()); n_node += E * tp.N
        hw_max = max(hw_max, float(ref.hw.max()))
    print('excluded %d of %d valid entries (%.2e); hw max %.0f s; wait_i > 0 in %.3f of the (replica, node, step) entries'
          % (n_excl, n_valid, n_excl / n_valid, hw_max, n_wait / n_node))
    assert n_excl <= 1e-3 * n_valid
    assert hw_max >= 50 and n_wait > 0.5 * n_node          # not vacuous: queues stood through many red steps


def random_state(ref, rng):
    """A random mid-episode state of the oracle (as test_gpu_realnet.py::test_single_step_tight_from_random_state) with
    standing times on the valid links."""
    E, tp = ref.E, ref.tp
    ref.q = (rng.uniform(0, 30, size=(E, tp.N, tp.L)) * (rng.rand(E, tp.N, tp.L) < 0.8) * ref.valid).astype(np.float32)
    ref.q = np.minimum(ref.q, np.float32(26.0))
    ref.tr = (rng.uniform(0, 3, size=(E, tp.N, tp.L)) * ref.valid).astype(np.float32)
    ref.prev = rand_actions(rng, E, tp)
    ref.t = rng.randint(0, 700, size=E)
    ref.hw = (5.0 * rng.randint(0, 40, size=(E, tp.N, tp.L)) * ref.valid).astype(np.float32)


def test_eight_replicas_per_block_form_with_a_ragged_last_block():
    """E = 2049: the dispatch runs 8 replicas per block above 2048, and 2049 leaves one replica in the last block."""
    from oracle import realnet_ref as R
    E, tp = 2049, R.TOPO
    env = make(E, 'hybrid')
    rng = np.random.RandomState(7)
    env.reset(u0=torch.from_numpy(rng.rand(E, 4).astype(np.float32)).cuda())
    ref = make_ref(env, 'hybrid')
    ref.reset(env.xi.cpu().numpy())
    random_state(ref, rng)
    before = ref.hw.copy()
    a = np.where(rng.rand(E, tp.N) < 0.6, ref.prev, rand_actions(rng, E, tp)).astype(np.uint8)
    excl, valid = handed_over_step(env, ref, a, 'E=2049')
    assert excl.sum() <= 1e-3 * valid.sum()
    grew, cleared = (ref.hw == before + 5) & valid, (ref.hw == 0) & (before > 0) & valid
    assert grew.mean() > 0.05 and cleared.mean() > 0.05 and grew[-1].any() and cleared[-1].any()    # both branches, last replica too


def test_resets_clear_head_wait():
    E = 40
    env = make(E, 'wait')
    env.reset()
    env.head_wait.fill_(5.0); env.q.fill_(3.0); env.transit.fill_(1.0)
    env.t.fill_(env.T - 1)
    obs, r, d, g = env.step(torch.zeros(E, env.n_agent, dtype=torch.uint8, device='cuda'), auto_reset=True)
    assert d.all() and (env.t == 0).all()
    assert (env.head_wait == 0).all() and (env.q == 0).all() and (env.transit == 0).all() and (obs == 0).all()
    assert (g < 0).all()                                   # the reward of the last step still saw the standing times
    env.head_wait.fill_(5.0); env.q.fill_(3.0)
    mask = torch.from_numpy((np.random.RandomState(0).rand(E) < 0.5).astype(np.uint8)).cuda()
    assert 0 < int(mask.sum()) < E
    env.reset(mask=mask)
    m = mask.bool()
    assert (env.head_wait[m] == 0).all() and (env.head_wait[~m] == 5.0).all()
    assert (env.q[m] == 0).all() and (env.q[~m] == 3.0).all()
    env.head_wait.fill_(5.0)
    env.reset()
    assert (env.head_wait == 0).all()


def test_queue_env_has_no_head_wait_and_the_traffic_ignores_the_objective():
    """`queue` is untouched: no head_wait; over 50 free-running steps from the same seed a `hybrid` env's q, observation and
    transit equal a `queue` env's bit for bit, and with coef_wait = 0 so do its rewards."""
    from oracle import realnet_ref as R
    assert make(4).head_wait is None and len(make(4).state_tensors()) == 8
    E, tp = 9, R.TOPO
    envs = {'queue': make(E), 'hybrid': make(E, 'hybrid'), 'hybrid0': make(E, 'hybrid', coef_wait=0.0)}
    for env in envs.values():
        env.reset()
    rng = np.random.RandomState(2)
    a = rand_actions(rng, E, tp)
    differs = False
    for t in range(50):
        a = np.where(rng.rand(E, tp.N) < 0.6, a, rand_actions(rng, E, tp))
        out = {k: env.step(torch.from_numpy(a.astype(np.uint8)).cuda()) for k, env in envs.items()}
        for k in ('hybrid', 'hybrid0'):
            assert torch.equal(envs[k].q, envs['queue'].q) and torch.equal(envs[k].transit, envs['queue'].transit)
            assert torch.equal(out[k][0], out['queue'][0])
        assert torch.equal(out['hybrid0'][1], out['queue'][1]) and torch.equal(out['hybrid0'][3], out['queue'][3])
        differs = differs or not torch.equal(out['hybrid'][1], out['queue'][1])
    assert differs and envs['queue'].q.max() > 1 and envs['hybrid'].head_wait.max() >= 10


def test_step_rejects_a_bad_objective():
    from deeprl_network_amd import _lib
    env = make(4)
    env.reset()
    P = _lib.ptr
    a = torch.zeros(4, env.n_agent, dtype=torch.uint8, device='cuda')

    def step(objective, head_wait):
        p = _lib.NetParams()
        for f, _ in _lib.NetParams._fields_:
            setattr(p, f, getattr(env.params, f))
        p.objective, p.head_wait = objective, head_wait
        return _lib.lib.nmarl_net_step(ctypes.byref(p), ctypes.byref(env.topo.c), env.E, P(a), P(env.q), P(env.transit),
                                       P(env.prev_action), P(env.t), P(env.xi), P(env.obs), P(env.reward), P(env.done),
                                       P(env.global_reward), 0, env.seed, env.env_id_base, P(env.episode), _lib.stream())
    NMARL_EINVAL = -1
    assert step(1, None) == NMARL_EINVAL and step(2, None) == NMARL_EINVAL
    assert step(3, None) == NMARL_EINVAL and step(-1, None) == NMARL_EINVAL
    hw = torch.zeros_like(env.q)
    assert step(3, hw.data_ptr()) == NMARL_EINVAL
    assert (env.t == 0).all()                              # nothing was launched
    assert step(0, None) == 0 and step(1, hw.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (env.t == 2).all()


def test_trainer_runs_on_a_hybrid_env():
    """The batched engine (hipGraph rollout + update) on a `hybrid` env: finite, bit-identical across two runs, and the
    standing times are part of the rolled-out state."""
    from deeprl_network_amd.main import AGENTS
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    outs = []
    for rep in range(2):
        cp = config('hybrid', agent='ma2c_nc', n_step=24)
        env = make(64, 'hybrid', agent='ma2c_nc', n_step=24)
        np.random.seed(5)
        model = AGENTS['ma2c_nc'](env.n_s_ls, env.n_a_ls, env.neighbor_mask, env.distance_mask, env.coop_gamma, 10 ** 9,
                                  cp['MODEL_CONFIG'], seed=5, num_envs=64, device='cuda', n_feat_ls=env.n_feat_ls)
        tr = BatchedTrainer(env, model, Counter(10 ** 9, 10 ** 9, 10 ** 9), use_graph=True)
        for _ in range(4):
            tr.run_batch()
        torch.cuda.synchronize()
        flat = model.policy.params.flat
        assert torch.isfinite(flat).all()
        assert env.head_wait.max() > 0 and (env.head_wait % 5 == 0).all()
        outs.append((flat.clone(), env.head_wait.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_greedy_agent_through_the_reference_api_and_evaluate(tmp_path, monkeypatch):
    """`agent = greedy` on the network: every node is handed its own wave vector (atsc_env.py:256-257) and the global reward
    (205-206); `main.py evaluate` on a greedy run directory drives RealNetController through Evaluator.perform."""
    import pandas as pd
    from deeprl_network_amd.envs import init_env
    from deeprl_network_amd.envs.real_net_env import RealNetController, RealNetEnv
    from deeprl_network_amd.main import init_agent, main
    cp = config(agent='greedy', coop_gamma=0.9)
    env = init_env(cp['ENV_CONFIG'])
    ob = env.reset()
    assert [len(o) for o in ob] == list(env.n_feat_ls) == list(env.n_s_ls)
    ctl = init_agent(env, cp['MODEL_CONFIG'], 0, 0)
    assert isinstance(ctl, RealNetController) and ctl.node_names == env.node_names
    for _ in range(5):
        ob, r, d, g = env.step(ctl.forward(ob))
        assert [len(o) for o in ob] == list(env.n_feat_ls)
        assert np.ndim(r) == 0 and r == g and g <= 0 and not d
    # evaluation through the CLI, the observations recorded on the way
    seen = []
    orig = RealNetEnv._state_list

    def recording(self):
        out = orig(self)
        seen.append(out)
        return out
    monkeypatch.setattr(RealNetEnv, '_state_list', recording)
    base = tmp_path / 'greedy'
    (base / 'data').mkdir(parents=True)
    (base / 'model').mkdir()
    cp['ENV_CONFIG']['episode_length_sec'] = '300'
    with open(base / 'data' / 'config_greedy_net.ini', 'w') as f:
        cp.write(f)
    frames = []
    for _ in range(2):
        main(['--base-dir', str(base), 'evaluate', '--evaluation-seeds', '10000,20000'])
        frames.append(pd.read_csv(str(base / 'eva_data') + '/atsc_real_net_greedy_control.csv'))
    df = frames[0]
    assert len(df) == 2 * 60 and set(df['episode']) == {1, 2} and (df['reward'] <= 0).all() and (df['reward'] < 0).any()
    assert frames[0].equals(frames[1])                     # deterministic across two calls
    assert len(seen) == 2 * 2 * 61                         # per call and episode: the reset's observation + one per step
    names = sorted(env.node_names)
    ref_ctl = RealNetController(names)
    acts = [[int(x) for x in s.split(',')] for s in df['action']]
    for ep in range(2):
        for k in range(60):
            assert acts[ep * 60 + k] == ref_ctl.forward(seen[ep * 61 + k]), (ep, k)
    assert len({tuple(a) for a in acts}) > 1               # the controller reacts to the traffic

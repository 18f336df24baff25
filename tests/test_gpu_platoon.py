"""CACC platoons of any length 2 <= n_vehicle <= 32 on the GPU (nmarl_cacc_step_nv / nmarl_cacc_reset_nv, csrc/cacc_tile.h
cacc_tile_nv): a platoon sits in an aligned group of G lanes, G the smallest power of two >= N, memory stays dense.
  (1) the trajectories of the real reference env at N = 2 .. 32 (tests/golden/platoon_*.npz),
  (2) one step from random states against the fp32 oracle, every G, ragged last tiles, several blocks,
  (3) padding lanes and tail lanes write nothing (sentinel-guarded buffers),
  (4) N = 8 through the new entries == the 8-vehicle kernels bit for bit,
  (5) the Philox reset contract and the fused auto-reset,
  (6) the reference duck-type `CACCEnv`, the batched engine (eager == hipGraph, rollout vs oracle) and the CLI.
Tolerances are those of tests/test_gpu_cacc.py: per step rtol 1e-5 / atol 1e-6 against the fp32 oracle;
trajectories |dh|, |dv| <= 1e-3, reward rel 1e-4, identical done, no borderline state excluded."""
import configparser
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, cacc_config, load_npz

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(glob.glob(os.path.join(GOLDEN, 'platoon_*.npz')))
IDS = [os.path.basename(c)[8:-4] for c in CASES]


def platoon_config(N, agent='ma2c_nc', scenario='catchup', seed=12, coop_gamma=-1, **kw):
    cp = cacc_config(agent, scenario, seed, coop_gamma, **kw)
    cp['ENV_CONFIG']['n_vehicle'] = str(N)
    return cp


def make_env(N, E, scenario='catchup', agent='ma2c_nc', seed=12, coop_gamma=-1, train_mode=True, env_id_base=0, compact=False):
    from deeprl_network_amd.envs.cacc_env import CACCBatchEnv
    env = CACCBatchEnv(platoon_config(N, agent, scenario, seed, coop_gamma)['ENV_CONFIG'], num_envs=E, env_id_base=env_id_base)
    env.train_mode = train_mode
    if compact:
        assert env.set_compact_obs(True) and env.obs.shape == (E, N, 5)
    return env


def oracle_for(env, dtype=np.float32):
    from oracle.cacc_ref import CaccBatchRef, CaccParams
    ref = CaccBatchRef(CaccParams(config=env.config), E=env.E, dtype=dtype, train_mode=env.train_mode)
    assert ref.N == env.n_agent
    return ref


def test_have_cases():
    assert len(CASES) == 8


# ------------------------------------------------------------------------------------------------ (1) golden trajectories
@pytest.mark.parametrize('path', CASES, ids=IDS)
def test_golden_trajectory(path):
    """tests/test_gpu_cacc.py::test_golden_trajectory for every platoon_*.npz: CACCBatchEnv(E = 1) in the gathered AND the compact
    form against the float64 trajectory of the real reference env; the observation check runs over all N agents."""
    z = load_npz(path)
    N, agent = int(z['n_vehicle']), str(z['agent'])
    args = (N, 1, str(z['scenario']), agent, int(z['seed']), float(z['coop_gamma']), bool(z['train_mode']))
    env, cenv = make_env(*args), make_env(*args, compact=True)
    assert env.n_agent == N and env.h.shape == (1, N) and env.obs.shape == (1, N, 15)
    assert np.array_equal(env.neighbor_mask, z['neighbor_mask'])
    U = torch.tensor([float(z['U'])], dtype=torch.float32, device='cuda')
    env.reset(u0=U)
    cenv.reset(u0=U)
    n_s = z['n_s']
    n_nb = z['neighbor_mask'].sum(axis=1)
    width = [5 if agent.startswith('ma2c') else (int(n_s[i]) if agent == 'ia2c' else int(n_s[i]) - 4 * int(n_nb[i])) for i in range(N)]
    np.testing.assert_allclose(env.h.cpu().numpy()[0], z['h'][0], rtol=1e-6)

    def check_obs(k):
        o, oc = env.obs.cpu().numpy()[0], cenv.obs.cpu().numpy()[0]
        for i in range(N):
            np.testing.assert_allclose(o[i, :width[i]], z['obs'][k, i, :width[i]], atol=2e-4, rtol=1e-4)
            assert not o[i, 5 * (1 + int(n_nb[i])):].any()              # left-packed: the unused slots are zero
        np.testing.assert_allclose(oc, z['obs'][k, :, :5], atol=2e-4, rtol=1e-4)
        assert np.array_equal(o[:, :5], oc)

    check_obs(0)
    near = 0
    for k, a in enumerate(z['acts']):
        act = torch.as_tensor(a.astype(np.uint8)[None], device='cuda')
        obs, r, d, g = env.step(act)
        _, rc, dc, gc = cenv.step(act)
        s = torch.stack([env.h[0], env.v[0], env.u[0]]).cpu().numpy()
        np.testing.assert_allclose(s[0], z['h'][k + 1], atol=1e-3, err_msg='h step %d' % k)
        np.testing.assert_allclose(s[1], z['v'][k + 1], atol=1e-3, err_msg='v step %d' % k)
        np.testing.assert_allclose(s[2], z['u'][k + 1], atol=2e-3, err_msg='u step %d' % k)
        if abs(z['h'][k + 1].min() - 1.0) < 1e-4:
            near += 1   # borderline collision states are excluded and counted
            continue
        np.testing.assert_allclose(g.item(), z['global_reward'][k], rtol=1e-4, atol=1e-3)
        np.testing.assert_allclose(np.broadcast_to(r.cpu().numpy()[0], (N,)), z['reward'][k], rtol=1e-4, atol=1e-3)
        assert bool(d.item()) == bool(z['done'][k]), k
        assert torch.equal(g, gc) and torch.equal(d, dc) and torch.equal(r, rc) and torch.equal(env.h, cenv.h)
        check_obs(k + 1)
    assert near == 0
    assert bool(d.item())


# ------------------------------------------------------------------------------------------------ (2) one step vs fp32 oracle
def _random_state(ref, env, rng, scenario):
    E, N = env.E, env.n_agent
    ref.reset(rng.rand(E).astype(np.float32))
    ref.h = rng.uniform(0.5, 45, size=(E, N)).astype(np.float32)
    ref.v = rng.uniform(0, 30, size=(E, N)).astype(np.float32)
    ref.u = rng.uniform(-2.5, 2.5, size=(E, N)).astype(np.float32)
    ref.t = rng.choice([0, 1, 58, 59, 119, 297, 298, 299, 300, 598, 599], size=E).astype(np.int64)
    ref.collided = rng.rand(E) < 0.2
    ref.v0_init = rng.uniform(22, 30, size=E).astype(np.float32) if scenario == 'slowdown' else np.full(E, 15, np.float32)
    env.reset(u0=torch.zeros(E, device='cuda'))
    env.h.copy_(torch.from_numpy(ref.h)); env.v.copy_(torch.from_numpy(ref.v)); env.u.copy_(torch.from_numpy(ref.u))
    env.t.copy_(torch.from_numpy(ref.t.astype(np.int32)))
    env.collided.copy_(torch.from_numpy(ref.collided.astype(np.uint8)))
    env.v0_init.copy_(torch.from_numpy(ref.v0_init))


@pytest.mark.parametrize('scenario', ['catchup', 'slowdown'])
@pytest.mark.parametrize('N', [2, 3, 5, 7, 12, 16, 17, 25, 32])
def test_step_vs_fp32_oracle_random_state(N, scenario):
    """tests/test_gpu_cacc.py::test_step_vs_fp32_oracle_random_state at every group width (G = 2, 4, 8, 8, 16, 16, 32, 32, 32):
    E = 1, 13, 77 leave the last wave partly filled at every G, 1000 spans several blocks; global / per-agent reward, test mode,
    gathered and compact observation.  The flip-zone mask must keep > 99 % of the replicas."""
    from oracle.cacc_ref import gather_line
    tol = dict(rtol=1e-5, atol=1e-6)
    for E in (1, 13, 77, 1000):
        for coop_gamma, train_mode, compact in ((-1, True, False), (0.9, True, True), (-1, False, True), (0.9, False, False)):
            rng = np.random.RandomState(1000 * N + E)
            env = make_env(N, E, scenario, coop_gamma=coop_gamma, train_mode=train_mode, compact=compact)
            ref = oracle_for(env)
            _random_state(ref, env, rng, scenario)
            acts = rng.randint(0, 4, size=(E, N)).astype(np.uint8)
            obs, r, d, g = env.step(torch.from_numpy(acts).cuda())
            ro, rr, rd, rg = ref.step(acts)
            ok = np.abs(ref.h.min(axis=1) - 1.0) > 1e-4          # fp32 flip zone of the collision test
            print('N %d E %d kept %.4f' % (N, E, ok.mean()))
            assert ok.mean() > 0.99
            assert r.shape == ((E, N) if coop_gamma >= 0 else (E,))
            np.testing.assert_allclose(env.h.cpu().numpy()[ok], ref.h[ok], **tol)
            np.testing.assert_allclose(env.v.cpu().numpy()[ok], ref.v[ok], **tol)
            np.testing.assert_allclose(env.u.cpu().numpy()[ok], ref.u[ok], rtol=1e-5, atol=2e-5)  # (v'-v)/dt cancels
            np.testing.assert_allclose(g.cpu().numpy()[ok], rg[ok], rtol=1e-5, atol=1e-3)
            np.testing.assert_allclose(r.cpu().numpy()[ok], rr[ok], rtol=1e-5, atol=1e-3)
            assert np.array_equal(d.cpu().numpy()[ok].astype(bool), rd[ok])
            assert np.array_equal(env.collided.cpu().numpy()[ok].astype(bool), ref.collided[ok])
            assert np.array_equal(env.t.cpu().numpy(), ref.t)
            want = ro if compact else gather_line(ro)
            np.testing.assert_allclose(obs.cpu().numpy()[ok], want[ok], rtol=1e-5, atol=2e-5)


# ------------------------------------------------------------------------------------------------ (3) padding lanes are inert
SENT_F, SENT_I, SENT_B = -777.25, -123456789, 0xAB


def _guarded(shape, dtype, front):
    """A tensor of `shape` inside a larger buffer filled with a sentinel, `front` elements in (so its address has no alignment
    beyond the element's) -> (view, buffer, slice of the view in the buffer)."""
    n = int(np.prod(shape))
    sent = {torch.float32: SENT_F, torch.int32: SENT_I, torch.uint8: SENT_B}[dtype]
    buf = torch.full((front + n + 131,), sent, dtype=dtype, device='cuda')
    return buf[front:front + n].view(*shape), buf, slice(front, front + n), sent


@pytest.mark.parametrize('compact', [False, True])
@pytest.mark.parametrize('N,E', [(2, 1), (2, 77), (3, 13), (5, 77), (7, 13), (12, 1), (12, 77), (17, 13), (25, 77), (32, 13), (31, 1000)])
def test_padding_and_tail_lanes_write_nothing(N, E, compact):
    """State and outputs live inside sentinel-filled buffers at odd offsets.  After a reset (all, masked) and steps (with the
    fused auto-reset: T = 10) every element outside [E,N,.] still holds the sentinel: the lanes a >= N of a group and the lanes
    of replicas >= E store nothing, the observation slab ends where the batch ends."""
    cp = platoon_config(N, 'ia2c', 'slowdown', coop_gamma=0.9)
    cp['ENV_CONFIG']['episode_length_sec'] = '1'
    from deeprl_network_amd.envs.cacc_env import CACCBatchEnv
    env = CACCBatchEnv(cp['ENV_CONFIG'], num_envs=E)
    if compact:
        env.set_compact_obs(True)
    guards = []
    for k, (name, front) in enumerate([('h', 1), ('v', 3), ('u', 5), ('t', 7), ('collided', 9), ('v0_init', 11), ('obs', 13),
                                       ('reward', 15), ('done', 17), ('global_reward', 19), ('episode', 21), ('fp', 23)]):
        old = getattr(env, name)
        view, buf, sl, sent = _guarded(tuple(old.shape), old.dtype, front)
        setattr(env, name, view)
        guards.append((name, buf, sl, sent))
    aview, abuf, asl, asent = _guarded((E, N), torch.uint8, 3)
    env.episode.zero_()

    def intact(what):
        torch.cuda.synchronize()
        for name, buf, sl, sent in guards:
            b = buf.cpu()
            assert bool((b[:sl.start] == sent).all()) and bool((b[sl.stop:] == sent).all()), '%s: %s written outside [E,N,.]' % (what, name)
            if name not in ('reward', 'done', 'global_reward') or what.startswith('step'):
                inside = b[sl]
                assert not bool((inside == sent).all()), '%s: %s not written' % (what, name)

    env.reset()
    intact('reset')
    assert bool((env.t == 0).all()) and bool((env.fp == 0.25).all()) and bool((env.episode == 1).all())
    mask = torch.zeros(E, dtype=torch.uint8, device='cuda')
    mask[::2] = 1
    env.reset(mask=mask)
    intact('masked reset')
    g = torch.Generator().manual_seed(N * E)
    for k in range(11):
        aview.copy_(torch.randint(0, 4, (E, N), generator=g, dtype=torch.uint8))
        env.step(aview, auto_reset=True)
        intact('step %d' % k)
    assert int(env.episode.min()) >= 2 and bool(torch.isfinite(env.obs).all()) and bool((env.t == 1).all())


# ------------------------------------------------------------------------------------------------ (4) N = 8 through the new entries
def _step_nv(env, action, auto_reset):
    from deeprl_network_amd import _lib
    P = _lib.ptr
    rc = _lib.lib.nmarl_cacc_step_nv(
        ctypes.byref(env.params), env.E, P(action, torch.uint8), P(env.h), P(env.v), P(env.u), P(env.t), P(env.collided),
        P(env.v0_init), P(env.obs), P(env.reward), P(env.done), P(env.global_reward), 1 if auto_reset else 0, env.seed,
        env.env_id_base, P(env.episode), env.n_agent, _lib.stream())
    _lib.check(rc, 'nmarl_cacc_step_nv')


def _reset_nv(env, mask=None):
    from deeprl_network_amd import _lib
    P = _lib.ptr
    rc = _lib.lib.nmarl_cacc_reset_nv(
        ctypes.byref(env.params), env.E, P(mask, torch.uint8), None, env.seed, env.env_id_base, P(env.episode), P(env.h), P(env.v),
        P(env.u), P(env.t), P(env.collided), P(env.v0_init), P(env.obs), P(env.fp), env.n_a, env.n_agent, _lib.stream())
    _lib.check(rc, 'nmarl_cacc_reset_nv')


@pytest.mark.parametrize('compact', [False, True])
@pytest.mark.parametrize('scenario,coop_gamma', [('catchup', -1), ('slowdown', 0.9)])
@pytest.mark.parametrize('E', [13, 4096])
def test_eight_vehicles_through_the_new_entries_are_bit_identical(E, scenario, coop_gamma, compact):
    """nmarl_cacc_step_nv / nmarl_cacc_reset_nv with n_vehicle = 8 against nmarl_cacc_step / nmarl_cacc_reset: every output and
    every state tensor bit for bit over a reset, a masked reset and 5 steps, the third of which ends the episode (t = T: the fused
    auto-reset), with a fifth of the platoons collided and frozen."""
    a = make_env(8, E, scenario, coop_gamma=coop_gamma, compact=compact)
    b = make_env(8, E, scenario, coop_gamma=coop_gamma, compact=compact)
    names = ('h', 'v', 'u', 't', 'collided', 'v0_init', 'obs', 'reward', 'done', 'global_reward', 'episode', 'fp')

    def same(what):
        for n in names:
            assert torch.equal(getattr(a, n), getattr(b, n)), '%s: %s differs' % (what, n)

    a.reset()
    _reset_nv(b)
    same('reset')
    mask = torch.zeros(E, dtype=torch.uint8, device='cuda')
    mask[1::3] = 1
    a.reset(mask=mask)
    _reset_nv(b, mask)
    same('masked reset')
    g = torch.Generator().manual_seed(E)
    for env in (a, b):
        env.t.fill_(a.T - 3)
        env.collided[::5] = 1
        env.u[::5] = 0.75
    for k in range(5):
        act = torch.randint(0, 4, (E, 8), generator=g, dtype=torch.uint8).cuda()
        a.step(act, auto_reset=True)
        _step_nv(b, act, True)
        same('step %d' % k)
        assert bool(a.done.all()) == (k == 2)
    assert bool((a.episode == 2 + mask.int()).all()) and bool((a.t == 2).all())


# ------------------------------------------------------------------------------------------------ (5) Philox reset, fused auto-reset
@pytest.mark.parametrize('N', [3, 12])
def test_philox_reset_matches_oracle_contract(N):
    from oracle import philox
    E, base, seed = 1000, 123456, 12
    env = make_env(N, E, 'catchup', seed=seed, env_id_base=base)
    for episode in range(3):
        env.reset()
        U = philox.reset_uniform(seed, base + np.arange(E), episode)
        np.testing.assert_array_equal(env.h.cpu().numpy()[:, 0], (np.float32(20) * (np.float32(1.5) + U)))
        assert np.all(env.h.cpu().numpy()[:, 1:] == 20) and np.all(env.v.cpu().numpy() == 15)
    assert np.all(env.episode.cpu().numpy() == 3)
    env2 = make_env(N, E, 'slowdown', seed=seed, env_id_base=base)
    env2.reset()
    U = philox.reset_uniform(seed, base + np.arange(E), 0)
    np.testing.assert_array_equal(env2.v.cpu().numpy(), np.repeat((np.float32(15) * (np.float32(1.5) + U))[:, None], N, 1))
    np.testing.assert_array_equal(env2.v0_init.cpu().numpy(), env2.v.cpu().numpy()[:, 0])
    assert np.all(env2.h.cpu().numpy() == 20)
    # masked reset: only the selected replicas move on (tests/test_gpu_cacc.py::test_masked_reset_only_touches_selected)
    a = torch.full((E, N), 3, dtype=torch.uint8, device='cuda')
    for _ in range(7):
        env.step(a)
    h0, t0, ob0 = env.h.clone(), env.t.clone(), env.obs.clone()
    mask = torch.zeros(E, dtype=torch.uint8, device='cuda')
    mask[::3] = 1
    env.reset(mask=mask)
    keep = mask == 0
    assert torch.equal(env.h[keep], h0[keep]) and torch.equal(env.t[keep], t0[keep]) and torch.equal(env.obs[keep], ob0[keep])
    assert torch.all(env.t[mask == 1] == 0) and torch.all(env.h[mask == 1][:, 1:] == 20)
    assert torch.all(env.episode[mask == 1] == 4) and torch.all(env.episode[keep] == 3)
    U = philox.reset_uniform(seed, base + np.arange(E), 3)
    np.testing.assert_array_equal(env.h.cpu().numpy()[::3, 0], (np.float32(20) * (np.float32(1.5) + U))[::3])


@pytest.mark.parametrize('scenario', ['catchup', 'slowdown'])
@pytest.mark.parametrize('N', [3, 12])
def test_fused_auto_reset_at_the_episode_end(N, scenario):
    """t == T with auto_reset: reward / done of the last step, then the state, v0_init and observation of the NEXT episode, drawn
    from Philox(seed, env id, episode) with the episode counter bumped once per replica; replicas not done are left alone."""
    from oracle import philox
    from oracle.cacc_ref import gather_line
    E, base, seed = 77, 5000, 12
    env = make_env(N, E, scenario, seed=seed, env_id_base=base)
    ref = oracle_for(env)
    env.reset()
    ref.reset(philox.reset_uniform(seed, base + np.arange(E), 0))
    last = np.arange(E) % 2 == 0                               # every other replica stands one step before T
    env.t[::2] = env.T - 1
    ref.t[last] = ref.p.T - 1
    acts = np.random.RandomState(N).randint(0, 4, size=(E, N)).astype(np.uint8)
    obs, r, d, g = env.step(torch.from_numpy(acts).cuda(), auto_reset=True)
    ro, rr, rd, rg = ref.step(acts)
    assert np.array_equal(rd, last) and np.array_equal(d.cpu().numpy().astype(bool), rd)
    np.testing.assert_allclose(g.cpu().numpy(), rg, rtol=1e-5, atol=1e-3)
    ro = ref.reset(philox.reset_uniform(seed, base + np.arange(E), 1), mask=rd)
    np.testing.assert_array_equal(env.h.cpu().numpy()[last], ref.h[last])
    np.testing.assert_array_equal(env.v.cpu().numpy()[last], ref.v[last])
    np.testing.assert_array_equal(env.v0_init.cpu().numpy()[last], ref.v0_init[last])
    np.testing.assert_allclose(env.h.cpu().numpy(), ref.h, rtol=1e-5, atol=1e-6)
    assert np.array_equal(env.t.cpu().numpy(), ref.t) and not env.collided.any() and not env.u[::2].any()
    assert np.array_equal(env.episode.cpu().numpy(), 1 + last.astype(np.int32))
    np.testing.assert_allclose(obs.cpu().numpy(), gather_line(ro), rtol=1e-5, atol=2e-5)


# ------------------------------------------------------------------------------------------------ (6) duck-type, engine, CLI
@pytest.mark.parametrize('case', ['n5_slowdown_fp_random', 'n12_catchup_mild'])
def test_reference_duck_type_any_length(case):
    """`CACCEnv` (E = 1, the reference's own interface) at N = 5 ia2c_fp and N = 12 ma2c_nc: list-of-arrays observations with the
    fixture's widths and, with the fixture's fingerprints, its values over the whole trajectory; neighbour actions; traffic columns."""
    from deeprl_network_amd.envs.cacc_env import CACCEnv
    z = load_npz(os.path.join(GOLDEN, 'platoon_%s.npz' % case))
    N, agent = int(z['n_vehicle']), str(z['agent'])
    cp = platoon_config(N, agent, str(z['scenario']), int(z['seed']), float(z['coop_gamma']))
    env = CACCEnv(cp['ENV_CONFIG'])
    assert env.n_agent == N and list(env.n_a_ls) == [4] * N and np.array_equal(env.neighbor_mask, z['neighbor_mask'])
    env.init_data(True, False, '/nonexistent/')
    ob = env.reset()
    fps = z['fps']
    if agent == 'ia2c_fp':
        env.update_fingerprint(fps[0])
        ob = env._state_list()
    assert [len(o) for o in ob] == [int(x) for x in z['n_s']]
    nb = env.get_neighbor_action(np.arange(N) % 4)
    assert [list(x) for x in nb] == [[j % 4 for j in (i - 1, i + 1) if 0 <= j < N] for i in range(N)]
    for k, a in enumerate(z['acts']):
        if agent == 'ia2c_fp':
            env.update_fingerprint(fps[k + 1])
        ob, r, d, g = env.step(a)
        for i, o in enumerate(ob):
            np.testing.assert_allclose(o, z['obs'][k + 1, i, :len(o)], atol=2e-4, rtol=1e-4)
        np.testing.assert_allclose(g, z['global_reward'][k], rtol=1e-4, atol=1e-3)
        assert d == bool(z['done'][k])
    assert d and len(env.traffic_data) == 1
    cols = set(env.traffic_data[0].columns)
    assert {'headway_%d_m' % N, 'velocity_%d_mps' % N, 'accel_%d_mps2' % N, 'headway_1_m'} <= cols and 'headway_%d_m' % (N + 1) not in cols


def test_every_shipped_cacc_ini_constructs_unchanged():
    from deeprl_network_amd.envs.cacc_env import CACCBatchEnv
    inis = sorted(glob.glob(os.path.join(ROOT, 'config', '*catchup*.ini')) + glob.glob(os.path.join(ROOT, 'config', '*slowdown*.ini')))
    assert len(inis) >= 7
    for f in inis:
        cp = configparser.ConfigParser()
        cp.read(f)
        env = CACCBatchEnv(cp['ENV_CONFIG'], num_envs=5)
        assert env.n_agent == 8 and env.supports_fused_encode and env.reset().shape == (5, 8, 15)
        assert env.set_compact_obs(True) and env.inkernel_step()['obs_out'].shape == (5, 8, 5)


def _build_trainer(agent, N, E, use_graph, n_step=20):
    from deeprl_network_amd.envs import make_batch_env
    from deeprl_network_amd.main import init_agent
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    cp = platoon_config(N, agent, 'catchup', n_step=n_step, reward_norm=800.0 if agent.startswith('ia2c') else 5000.0)
    env = make_batch_env(cp['ENV_CONFIG'], num_envs=E)
    np.random.seed(12)
    model = init_agent(env, cp['MODEL_CONFIG'], 10 ** 9, 12, num_envs=E)
    return env, model, BatchedTrainer(env, model, Counter(10 ** 12, 10 ** 12, 10 ** 12), use_graph=use_graph)


def _replay_on_oracle(env, model, tr):
    """The first rollout on the fp32 oracle: Philox reset uniforms of episode 0, then the actions the policy drew (buf_act);
    compact observation, raw reward and done of every lock-step at the trajectory tolerances."""
    from oracle import philox
    E, T = env.E, tr.n_step
    assert tr.compact_obs and model.buf_x.shape[-1] == 5 and not tr.env_in_kernel and not tr.fused_encode
    ref = oracle_for(env)
    ref.reset(philox.reset_uniform(env.seed, env.env_id_base + np.arange(E), 0))
    acts, rraw, g = model.buf_act.cpu().numpy(), tr.buf_rraw.cpu().numpy(), tr.buf_g.cpu().numpy()
    done, X = model.buf_done_post.cpu().numpy().astype(bool), model.buf_x.cpu().numpy()
    near = 0
    for t in range(T):
        ro, rr, rd, rg = ref.step(acts[t])
        near += int((np.abs(ref.h.min(axis=1) - 1.0) < 1e-4).sum())
        assert np.array_equal(done[t], rd), t
        np.testing.assert_allclose(rraw[t], rr, rtol=1e-4, atol=1e-3)
        np.testing.assert_allclose(g[t], rg, rtol=1e-4, atol=1e-3)
        np.testing.assert_allclose(X[t + 1], ro, rtol=1e-4, atol=2e-4)
    assert near == 0 and not done.any()


@pytest.mark.parametrize('agent,N,E', [('ia2c', 3, 77), ('ia2c_fp', 5, 77), ('ma2c_cu', 12, 64), ('ma2c_nc', 12, 130), ('ma2c_ic3', 16, 64),
                                       ('ma2c_dial', 3, 77), ('ma2c_nc', 2, 13)])
def test_batched_engine_any_length(agent, N, E):
    """BatchedTrainer for two batches (n_step = 20) with an ini whose only change is n_vehicle, eager and with hipGraphs: actions,
    rewards and post-update weights bit-identical, finite losses, hand-off status 0, weights moved.  For NV != 8 a lock-step is
    the lock-step launch plus ONE env launch (no env step inside the launch, no encoders behind the env step)."""
    from deeprl_network_amd import ops
    runs = []
    for use_graph in (False, True):
        env, model, tr = _build_trainer(agent, N, E, use_graph)
        assert tr.N == N and not tr.env_in_kernel and not tr.fused_encode and not env.supports_fused_encode
        w0 = model.policy.params.flat.clone()
        rec = []
        for b in range(2):
            tr.run_batch()
            torch.cuda.synchronize()
            rec += [model.buf_act.clone(), tr.buf_rraw.clone(), tr.buf_g.clone(), model.policy.params.flat.clone()]
            assert all(bool(torch.isfinite(x).all()) for x in model.last_loss if torch.is_tensor(x))
            if b == 0 and not use_graph and (agent, N, E) in (('ia2c_fp', 5, 77), ('ma2c_nc', 12, 130)):
                _replay_on_oracle(env, model, tr)
        assert tr.handoff_fallbacks == 0 and int(ops.handoff_status(env.device)[0].item()) == 0
        assert bool(torch.isfinite(rec[-1]).all()) and not torch.equal(rec[-1], w0) and not torch.equal(rec[3], rec[-1])
        assert int(model.buf_act.max()) <= 3 and model.buf_act.shape == (20, E, N)
        runs.append(rec)
        del env, model, tr
    for k, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), 'hipGraph replay differs from eager launches (record %d)' % k


def test_cli_train_and_evaluate_a_twelve_car_platoon(tmp_path):
    """main.py train on an ini with n_vehicle = 12 -- the batched loop (--num-envs 64, three batches) and the E = 1 reference loop
    -- writes train_reward.csv and a checkpoint; main.py evaluate loads it and writes the traffic table with 12 vehicles."""
    import pandas as pd
    from deeprl_network_amd.main import main
    for num_envs, sub in ((64, 'batched'), (1, 'single')):
        cp = platoon_config(12, 'ma2c_nc', 'catchup', n_step=20, reward_norm=5000.0, total_step=60)
        cp['ENV_CONFIG']['episode_length_sec'] = '6'
        ini = tmp_path / ('config_%s.ini' % sub)
        with open(ini, 'w') as f:
            cp.write(f)
        base = str(tmp_path / sub)
        main(['--base-dir', base, 'train', '--config-dir', str(ini), '--num-envs', str(num_envs)])
        df = pd.read_csv(base + '/data/train_reward.csv')
        assert {'agent', 'step', 'avg_reward', 'std_reward'} <= set(df.columns) and len(df) >= 1 and np.isfinite(df['avg_reward']).all()
        assert len([f for f in os.listdir(base + '/model') if f.startswith('checkpoint-')]) == 1
        main(['--base-dir', base, 'evaluate', '--evaluation-seeds', '2000'])
        tdf = pd.read_csv(base + '/eva_data/catchup_ma2c_nc_traffic.csv')
        assert {'headway_12_m', 'velocity_12_mps', 'accel_12_mps2'} <= set(tdf.columns) and 'headway_13_m' not in tdf.columns

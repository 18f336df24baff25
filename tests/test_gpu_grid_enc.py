"""The input encoders of the uncoupled nets inside the policy + value launch on a GENERAL input layout (csrc/lstm_mfma.hip
lstm_step_x_kernel<3,0,3> / <3,0,4>; the 5 x 5 ATSC grid: 12 own features x (1 + 4 neighbour slots), 5 fingerprint entries x 4
neighbours): the op against a float64 restatement and against the separate encoder launch, what the launcher refuses, and the
batched engine (IA2C-FP, IA2C, ConseNet on LargeGridBatchEnv) with the encoders inside the launch against the separate ones."""
import os
import sys

import numpy as np
import pytest
import torch

from helpers import GOLDEN, build_product_batched, grid_config, load_npz, var_stats_from_named

pytestmark = pytest.mark.gpu

N_GRID, F_GRID, A_GRID, M_GRID, H = 25, 12, 5, 4, 64


def grid_nbrs():
    """The 5 x 5 grid's neighbour lists in the slab's (ascending) slot order: corners 2, edges 3, interior nodes 4."""
    out = []
    for i in range(N_GRID):
        r, c = divmod(i, 5)
        out.append(sorted(5 * rr + cc for rr, cc in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)) if 0 <= rr < 5 and 0 <= cc < 5))
    return out


def nbr_tables(nbrs, m_max):
    idx = -torch.ones(len(nbrs), max(m_max, 1), dtype=torch.int32)
    for i, lst in enumerate(nbrs):
        idx[i, :len(lst)] = torch.tensor(lst, dtype=torch.int32)
    return idx, torch.cat([torch.arange(len(nbrs), dtype=torch.int32).view(-1, 1), idx], dim=1)


def make_case(form, E, seed):
    """form 'fp': both encoders (IA2C-FP); 'ob': the observation encoder alone over [own | 4 neighbours] (IA2C); 'own': alone over the
    own features (ConseNet).  Weight rows of absent slots are zero, as ParamStore's masks leave them."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                         # noqa: E731
    N, F, A = N_GRID, F_GRID, A_GRID
    m = 0 if form == 'own' else M_GRID
    nbrs = grid_nbrs()
    KX = 2 * H if form == 'fp' else H
    rows = F * (1 + m)
    d = dict(form=form, E=E, m=m, nbrs=nbrs, KX=KX,
             ob=r(E, N, F), fp=torch.softmax(r(N, E, A), dim=-1),
             w_ob=r(N, rows, H) * 0.2 + torch.arange(rows).view(1, -1, 1) * 0.002, b_ob=r(N, H) * 0.2,
             w_fp=r(N, A * M_GRID, H) * 0.4 + torch.arange(H).view(1, 1, -1) * 0.003, b_fp=r(N, H) * 0.2,
             h=r(N, E, H) * 0.7, c=r(N, E, H), done=(torch.rand(E, generator=g) < 0.3).float(),
             wx=r(N, KX, 4 * H) * 0.15 + torch.arange(4 * H).view(1, 1, -1) * 1e-3 + torch.arange(KX).view(1, -1, 1) * 1e-3,
             wh=r(N, H, 4 * H) * 0.2 + torch.arange(4 * H).view(1, 1, -1) * 1e-3, b=r(N, 4 * H) * 0.1,
             pi_w=r(N, H, A) * 0.5, pi_b=r(N, A) * 0.3, v_w=r(N, H + M_GRID * A, 1), v_b=r(N, 1))
    for i in range(N):
        if m:
            d['w_ob'][i, F * (1 + len(nbrs[i])):] = 0
        d['w_fp'][i, A * len(nbrs[i]):] = 0
    d['idx'], d['idx_self'] = nbr_tables(nbrs, M_GRID)
    return d


def reference_f64(d):
    """float64 restatement: S = [relu(x~ W_ob + b) | relu(p~ W_fp + b)], the LSTM step (gate order i, f, o, u), the actor head, and the
    value re-step from the new state with the same input (the critic's h part; the neighbour-action term is deferred)."""
    f = lambda k: d[k].double()                                                          # noqa: E731
    N, E, m, nbrs = N_GRID, d['E'], d['m'], d['nbrs']
    ob, fp = f('ob'), f('fp')
    S = []
    for i in range(N):
        slots = [ob[:, i]] + [ob[:, nbrs[i][k]] if k < len(nbrs[i]) else torch.zeros(E, F_GRID, dtype=torch.float64) for k in range(m)]
        s = torch.relu(torch.cat(slots, dim=1) @ f('w_ob')[i] + f('b_ob')[i])
        if d['form'] == 'fp':
            ps = [fp[nbrs[i][k]] if k < len(nbrs[i]) else torch.zeros(E, A_GRID, dtype=torch.float64) for k in range(M_GRID)]
            s = torch.cat([s, torch.relu(torch.cat(ps, dim=1) @ f('w_fp')[i] + f('b_fp')[i])], dim=1)
        S.append(s)
    S = torch.stack(S)
    keep = (1.0 - f('done')).view(1, E, 1)

    def cell(h, c):
        z = torch.bmm(S, f('wx')) + torch.bmm(h * keep, f('wh')) + f('b').unsqueeze(1)
        gi, gf, go, gu = torch.sigmoid(z[..., :H]), torch.sigmoid(z[..., H:2 * H]), torch.sigmoid(z[..., 2 * H:3 * H]), torch.tanh(z[..., 3 * H:])
        c2 = gf * (c * keep) + gi * gu
        return torch.cat([gi, gf, go, gu], dim=-1), c2, go * torch.tanh(c2)
    gates, c1, h1 = cell(f('h'), f('c'))
    pi = torch.softmax(torch.bmm(h1, f('pi_w')) + f('pi_b').unsqueeze(1), dim=-1)
    _, _, h2 = cell(h1, c1)
    v = torch.bmm(h2, f('v_w')[:, :H]).squeeze(-1) + f('v_b')
    return dict(S=S, gates=gates, c=c1, h=h1, pi=pi, v=v)


SENT = -7.0


def device_buffers(d):
    """Every output as the middle slot of a sentinel-filled buffer of three: what lies in front of row 0 and behind row E - 1 shows."""
    N, E, KX = N_GRID, d['E'], d['KX']
    full = lambda *s: torch.full(s, SENT, device='cuda')                                 # noqa: E731
    return dict(S=full(N, 3, E, KX), h=full(N, 3, E, H), c=full(N, 3, E, H), gates=full(N, 3, E, 4 * H), pi=full(3, N, E, A_GRID),
                v=full(N, 3, E), act=torch.full((3, E, N), 99, dtype=torch.uint8, device='cuda'),
                bits=torch.full((N, 3, E, 4), 0x5a5a5a5a, dtype=torch.int32, device='cuda'))


def slot(o, k):
    return o[k][1] if k in ('pi', 'act') else o[k][:, 1]


def padding_untouched(o, written):
    for k, t in o.items():
        sent = 99 if k == 'act' else (0x5a5a5a5a if k == 'bits' else SENT)
        outer = [t[0], t[2]] if k in ('pi', 'act') else [t[:, 0], t[:, 2]]
        if not all(bool(torch.all(x == sent)) for x in outer):
            return False
        if k not in written and not bool(torch.all(t == sent)):
            return False
    return True


def launch(d, o, x, draw, precision='fp32'):
    from deeprl_network_amd import ops
    cu = lambda k: d[k].cuda()                                                           # noqa: E731
    img = ops.lstm_wimage(cu('wx'), cu('wh'), **({} if precision == 'fp32' else dict(precision=precision)))
    ops.lstm_step_policy_value(cu('h'), None, cu('b'), None, None, cu('c'), cu('done'), cu('pi_w'), cu('pi_b'), slot(o, 'pi'), slot(o, 'act'),
                               cu('v_w'), cu('v_b'), cu('idx'), A_GRID, slot(o, 'v'), xs=(x, None, img), h_out=slot(o, 'h'),
                               c_out=slot(o, 'c'), gates=slot(o, 'gates'), defer_action_term=True,
                               **({} if precision == 'fp32' else dict(precision=precision)), **draw)
    torch.cuda.synchronize()


def enc_spec(d, o, **over):
    from deeprl_network_amd import ops
    cu = lambda k: d[k].cuda()                                                           # noqa: E731
    two = d['form'] == 'fp'
    kw = dict(ob=cu('ob'), fp=cu('fp'), w_ob=cu('w_ob'), b_ob=cu('b_ob'), w_fp=cu('w_fp') if two else None, b_fp=cu('b_fp') if two else None,
              nbrs=d['nbrs'], out=slot(o, 'S'), bits=slot(o, 'bits') if two else None)
    kw.update(over)
    return ops.step_enc_spec(kw['ob'], kw['fp'], kw['w_ob'], kw['b_ob'], kw['w_fp'], kw['b_fp'], kw['nbrs'], out=kw['out'], bits=kw['bits'])


@pytest.mark.parametrize('E', [77, 130, 1000])
@pytest.mark.parametrize('form', ['fp', 'ob', 'own'])
def test_general_layout_encoders_inside_the_launch(form, E):
    """nmarl_lstm_step_x with enc on the grid's layout (N = 25, the real neighbour table: 2 / 3 / 4 neighbours): encoder output S,
    gates, c', h', pi and v against float64 at the tolerances of the CACC form's test (rtol 3e-5 / atol 5e-6; v: 1e-4 / 2e-5), the
    sign image == relu_bits_pack of the kernel's own S, padding and rows past E untouched; then the same inputs through the separate
    encoder launch (fc_fwd_multi) + the step on its output at rtol 2e-5 / atol 2e-6.  E: a partial 16-row strip, one row past a
    128-row block, many blocks."""
    from deeprl_network_amd import ops
    d = make_case(form, E, 1000 * E + len(form))
    ref = reference_f64(d)
    draw = dict(mode=1, seed=9, env_id_base=17, step=5)
    o = device_buffers(d)
    launch(d, o, enc_spec(d, o), draw)
    written = {'S', 'h', 'c', 'gates', 'pi', 'v', 'act'} | ({'bits'} if form == 'fp' else set())
    assert padding_untouched(o, written)
    if form == 'fp':
        assert torch.equal(slot(o, 'bits'), ops.relu_bits_pack(slot(o, 'S')))
    tol = dict(rtol=3e-5, atol=5e-6)
    for k in ('S', 'gates', 'c', 'h', 'pi'):
        err = (slot(o, k).cpu().double() - ref[k]).abs().max().item()
        print('%s E=%d %s: max abs err %.3g' % (form, E, k, err))
        torch.testing.assert_close(slot(o, k).cpu().double(), ref[k], msg=lambda m, k=k: '%s: %s' % (k, m), **tol)
    torch.testing.assert_close(slot(o, 'v').cpu().double(), ref['v'], rtol=1e-4, atol=2e-5)
    from oracle import ops_ref
    act_chk = torch.zeros(E, N_GRID, dtype=torch.uint8)
    ops_ref.sample_actions(slot(o, 'pi').cpu(), act_chk, **draw)
    assert torch.equal(slot(o, 'act').cpu(), act_chk)
    # the separate encoders + the xs = (S, ...) step
    cu = lambda k: d[k].cuda()                                                           # noqa: E731
    parts = [(cu('ob').transpose(0, 1), cu('w_ob'), cu('b_ob'), d['idx_self'].cuda() if d['m'] else None)]
    if form == 'fp':
        parts.append((cu('fp'), cu('w_fp'), cu('b_fp'), d['idx'].cuda()))
    S2 = ops.fc_fwd_multi(parts, ops.BIAS_RELU)
    o2 = device_buffers(d)
    launch(d, o2, S2, draw)
    same = dict(rtol=2e-5, atol=2e-6)
    torch.testing.assert_close(slot(o, 'S'), S2, **same)
    for k in ('gates', 'c', 'h', 'pi', 'v'):
        torch.testing.assert_close(slot(o, k), slot(o2, k), msg=lambda m, k=k: '%s: %s' % (k, m), **same)
    assert (slot(o, 'act') != slot(o2, 'act')).float().mean().item() < 1e-3         # a draw flips only where a uniform meets a CDF boundary
    # no output slot (the bootstrap step): same results, nothing of S or its sign image written
    o3 = device_buffers(d)
    launch(d, o3, enc_spec(d, o3, out=None, bits=None), draw)
    assert padding_untouched(o3, {'h', 'c', 'gates', 'pi', 'v', 'act'})
    for k in ('h', 'v', 'act'):
        assert torch.equal(slot(o3, k), slot(o, k))


def test_launcher_refuses_what_the_general_forms_cannot_do():
    """NMARL_EINVAL without a launch (every output stays at its sentinel): F no multiple of 4, more than 64 observation inputs, more
    than 32 fingerprint inputs, a neighbour index >= N, bf16x3."""
    from deeprl_network_amd import _lib
    E, N = 77, N_GRID
    d = make_case('fp', E, 5)
    g = torch.Generator().manual_seed(6)
    r = lambda *s: torch.randn(*s, generator=g).cuda()                                   # noqa: E731
    bad_nbrs = [list(x) for x in d['nbrs']]
    bad_nbrs[7][1] = N
    cases = {
        'F = 10': dict(ob=r(E, N, 10), w_ob=r(N, 50, H)),
        'F (1 + m_max) = 80': dict(ob=r(E, N, 16), w_ob=r(N, 80, H)),
        'A m_max = 36': dict(fp=torch.softmax(r(N, E, 9), dim=-1), w_fp=r(N, 36, H)),
        'neighbour index N': dict(nbrs=bad_nbrs),
    }
    draw = dict(mode=1, seed=9, env_id_base=17, step=5)
    for what, over in cases.items():
        o = device_buffers(d)
        with pytest.raises(_lib.NmarlError):
            launch(d, o, enc_spec(d, o, **over), draw)
        torch.cuda.synchronize()
        assert padding_untouched(o, set()), what
    o = device_buffers(d)
    with pytest.raises(_lib.NmarlError):
        launch(d, o, enc_spec(d, o), draw, precision='bf16x3')
    torch.cuda.synchronize()
    assert padding_untouched(o, set())


# --------------------------------------------------------------------------- the batched engine on the grid
AGENTS = ['ia2c_fp', 'ia2c', 'ma2c_cu']
SAME = dict(rtol=2e-5, atol=2e-6)          # tests/test_gpu_models.py: in-kernel encoders vs the separate ones


def build_trainer(agent, E, use_graph, n_step=5, **kw):
    from deeprl_network_amd.envs import make_batch_env
    from deeprl_network_amd.main import init_agent
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    cp = grid_config(agent=agent, n_step=n_step)
    env = make_batch_env(cp['ENV_CONFIG'], num_envs=E)
    np.random.seed(12)
    model = init_agent(env, cp['MODEL_CONFIG'], 10 ** 9, 12, num_envs=E)
    return env, model, BatchedTrainer(env, model, Counter(10 ** 12, 10 ** 12, 10 ** 12), use_graph=use_graph, **kw)


@pytest.mark.parametrize('agent', AGENTS)
def test_engine_runs_the_encoders_inside_the_launch_on_the_grid(agent, monkeypatch):
    """BatchedTrainer on LargeGridBatchEnv (E = 130, n_step = 5): enc_in_kernel is true (false with NMARL_INKERNEL_ENCODE=0); one
    eager lock-step from an identical snapshot in both arms: pi and v agree at rtol 2e-5 / atol 2e-6, the actions wherever the
    draw lies farther than 2.2e-5 from every interior CDF boundary (at most 1e-3 of the rows may be that close: four boundaries x
    2 x 2.2e-5 = 1.8e-4 expected); then graph == eager over 3 batches of the in-kernel arm, bit for bit, kernel nodes only."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import graph_nodes as G
    from deeprl_network_amd import ops
    from oracle import philox
    E, T = 130, 5
    env, model, tr = build_trainer(agent, E, False)
    assert tr.enc_in_kernel and model.policy.enc_in_kernel(E, True)
    tr._rollout()                            # a state worth comparing from: advanced recurrent state, non-uniform fingerprints
    torch.cuda.synchronize()
    snap = [t.clone() for t in env.state_tensors()] + [model.h_fw.clone(), model.c_fw.clone(), model.buf_x[T].clone(),
                                                       model.buf_fp[T].clone(), tr.step_dev.clone(), torch.zeros_like(tr.done_pre)]
    monkeypatch.setenv('NMARL_INKERNEL_ENCODE', '0')
    env2, model2, tr2 = build_trainer(agent, E, False)
    assert not tr2.enc_in_kernel and not model2.policy.enc_in_kernel(E, True)
    assert torch.equal(model.policy.params.flat, model2.policy.params.flat)
    got = []
    for e_, m_, t_, flag in ((env, model, tr, '1'), (env2, model2, tr2, '0')):
        monkeypatch.setenv('NMARL_INKERNEL_ENCODE', flag)
        t_._restore(snap)
        m_.t = 0
        m_.act(t_.done_pre, mode=ops.SAMPLE_PHILOX, seed=e_.seed, env_id_base=e_.env_id_base, step=0, step_dev=t_.step_dev)
        torch.cuda.synchronize()
        got.append((m_.buf_fp[1].clone(), m_.buf_vn[:, 0].clone(), m_.buf_act[0].clone()))
    (pi_a, v_a, act_a), (pi_b, v_b, act_b) = got
    torch.testing.assert_close(pi_a, pi_b, **SAME)
    torch.testing.assert_close(v_a, v_b, **SAME)
    N = model.n_agent
    u = philox.action_uniform(env.seed, env.env_id_base + np.arange(E), N, int(tr.step_dev.item()))              # [E,N]
    p = pi_a.double().cpu().numpy().transpose(1, 0, 2)
    cdf = np.cumsum(p, axis=-1)
    cdf = (cdf / cdf[..., -1:])[..., :-1]
    near = (np.abs(cdf - np.asarray(u, dtype=np.float64)[..., None]) <= 2.2e-5).any(-1)
    print('%s: %d of %d draws within 2.2e-5 of a CDF boundary' % (agent, near.sum(), near.size))
    assert near.mean() <= 1e-3
    assert np.array_equal(act_a.cpu().numpy()[~near], act_b.cpu().numpy()[~near])
    del env2, model2, tr2
    # graph == eager, in-kernel arm
    monkeypatch.setenv('NMARL_INKERNEL_ENCODE', '1')
    runs = []
    for use_graph in (True, False):
        e_, m_, t_ = build_trainer(agent, E, use_graph, keep_graphs=use_graph)
        assert t_.enc_in_kernel
        for _ in range(3):
            t_.run_batch()
        torch.cuda.synchronize()
        runs.append((m_.policy.params.flat.clone(), e_.state_tensors()[0].clone(), m_.buf_act.clone(), t_.R_end.clone()))
        if use_graph:
            assert t_.graph is not None and t_.update_capture_error is None
            graphs = {'rollout': t_.graph}
            if t_._upd is not None:
                graphs['update'] = t_._upd['grads']
                if t_._upd['apply'] is not None:
                    graphs['apply'] = t_._upd['apply']
            names = G.tensor_names(t_, m_, m_.policy, e_, m_.policy.params)
            for what, g in graphs.items():
                c = G.census(g)
                assert c.get('kernel', 0) > 0 and set(c) == {'kernel'}, '%s graph of %s: %s\n%s' % (what, agent, c, G.describe(g, names))
        del e_, m_, t_
    for a, b in zip(*runs):
        assert torch.equal(a, b), 'hipGraph replay differs from eager launches'
    assert torch.isfinite(runs[0][0]).all()


def drive(model, X, U, R, check_act=None):
    """One batch on the batched engine as helpers.drive_batched drives it: scripted compact observations, draws forced through the
    kernels' own sampling by the given uniforms, scripted rewards, ONE update.  -> (pi [T+1,N,E,A], actions [T,E,N])."""
    from deeprl_network_amd import ops
    T, E, dev = model.n_step, model.E, model.device
    assert model.enable_saved_activations() and model.enable_compact_obs()
    zero, one = torch.zeros(E, device=dev), torch.ones(E, device=dev)
    scratch = torch.zeros(E, model.n_agent, dtype=torch.uint8, device=dev)
    model.reset_states()
    model.t = 0
    for t in range(T):
        model.buf_x[t].copy_(X[t])
        d = one if t == 0 else zero
        model.buf_done_pre[t].copy_(d)
        model.act(d, mode=ops.SAMPLE_UNIFORM, u=U[t], done_is_zero=(t > 0))
        if check_act is not None:
            assert torch.equal(model.buf_act[t], check_act[t]), 'forced action draw failed at step %d' % t
        model.t = t + 1
    model.buf_x[T].copy_(X[T])
    v = model.bootstrap(zero, scratch, mode=ops.SAMPLE_UNIFORM, u=U[T], done_is_zero=True)
    pi = torch.cat([model.buf_fp[1:T + 1], model._pi_boot.unsqueeze(0)]).clone()
    act = model.buf_act[:T].clone()
    model.buf_done_post.zero_()
    model.load_rewards(R)
    model.update(v.clone().contiguous())
    torch.cuda.synchronize()
    return pi, act


@pytest.mark.parametrize('agent', AGENTS)
def test_update_behind_the_in_kernel_encoders_on_the_grid(agent, monkeypatch):
    """The same forced action and reward sequence through both arms (E = 4 replicas, 6 lock-steps, the 5 x 5 grid's shapes), one
    update each: the weights agree at rtol 2e-5 / atol 2e-6 (tests/test_gpu_models.py's bound for in-kernel vs separate encoders),
    and IA2C-FP's update took fc_concat's bits= path (the sign image the rollout's kernel wrote)."""
    from deeprl_network_amd import ops
    zg = load_npz(os.path.join(GOLDEN, 'nnb_ma2c_nc_grid.npz'))
    T, K = 6, 4
    z = dict(agent=agent, topo='grid', n_step=T, seed=7, K=K, reward_norm=2000.0, nb=zg['nb'], dist=zg['dist'])
    g = torch.Generator().manual_seed(11)
    N = z['nb'].shape[0]
    X = torch.randn(T + 1, K, N, F_GRID, generator=g).cuda()
    R = (torch.randn(T, K, generator=g) * 100).cuda()
    want = torch.randint(0, A_GRID, (T + 1, K, N), generator=g)
    # the policies do not depend on the draws (no cross-agent recurrence): a first pass fixes them, the uniforms then sit in the middle
    # of the wanted action's CDF interval
    monkeypatch.setenv('NMARL_INKERNEL_ENCODE', '0')
    probe = build_product_batched(z, 'cuda')
    pi0, _ = drive(probe, X, [torch.full((K, N), 0.5, device='cuda')] * (T + 1), R)
    cdf = torch.cumsum(pi0.double().cpu().permute(0, 2, 1, 3), dim=-1)                       # [T+1,K,N,A]
    cdf = cdf / cdf[..., -1:]
    hi = torch.gather(cdf, -1, want.unsqueeze(-1)).squeeze(-1)
    lo = torch.where(want > 0, torch.gather(cdf, -1, (want - 1).clamp(min=0).unsqueeze(-1)).squeeze(-1), torch.zeros_like(hi))
    U = [(0.5 * (lo[t] + hi[t])).float().cuda() for t in range(T + 1)]
    wanted = want[:T].to(torch.uint8).cuda()
    calls = []
    orig = ops.fc_concat

    def spy(parts, act, saved=None, bits=None):
        calls.append((saved is not None, bits is not None))
        return orig(parts, act, saved=saved, bits=bits)
    monkeypatch.setattr(ops, 'fc_concat', spy)
    stats = {}
    for flag in ('1', '0'):
        monkeypatch.setenv('NMARL_INKERNEL_ENCODE', flag)
        del calls[:]
        model = build_product_batched(z, 'cuda')
        assert model.policy.enc_in_kernel(K, True) == (flag == '1')
        drive(model, X, U, R, check_act=wanted)
        assert torch.isfinite(model.policy.params.flat).all()
        stats[flag] = (var_stats_from_named(model.policy.params.ref_variables()), list(calls))
    np.testing.assert_allclose(stats['1'][0], stats['0'][0], rtol=SAME['rtol'], atol=SAME['atol'])
    assert stats['1'][1] and all(saved for saved, _ in stats['1'][1])
    if agent == 'ia2c_fp':
        assert any(bits for _, bits in stats['1'][1]), 'the update did not get the sign image of the rollout'
        assert not any(bits for _, bits in stats['0'][1])

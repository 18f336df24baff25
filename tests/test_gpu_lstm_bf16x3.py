"""The opt-in bf16x3 mode of the uncoupled nets' lock-step (csrc/lstm_mfma.hip chunk_bf16x3, lstm_wimage_bf16x3_kernel): the split
image bit for bit, the new step entry points against a float64 emulation of the split products and against exact float64, and the
IA2C-FP catch-up rollout under it (graph = eager, deterministic, kernel nodes only, actions close to the fp32 run's)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

from helpers import cacc_config  # noqa: E402
from step_edge_checks import _cell, _check, _emul, _split  # noqa: E402,F401  (the split emulation and its bounds live with the edge checks)

pytestmark = pytest.mark.gpu

H, CH, PITCH, CHUNK = 64, 32, 132, 10240


def _image_ref(w):
    """Expected split image [N, 2 (K*320)] int16 of w = [wx; wh] [N,K,4H] (layout of nmarl_lstm_wimage with precision 1)."""
    N, K, _ = w.shape
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    out = torch.zeros(N, 2 * K * 320, dtype=torch.int16)
    gc, q = np.meshgrid(np.arange(64), np.arange(128), indexing='ij')
    grp, c, t, hl, jp = gc >> 4, gc & 15, q >> 3, (q >> 2) & 1, q & 3
    col = (t >> 2) * H + 4 * c + (t & 3)
    for ch in range(K // CH):
        for e in range(2):
            j = 2 * jp + e
            k = ch * CH + np.where(j < 4, 4 * grp + j, 16 + 4 * grp + j - 4)
            pos = torch.from_numpy((2 * (ch * CHUNK + gc * PITCH + q) + e).ravel())
            kk, cc, hh = (torch.from_numpy(v.ravel()) for v in (k, col, hl))
            val = torch.where(hh.bool().view(1, -1), lo[:, kk, cc].view(torch.int16), hi[:, kk, cc].view(torch.int16))
            out[:, pos] = val
    return out


@pytest.mark.parametrize('N,KX', [(8, 128), (3, 64), (2, 0), (1, 256)])
def test_split_image_is_bf16_rne_hi_lo_bit_for_bit(N, KX):
    from deeprl_network_amd import ops
    g = torch.Generator().manual_seed(N + KX)
    wx = torch.randn(N, KX, 4 * H, generator=g) * 0.3 if KX else None
    wh = torch.randn(N, H, 4 * H, generator=g) * 0.3
    wh[0, 0, :6] = torch.tensor([0.0, -0.0, 1e-30, 3.0e38, 1.0 + 2 ** -9, -(1.0 + 3 * 2 ** -9)])     # tiny, huge, exact ties
    img = ops.lstm_wimage(None if wx is None else wx.cuda(), wh.cuda(), precision='bf16x3')
    assert img.dtype == torch.bfloat16 and img.shape == (N, 2 * (KX + H) * 320)
    w = wh if wx is None else torch.cat([wx, wh], dim=1)
    assert torch.equal(img.cpu().view(torch.int16), _image_ref(w))
    with pytest.raises(Exception):
        ops.lstm_wimage(None if wx is None else wx.cuda(), wh.cuda(), precision='bf16')


def _case(N, E, KX, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                          # noqa: E731
    return dict(x=torch.relu(r(N, E, KX)), h=torch.tanh(r(N, E, H)), c=r(N, E, H), done=(torch.rand(E, generator=g) < 0.2).float(),
                wx=r(N, KX, 4 * H) * 0.15, wh=r(N, H, 4 * H) * 0.2, b=r(N, 4 * H) * 0.1, pi_w=r(N, H, 4) * 0.5, pi_b=r(N, 4) * 0.3,
                v_w=r(N, H + 2 * 4, 1), v_b=r(N, 1))


@pytest.mark.parametrize('E', [77, 1000, 4096])
@pytest.mark.parametrize('entry', ['step_x', 'step_x_enc'])
def test_bf16x3_step_is_the_split_product(E, entry):
    """nmarl_lstm_step_x with precision 1 (policy + value, kind 3), without and with enc (<3,0,1>: encoders inside): the policy
    step's gates, c', h' vs the float64 split emulation (fp32 accumulation bound 2^-20 sum|a||b|) and vs exact float64 (split
    bound); the fp32 kernel is >= 10x farther from the emulation than the bf16x3 one; the draw follows the kernel's pi; the value
    re-step is the split product too."""
    from deeprl_network_amd import ops
    from oracle import ops_ref
    N, A, KX = 8, 4, 128
    d = _case(N, E, KX, E + (7 if entry == 'step_x_enc' else 0))
    cu = lambda t: t.cuda()                                                                 # noqa: E731
    draw = dict(mode=1, seed=5, env_id_base=40, step=3)
    img3 = ops.lstm_wimage(cu(d['wx']), cu(d['wh']), precision='bf16x3')
    img = ops.lstm_wimage(cu(d['wx']), cu(d['wh']))
    nbrs = [[j for j in (i - 1, i + 1) if 0 <= j < N] for i in range(N)]
    idx = -torch.ones(N, 2, dtype=torch.int32)
    for i, lst in enumerate(nbrs):
        idx[i, :len(lst)] = torch.tensor(lst, dtype=torch.int32)
    g = torch.Generator().manual_seed(E)
    ob, fp = torch.randn(E, N, 5, generator=g), torch.softmax(torch.randn(N, E, A, generator=g), dim=-1)
    w_ob, b_ob = torch.randn(N, 15, H, generator=g) * 0.4, torch.randn(N, H, generator=g) * 0.2
    w_fp, b_fp = torch.randn(N, 8, H, generator=g) * 0.4, torch.randn(N, H, generator=g) * 0.2
    for i in range(N):
        w_ob[i, 5 * (1 + len(nbrs[i])):] = 0
        w_fp[i, 4 * len(nbrs[i]):] = 0

    def run(image, precision):
        hg, cg = cu(d['h']), cu(d['c'])
        ho, co, gg = torch.empty_like(hg), torch.empty_like(cg), torch.empty(N, E, 4 * H, device='cuda')
        pig, actg, vg = torch.zeros(N, E, A, device='cuda'), torch.zeros(E, N, dtype=torch.uint8, device='cuda'), torch.zeros(N, E, device='cuda')
        S = torch.zeros(N, E, KX, device='cuda')
        if entry == 'step_x':
            S.copy_(d['x'])
            x = S
        else:
            x = ops.step_enc_spec(cu(ob), cu(fp), cu(w_ob), cu(b_ob), cu(w_fp), cu(b_fp), nbrs, out=S)
        ops.lstm_step_policy_value(hg, None, cu(d['b']), None, None, cg, cu(d['done']), cu(d['pi_w']), cu(d['pi_b']), pig, actg,
                                   cu(d['v_w']), cu(d['v_b']), cu(idx), A, vg, xs=(x, None, image), h_out=ho, c_out=co, gates=gg,
                                   defer_action_term=True, precision=precision, **draw)
        torch.cuda.synchronize()
        return S.cpu(), gg, co, ho, pig, actg, vg

    S, G3, C3, H3, pi3, act3, v3 = run(img3, 'bf16x3')
    S32, G32, C32, H32, _, _, _ = run(img, 'fp32')
    assert torch.equal(S, S32)                           # the encoders stay fp32 (and the same)
    keep = (1.0 - d['done']).double().view(1, E, 1)
    hk = (d['h'] * (1.0 - d['done']).view(1, E, 1))      # the kernel masks h in fp32, then splits
    A_in = torch.cat([S, hk], dim=2)
    W = torch.cat([d['wx'], d['wh']], dim=1)
    z_e, absum = _emul(A_in, W)
    z_e = z_e + d['b'].double().view(N, 1, -1)
    z_x = torch.bmm(A_in.double(), W.double()) + d['b'].double().view(N, 1, -1)
    c = d['c'].double()
    _check(G3, C3, H3, z_e, c, keep, 2.0 ** -20 * absum, 'bf16x3 vs split emulation')
    _check(G3, C3, H3, z_x, c, keep, (3 * 2.0 ** -18 + 2.0 ** -20) * absum, 'bf16x3 vs exact float64')
    ge, _, _ = _cell(z_e, c, keep)
    d3 = float(((G3.cpu().double() - ge) ** 2).mean().sqrt())
    d32 = float(((G32.cpu().double() - ge) ** 2).mean().sqrt())
    assert d32 >= 10 * d3, 'fp32 kernel %.3g vs bf16x3 kernel %.3g from the split emulation' % (d32, d3)
    act_chk = torch.zeros(E, N, dtype=torch.uint8)
    ops_ref.sample_actions(pi3.cpu(), act_chk, **draw)
    assert torch.equal(act3.cpu(), act_chk)
    # value re-step from the kernel's own h': the same x-side part + split(h' keep) @ Wh, critic on h'' (action term deferred)
    h1 = H3.cpu() * (1.0 - d['done']).view(1, E, 1)
    zx_e, absx = _emul(S, d['wx'])
    zh_e, absh = _emul(h1, d['wh'])
    _, _, h2 = _cell(zx_e + zh_e + d['b'].double().view(N, 1, -1), C3.cpu().double(), keep)
    v_e = torch.bmm(h2, d['v_w'][:, :H].double()).squeeze(-1) + d['v_b'].double()
    vb = (d['v_w'][:, :H].double().abs().sum(dim=1) * (3 * (2.0 ** -20 * (absx + absh).max()) + 1e-5)).view(N, 1)
    assert bool(((v3.cpu().double() - v_e).abs() <= vb).all())


def test_bf16x3_refuses_the_message_term_and_fp32_only_paths():
    from deeprl_network_amd import _lib, ops
    N, E = 2, 16
    d = _case(N, E, 64, 1)
    cu = lambda t: t.cuda()                                                                 # noqa: E731
    img = ops.lstm_wimage(cu(d['wx']), cu(d['wh']))
    img3 = ops.lstm_wimage(cu(d['wx']), cu(d['wh']), precision='bf16x3')
    hg, cg = cu(d['h']), cu(d['c'])
    with pytest.raises(_lib.NmarlError):           # fp32 image under bf16x3 (and vice versa): refused, not misread
        ops.lstm_step_fused(hg, None, cu(d['b']), None, None, cg, cu(d['done']), None, cg, hg, xs=(cu(d['x']), None, img), precision='bf16x3')
    with pytest.raises(_lib.NmarlError):
        ops.lstm_step_fused(hg, None, cu(d['b']), None, None, cg, cu(d['done']), None, cg, hg, xs=(cu(d['x']), None, img3))
    with pytest.raises(_lib.NmarlError):           # no image given: the KX = 0 compatibility form builds an fp32 one
        ops.lstm_step_fused(hg, cu(d['wh']), cu(d['b']), cu(torch.zeros(N, E, 4 * H)), None, cg, cu(d['done']), None, cg, hg, precision='bf16x3')
    # HEAD 0 (no heads) under bf16x3 runs and is close to fp32
    h0, c0 = cu(d['h']), cu(d['c'])
    ops.lstm_step_fused(h0, None, cu(d['b']), None, None, c0, cu(d['done']), None, c0, h0, xs=(cu(d['x']), None, img3), precision='bf16x3')
    ops.lstm_step_fused(hg, None, cu(d['b']), None, None, cg, cu(d['done']), None, cg, hg, xs=(cu(d['x']), None, img))
    torch.testing.assert_close(h0, hg, rtol=0, atol=2e-3)


def _build(agent, E, use_graph, precision, n_step=60, **kw):
    from deeprl_network_amd.envs import make_batch_env
    from deeprl_network_amd.main import init_agent
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    cp = cacc_config(agent=agent, scenario='catchup', n_step=n_step, reward_norm=800.0)
    cp['MODEL_CONFIG']['lstm_precision'] = precision
    env = make_batch_env(cp['ENV_CONFIG'], num_envs=E)
    np.random.seed(12)
    model = init_agent(env, cp['MODEL_CONFIG'], 10 ** 9, 12, num_envs=E)
    assert model.policy.precision == precision
    return env, model, BatchedTrainer(env, model, Counter(10 ** 12, 10 ** 12, 10 ** 12), use_graph=use_graph, **kw)


def test_ia2c_fp_catchup_under_bf16x3():
    """IA2C-FP catch-up, 8 x 4096, 3 batches under bf16x3: hipGraph = eager, two runs identical, every captured graph holds
    kernel nodes only; against fp32 the first lock-step's actions agree >= 99.9 %, the first batch's >= 98 %."""
    import graph_nodes as Gn
    E = 4096
    env, model, tr = _build('ia2c_fp', E, True, 'fp32')
    tr.run_batch()
    torch.cuda.synchronize()
    act32 = model.buf_act.clone()
    del env, model, tr
    runs = []
    for use_graph in (True, False, True):
        env, model, tr = _build('ia2c_fp', E, use_graph, 'bf16x3', keep_graphs=use_graph)
        acts = []
        for _ in range(3):
            tr.run_batch()
            acts.append(model.buf_act.clone())
        torch.cuda.synchronize()
        assert tr.handoff_fallbacks == 0
        if use_graph and not runs:
            assert tr.graph is not None and tr._upd is not None and tr.update_capture_error is None
            graphs = {'rollout': tr.graph, 'update': tr._upd['grads']}
            if tr._upd['apply'] is not None:
                graphs['apply'] = tr._upd['apply']
            for what, g in graphs.items():
                cen = Gn.census(g)
                assert cen.get('kernel', 0) > 0 and set(cen) == {'kernel'}, '%s graph holds non-kernel nodes: %s' % (what, cen)
        runs.append([model.policy.params.flat.clone(), env.state_tensors()[0].clone(), tr.R_end.clone()] + acts)
        del env, model, tr
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b), 'bf16x3: hipGraph replay differs from eager launches'
    for a, b in zip(runs[0], runs[2]):
        assert torch.equal(a, b), 'bf16x3: two identical runs differ'
    assert torch.isfinite(runs[0][0]).all()
    act3 = runs[0][3]
    first = float((act3[0] == act32[0]).float().mean())
    whole = float((act3 == act32).float().mean())
    assert first >= 0.999 and whole >= 0.98, 'action agreement with fp32: first lock-step %.5f, first batch %.5f' % (first, whole)


@pytest.mark.parametrize('E', [4096, 77])
def test_bf16x3_env_step_inside_the_launch_is_the_env_kernel(E, monkeypatch):
    """<3,0,1,0,1> stepping the env behind its draw = the same launch without it followed by nmarl_cacc_step: bit-identical."""
    out = []
    for inside in ('1', '0'):
        monkeypatch.setenv('NMARL_INKERNEL_ENV', inside)
        env, model, tr = _build('ia2c_fp', E, True, 'bf16x3', n_step=20)
        assert tr.enc_in_kernel and tr.env_in_kernel == (inside == '1')
        rec = []
        for _ in range(2):
            tr.run_batch()
            rec += [model.buf_act.clone(), tr.buf_rraw.clone(), model.buf_done_post.clone(), model.buf_x.clone()]
        tr.flush()
        torch.cuda.synchronize()
        out.append(rec + [env.h.clone(), env.v.clone(), env.u.clone(), env.t.clone(), env.collided.clone(), model.buf_v.clone(),
                          model.policy.params.flat.clone()])
        del env, model, tr
    for k, (a, b) in enumerate(zip(*out)):
        assert torch.equal(a, b), 'item %d differs between the in-launch env step and the env kernel (bf16x3)' % k

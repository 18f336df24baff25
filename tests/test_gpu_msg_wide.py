"""lstm_comm's message term inside the step kernel for three and four neighbour slots (K = 64 m_max = 192 / 256: the ATSC grid's
NeurComm): the launch-per-step forms lstm_step_x_kernel<1,1> / <2,1> take the neighbours' rows in two rounds of two slots and
stream W_msg through LDS in two 128-row halves.  Step parity against the float64 restatement, the launcher's refusals, and the
policy on the 5 x 5 grid against its own fallback (gather + fc launches)."""
import functools
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, build_product_batched, load_npz

pytestmark = pytest.mark.gpu

H = 64
DRAW = dict(mode=2, seed=5, env_id_base=40, step=3)
CASES = [(25, 130, 5, 4), (5, 127, 4, 3), (6, 17, 4, 4)]


def ragged_table(N, m_max):
    """-1 padded, ascending: agent i has i % (m_max + 1) neighbours -- none, one, two (the whole second round absent), three, (four)."""
    idx = -torch.ones(N, m_max, dtype=torch.int32)
    for i in range(N):
        cnt = i % (m_max + 1)
        nb = sorted({(i + 1 + 2 * k) % N for k in range(N)} - {i})[:cnt]
        if nb:
            idx[i, :len(nb)] = torch.tensor(nb, dtype=torch.int32)
    return idx


@functools.lru_cache(maxsize=None)
def case(N, E, A, m_max):
    """Operands (as test_gpu_ops.test_lstm_step_x_in_kernel_message_term sets them up, KX = 192) and the float64 reference of the
    policy step and of the value step from its new state; computed once, read-only."""
    from oracle import ops_ref
    g = torch.Generator().manual_seed(N * 13 + E + 1)
    r = lambda *s: torch.randn(*s, generator=g)                                         # noqa: E731
    KXg, KX, Km = 2 * H, 3 * H, H * m_max
    o = dict(N=N, E=E, A=A, m_max=m_max, KXg=KXg, KX=KX)
    o['h'], o['c'], o['done'] = r(N, E, H) * 0.7, r(N, E, H), (torch.rand(E, generator=g) < 0.3).float()
    o['xg'] = torch.relu(r(N, E, KXg))
    o['wx'] = r(N, KX, 4 * H) * 0.15 + torch.arange(4 * H).view(1, 1, -1) * 1e-3 + torch.arange(KX).view(1, -1, 1) * 1e-3
    o['wh'], o['b'] = r(N, H, 4 * H) * 0.2, r(N, 4 * H) * 0.1
    o['w_msg'] = r(N, Km, H) * 0.2 + torch.arange(H).view(1, 1, -1) * 2e-3 + torch.arange(Km).view(1, -1, 1) * 1e-3
    o['b_msg'] = r(N, H) * 0.2
    o['pi_w'], o['pi_b'], o['v_w'], o['v_b'] = r(N, H, A) * 0.5, r(N, A) * 0.3, r(N, H + m_max * A, 1), r(N, 1)
    o['idx'] = idx = ragged_table(N, m_max)
    f64 = lambda t: t.double()                                                           # noqa: E731
    ref = dict(hm=torch.zeros(N, E, H, dtype=torch.float64), h=torch.empty(N, E, H, dtype=torch.float64),
               c=torch.empty(N, E, H, dtype=torch.float64), pi=torch.zeros(N, E, A, dtype=torch.float64),
               act=torch.zeros(E, N, dtype=torch.uint8), gates=torch.zeros(N, E, 4 * H, dtype=torch.float64))
    msg_r = dict(kind=1, nbr_idx=idx, w_msg=f64(o['w_msg']), b_msg=f64(o['b_msg']), enc=None, out=ref['hm'])
    ops_ref.lstm_step_policy(f64(o['h']), f64(o['wh']), f64(o['b']), None, None, f64(o['c']), f64(o['done']), ref['c'], ref['h'],
                             f64(o['pi_w']), f64(o['pi_b']), ref['pi'], ref['act'], xs=(f64(o['xg']), f64(o['wx']), None, None, msg_r),
                             gates=ref['gates'], **DRAW)
    o['ref'], o['msg_r'] = ref, msg_r
    return o


def test_tables_cover_every_neighbour_count():
    counts = set()
    for N, _, _, m_max in CASES:
        counts |= {int(n) for n in (ragged_table(N, m_max) >= 0).sum(1)}
    assert counts == {0, 1, 2, 3, 4}
    assert {int(n) for n in (ragged_table(5, 3) >= 0).sum(1)} == {0, 1, 2, 3}


@pytest.mark.parametrize('N,E,A,m_max', CASES)
def test_step_parity(N, E, A, m_max):
    """Policy step (hm stored into the last third of the S slot) and value step (S untouched) with the in-kernel message term at
    K = 192 / 256 vs oracle.ops_ref in float64.  Bounds: hm at the narrow test's rtol 5e-5 / atol 1e-5; gates, c', h', pi at rtol
    1e-4 / atol 1e-5; v -- a 64-term dot product of h'' with unit-variance weights, so its absolute error is ~8 x that of h'' --
    at rtol 1e-4 / atol 5e-5 (the narrow test's atol)."""
    from deeprl_network_amd import ops
    from oracle import ops_ref, philox
    o = case(N, E, A, m_max)
    ref, idx, KXg, KX = o['ref'], o['idx'], o['KXg'], o['KX']
    cu = lambda t: t.cuda()                                                              # noqa: E731
    f64 = lambda t: t.double()                                                           # noqa: E731
    assert ops.msg_supported(ops.MSG_GATHER_RELU, m_max, H)
    img, mimg = ops.lstm_wimage(cu(o['wx']), cu(o['wh'])), ops.lstm_msg_wimage(cu(o['w_msg']))
    slot = torch.zeros(N, E, KX, device='cuda')
    slot[:, :, :KXg].copy_(o['xg'])
    msg_g = dict(kind=1, nbr_idx=cu(idx), w_msg=cu(o['w_msg']), b_msg=cu(o['b_msg']), img=mimg, enc=None, out=slot[:, :, KXg:])
    hg, cg = torch.zeros(N, E, H, device='cuda'), torch.zeros(N, E, H, device='cuda')
    pig, actg = torch.zeros(N, E, A, device='cuda'), torch.zeros(E, N, dtype=torch.uint8, device='cuda')
    gg = torch.zeros(N, E, 4 * H, device='cuda')
    ops.lstm_step_policy(cu(o['h']), None, cu(o['b']), None, None, cu(o['c']), cu(o['done']), cg, hg, cu(o['pi_w']), cu(o['pi_b']),
                         pig, actg, xs=(slot[:, :, :KXg], None, img, None, msg_g), gates=gg, **DRAW)
    torch.cuda.synchronize()
    err = lambda a, b: float((a.cpu().double() - b).abs().max())                         # noqa: E731
    print('max abs err: hm %.3g gates %.3g c %.3g h %.3g pi %.3g' % (err(slot[:, :, KXg:], ref['hm']), err(gg, ref['gates']),
                                                                     err(cg, ref['c']), err(hg, ref['h']), err(pig, ref['pi'])))
    assert float(ref['hm'].abs().max()) > 0
    torch.testing.assert_close(slot[:, :, KXg:].cpu().double(), ref['hm'], rtol=5e-5, atol=1e-5)
    assert torch.equal(slot[:, :, :KXg].cpu(), o['xg'])
    tol = dict(rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(gg.cpu().double(), ref['gates'], **tol)
    torch.testing.assert_close(cg.cpu().double(), ref['c'], **tol)
    torch.testing.assert_close(hg.cpu().double(), ref['h'], **tol)
    torch.testing.assert_close(pig.cpu().double(), ref['pi'], **tol)
    # the draw: the kernel's own pi through the restated sampler gives the kernel's actions (the narrow test's rule), and they are
    # the reference's wherever the reference's CDF leaves the uniform a margin of 2.2e-5 (fp32 pi, rtol 1e-4 on a CDF <= 1, rounded up)
    act_chk = torch.zeros(E, N, dtype=torch.uint8)
    ops_ref.sample_actions(pig.cpu(), act_chk, **DRAW)
    assert torch.equal(actg.cpu(), act_chk)
    u = philox.action_uniform(DRAW['seed'], DRAW['env_id_base'] + np.arange(E), N, DRAW['step'])              # [E,N]
    cdf = np.cumsum(ref['pi'].numpy().transpose(1, 0, 2), axis=-1)
    cdf = (cdf / cdf[..., -1:])[..., :-1]
    near = (np.abs(cdf - np.asarray(u, dtype=np.float64)[..., None]) <= 2.2e-5).any(-1)
    assert near.mean() <= 0.01
    assert np.array_equal(actg.cpu().numpy()[~near], ref['act'].numpy()[~near])
    # value step from the new state: the message term recomputed from h', nothing of it kept
    vr = torch.zeros(N, E, dtype=torch.float64)
    ops_ref.lstm_step_value(ref['h'], f64(o['wh']), f64(o['b']), None, None, ref['c'], f64(o['done']), torch.empty_like(ref['c']),
                            torch.empty_like(ref['h']), f64(o['v_w']), f64(o['v_b']), act_chk, idx, A, vr,
                            xs=(f64(o['xg']), f64(o['wx']), None, None, dict(o['msg_r'], out=None)))
    vg, h2, c2 = torch.zeros(N, E, device='cuda'), torch.zeros_like(hg), torch.zeros_like(cg)
    keep = slot.clone()
    ops.lstm_step_value(hg, None, cu(o['b']), None, None, cg, cu(o['done']), c2, h2, cu(o['v_w']), cu(o['v_b']), actg, cu(idx), A, vg,
                        xs=(slot[:, :, :KXg], None, img, None, dict(msg_g, out=None)))
    torch.cuda.synchronize()
    print('max abs err: v %.3g' % err(vg, vr))
    torch.testing.assert_close(vg.cpu().double(), vr, rtol=1e-4, atol=5e-5)
    assert torch.equal(slot, keep)


def _refusal_operands(N, E, A, m_max, KX):
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g).cuda()                                   # noqa: E731
    from deeprl_network_amd import ops
    o = dict(h=r(N, E, H), c=r(N, E, H), done=torch.zeros(E, device='cuda'), b=r(N, 4 * H), pi_w=r(N, H, A), pi_b=r(N, A),
             v_w=r(N, H + m_max * A, 1), v_b=r(N, 1), w_msg=r(N, H * m_max, H), b_msg=r(N, H))
    o['img'] = ops.lstm_wimage(r(N, KX, 4 * H), r(N, H, 4 * H))
    o['idx'] = torch.zeros(N, m_max, dtype=torch.int32, device='cuda')
    o['idx'][:, 0] = (torch.arange(N, dtype=torch.int32, device='cuda') + 1) % N
    o['idx'][:, 1:] = -1
    # (nmarl_lstm_msg_wimage itself stops at K = 256: the refused launch is handed a buffer of the right size instead)
    o['mimg'] = torch.zeros(N, H * m_max * H, device='cuda')
    o['out'] = dict(hg=torch.full((N, E, H), 7.0, device='cuda'), cg=torch.full((N, E, H), 7.0, device='cuda'),
                    pi=torch.full((N, E, A), 7.0, device='cuda'), act=torch.full((E, N), 9, dtype=torch.uint8, device='cuda'),
                    v=torch.full((N, E), 7.0, device='cuda'), slot=torch.full((N, E, KX), 7.0, device='cuda'))
    return o


def _untouched(out):
    torch.cuda.synchronize()
    assert all(bool((t == (9 if t.dtype == torch.uint8 else 7.0)).all()) for t in out.values())


def test_wider_than_four_slots_is_refused():
    from deeprl_network_amd import _lib, ops
    N, E, A, m_max = 6, 17, 4, 5
    assert not ops.msg_supported(ops.MSG_GATHER_RELU, m_max, H)
    o = _refusal_operands(N, E, A, m_max, 3 * H)
    out = o['out']
    msg = dict(kind=1, nbr_idx=o['idx'], w_msg=o['w_msg'], b_msg=o['b_msg'], img=o['mimg'], enc=None, out=out['slot'][:, :, 2 * H:])
    with pytest.raises(_lib.NmarlError):
        ops.lstm_step_policy(o['h'], None, o['b'], None, None, o['c'], o['done'], out['cg'], out['hg'], o['pi_w'], o['pi_b'], out['pi'],
                             out['act'], xs=(out['slot'][:, :, :2 * H], None, o['img'], None, msg), **DRAW)
    with pytest.raises(_lib.NmarlError):
        ops.lstm_step_value(o['h'], None, o['b'], None, None, o['c'], o['done'], out['cg'], out['hg'], o['v_w'], o['v_b'],
                            torch.zeros(E, N, dtype=torch.uint8, device='cuda'), o['idx'], A, out['v'],
                            xs=(out['slot'][:, :, :2 * H], None, o['img'], None, dict(msg, out=None)))
    _untouched(out)


def test_one_launch_form_refuses_four_slots():
    """Head kind 3 (policy step + value re-step in one launch, <4,1>) stays at K <= 128."""
    from deeprl_network_amd import _lib, ops
    N, E, A, m_max = 6, 17, 4, 4
    o = _refusal_operands(N, E, A, m_max, 3 * H)
    out = o['out']
    sync = ops.step_sync_words(N, E, 'cuda')
    before = sync.clone()
    msg = dict(kind=1, nbr_idx=o['idx'], w_msg=o['w_msg'], b_msg=o['b_msg'], img=ops.lstm_msg_wimage(o['w_msg']), enc=None,
               out=out['slot'][:, :, 2 * H:], sync=sync)
    with pytest.raises(_lib.NmarlError):
        ops.lstm_step_policy_value(o['h'], None, o['b'], None, None, o['c'], o['done'], o['pi_w'], o['pi_b'], out['pi'], out['act'],
                                   o['v_w'], o['v_b'], o['idx'], A, out['v'], xs=(out['slot'][:, :, :2 * H], None, o['img'], None, msg),
                                   h_out=out['hg'], c_out=out['cg'], defer_action_term=True, **DRAW)
    _untouched(out)
    assert torch.equal(sync, before)


def test_dial_refuses_four_slots():
    """lstm_dial's forms stage a second image behind the first: K <= 128."""
    from deeprl_network_amd import _lib, ops
    N, E, A, m_max = 6, 17, 4, 4
    assert not ops.msg_supported(ops.MSG_DIAL, m_max, H) and not ops.msg_supported(ops.MSG_DIAL, 3, H)
    o = _refusal_operands(N, E, A, m_max, H)
    out = o['out']
    src, enc = torch.rand(N, E, H, device='cuda'), torch.rand(N, E, H, device='cuda')
    msg = dict(kind=3, nbr_idx=o['idx'], w_msg=o['w_msg'], b_msg=o['b_msg'], img=ops.lstm_msg_wimage(o['w_msg']), enc=enc, src=src,
               out=out['slot'])
    with pytest.raises(_lib.NmarlError):
        ops.lstm_step_policy(o['h'], None, o['b'], None, None, o['c'], o['done'], out['cg'], out['hg'], o['pi_w'], o['pi_b'], out['pi'],
                             out['act'], xs=(None, None, o['img'], None, msg), **DRAW)
    _untouched(out)


def test_neurcomm_on_the_grid_runs_the_in_kernel_term(monkeypatch):
    """NCMultiAgentPolicy on the 5 x 5 grid (N = 25, m_max = 4), E = 130: one lock-step (policy step + value step) through the
    in-kernel message term vs the fallback (nbr_gather + fc launches, selected by holding ops.msg_supported to the 128-float
    bound).  Same formula, different fp32 summation order: rtol 1e-4 / atol 1e-5."""
    from deeprl_network_amd import ops
    zg = load_npz(os.path.join(GOLDEN, 'nnb_ma2c_nc_grid.npz'))
    E, T = 130, 2
    z = dict(agent='ma2c_nc', topo='grid', n_step=T, seed=7, K=E, reward_norm=2000.0, nb=zg['nb'], dist=zg['dist'])
    N = z['nb'].shape[0]
    g = torch.Generator().manual_seed(19)
    X = torch.randn(E, N, 12, generator=g).cuda()
    fp = torch.softmax(torch.randn(N, E, 5, generator=g), -1).cuda()
    h0, c0 = (torch.randn(N, E, H, generator=g) * 0.7).cuda(), torch.randn(N, E, H, generator=g).cuda()
    done = (torch.rand(E, generator=g) < 0.3).float().cuda()
    u = torch.rand(E, N, generator=g).cuda()
    orig = ops.msg_supported
    got, launches = {}, {}
    for arm in ('fallback', 'kernel'):
        if arm == 'fallback':
            monkeypatch.setattr(ops, 'msg_supported', lambda kind, m_max, n_h: orig(kind, m_max, n_h) and
                                (n_h if kind == ops.MSG_MEAN_ADD else n_h * m_max) <= 128)
        else:
            monkeypatch.setattr(ops, 'msg_supported', orig)
        gathers = []
        real_gather = ops.nbr_gather
        monkeypatch.setattr(ops, 'nbr_gather', lambda *a, **k: (gathers.append(1), real_gather(*a, **k))[1])
        model = build_product_batched(z, 'cuda')
        p = model.policy
        assert model.enable_saved_activations() and model.enable_compact_obs()
        assert p.m_max == 4 and N == 25
        p.refresh_wimage()
        assert (p._msg() is not None) == (arm == 'kernel')
        assert p.pv_one_launch(E) is False and p.enc_in_kernel(E, True) is False
        model.reset_states()
        model.h_fw.copy_(h0), model.c_fw.copy_(c0)
        model.t = 0
        model.buf_x[0].copy_(X)
        model.buf_fp[0].copy_(fp)
        del gathers[:]
        model.act(done, mode=ops.SAMPLE_UNIFORM, u=u)
        torch.cuda.synchronize()
        launches[arm] = len(gathers)
        monkeypatch.setattr(ops, 'nbr_gather', real_gather)
        got[arm] = dict(h=model.H_all[:, 1].clone(), c=model.C_all[:, 1].clone(), pi=model.buf_fp[1].clone(), v=model.buf_v[0].clone(),
                        S=model.S_buf[:, 0].clone(), act=model.buf_act[0].clone())
        del model
    a, b = got['fallback'], got['kernel']
    assert float(b['S'][:, :, 2 * H:].abs().max()) > 0 and float(b['h'].abs().max()) > 0
    for k in ('h', 'c', 'pi', 'v', 'S'):
        print('%s: max abs diff %.3g' % (k, float((a[k] - b[k]).abs().max())))
        torch.testing.assert_close(b[k], a[k], rtol=1e-4, atol=1e-5)
    # the in-kernel arm gathers the fingerprints once (the encoder) and no h; the fallback also gathers h in both steps
    assert launches['fallback'] - launches['kernel'] == 2, launches

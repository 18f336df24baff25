"""Edge checks of the lock-step LSTM kernel (csrc/lstm_mfma.hip, nmarl_lstm_step_x), written as functions of the implementation
under test: `ops` on the GPU (tests/test_gpu_step_edges.py), the restatement `oracle/ops_ref` or a deliberately wrong variant of
it on the CPU (tests/test_step_edges_cpu.py, which proves that the checks are sharp).  Each check draws its inputs from a seeded
generator, forms the expectation in float64 itself from the reference's formulas (agents/utils.py:102-113 the cell,
policies.py:50-77 the heads, agents/utils.py:182-199 / 395-400 / 560-580 the message terms), asserts, prints the worst share of
its bound that was used, and returns it.

A test cannot observe which kernel the launcher chose.  Every check therefore asserts, on the tensors and arguments it built, the
PRECONDITIONS of the branch it is meant for (head kind, message kind, KX, KX2, the precision, which optional tensors are None):
an edit of the inputs that moves a case to another instantiation fails the check instead of passing through the other kernel.

Dispatch census: every hipLaunchKernelGGL of nmarl_lstm_step_x, lstm_step_x_kernel<HEAD, MSG, ENC, CARRY, PREC>.  kind = head kind
(0 without a head), mk = message kind, prec = nmarl_step_x_t.precision.  NMARL_LX / NMARL_LC are the launch macros at
lstm_mfma.hip:2075-2083.  Test ids: [E] tests/test_gpu_step_edges.py, [O] tests/test_gpu_ops.py, other GPU test files by name.

  instantiation     selected when (file:line)                                        check, parameters
  ----------------  ---------------------------------------------------------------  ------------------------------------------------------------
  <0,0>             mk 0, kind 0, prec 0 (lstm_mfma.hip:2085, NMARL_LX :2077)        [E] test_row_edges form=head0; test_two_piece head=0; [O] test_lstm_step_x_whole_preactivation_on_mfma
  <1,0>             mk 0, kind 1, prec 0 (:2085)                                     [E] test_row_edges form=head1 A=1,8; [O] test_lstm_step_x_heads
  <2,0>             mk 0, kind 2, prec 0 (:2085)                                     [E] test_row_edges form=head2 (m_max 2 and 0); test_two_piece head=2; [O] test_lstm_step_x_heads
  <3,0>             mk 0, kind 3, prec 0, no enc (:2085)                             [E] test_row_edges form=head3 A=1,8; test_two_piece head=3; test_done_mask head=3; [O] test_lstm_step_x_heads
  <1,1>             mk 1, kind 1 (:2087)                                             [E] test_row_edges_message_forms form=msg1+head1; [O] test_lstm_step_x_in_kernel_message_term kind=1
  <2,1>             mk 1, kind 2 (:2087)                                             [E] test_row_edges_message_forms form=msg1+head2; [O] test_lstm_step_x_in_kernel_message_term kind=1
  <1,2>             mk 2, kind 1 (:2091)                                             [E] test_row_edges_message_forms form=msg2+head1; [O] test_lstm_step_x_in_kernel_message_term kind=2
  <2,2>             mk 2, kind 2 (:2091)                                             [E] test_row_edges_message_forms form=msg2+head2; [O] test_lstm_step_x_in_kernel_message_term kind=2
  <1,3>             mk 3, kind 1 (:2093)                                             [E] test_row_edges_message_forms form=msg3+head1; [O] test_lstm_step_x_dial_message_term
  <2,3>             mk 3, kind 2 (:2093)                                             [E] test_row_edges_message_forms form=msg3+head2; [O] test_lstm_step_x_dial_message_term
  <3,0,1>           enc, F = 5, two encoders, mk 0, prec 0 (:2014)                   [E] test_bf16x3_form form=enc_pair (its fp32 run); [O] test_lstm_step_x_input_encoders_inside_the_launch
  <3,0,2>           enc, F = 5, w_fp NULL, mk 0, prec 0 (:2013)                      [E] test_bf16x3_form form=enc_single_m2,enc_single_m0 (their fp32 runs); test_gpu_trainer.py test_env_step_inside_the_lock_step_launch_is_the_env_kernel agent=ia2c,ma2c_cu
  <3,0,3>           enc, F != 5, two encoders (:1948)                                test_gpu_grid_enc.py test_general_layout_encoders_inside_the_launch form=pair
  <3,0,4>           enc, F != 5, w_fp NULL (:1947)                                   test_gpu_grid_enc.py test_general_layout_encoders_inside_the_launch form=single
  <4,1,0,0>         mk 1, kind 3, no enc, no carry (:2089, NMARL_LC :2083)           [O] test_lstm_step_x_in_kernel_message_term kind=1 (the one-launch part)
  <4,1,0,1>         mk 1, kind 3, no enc, carry_out alone (:2089, :2082)             test_gpu_trainer.py test_compact_observation_equals_gathered_slab agent=ma2c_nc (encoders as launches; lock-step 0)
  <4,1,0,2>         mk 1, kind 3, no enc, carry_in (:2089, :2081)                    test_gpu_trainer.py test_compact_observation_equals_gathered_slab agent=ma2c_nc (lock-steps >= 1)
  <4,1,1,0>         mk 1, kind 3, enc, no carry (:2088, :2083)                       test_gpu_trainer.py test_message_term_handed_from_the_re_step_to_the_next_lock_step agent=ma2c_nc carry=0
  <4,1,1,1>         mk 1, kind 3, enc, carry_out alone (:2088, :2082)                test_gpu_trainer.py test_message_term_handed_... agent=ma2c_nc carry=1 (lock-step 0)
  <4,1,1,2>         mk 1, kind 3, enc, carry_in (:2088, :2081)                       test_gpu_trainer.py test_message_term_handed_... agent=ma2c_nc carry=1 (lock-steps >= 1)
  <4,2,0,0>         mk 2, kind 3, no carry (:2091, :2083)                            [O] test_lstm_step_x_in_kernel_message_term kind=2 (the one-launch part)
  <4,2,0,1>         mk 2, kind 3, carry_out / mean_next alone (:2091, :2082)         test_gpu_trainer.py test_message_term_handed_... agent=ma2c_ic3 carry=1 (lock-step 0)
  <4,2,0,2>         mk 2, kind 3, carry_in (:2091, :2081)                            test_gpu_trainer.py test_message_term_handed_... agent=ma2c_ic3 carry=1 (lock-steps >= 1)
  <0,0,0,0,1>       mk 0, kind 0, prec 1 (:2085, NMARL_LX :2076)                     [E] test_bf16x3_form form=head0; test_done_mask head=0 bf16x3
  <1,0,0,0,1>       mk 0, kind 1, prec 1 (:2085, :2076)                              [E] test_bf16x3_form form=head1
  <2,0,0,0,1>       mk 0, kind 2, prec 1 (:2085, :2076)                              [E] test_bf16x3_form form=head2; test_two_piece head=2 bf16x3
  <3,0,0,0,1>       mk 0, kind 3, no enc, prec 1 (:2085, :2076)                      [E] test_bf16x3_form form=head3; test_gpu_lstm_bf16x3.py test_bf16x3_step_is_the_split_product entry=step_x
  <3,0,1,0,1>       enc, F = 5, two encoders, prec 1 (:2012)                         [E] test_bf16x3_form form=enc_pair; test_gpu_lstm_bf16x3.py test_bf16x3_step_is_the_split_product entry=step_x_enc
  <3,0,2,0,1>       enc, F = 5, w_fp NULL, prec 1 (:2011)                            [E] test_bf16x3_form form=enc_single_m2,enc_single_m0

The nine <4, ...> forms (head kind 3 with a message term: blocks wait for each other inside the launch) are named with their
existing tests only; nothing in this module launches them.  The refusals around the two-piece input: check_x2_refusals."""
import ctypes as C

import torch

from fc_edge_checks import SENTINEL, SWEEP_TOL, _close, _same_bits
from oracle import ops_ref

F32, F64 = torch.float32, torch.float64
H = 64
V_TOL = dict(rtol=1e-4, atol=3e-5)                       # test_lstm_step_x_heads's for v
ACT_SENTINEL = 0xEE
DRAW = dict(seed=5, env_id_base=40, step=3)


# ------------------------------------------------------------------------------- the split product (bf16x3) in float64
def _split(a):
    """fp32 tensor -> (hi, lo) float64, hi = bf16_rne(a), lo = bf16_rne(a - hi): what the kernels multiply."""
    hi = a.float().to(torch.bfloat16)
    lo = (a.float() - hi.float()).to(torch.bfloat16)
    return hi.double(), lo.double()


def _emul(A, W):
    """float64 sum of the three bf16 products hi_a hi_b + hi_a lo_b + lo_a hi_b of A [N,E,K] @ W [N,K,4H], and sum |a||b|."""
    ah, al = _split(A)
    wh, wl = _split(W)
    return torch.bmm(ah, wh) + torch.bmm(ah, wl) + torch.bmm(al, wh), torch.bmm(A.double().abs(), W.double().abs())


def _cell(z, c, keep):
    i, f, o, u = torch.sigmoid(z[..., :H]), torch.sigmoid(z[..., H:2 * H]), torch.sigmoid(z[..., 2 * H:3 * H]), torch.tanh(z[..., 3 * H:])
    cn = f * c * keep + i * u
    return torch.cat([i, f, o, u], dim=-1), cn, o * torch.tanh(cn)


def _cell_bounds(z, c, keep, bound):
    """(gates, c', h') of the cell at z and the elementwise error bounds (eg, ec, eh) that a pre-activation error <= `bound`
    propagates to (the activations' slopes are <= 1), each with the fp32 epilogue's own rounding of 2e-6."""
    tol = 2e-6
    g, cn, hn = _cell(z, c, keep)
    eg = bound + tol
    ec = (c * keep).abs() * eg[..., H:2 * H] + g[..., 3 * H:].abs() * eg[..., :H] + g[..., :H].abs() * eg[..., 3 * H:] + tol
    eh = torch.tanh(cn).abs() * eg[..., 2 * H:3 * H] + g[..., 2 * H:3 * H].abs() * ec + tol
    return (g, cn, hn), (eg, ec, eh)


def _check(G, C, Hn, z, c, keep, bound, what):
    """Kernel gates / c' / h' against the cell applied to the pre-activation z whose error is at most `bound` (elementwise; the
    activations' slopes are <= 1, c' and h' take the propagated bound), plus the fp32 epilogue's own rounding.  G may be None (the
    value step keeps no gates).  -> the worst share of the bound that was used."""
    (g, cn, hn), (eg, ec, eh) = _cell_bounds(z, c, keep, bound)
    worst = 0.0
    for got, want, err, name in ((G, g, eg, 'gates'), (C, cn, ec, "c'"), (Hn, hn, eh, "h'")):
        if got is None:
            continue
        d = (got.cpu().double() - want).abs()
        assert bool((d <= err).all()), '%s: %s off by %.3g (bound %.3g there)' % (what, name, float(d.max()), float(err.view(-1)[d.argmax()]))
        worst = max(worst, float((d / err).max()))
    return worst


# ------------------------------------------------------------------------------------------------------- inputs, one call
def step_inputs(N, E, KX, A, m_max, seed, addends=0, x3=False):
    """One lock-step's operands (fp32, CPU).  Asymmetric weights: a swapped row / column / chunk of the image cannot pass.  x3: the
    scales of test_gpu_lstm_bf16x3's cases."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                          # noqa: E731
    d = dict(h=torch.tanh(r(N, E, H)), c=r(N, E, H), done=(torch.rand(E, generator=g) < 0.25).float(),
             x=torch.relu(r(N, E, KX)) if KX else None,
             wx=None if KX == 0 else r(N, KX, 4 * H) * 0.15 + torch.arange(4 * H).view(1, 1, -1) * 1e-3 + torch.arange(KX).view(1, -1, 1) * 1e-3,
             wh=r(N, H, 4 * H) * 0.2 + torch.arange(4 * H).view(1, 1, -1) * 1e-3, b=r(N, 4 * H) * 0.1,
             z1=r(N, E, 4 * H) if addends >= 1 else None, z2=r(N, E, 4 * H) if addends >= 2 else None,
             pi_w=r(N, H, A) * 0.5, pi_b=r(N, A) * 0.3, v_w=r(N, H + m_max * A, 1), v_b=r(N, 1),
             act_in=torch.randint(0, A, (E, N), generator=g).to(torch.uint8))
    if x3 and KX:
        d['wx'] = r(N, KX, 4 * H) * 0.15
    d['done'][0] = 0.0                                   # (E = 1: the one row is live, the recurrent product is not all zeros)
    idx = -torch.ones(N, m_max, dtype=torch.int32)
    for i in range(N):
        others = [j for j in range(N) if j != i][:(i % m_max) + 1] if m_max else []
        if others:
            idx[i, :len(others)] = torch.tensor(others, dtype=torch.int32)
    d['idx'] = idx
    return d


def run_step(impl, dev, d, head, x=None, x2=None, precision='fp32', inplace=False, mode=1, msg=None, enc=None, img=None):
    """One call of the step in the form `head` (0: no head, 1: policy, 2: value, 3: policy + value with the action term deferred) on
    `dev`.  x / x2: device tensors (or None), enc: a step_enc_spec built for `impl` in place of x.  Every output is slot 1 of a
    sentinel-filled three-slot buffer ([N,3,E,W]; actions [3,E,N]); in place: the state goes in through slot 1 as well.
    -> dict of the buffers (`*_buf`) and of their slots 1."""
    N, E = d['h'].shape[:2]
    A = d['pi_w'].shape[2]
    t = lambda v: None if v is None else v.to(dev)                                      # noqa: E731
    kw = {}
    if precision != 'fp32':
        impl.check_precision(precision)
        kw = dict(precision=precision)
    if img is None:
        img = impl.lstm_wimage(t(d['wx']), t(d['wh']), **kw)
    o = dict(img=img)
    for name, W in (('h', H), ('c', H), ('g', 4 * H), ('pi', A)):
        o[name + '_buf'] = torch.full((N, 3, E, W), SENTINEL, device=dev)
        o[name] = o[name + '_buf'][:, 1]
    o['v_buf'] = torch.full((N, 3, E), SENTINEL, device=dev)
    o['v'] = o['v_buf'][:, 1]
    o['act_buf'] = torch.full((3, E, N), ACT_SENTINEL, dtype=torch.uint8, device=dev)
    o['act'] = o['act_buf'][1]
    assert o['v'].stride(1) == 1 and o['v'].stride(0) == 3 * E and o['act'].is_contiguous()
    if inplace:
        o['h'].copy_(d['h'])
        o['c'].copy_(d['c'])
        h_in, c_in = o['h'], o['c']
    else:
        h_in, c_in = t(d['h']), t(d['c'])
    xs = (enc if enc is not None else x, t(d['wx']), img) + ((x2, msg) if msg is not None else (x2,) if x2 is not None else ())
    st = (h_in, t(d['wh']), t(d['b']), t(d['z1']), t(d['z2']), c_in, t(d['done']))
    draw = dict(DRAW, mode=mode)
    if head == 0:
        impl.lstm_step_fused(*st, o['g'], o['c'], o['h'], xs=xs, **kw)
    elif head == 1:
        impl.lstm_step_policy(*st, o['c'], o['h'], t(d['pi_w']), t(d['pi_b']), o['pi'], o['act'], xs=xs, gates=o['g'], **draw, **kw)
    elif head == 2:
        o['g'] = None
        impl.lstm_step_value(*st, o['c'], o['h'], t(d['v_w']), t(d['v_b']), t(d['act_in']), t(d['idx']), A, o['v'], xs=xs, **kw)
    else:
        assert head == 3 and msg is None           # (head kind 3 with a message term is a hand-off form: never launched here)
        impl.lstm_step_policy_value(*st, t(d['pi_w']), t(d['pi_b']), o['pi'], o['act'], t(d['v_w']), t(d['v_b']), t(d['idx']), A, o['v'],
                                    xs=xs, h_out=o['h'], c_out=o['c'], gates=o['g'], defer_action_term=True, **draw, **kw)
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize()
    return o


OUT_KEYS = {0: ('g', 'c', 'h'), 1: ('g', 'c', 'h', 'pi', 'act'), 2: ('c', 'h', 'v'), 3: ('g', 'c', 'h', 'pi', 'act', 'v')}


def assert_slots_kept(o, head, what):
    """Slots 0 and 2 of every output buffer keep the sentinel (row E of slot 1 is row 0 of slot 2); outputs the form does not have
    keep it everywhere."""
    for k in ('g', 'c', 'h', 'pi', 'v', 'act'):
        buf = o[k + '_buf'].cpu()
        sent = ACT_SENTINEL if k == 'act' else SENTINEL
        slots = (buf[0], buf[2]) if k == 'act' else (buf[:, 0], buf[:, 2])
        for s, slot in zip((0, 2), slots):
            assert bool((slot == sent).all()), '[slots] %s: slot %d of %s was written' % (what, s, k)
        if k not in OUT_KEYS[head]:
            assert bool((buf == sent).all()), '[slots] %s: %s was written by a form without it' % (what, k)


def assert_written(o, head, what):
    """Every element of slot 1 of the form's outputs was written (none keeps the sentinel)."""
    for k in OUT_KEYS[head]:
        t = o[k].cpu()
        assert not bool((t == (ACT_SENTINEL if k == 'act' else SENTINEL)).any()), '[written] %s: %s keeps a sentinel (a row was left out)' % (what, k)


def same_outputs(a, b, head, what):
    for k in OUT_KEYS[head]:
        assert _same_bits(a[k], b[k]), '[bits] %s: %s differs' % (what, k)


def expect64(d, head, xfull=None, emul=False, msg_t=None):
    """The float64 expectation of one call from the reference's formulas.  xfull: the whole LSTM input x [N,E,KX] (fp32) or None.
    emul: the main products as the float64 split emulation.  -> dict(g, c, h, pi, v, z, absum, zx) (v of kind 3: the h part)."""
    N, E = d['h'].shape[:2]
    keep32 = (1.0 - d['done']).view(1, E, 1)
    keep = keep32.double()
    hk = d['h'] * keep32                                  # the kernel masks h in fp32 (exact), then multiplies
    prod = (lambda a, w: _emul(a, w)[0]) if emul else (lambda a, w: torch.bmm(a.double(), w.double()))      # noqa: E731
    add = d['b'].double().view(N, 1, -1)
    for zz in (d['z1'], d['z2']):
        if zz is not None:
            add = add + zz.double()
    zx = add if xfull is None else prod(xfull, d['wx']) + add
    z = zx + prod(hk, d['wh'])
    absum = torch.bmm(hk.double().abs(), d['wh'].double().abs())
    if xfull is not None:
        absum = absum + torch.bmm(xfull.double().abs(), d['wx'].double().abs())
    g, cn, hn = _cell(z, d['c'].double(), keep)
    e = dict(g=g, c=cn, h=hn, z=z, absum=absum, zx=zx, keep=keep)
    if head in (1, 3):
        e['pi'] = torch.softmax(torch.bmm(hn, d['pi_w'].double()) + d['pi_b'].double().unsqueeze(1), dim=-1)
    if head == 2:
        e['v'] = critic64(d, hn, True)
    if head == 3:                                          # the value re-step (quirk Q1) from the new state, masked again
        z2 = zx + prod((hn * keep).float(), d['wh']) if emul else zx + torch.bmm(hn * keep, d['wh'].double())
        _, _, h2 = _cell(z2, cn, keep)
        e['v'] = critic64(d, h2, False)
    return e


def critic64(d, h, action_term):
    """policies.py:59-77: v = [h, one_hot(neighbour actions)] w + b (action_term False: the h part alone)."""
    N, E = h.shape[:2]
    A = d['pi_w'].shape[2]
    v = torch.bmm(h.double(), d['v_w'][:, :H].double()).squeeze(-1) + d['v_b'].double()
    if action_term:
        for i in range(N):
            for k in range(d['idx'].shape[1]):
                j = int(d['idx'][i, k])
                if j >= 0:
                    v[i] += d['v_w'][i, H + k * A + d['act_in'][:, j].long(), 0].double()
    return v


def assert_draw(o, mode, what):
    """The drawn actions are ops_ref.sample_actions of the implementation's OWN probabilities."""
    chk = torch.zeros_like(o['act'].cpu())
    ops_ref.sample_actions(o['pi'].cpu(), chk, mode=mode, **DRAW)
    assert torch.equal(o['act'].cpu(), chk), '[draw] %s: the actions are not the draw from the implementation\'s pi (mode %d)' % (what, mode)


def close_fp32(o, e, head, what, v_tol=V_TOL):
    """The fp32 forms against float64: gates, c', h', pi at SWEEP_TOL, v at `v_tol`.  -> worst share."""
    worst = 0.0
    for k in OUT_KEYS[head]:
        if k == 'act':
            continue
        tol = v_tol if k == 'v' else SWEEP_TOL
        worst = max(worst, _close('%s %s' % (what, k), o[k], e[k], tag='close', **tol))
    return worst


# --------------------------------------------------------------------------------------------------- 2. the two-piece input
TWO_PIECE_E = [1, 17, 129]
TWO_PIECE_SPLITS = [(32, 32), (128, 64), (0, 64), (0, 256), (224, 32), (96, 96)]
TWO_PIECE_X3_SPLITS = [(128, 64), (0, 64)]
TWO_PIECE_PITCH = ['contiguous', 'block']
TWO_PIECE_HEADS = [0, 2, 3]


def _place_cols(t, pitch, dev):
    """t [N,E,K] on `dev`: contiguous, or columns [32, 32 + K) of a sentinel-filled [N,E,K + 64] buffer.  -> (buffer, view)."""
    N, E, K = t.shape
    if pitch == 'contiguous':
        buf = t.to(dev).contiguous()
        v = buf
        assert v.stride(1) == K
    else:
        buf = torch.full((N, E, K + 64), SENTINEL, device=dev)
        v = buf[:, :, 32:32 + K]
        v.copy_(t)
        assert v.stride(1) == K + 64 and v.stride(1) > v.shape[2]
    assert v.data_ptr() % 16 == 0 and v.stride(2) == 1 and v.stride(0) % 4 == 0 and v.stride(1) % 4 == 0
    return buf, v


def _guards_kept(buf, v, t):
    b = buf.cpu()
    if b.shape[2] == t.shape[2]:
        return torch.equal(b, t)
    K = t.shape[2]
    return torch.equal(b[:, :, 32:32 + K], t) and bool((b[:, :, :32] == SENTINEL).all()) and bool((b[:, :, 32 + K:] == SENTINEL).all())


def check_two_piece(impl, dev, N, E, KX1, KX2, pitch, head, addends, precision):
    """The LSTM input handed over as [x | x2] (KX2 > 0; KX1 = 0: x = None) against the one-piece call on torch.cat([x, x2], -1) with
    the same image and the same other operands: bit for bit in gates, c', h', pi, actions, v -- the chunk loop reads the same
    values in the same order from another pointer (lstm_mfma.hip:607-610).  The one-piece result against float64: fp32 at SWEEP_TOL
    (v included), bf16x3 at the bounds of `_check` / check_bf16x3_form.  Sentinel columns around the blocks and sentinel slots
    around the outputs unchanged."""
    KX = KX1 + KX2
    assert KX2 > 0 and KX2 % 32 == 0 and KX1 % 32 == 0 and KX <= 256 and head in (0, 2, 3) and precision in ('fp32', 'bf16x3')
    d = step_inputs(N, E, KX, 4, 2, N * 1000 + E * 7 + KX1 * 3 + KX2 + head, addends, x3=precision != 'fp32')
    what = 'two-piece N=%d E=%d %d|%d %s head=%d addends=%d %s' % (N, E, KX1, KX2, pitch, head, addends, precision)
    x1_c, x2_c = d['x'][:, :, :KX1].contiguous(), d['x'][:, :, KX1:].contiguous()
    b1 = v1 = None
    if KX1:
        b1, v1 = _place_cols(x1_c, pitch, dev)
    b2, v2 = _place_cols(x2_c, pitch, dev)
    assert (v1 is None) == (KX1 == 0) and v2.shape[2] == KX2 and (addends == 0) == (d['z1'] is None) and d['z2'] is None
    xcat = d['x'].to(dev)
    assert xcat.is_contiguous() and xcat.shape[2] == KX
    kw = {} if precision == 'fp32' else dict(precision=precision)
    img = impl.lstm_wimage(d['wx'].to(dev), d['wh'].to(dev), **kw)
    two = run_step(impl, dev, d, head, x=v1, x2=v2, precision=precision, img=img)
    one = run_step(impl, dev, d, head, x=xcat, precision=precision, img=img)
    same_outputs(two, one, head, what)
    for o in (two, one):
        assert_slots_kept(o, head, what)
        assert_written(o, head, what)
    assert _guards_kept(b2, v2, x2_c) and (b1 is None or _guards_kept(b1, v1, x1_c)), '[guards] %s: an input buffer changed' % what
    if head == 3:
        assert_draw(one, 1, what)
    if precision == 'fp32':
        return close_fp32(one, expect64(d, head, d['x']), head, what, v_tol=SWEEP_TOL)
    return _x3_bounds(one, d, head, d['x'], what)


def _x3_bounds(o, d, head, xfull, what):
    """A bf16x3 call's outputs against the split emulation (fp32 accumulation: 2^-20 sum|a||b|) and against exact float64 (split:
    (3 2^-18 + 2^-20) sum|a||b|), propagated through the cell as `_check` does and on through the heads:
      pi:        with delta = max_a(sum_k |w_ka| eh_k) + 2e-6, |d pi_a| <= pi_a (e^{2 delta} - 1) + 2e-6 (softmax's exact sensitivity);
      v, kind 2: sum_k |w_k| eh_k + 1e-5;
      v, kind 3: from the implementation's OWN h', c': test_bf16x3_step_is_the_split_product's bound.
    -> the worst share of a bound that was used."""
    worst = 0.0
    N, E = d['h'].shape[:2]
    for emul, factor, tag in ((True, 2.0 ** -20, 'split emulation'), (False, 3 * 2.0 ** -18 + 2.0 ** -20, 'exact float64')):
        e = expect64(d, head, xfull, emul=emul)
        bound = factor * e['absum']
        worst = max(worst, _check(o['g'], o['c'], o['h'], e['z'], d['c'].double(), e['keep'], bound, '[x3] %s vs %s' % (what, tag)))
        _, (_, _, eh) = _cell_bounds(e['z'], d['c'].double(), e['keep'], bound)
        if head in (1, 3):
            delta = torch.bmm(eh, d['pi_w'].double().abs()).amax(dim=-1, keepdim=True) + 2e-6
            err = e['pi'] * torch.expm1(2 * delta) + 2e-6
            dpi = (o['pi'].cpu().double() - e['pi']).abs()
            assert bool((dpi <= err).all()), '[x3-pi] %s vs %s: pi off by %.3g' % (what, tag, float(dpi.max()))
            worst = max(worst, float((dpi / err).max()))
        if head == 2:
            err = torch.bmm(eh, d['v_w'][:, :H].double().abs()).squeeze(-1) + 1e-5
            dv = (o['v'].cpu().double() - e['v']).abs()
            assert bool((dv <= err).all()), '[x3-v] %s vs %s: v off by %.3g' % (what, tag, float(dv.max()))
            worst = max(worst, float((dv / err).max()))
    if head == 3:
        # value re-step from the implementation's own h', c': the same x-side part + split(h' keep) @ Wh, critic on h''
        keep32 = (1.0 - d['done']).view(1, E, 1)
        h1 = o['h'].cpu() * keep32
        zh_e, absh = _emul(h1, d['wh'])
        zx = expect64(d, 0, xfull, emul=True)['zx']
        absx = torch.bmm(xfull.double().abs(), d['wx'].double().abs()) if xfull is not None else torch.zeros_like(absh)
        _, _, h2 = _cell(zx + zh_e, o['c'].cpu().double(), keep32.double())
        v_e = critic64(d, h2, False)
        vb = (d['v_w'][:, :H].double().abs().sum(dim=1) * (3 * (2.0 ** -20 * (absx + absh).max()) + 1e-5)).view(N, 1)
        dv = (o['v'].cpu().double() - v_e).abs()
        assert bool((dv <= vb).all()), '[x3-v] %s: the value re-step is not the split product of the own h\' (off by %.3g, bound %.3g)' % (
            what, float(dv.max()), float(vb.min()))
        worst = max(worst, float((dv / vb).max()))
    print('%s: %.3g of its split-product bounds' % (what, worst))
    return worst


# ------------------------------------------------------------------------------------------------ 3. refusals around x2
def check_x2_refusals(dev):
    """Straight through the C struct (as test_lstm_step_x_refuses_combinations_no_form_has): what the launcher refuses around x2
    returns NMARL_EINVAL with the sentinel-filled outputs untouched; KX2 == KX with x = NULL and KX2 = 0 with a garbage non-NULL x2
    (ignored, lstm_mfma.hip:1848) run, and give the one-piece result bit for bit.  -> number of cases."""
    from deeprl_network_amd import _lib, ops
    EINVAL, OK = -1, 0
    N, E, KX, A = 2, 32, 64, 4
    g = torch.Generator().manual_seed(11)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)                                  # noqa: E731
    h, c, bias = r(N, E, H), r(N, E, H), r(N, 4 * H)
    xflat = torch.zeros(N * E * KX + 8, device=dev)
    x = xflat[:N * E * KX].view(N, E, KX)
    x.copy_(torch.randn(N, E, KX, generator=g))
    x_off = xflat[1:1 + N * E * KX].view(N, E, KX)                                      # one float behind a 16-byte boundary
    assert x.data_ptr() % 16 == 0 and x_off.data_ptr() % 16 == 4
    img = ops.lstm_wimage(r(N, KX, 4 * H) * 0.1, r(N, H, 4 * H) * 0.1)
    done = torch.zeros(E, device=dev)
    pi_w, pi_b, v_w, v_b = r(N, H, A), r(N, A), r(N, H, 1), r(N, 1)
    pi, v, act = torch.zeros(N, E, A, device=dev), torch.zeros(N, E, device=dev), torch.zeros(E, N, dtype=torch.uint8, device=dev)
    nbr = torch.tensor([[1], [0]], dtype=torch.int32, device=dev)
    m_img, m_b = ops.lstm_msg_wimage(r(N, H, H) * 0.1), r(N, H)
    enc = ops._step_enc(dict(ob=r(E, N, 5), fp=None, w_ob=r(N, 5, H), b_ob=r(N, H), w_fp=None, b_fp=None, nbrs=[[1], [0]]), N, E)
    msg = _lib.Msg(kind=1, m_max=1, K=H, nbr_idx=nbr.data_ptr(), img=m_img.data_ptr(), img_sn=H * H, b=m_b.data_ptr(), b_sn=H)
    outs = []

    def step(head=None, x=None, KX2=KX, x2=x.data_ptr(), x2_row=KX, x2_sn=E * KX, msg=None, enc=None, kx=KX):
        h_new, c_new = torch.full((N, E, H), SENTINEL, device=dev), torch.full((N, E, H), SENTINEL, device=dev)
        outs.append((h_new, c_new))
        a = _lib.StepX(E=E, N=N, H=H, KX=kx, KX2=KX2, precision=0, x_sn=E * KX, x_row=KX, x2_sn=x2_sn, x2_row=x2_row, h_in=h.data_ptr(),
                       h_sn=E * H, img=img.data_ptr(), img_sn=img.stride(0), bias=bias.data_ptr(), bias_sn=4 * H, c_prev=c.data_ptr(),
                       c_prev_sn=E * H, done=done.data_ptr(), c_new=c_new.data_ptr(), c_new_sn=E * H, h_new=h_new.data_ptr(), h_new_sn=E * H)
        a.x, a.x2 = (None if x is None else x.data_ptr()), x2
        if head is not None:
            a.head = C.pointer(_lib.Head(kind=head, A=A, mode=1, w=pi_w.data_ptr(), w_sn=H * A, b=pi_b.data_ptr(), b_sn=A,
                                         pi_out=pi.data_ptr(), pi_sn=E * A, act_out=act.data_ptr(), v_out=v.data_ptr(), v_sn=E,
                                         w2=v_w.data_ptr(), w2_sn=H, b2=v_b.data_ptr(), b2_sn=1))
        if msg is not None:
            a.msg = C.pointer(msg)
        if enc is not None:
            a.enc = C.pointer(enc)
        return _lib.lib.nmarl_lstm_step_x(C.byref(a), _lib.stream())

    refused = {
        'KX2 > KX': dict(KX2=KX + 32),
        'KX2 % 32 != 0': dict(KX2=48),
        'KX2 > 0 with x2 = NULL': dict(x2=None),
        'x2_row < KX2': dict(x2_row=KX - 4),
        'x2_row % 4 != 0': dict(x2_row=KX + 2),
        'x2_sn % 4 != 0': dict(x2_sn=E * KX + 2),
        'x2 off by one float': dict(x2=x_off.data_ptr()),
        'KX2 > 0 with a message term': dict(head=1, msg=msg, KX2=32),
        'KX2 > 0 with enc': dict(head=3, enc=enc, KX2=32),
    }
    for what, kw in refused.items():
        assert step(**kw) == EINVAL, what
    torch.cuda.synchronize()
    for i, (h_new, c_new) in enumerate(outs):
        assert bool((h_new == SENTINEL).all()) and bool((c_new == SENTINEL).all()), 'refusal %d wrote an output' % i
    # the twins that run: the whole input through x2, x2 ignored when KX2 = 0 -- both the one-piece result
    assert step() == OK and step(x=x, KX2=0, x2=0x10) == OK and step(x=x, KX2=0, x2=None) == OK
    torch.cuda.synchronize()
    (ha, ca), (hb, cb), (hc, cc) = outs[-3:]
    assert bool(torch.isfinite(hc).all()) and not bool((hc == SENTINEL).any())
    assert _same_bits(ha, hc) and _same_bits(ca, cc) and _same_bits(hb, hc) and _same_bits(cb, cc)
    return len(refused) + 2


# ----------------------------------------------------------------- 4. every bf16x3 instantiation at the split-product bound
X3_FORMS = ['head0', 'head1', 'head2', 'head3', 'enc_pair', 'enc_single_m2', 'enc_single_m0']
X3_E = [1, 16, 129]
X3_KX = [(0, 1), (32, 0), (128, 1), (256, 0)]          # (KX, addends) of the head forms; KX = 0: the addend is the whole x-side part
X3_DISCRIMINATE = 10.0
# the same question asked of the value re-step alone, whose only output is v (one number per row): under a re-step that runs the
# fp32 product the two distances below are the same quantity -- ratio 1, to the sampling noise of an rms over N E >= 48 values,
# 1 / sqrt(2 * 48) ~ 10 % --, under the split product the ratio is the gates' (>= 10, v being a fixed linear map of the same
# errors) less what the critic's own fp32 dot product adds to both.  3 lies a factor of 3 from either.
X3_RESTEP_DISCRIMINATE = 3.0
X3_RESTEP_MIN_ROWS = 48


def _enc_case(form, N, E, seed):
    """The CACC input layout of the in-launch encoders (F = 5, A = 4): both (enc_pair, KX = 128), the observation encoder over
    [own | 2 neighbour slots] (enc_single_m2) or over the own features alone (enc_single_m0), KX = 64.  Agent 1 has two neighbours,
    agent 0 one, the last none."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                          # noqa: E731
    nbrs = [[j for j in (i - 1, i + 1) if 0 <= j < N] for i in range(N)]
    nbrs[N - 1] = []
    m0 = form == 'enc_single_m0'
    rows = 5 if m0 else 15
    e = dict(ob=r(E, N, 5), w_ob=r(N, rows, H) * 0.4 + torch.arange(rows).view(1, -1, 1) * 0.01, b_ob=r(N, H) * 0.2, fp=None, w_fp=None,
             b_fp=None, nbrs=[[] for _ in range(N)] if m0 else nbrs)
    if form == 'enc_pair':
        e.update(fp=torch.softmax(r(N, E, 4), dim=-1), w_fp=r(N, 8, H) * 0.4 + torch.arange(H).view(1, 1, -1) * 0.003, b_fp=r(N, H) * 0.2)
    if not m0:
        for i in range(N):                   # rows of absent slots are zero in the product's padded weights
            e['w_ob'][i, 5 * (1 + len(nbrs[i])):] = 0
            if e['w_fp'] is not None:
                e['w_fp'][i, 4 * len(nbrs[i]):] = 0
    return e


def _enc_spec(impl, dev, e, out):
    t = lambda v: None if v is None else v.to(dev)                                      # noqa: E731
    return impl.step_enc_spec(t(e['ob']), t(e['fp']), t(e['w_ob']), t(e['b_ob']), t(e['w_fp']), t(e['b_fp']), e['nbrs'], out=out)


def check_bf16x3_form(impl, dev, form, N, E, KX, addends):
    """One bf16x3 instantiation of the step at the split-product bound (see `_x3_bounds`), on top of it:
      [draw]          modes 1 and 2: the actions are ops_ref.sample_actions of the implementation's own pi; pi does not depend on the mode;
      [enc]           the encoders stay fp32: their output S is bit-identical under both precisions, and is float64's at SWEEP_TOL;
      [discriminate]  the fp32 implementation's gates (head2 keeps none: its c' and h') are >= 10 times farther, in rms, from the split
                      emulation than the bf16x3 implementation's -- what fails if a form silently runs the fp32 product."""
    assert form in X3_FORMS
    is_enc = form.startswith('enc')
    head = 3 if is_enc else int(form[-1])
    if is_enc:
        assert KX == (128 if form == 'enc_pair' else 64) and addends == 0
    else:
        assert KX in (0, 32, 128, 256) and (KX > 0 or addends >= 1)
    what = 'bf16x3 %s N=%d E=%d KX=%d addends=%d' % (form, N, E, KX, addends)
    d = step_inputs(N, E, KX, 4, 2, N * 31 + E * 5 + KX + X3_FORMS.index(form), addends, x3=True)
    assert (d['x'] is None) == (KX == 0) and (d['z1'] is not None) == (addends >= 1) and d['z2'] is None
    runs = {}
    for precision in ('bf16x3', 'fp32'):
        for mode in ((1, 2) if precision == 'bf16x3' and head in (1, 3) else (1,)):
            S = enc = None
            if is_enc:
                e = _enc_case(form, N, E, E + 17)
                S = torch.full((N, 3, E, KX), SENTINEL, device=dev)
                enc = _enc_spec(impl, dev, e, S[:, 1])
                assert (e['w_fp'] is None) == (form != 'enc_pair') and e['w_ob'].shape[1] == (5 if form == 'enc_single_m0' else 15)
            x = None if (is_enc or KX == 0) else d['x'].to(dev)
            o = run_step(impl, dev, d, head, x=x, precision=precision, mode=mode, enc=enc)
            o['S'] = S
            assert_slots_kept(o, head, what)
            assert_written(o, head, what)
            if head in (1, 3):
                assert_draw(o, mode, what)
            runs[precision, mode] = o
    o3, o32 = runs['bf16x3', 1], runs['fp32', 1]
    if ('bf16x3', 2) in runs:
        for k in ('g', 'c', 'h', 'pi'):
            assert _same_bits(runs['bf16x3', 2][k], o3[k]), '[draw] %s: %s depends on the draw mode' % (what, k)
    xfull = d['x']
    worst = 0.0
    if is_enc:
        assert _same_bits(o3['S'], o32['S']), '[enc] %s: the encoders\' output differs between the precisions' % what
        Sc = o3['S'].cpu()
        assert bool((Sc[:, 0] == SENTINEL).all()) and bool((Sc[:, 2] == SENTINEL).all()), '[enc] %s: a slot around S was written' % what
        f64 = lambda v: None if v is None else v.double()                                # noqa: E731
        S64 = ops_ref.step_enc_forward(dict(ob=f64(e['ob']), fp=f64(e['fp']), w_ob=f64(e['w_ob']), b_ob=f64(e['b_ob']), w_fp=f64(e['w_fp']),
                                            b_fp=f64(e['b_fp']), nbrs=e['nbrs']))
        worst = _close(what + ' S', Sc[:, 1], S64, tag='enc', **SWEEP_TOL)
        xfull = Sc[:, 1].contiguous()                     # the LSTM input is the implementation's own S (fp32)
    worst = max(worst, _x3_bounds(o3, d, head, xfull, what))
    e_em = expect64(d, head, xfull, emul=True)
    keys = ('g',) if head != 2 else ('c', 'h')
    rms = lambda o: float(torch.cat([(o[k].cpu().double() - e_em[k]).reshape(-1) for k in keys]).pow(2).mean().sqrt())      # noqa: E731
    d3, d32 = rms(o3), rms(o32)
    print('%s: rms distance from the split emulation: bf16x3 %.3g, fp32 %.3g (ratio %.3g, >= %g asked)' % (what, d3, d32, d32 / max(d3, 1e-300),
                                                                                                           X3_DISCRIMINATE))
    assert d32 >= X3_DISCRIMINATE * d3, '[discriminate] %s: fp32 %.3g vs bf16x3 %.3g from the split emulation' % (what, d32, d3)
    if head == 3 and N * E >= X3_RESTEP_MIN_ROWS:
        v3, v32 = _restep_distance(o3, d, xfull, True), _restep_distance(o32, d, xfull, False)
        print('%s: rms distance of v from the split re-step of the own state: bf16x3 %.3g, fp32 %.3g (ratio %.3g, >= %g asked)'
              % (what, v3, v32, v32 / max(v3, 1e-300), X3_RESTEP_DISCRIMINATE))
        assert v32 >= X3_RESTEP_DISCRIMINATE * v3, '[restep-x3] %s: fp32 %.3g vs bf16x3 %.3g from the split re-step' % (what, v32, v3)
    return worst


def _restep_distance(o, d, xfull, emul_x):
    """rms of v - critic(cell(zx + split_emulation((h' keep) Wh), c' keep)) with the run's OWN h', c': how far the value re-step's
    recurrent product is from the split product.  zx, the x-side part both steps share, in the arithmetic the run used for it
    (emul_x: the split emulation; else exact) -- it is not what is asked about."""
    E = d['h'].shape[1]
    keep32 = (1.0 - d['done']).view(1, E, 1)
    zx = expect64(d, 0, xfull, emul=emul_x)['zx']
    zh, _ = _emul(o['h'].cpu() * keep32, d['wh'])
    _, _, h2 = _cell(zx + zh, o['c'].cpu().double(), keep32.double())
    return float((o['v'].cpu().double() - critic64(d, h2, False)).pow(2).mean().sqrt())


# ------------------------------------------------------------------------------- 5. wave and block edges of the fp32 forms
ROW_EDGE_E = [15, 16, 17, 127, 128, 129]
ROW_EDGE_KX = [(0, 2), (96, 0), (160, 0)]              # (KX, addends): five and seven chunks through the three chunk buffers
ROW_EDGE_HEAD_FORMS = ['head0', 'head1', 'head2', 'head3']
ROW_EDGE_MSG_FORMS = ['msg1+head1', 'msg1+head2', 'msg2+head1', 'msg2+head2', 'msg3+head1', 'msg3+head2']


def msg_table():
    """Ragged, -1 padded table of 3 agents, m_max = 2: agent 0 has both others, agent 1 one (and a padded slot), agent 2 none."""
    t = torch.tensor([[1, 2], [0, -1], [-1, -1]], dtype=torch.int32)
    assert int((t[2] >= 0).sum()) == 0 and int((t[1] >= 0).sum()) == 1
    return t


def _msg_term64(kind, src, tab, w_msg, b_msg, enc):
    """The message term in float64.  kind 1 (lstm_comm, agents/utils.py:182-199): relu([src_j] W + b), absent slots zero; kind 2
    (lstm_ic3, :395-400): mean_j(src_j) W + b + enc, the mean over the neighbours PRESENT, no neighbour: 0; kind 3 (lstm_dial,
    :560-580): relu([src_j] W + b) + enc."""
    N, E, _ = src.shape
    m = tab.shape[1]
    s64, W, b = src.double(), w_msg.double(), b_msg.double().unsqueeze(1)
    if kind == 2:
        mean = torch.zeros(N, E, H, dtype=F64)
        for i in range(N):
            js = [int(j) for j in tab[i] if j >= 0]
            for j in js:
                mean[i] += s64[j] / len(js)
        return torch.bmm(mean, W) + b + enc.double()
    gath = torch.zeros(N, E, m * H, dtype=F64)
    for i in range(N):
        for k in range(m):
            j = int(tab[i, k])
            if j >= 0:
                gath[i, :, k * H:(k + 1) * H] = s64[j]
    t = torch.relu(torch.bmm(gath, W) + b)
    return t + enc.double() if kind == 3 else t


def check_row_edges(impl, dev, form, E, KX=96, addends=0, A=4, m_max=2, N=3):
    """A fp32 form at a row count around a wave (16 rows) or block (8 waves) edge against float64 at SWEEP_TOL (v: V_TOL), the
    outputs slot 1 of sentinel-filled three-slot buffers: [slots] slots 0 and 2 keep the sentinel -- row E is never written --,
    [written] rows 0 .. E - 1 all are; act_out / v_out for exactly E rows.  The message forms (msg<k>+head<1|2>) use the ragged
    table of `msg_table` (one agent without a neighbour) and launch no hand-off form."""
    what = 'row edges %s E=%d A=%d m_max=%d' % (form, E, A, m_max)
    if form in ROW_EDGE_HEAD_FORMS:
        what += ' KX=%d addends=%d' % (KX, addends)
        head = int(form[-1])
        assert (KX, addends) in ROW_EDGE_KX and A in (1, 4, 8) and m_max in (0, 2)
        d = step_inputs(N, E, KX, A, m_max, E * 13 + KX + A + head, addends)
        assert (d['x'] is None) == (KX == 0) and (d['z2'] is not None) == (addends == 2) and d['idx'].shape == (N, m_max)
        assert d['v_w'].shape[1] == H + m_max * A
        o = run_step(impl, dev, d, head, x=None if KX == 0 else d['x'].to(dev))
        e = expect64(d, head, d['x'])
    else:
        kind, head = int(form[3]), int(form[-1])
        assert form in ROW_EDGE_MSG_FORMS and head in (1, 2) and kind in (1, 2, 3) and N == 3 and m_max == 2
        KXg = 64 if kind == 1 else 0                       # lstm_comm: [x | message term]; lstm_ic3 / lstm_dial: the message term alone
        KX = KXg + H
        d = step_inputs(N, E, KX, A, m_max, E * 17 + kind * 5 + head, 0)
        tab = msg_table()
        g = torch.Generator().manual_seed(E + kind)
        r = lambda *s: torch.randn(*s, generator=g)                                      # noqa: E731
        Km = H if kind == 2 else H * m_max
        w_msg = r(N, Km, H) * 0.2 + torch.arange(H).view(1, 1, -1) * 2e-3 + torch.arange(Km).view(1, -1, 1) * 1e-3
        b_msg = r(N, H) * 0.2
        enc = None if kind == 1 else torch.tanh(r(N, E, H))
        src = torch.relu(r(N, E, H)) if kind == 3 else d['h']       # the neighbours' un-masked h (quirk Q3) / the senders' vectors
        xg = d['x'][:, :, :KXg].contiguous() if KXg else None
        t = lambda v: None if v is None else v.to(dev)                                   # noqa: E731
        mbuf = torch.full((N, 3, E, H), SENTINEL, device=dev)
        msg = dict(kind=kind, nbr_idx=t(tab), w_msg=t(w_msg), b_msg=t(b_msg), img=impl.lstm_msg_wimage(t(w_msg)), enc=t(enc), out=mbuf[:, 1])
        if kind == 3:
            msg['src'] = t(src)
        assert msg['kind'] in (1, 2, 3) and head != 3 and 'sync' not in msg and int((tab[N - 1] >= 0).sum()) == 0
        o = run_step(impl, dev, d, head, x=t(xg), msg=msg)
        term = _msg_term64(kind, src, tab, w_msg, b_msg, enc)
        # the float64 expectation takes [x | term] in float64 (the term is no fp32 tensor of the inputs)
        e = _expect64_x64(d, head, term if xg is None else torch.cat([xg.double(), term], dim=-1))
        mb = mbuf.cpu()
        assert bool((mb[:, 0] == SENTINEL).all()) and bool((mb[:, 2] == SENTINEL).all()), '[slots] %s: a slot around the message output was written' % what
        assert not bool((mb[:, 1] == SENTINEL).any()), '[written] %s: the message output keeps a sentinel' % what
        _close(what + ' message term', mb[:, 1], term, tag='msg', **SWEEP_TOL)
    assert_slots_kept(o, head, what)
    assert_written(o, head, what)
    worst = close_fp32(o, e, head, what)
    if head in (1, 3):
        assert_draw(o, 1, what)
    return worst


def _expect64_x64(d, head, x64):
    """expect64 for an LSTM input that is float64 already (heads 1 and 2)."""
    N, E = d['h'].shape[:2]
    keep = (1.0 - d['done']).double().view(1, E, 1)
    z = torch.bmm(x64, d['wx'].double()) + torch.bmm(d['h'].double() * keep, d['wh'].double()) + d['b'].double().view(N, 1, -1)
    g, cn, hn = _cell(z, d['c'].double(), keep)
    e = dict(g=g, c=cn, h=hn)
    if head == 1:
        e['pi'] = torch.softmax(torch.bmm(hn, d['pi_w'].double()) + d['pi_b'].double().unsqueeze(1), dim=-1)
    else:
        e['v'] = critic64(d, hn, True)
    return e


# ----------------------------------------------------------------------------------- 6. the done mask on large stale state
DONE_HEADS = [0, 2, 3]
DONE_N, DONE_E, DONE_KX = 3, 130, 64
GARBAGE = 1e30


def _done_inputs(head, precision, big_bias):
    N, E = DONE_N, DONE_E
    d = step_inputs(N, E, DONE_KX, 4, 2, 900 + head + (7 if precision != 'fp32' else 0) + (3 if big_bias else 0), 0, x3=precision != 'fp32')
    done = (torch.arange(E) % 3 == 1).float()
    done[E - 1] = 1.0
    done[E - 2] = 0.0                                    # (the last row is finished, the one before it is not)
    d['done'] = done
    assert 0 < int(done.sum()) < E and float(done[E - 1]) == 1.0 and float(done[0]) == 0.0 and float(done[1]) == 1.0 and float(done[2]) == 0.0
    if big_bias:
        for k in (0, 2, 3):                              # b_i, b_o, b_u = +20: c' = f c keep + 1, h' = tanh(c') -- large in every row
            d['b'][:, k * H:(k + 1) * H] = 20.0
    return d


def check_done_mask(impl, dev, head, precision):
    """The (1 - done) mask on state that is LARGE where it must not be seen.  N = 3, E = 130, KX = 64, a third of the rows finished,
    the last one among them.
      [bits]    every output agrees bit for bit between h_in / c_prev = +-1e30 in the finished rows and exact zeros there (x * 0 is
                exact for finite x), in place and out of place;
      [close]   fp32: the unfinished rows of the garbage run, and every row of the zero run, are float64's at SWEEP_TOL (v: V_TOL);
                bf16x3: the bounds of `_x3_bounds` on the zero run;
      [restep]  head kind 3: a second pair with b_i, b_o, b_u = +20, i.e. the policy step's OWN h', c' large in the finished rows: the
                critic must see h' (1 - done) and c' (1 - done) -- v against ops_ref.lstm_step_policy followed by
                ops_ref.lstm_step_value in float64."""
    assert head in DONE_HEADS and precision in ('fp32', 'bf16x3')
    N, E = DONE_N, DONE_E
    worst = 0.0
    for big_bias in ((False, True) if head == 3 else (False,)):
        d0 = _done_inputs(head, precision, big_bias)
        fin = d0['done'].bool()
        sign = torch.where(torch.arange(N * E * H).view(N, E, H) % 2 == 0, 1.0, -1.0)
        dg = dict(d0, h=d0['h'].clone(), c=d0['c'].clone())
        dz = dict(d0, h=d0['h'].clone(), c=d0['c'].clone())
        dg['h'][:, fin], dg['c'][:, fin] = (GARBAGE * sign)[:, fin], (-GARBAGE * sign)[:, fin]
        dz['h'][:, fin], dz['c'][:, fin] = 0.0, 0.0
        assert bool(torch.isfinite(dg['h']).all()) and float(dg['h'][:, fin].abs().min()) > 0.99 * GARBAGE and float(dz['c'][:, fin].abs().max()) == 0.0
        e = expect64(dz, head, d0['x'])
        for inplace in (False, True):
            what = 'done mask head=%d %s%s%s' % (head, precision, ' in place' if inplace else '', ' bias +20' if big_bias else '')
            x = d0['x'].to(dev)
            og = run_step(impl, dev, dg, head, x=x, precision=precision, inplace=inplace)
            oz = run_step(impl, dev, dz, head, x=x, precision=precision, inplace=inplace)
            for k in OUT_KEYS[head]:
                if k != 'act':
                    assert bool(torch.isfinite(og[k]).all()), '[bits] %s: %s is not finite (stale state leaked in)' % (what, k)
            same_outputs(og, oz, head, what)
            for o in (og, oz):
                assert_slots_kept(o, head, what)
                assert_written(o, head, what)
            if precision == 'fp32':
                live = dict((k, og[k][:, ~fin.to(og[k].device)]) for k in OUT_KEYS[head] if k != 'act')
                worst = max(worst, close_fp32(live, dict((k, e[k][:, ~fin]) for k in live), head, what + ' (unfinished rows)'),
                            close_fp32(oz, e, head, what))
            else:
                worst = max(worst, _x3_bounds(oz, dz, head, d0['x'], what))
            if head == 3:
                assert_draw(oz, 1, what)
            if big_bias and precision == 'fp32':
                worst = max(worst, _restep_vs_ops_ref(oz, dz, e, what))
    return worst


def _restep_vs_ops_ref(o, d, e, what):
    """v of the policy + value step against the float64 two-step restatement: ops_ref.lstm_step_policy, then ops_ref.lstm_step_value
    from the state it left (the action term deferred: a critic without neighbours)."""
    N, E = d['h'].shape[:2]
    f64 = lambda t: t.double()                                                          # noqa: E731
    hr, cr = torch.empty(N, E, H, dtype=F64), torch.empty(N, E, H, dtype=F64)
    pir, actr = torch.zeros(N, E, 4, dtype=F64), torch.zeros(E, N, dtype=torch.uint8)
    xs = (f64(d['x']), f64(d['wx']), None)
    ops_ref.lstm_step_policy(f64(d['h']), f64(d['wh']), f64(d['b']), None, None, f64(d['c']), f64(d['done']), cr, hr, f64(d['pi_w']),
                             f64(d['pi_b']), pir, actr, xs=xs, mode=1, **DRAW)
    fin = d['done'].bool()
    assert float(hr[:, fin].abs().min()) > 0.7 and float(cr[:, fin].min()) > 0.99, 'the policy step\'s own state is not large in the finished rows'
    vr = torch.zeros(N, E, dtype=F64)
    none = torch.zeros(N, 0, dtype=torch.int32)
    ops_ref.lstm_step_value(hr, f64(d['wh']), f64(d['b']), None, None, cr, f64(d['done']), torch.empty_like(cr), torch.empty_like(hr),
                            f64(d['v_w'][:, :H]), f64(d['v_b']), actr, none, 4, vr, xs=xs)
    assert float((vr - e['v']).abs().max()) < 1e-9       # (the expectation formed here is the same two steps)
    return _close(what + ' v vs the two-step restatement', o['v'], vr, tag='restep', **V_TOL)

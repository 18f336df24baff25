"""Edge checks of the update's encoder and heads kernels (csrc/fc.hip, csrc/nbr.hip) and of the step / cell kernels'
transcendentals, written as functions of the implementation under test: `ops` on the GPU (tests/test_gpu_fc_edges.py), the
restatement `oracle/ops_ref` or a deliberately wrong variant of it on the CPU (tests/test_fc_edges_cpu.py, which proves that the
checks are sharp).  Each check draws its inputs from a seeded generator, forms the expectation in float64 itself from the
reference's formulas (policies.py:20-30, 50-77; agents/utils.py:65-73, 102-113, 192-195, 395), asserts, and returns the worst error
it measured.

A test cannot observe which kernel a host wrapper launched.  Every check therefore asserts, on the tensors it built, the
PRECONDITIONS of the branch it is meant for (`data_ptr() % 16`, `stride(0) % 4`, `stride(1) % 4`, the width class): an edit of the
inputs that moves a case back to another branch fails the check instead of silently passing through the vector kernel.

Dispatch census: every hipLaunchKernelGGL of csrc/fc.hip and csrc/nbr.hip.  `vec` of launch_fc_bwd = y and dy 16-byte aligned, their
agent strides and row pitches multiples of 4.  Test ids: [E] tests/test_gpu_fc_edges.py, [O] tests/test_gpu_ops.py.

  extern entry                 kernel instantiation              selected when (file:line)                            check, parameters
  ---------------------------  --------------------------------  ---------------------------------------------------  -----------------------------------
  nmarl_fc_fwd                 fc_fwd_kernel<16>                 F <= 16 (fc.hip:1227)                                [O] test_fc_small_layer_fwd_bwd F=15,8
                               fc_fwd_kernel<32>                 16 < F <= 32 (fc.hip:1227)                           [O] test_fc_small_layer_fwd_bwd F=20
                               fc_fwd_kernel<64>                 F > 32 (fc.hip:1227)                                 [O] test_fc_small_layer_fwd_bwd F=60,64
  nmarl_fc_fwd_multi           fc_fwd_multi_kernel<16, true>     fmax <= 16 and y / w / b aligned (fc.hip:1257)       [O] test_fc_fwd_multi_with_gathered_fingerprints Fx=15
                               fc_fwd_multi_kernel<16, false>    fmax <= 16, not aligned (fc.hip:1258)                [E] test_fc_fwd_multi_branches case=w_odd,b_odd,pitch130
                               fc_fwd_multi_kernel<32>           16 < fmax <= 32 (fc.hip:1258)                        [E] test_fc_fwd_multi_branches case=f32,f32_gather
                               fc_fwd_multi_kernel<64>           fmax > 32 (fc.hip:1258)                              [O] test_fc_fwd_multi_with_gathered_fingerprints Fx=60
  nmarl_onehot_argmax_add      onehot_argmax_add_kernel          always (fc.hip:1286)                                 [E] test_onehot_argmax_ties, [O] test_onehot_argmax_add
  nmarl_fc_bwd,                fc_bwd_kernel<16>                 F <= 16 and vec (fc.hip:1311)                        [O] test_fc_small_layer_fwd_bwd F=15,8
  nmarl_fc_bwd_gather          fc_bwd_mfma_kernel<64>            F > 32 and vec (fc.hip:1312)                         [O] test_fc_small_layer_fwd_bwd F=60,64
  (launch_fc_bwd)              fc_bwd_mfma_kernel<32>            16 < F <= 32 and vec (fc.hip:1313)                   [O] test_fc_small_layer_fwd_bwd F=20
                               fc_bwd_rows_kernel<16>            F <= 16, not vec (fc.hip:1314)                       [E] test_fc_bwd_rows_branch F=15, every layout
                               fc_bwd_rows_kernel<32>            16 < F <= 32, not vec (fc.hip:1315)                  [E] test_fc_bwd_rows_branch F=20, every layout
                               fc_bwd_rows_kernel<64>            F > 32, not vec (fc.hip:1316)                        [E] test_fc_bwd_rows_branch F=60, every layout
                               fc_bwd_reduce_kernel              always, second launch (fc.hip:1318)                  (every row above)
  nmarl_fc_bwd_pair            fc_bwd_pair_kernel<true>          relu_bits given (fc.hip:1358)                        [O] test_fc_bwd_pair_equals_two_fc_bwd_launches (act 1: bits)
                               fc_bwd_pair_kernel<false>         relu_bits NULL (fc.hip:1361)                         [O] test_fc_bwd_pair_equals_two_fc_bwd_launches
                               fc_bwd_pair_reduce_kernel         always, second launch (fc.hip:1363)                  (both rows above)
  nmarl_thin_linear_bwd        thin_bwd_kernel                   always (fc.hip:1381)                                 [E] test_thin_linear_bwd_eight_outputs, [O] test_thin_linear_bwd
                               thin_bwd_reduce_kernel            always, second launch (fc.hip:1383)                  (the row above)
  nmarl_heads_loss             heads_loss_kernel<true, 5>        dh given, A = 4 (fc.hip:1403)                        [E] test_heads_loss_at_peaked_policies A=4 want_dh
                               heads_loss_kernel<true, 6>        dh given, A = 5 (fc.hip:1403)                        [E] ... A=5 want_dh
                               heads_loss_kernel<true, 8>        dh given, any other A (fc.hip:1403)                  [E] ... A=3,7 want_dh
                               heads_loss_kernel<false, 5>       dh NULL, A = 4 (fc.hip:1404)                         [E] ... A=4 no dh
                               heads_loss_kernel<false, 6>       dh NULL, A = 5 (fc.hip:1404)                         [E] ... A=5 no dh
                               heads_loss_kernel<false, 8>       dh NULL, any other A (fc.hip:1404)                   [E] ... A=3,7 no dh
                               heads_loss_reduce_kernel          always, second launch (fc.hip:1406)                  (every row above)
  nmarl_nbr_action_value_fwd   nbr_action_value_kernel           always (fc.hip:1419)                                 [E] test_nbr_action_value_accumulates (and every heads_loss case)
  nmarl_nbr_action_value_bwd   nbr_action_value_bwd_kernel       always (fc.hip:1433)                                 [E] every heads_loss case, [O] test_heads_and_neighbour_action_value
                               nbr_action_value_reduce_kernel    always, second launch (fc.hip:1434)                  (the row above)
  nmarl_nbr_gather_fwd         gather_fwd_kernel<float4>         F % 4 == 0, x and y aligned (nbr.hip:155)            [E] test_nbr_ragged_table F=12,64
                               gather_fwd_kernel<float>          otherwise (nbr.hip:158)                              [E] test_nbr_ragged_table F=5; F=12,64 with x off by a float
  nmarl_nbr_gather_bwd,        gather_bwd_kernel<float4>         F % 4 == 0, dy / dx / add aligned (nbr.hip:170)      [E] test_nbr_ragged_table F=12,64 add=none,aligned
  nmarl_nbr_gather_bwd_add     gather_bwd_kernel<float>          otherwise (nbr.hip:173)                              [E] test_nbr_ragged_table F=5; F=12,64 add off by a float
  nmarl_nbr_mean_fwd           mean_fwd_kernel<float4>           F % 4 == 0, x and y aligned (nbr.hip:196)            [E] test_nbr_ragged_table F=12,64
                               mean_fwd_kernel<float>            otherwise (nbr.hip:199)                              [E] test_nbr_ragged_table F=5; F=12,64 with x off by a float
  nmarl_nbr_mean_bwd,          mean_bwd_kernel<float4>           F % 4 == 0, dy / dx / add aligned (nbr.hip:210)      [E] test_nbr_ragged_table F=12,64 add=none,aligned
  nmarl_nbr_mean_bwd_add       mean_bwd_kernel<float>            otherwise (nbr.hip:213)                              [E] test_nbr_ragged_table F=5; F=12,64 add off by a float
  nmarl_nbr_onehot             nbr_onehot_kernel                 always (nbr.hip:233)                                 [O] test_nbr_onehot

The refusals in front of those launches (NMARL_EINVAL, nothing written) and the empty forward calls: check_refusals."""
import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
H = 64


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _used(got, exp, rtol, atol):
    """max |got - exp| / (atol + rtol |exp|): <= 1 is torch.testing.assert_close's criterion; nan if anything is not finite."""
    got, exp = got.detach().cpu().double(), exp.detach().cpu().double()
    assert got.shape == exp.shape, (tuple(got.shape), tuple(exp.shape))
    if got.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return float('nan')
    return float(((got - exp).abs() / (atol + rtol * exp.abs())).max())


def _close(what, got, exp, rtol, atol, tag=None):
    u = _used(got, exp, rtol, atol)
    print('%s: %.3g of its bound (rtol %g, atol %.3g)' % (what, u, rtol, atol))
    assert u <= 1.0, '[%s] %s: %.3g of its bound (rtol %g, atol %.3g)' % (tag or what, what, u, rtol, atol)
    return u


SENTINEL = -777.0


def ragged_table():
    """Asymmetric, ragged, -1 padded table of 9 agents, m_max = 8: agent i has the i neighbours (i + 1 .. i + i) mod 9, listed in
    ascending index.  Agent 0 has none, agent 8 all the others; 2 is a neighbour of 1 but 1 is none of 2."""
    N = 9
    tab = -np.ones((N, 8), dtype=np.int32)
    for i in range(N):
        js = sorted({(i + 1 + k) % N for k in range(i)})
        tab[i, :len(js)] = js
    t = torch.from_numpy(tab)
    assert int((t[0] >= 0).sum()) == 0 and int((t[1] >= 0).sum()) == 1 and int((t[8] >= 0).sum()) == 8
    assert 2 in t[1].tolist() and 1 not in t[2].tolist()
    return t


def small_table(N, m_max):
    """-1 padded table of N agents with 0 .. m_max neighbours (agent i: i % (m_max + 1) of them, ascending, never itself)."""
    tab = -torch.ones(N, m_max, dtype=torch.int32)
    for i in range(N):
        js = sorted([(i + 1 + 2 * k) % N for k in range(min(i % (m_max + 1), N - 1))])
        js = sorted(set(j for j in js if j != i))
        tab[i, :len(js)] = torch.tensor(js, dtype=torch.int32)
    return tab


def _gather64(x, tab):
    """[N,E,F] -> [N,E,m*F] float64: slot k of agent i = x[tab[i,k]], zero where padded (agents/utils.py:192-195)."""
    N, E, F = x.shape
    m = tab.shape[1]
    y = torch.zeros(N, E, m * F, dtype=F64)
    for i in range(tab.shape[0]):
        for k in range(m):
            j = int(tab[i, k])
            if j >= 0:
                y[i, :, k * F:(k + 1) * F] = x[j].double()
    return y


# ----------------------------------------------------------------------------------------- A.1 fc_bwd, the scalar-row kernels
FC_BWD_LAYOUTS = ['pitch66', 'offset1', 'stride2']
FC_BWD_ROWS = [1, 63, 65, 130, 4103]
FC_BWD_F = [15, 20, 60]
FC_BWD_GATHER = {15: (5, 3), 20: (5, 4), 60: (12, 5)}       # F -> (A, m_max): 12 | 4 takes the float4 staging of the gathered input


def _place(t, layout, dev):
    """A sentinel-filled buffer on `dev` and the [N,rows,64] view of it that holds t, laid out so that launch_fc_bwd's `vec` is false:
    pitch66: columns [1:65] of a 66-wide buffer;  offset1: pitch 64, one float into a flat allocation;  stride2: agent stride = 2 mod 4."""
    N, rows, W = t.shape
    assert W == 64
    if layout == 'pitch66':
        buf = torch.full((N, rows, 66), SENTINEL, device=dev)
        v = buf[:, :, 1:65]
        assert v.stride(1) == 66 and v.stride(1) % 4 == 2 and v.data_ptr() % 16 == 4
    elif layout == 'offset1':
        buf = torch.full((N * rows * 64 + 8,), SENTINEL, device=dev)
        v = buf[1:1 + N * rows * 64].view(N, rows, 64)
        assert v.stride(1) == 64 and v.stride(0) % 4 == 0 and v.data_ptr() % 16 == 4
    else:
        buf = torch.full((N, rows * 64 + 2), SENTINEL, device=dev)
        v = buf[:, :rows * 64].view(N, rows, 64)
        assert v.stride(1) == 64 and v.stride(0) % 4 == 2 and v.data_ptr() % 16 == 0
    assert buf.data_ptr() % 16 == 0 and v.stride(2) == 1
    v.copy_(t)
    return buf, v


def check_fc_bwd_rows(impl, dev, N, rows, F, layout, act, gather=False):
    """(dw, db) of y = act(x w + b) from y / dy that are not 16-byte rows: fc_bwd_rows_kernel<16|32|64> by F.  x is read in place from
    the env-major slab; gather: through a -1 padded table inside the kernel.  The activation derivative is taken from the y handed
    over.  |got - exp| <= 2e-5 sqrt(rows) + 1e-4 |exp| (test_fc_small_layer_fwd_bwd's), two calls bit-equal, y / dy and the
    sentinels around them untouched."""
    g = torch.Generator().manual_seed(N * 7919 + rows * 13 + F)
    tab = None
    if gather:
        A, m = FC_BWD_GATHER[F]
        tab = small_table(N, m)
        slab = torch.randn(rows, N, A, generator=g)
        x64 = _gather64(slab.transpose(0, 1), tab)
    else:
        slab = torch.randn(rows, N, F, generator=g)
        x64 = slab.transpose(0, 1).double()
    y = torch.randn(N, rows, 64, generator=g)
    y = torch.relu(y) if act == 1 else torch.tanh(y)
    dy = torch.randn(N, rows, 64, generator=g)
    gg = dy.double() * ((y > 0).double() if act == 1 else (1.0 - y.double() ** 2) if act == 2 else 1.0)
    dw_e, db_e = torch.bmm(x64.transpose(1, 2), gg), gg.sum(1)
    xd = slab.to(dev).transpose(0, 1)
    ybuf, yv = _place(y, layout, dev)
    dbuf, dv = _place(dy, layout, dev)
    assert not all(t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0 and t.stride(1) % 4 == 0 for t in (yv, dv))      # `vec` is false
    assert F <= 64 and x64.shape[2] == F
    y0, d0 = ybuf.clone(), dbuf.clone()
    tabd = None if tab is None else tab.to(dev)
    dw, db = impl.fc_bwd(xd, yv, dv, act, nbr_idx=tabd)
    dw2, db2 = impl.fc_bwd(xd, yv, dv, act, nbr_idx=tabd)
    assert tuple(dw.shape) == (N, F, 64) and tuple(db.shape) == (N, 64)
    atol = 2e-5 * float(rows) ** 0.5
    what = 'fc_bwd N=%d rows=%d F=%d %s act=%d gather=%d' % (N, rows, F, layout, act, gather)
    worst = max(_close(what + ' dw', dw, dw_e, 1e-4, atol), _close(what + ' db', db, db_e, 1e-4, atol))
    assert _same_bits(dw, dw2) and _same_bits(db, db2), 'two calls differ'
    assert _same_bits(ybuf, y0) and _same_bits(dbuf, d0), 'an input buffer changed'
    return worst


# ------------------------------------------------------------------------------------------------------ A.2 fc_fwd_multi
FC_MULTI_CASES = ['w_odd', 'b_odd', 'pitch130', 'f32', 'f32_gather']
FC_MULTI_ROWS = [1, 65, 1030]


def check_fc_fwd_multi(impl, dev, rows, case):
    """Two encoder layers in one launch == act(x w + b) per layer in float64 (rtol 1e-5, atol 1e-5), columns outside the layers'
    blocks untouched.
    w_odd / b_odd: widths (15, 8), the first layer's w / b a view of the flat parameter row at an ODD float offset (row stride a
    multiple of 4: the offset alone decides); pitch130: everything aligned, the output the first 128 columns of a 130-wide buffer
    -> fc_fwd_multi_kernel<16, false>.  f32: widths (20, 8); f32_gather: widths (12, 32), the second gathered through the ragged
    table (A = 4, m_max = 8) -> fc_fwd_multi_kernel<32>."""
    g = torch.Generator().manual_seed(rows * 31 + FC_MULTI_CASES.index(case))
    tab = ragged_table() if case == 'f32_gather' else None
    N = 9 if tab is not None else 3
    F1, F2 = {'f32': (20, 8), 'f32_gather': (12, 32)}.get(case, (15, 8))
    act = 1 if case in ('w_odd', 'f32_gather') else 2
    P = 8 + F1 * 64 + 8 + 64 + 8 + F2 * 64 + 8 + 64 + 8
    assert P % 4 == 0
    flat = (torch.randn(N, P, generator=g) * 0.3).to(dev)
    o = 9 if case == 'w_odd' else 8
    w1 = flat[:, o:o + F1 * 64].view(N, F1, 64)
    o = 8 + F1 * 64 + (9 if case == 'b_odd' else 8)
    b1 = flat[:, o:o + 64]
    o = 8 + F1 * 64 + 8 + 64 + 8
    w2 = flat[:, o:o + F2 * 64].view(N, F2, 64)
    o += F2 * 64 + 8
    b2 = flat[:, o:o + 64]
    slab = torch.randn(rows, N, F1, generator=g).to(dev)
    x1 = slab.transpose(0, 1)
    if tab is None:
        x2 = torch.randn(N, rows, F2, generator=g).to(dev)
        x2_64 = x2.cpu().double()
    else:
        x2 = torch.softmax(torch.randn(N, rows, 4, generator=g), -1).to(dev)
        x2_64 = _gather64(x2.cpu(), tab)
        assert tab.shape[1] * x2.shape[2] == 32 and bool((tab < 0).any())
    if case == 'pitch130':
        wide = torch.full((N, rows, 130), SENTINEL, device=dev)
        out, lo = wide[:, :, :128], 0
    else:
        wide = torch.full((N, rows, 192), SENTINEL, device=dev)
        out, lo = wide[:, :, 32:160], 32
    al = lambda t: t.data_ptr() % 16 == 0                                               # noqa: E731
    params_vec = all(al(t) and t.stride(0) % 4 == 0 for t in (w1, b1, w2, b2))
    out_vec = al(out) and out.stride(0) % 4 == 0 and out.stride(1) % 4 == 0
    fmax = max(F1, F2)
    if case in ('w_odd', 'b_odd'):
        odd = w1 if case == 'w_odd' else b1
        assert fmax <= 16 and odd.data_ptr() % 16 == 4 and odd.stride(0) % 4 == 0 and out_vec and not params_vec
        assert all(al(t) for t in (w1, b1, w2, b2) if t is not odd)
    elif case == 'pitch130':
        assert fmax <= 16 and params_vec and al(out) and out.stride(1) == 130
    else:
        assert 16 < fmax <= 32 and params_vec and out_vec
    f64 = lambda t: t.cpu().double()                                                    # noqa: E731
    fn = (lambda t: torch.relu(t)) if act == 1 else (lambda t: torch.tanh(t))           # noqa: E731
    exp = torch.cat([fn(torch.bmm(f64(x1), f64(w1)) + f64(b1).unsqueeze(1)), fn(torch.bmm(x2_64, f64(w2)) + f64(b2).unsqueeze(1))], dim=-1)
    flat0 = flat.clone()
    got = impl.fc_fwd_multi([(x1, w1, b1, None), (x2, w2, b2, None if tab is None else tab.to(dev))], act, out=out)
    worst = _close('fc_fwd_multi rows=%d %s' % (rows, case), wide[:, :, lo:lo + 128], exp, 1e-5, 1e-5)
    assert got is out or _same_bits(got, out)
    guard = torch.ones(wide.shape[2], dtype=torch.bool)
    guard[lo:lo + 128] = False
    assert bool((wide.cpu()[:, :, guard] == SENTINEL).all()), 'a column outside the layers\' blocks was written'
    assert _same_bits(flat, flat0)
    return worst


# ------------------------------------------------------------------------------------- A.3 neighbour gather / mean, ragged table
NBR_E = [1, 33, 300]
NBR_F = [5, 12, 64]


def _off_by_a_float(t, dev):
    """A contiguous copy of t on `dev` whose first element sits 4 bytes behind a 16-byte boundary."""
    flat = torch.full((t.numel() + 8,), SENTINEL, device=dev)
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def check_nbr_ragged(impl, dev, E, F):
    """nbr_gather / nbr_mean and their adjoints (plain and `_add` forms) on the ragged asymmetric table against float64 sums written
    out here.  Gather forward: equal; mean forward: rtol 1e-6, atol 1e-7; adjoints: rtol 1e-6, atol 1e-6
    (test_nbr_gather_and_mean_fwd_bwd's).  `add` once 16-byte aligned and once one float off (F % 4 == 0: the alignment alone
    decides between the float4 and the scalar kernel); the forward input likewise."""
    tab = ragged_table()
    N, m = tab.shape
    g = torch.Generator().manual_seed(E * 131 + F)
    x = torch.randn(N, E, F, generator=g)
    cnt = (tab >= 0).sum(1)
    y_g = _gather64(x, tab)
    y_m = torch.zeros(N, E, F, dtype=F64)
    for i in range(N):
        for k in range(int(cnt[i])):
            y_m[i] += x[int(tab[i, k])].double() / float(cnt[i])
    dy_g, dy_m, add = torch.randn(N, E, m * F, generator=g), torch.randn(N, E, F, generator=g), torch.randn(N, E, F, generator=g)
    dx_g, dx_m = torch.zeros(N, E, F, dtype=F64), torch.zeros(N, E, F, dtype=F64)
    for i in range(N):
        for k in range(int(cnt[i])):
            j = int(tab[i, k])
            dx_g[j] += dy_g[i, :, k * F:(k + 1) * F].double()
            dx_m[j] += dy_m[i].double() / float(cnt[i])
    tabd = tab.to(dev)
    worst = 0.0
    xs = {'aligned': x.to(dev), 'off': _off_by_a_float(x, dev)}
    assert xs['aligned'].data_ptr() % 16 == 0
    for name, xd in xs.items():
        got = impl.nbr_gather(xd, tabd)
        assert torch.equal(got.cpu().double(), y_g), 'gather forward (x %s)' % name
        worst = max(worst, _close('nbr_mean E=%d F=%d x %s' % (E, F, name), impl.nbr_mean(xd, tabd), y_m, 1e-6, 1e-7))
    adds = {'none': None, 'aligned': add.to(dev), 'off': _off_by_a_float(add, dev)}
    assert adds['aligned'].data_ptr() % 16 == 0
    for name, ad in adds.items():
        plus = 0.0 if ad is None else add.double()
        d1 = impl.nbr_gather_bwd(dy_g.to(dev), tabd, F, add=ad)
        d2 = impl.nbr_mean_bwd(dy_m.to(dev), tabd, add=ad)
        worst = max(worst, _close('nbr_gather_bwd E=%d F=%d add %s' % (E, F, name), d1, dx_g + plus, 1e-6, 1e-6),
                    _close('nbr_mean_bwd E=%d F=%d add %s' % (E, F, name), d2, dx_m + plus, 1e-6, 1e-6))
        assert tuple(d1.shape) == (N, E, F) and tuple(d2.shape) == (N, E, F)
        if ad is not None:
            assert torch.equal(ad.cpu(), add), 'add changed'
    return worst


# ------------------------------------------------------------------------------------------------------------ A.4 refusals
def check_refusals(dev):
    """Calls the wrappers refuse in front of every launch -- NMARL_EINVAL, the sentinel-filled outputs untouched -- and the empty
    forward calls (rows == 0: NMARL_OK, nothing written).  Straight through ctypes; nothing here launches a kernel."""
    from deeprl_network_amd import _lib
    lib, st = _lib.lib, _lib.stream()
    EINVAL, OK = -1, 0
    N, rows = 2, 8
    z = lambda *s: torch.zeros(*s, device=dev)                                          # noqa: E731
    sent = lambda *s: torch.full(s, SENTINEL, device=dev)                               # noqa: E731
    p = lambda t: None if t is None else t.data_ptr()                                   # noqa: E731
    outs = []

    def fc_fwd(F=8, act=1, Jw=64, rows=rows):
        x, w, b, y = z(N, max(rows, 1), 64), z(N, 64, 64), z(N, 64), sent(N, max(rows, 1), 64)
        outs.append(y)
        return lib.nmarl_fc_fwd(rows, N, F, Jw, p(x), x.stride(0), 64, p(w), 64 * 64, p(b), 64, act, p(y), y.stride(0), 64, st)

    def fc_bwd(F=8, act=1, Jw=64):
        x, y, dy = z(N, rows, 64), z(N, rows, 64), z(N, rows, 64)
        part, dw, db = sent(N, 4, 65, 64), sent(N, 64, 64), sent(N, 64)
        outs.extend([part, dw, db])
        return lib.nmarl_fc_bwd(rows, N, F, Jw, p(x), rows * 64, 64, p(y), rows * 64, 64, p(dy), rows * 64, 64, act, p(part), p(dw), 64 * 64,
                                p(db), 64, st)

    def parts(F=(8, 8)):
        arr = (_lib.FcPart * 2)()
        keep = []
        for i in range(2):
            x, w, b = z(N, rows, 64), z(N, 64, 64), z(N, 64)
            keep.extend([x, w, b])
            arr[i].x, arr[i].x_sn, arr[i].x_row, arr[i].F = p(x), rows * 64, 64, F[i]
            arr[i].w, arr[i].w_sn, arr[i].b, arr[i].b_sn = p(w), 64 * 64, p(b), 64
        return arr, keep

    def fc_fwd_multi(F=(8, 8), act=1, rows=rows):
        arr, keep = parts(F)
        y = sent(N, max(rows, 1), 128)
        outs.append(y)
        return lib.nmarl_fc_fwd_multi(rows, N, 2, arr, act, p(y), y.stride(0), 128, st)

    def fc_bwd_pair(off):
        arr, keep = parts()
        y = z(N, rows, 128)
        flat = z(N * rows * 128 + 8)
        dy = flat[off:off + N * rows * 128].view(N, rows, 128)
        assert (dy.data_ptr() % 16 != 0) == (off % 4 != 0)
        part, dwb = sent(N, 4, 2, 17, 64), sent(N, 2, 17, 64)
        outs.extend([part, dwb])
        return lib.nmarl_fc_bwd_pair(rows, N, arr, p(y), rows * 128, 128, None, 0, p(dy), rows * 128, 128, 1, p(part), p(dwb), st)

    def heads_loss(A=4, h_off=0):
        O = A + 1
        flat = z(N * rows * 64 + 8)
        h = flat[h_off:h_off + N * rows * 64].view(N, rows, 64)
        w, b, va = z(N, 64, O), z(N, O), z(N, rows)
        action, adv, R = torch.zeros(rows, N, dtype=torch.uint8, device=dev), z(N, rows), z(N, rows)
        part, loss, dy8, dv, dh = sent(N, 4, 65 * O + 3), sent(N, 3), sent(N, rows, 8), sent(N, rows), sent(N, rows, 64)
        dw, db = sent(N, 64, O), sent(N, O)
        outs.extend([part, loss, dy8, dv, dh, dw, db])
        return lib.nmarl_heads_loss(rows, N, 64, A, p(h), rows * 64, p(w), 64 * O, p(b), O, p(va), p(action), p(adv), p(R), 0.5, 0.01, p(part),
                                    p(loss), p(dy8), p(dv), p(dh), rows * 64, p(dw), 64 * O, p(db), O, st)

    def thin(O):
        h, dy, w = z(N, rows, 64), z(N, rows, O), z(N, 64, O)
        part, dh, dw, db = sent(N, 4, 65, O), sent(N, rows, 64), sent(N, 64, O), sent(N, O)
        outs.extend([part, dh, dw, db])
        return lib.nmarl_thin_linear_bwd(rows, N, 64, O, p(h), rows * 64, p(dy), rows * O, None, 0, p(w), 64 * O, p(part), p(dh), rows * 64,
                                         p(dw), 64 * O, p(db), O, st)

    def action_value_bwd(A, m):
        nbr = torch.zeros(N, m, dtype=torch.int32, device=dev)
        action, dv = torch.zeros(rows, N, dtype=torch.uint8, device=dev), z(N, rows)
        part, dw = sent(N, 4, m * A), sent(N, m * A)
        outs.extend([part, dw])
        return lib.nmarl_nbr_action_value_bwd(rows, N, A, m, p(nbr), p(action), p(dv), p(part), p(dw), m * A, st)

    def nbr(entry, Nn=129, m=8, E=1, F=4):
        tab = -torch.ones(Nn, m, dtype=torch.int32, device=dev)
        a, b_, c = z(Nn, max(E, 1), m * F), sent(Nn, max(E, 1), m * F), z(Nn, max(E, 1), m * F)
        outs.append(b_)
        if entry == 'nmarl_nbr_onehot':
            act = torch.zeros(max(E, 1), Nn, dtype=torch.uint8, device=dev)
            return lib.nmarl_nbr_onehot(E, Nn, F, m, p(tab), p(act), p(b_), E * m * F, st)
        fn = getattr(lib, entry)
        if entry.endswith('_add'):
            return fn(E, Nn, F, m, p(tab), p(a), p(c), p(b_), st)
        return fn(E, Nn, F, m, p(tab), p(a), p(b_), st)

    refused = {
        'fc_fwd F = 65': lambda: fc_fwd(F=65), 'fc_fwd act = 3': lambda: fc_fwd(act=3), 'fc_fwd Jw = 32': lambda: fc_fwd(Jw=32),
        'fc_bwd F = 65': lambda: fc_bwd(F=65), 'fc_bwd act = 3': lambda: fc_bwd(act=3), 'fc_bwd Jw = 32': lambda: fc_bwd(Jw=32),
        'fc_fwd_multi F = 65': lambda: fc_fwd_multi(F=(8, 65)), 'fc_fwd_multi act = 3': lambda: fc_fwd_multi(act=3),
        'fc_bwd_pair dy off alignment': lambda: fc_bwd_pair(1),
        'heads_loss h off alignment': lambda: heads_loss(h_off=1), 'heads_loss A = 8': lambda: heads_loss(A=8),
        'thin_linear_bwd O = 9': lambda: thin(9),
        'nbr_action_value_bwd m_max A = 33': lambda: action_value_bwd(11, 3),
    }
    assert 129 * 8 > 1024                                                # MAX_PAIRS of csrc/nbr.hip
    for entry in ('nmarl_nbr_gather_fwd', 'nmarl_nbr_gather_bwd', 'nmarl_nbr_gather_bwd_add', 'nmarl_nbr_mean_fwd', 'nmarl_nbr_mean_bwd',
                  'nmarl_nbr_mean_bwd_add', 'nmarl_nbr_onehot'):
        refused[entry + ' N m_max = 1032'] = (lambda e=entry: nbr(e))
    for what, call in refused.items():
        assert call() == EINVAL, what
    empty = {
        'fc_fwd': lambda: fc_fwd(rows=0), 'fc_fwd_multi': lambda: fc_fwd_multi(rows=0),
        'nbr_gather_fwd': lambda: nbr('nmarl_nbr_gather_fwd', Nn=3, m=2, E=0), 'nbr_mean_fwd': lambda: nbr('nmarl_nbr_mean_fwd', Nn=3, m=2, E=0),
        'nbr_onehot': lambda: nbr('nmarl_nbr_onehot', Nn=3, m=2, E=0),
    }
    for what, call in empty.items():
        assert call() == OK, what
    y, pp = sent(N, 1, 64), z(N, 1, 4)
    outs.append(y)
    assert lib.nmarl_onehot_argmax_add(0, N, 4, 64, p(pp), 4, None, p(y), 64, 64, st) == OK
    va = sent(N, 1)
    outs.append(va)
    tab = torch.zeros(N, 1, dtype=torch.int32, device=dev)
    assert lib.nmarl_nbr_action_value_fwd(0, N, 4, 1, p(tab), p(torch.zeros(1, N, dtype=torch.uint8, device=dev)), p(z(N, 4)), 4, p(va), 0, st) == OK
    torch.cuda.synchronize()
    for i, t in enumerate(outs):
        assert bool((t == SENTINEL).all()), 'output %d was written' % i
    # the aligned twins of the two alignment refusals run (the refusal is about the alignment, nothing else)
    assert fc_bwd_pair(0) == OK and heads_loss(h_off=0) == OK
    torch.cuda.synchronize()
    return len(refused) + len(empty) + 2


# -------------------------------------------------------------------------------------------- B. heads_loss at peaked policies
HEADS_LOSS_N, HEADS_LOSS_ROWS, HEADS_LOSS_A = [2, 5], [1, 129, 1003], [4, 5, 3, 7]      # A: the compiled forms O = 5, 6 and the generic one
HL_OFFSET = -35.0
HL_SHIFT = 90.0
HL_TERMS_TOL = dict(rtol=2e-5, atol=1e-7)
HL_GRAD_RTOL, HL_GRAD_ATOL = 2e-4, 2e-6                # atol in units of max |reference|
HL_ENT_RTOL = 2e-4     # d logits of a clipped column on rows with a zero advantage: see check_heads_loss_clip


def heads_loss_inputs(N, rows, A):
    """h, W, b such that logits = noise (|.| <= 3) + offset in {0, -35}: h channels 62 / 63 are per-row selectors in {0, 1} whose
    weight rows hold 0 or -35 per column (selector 1 of agent n knocks out column n % A, selector 2 columns (n + 1) % A and, for
    A >= 4, (n + 2) % A: at least one column keeps offset 0); channels 60 / 61 are uniform in [-1, 1] with weights of magnitude 1.2 / 1.0
    (a bounded, wide noise); the last agent's bias is shifted by +90 as a whole."""
    g = torch.Generator().manual_seed(N * 1009 + rows * 7 + A)
    r = lambda *s: torch.randn(*s, generator=g)                                         # noqa: E731
    h = torch.tanh(r(N, rows, H))
    h[:, :, 60:62] = torch.rand(N, rows, 2, generator=g) * 2 - 1
    pi_w = r(N, H, A) * 0.05
    sign = (torch.rand(N, 2, A, generator=g) < 0.5).float() * 2 - 1
    pi_w[:, 60], pi_w[:, 61] = 1.2 * sign[:, 0], 1.0 * sign[:, 1]
    pi_b = r(N, A) * 0.1
    pi_w[:, 62:] = 0.0
    h[:, :, 62:] = 0.0
    noise = torch.baddbmm(pi_b.double().unsqueeze(1), h.double(), pi_w.double()).abs().amax(dim=(1, 2))
    s = torch.clamp(2.9 / noise, max=1.0).float()
    pi_w, pi_b = pi_w * s.view(N, 1, 1), pi_b * s.view(N, 1)
    n_idx, r_idx = torch.arange(N).view(N, 1), torch.arange(rows).view(1, rows)
    s1 = ((r_idx + n_idx) % 2 == 1)
    s2 = ((r_idx // 2 + n_idx) % 3 == 0)
    h[:, :, 62], h[:, :, 63] = s1.float(), s2.float()
    off = torch.zeros(N, rows, A, dtype=torch.bool)
    for n in range(N):
        pi_w[n, 62, n % A] = HL_OFFSET
        off[n, s1[n], n % A] = True
        for q in ((1, 2) if A >= 4 else (1,)):
            pi_w[n, 63, (n + q) % A] = HL_OFFSET
            off[n, s2[n], (n + q) % A] = True
    pi_b[N - 1] += HL_SHIFT
    m_max = 2
    nbr = torch.tensor([[(i + k + 1) % N if k < 1 + (i % m_max) else -1 for k in range(m_max)] for i in range(N)], dtype=torch.int32)
    v_w, v_b = r(N, H + m_max * A, 1) * .2, r(N, 1) * .1
    action = torch.randint(0, A, (rows, N), generator=g).to(torch.uint8)
    for n in range(N):                                          # every 7th row takes a knocked-out column where the row has one
        for rr in range(0, rows, 7):
            ks = torch.nonzero(off[n, rr]).view(-1)
            if len(ks):
                action[rr, n] = int(ks[0])
    adv, R = r(N, rows), r(N, rows)
    adv[:, 2::5] = 0.0                                          # rows whose d logits is the entropy term alone
    if rows == 1:
        adv[0] = 0.0
    return dict(h=h, pi_w=pi_w, pi_b=pi_b, v_w=v_w, v_b=v_b, nbr=nbr, action=action, adv=adv, R=R, off=off, m_max=m_max)


def check_heads_loss_clip(impl, dev, N, rows, A, want_dh):
    """heads + A2C loss + the heads' backward (policies.py:20-30, 50-77) where log(clip(pi, 1e-10, 1)) clips: float64 autograd of the
    reference chain (clamp: gradient blocked outside) against impl.heads_loss.
    Conditions on the inputs, asserted on the float64 reference: no probability in [1e-11, 1e-9] (fp32 and float64 cannot fall on
    different sides of the clip), >= 25 % of the rows have a clipped column, in >= 5 % the clipped column is the action taken.
    Assertions, in this order (the tag in brackets opens the message):
      [finite]   every output is finite (a softmax without the max subtraction overflows at the agent shifted by +90);
      [terms]    the three loss terms, rtol 2e-5 / atol 1e-7;
      [entropy]  d logits of the clipped columns on rows with advantage 0 -- there it is the entropy term alone,
                 -(e_coef / rows) p_k (g_k - sum_j p_j g_j) with g_k = -log(1e-10) for a clipped k (no `+ 1`: the clamp blocks it): a pure
                 relative bound of 2e-4.  fp32 gets p_k = exp(z_k - max) / sum from logits of magnitude <= 93 rounded to 2^-18 (a few
                 such roundings: |d(z_k - max)| < 3e-5), and g_k - gbar to ~1e-6 relative: 2e-4 leaves a factor of 5;
      [blocked]  d logits on the rows whose taken action is clipped (the policy term's gradient is blocked there), rtol 2e-4, atol 2e-6 max|ref|;
      [dy8] [dv] [dh] [pi_w] [pi_b] [v_w] [v_b]  everything else, rtol 2e-4, atol 2e-6 max|ref| (test_heads_loss_one_pass_vs_torch's)."""
    d = heads_loss_inputs(N, rows, A)
    m_max, nbr, action = d['m_max'], d['nbr'], d['action']
    v_coef, e_coef = 0.5, 0.01
    P = [d[k].double().requires_grad_(True) for k in ('h', 'pi_w', 'pi_b', 'v_w', 'v_b')]
    hd, pw, pb, vw, vb = P
    logits = torch.baddbmm(pb.unsqueeze(1), hd, pw)
    na = torch.zeros(N, rows, m_max * A, dtype=F64)
    for i in range(N):
        for k in range(m_max):
            j = int(nbr[i, k])
            if j >= 0:
                na[i, torch.arange(rows), k * A + action[:, j].long()] = 1.0
    v = (torch.baddbmm(vb.unsqueeze(1), hd, vw[:, :H]) + torch.bmm(na, vw[:, H:])).squeeze(-1)
    pi = torch.softmax(logits, dim=-1)
    log_pi = torch.log(torch.clamp(pi, 1e-10, 1.0))
    ent = -(pi * log_pi).sum(-1)
    acts = action.t().long().unsqueeze(-1)
    logp_a = log_pi.gather(-1, acts).squeeze(-1)
    adv64, R64 = d['adv'].double(), d['R'].double()
    terms_r = torch.stack([-(logp_a * adv64).mean(-1), (R64 - v).pow(2).mean(-1) * 0.5 * v_coef, -ent.mean(-1) * e_coef], dim=1)
    logits.retain_grad()
    v.retain_grad()
    terms_r.sum().backward()
    # ---- conditions on the inputs
    p64 = pi.detach()
    shift = torch.zeros(N, 1, 1, dtype=F64)
    shift[N - 1] = HL_SHIFT
    noise = logits.detach() - shift - HL_OFFSET * d['off'].double()
    assert float(noise.abs().max()) <= 3.0, float(noise.abs().max())
    assert not bool(((p64 >= 1e-11) & (p64 <= 1e-9)).any())
    clipped = p64 < 1e-10
    assert torch.equal(clipped, d['off'])
    assert bool((p64[clipped] <= np.exp(-29.0)).all()) and bool((p64[~clipped] >= np.exp(-6.0) / A).all())
    frac_rows = float(clipped.any(-1).double().mean())
    taken_clipped = clipped.gather(-1, acts).squeeze(-1)
    frac_taken = float(taken_clipped.double().mean())
    assert frac_rows >= 0.25 and frac_taken >= 0.05, (frac_rows, frac_taken)
    ent_rows = (d['adv'] == 0).unsqueeze(-1) & clipped
    assert bool(ent_rows.any()) or rows == 1
    # ---- the implementation
    c = lambda t: t.to(dev)                                                             # noqa: E731
    out = impl.heads_loss(c(d['h']), c(d['pi_w']), c(d['pi_b']), c(d['v_w']), c(d['v_b']), c(action), c(nbr), A, c(d['adv']), c(d['R']),
                          v_coef, e_coef, want_dh=want_dh)
    what = 'heads_loss N=%d rows=%d A=%d dh=%d' % (N, rows, A, want_dh)
    assert (out['dh'] is not None) == want_dh
    for k in ('terms', 'dy8', 'pi_w', 'pi_b', 'v_w', 'v_b') + (('dh',) if want_dh else ()):
        assert bool(torch.isfinite(out[k]).all()), '[finite] %s: %s' % (what, k)
    worst = dict(frac_rows=frac_rows, frac_taken=frac_taken)
    worst['terms'] = _close(what + ' terms', out['terms'], terms_r.detach(), tag='terms', **HL_TERMS_TOL)
    dy8 = out['dy8'].cpu().double()
    dl, dlr = dy8[:, :, :A], logits.grad
    scale = float(dlr.abs().max())
    if bool(ent_rows.any()):
        assert bool((dlr[ent_rows] != 0).all())
        worst['entropy'] = _close(what + ' d logits, clipped columns, advantage 0', dl[ent_rows], dlr[ent_rows], HL_ENT_RTOL, 0.0, tag='entropy')
    worst['blocked'] = _close(what + ' d logits, taken action clipped', dl[taken_clipped], dlr[taken_clipped], HL_GRAD_RTOL,
                              HL_GRAD_ATOL * scale, tag='blocked')
    worst['dy8'] = _close(what + ' d logits', dl, dlr, HL_GRAD_RTOL, HL_GRAD_ATOL * scale, tag='dy8')
    worst['dv'] = _close(what + ' d v', dy8[:, :, A], v.grad, HL_GRAD_RTOL, HL_GRAD_ATOL * float(v.grad.abs().max()), tag='dv')
    assert float(dy8[:, :, A + 1:].abs().max() if A + 1 < 8 else 0.0) == 0.0, '[dy8] padding columns'
    if want_dh:
        worst['dh'] = _close(what + ' dh', out['dh'], hd.grad, HL_GRAD_RTOL, HL_GRAD_ATOL * float(hd.grad.abs().max()), tag='dh')
    for key, ref in (('pi_w', pw.grad), ('pi_b', pb.grad), ('v_w', vw.grad), ('v_b', vb.grad)):
        worst[key] = _close(what + ' ' + key, out[key].cpu().double().reshape(ref.shape), ref, HL_GRAD_RTOL,
                            HL_GRAD_ATOL * float(ref.abs().max()), tag=key)
    return worst


# -------------------------------------------------------------------------- C. the step and cell kernels' transcendentals
# csrc/lstm_mfma.hip, the comment above sigm() / tanh_fast(): the project's own claim, compared without a margin
SIGMOID_REL_BOUND = 1e-6       # relative error of sigmoid on |z| < 20
TANH_ABS_BOUND = 2.4e-7        # absolute error of tanh
SWEEP_TOL = dict(rtol=3e-5, atol=5e-6)       # test_lstm_step_x_whole_preactivation_on_mfma's
SWEEP_PATHS = ['step', 'step_bf16x3', 'cell']


def sweep_grid():
    """-200 ... -1e-30, -0, +0, 1e-30 ... 200 in ascending order (float32)."""
    pos = np.concatenate([[1e-30, 1e-8, 1e-4], np.logspace(np.log10(0.01), np.log10(20.0), 4096), [25, 44, 50, 88, 90, 100, 200]])
    pos = np.unique(pos.astype(np.float32))
    z = np.concatenate([-pos[::-1], np.float32([-0.0, 0.0]), pos]).astype(np.float32)
    assert np.all(np.diff(z.astype(np.float64)) >= 0) and np.signbit(z[len(pos)]) and not np.signbit(z[len(pos) + 1])
    return z


SWEEP_C = np.float32([0, 1e-3, 0.25, 0.5, 1, 2, 5, 9, 10, 20, 40, 60, -1e-3, -0.25, -0.5, -1, -2, -5, -9, -10, -20, -40, -60])


def check_gate_sweep(impl, dev, path='step'):
    """sigmoid / tanh of the LSTM epilogues over a deterministic grid of pre-activations, through the plain step (KX = 0, one
    addend, h = 0, Wh = 0, bias = 0: z is the addend bit for bit) or through cell_fwd (H = 32).  Every gate block sees every grid
    value at least twice (in other lanes); c_prev walks +-{0 ... 60}, a fifth of the rows is `done`.
    Assertions in this order: [finite]; [saturation] sigmoid(z >= 25) == 1, sigmoid(z <= -90) == 0, tanh(|z| >= 10) == +-1;
    [monotone] sigmoid non-decreasing along the grid; [sigmoid-rel] / [tanh-abs] the measured worst errors against the bounds of the
    source comment; [close] gates, c', h' to rtol 3e-5 / atol 5e-6 against float64.  -> (worst sigmoid relative error on |z| < 20,
    worst tanh absolute error)."""
    grid = sweep_grid()
    G = len(grid)
    Hc = 32 if path == 'cell' else H
    N, E = (2, 260) if path == 'cell' else (2, 130)
    S = N * E * Hc
    assert S >= 2 * G and G % len(SWEEP_C) != 0
    slot = np.arange(S)
    shifts = (0, 2741, 5477, 1371)
    idx = np.stack([(slot + s) % G for s in shifts], 0).reshape(4, N, E, Hc)                  # grid index per gate block
    z = torch.from_numpy(grid[idx]).permute(1, 2, 0, 3).reshape(N, E, 4 * Hc).contiguous()
    c_prev = torch.from_numpy(SWEEP_C[slot % len(SWEEP_C)]).reshape(N, E, Hc).contiguous()
    done = (torch.arange(E) % 5 == 3).float()
    z64, keep = z.double(), (1.0 - done.double()).view(1, E, 1)
    gi, gf, go = (torch.sigmoid(z64[..., k * Hc:(k + 1) * Hc]) for k in range(3))
    gu = torch.tanh(z64[..., 3 * Hc:])
    c_e = gf * (c_prev.double() * keep) + gi * gu
    h_e = go * torch.tanh(c_e)
    gates = torch.full((N, E, 4 * Hc), SENTINEL, device=dev)
    c_new, h_new = torch.full((N, E, Hc), SENTINEL, device=dev), torch.full((N, E, Hc), SENTINEL, device=dev)
    bias = torch.zeros(N, 4 * Hc, device=dev)
    if path == 'cell':
        impl.cell_fwd(z.to(dev), bias, c_prev.to(dev), done.to(dev), gates, c_new, h_new)
    else:
        wh = torch.zeros(N, Hc, 4 * Hc, device=dev)
        kw = {}
        if path == 'step_bf16x3':
            impl.check_precision('bf16x3')
            kw = dict(precision='bf16x3')
        img = impl.lstm_wimage(None, wh, **kw)
        impl.lstm_step_fused(torch.zeros(N, E, Hc, device=dev), wh, bias, z.to(dev), None, c_prev.to(dev), done.to(dev), gates, c_new, h_new,
                             xs=(None, None, img), **kw)
    gt, cn, hn = gates.cpu(), c_new.cpu(), h_new.cpu()
    what = 'gate sweep (%s)' % path
    for name, t in (('gates', gt), ('c', cn), ('h', hn)):
        assert bool(torch.isfinite(t).all()), '[finite] %s: %s' % (what, name)
    sig = gt[..., :3 * Hc].reshape(N, E, 3, Hc).permute(2, 0, 1, 3).reshape(3, S).numpy()      # [gate, slot]
    tnh = gt[..., 3 * Hc:].reshape(S).numpy()
    zi = grid[idx.reshape(4, S)]
    zs, zt = zi[:3], zi[3]
    assert np.all(sig[zs >= 25] == 1.0) and np.all(sig[zs <= -90] == 0.0), '[saturation] %s: sigmoid' % what
    assert np.all(tnh[zt >= 10] == 1.0) and np.all(tnh[zt <= -10] == -1.0), '[saturation] %s: tanh' % what
    for k in range(3):
        lo, hi = np.full(G, np.inf), np.full(G, -np.inf)
        np.minimum.at(lo, idx.reshape(4, S)[k], sig[k])
        np.maximum.at(hi, idx.reshape(4, S)[k], sig[k])
        assert np.all(hi[:-1] <= lo[1:]), '[monotone] %s: sigmoid, gate block %d' % (what, k)
    s64 = 1.0 / (1.0 + np.exp(-zs.astype(np.float64)))
    inner = np.abs(zs) < 20
    sig_rel = float(np.max(np.abs(sig.astype(np.float64) - s64)[inner] / s64[inner]))
    tanh_abs = float(np.max(np.abs(tnh.astype(np.float64) - np.tanh(zt.astype(np.float64)))))
    print('%s: worst sigmoid relative error on |z| < 20 %.4g (bound %g), worst tanh absolute error %.4g (bound %g)'
          % (what, sig_rel, SIGMOID_REL_BOUND, tanh_abs, TANH_ABS_BOUND))
    assert sig_rel <= SIGMOID_REL_BOUND, '[sigmoid-rel] %s: %.4g > %g' % (what, sig_rel, SIGMOID_REL_BOUND)
    assert tanh_abs <= TANH_ABS_BOUND, '[tanh-abs] %s: %.4g > %g' % (what, tanh_abs, TANH_ABS_BOUND)
    exp_g = torch.cat([gi, gf, go, gu], dim=-1)
    _close(what + ' gates', gt, exp_g, tag='close', **SWEEP_TOL)
    _close(what + ' c', cn, c_e, tag='close', **SWEEP_TOL)
    _close(what + ' h', hn, h_e, tag='close', **SWEEP_TOL)
    return sig_rel, tanh_abs


def forward_cells(gates, c0, done):
    """The cell-state sequence a forward pass saves with these gates, in float32, operation for operation the forward kernels':
    c[t + 1] = gf (c[t] keep_t) + gi gu (the one-launch BPTT kernel recomputes c_t from the gates)."""
    N, T, E, H4 = gates.shape
    Hh = H4 // 4
    call = torch.empty(N, T + 1, E, Hh)
    call[:, 0] = c0
    for t in range(T):
        keep = (1.0 - done[t]).view(1, E, 1)
        call[:, t + 1] = gates[:, t, :, Hh:2 * Hh] * (call[:, t] * keep) + gates[:, t, :, :Hh] * gates[:, t, :, 3 * Hh:]
    return call


def saturated_gates(g, *shape):
    """[..., 4H] gates (sigmoid | tanh of randn) with a quarter of the entries overwritten by exactly 0.0 or 1.0 (i, f, o) and
    -1.0 or +1.0 (the candidate gate)."""
    r = torch.randn(*shape, 4 * H, generator=g)
    gates = torch.cat([torch.sigmoid(r[..., :3 * H]), torch.tanh(r[..., 3 * H:])], dim=-1)
    hit = torch.rand(*shape, 4 * H, generator=g) < 0.25
    one = torch.rand(*shape, 4 * H, generator=g) < 0.5
    sat = torch.where(one, torch.ones(()), torch.zeros(()))
    sat[..., 3 * H:] = sat[..., 3 * H:] * 2 - 1
    return torch.where(hit, sat, gates), hit


def _cell_bwd64(gates, c_prev, c_new, done, g_h, dc):
    """agents/utils.py:102-113 backwards from the saved gates, float64 -> (dz, dc_prev)."""
    gi, gf, go, gu = gates.double().split(H, dim=-1)
    keep = (1.0 - done.double()).view(1, -1, 1)
    tc = torch.tanh(c_new.double())
    g_c = dc + g_h * go * (1 - tc * tc)
    dz = torch.cat([g_c * gu * gi * (1 - gi), g_c * (c_prev.double() * keep) * gf * (1 - gf), g_h * tc * go * (1 - go), g_c * gi * (1 - gu * gu)], dim=-1)
    return dz, g_c * gf * keep


def _zero_factor(gates):
    """Where the gate's own derivative factor is exactly 0: gi, gf, go in {0, 1}; gu = +-1 or gi = 0 (d z_u carries the factor gi)."""
    gi, gf, go, gu = gates.split(H, dim=-1)
    sat = lambda t: (t == 0) | (t == 1)                                                 # noqa: E731
    return torch.cat([sat(gi), sat(gf), sat(go), (gu.abs() == 1) | (gi == 0)], dim=-1)


BPTT_SAT_PARTS = ['cell_bwd', 'step_km0', 'step_km64', 'seq']


def check_bptt_saturated(impl, dev, part):
    """The cell backward with gates that are exactly 0 / 1 / +-1 in a quarter of the entries, through cell_bwd, bptt_step (KM = 0 and
    64) and bptt_seq (N, T, E = 2, 3, 70; cell trace from forward_cells) against float64: dz / dc_prev rtol 2e-5, atol 3e-6 and the
    products rtol 1e-4, atol 2e-5 (test_lstm_bptt_step_fused's); bptt_seq rtol 1e-4, atol 2e-5, db atol 1e-4 max(1, |db|)
    (test_lstm_bptt_seq_one_launch's).  dz is exactly 0 wherever the gate's derivative factor is."""
    g = torch.Generator().manual_seed(BPTT_SAT_PARTS.index(part) + 41)
    r = lambda *s: torch.randn(*s, generator=g)                                         # noqa: E731
    c = lambda t: None if t is None else t.to(dev)                                      # noqa: E731
    worst = 0.0
    if part == 'seq':
        N, T, E = 2, 3, 70
        gates, hit = saturated_gates(g, N, T, E)
        done = (torch.rand(T, E, generator=g) < 0.2).float()
        call = forward_cells(gates, r(N, E, H) * 0.8, done)
        dhs = r(N, T, E, H)
        wh = r(N, H, 4 * H) * 0.1 + torch.arange(4 * H).view(1, 1, -1) * 1e-4 + torch.arange(H).view(1, -1, 1) * 2e-4
        dz_e = torch.empty(N, T, E, 4 * H, dtype=F64)
        dc, dh_rec = torch.zeros(N, E, H, dtype=F64), torch.zeros(N, E, H, dtype=F64)
        for t in range(T - 1, -1, -1):
            dz_e[:, t], dc = _cell_bwd64(gates[:, t], call[:, t], call[:, t + 1], done[t], dhs[:, t].double() + dh_rec, dc)
            dh_rec = torch.bmm(dz_e[:, t], wh.double().transpose(1, 2)) * (1.0 - done[t].double()).view(1, E, 1)
        db_e = dz_e.sum(dim=(1, 2))
        Gd, Cd, Dd = c(gates), c(call), c(dhs)
        dZ = torch.full((N, T, E, 4 * H), SENTINEL, device=dev)
        img = impl.lstm_bptt_wimage(None, c(wh))
        db, dh0, dc0 = impl.bptt_seq(Gd, Cd, c(done), Dd, img, dZ, want_state_grad=True)
        worst = max(_close('bptt_seq dz', dZ, dz_e, 1e-4, 2e-5), _close('bptt_seq dh0', dh0, dh_rec, 1e-4, 2e-5),
                    _close('bptt_seq dc0', dc0, dc, 1e-4, 2e-5),
                    _close('bptt_seq db', db, db_e, 1e-4, 1e-4 * max(1.0, float(db_e.abs().max()))))
        zero = _zero_factor(gates)
        assert bool(hit.any()) and float(zero.float().mean()) > 0.2
        assert bool((dZ.cpu()[zero] == 0).all()), 'dz is not exactly 0 where the derivative factor is'
        return worst
    N, E = 3, 130
    KM = 64 if part == 'step_km64' else 0
    gates, hit = saturated_gates(g, N, E)
    c_prev, c_new = r(N, E, H), r(N, E, H) * 0.8
    done = (torch.rand(E, generator=g) < 0.3).float()
    dh, dh2, dcin = r(N, E, H), r(N, E, H), r(N, E, H)
    dz_e, dcp_e = _cell_bwd64(gates, c_prev, c_new, done, dh.double() + dh2.double(), dcin.double())
    dz = torch.full((N, E, 4 * H), SENTINEL, device=dev)
    dcp = torch.full((N, E, H), SENTINEL, device=dev)
    if part == 'cell_bwd':
        impl.cell_bwd(c(gates), c(c_prev), c(c_new), c(done), c(dh), c(dcin), dz, dcp, dh2=c(dh2))
    else:
        wh = r(N, H, 4 * H) * 0.2 + torch.arange(4 * H).view(1, 1, -1) * 1e-3 + torch.arange(H).view(1, -1, 1) * 2e-3
        wxm = None if KM == 0 else r(N, KM, 4 * H) * 0.2 + torch.arange(4 * H).view(1, 1, -1) * 1e-3
        mask = None if KM == 0 else torch.relu(r(N, E, H))
        ws = (c(wxm), c(wh), impl.lstm_bptt_wimage(c(wxm), c(wh)))
        dhd = torch.full((N, E, H), SENTINEL, device=dev)
        dx = None if KM == 0 else torch.full((N, E, H), SENTINEL, device=dev)
        impl.bptt_step(c(gates), c(c_prev), c(c_new), c(done), c(dh), c(dh2), c(dcin), ws, dz, dcp, dhd, True, dx=dx, mask=c(mask))
        dhd_e = torch.bmm(dz_e, wh.double().transpose(1, 2)) * (1.0 - done.double()).view(1, E, 1)
        worst = max(worst, _close(part + ' dhd', dhd, dhd_e, 1e-4, 2e-5))
        if KM:
            dx_e = torch.bmm(dz_e, wxm.double().transpose(1, 2)) * (mask > 0).double()
            worst = max(worst, _close(part + ' dx', dx, dx_e, 1e-4, 2e-5))
    worst = max(worst, _close(part + ' dz', dz, dz_e, 2e-5, 3e-6), _close(part + ' dc_prev', dcp, dcp_e, 2e-5, 3e-6))
    zero = _zero_factor(gates)
    assert bool(hit.any()) and float(zero.float().mean()) > 0.2
    assert bool((dz.cpu()[zero] == 0).all()), 'dz is not exactly 0 where the derivative factor is'
    return worst


# ------------------------------------------------------------------------------------------------- D. small things
def check_nbr_action_value_accumulate(impl, dev, rows, A=4):
    """va [N,rows] (+)= onehot(neighbours' actions) @ w_a (policies.py:66-72) on the ragged table (m_max A = 32, the widest the
    kernels take), overwriting and accumulating onto a non-zero va: rtol 1e-6, atol 1e-6 (test_heads_and_neighbour_action_value's)."""
    tab = ragged_table()
    N, m = tab.shape
    assert m * A == 32
    g = torch.Generator().manual_seed(rows + A)
    action = torch.randint(0, A, (rows, N), generator=g).to(torch.uint8)
    w_a = torch.randn(N, m * A, 1, generator=g)
    va0 = torch.randn(N, rows, generator=g)
    exp = torch.zeros(N, rows, dtype=F64)
    for i in range(N):
        for k in range(m):
            j = int(tab[i, k])
            if j >= 0:
                exp[i] += w_a[i, k * A + action[:, j].long(), 0].double()
    va = va0.to(dev).clone()
    got = impl.nbr_action_value(action.to(dev), tab.to(dev), w_a.to(dev), A, out=va, accumulate=True)
    assert got is va or _same_bits(got, va)
    worst = _close('nbr_action_value accumulate rows=%d' % rows, va, va0.double() + exp, 1e-6, 1e-6)
    assert bool((exp[0] == 0).all()) and _same_bits(va[0], va0[0])                       # agent 0 has no neighbour: its va keeps its bits
    impl.nbr_action_value(action.to(dev), tab.to(dev), w_a.to(dev), A, out=va, accumulate=False)
    worst = max(worst, _close('nbr_action_value overwrite rows=%d' % rows, va, exp, 1e-6, 1e-6))
    return worst


def check_onehot_argmax_ties(impl, dev):
    """y[n, r, argmax_a p] += scale[n] (agents/utils.py:577-579): the FIRST maximum on ties (tf.argmax), A = 1, a per-agent scale;
    y a column block of a wider buffer.  Equal to the expectation bit for bit (one fp32 addition)."""
    N, E = 3, 77
    for A in (1, 3, 8):
        g = torch.Generator().manual_seed(A)
        p = torch.softmax(torch.randn(N, E, A, generator=g), dim=-1)
        p[:, ::3] = 1.0 / A                                          # all equal: index 0
        if A >= 3:
            p[:, 1::7, A - 1] = p[:, 1::7, 1] = 2.0                  # the last and the second: index 1
        want = torch.from_numpy(np.argmax(p.numpy(), axis=-1))       # np.argmax: the first maximum
        y0 = torch.randn(N, E, 64, generator=g)
        scale = torch.tensor([0.5, -2.0, 3.0])
        for sc in (None, scale):
            exp = y0.clone()
            add = torch.ones(N) if sc is None else sc
            for n in range(N):
                exp[n, torch.arange(E), want[n]] += add[n]
            wide = torch.full((N, E, 192), SENTINEL, device=dev)
            view = wide[:, :, 64:128]
            view.copy_(y0)
            impl.onehot_argmax_add_(view, p.to(dev), None if sc is None else sc.to(dev))
            assert torch.equal(view.cpu(), exp), 'A = %d, scale %s' % (A, sc is not None)
            assert bool((wide.cpu()[:, :, :64] == SENTINEL).all()) and bool((wide.cpu()[:, :, 128:] == SENTINEL).all())
    return 0.0


def check_thin_linear_bwd_o8(impl, dev, rows):
    """The heads' backward at the widest output count (O = 8) with the last column's gradient handed over separately (dy2):
    dh = dy w^T (rtol 1e-5, atol 1e-5), dw = h^T dy, db = sum dy (rtol 1e-4, atol 2e-5 sqrt(rows)) -- test_thin_linear_bwd's."""
    N, O = 3, 8
    g = torch.Generator().manual_seed(rows)
    h, dy, w = torch.randn(N, rows, 64, generator=g), torch.randn(N, rows, O, generator=g), torch.randn(N, 64, O, generator=g)
    dh_e, dw_e, db_e = torch.bmm(dy.double(), w.double().transpose(1, 2)), torch.bmm(h.double().transpose(1, 2), dy.double()), dy.double().sum(1)
    dh, dw, db = impl.thin_linear_bwd(h.to(dev), dy[..., :O - 1].contiguous().to(dev), w.to(dev), dy2=dy[..., O - 1].contiguous().to(dev))
    atol = 2e-5 * float(rows) ** 0.5
    what = 'thin_linear_bwd O=8 dy2 rows=%d' % rows
    return max(_close(what + ' dh', dh, dh_e, 1e-5, 1e-5), _close(what + ' dw', dw, dw_e, 1e-4, atol), _close(what + ' db', db, db_e, 1e-4, atol))

"""Edge checks of the reverse-recurrence kernels (csrc/lstm_bptt.hip: nmarl_lstm_bptt_step / _seq / _coupled / _dial), written as
functions of the implementation under test: `ops` on the GPU (tests/test_gpu_bptt_edges.py), the restatement `oracle/ops_ref` or a
deliberately wrong variant of it on the CPU (tests/test_bptt_edges_cpu.py, which proves that the checks are sharp).  Each check
draws its inputs from a seeded generator, forms the expectation in float64 (the cell backward of agents/utils.py:102-113 and the
transposed products restated here; the coupled and dial recurrences through oracle/ops_ref.bptt_coupled / bptt_dial on float64
operands), asserts, prints the worst share of its bound that was used, and returns it.

A test cannot observe which kernel the launcher chose.  Every check therefore asserts, on the tensors and arguments it built, the
PRECONDITIONS of the branch it is meant for (KM, which optional operands are None, the table's m_max, fan-in and symmetry, the
form of the heads' gradient, the ring's slot count): an edit of the inputs that moves a case to another branch fails the check.

Dispatch census: every instantiation behind the hipLaunchKernelGGL sites of lstm_bptt.hip.  kind 1 = lstm_comm, 2 = lstm_ic3;
coupled<NTM,RMAX,MASK,DY[,DIAL]> = lstm_bptt_coupled_kernel; NTM = 4 m_max (kind 1 / dial) or 4 (kind 2), RMAX = 2 for a fan-in
<= 2 else 4, DY = the heads' gradient comes as dy8.  Test ids: [E] tests/test_gpu_bptt_edges.py, [O] tests/test_gpu_ops.py,
[D] tests/test_gpu_bptt_dial.py.

  instantiation                 selected when (file:line)                                    test, parameters
  ----------------------------  -----------------------------------------------------------  ---------------------------------------------------------
  lstm_bptt_wimage_kernel       every nmarl_lstm_bptt_wimage (lstm_bptt.hip:1278)            [E] every test (KM = 0 and 64); [O] test_lstm_bptt_step_fused
  lstm_bptt_msg_wimage_kernel   every nmarl_lstm_bptt_msg_wimage (:1381)                     [E] test_coupled_edges (K = 64, 128), test_dial_edges; [O] test_lstm_bptt_coupled_one_launch
  step<4>                       KM == 0 (:1322)                                              [E] test_step_operands (KM = 0 half), test_seq_edges (the step-wise twin), test_saturation entry=step; [O] test_lstm_bptt_step_fused KM=0
  step<8>                       KM == 64 (:1323)                                             [E] test_step_operands (KM = 64, mask absent / present), test_tanh_midrange; [O] test_lstm_bptt_step_fused KM=64
  seq<false>                    dh_ext given (:1370)                                         [E] test_seq_edges (tensor form), test_saturation entry=seq; [O] test_lstm_bptt_seq_one_launch
  seq<true>                     dy8 given (:1367)                                            [E] test_seq_edges (O = 1, 4, 5, 7, 8); [O] test_lstm_bptt_seq_expands_the_heads_gradient_itself
  coupled<8,2,true,false>       kind 1, m_max 2, fan-in <= 2, dh_ext (:1531, :1405)          [E] test_coupled_edges kind=1 table=line3,ragged form=tensor; [O] test_lstm_bptt_coupled_one_launch kind=1 N=8,3
  coupled<8,2,true,true>        kind 1, m_max 2, fan-in <= 2, dy8 (:1531, :1404)             [E] test_coupled_edges kind=1 table=line3,ragged form=dy8; [O] test_lstm_bptt_coupled_expands_... kind=1
  coupled<4,2,true,false>       kind 1, m_max 1, dh_ext (:1532, :1405)                       [E] test_coupled_edges kind=1 table=line2 form=tensor; [O] test_lstm_bptt_coupled_one_launch (1, line, 2, 3, 1)
  coupled<4,2,true,true>        kind 1, m_max 1, dy8 (:1532, :1404)                          [E] test_coupled_edges kind=1 table=line2 form=dy8 (nothing else)
  coupled<4,2,false,false>      kind 2, fan-in <= 2, dh_ext (:1533, :1405)                   [E] test_coupled_edges kind=2 table=line3 form=tensor; [O] test_lstm_bptt_coupled_one_launch kind=2 line
  coupled<4,2,false,true>       kind 2, fan-in <= 2, dy8 (:1533, :1404)                      [E] test_coupled_edges kind=2 table=line3 form=dy8; [O] test_lstm_bptt_coupled_expands_... (2, line, 8, 7, 300, 5)
  coupled<4,4,false,false>      kind 2, fan-in 3..4, dh_ext (:1534, :1405)                   [E] test_coupled_edges kind=2 table=grid,grid_cut form=tensor; [O] test_lstm_bptt_coupled_one_launch kind=2 grid
  coupled<4,4,false,true>       kind 2, fan-in 3..4, dy8 (:1534, :1404)                      [E] test_coupled_edges kind=2 table=grid,grid_cut form=dy8; [O] test_lstm_bptt_coupled_expands_... kind=2 grid
  coupled<8,2,true,false,true>  dial, m_max 2, dh_ext (:1643, :1554)                         [E] test_dial_edges table=line3,ragged form=tensor; [D] test_bptt_dial_against_float64
  coupled<8,2,true,true,true>   dial, m_max 2, dy8 (:1643, :1553)                            [E] test_dial_edges table=line3,ragged form=dy8; [D] test_bptt_dial_forms_agree
  coupled<4,2,true,false,true>  dial, m_max 1, dh_ext (:1643, :1554)                         [D] test_bptt_dial_against_float64 (2, 3, 1, line)
  coupled<4,2,true,true,true>   dial, m_max 1, dy8 (:1643, :1553)                            [D] test_bptt_dial_forms_agree (2, 3, 1, line)
  zero_words_kernel             every nmarl_lstm_bptt_coupled / _dial call (:1510, :1630)    [E] test_coupled_edges, test_dial_edges; [O] test_lstm_bptt_coupled_one_launch

The launchers' own choices (:1518, :1633: one launch if mode != 2, ring_slots >= T and (mode == 1 or (symmetric and grid <= cap))):
  asymmetric table, mode 0 -> step-wise     [E] test_coupled_edges table=ragged,grid_cut; test_dial_edges table=ragged
  ring_slots (2) < T, mode 1 -> step-wise   [E] test_launcher_fallbacks (ops.COUPLED_RING_MAX_BYTES one byte short of T slots)
  mode 0, symmetric, grid > cap             [E] test_launcher_fallbacks (NMARL_TEST_FAKE_CUS=1)
  mode 0, symmetric, grid <= cap            [E] test_launcher_fallbacks (mode 0 without the variable == mode 1)
What the launchers refuse: check_refusals."""
import itertools

import torch

from fc_edge_checks import SENTINEL, _same_bits
from oracle import ops_ref

F32, F64 = torch.float32, torch.float64
H = 64
E_EDGES = (1, 15, 16, 17, 127, 128, 129, 257)       # around a wave (16 rows) and a tile (128 rows); two tiles + 1
T_EDGES = (1, 2, 3)                                  # 2: the shortest with slot parity and the prefetch of step t - 1 both running
N_AGENTS = 3
COUPLED_E = (1, 17, 129)
STEP_TOL = dict(rtol=2e-5, atol=3e-6)                # test_lstm_bptt_step_fused: dz, dc_prev
PROD_TOL = dict(rtol=1e-4, atol=2e-5)                # test_lstm_bptt_step_fused: dhd, dx; test_lstm_bptt_seq_one_launch: everything
COUPLED_TOL = dict(rtol=2e-4, atol=5e-5)             # test_lstm_bptt_coupled_one_launch
GARBAGE = 1e30
PAD_ROWS = 5                                         # rows past E in every padded output buffer


# ----------------------------------------------------------------------------------------------------------- tables
def line_table(N):
    """The CACC line (ops.neighbor_table of it): ascending, -1 padded; N = 2: m_max 1."""
    m = 1 if N == 2 else 2
    tab = -torch.ones(N, m, dtype=torch.int32)
    for i in range(N):
        js = [j for j in (i - 1, i + 1) if 0 <= j < N]
        tab[i, :len(js)] = torch.tensor(js, dtype=torch.int32)
    return tab


def grid_table(cut=False):
    """The 3 x 3 grid (m_max 4; the centre has 4 sources).  cut: three directed edges deleted (0 -> 1, 0 -> 3, 8 -> 7): agent 0 keeps
    its sources 1 and 3 but has no neighbour, the relation is asymmetric."""
    tab = -torch.ones(9, 4, dtype=torch.int32)
    for i in range(9):
        r, c = divmod(i, 3)
        js = sorted(rr * 3 + cc for rr, cc in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)) if 0 <= rr < 3 and 0 <= cc < 3)
        if cut:
            js = [j for j in js if (i, j) not in ((0, 1), (0, 3), (8, 7))]
        tab[i, :len(js)] = torch.tensor(js, dtype=torch.int32)
    return tab


def ragged_table():
    """test_gpu_bptt_dial._table(6, 'ragged'): asymmetric, -1 padded, m_max 2, fan-in <= 2; agents 3 and 5 have no neighbour, 5 no
    source either."""
    idx = -torch.ones(6, 2, dtype=torch.int32)
    idx[0, 0], idx[1, 0], idx[1, 1], idx[2, 0], idx[4, 0], idx[4, 1] = 3, 0, 3, 1, 1, 2
    return idx


TABLES = {'line2': lambda: line_table(2), 'line3': lambda: line_table(3), 'ragged': ragged_table, 'grid': grid_table,
          'grid_cut': lambda: grid_table(True)}
COUPLED_TABLES = {1: ('line2', 'line3', 'ragged'), 2: ('line3', 'grid', 'grid_cut')}
DIAL_TABLES = ('line3', 'ragged')
# (kind, table) -> (NTM, RMAX) of the instantiation the launcher picks (lstm_bptt.hip:1531-1534); kind 3: the dial forms
INSTANTIATION = {(1, 'line2'): (4, 2), (1, 'line3'): (8, 2), (1, 'ragged'): (8, 2), (2, 'line3'): (4, 2), (2, 'grid'): (4, 4),
                 (2, 'grid_cut'): (4, 4), (3, 'line3'): (8, 2), (3, 'ragged'): (8, 2)}


def table_facts(tab):
    """-> (fan-in maximum, symmetric) of a neighbour table."""
    N = tab.shape[0]
    nb = [set(int(j) for j in tab[i] if j >= 0) for i in range(N)]
    fan = [sum(1 for a in range(N) if i in nb[a]) for i in range(N)]
    return max(1, max(fan)), all(i in nb[j] for i in range(N) for j in nb[i])


# ----------------------------------------------------------------------------------------------------- inputs, buffers
def _rand(seed):
    g = torch.Generator().manual_seed(seed)
    return (lambda *s: torch.randn(*s, generator=g)), (lambda *s: torch.rand(*s, generator=g))


def _gates(r, *lead):
    return torch.cat([torch.sigmoid(r(*lead, 3 * H)), torch.tanh(r(*lead, H))], dim=-1)


def forward_cells(gates, c0, done):
    """The cell-state sequence a forward pass would have saved with these gates: c[t + 1] = gf * (c[t] * keep_t) + gi * gu in float32,
    operation for operation what the forward kernels compute -- the one-launch kernels recompute c_t from the gates."""
    N, T, E, _ = gates.shape
    call = torch.empty(N, T + 1, E, H)
    call[:, 0] = c0
    for t in range(T):
        keep = (1.0 - done[t]).view(1, E, 1)
        call[:, t + 1] = gates[:, t, :, H:2 * H] * (call[:, t] * keep) + gates[:, t, :, :H] * gates[:, t, :, 3 * H:]
    return call


def _in_slot(x, dev):
    """[N,E,W] -> slot 1 of a zeroed [N,3,E,W] buffer on `dev` (the agent stride is three panels)."""
    N, E, W = x.shape
    buf = torch.zeros(N, 3, E, W, device=dev)
    buf[:, 1].copy_(x)
    return buf[:, 1]


def _in_seq(x, dev):
    """[N,T,E,W] -> slabs 1 .. T of a zeroed [N,T+2,E,W] buffer on `dev`."""
    N, T, E, W = x.shape
    buf = torch.zeros(N, T + 2, E, W, device=dev)
    buf[:, 1:T + 1].copy_(x)
    return buf[:, 1:T + 1]


class Out:
    """An output operand: rows 0 .. E - 1 of slot 1 ([N,E,W]) or of slabs 1 .. T ([N,T,E,W]) of a sentinel-filled buffer with
    PAD_ROWS more rows per panel and a guard slab on either side."""

    def __init__(self, dev, N, E, W, T=None):
        self.buf = torch.full((N, 3 if T is None else T + 2, E + PAD_ROWS, W), SENTINEL, device=dev)
        self.idx = (slice(None), 1, slice(0, E)) if T is None else (slice(None), slice(1, T + 1), slice(0, E))
        self.v = self.buf[self.idx]
        assert self.v.stride(-1) == 1 and self.v.stride(-2) == W and self.v.data_ptr() % 16 == 0

    def kept(self):
        c = self.buf.clone()
        c[self.idx] = SENTINEL
        return bool((c == SENTINEL).all())

    def written(self):
        return not bool((self.v == SENTINEL).any())

    def cpu(self):
        return self.v.detach().cpu()


def _assert_outs(outs, what):
    for name, o in outs.items():
        assert o.kept(), '[guards] %s: a guard slab or a row >= E of %s was written' % (what, name)
        assert o.written(), '[written] %s: %s keeps a sentinel (a row was left out)' % (what, name)


def _sync(impl, dev):
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize()
        impl.check_coupled_status()


# --------------------------------------------------------------------------------------------- the expectation in float64
def cell_bwd64(gates, c_prev, c_new, done, dh, dh2, dc):
    """agents/utils.py:102-113 differentiated, from the saved post-activation gates.  -> (dz [.,4H], dc_prev, parts) in float64;
    parts: the factors the tanh bound of check_tanh_midrange needs."""
    gi, gf, go, gu = gates.double().split(H, dim=-1)
    keep = (1.0 - done.double()).view(1, -1, 1)
    tc = torch.tanh(c_new.double())
    gh = torch.zeros_like(tc)
    for x in (dh, dh2):
        if x is not None:
            gh = gh + x.double()
    gc = gh * go * (1 - tc * tc)
    if dc is not None:
        gc = gc + dc.double()
    cpk = c_prev.double() * keep
    dz = torch.cat([gc * gu * gi * (1 - gi), gc * cpk * gf * (1 - gf), gh * tc * go * (1 - go), gc * gi * (1 - gu * gu)], dim=-1)
    return dz, gc * gf * keep, dict(gi=gi, gf=gf, go=go, gu=gu, keep=keep, tc=tc, gh=gh, cpk=cpk)


def seq64(gates, call, done, dhs, wh):
    """T reverse steps: cell_bwd64, then dh_rec = (dz wh^T) (1 - done_t).  -> (dz [N,T,E,4H], dh0, dc0)."""
    N, T, E, _ = gates.shape
    dz = torch.zeros(N, T, E, 4 * H, dtype=F64)
    dc, dh_rec = None, None
    for t in range(T - 1, -1, -1):
        dz[:, t], dc, _ = cell_bwd64(gates[:, t], call[:, t], call[:, t + 1], done[t], dhs[:, t], dh_rec, dc)
        dh_rec = torch.bmm(dz[:, t], wh.double().transpose(1, 2)) * (1.0 - done[t].double()).view(1, -1, 1)
    return dz, dh_rec, dc


def _done_pattern(name, T, E, u):
    done = torch.zeros(T, E)
    if name == 'last':
        done[T - 1] = 1.0
    elif name == 'first':
        done[0] = 1.0
    elif name == 'random':
        done = (u(T, E) < 0.3).float()
    else:
        assert name == 'none'
    return done


def _weights(r, N, scale=0.1):
    """Asymmetric recurrent and x-side weights: a swapped row / column of the image cannot pass."""
    wh = r(N, H, 4 * H) * scale + torch.arange(4 * H).view(1, 1, -1) * 1e-4 + torch.arange(H).view(1, -1, 1) * 2e-4
    wxm = r(N, H, 4 * H) * scale + torch.arange(4 * H).view(1, 1, -1) * 1e-4
    return wh, wxm


# ------------------------------------------------------------------------------ 1. bptt_step: the cross of optional operands
def check_step_operands(impl, dev, E, N=N_AGENTS):
    """nmarl_lstm_bptt_step over dh / dh2 / dc each present or absent x apply_keep 0 / 1 x (KM = 0 | KM = 64 without mask | KM = 64
    with the mask a column slice of a 192-pitch buffer that holds exact +0 and -0), each also with db_part handed over and called
    twice.  dz / dc_prev at STEP_TOL, dhd / dx at PROD_TOL against float64; dx exactly 0 where the mask is <= 0; the db_part runs
    bit-equal to the plain run and db_part.sum(1) = 2 column sums of dz (rtol 1e-4, atol 2e-5 sqrt(E):
    test_lstm_bptt_step_fused's); inputs slots of zeroed wider buffers, outputs rows of sentinel-filled padded ones that stay
    untouched outside rows 0 .. E - 1."""
    assert E in E_EDGES and N <= 9
    r, u = _rand(E * 31 + 7)
    gates, c_prev, c_new = _gates(r, N, E), r(N, E, H), r(N, E, H) * 0.8
    done = (u(E) < 0.3).float()
    done[0] = 0.0
    if E > 1:
        done[E - 1] = 1.0                                  # (the last row of the last tile is finished)
    opt = dict(dh=r(N, E, H), dh2=r(N, E, H), dc=r(N, E, H))
    wh, wxm = _weights(r, N, 0.2)
    hm = torch.relu(r(N, E, 3 * H))
    hm[:, ::2, 2 * H + 1::5] = -0.0
    mask = hm[:, :, 2 * H:]
    assert bool((mask == 0).any()) and bool(torch.signbit(mask).any()) and bool((mask > 0).any())
    t = lambda x: x.to(dev)                                                             # noqa: E731
    Gd, Cd, doned, whd, wxd, hmd = _in_slot(gates, dev), torch.zeros(N, 4, E, H, device=dev), t(done), t(wh), t(wxm), t(hm)
    Cd[:, 1].copy_(c_prev), Cd[:, 2].copy_(c_new)
    optd = {k: _in_slot(v, dev) for k, v in opt.items()}
    assert Gd.stride(0) == 3 * E * 4 * H and hmd[:, :, 2 * H:].stride(1) == 3 * H
    worst, ncomb = 0.0, 0
    for KM, masked in ((0, False), (64, False), (64, True)):
        ws = (wxd if KM else None, whd, impl.lstm_bptt_wimage(wxd if KM else None, whd))
        for has in itertools.product((True, False), repeat=3):
            for keep in (1, 0):
                sel = {k: (opt[k] if h else None) for k, h in zip(('dh', 'dh2', 'dc'), has)}
                seld = {k: (optd[k] if h else None) for k, h in zip(('dh', 'dh2', 'dc'), has)}
                what = 'step E=%d KM=%d mask=%d dh=%d dh2=%d dc=%d keep=%d' % ((E, KM, masked) + tuple(map(int, has)) + (keep,))
                assert (ws[0] is None) == (KM == 0) and all((seld[k] is None) == (not h) for k, h in zip(('dh', 'dh2', 'dc'), has))
                dz64, dcp64, _ = cell_bwd64(gates, c_prev, c_new, done, sel['dh'], sel['dh2'], sel['dc'])
                dhd64 = torch.bmm(dz64, wh.double().transpose(1, 2))
                if keep:
                    dhd64 = dhd64 * (1.0 - done.double()).view(1, -1, 1)
                dx64 = torch.bmm(dz64, wxm.double().transpose(1, 2)) * ((mask > 0) if masked else 1.0) if KM else None
                runs = []
                for with_db in (False, True):
                    o = dict(dz=Out(dev, N, E, 4 * H), dcp=Out(dev, N, E, H), dhd=Out(dev, N, E, H))
                    if KM:
                        o['dx'] = Out(dev, N, E, H)
                    part = impl.bptt_step_db_parts(N, E, H, dev) if with_db else None
                    for _ in range(2 if with_db else 1):
                        impl.bptt_step(Gd, Cd[:, 1], Cd[:, 2], doned, seld['dh'], seld['dh2'], seld['dc'], ws, o['dz'].v, o['dcp'].v,
                                       o['dhd'].v, bool(keep), dx=o['dx'].v if KM else None, mask=hmd[:, :, 2 * H:] if masked else None,
                                       db_part=part)
                    _assert_outs(o, what)
                    runs.append((o, part))
                (o, _), (o2, part) = runs
                for k in o:
                    assert _same_bits(o[k].v, o2[k].v), '[bits] %s: %s differs once db_part is handed over' % (what, k)
                used = [_used_tag('close', what + ' dz', o['dz'].v, dz64, **STEP_TOL), _used_tag('close', what + ' dc_prev', o['dcp'].v, dcp64, **STEP_TOL),
                        _used_tag('close', what + ' dhd', o['dhd'].v, dhd64, **PROD_TOL)]
                if KM:
                    used.append(_used_tag('close', what + ' dx', o['dx'].v, dx64, **PROD_TOL))
                    if masked:
                        assert bool((o['dx'].cpu()[~(mask > 0)] == 0).all()), '[mask] %s: dx is not exactly 0 where the mask is <= 0' % what
                used.append(_used_tag('db', what + ' db_part', part.sum(1), 2 * dz64.sum(1), rtol=1e-4, atol=2e-5 * max(1.0, E ** 0.5)))
                worst = max(worst, max(used))
                ncomb += 1
    assert ncomb == 48
    print('step operands E=%d: %d combinations, %.3g of a bound at worst' % (E, ncomb, worst))
    return worst


def _used_tag(tag, what, got, exp, rtol, atol):
    """fc_edge_checks._close without a line per call: -> the share of the bound used; raises '[tag] ...' past it."""
    got, exp = got.detach().cpu().double(), exp.detach().cpu().double()
    assert got.shape == exp.shape, (tuple(got.shape), tuple(exp.shape))
    assert bool(torch.isfinite(got).all()), '[%s] %s: not finite' % (tag, what)
    if got.numel() == 0:
        return 0.0
    share = (got - exp).abs() / (atol + rtol * exp.abs())
    used = float(share.max())
    assert used <= 1.0, '[%s] %s: %.3g of its bound (rtol %g, atol %.3g), off by %.3g' % (tag, what, used, rtol, atol, float((got - exp).abs().max()))
    return used


# ---------------------------------------------------------------------------------------- 2. bptt_seq: T, E and done edges
SEQ_DONE = ('none', 'last', 'first', 'random')
SEQ_O = (1, 4, 5, 7, 8)


def check_seq_edges(impl, dev, T, E, N=N_AGENTS):
    """nmarl_lstm_bptt_seq at T in T_EDGES, E in E_EDGES: done patterns none / all ones at t = T - 1 / all ones at t = 0 / random,
    each with want_db and want_state_grad on or off.  dz, dh0, dc0 against float64 at PROD_TOL, db at rtol 1e-4, atol 1e-4 max(1,
    |db|) (test_lstm_bptt_seq_one_launch's); dz, dh0, dc0 bit for bit the T launches of bptt_step; all ones at t = 0: dh0 and dc0
    exactly 0.  The dy8 form at O in SEQ_O against the tensor form on dL/dh = dy hw^T (float64 product rounded once) at rtol 2e-5,
    atol 2e-6 max (test_lstm_bptt_seq_expands_the_heads_gradient_itself's)."""
    assert T in T_EDGES and E in E_EDGES
    r, u = _rand(T * 1009 + E * 13 + 1)
    gates, c0, dhs = _gates(r, N, T, E), r(N, E, H) * 0.8, r(N, T, E, H)
    wh, _ = _weights(r, N)
    t = lambda x: x.to(dev)                                                             # noqa: E731
    whd = t(wh)
    img = impl.lstm_bptt_wimage(None, whd)
    Gd, Dd = _in_seq(gates, dev), _in_seq(dhs, dev)
    worst = 0.0
    for pattern in SEQ_DONE:
        done = _done_pattern(pattern, T, E, u)
        call = forward_cells(gates, c0, done)
        Cd = torch.zeros(N, T + 3, E, H, device=dev)
        Cd[:, 1:T + 2].copy_(call)
        doned = t(done)
        dz64, dh064, dc064 = seq64(gates, call, done, dhs, wh)
        db64 = dz64.sum(dim=(1, 2))
        # the step-wise twin
        dz2 = Out(dev, N, E, 4 * H, T=T)
        dc, dcn = torch.zeros(N, E, H, device=dev), torch.empty(N, E, H, device=dev)
        dh_a, dh_b, dh_rec = torch.empty(N, E, H, device=dev), torch.empty(N, E, H, device=dev), None
        for s in range(T - 1, -1, -1):
            impl.bptt_step(Gd[:, s], Cd[:, 1 + s], Cd[:, 2 + s], doned[s], Dd[:, s], dh_rec, dc, (None, whd, img), dz2.v[:, s], dcn, dh_a, True)
            dc, dcn = dcn, dc
            dh_rec, dh_a, dh_b = dh_a, dh_b, dh_a
        for want_db, want_state in itertools.product((True, False), repeat=2):
            what = 'seq T=%d E=%d done=%s db=%d state=%d' % (T, E, pattern, want_db, want_state)
            dz = Out(dev, N, E, 4 * H, T=T)
            db, dh0, dc0 = impl.bptt_seq(Gd, Cd[:, 1:T + 2], doned, Dd, img, dz.v, want_db=want_db, want_state_grad=want_state)
            assert (db is None) == (not want_db) and (dh0 is None) == (not want_state) and (dc0 is None) == (not want_state), what
            _assert_outs(dict(dz=dz), what)
            assert _same_bits(dz.v, dz2.v), '[bits] %s: dz differs from the T launches of bptt_step' % what
            worst = max(worst, _used_tag('close', what + ' dz', dz.v, dz64, **PROD_TOL))
            if want_state:
                assert _same_bits(dh0, dh_rec) and _same_bits(dc0, dc), '[bits] %s: dh0 / dc0 differ from the T launches of bptt_step' % what
                worst = max(worst, _used_tag('close', what + ' dh0', dh0, dh064, **PROD_TOL), _used_tag('close', what + ' dc0', dc0, dc064, **PROD_TOL))
                if pattern == 'first':
                    assert float(dh0.abs().max()) == 0.0 and float(dc0.abs().max()) == 0.0, '[done] %s: a finished step hands a gradient back' % what
            if want_db:
                worst = max(worst, _used_tag('db', what + ' db', db, db64, rtol=1e-4, atol=1e-4 * max(1.0, float(db64.abs().max()))))
                worst = max(worst, _used_tag('db', what + ' db vs its own dz', db, dz.cpu().double().sum(dim=(1, 2)), rtol=1e-5,
                                             atol=1e-6 * max(1.0, float(db64.abs().max())) * (T * E) ** 0.5))
    # the dy8 form
    done = _done_pattern('random', T, E, u)
    call = forward_cells(gates, c0, done)
    Cd = torch.zeros(N, T + 3, E, H, device=dev)
    Cd[:, 1:T + 2].copy_(call)
    for O in SEQ_O:
        what = 'seq T=%d E=%d dy8 O=%d' % (T, E, O)
        dy8 = torch.zeros(N, T * E, 8)
        dy8[:, :, :O] = r(N, T * E, O)
        hw = r(N, H, O) * 0.3
        dhs_o = torch.bmm(dy8[:, :, :O].double(), hw.double().transpose(1, 2)).float().view(N, T, E, H)
        assert hw.shape[2] == O and (O == 8 or float(dy8[:, :, O:].abs().max()) == 0.0) and float(dy8[:, :, O - 1].abs().min()) > 0.0
        out = []
        for head_dy in (None, (t(dy8), t(hw))):
            dz = Out(dev, N, E, 4 * H, T=T)
            db, dh0, dc0 = impl.bptt_seq(Gd, Cd[:, 1:T + 2], t(done), t(dhs_o) if head_dy is None else None, img, dz.v, want_db=True,
                                         want_state_grad=True, head_dy=head_dy)
            _assert_outs(dict(dz=dz), what)
            out.append((dz.v, db, dh0, dc0))
        for name, a, b in zip(('dz', 'db', 'dh0', 'dc0'), out[1], out[0]):
            worst = max(worst, _used_tag('dy8', '%s %s' % (what, name), a, b, rtol=2e-5, atol=2e-6 * float(b.abs().max())))
        dz64, _, _ = seq64(gates, call, done, dhs_o, wh)
        worst = max(worst, _used_tag('close', what + ' dz', out[1][0], dz64, **PROD_TOL))
    print('seq edges T=%d E=%d: %.3g of a bound at worst' % (T, E, worst))
    return worst


# ------------------------------------------------------------------------------------ 3. bptt_coupled: tables, T, E, forms
COUPLED_FORMS = ('tensor', 'dy8')


def _coupled_inputs(kind, tab, T, E, form, seed, O=5):
    N, m_max = tab.shape
    K = H * m_max if kind == 1 else H
    r, u = _rand(seed)
    d = dict(gates=_gates(r, N, T, E), done=(u(T, E) < 0.2).float())
    d['call'] = forward_cells(d['gates'], r(N, E, H) * 0.8, d['done'])
    d['wh'], d['wxm'] = r(N, H, 4 * H) * 0.1, r(N, H, 4 * H) * 0.1
    d['w_msg'] = r(N, K, H) * 0.15 + torch.arange(K).view(1, -1, 1) * 1e-4
    d['S'] = torch.relu(r(N, T, E, 3 * H))                # lstm_comm's saved LSTM input; its last third is the message term hm
    d['S'][:, :, ::2, 2 * H + 1::5] = -0.0
    if form == 'dy8':
        d['dy8'] = torch.zeros(N, T * E, 8)
        d['dy8'][:, :, :O] = r(N, T * E, O)
        d['hw'] = r(N, H, O) * 0.3
    else:
        d['dhs'] = r(N, T, E, H)
    return d


def check_coupled_edges(impl, dev, kind, table, T, E, form):
    """nmarl_lstm_bptt_coupled against ops_ref.bptt_coupled on float64 operands at COUPLED_TOL (bias sums: rtol 1e-4, atol 1e-4
    max(1, |.|)), the heads' gradient as a tensor or as dy8 (O = 5).  Symmetric tables: modes 1 and 2, asymmetric ones: modes 0 and 2
    (the launcher never takes the one-launch form there) -- dZ and D1 bit for bit between the two, the bias sums within summation
    order.  D1 exactly 0 where the relu mask is <= 0 (+0, -0).  Outputs rows of padded sentinel buffers between guard slabs."""
    assert kind in (1, 2) and table in COUPLED_TABLES[kind] and T in T_EDGES and E in COUPLED_E and form in COUPLED_FORMS
    tab = TABLES[table]()
    N, m_max = tab.shape
    r_max, sym = table_facts(tab)
    K = H * m_max if kind == 1 else H
    assert N <= 9 and (K // 16 if kind == 1 else 4, 2 if r_max <= 2 else 4) == INSTANTIATION[kind, table]
    assert sym == (table in ('line2', 'line3', 'grid'))
    what = 'coupled kind=%d %s T=%d E=%d %s' % (kind, table, T, E, form)
    d = _coupled_inputs(kind, tab, T, E, form, kind * 7919 + T * 101 + E + len(table) + (3 if form == 'dy8' else 0))
    f = lambda x: x.double()                                                            # noqa: E731
    hm = d['S'][..., 2 * H:]
    dz_r, d1_r = torch.zeros(N, T, E, 4 * H, dtype=F64), torch.zeros(N, T, E, H, dtype=F64)
    db_r, dbm_r = ops_ref.bptt_coupled(kind, dict(nbr_idx=tab), m_max, f(d['gates']), f(d['call']), f(d['done']),
                                       f(d['dhs']) if form == 'tensor' else None, (f(d['wxm']), f(d['wh']), None), (f(d['w_msg']), None),
                                       f(hm) if kind == 1 else None, dz_r, d1_r, head_dy=(f(d['dy8']), f(d['hw'])) if form == 'dy8' else None)
    t = lambda x: x.to(dev)                                                             # noqa: E731
    rev = impl.reverse_neighbor_table(t(tab), kind)
    cuda = torch.device(dev).type == 'cuda'
    if cuda:
        assert rev is not None and bool(rev['symmetric']) == sym and rev['r_max'] == r_max
        assert N * -(-E // 128) <= torch.cuda.get_device_properties(0).multi_processor_count      # mode 1 is forced below
    wxd, whd, wmd = t(d['wxm']), t(d['wh']), t(d['w_msg'])
    ws, wm = (wxd, whd, impl.lstm_bptt_wimage(wxd, whd)), (wmd, impl.lstm_bptt_msg_wimage(wmd))
    Gd, Sd, doned = _in_seq(d['gates'], dev), t(d['S']), t(d['done'])
    Cd = torch.zeros(N, T + 3, E, H, device=dev)
    Cd[:, 1:T + 2].copy_(d['call'])
    Dd = _in_seq(d['dhs'], dev) if form == 'tensor' else None
    hd = (t(d['dy8']), t(d['hw'])) if form == 'dy8' else None
    assert (Dd is None) != (hd is None)
    out, worst = {}, 0.0
    modes = (1, 2) if sym else (0, 2)
    for mode in modes:
        o = dict(dZ=Out(dev, N, E, 4 * H, T=T), D1=Out(dev, N, E, H, T=T))
        db, dbm = impl.bptt_coupled(kind, rev, m_max, Gd, Cd[:, 1:T + 2], doned, Dd, ws, wm, Sd[..., 2 * H:] if kind == 1 else None,
                                    o['dZ'].v, o['D1'].v, mode=mode, head_dy=hd)
        db, dbm = db.clone(), dbm.clone()
        _sync(impl, dev)
        w = '%s mode=%d' % (what, mode)
        _assert_outs(o, w)
        worst = max(worst, _used_tag('close', w + ' dZ', o['dZ'].v, dz_r, **COUPLED_TOL), _used_tag('close', w + ' D1', o['D1'].v, d1_r, **COUPLED_TOL),
                    _used_tag('db', w + ' db', db, db_r, rtol=1e-4, atol=1e-4 * max(1.0, float(db_r.abs().max()))),
                    _used_tag('db', w + ' dbmsg', dbm, dbm_r, rtol=1e-4, atol=1e-4 * max(1.0, float(dbm_r.abs().max()))))
        if kind == 1:
            assert bool((o['D1'].cpu()[~(hm > 0)] == 0).all()), '[mask] %s: D1 is not exactly 0 where the mask is <= 0' % w
        out[mode] = (o, db, dbm)
    (a, dba, dbma), (b, dbb, dbmb) = out[modes[0]], out[modes[1]]
    for k in ('dZ', 'D1'):
        assert _same_bits(a[k].v, b[k].v), '[bits] %s: %s differs between modes %d and %d' % (what, k, modes[0], modes[1])
    worst = max(worst, _used_tag('db', what + ' db between the modes', dba, dbb, rtol=1e-5, atol=1e-5 * (T * E) ** 0.5),
                _used_tag('db', what + ' dbmsg between the modes', dbma, dbmb, rtol=1e-5, atol=1e-5 * (T * E) ** 0.5))
    print('%s <%d,%d>: %.3g of a bound at worst' % ((what,) + INSTANTIATION[kind, table] + (worst,)))
    return worst


# --------------------------------------------------------------------------------------------------------- 4. bptt_dial
DIAL_T, DIAL_E = (1, 2), (17, 129)


def _dial_inputs(tab, T, E, form, seed, O=5):
    N = tab.shape[0]
    d = _coupled_inputs(1, tab, T, E, form, seed, O)
    r, _ = _rand(seed + 1)
    d['mfc_w'] = r(N, H, H) * 0.2
    d['hm'], d['msg'] = torch.relu(r(N, T, E, H)), torch.relu(r(N, T, E, H))
    d['hm'][:, :, ::2, 1::5] = -0.0
    d['msg'][:, :, 1::2, 2::7] = -0.0
    return d


def run_dial(impl, dev, tab, d, mode, form):
    """impl.bptt_dial on slots of wider allocations, the outputs rows of padded sentinel buffers.  -> dict of Outs and tensors."""
    N, m_max = tab.shape
    _, T, E, _ = d['gates'].shape
    t = lambda x: x.to(dev)                                                             # noqa: E731
    Gd = _in_seq(d['gates'], dev)
    Cd = torch.zeros(N, T + 3, E, H, device=dev)
    Cd[:, 1:T + 2].copy_(d['call'])
    HM = torch.zeros(N, T, E, 3 * H, device=dev)
    HM[..., H:2 * H].copy_(d['hm'])
    MSG = torch.zeros(N, T + 1, E, H, device=dev)
    MSG[:, :T].copy_(d['msg'])
    wx, wh, w_msg, mfc_w = t(d['wxm']), t(d['wh']), t(d['w_msg']), t(d['mfc_w'])
    rev = impl.reverse_neighbor_table(t(tab), 1)
    o = dict(dZ=Out(dev, N, E, 4 * H, T=T), DS=Out(dev, N, E, H, T=T), D1=Out(dev, N, E, H, T=T), D2=Out(dev, N, E, H, T=T))
    Dd = _in_seq(d['dhs'], dev) if form == 'tensor' else None
    hd = (t(d['dy8']), t(d['hw'])) if form == 'dy8' else None
    assert (Dd is None) != (hd is None) and HM[..., H:2 * H].stride(2) == 3 * H
    db, dbm, dbf, dh0, dc0 = impl.bptt_dial(rev, m_max, Gd, Cd[:, 1:T + 2], t(d['done']), Dd, (wx, wh, impl.lstm_bptt_wimage(wx, wh)),
                                            (w_msg, impl.lstm_bptt_msg_wimage(w_msg)), impl.lstm_bptt_msg_wimage(mfc_w), HM[..., H:2 * H], MSG,
                                            o['dZ'].v, o['DS'].v, o['D1'].v, o['D2'].v, mode=mode, head_dy=hd, want_state_grad=True)
    res = dict(o, db=db.clone(), dbm=dbm.clone(), dbf=dbf.clone(), dh0=dh0.clone(), dc0=dc0.clone())
    _sync(impl, dev)
    return res


def dial64(tab, d, form):
    f = lambda x: x.double()                                                            # noqa: E731
    N, T, E, _ = d['gates'].shape
    ref = dict(dZ=torch.zeros(N, T, E, 4 * H, dtype=F64), DS=torch.zeros(N, T, E, H, dtype=F64), D1=torch.zeros(N, T, E, H, dtype=F64),
               D2=torch.zeros(N, T, E, H, dtype=F64))
    ref['db'], ref['dbm'], ref['dbf'], ref['dh0'], ref['dc0'] = ops_ref.bptt_dial(
        dict(nbr_idx=tab), tab.shape[1], f(d['gates']), f(d['call']), f(d['done']), f(d['dhs']) if form == 'tensor' else None,
        (f(d['wxm']), f(d['wh']), None), (f(d['w_msg']), None), f(d['mfc_w']), f(d['hm']), f(d['msg']), ref['dZ'], ref['DS'], ref['D1'], ref['D2'],
        head_dy=(f(d['dy8']), f(d['hw'])) if form == 'dy8' else None, want_state_grad=True)
    return ref


def check_dial_edges(impl, dev, table, T, E, form):
    """nmarl_lstm_bptt_dial against ops_ref.bptt_dial on float64 operands (tolerances of check_coupled_edges); D1 / D2 exactly 0 where
    their relu masks are <= 0; modes (1, 2) on the symmetric line, (0, 2) on the ragged table, bit for bit in dZ, DS, D1, D2, dh0,
    dc0."""
    assert table in DIAL_TABLES and T in DIAL_T and E in DIAL_E and form in COUPLED_FORMS
    tab = TABLES[table]()
    N, m_max = tab.shape
    r_max, sym = table_facts(tab)
    assert (4 * m_max, 2) == INSTANTIATION[3, table] and r_max <= 2 and sym == (table == 'line3') and N <= 9
    what = 'dial %s T=%d E=%d %s' % (table, T, E, form)
    d = _dial_inputs(tab, T, E, form, T * 977 + E * 3 + len(table) + (5 if form == 'dy8' else 0))
    ref = dial64(tab, d, form)
    if torch.device(dev).type == 'cuda':
        assert N * -(-E // 128) <= torch.cuda.get_device_properties(0).multi_processor_count
    modes = (1, 2) if sym else (0, 2)
    out, worst = {}, 0.0
    for mode in modes:
        o = out[mode] = run_dial(impl, dev, tab, d, mode, form)
        w = '%s mode=%d' % (what, mode)
        _assert_outs({k: o[k] for k in ('dZ', 'DS', 'D1', 'D2')}, w)
        for k in ('dZ', 'DS', 'D1', 'D2', 'dh0', 'dc0'):
            got = o[k].v if isinstance(o[k], Out) else o[k]
            worst = max(worst, _used_tag('close', '%s %s' % (w, k), got, ref[k], **COUPLED_TOL))
        for k in ('db', 'dbm', 'dbf'):
            worst = max(worst, _used_tag('db', '%s %s' % (w, k), o[k], ref[k], rtol=1e-4, atol=1e-4 * max(1.0, float(ref[k].abs().max()))))
        assert bool((o['D1'].cpu()[~(d['hm'] > 0)] == 0).all()), '[mask] %s: D1 is not exactly 0 where hm <= 0' % w
        assert bool((o['D2'].cpu()[~(d['msg'] > 0)] == 0).all()), '[mask] %s: D2 is not exactly 0 where msg <= 0' % w
    a, b = out[modes[0]], out[modes[1]]
    for k in ('dZ', 'DS', 'D1', 'D2', 'dh0', 'dc0'):
        x, y = (a[k].v, b[k].v) if isinstance(a[k], Out) else (a[k], b[k])
        assert _same_bits(x, y), '[bits] %s: %s differs between modes %d and %d' % (what, k, modes[0], modes[1])
    print('%s: %.3g of a bound at worst' % (what, worst))
    return worst


# ------------------------------------------------------------------------------------------- 5. the launchers' own choices
def check_launcher_fallbacks(impl, dev, monkeypatch):
    """(a) COUPLED_RING_MAX_BYTES one byte below T N E K 4: the workspace's ring gets 2 slots, mode 1 is demoted to step-wise launches
    (lstm_bptt.hip:1518, :1633: ring_slots < T) and equals mode 2 bit for bit -- coupled (kind 1, line of 3) and dial.  (b)
    NMARL_TEST_FAKE_CUS=1: mode 0 on a symmetric table finds grid > cap and goes step-wise; without the variable it takes the one
    launch: both equal mode 2, and mode 1, bit for bit.  Both settings are restored through `monkeypatch`."""
    T, E = 3, 17
    tab = line_table(3)
    N, m_max = tab.shape
    K = H * m_max
    cuda = torch.device(dev).type == 'cuda'
    t = lambda x: x.to(dev)                                                             # noqa: E731
    dC = _coupled_inputs(1, tab, T, E, 'tensor', 4242)
    dD = _dial_inputs(tab, T, E, 'tensor', 4243)
    rev = impl.reverse_neighbor_table(t(tab), 1)
    wxd, whd, wmd = t(dC['wxm']), t(dC['wh']), t(dC['w_msg'])
    ws, wm = (wxd, whd, impl.lstm_bptt_wimage(wxd, whd)), (wmd, impl.lstm_bptt_msg_wimage(wmd))
    Gd, Sd, Dd = _in_seq(dC['gates'], dev), t(dC['S']), _in_seq(dC['dhs'], dev)
    Cd = torch.zeros(N, T + 3, E, H, device=dev)
    Cd[:, 1:T + 2].copy_(dC['call'])

    def coupled(mode):
        o = dict(dZ=Out(dev, N, E, 4 * H, T=T), D1=Out(dev, N, E, H, T=T))
        impl.bptt_coupled(1, rev, m_max, Gd, Cd[:, 1:T + 2], t(dC['done']), Dd, ws, wm, Sd[..., 2 * H:], o['dZ'].v, o['D1'].v, mode=mode)
        _sync(impl, dev)
        _assert_outs(o, 'fallbacks coupled mode=%d' % mode)
        return [o['dZ'].v, o['D1'].v]

    def dial(mode):
        o = run_dial(impl, dev, tab, dD, mode, 'tensor')
        return [o[k].v for k in ('dZ', 'DS', 'D1', 'D2')] + [o['dh0'], o['dc0']]

    def same(a, b, what):
        for i, (x, y) in enumerate(zip(a, b)):
            assert _same_bits(x, y), '[bits] fallbacks: %s (output %d)' % (what, i)

    pool = getattr(impl, '_coupled_ws', {})
    orig = getattr(impl, 'COUPLED_RING_MAX_BYTES', 4 << 30)
    ref = {}
    for name, fn in (('coupled', coupled), ('dial', dial)):
        pool.clear()
        ref[name] = fn(2)
        if cuda:
            assert len(pool) == 1 and all(w['ring'].shape[0] == T for w in pool.values())
    # (a) a ring of two slots
    monkeypatch.setattr(impl, 'COUPLED_RING_MAX_BYTES', T * N * E * K * 4 - 1, raising=False)
    for name, fn in (('coupled', coupled), ('dial', dial)):
        pool.clear()
        got = fn(1)
        if cuda:
            assert len(pool) == 1 and all(w['ring'].shape[0] == 2 for w in pool.values()), 'the ring was not capped at two slots'
        same(got, ref[name], '%s: mode 1 on a ring of 2 slots < T differs from mode 2' % name)
    monkeypatch.setattr(impl, 'COUPLED_RING_MAX_BYTES', orig, raising=False)
    pool.clear()
    # (b) mode 0 choosing by itself
    for name, fn, cap_kind in (('coupled', coupled, 2), ('dial', dial, 3)):
        one = fn(1)
        same(one, ref[name], '%s: mode 1 differs from mode 2' % name)
        same(fn(0), one, '%s: mode 0 (grid <= cap: one launch) differs from mode 1' % name)
        monkeypatch.setenv('NMARL_TEST_FAKE_CUS', '1')
        if cuda:
            from deeprl_network_amd import _lib
            assert _lib.lib.nmarl_handoff_capacity(cap_kind, K) == 1 and N * -(-E // 128) > 1
        same(fn(0), ref[name], '%s: mode 0 with one CU (grid > cap: step-wise) differs from mode 2' % name)
        monkeypatch.delenv('NMARL_TEST_FAKE_CUS')
    print('launcher fallbacks: every choice agrees bit for bit')
    return 0.0


# ------------------------------------------------------------------------------------------------------- 6. saturation
SAT_ENTRIES = ('step', 'seq', 'coupled')
SAT_C = (20.0, -20.0, 1e4, -1e4)


def _saturated(N, T, E, seed):
    """Gates with exact 0.0 / 1.0 / +-1.0 planted by unit, a cell trace that holds +-20 and +-1e4 (units 0 .. 7: c0 planted, gf = 1,
    gi = 0 exactly, so the forward trace keeps the value while the row is live), c0 = 1e30 in the rows finished at t = 0."""
    r, _ = _rand(seed)
    g = _gates(r, N, T, E)
    c0 = r(N, E, H) * 0.8
    for k, v in enumerate(SAT_C * 2):
        c0[:, :, k] = v
        g[..., H + k] = 1.0                               # gf
        g[..., k] = 0.0                                   # gi
    for k, (gate, v) in enumerate(((0, 0.0), (0, 1.0), (1, 0.0), (1, 1.0), (2, 0.0), (2, 1.0), (3, 1.0), (3, -1.0))):
        g[..., gate * H + 8 + 2 * k:gate * H + 10 + 2 * k] = v      # units 8 .. 23, two each
    g[..., 2 * H:2 * H + 4] = 1.0                          # go = 1 on four of the planted cells: dL/dh reaches tanh'(c) = 0 there
    done = torch.zeros(T, E)
    done[0, 1::4] = 1.0
    if T > 1:
        done[T - 1, 2::5] = 1.0
    fin0 = done[0].bool()
    c0[:, fin0] = GARBAGE
    call = forward_cells(g, c0, done)
    assert bool(torch.isfinite(call[:, 1:]).all()) and float(call[:, 0][:, fin0].min()) > 0.99 * GARBAGE
    live = ~done.bool().any(dim=0) if E > 1 else ~fin0
    if bool(live.any()):
        assert sorted(set(call[0, T][live][0, :4].tolist())) == sorted(SAT_C), 'the planted cells did not survive the trace'
    return g, c0, call, done


def _assert_saturated(dz, dcp_t0, g, done, what):
    """dz [N,T,E,4H] (CPU): finite; exactly 0 where the gate's own derivative factor is exactly 0; the finished rows: forget-gate dz
    exactly 0 (every step), dc_prev of step 0 exactly 0."""
    assert bool(torch.isfinite(dz).all()), '[finite] %s: dz is not finite' % what
    gi, gf, go, gu = g.split(H, dim=-1)
    zero = torch.cat([(gi * (1 - gi) == 0) | (gu == 0), gf * (1 - gf) == 0, go * (1 - go) == 0, (1 - gu * gu == 0) | (gi == 0)], dim=-1)
    assert int(zero.sum()) >= 20 * dz.shape[0] * dz.shape[1] * dz.shape[2]
    assert bool((dz[zero] == 0).all()), '[exact] %s: dz is not exactly 0 where its derivative factor is exactly 0' % what
    fin = done.bool()                                      # [T,E]
    assert bool((dz[:, :, :, H:2 * H][:, fin] == 0).all()), '[exact] %s: the forget gate\'s dz is not exactly 0 in a finished row' % what
    if dcp_t0 is not None:
        assert bool(torch.isfinite(dcp_t0).all()), '[finite] %s: dc_prev is not finite' % what
        assert bool((dcp_t0[:, fin[0]] == 0).all()), '[exact] %s: dc_prev is not exactly 0 in a finished row' % what


def check_saturation(impl, dev, entry, N=N_AGENTS):
    """Saturated gates (exact 0.0, 1.0, +-1.0), c_new in {+-20, +-1e4} (the fast tanh runs through exp2 -> inf / 0) and c_prev = 1e30
    in finished rows: every output finite, dz exactly 0 where its own derivative factor is, dc_prev and the forget gate's dz exactly
    0 in the finished rows, everything else at the entry point's ordinary tolerance against float64.  step: T = 1, E = 129; seq:
    T = 3, E = 129; coupled: kind 1 on the line of 3, T = 3, E = 17, modes 1 and 2.  The one-launch kernels get a consistent forward
    trace (forward_cells of the planted gates and c0)."""
    assert entry in SAT_ENTRIES
    T, E = (1, 129) if entry == 'step' else (3, 129) if entry == 'seq' else (3, 17)
    g, _, call, done = _saturated(N, T, E, 99 + SAT_ENTRIES.index(entry))
    r, _ = _rand(5 + T)
    dhs = r(N, T, E, H)
    wh, wxm = _weights(r, N)
    t = lambda x: x.to(dev)                                                             # noqa: E731
    what = 'saturation ' + entry
    Gd = _in_seq(g, dev)
    Cd = torch.zeros(N, T + 3, E, H, device=dev)
    Cd[:, 1:T + 2].copy_(call)
    whd, wxd = t(wh), t(wxm)
    worst = 0.0
    if entry == 'step':
        dh2, dc = r(N, E, H), r(N, E, H)
        dz64, dcp64, _ = cell_bwd64(g[:, 0], call[:, 0], call[:, 1], done[0], dhs[:, 0], dh2, dc)
        keep = (1.0 - done[0].double()).view(1, -1, 1)
        dhd64, dx64 = torch.bmm(dz64, wh.double().transpose(1, 2)) * keep, torch.bmm(dz64, wxm.double().transpose(1, 2))
        o = dict(dz=Out(dev, N, E, 4 * H), dcp=Out(dev, N, E, H), dhd=Out(dev, N, E, H), dx=Out(dev, N, E, H))
        impl.bptt_step(Gd[:, 0], Cd[:, 1], Cd[:, 2], t(done[0]), _in_slot(dhs[:, 0], dev), _in_slot(dh2, dev), _in_slot(dc, dev),
                       (wxd, whd, impl.lstm_bptt_wimage(wxd, whd)), o['dz'].v, o['dcp'].v, o['dhd'].v, True, dx=o['dx'].v)
        _assert_outs(o, what)
        _assert_saturated(o['dz'].cpu().unsqueeze(1), o['dcp'].cpu(), g, done, what)
        worst = max(_used_tag('close', what + ' dz', o['dz'].v, dz64, **STEP_TOL), _used_tag('close', what + ' dc_prev', o['dcp'].v, dcp64, **STEP_TOL),
                    _used_tag('close', what + ' dhd', o['dhd'].v, dhd64, **PROD_TOL), _used_tag('close', what + ' dx', o['dx'].v, dx64, **PROD_TOL))
    elif entry == 'seq':
        dz64, dh064, dc064 = seq64(g, call, done, dhs, wh)
        dz = Out(dev, N, E, 4 * H, T=T)
        db, dh0, dc0 = impl.bptt_seq(Gd, Cd[:, 1:T + 2], t(done), _in_seq(dhs, dev), impl.lstm_bptt_wimage(None, whd), dz.v, want_db=True,
                                     want_state_grad=True)
        _assert_outs(dict(dz=dz), what)
        _assert_saturated(dz.cpu(), dc0.cpu(), g, done, what)
        assert bool(torch.isfinite(db).all()) and bool(torch.isfinite(dh0).all()), '[finite] %s: db / dh0' % what
        worst = max(_used_tag('close', what + ' dz', dz.v, dz64, **PROD_TOL), _used_tag('close', what + ' dh0', dh0, dh064, **PROD_TOL),
                    _used_tag('close', what + ' dc0', dc0, dc064, **PROD_TOL))
    else:
        tab = line_table(3)
        assert N == 3
        r2, _ = _rand(77)
        w_msg = r2(N, 2 * H, H) * 0.15
        S = torch.relu(r2(N, T, E, 3 * H))
        f = lambda x: x.double()                                                        # noqa: E731
        dz_r, d1_r = torch.zeros(N, T, E, 4 * H, dtype=F64), torch.zeros(N, T, E, H, dtype=F64)
        ops_ref.bptt_coupled(1, dict(nbr_idx=tab), 2, f(g), f(call), f(done), f(dhs), (f(wxm), f(wh), None), (f(w_msg), None), f(S[..., 2 * H:]),
                             dz_r, d1_r)
        rev = impl.reverse_neighbor_table(t(tab), 1)
        wmd, Sd, Dd = t(w_msg), t(S), _in_seq(dhs, dev)
        outs = []
        for mode in (1, 2):
            o = dict(dZ=Out(dev, N, E, 4 * H, T=T), D1=Out(dev, N, E, H, T=T))
            db, dbm = impl.bptt_coupled(1, rev, 2, Gd, Cd[:, 1:T + 2], t(done), Dd, (wxd, whd, impl.lstm_bptt_wimage(wxd, whd)),
                                        (wmd, impl.lstm_bptt_msg_wimage(wmd)), Sd[..., 2 * H:], o['dZ'].v, o['D1'].v, mode=mode)
            assert bool(torch.isfinite(db).all()) and bool(torch.isfinite(dbm).all()), '[finite] %s: bias sums' % what
            _sync(impl, dev)
            _assert_outs(o, what)
            _assert_saturated(o['dZ'].cpu(), None, g, done, what)
            worst = max(worst, _used_tag('close', what + ' dZ', o['dZ'].v, dz_r, **COUPLED_TOL), _used_tag('close', what + ' D1', o['D1'].v, d1_r, **COUPLED_TOL))
            outs.append(o)
        for k in ('dZ', 'D1'):
            assert _same_bits(outs[0][k].v, outs[1][k].v), '[bits] %s: %s differs between modes 1 and 2' % (what, k)
    print('%s: %.3g of a bound at worst' % (what, worst))
    return worst


# ----------------------------------------------------------------------------------------- 7. the fast tanh's mid-range
TANH_EPS = 2.0 ** -21


def check_tanh_midrange(impl, dev, N=N_AGENTS):
    """c_new swept over [-9, 9] in steps of 1/16 across rows and units (E = 289 rows, each unit shifted), |dh| <= 4, through bptt_step
    (KM = 64).  For |c| in [3, 9] the factor 1 - tanh(c)^2 is 1e-2 .. 6e-8: what is left of the kernels' fast tanh
    tanh_fast_(x) = 2 rcp(1 + exp2(-2 log2(e) x)) - 1 there is its ABSOLUTE error eps.

    eps: no accuracy statement for the fp32 exp2 and rcp instructions is at hand, so each is taken as 1 ulp (2^-23 relative).  With
    s = 1 / (1 + e), e = exp2(a): the rcp contributes s 2^-23 <= 2^-23, the rounding of 1 + e: s 2^-24, exp2's ulp: s (1 - s) 2^-23
    <= 2^-25, the two roundings of the argument a: |a| s (1 - s) ln 2 2^-23 <= 0.16 2^-23; tanh = 2 s - 1 doubles the sum and adds
    its own rounding only below 1/2 (Sterbenz above): eps <= 2 (1 + 1/2 + 1/4 + 0.16) 2^-23 < 2^-21.  TANH_EPS = 2^-21.

    The bound, elementwise: |d(1 - tc^2)| <= 2 |tc| eps + eps^2 =: D; g_c = dc + gh go (1 - tc^2) moves by |gh go| D; the i, f, u
    parts of dz and dc_prev by their factor times that, the o part gh tc go (1 - go) by |gh go (1 - go)| eps -- plus the ordinary
    STEP_TOL.  dhd / dx are not held to it (a sum of 256 such terms: PROD_TOL covers them).  -> the worst share of the bound used."""
    E = 289
    r, _ = _rand(2024)
    gates, c_prev = _gates(r, N, E), r(N, E, H)
    c_new = -9.0 + ((torch.arange(E).view(1, E, 1) + 5 * torch.arange(H).view(1, 1, H) + 97 * torch.arange(N).view(N, 1, 1)) % 289).float() / 16.0
    assert float(c_new.min()) == -9.0 and float(c_new.max()) == 9.0 and len(torch.unique(c_new[0, :, 0])) == 289 and E <= 300
    dh, dc = (r(N, E, H) * 2).clamp(-4, 4), r(N, E, H)
    done = torch.zeros(E)
    done[3::7] = 1.0
    wh, wxm = _weights(r, N)
    dz64, dcp64, p = cell_bwd64(gates, c_prev, c_new, done, dh, None, dc)
    D = 2 * p['tc'].abs() * TANH_EPS + TANH_EPS ** 2
    egc = (p['gh'] * p['go']).abs() * D
    edz = torch.cat([(p['gu'] * p['gi'] * (1 - p['gi'])).abs() * egc, (p['cpk'] * p['gf'] * (1 - p['gf'])).abs() * egc,
                     (p['gh'] * p['go'] * (1 - p['go'])).abs() * TANH_EPS, (p['gi'] * (1 - p['gu'] * p['gu'])).abs() * egc], dim=-1)
    edcp = (p['gf'] * p['keep']).abs() * egc
    t = lambda x: x.to(dev)                                                             # noqa: E731
    wxd, whd = t(wxm), t(wh)
    o = dict(dz=Out(dev, N, E, 4 * H), dcp=Out(dev, N, E, H), dhd=Out(dev, N, E, H), dx=Out(dev, N, E, H))
    impl.bptt_step(_in_slot(gates, dev), _in_slot(c_prev, dev), _in_slot(c_new, dev), t(done), _in_slot(dh, dev), None, _in_slot(dc, dev),
                   (wxd, whd, impl.lstm_bptt_wimage(wxd, whd)), o['dz'].v, o['dcp'].v, o['dhd'].v, True, dx=o['dx'].v)
    _assert_outs(o, 'tanh mid-range')
    worst = 0.0
    for name, got, exp, err in (('dz', o['dz'].cpu().double(), dz64, edz), ('dc_prev', o['dcp'].cpu().double(), dcp64, edcp)):
        bound = err + STEP_TOL['atol'] + STEP_TOL['rtol'] * exp.abs()
        share = (got - exp).abs() / bound
        print('tanh mid-range %s: %.3g of its bound (the tanh part alone is %.3g of the bound there)' % (
            name, float(share.max()), float((err / bound).view(-1)[share.argmax()])))
        assert bool(torch.isfinite(got).all()) and float(share.max()) <= 1.0, '[tanh] %s: %.3g of the propagated bound (eps = 2^-21)' % (name, float(share.max()))
        worst = max(worst, float(share.max()))
    mid = (c_new.abs() >= 3).double()
    resid = ((o['dz'].cpu().double() - dz64).abs()[..., :H] * mid).max()
    print('tanh mid-range: largest |dz_i - float64| at |c| >= 3: %.3g' % float(resid))
    dhd64 = torch.bmm(dz64, wh.double().transpose(1, 2)) * p['keep']
    _used_tag('close', 'tanh mid-range dhd', o['dhd'].v, dhd64, **PROD_TOL)
    _used_tag('close', 'tanh mid-range dx', o['dx'].v, torch.bmm(dz64, wxm.double().transpose(1, 2)), **PROD_TOL)
    print('tanh mid-range: %.3g of the propagated bound at worst' % worst)
    return worst


# --------------------------------------------------------------------------------------------------------- 8. refusals
def check_refusals(dev):
    """Straight through the C ABI: every call below returns NMARL_EINVAL and writes nothing (the outputs are sentinel-filled; every
    buffer is large enough for the call had it not been refused).  step: Hh = 32, KM = 32, a row stride one float too small, dz 4
    bytes off, db_sn one too small, mask_row < 64.  seq: dh_ext and dy8 both / neither, O = 0 / 9, T = 0, dy_st no multiple of 4.
    coupled: ring_slots = 1, r_row != the padded fan-in, kind = 3, m_max = 3, ws off a word; dial: the same without kind.  The
    coupled / dial argument structs are the ones ops.bptt_coupled / ops.bptt_dial build (caught in front of the library call).
    -> the number of refused calls."""
    import ctypes as C
    from deeprl_network_amd import _lib, ops
    lib = _lib.lib
    EINVAL, OK = -1, 0
    N, T, E = 2, 3, 32
    G4 = 4 * H
    r, _ = _rand(31)
    z = lambda *s: torch.zeros(*s, device=dev)                                          # noqa: E731
    sent = lambda n: torch.full((n + 16,), SENTINEL, device=dev)                         # noqa: E731
    p = lambda x: x.data_ptr()                                                           # noqa: E731
    count = 0
    # ---- step
    gates, cp, cn, done = _gates(r, N, E).to(dev), r(N, E, H).to(dev), r(N, E, H).to(dev), z(E)
    dh = r(N, E, H).to(dev)
    img = ops.lstm_bptt_wimage(r(N, H, G4).to(dev), r(N, H, G4).to(dev))
    mask = torch.ones(N, E, H, device=dev)
    parts = lib.nmarl_lstm_bptt_step_parts(E)
    outs = {k: sent(N * E * w) for k, w in (('dz', G4), ('dcp', H), ('dx', H), ('dhd', H), ('db', parts * G4))}
    keys = ['E', 'N', 'Hh', 'KM', 'gates', 'gates_sn', 'c_prev', 'c_prev_sn', 'c_new', 'c_new_sn', 'done', 'dh', 'dh_sn', 'dh2', 'dh2_sn', 'dc', 'dc_sn',
            'img', 'img_sn', 'dz', 'dz_sn', 'dc_prev', 'dc_prev_sn', 'dx', 'dx_sn', 'mask', 'mask_sn', 'mask_row', 'dhd', 'dhd_sn', 'apply_keep',
            'db_part', 'db_sn']
    base = dict(E=E, N=N, Hh=H, KM=64, gates=p(gates), gates_sn=E * G4, c_prev=p(cp), c_prev_sn=E * H, c_new=p(cn), c_new_sn=E * H, done=p(done),
                dh=p(dh), dh_sn=E * H, dh2=None, dh2_sn=0, dc=None, dc_sn=0, img=p(img), img_sn=img.stride(0), dz=p(outs['dz']), dz_sn=E * G4,
                dc_prev=p(outs['dcp']), dc_prev_sn=E * H, dx=p(outs['dx']), dx_sn=E * H, mask=p(mask), mask_sn=E * H, mask_row=H,
                dhd=p(outs['dhd']), dhd_sn=E * H, apply_keep=1, db_part=p(outs['db']), db_sn=parts * G4)
    assert len(keys) + 1 == len(_lib.SIGNATURES['nmarl_lstm_bptt_step']) and set(keys) == set(base)
    step_cases = {'Hh = 32': dict(Hh=32), 'KM = 32': dict(KM=32), 'gates_sn one float short': dict(gates_sn=E * G4 - 1),
                  'dz 4 bytes off': dict(dz=p(outs['dz']) + 4), 'db_sn one short': dict(db_sn=parts * G4 - 1), 'mask_row < 64': dict(mask_row=63)}
    for what, kw in step_cases.items():
        a = dict(base, **kw)
        assert lib.nmarl_lstm_bptt_step(*[a[k] for k in keys], _lib.stream()) == EINVAL, 'step: %s was not refused' % what
        count += 1
    # ---- seq
    Gs, Cs, dones, Ds = _gates(r, N, T, E).to(dev), r(N, T + 1, E, H).to(dev), z(T, E), r(N, T, E, H).to(dev)
    dy8, hw = z(N, T * E * 8 + 64), z(N, H, 16)
    img_s = ops.lstm_bptt_wimage(None, r(N, H, G4).to(dev))
    nblk = lib.nmarl_lstm_bptt_seq_blocks(E)
    outs.update({k: sent(N * n) for k, n in (('sdz', T * E * G4), ('sdb', nblk * G4), ('dh0', E * H), ('dc0', E * H))})
    skeys = ['T', 'E', 'N', 'Hh', 'gates', 'gates_sn', 'gates_st', 'c_all', 'c_sn', 'c_st', 'done', 'dh_ext', 'dh_sn', 'dh_st', 'dy8', 'dy_sn', 'dy_st',
             'hw', 'hw_sn', 'O', 'img', 'img_sn', 'dz', 'dz_sn', 'dz_st', 'db_part', 'db_sn', 'dh0', 'dh0_sn', 'dc0', 'dc0_sn']
    sbase = dict(T=T, E=E, N=N, Hh=H, gates=p(Gs), gates_sn=T * E * G4, gates_st=E * G4, c_all=p(Cs), c_sn=(T + 1) * E * H, c_st=E * H, done=p(dones),
                 dh_ext=p(Ds), dh_sn=T * E * H, dh_st=E * H, dy8=None, dy_sn=0, dy_st=0, hw=None, hw_sn=0, O=0, img=p(img_s), img_sn=img_s.stride(0),
                 dz=p(outs['sdz']), dz_sn=T * E * G4, dz_st=E * G4, db_part=p(outs['sdb']), db_sn=nblk * G4, dh0=p(outs['dh0']), dh0_sn=E * H,
                 dc0=p(outs['dc0']), dc0_sn=E * H)
    assert len(skeys) + 1 == len(_lib.SIGNATURES['nmarl_lstm_bptt_seq']) and set(skeys) == set(sbase)
    dy = dict(dh_ext=None, dh_sn=0, dh_st=0, dy8=p(dy8), dy_sn=dy8.stride(0), dy_st=E * 8, hw=p(hw), hw_sn=hw.stride(0), O=5)
    seq_cases = {'dh_ext and dy8 both': dict(dy, dh_ext=p(Ds), dh_sn=T * E * H, dh_st=E * H), 'neither dh_ext nor dy8': dict(dh_ext=None),
                 'O = 0': dict(dy, O=0), 'O = 9': dict(dy, O=9), 'T = 0': dict(T=0), 'dy_st no multiple of 4': dict(dy, dy_st=E * 8 + 2)}
    for what, kw in seq_cases.items():
        a = dict(sbase, **kw)
        assert lib.nmarl_lstm_bptt_seq(*[a[k] for k in skeys], _lib.stream()) == EINVAL, 'seq: %s was not refused' % what
        count += 1
    # ---- coupled and dial: the structs the wrappers build
    tab = line_table(3)
    Nc, m_max = tab.shape
    d = _dial_inputs(tab, T, E, 'tensor', 17)
    t = lambda x: x.to(dev)                                                             # noqa: E731
    rev = ops.reverse_neighbor_table(t(tab), 1)
    wxd, whd, wmd, mfd = t(d['wxm']), t(d['wh']), t(d['w_msg']), t(d['mfc_w'])
    ws, wm = (wxd, whd, ops.lstm_bptt_wimage(wxd, whd)), (wmd, ops.lstm_bptt_msg_wimage(wmd))
    co = {k: torch.full((Nc, T, E, w), SENTINEL, device=dev) for k, w in (('dZ', G4), ('D1', H), ('DS', H), ('D2', H))}
    Sd, hmd, msgd = t(d['S']), t(d['hm']), t(d['msg'])
    caught = {}

    def capture(name, call):
        real = getattr(lib, name)
        setattr(lib, name, lambda a, st: caught.__setitem__(name, a._obj) or OK)
        try:
            call()
        finally:
            setattr(lib, name, real)
        assert getattr(lib, name) is real
        return caught[name]

    Gc, Cc, donec, Dc, img_f = t(d['gates']), t(d['call']), t(d['done']), t(d['dhs']), ops.lstm_bptt_msg_wimage(mfd)      # (kept alive)
    ac = capture('nmarl_lstm_bptt_coupled', lambda: ops.bptt_coupled(1, rev, m_max, Gc, Cc, donec, Dc, ws, wm, Sd[..., 2 * H:], co['dZ'], co['D1'],
                                                                      mode=2))
    ad = capture('nmarl_lstm_bptt_dial', lambda: ops.bptt_dial(rev, m_max, Gc, Cc, donec, Dc, ws, wm, img_f, hmd, msgd, co['dZ'], co['DS'], co['D1'],
                                                                co['D2'], mode=2))
    # operands for the cases whose refused geometry is larger than the wrappers': message rows of 192 floats, tables padded to 4
    ring3, img3 = z(max(T, 2), Nc, E, 3 * H), z(Nc, 3 * H * H)
    rev4 = [torch.zeros(Nc, 4, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.float32)]
    ws_big = torch.zeros(int(lib.nmarl_lstm_bptt_coupled_ws_words(E, Nc)) + 64, dtype=torch.int32, device=dev)
    wide = dict(m_max=3, ring=p(ring3), ring_sn=ring3.stride(1), ring_slot=ring3.stride(0), ring_slots=ring3.shape[0], img_m=p(img3), imgm_sn=img3.stride(0))
    r4 = dict(r_row=4, rev_agent=p(rev4[0]), rev_col=p(rev4[1]), rev_w=p(rev4[2]))
    cases = {'ring_slots = 1': dict(ring_slots=1), 'r_row != the padded fan-in': r4, 'kind = 3': dict(kind=3), 'm_max = 3': wide,
             'ws off a word': dict(ws=p(ws_big) + 2)}
    for fn, arg, cls in ((lib.nmarl_lstm_bptt_coupled, ac, _lib.BpttCoupled), (lib.nmarl_lstm_bptt_dial, ad, _lib.BpttDial)):
        assert arg.ring_slots >= 2 and arg.r_row == 2 and arg.m_max == 2 and arg.T == T and arg.E == E
        for what, kw in cases.items():
            if what == 'kind = 3' and cls is _lib.BpttDial:
                continue
            a = cls.from_buffer_copy(arg)
            for k, v in kw.items():
                setattr(a, k, v)
            assert fn(C.byref(a), _lib.stream()) == EINVAL, '%s: %s was not refused' % (cls.__name__, what)
            count += 1
    torch.cuda.synchronize()
    ops.check_coupled_status()
    for k, b in list(outs.items()) + list(co.items()):
        assert bool((b == SENTINEL).all()), 'a refused call wrote %s' % k
    print('refusals: %d calls refused, nothing written' % count)
    return count

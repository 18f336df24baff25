"""Every tier and buffer layout of the update's reverse recurrence (agents/sequence.py: coupled_sequence_saved; ops.py:
_LstmSequenceSaved, _LstmSequenceX), written as functions of the device: the CPU under cpu_ops() (tests/test_sequence_tiers_cpu.py)
and the real kernels (tests/test_gpu_sequence_tiers.py).

Reference: `unroll64` below, a plain autograd unroll in float64 of the three recurrences in the docstring of agents/sequence.py
(+ the message-less one of the uncoupled nets), the cell being oracle/ops_ref.lstm_cell.  It calls nothing of agents/sequence.py
and none of ops' sequence Functions.  The same unroll yields the "saved" inputs the product's backward starts from (gates G, state
sequences Hall / Call, LSTM inputs S, message terms hm / msg, lstm_ic3's mean_nbr(h_{t-1}) rows), rounded to float32 -- both sides
take their relu masks from them, so no kink can flip.

Cases: 4 agents on a line (m_max 2, neighbour counts 1 and 2), T = 3, H = 64.  Coupled: kind x tier x layout x masked_steps; a tier is
selected by patching the predicates the engine asks (TIER_PATCHES), a layout by how the saved buffers are handed over (LAYOUTS).
Uncoupled: function x tier x layout x masked_steps x form of the heads' gradient (tensor or dy8 placeholder).  Every run asserts the
BRANCH it took -- the call counts of the launch wrappers and the row counts of ops.wgrad's operands -- and then every gradient.

Bounds (the project's own): on the CPU rtol 2e-4, atol 2e-5 for every gradient (tests/test_sequence_cpu.py); on the GPU per-row
outputs (d enc, d s, d h0, d c0) at rtol 2e-4, atol 5e-5 and sums over rows (every weight and bias gradient) at rtol 1e-4, atol
1e-4 max(1, |ref| max) (tests/test_gpu_bptt_dial.py:128-131)."""
import contextlib
import functools

import torch

from bptt_edge_checks import line_table
from oracle import ops_ref

F32, F64 = torch.float32, torch.float64
H = 64
N, T = 4, 3
KX_UNCOUPLED = 32
HEAD_O = 5                                           # columns of dy8 in use (the heads' outputs)
KINDS = ('nc', 'ic3', 'dial')
MASKS = ('any', 'first')                             # masked_steps None with a done at t = 2 | masked_steps (0,)
TIERS = {'nc': ('one', 'step', 'torch'), 'ic3': ('one', 'step', 'torch'), 'dial': ('one', 'step', 'step_noadj', 'torch')}
# s_ext given (and lstm_dial's A2 padded) | neither | lstm_dial: A2 padded alone | lstm_ic3: the padded mean buffer as A1
LAYOUTS = {'nc': ('flat', 'padded'), 'ic3': ('flat', 'padded', 'flat+mm', 'padded+mm'), 'dial': ('flat', 'padded', 'a2pad')}
GPU_TIERS = {'nc': ('one', 'step', 'torch'), 'ic3': ('one', 'torch'), 'dial': ('one', 'step', 'torch')}
LAUNCHES = ('bptt_dial', 'bptt_coupled', 'bptt_seq', 'bptt_step', 'dial_msg_adjoint', 'cell_bwd')


def _no(*a, **k):
    return False


TIER_PATCHES = {'one': {},
                'step': dict(bptt_coupled_supported=_no, bptt_dial_supported=_no),
                'step_noadj': dict(bptt_coupled_supported=_no, bptt_dial_supported=_no, dial_adjoint_supported=_no),
                'torch': dict(bptt_supported=_no)}


def expected_launches(kind, tier, cuda):
    """The call counts a tier implies.  lstm_dial's one-launch kernel needs a GPU: on the CPU its 'one' is the step-wise pair."""
    e = dict.fromkeys(LAUNCHES, 0)
    if tier == 'torch':
        e['cell_bwd'] = T
    elif kind == 'x':
        e['bptt_seq'] = 1
    elif tier == 'one' and kind != 'dial':
        e['bptt_coupled'] = 1
    elif tier == 'one' and cuda:
        e['bptt_dial'] = 1
    else:
        e['bptt_step'] = T
        if kind == 'dial' and tier != 'step_noadj':
            e['dial_msg_adjoint'] = T
    return e


# ------------------------------------------------------------------------------------------------- patching and spying
@contextlib.contextmanager
def patched(ops, **attrs):
    saved = {k: getattr(ops, k) for k in attrs}
    try:
        for k, v in attrs.items():
            setattr(ops, k, v)
        yield
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)


@contextlib.contextmanager
def spied(ops):
    """-> {name: one entry per call}: ops.wgrad: the operands' row count; the launch wrappers: whether head_dy was given."""
    calls = {k: [] for k in LAUNCHES + ('wgrad',)}

    def wrap(name, f):
        def g(*a, **k):
            calls[name].append(a[0].shape[1] if name == 'wgrad' else k.get('head_dy') is not None)
            return f(*a, **k)
        return g
    with patched(ops, **{k: wrap(k, getattr(ops, k)) for k in calls}):
        yield calls


# ------------------------------------------------------------------------------------------------ the float64 reference
def _gather(x, tab):
    zero = torch.zeros_like(x[0])
    return torch.stack([torch.cat([x[j] if j >= 0 else zero for j in row], dim=-1) for row in tab.tolist()], dim=0)


def _mean(x, tab):
    rows = [[j for j in row if j >= 0] for row in tab.tolist()]
    return torch.stack([sum(x[j] for j in js) / len(js) if js else torch.zeros_like(x[0]) for js in rows], dim=0)


def unroll64(kind, tab, p, enc, h0, c0, done):
    """-> (Hs [N,T,E,H] attached to the graph, the saved sequences as lists of detached per-step tensors)."""
    E = done.shape[1]
    h, c = h0, c0
    sv = dict(G=[], H=[h0.detach()], C=[c0.detach()], S=[], hm=[], msg=[], mm=[])
    hs = []
    for t in range(T):
        keep = (1.0 - done[t]).view(1, E, 1)
        if kind == 'nc':
            hm = torch.relu(torch.bmm(_gather(h, tab), p['w_msg']) + p['b_msg'].unsqueeze(1))
            s = torch.cat([enc[:, t], hm], dim=-1)
        elif kind == 'ic3':
            mm = _mean(h, tab)
            sv['mm'].append(mm.detach())
            s = enc[:, t] + torch.bmm(mm, p['w_msg']) + p['b_msg'].unsqueeze(1)
        elif kind == 'dial':
            msg = torch.relu(torch.bmm(h, p['mfc_w']) + p['mfc_b'].unsqueeze(1))
            hm = torch.relu(torch.bmm(_gather(msg, tab), p['w_msg']) + p['b_msg'].unsqueeze(1))
            sv['msg'].append(msg.detach())
            s = enc[:, t] + hm
        else:
            s = enc[:, t]
        if kind in ('nc', 'dial'):
            sv['hm'].append(hm.detach())
        z = torch.bmm(s, p['wx']) + torch.bmm(h * keep, p['wh'])
        h, c = ops_ref.lstm_cell(z, p['b'], c, done[t])
        zb = (z + p['b'].unsqueeze(1)).detach()
        sv['G'].append(torch.cat([torch.sigmoid(zb[..., :3 * H]), torch.tanh(zb[..., 3 * H:])], dim=-1))
        sv['S'].append(s.detach())
        sv['H'].append(h.detach())
        sv['C'].append(c.detach())
        hs.append(h)
    return torch.stack(hs, dim=1), sv


@functools.lru_cache(maxsize=None)
def case(kind, mask, E, form='tensor'):
    """Inputs (float32, CPU), the saved sequences and the float64 gradients of sum(Hs dL/dh) for one (kind, done pattern, E, form of
    dL/dh).  Computed once and shared: callers clone what they hand to the product (it masks Hall in place)."""
    g = torch.Generator().manual_seed(KINDS.index(kind) * 100 + MASKS.index(mask) * 10 + E if kind != 'x' else 7000 + MASKS.index(mask) * 10 + E)
    r = lambda *s: torch.randn(*s, generator=g)                                         # noqa: E731
    tab = line_table(N)
    m_max = tab.shape[1]
    assert m_max == 2 and sorted(int((row >= 0).sum()) for row in tab) == [1, 1, 2, 2]
    w_enc, kx = {'nc': (2 * H, 3 * H), 'ic3': (H, H), 'dial': (H, H), 'x': (KX_UNCOUPLED, KX_UNCOUPLED)}[kind]
    p = dict(wx=r(N, kx, 4 * H) * 0.1, wh=r(N, H, 4 * H) * 0.1, b=r(N, 4 * H) * 0.1)
    if kind != 'x':
        p['w_msg'], p['b_msg'] = r(N, H if kind == 'ic3' else H * m_max, H) * 0.15, r(N, H) * 0.1
    if kind == 'dial':
        p['mfc_w'], p['mfc_b'] = r(N, H, H) * 0.2, r(N, H) * 0.1
    x = dict(enc=r(N, T, E, w_enc) * 0.5, h0=r(N, E, H) * 0.3, c0=r(N, E, H) * 0.3)
    done = torch.zeros(T, E)
    done[0, 1 % E] = 1.0
    if mask == 'any':
        done[2, 0] = 1.0                                   # a mid-batch episode start: every step masks
    if form == 'dy8':
        dy8 = torch.zeros(N, T * E, 8)
        dy8[:, :, :HEAD_O] = r(N, T * E, HEAD_O)
        hw = r(N, H, HEAD_O) * 0.3
        x['dy8'], x['hw'] = dy8, hw
        dh64 = torch.bmm(dy8[:, :, :HEAD_O].double(), hw.double().transpose(1, 2)).view(N, T, E, H)
    else:
        x['dh'] = r(N, T, E, H)
        dh64 = x['dh'].double()
    leaves = {k: v.double().requires_grad_(True) for k, v in {**p, **x}.items() if k in p or k in ('enc', 'h0', 'c0')}
    Hs, sv = unroll64(kind, tab, leaves, leaves['enc'], leaves['h0'], leaves['c0'], done.double())
    (Hs * dh64).sum().backward()
    ref = {k: v.grad for k, v in leaves.items()}
    assert any(float(v.abs().max()) > 0 for v in ref.values())
    saved = {k: torch.stack(v, dim=1).float() for k, v in sv.items() if v}
    return dict(tab=tab, p=p, x=x, done=done, saved=saved, ref=ref, Hs=Hs.detach())


def _padded(x, dev):
    """[N,T,E,W] -> the (T + 1)-slab buffer on `dev` whose first T slabs hold x, last slab zero."""
    buf = torch.zeros(N, T + 1, x.shape[2], x.shape[3], device=dev)
    buf[:, :T].copy_(x)
    return buf


def _compare(got, ref, cuda, what):
    """got: {name: (tensor, per_row)}.  -> the largest |difference|."""
    worst = 0.0
    for name, (a, per_row) in got.items():
        assert a is not None, '%s: no gradient for %s' % (what, name)
        a, b = a.detach().cpu().double(), ref[name]
        if not cuda:
            tol = dict(rtol=2e-4, atol=2e-5)
        elif per_row:
            tol = dict(rtol=2e-4, atol=5e-5)
        else:
            tol = dict(rtol=1e-4, atol=1e-4 * max(1.0, float(b.abs().max())))
        worst = max(worst, float((a - b).abs().max()))
        torch.testing.assert_close(a, b, msg=lambda m, name=name: '%s %s: %s' % (what, name, m), **tol)
    return worst


def _sync(ops, dev):
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize()
        ops.check_coupled_status()


# ------------------------------------------------------------------------------------------------- the coupled recurrences
def check_coupled(ops, sequence, dev, kind, tier, layout, mask, E, flat_weights=True):
    """sequence.coupled_sequence_saved on the saved sequences of `case`: the launches of the tier, the operand rows of the layout,
    then every gradient (the flat [wx; wh], b, w_msg, b_msg, mfc_w, mfc_b, enc) against the float64 unroll."""
    assert tier in TIERS[kind] and layout in LAYOUTS[kind] and mask in MASKS
    cuda = torch.device(dev).type == 'cuda'
    what = 'coupled %s tier=%s layout=%s mask=%s E=%d%s' % (kind, tier, layout, mask, E, '' if flat_weights else ' separate weights')
    c = case(kind, mask, E)
    sv, p = c['saved'], c['p']
    t = lambda v: v.clone().to(dev)                                                     # noqa: E731
    kx = p['wx'].shape[1]
    if flat_weights:                                       # [wx; wh] adjacent rows of one buffer: the one-GEMM dgrad of the torch tier
        flat = t(torch.cat([p['wx'], p['wh']], dim=1)).requires_grad_(True)
        wx, wh = flat[:, :kx], flat[:, kx:]
        assert wx.data_ptr() + kx * 4 * H * 4 == wh.data_ptr()
    else:
        wx, wh = t(p['wx']).requires_grad_(True), t(p['wh']).requires_grad_(True)
    prm = {k: t(p[k]).requires_grad_(True) for k in ('b', 'w_msg', 'b_msg', 'mfc_w', 'mfc_b') if k in p}
    enc = t(c['x']['enc']).requires_grad_(True)
    pad = layout.startswith('padded')
    s_ext = _padded(sv['S'], dev) if pad else None
    S = s_ext[:, :T] if pad else t(sv['S'])
    extra = {}
    if kind == 'dial':
        extra = dict(A1=t(sv['hm']), A2=_padded(sv['msg'], dev) if layout in ('padded', 'a2pad') else t(sv['msg']))
    elif kind == 'ic3' and layout.endswith('+mm'):
        extra = dict(A1=_padded(sv['mm'], dev))
    with patched(ops, **TIER_PATCHES[tier]), spied(ops) as calls:
        Hs = sequence.coupled_sequence_saved(kind, c['tab'].to(dev), None if mask == 'any' else (0,), enc, t(c['done']), wx, wh, prm['b'],
                                             prm['w_msg'], prm['b_msg'], prm.get('mfc_w'), prm.get('mfc_b'), t(sv['G']), t(sv['H']),
                                             t(sv['C']), S, extra, s_ext=s_ext)
        (Hs * t(c['x']['dh'])).sum().backward()
        _sync(ops, dev)
    assert {k: len(calls[k]) for k in LAUNCHES} == expected_launches(kind, tier, cuda), '%s: launches %s' % (what, {k: len(calls[k]) for k in LAUNCHES})
    rows, small, big = calls['wgrad'], T * E, (T + 1) * E
    if pad:
        assert rows and set(rows) == {big}, '%s: a weight gradient left the padded layout: rows %s' % (what, rows)
    elif layout == 'a2pad':                                # D1 follows A2 into the padded layout (the per-run products); dZ, D2 and S stay flat
        assert rows.count(small) == 3 and rows.count(big) == len(rows) - 3 >= 1, '%s: rows %s' % (what, rows)
    else:
        assert rows and set(rows) == {small}, '%s: rows %s' % (what, rows)
    got = {k: (v.grad, False) for k, v in prm.items()}
    got['enc'] = (enc.grad, True)
    ref = dict(c['ref'])
    if flat_weights:
        got['[wx; wh]'] = (flat.grad, False)
        ref['[wx; wh]'] = torch.cat([ref['wx'], ref['wh']], dim=1)
    else:
        got['wx'], got['wh'] = (wx.grad, False), (wh.grad, False)
    worst = _compare(got, ref, cuda, what)
    print('%s: largest |difference| %.3g' % (what, worst))
    return worst


# ----------------------------------------------------------------------------------------------- the uncoupled recurrences
UNCOUPLED_TIERS = ('one', 'torch')
FORMS = ('tensor', 'dy8')


def check_uncoupled(ops, dev, fn, tier, layout, mask, form, E):
    """ops._LstmSequenceSaved (fn 'saved'; layouts flat / padded) or ops._LstmSequenceX (fn 'x': its own forward, no s_ext) with the
    heads' gradient as a tensor or as the dy8 placeholder: launches, operand rows -- the padded layout only where it is offered,
    few steps mask and (T + 1) E is a multiple of ops.WGRAD_SPLIT --, gradients; no dy8 entry left pending."""
    assert fn in ('saved', 'x') and tier in UNCOUPLED_TIERS and layout in ('flat', 'padded') and form in FORMS and (fn == 'saved' or layout == 'flat')
    cuda = torch.device(dev).type == 'cuda'
    what = 'uncoupled %s tier=%s layout=%s mask=%s %s E=%d' % (fn, tier, layout, mask, form, E)
    c = case('x', mask, E, form)
    sv, p, x = c['saved'], c['p'], c['x']
    t = lambda v: v.clone().to(dev)                                                     # noqa: E731
    prm = {k: t(p[k]).requires_grad_(True) for k in ('wx', 'wh', 'b')}
    s_ext = _padded(x['enc'], dev) if layout == 'padded' else None
    s = (s_ext[:, :T].detach() if s_ext is not None else t(x['enc'])).requires_grad_(True)
    assert s_ext is None or s.data_ptr() == s_ext.data_ptr()
    masked = None if mask == 'any' else (0,)
    ops._pending_head_dy.clear()
    with patched(ops, **TIER_PATCHES[tier]), spied(ops) as calls:
        if fn == 'saved':
            Hs = ops._LstmSequenceSaved.apply(s, prm['wx'], prm['wh'], prm['b'], t(sv['G']), t(sv['H']), t(sv['C']), t(c['done']), masked, s_ext)
        else:
            prm['h0'], prm['c0'] = t(x['h0']).requires_grad_(True), t(x['c0']).requires_grad_(True)
            img = ops.lstm_wimage(prm['wx'].detach(), prm['wh'].detach())
            Hs = ops._LstmSequenceX.apply(s, prm['wx'], prm['wh'], prm['b'], prm['h0'], prm['c0'], t(c['done']), masked, img)
        if form == 'dy8':
            Hs.backward(gradient=ops.head_dy_placeholder(t(x['dy8']), t(x['hw']), Hs))
            assert not ops._pending_head_dy, '%s: the dy8 entry was not taken' % what
        else:
            Hs.backward(gradient=t(x['dh']))
        _sync(ops, dev)
    assert {k: len(calls[k]) for k in LAUNCHES} == expected_launches('x', tier, cuda), '%s: launches %s' % (what, {k: len(calls[k]) for k in LAUNCHES})
    if tier == 'one':
        assert calls['bptt_seq'] == [form == 'dy8'], '%s: the one-launch kernel did not get the gradient in the form handed over' % what
    in_place = layout == 'padded' and mask == 'first' and ((T + 1) * E) % ops.WGRAD_SPLIT == 0
    assert calls['wgrad'] == [(T + 1) * E if in_place else T * E] * 2, '%s: rows %s' % (what, calls['wgrad'])
    got = {k: (v.grad, k in ('h0', 'c0')) for k, v in prm.items()}
    got['enc'] = (s.grad, True)
    if fn == 'x':
        got_hs = Hs.detach().cpu().double()
        torch.testing.assert_close(got_hs, c['Hs'], rtol=2e-4, atol=5e-5 if cuda else 2e-5, msg=lambda m: '%s Hs: %s' % (what, m))
    worst = _compare(got, c['ref'], cuda, what)
    print('%s: largest |difference| %.3g' % (what, worst))
    return worst


COUPLED_CASES = [(k, tier, lay, m) for k in KINDS for tier in TIERS[k] for lay in LAYOUTS[k] for m in MASKS]
GPU_COUPLED_CASES = [c for c in COUPLED_CASES if c[1] in GPU_TIERS[c[0]]]
UNCOUPLED_CASES = [(fn, tier, lay, m, f) for fn in ('saved', 'x') for tier in UNCOUPLED_TIERS for lay in (('flat', 'padded') if fn == 'saved' else ('flat',))
                   for m in MASKS for f in FORMS]

"""The edge checks of tests/bptt_edge_checks.py are sharp: (a) the restatement oracle/ops_ref (fp32 on the CPU) stays within every
bound -- the chosen inputs and tolerances are satisfiable by the reference alone --, (b) every named wrong variant of it --
mistakes the reverse-recurrence kernels of csrc/lstm_bptt.hip could make without the older tests noticing -- makes the check that
targets it raise, at the edge shapes the GPU file runs.

The variants need single factors taken out of the cell backward, the products and the message adjoint, so `_Bptt` below restates
bptt_step / bptt_seq / bptt_coupled / bptt_dial with one switch per mistake -- test_switchable_restatement_is_ops_ref shows that
with every switch off it is ops_ref bit for bit.  check_refusals talks to the library and has no CPU twin."""
import types

import pytest
import torch

import bptt_edge_checks as bec
from oracle import ops_ref

H = bec.H
_NAMES = ('lstm_bptt_wimage', 'lstm_bptt_msg_wimage', 'reverse_neighbor_table', 'bptt_step_db_parts', 'bptt_step', 'bptt_seq', 'bptt_coupled',
          'bptt_dial')


def _impl():
    return types.SimpleNamespace(**{k: getattr(ops_ref, k) for k in _NAMES})


class _Bptt:
    """oracle/ops_ref's reverse recurrences, one switch per mistake."""
    FLAGS = ('no_keep_dhd', 'cprev_unmasked', 'tanh_at_cprev', 'mask_ge', 'swap_slot', 'ic3_recv_weight', 'drop_last_dy', 'bias_skip_tile_row',
             'dh2_needs_dc')

    def __init__(self, **flags):
        assert set(flags) <= set(self.FLAGS)
        for k in self.FLAGS:
            setattr(self, k, bool(flags.get(k, False)))
        for k in _NAMES[:4]:
            setattr(self, k, getattr(ops_ref, k))

    def cell_bwd(self, gates, c_prev, c_new, done, dh, dc, dz, dc_prev, dh2=None):
        gi, gf, go, gu = gates.split(H, dim=-1)
        keep = (1.0 - done).view(1, -1, 1)
        tc = torch.tanh(c_prev if self.tanh_at_cprev else c_new)
        g_h = torch.zeros_like(c_new) if dh is None else dh
        if dh2 is not None and not (self.dh2_needs_dc and dc is None):
            g_h = g_h + dh2
        g_c = (torch.zeros_like(c_new) if dc is None else dc) + g_h * go * (1 - tc * tc)
        cp = c_prev if self.cprev_unmasked else c_prev * keep
        dz.copy_(torch.cat([g_c * gu * gi * (1 - gi), g_c * cp * gf * (1 - gf), g_h * tc * go * (1 - go), g_c * gi * (1 - gu * gu)], dim=-1))
        dc_prev.copy_(g_c * gf * keep)

    def _rows(self, E):
        """The rows that reach the bias sums: all, or all but the last row of every 128-row tile."""
        r = torch.arange(E)
        return r[r % 128 != 127] if self.bias_skip_tile_row else r

    def _relu_mask(self, m):
        return (m >= 0) if self.mask_ge else (m > 0)

    def bptt_step(self, gates, c_prev, c_new, done, dh, dh2, dc, ws, dz, dc_prev, dhd, apply_keep, dx=None, mask=None, db_part=None):
        self.cell_bwd(gates, c_prev, c_new, done, dh, dc, dz, dc_prev, dh2=dh2)
        if db_part is not None:
            db_part[:, 0] += (dz[:, self._rows(dz.shape[1])] if self.bias_skip_tile_row else dz).sum(dim=1).to(db_part.dtype)
        wxm, wh, _ = ws
        r = torch.bmm(dz, wh.transpose(1, 2))
        if apply_keep and not self.no_keep_dhd:
            r = r * (1.0 - done).view(1, -1, 1)
        dhd.copy_(r)
        if wxm is not None:
            v = torch.bmm(dz, wxm.transpose(1, 2))
            if mask is not None:
                v = v * self._relu_mask(mask)
            dx.copy_(v)

    def _head_dh(self, head_dy, shape):
        dy8, hw = head_dy
        O = hw.shape[2] - (1 if self.drop_last_dy else 0)
        return torch.bmm(dy8[:, :, :O].to(hw.dtype), hw[:, :, :O].transpose(1, 2)).view(*shape, -1)

    def _bias(self, dZ):
        N, T, E, W = dZ.shape
        if self.bias_skip_tile_row:
            return dZ[:, :, self._rows(E)].sum(dim=(1, 2))
        return dZ.reshape(N, T * E, W).sum(dim=1)

    def bptt_seq(self, G, Call, done, dHs, img, dZ, want_db=True, want_state_grad=False, wh=None, head_dy=None):
        N, T, E, _ = G.shape
        if head_dy is not None:
            dHs = self._head_dh(head_dy, (N, T, E))
        wh = img if wh is None else wh
        dh_rec = None
        dc = torch.zeros(N, E, H, dtype=G.dtype)
        for t in range(T - 1, -1, -1):
            dc_prev, dhd = torch.empty_like(dc), torch.empty_like(dc)
            self.bptt_step(G[:, t], Call[:, t], Call[:, t + 1], done[t], dHs[:, t], dh_rec, dc, (None, wh, None), dZ[:, t], dc_prev, dhd, True)
            dc, dh_rec = dc_prev, dhd
        return (self._bias(dZ) if want_db else None), (dh_rec if want_state_grad else None), (dc if want_state_grad else None)

    def _gather_bwd(self, m_t, tab):
        """Adjoint of the neighbour gather: source (i, slot k) -> agent tab[i][k]; swap_slot: read from slot m_max - 1 - k."""
        if not self.swap_slot:
            return ops_ref.nbr_gather_bwd(m_t, tab, H)
        N, E, _ = m_t.shape
        m = tab.shape[1]
        out = torch.zeros(N, E, H, dtype=m_t.dtype)
        for i, js in enumerate(ops_ref.neighbor_lists(tab)):
            for k, j in enumerate(js):
                kk = m - 1 - k
                out[j] += m_t[i][:, kk * H:(kk + 1) * H]
        return out

    def _mean_bwd(self, m_t, tab):
        """Adjoint of the neighbour mean: weight 1 / |nbr(i)| of the agent i that formed the mean; ic3_recv_weight: 1 / |nbr(j)| of the
        agent j the adjoint goes to."""
        if not self.ic3_recv_weight:
            return ops_ref.nbr_mean_bwd(m_t, tab)
        lists = ops_ref.neighbor_lists(tab)
        out = torch.zeros_like(m_t)
        for i, js in enumerate(lists):
            for j in js:
                out[j] += m_t[i] / max(1, len(lists[j]))
        return out

    def bptt_coupled(self, kind, rev, m_max, G, Call, done, dHs, ws, wm, mask, dZ, D1, mode=0, head_dy=None):
        N, T, E, H4 = G.shape
        if head_dy is not None:
            dHs = self._head_dh(head_dy, (N, T, E))
        wxm, wh, _ = ws
        tab = rev['nbr_idx']
        dh_rec = None
        dc = torch.zeros(N, E, H, dtype=G.dtype)
        for t in range(T - 1, -1, -1):
            dz_t, dc_prev = torch.empty(N, E, H4, dtype=G.dtype), torch.empty(N, E, H, dtype=G.dtype)
            self.cell_bwd(G[:, t], Call[:, t], Call[:, t + 1], done[t], dHs[:, t], dc, dz_t, dc_prev, dh2=dh_rec)
            dc = dc_prev
            dZ[:, t].copy_(dz_t)
            dhd = torch.bmm(dz_t, wh.transpose(1, 2))
            if not self.no_keep_dhd:
                dhd = dhd * (1.0 - done[t]).view(1, -1, 1)
            dx = torch.bmm(dz_t, wxm.transpose(1, 2))
            if kind == 1:
                dx = dx * self._relu_mask(mask[:, t])
            D1[:, t].copy_(dx)
            m_t = torch.bmm(dx, wm[0].transpose(1, 2))
            dh_rec = (self._gather_bwd(m_t, tab) if kind == 1 else self._mean_bwd(m_t, tab)) + dhd
        if self.bias_skip_tile_row:
            return self._bias(dZ), D1[:, :, self._rows(E)].sum(dim=(1, 2))
        return dZ.sum(dim=(1, 2)), D1.sum(dim=(1, 2))

    def bptt_dial(self, rev, m_max, G, Call, done, dHs, ws, wm, img_f, hm, msg, dZ, DS, D1, D2, mode=0, head_dy=None, want_state_grad=False):
        N, T, E, _ = G.shape
        if head_dy is not None:
            dHs = self._head_dh(head_dy, (N, T, E))
        z = lambda: torch.zeros(N, E, H, dtype=G.dtype)                                 # noqa: E731
        dc, dc_next, dh_rec = z(), z(), None
        for t in range(T - 1, -1, -1):
            dhd = z()
            self.bptt_step(G[:, t], Call[:, t], Call[:, t + 1], done[t], dHs[:, t], dh_rec, dc, (ws[0], ws[1], None), dZ[:, t], dc_next, dhd, True,
                           dx=DS[:, t])
            dc, dc_next = dc_next, dc
            dh_rec = z()
            if self.mask_ge or self.swap_slot:
                D1[:, t].copy_(DS[:, t] * self._relu_mask(hm[:, t]).to(G.dtype))
                dmsg = self._gather_bwd(torch.bmm(D1[:, t], wm[0].transpose(1, 2)), rev['nbr_idx'])
                D2[:, t].copy_(dmsg * self._relu_mask(msg[:, t]).to(G.dtype))
                dh_rec.copy_(dhd + torch.bmm(D2[:, t], img_f.transpose(1, 2)))
            else:
                ops_ref.dial_msg_adjoint(DS[:, t], hm[:, t], msg[:, t], dhd, wm[0], img_f, rev['nbr_idx'], None, None, D1[:, t], D2[:, t], dh_rec)
        dh0, dc0 = (dh_rec, dc) if want_state_grad else (None, None)
        if self.bias_skip_tile_row:
            rows = self._rows(E)
            return self._bias(dZ), D1[:, :T][:, :, rows].sum(dim=(1, 2)), D2[:, :T][:, :, rows].sum(dim=(1, 2)), dh0, dc0
        return dZ.sum(dim=(1, 2)), D1[:, :T].sum(dim=(1, 2)), D2[:, :T].sum(dim=(1, 2)), dh0, dc0


# ------------------------------------------------------------------------------------------ (a) the restatement passes
@pytest.mark.parametrize('E', bec.E_EDGES)
def test_restatement_step_operands(E):
    assert bec.check_step_operands(_impl(), 'cpu', E) <= 1.0


@pytest.mark.parametrize('E', bec.E_EDGES)
@pytest.mark.parametrize('T', bec.T_EDGES)
def test_restatement_seq_edges(T, E):
    assert bec.check_seq_edges(_impl(), 'cpu', T, E) <= 1.0


@pytest.mark.parametrize('form', bec.COUPLED_FORMS)
@pytest.mark.parametrize('kind,table', [(k, t) for k in (1, 2) for t in bec.COUPLED_TABLES[k]])
def test_restatement_coupled_edges(kind, table, form):
    for T in bec.T_EDGES:
        for E in bec.COUPLED_E:
            bec.check_coupled_edges(_impl(), 'cpu', kind, table, T, E, form)


@pytest.mark.parametrize('form', bec.COUPLED_FORMS)
@pytest.mark.parametrize('table', bec.DIAL_TABLES)
def test_restatement_dial_edges(table, form):
    for T in bec.DIAL_T:
        for E in bec.DIAL_E:
            bec.check_dial_edges(_impl(), 'cpu', table, T, E, form)


def test_restatement_launcher_fallbacks(monkeypatch):
    """On the restatement every mode is the same loop: the check's plumbing (the cap, the pool, the variable) runs and is restored."""
    import os
    bec.check_launcher_fallbacks(_impl(), 'cpu', monkeypatch)
    assert 'NMARL_TEST_FAKE_CUS' not in os.environ


@pytest.mark.parametrize('entry', bec.SAT_ENTRIES)
def test_restatement_saturation(entry):
    bec.check_saturation(_impl(), 'cpu', entry)


def test_restatement_tanh_midrange():
    assert bec.check_tanh_midrange(_impl(), 'cpu') <= 1.0


def test_tables_are_what_the_census_says():
    """The restated ragged table is test_gpu_bptt_dial's; fan-in and symmetry of every table the checks launch."""
    facts = {k: bec.table_facts(f()) for k, f in bec.TABLES.items()}
    assert facts == {'line2': (1, True), 'line3': (2, True), 'ragged': (2, False), 'grid': (4, True), 'grid_cut': (4, False)}
    cut = bec.grid_table(True)
    assert int((cut[0] >= 0).sum()) == 0 and sum(int((cut[a] == 0).sum()) for a in range(9)) == 2      # agent 0: no neighbour, two sources
    assert bec.grid_table().ge(0).sum() - cut.ge(0).sum() == 3
    rag = bec.ragged_table().tolist()
    assert rag == [[3, -1], [0, 3], [1, -1], [-1, -1], [1, 2], [-1, -1]]


# ------------------------------------------------------------------------------------------ (b) the wrong variants fail
def _step(E):
    return lambda impl: bec.check_step_operands(impl, 'cpu', E)


def _seq(T, E):
    return lambda impl: bec.check_seq_edges(impl, 'cpu', T, E)


def _coupled(kind, table, T, E, form):
    return lambda impl: bec.check_coupled_edges(impl, 'cpu', kind, table, T, E, form)


def _dial(table, T, E, form):
    return lambda impl: bec.check_dial_edges(impl, 'cpu', table, T, E, form)


def _sat(entry):
    return lambda impl: bec.check_saturation(impl, 'cpu', entry)


# name -> (flag, [(check, tag of the assertion that must fire)])
MUTANTS = {
    '(1 - done) missing from dhd': ('no_keep_dhd', [(_step(17), 'close'), (_seq(2, 16), 'bits|close'), (_coupled(1, 'line3', 2, 17, 'tensor'), 'close'),
                                                    (_dial('line3', 2, 17, 'tensor'), 'close')]),
    'c_prev not masked in the forget-gate term': ('cprev_unmasked', [(_step(15), 'close'), (_seq(3, 129), 'bits|close'), (_sat('step'), 'exact|close'),
                                                                     (_sat('seq'), 'exact|close'), (_sat('coupled'), 'exact|close')]),
    'tanh\' taken at c_prev instead of c_new': ('tanh_at_cprev', [(_step(1), 'close'), (_seq(1, 1), 'bits|close'),
                                                                  (lambda impl: bec.check_tanh_midrange(impl, 'cpu'), 'tanh')]),
    'relu mask >= 0 instead of > 0': ('mask_ge', [(_step(16), 'close|mask'), (_coupled(1, 'line2', 1, 1, 'tensor'), 'close|mask'),
                                                  (_dial('ragged', 1, 17, 'tensor'), 'close|mask')]),
    'the lstm_comm slot column of a source swapped': ('swap_slot', [(_coupled(1, 'line3', 2, 17, 'tensor'), 'close'),
                                                                    (_coupled(1, 'ragged', 2, 17, 'dy8'), 'close'), (_dial('line3', 2, 17, 'tensor'), 'close')]),
    'the lstm_ic3 weight 1 / |nbr(receiver)|': ('ic3_recv_weight', [(_coupled(2, 'line3', 2, 17, 'tensor'), 'close'), (_coupled(2, 'grid', 3, 1, 'dy8'), 'close'),
                                                                    (_coupled(2, 'grid_cut', 2, 129, 'tensor'), 'close')]),
    'the last column of dy8 dropped': ('drop_last_dy', [(_seq(2, 17), 'dy8|close'), (_coupled(1, 'line2', 2, 17, 'dy8'), 'close'),
                                                        (_coupled(2, 'grid', 1, 17, 'dy8'), 'close'), (_dial('line3', 1, 17, 'dy8'), 'close')]),
    'the last row of a tile left out of the bias sum': ('bias_skip_tile_row', [(_step(128), 'db'), (_step(257), 'db'), (_seq(2, 129), 'db'),
                                                                               (_coupled(1, 'line3', 1, 129, 'tensor'), 'db'),
                                                                               (_dial('line3', 1, 129, 'tensor'), 'db')]),
    'dh2 ignored when dc is absent': ('dh2_needs_dc', [(_step(127), 'close')]),
}


@pytest.mark.parametrize('name', list(MUTANTS))
def test_mutant_fails(name):
    """Every wrong variant is caught by each check listed for it, at an edge shape of the GPU file.  Visible only on some tables: the
    swapped slot column needs m_max = 2 (line of 3, ragged; on the line of 2 the one slot is its own mirror); the lstm_ic3 weight
    needs two agents with different neighbour counts (every table used: the line's ends have 1, its middle 2).  The bias row needs
    E >= 128: see test_mutants_below_their_edge_pass."""
    flag, checks = MUTANTS[name]
    for check, tag in checks:
        with pytest.raises(AssertionError, match=r'^\[(%s)\]' % tag):
            check(_Bptt(**{flag: True}))


def test_mutants_below_their_edge_pass():
    """The same variants where their mistake cannot show: the bias row below one full tile, the slot swap with one slot, the dy8
    column in the tensor form -- the checks fail for the mistake, not for the variant's plumbing."""
    bec.check_step_operands(_Bptt(bias_skip_tile_row=True), 'cpu', 127)
    bec.check_coupled_edges(_Bptt(swap_slot=True), 'cpu', 1, 'line2', 2, 17, 'tensor')
    bec.check_coupled_edges(_Bptt(drop_last_dy=True), 'cpu', 2, 'grid', 2, 17, 'tensor')
    bec.check_coupled_edges(_Bptt(ic3_recv_weight=True), 'cpu', 1, 'line3', 2, 17, 'tensor')


def test_switchable_restatement_is_ops_ref():
    """_Bptt with every switch off == ops_ref bit for bit (the variants differ from the restatement by their one mistake alone), and
    passes the checks."""
    a, b = _Bptt(), _impl()
    N, T, E = 3, 3, 17
    tab = bec.line_table(3)
    for kind, form in ((1, 'tensor'), (2, 'dy8')):
        d = bec._coupled_inputs(kind, tab, T, E, form, 5)
        outs = []
        for impl in (a, b):
            dZ, D1 = torch.zeros(N, T, E, 4 * H), torch.zeros(N, T, E, H)
            db, dbm = impl.bptt_coupled(kind, dict(nbr_idx=tab), 2, d['gates'], d['call'], d['done'], d.get('dhs'), (d['wxm'], d['wh'], None),
                                        (d['w_msg'], None), d['S'][..., 2 * H:] if kind == 1 else None, dZ, D1,
                                        head_dy=(d['dy8'], d['hw']) if form == 'dy8' else None)
            outs.append((dZ, D1, db, dbm))
        assert all(torch.equal(x, y) for x, y in zip(*outs))
    d = bec._dial_inputs(tab, T, E, 'tensor', 6)
    x, y = bec.run_dial(a, 'cpu', tab, d, 1, 'tensor'), bec.run_dial(b, 'cpu', tab, d, 1, 'tensor')
    for k in x:
        assert torch.equal(*(v.v if isinstance(v, bec.Out) else v for v in (x[k], y[k]))), k
    outs = []
    for impl in (a, b):
        dZ = torch.zeros(N, T, E, 4 * H)
        outs.append((dZ,) + tuple(impl.bptt_seq(d['gates'], d['call'], d['done'], d['dhs'], d['wh'], dZ, want_state_grad=True)))
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    for impl in (a,):
        bec.check_step_operands(impl, 'cpu', 129)
        bec.check_seq_edges(impl, 'cpu', 2, 17)
        bec.check_saturation(impl, 'cpu', 'coupled')
        bec.check_tanh_midrange(impl, 'cpu')


def test_every_named_variant_is_there():
    """The issue names nine wrong variants, one per switch; none is silently dropped."""
    assert len(MUTANTS) == 9 and sorted(f for f, _ in MUTANTS.values()) == sorted(_Bptt.FLAGS)

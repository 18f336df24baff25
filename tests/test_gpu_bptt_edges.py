"""The reverse-recurrence kernels (csrc/lstm_bptt.hip: nmarl_lstm_bptt_step / _seq / _coupled / _dial) in every launch branch and at
the input edges the older tests leave out: the cross of bptt_step's optional operands, T = 1 / 2 / 3 and row counts around a wave
and a tile, done patterns, every heads-gradient width of the dy8 forms, asymmetric and -1 padded tables, the launchers' own
fallbacks, saturated gates and cells, the fast tanh's mid-range and what the launchers refuse -- each against a float64
expectation (tests/bptt_edge_checks.py, whose docstring holds the dispatch census; tests/test_bptt_edges_cpu.py shows that the
checks fail for the mistakes they are meant to see)."""
import pytest

import bptt_edge_checks as bec

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('E', bec.E_EDGES)
def test_step_operands(E):
    from deeprl_network_amd import ops
    bec.check_step_operands(ops, 'cuda', E)


@pytest.mark.parametrize('E', bec.E_EDGES)
@pytest.mark.parametrize('T', bec.T_EDGES)
def test_seq_edges(T, E):
    from deeprl_network_amd import ops
    bec.check_seq_edges(ops, 'cuda', T, E)


@pytest.mark.parametrize('form', bec.COUPLED_FORMS)
@pytest.mark.parametrize('kind,table', [(k, t) for k in (1, 2) for t in bec.COUPLED_TABLES[k]])
def test_coupled_edges(kind, table, form):
    from deeprl_network_amd import ops
    for T in bec.T_EDGES:
        for E in bec.COUPLED_E:
            bec.check_coupled_edges(ops, 'cuda', kind, table, T, E, form)


@pytest.mark.parametrize('form', bec.COUPLED_FORMS)
@pytest.mark.parametrize('table', bec.DIAL_TABLES)
def test_dial_edges(table, form):
    from deeprl_network_amd import ops
    for T in bec.DIAL_T:
        for E in bec.DIAL_E:
            bec.check_dial_edges(ops, 'cuda', table, T, E, form)


def test_launcher_fallbacks(monkeypatch):
    from deeprl_network_amd import ops
    bec.check_launcher_fallbacks(ops, 'cuda', monkeypatch)


@pytest.mark.parametrize('entry', bec.SAT_ENTRIES)
def test_saturation(entry):
    from deeprl_network_amd import ops
    bec.check_saturation(ops, 'cuda', entry)


def test_tanh_midrange():
    from deeprl_network_amd import ops
    bec.check_tanh_midrange(ops, 'cuda')


def test_refusals_write_nothing():
    assert bec.check_refusals('cuda') == 21

"""The lock-step LSTM kernel (csrc/lstm_mfma.hip, nmarl_lstm_step_x) in every instantiation that waits for no other block and at
the input edges the older tests leave out: the two-piece input [x | x2] and the refusals around it, every bf16x3 form at the
split-product bound, row counts around a wave and a block edge, and the (1 - done) mask on large stale state -- each against a
float64 expectation formed inside the check (tests/step_edge_checks.py, whose docstring holds the dispatch census;
tests/test_step_edges_cpu.py shows that the checks fail for the mistakes they are meant to see)."""
import pytest

import step_edge_checks as sec

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('split,precision', [(s, 'fp32') for s in sec.TWO_PIECE_SPLITS] + [(s, 'bf16x3') for s in sec.TWO_PIECE_X3_SPLITS])
@pytest.mark.parametrize('E', sec.TWO_PIECE_E)
def test_two_piece(E, split, precision):
    from deeprl_network_amd import ops
    for pitch in sec.TWO_PIECE_PITCH:
        for head in sec.TWO_PIECE_HEADS:
            for addends in (0, 1):
                sec.check_two_piece(ops, 'cuda', 3, E, split[0], split[1], pitch, head, addends, precision)


def test_x2_refusals_write_nothing():
    assert sec.check_x2_refusals('cuda') == 11


@pytest.mark.parametrize('form', sec.X3_FORMS)
@pytest.mark.parametrize('E', sec.X3_E)
def test_bf16x3_form(E, form):
    from deeprl_network_amd import ops
    for KX, addends in ([(128 if form == 'enc_pair' else 64, 0)] if form.startswith('enc') else sec.X3_KX):
        sec.check_bf16x3_form(ops, 'cuda', form, 3, E, KX, addends)


@pytest.mark.parametrize('form', sec.ROW_EDGE_HEAD_FORMS)
@pytest.mark.parametrize('E', sec.ROW_EDGE_E)
def test_row_edges(E, form):
    from deeprl_network_amd import ops
    for KX, addends in sec.ROW_EDGE_KX:
        for A in ((1, 8) if form in ('head1', 'head3') else (4,)):
            sec.check_row_edges(ops, 'cuda', form, E, KX=KX, addends=addends, A=A)
        if form == 'head2':                  # a critic without a neighbour term (m_max = 0: the wrapper admits it)
            sec.check_row_edges(ops, 'cuda', form, E, KX=KX, addends=addends, m_max=0)


@pytest.mark.parametrize('form', sec.ROW_EDGE_MSG_FORMS)
@pytest.mark.parametrize('E', sec.ROW_EDGE_E)
def test_row_edges_message_forms(E, form):
    from deeprl_network_amd import ops
    sec.check_row_edges(ops, 'cuda', form, E)


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('head', sec.DONE_HEADS)
def test_done_mask(head, precision):
    from deeprl_network_amd import ops
    sec.check_done_mask(ops, 'cuda', head, precision)

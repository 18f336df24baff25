"""The update's encoder and heads kernels (csrc/fc.hip, csrc/nbr.hip) in every branch their host wrappers can take, the one-pass
heads + loss kernel where the probability clip acts, and the step / cell kernels' transcendentals at saturation -- each against a
float64 expectation formed inside the check (tests/fc_edge_checks.py, whose docstring holds the dispatch census;
tests/test_fc_edges_cpu.py shows that the checks fail for the mistakes they are meant to see)."""
import pytest

import fc_edge_checks as fec

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('layout', fec.FC_BWD_LAYOUTS)
@pytest.mark.parametrize('F', fec.FC_BWD_F)
@pytest.mark.parametrize('rows', fec.FC_BWD_ROWS)
@pytest.mark.parametrize('N', [2, 5])
def test_fc_bwd_rows_branch(N, rows, F, layout):
    from deeprl_network_amd import ops
    fec.check_fc_bwd_rows(ops, 'cuda', N, rows, F, layout, (rows + F + len(layout)) % 3)


@pytest.mark.parametrize('layout', fec.FC_BWD_LAYOUTS)
@pytest.mark.parametrize('F', fec.FC_BWD_F)
@pytest.mark.parametrize('rows', [63, 4103])
def test_fc_bwd_rows_branch_with_in_kernel_gather(rows, F, layout):
    from deeprl_network_amd import ops
    fec.check_fc_bwd_rows(ops, 'cuda', 5, rows, F, layout, 1 + rows % 2, gather=True)


@pytest.mark.parametrize('case', fec.FC_MULTI_CASES)
@pytest.mark.parametrize('rows', fec.FC_MULTI_ROWS)
def test_fc_fwd_multi_branches(rows, case):
    from deeprl_network_amd import ops
    fec.check_fc_fwd_multi(ops, 'cuda', rows, case)


@pytest.mark.parametrize('F', fec.NBR_F)
@pytest.mark.parametrize('E', fec.NBR_E)
def test_nbr_ragged_table(E, F):
    from deeprl_network_amd import ops
    fec.check_nbr_ragged(ops, 'cuda', E, F)


def test_fc_and_nbr_refusals_write_nothing():
    fec.check_refusals('cuda')


@pytest.mark.parametrize('want_dh', [True, False])
@pytest.mark.parametrize('A', fec.HEADS_LOSS_A)
@pytest.mark.parametrize('rows', fec.HEADS_LOSS_ROWS)
@pytest.mark.parametrize('N', fec.HEADS_LOSS_N)
def test_heads_loss_at_peaked_policies(N, rows, A, want_dh):
    from deeprl_network_amd import ops
    fec.check_heads_loss_clip(ops, 'cuda', N, rows, A, want_dh)


@pytest.mark.parametrize('path', fec.SWEEP_PATHS)
def test_gate_sweep(path):
    from deeprl_network_amd import ops
    fec.check_gate_sweep(ops, 'cuda', path)


@pytest.mark.parametrize('part', fec.BPTT_SAT_PARTS)
def test_bptt_with_saturated_gates(part):
    from deeprl_network_amd import ops
    fec.check_bptt_saturated(ops, 'cuda', part)


@pytest.mark.parametrize('rows', [1, 300])
def test_nbr_action_value_accumulates(rows):
    from deeprl_network_amd import ops
    fec.check_nbr_action_value_accumulate(ops, 'cuda', rows)


def test_onehot_argmax_ties():
    from deeprl_network_amd import ops
    fec.check_onehot_argmax_ties(ops, 'cuda')


@pytest.mark.parametrize('rows', [63, 65])
def test_thin_linear_bwd_eight_outputs(rows):
    from deeprl_network_amd import ops
    fec.check_thin_linear_bwd_o8(ops, 'cuda', rows)

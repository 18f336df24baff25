"""The update path's small kernels (csrc/a2c.hip: return scan, clip + RMSProp, action draw, batch epilogue, multi-copy) at their
edges, each against a float64 expectation formed inside the check (tests/update_edge_checks.py; tests/test_update_edges_cpu.py shows
that every check fails for every mistake it is meant to see)."""
import pytest

import update_edge_checks as uec

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('use_lr_dev', [False, True])
@pytest.mark.parametrize('G,P,max_norm,grad_scale', uec.RMSPROP_SHAPES)
def test_rmsprop_step_state_and_norm(G, P, max_norm, grad_scale, use_lr_dev):
    from deeprl_network_amd import ops
    uec.check_rmsprop(ops, 'cuda', G, P, max_norm, grad_scale, use_lr_dev)


def test_rmsprop_guard_with_a_private_status_word():
    uec.check_rmsprop_guard('cuda')


@pytest.mark.parametrize('table', uec.NSTEP_TABLES)
@pytest.mark.parametrize('alpha', uec.NSTEP_ALPHAS)
@pytest.mark.parametrize('N,E,T', uec.NSTEP_SHAPES)
def test_nstep_return_edges(N, E, T, alpha, table):
    from deeprl_network_amd import ops
    uec.check_nstep(ops, 'cuda', N, E, T, alpha, table)


def test_nstep_return_abi_refusals():
    uec.check_nstep_abi_refusals('cuda')


@pytest.mark.parametrize('mode', uec.SAMPLE_MODES)
@pytest.mark.parametrize('N,A', uec.SAMPLE_SHAPES)
def test_sample_actions_edges(N, A, mode):
    from deeprl_network_amd import ops
    uec.check_sample(ops, 'cuda', N, uec.SAMPLE_E, A, mode)


@pytest.mark.parametrize('skip_pattern', [False, True])
@pytest.mark.parametrize('N,E,H,A,F,T', uec.EPILOGUE_SHAPES)
def test_batch_epilogue_edges(N, E, H, A, F, T, skip_pattern):
    from deeprl_network_amd import ops
    uec.check_epilogue(ops, 'cuda', N, E, H, A, F, T, 4, skip_pattern)


def test_copy_multi_skip_word():
    uec.check_copy_multi_skip('cuda')

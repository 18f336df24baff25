"""The opt-in `lstm_precision` of the uncoupled nets' lock-step (fp32 | bf16x3) on the host side: the ini key and the CLI flag, the
fp32 default of every reference ini, the refusal of the nets the mode does not exist for, and the bf16x3 kernels' resources."""
import configparser
import json
import os
import sys

import numpy as np
import pytest

from cpu_emulation import cpu_ops
from helpers import GOLDEN, cacc_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = json.load(open(os.path.join(GOLDEN, 'reference_tables.json')))['configs']
NB = np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]])


def _model(agent, precision=None):
    from deeprl_network_amd.agents import models
    cls = {'ia2c': models.IA2C, 'ia2c_fp': models.IA2C_FP, 'ma2c_nc': models.MA2C_NC, 'ma2c_ic3': models.MA2C_IC3,
           'ma2c_cu': models.IA2C_CU, 'ma2c_dial': models.MA2C_DIAL}[agent]
    cp = cacc_config(agent=agent)
    if precision is not None:
        cp['MODEL_CONFIG']['lstm_precision'] = precision
    n_s = [5 if agent.startswith('ma2c') else 5 * (1 + int(NB[i].sum())) for i in range(3)]
    np.random.seed(12)
    with cpu_ops():
        return cls(n_s, [4] * 3, NB, NB, -1.0, 0, cp['MODEL_CONFIG'], seed=12, num_envs=1, device='cpu')


@pytest.mark.parametrize('agent', ['ia2c', 'ia2c_fp', 'ma2c_cu'])
@pytest.mark.parametrize('precision', [None, 'fp32', 'bf16x3', ' bf16x3 '])
def test_ini_key_reaches_the_policy(agent, precision):
    m = _model(agent, precision)
    want = 'fp32' if precision is None else precision.strip()
    assert m.lstm_precision == want and m.policy.precision == want


def test_unknown_precision_is_refused():
    with pytest.raises(ValueError, match='lstm_precision'):
        _model('ia2c_fp', 'bf16')


@pytest.mark.parametrize('path', sorted(p for p in CONFIGS if 'MODEL_CONFIG' in CONFIGS[p]))
def test_absent_key_means_fp32_for_every_reference_ini(path):
    from deeprl_network_amd import ops
    cp = configparser.ConfigParser()
    cp.read_dict(CONFIGS[path])
    assert not cp.has_option('MODEL_CONFIG', 'lstm_precision')
    assert ops.check_precision(cp['MODEL_CONFIG'].get('lstm_precision', fallback='fp32')) == 'fp32'


@pytest.mark.parametrize('agent,net', [('ma2c_nc', 'NCMultiAgentPolicy'), ('ma2c_ic3', 'IC3MultiAgentPolicy'),
                                       ('ma2c_dial', 'DIALMultiAgentPolicy')])
def test_coupled_nets_are_fp32_only(agent, net):
    with pytest.raises(ValueError, match='%s.*fp32-only' % net):
        _model(agent, 'bf16x3')
    assert _model(agent).policy.precision == 'fp32'


def test_cli_flag_parses():
    from deeprl_network_amd.main import parse_args
    assert parse_args(['train']).lstm_precision is None
    assert parse_args(['train', '--lstm-precision', 'bf16x3']).lstm_precision == 'bf16x3'
    assert parse_args(['train', '--lstm-precision', 'fp32']).lstm_precision == 'fp32'
    with pytest.raises(SystemExit):
        parse_args(['train', '--lstm-precision', 'fp16'])


def test_bf16x3_kernels_do_not_spill():
    """Every bf16x3 instantiation of lstm_step_x_kernel (PREC = 1): no scratch, <= 256 VGPRs, an occupancy no lower than its
    fp32 twin's."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import resource_usage
    rows = resource_usage.usage(os.path.join(ROOT, 'deeprl_network_amd', 'csrc', 'lstm_mfma.hip'))
    step = {r['name']: r for r in rows if r['name'].startswith('lstm_step_x_kernel<')}
    x3 = {n: r for n, r in step.items() if n.endswith(', 1>')}
    assert len(x3) == 6, sorted(step)
    for n, r in x3.items():
        assert r['ScratchSize [bytes/lane]'] == 0 and r['VGPRs'] + r.get('AGPRs', 0) <= 256, (n, r)
        twin = step[n[:-len(', 1>')] + ', 0>']
        assert r['Occupancy [waves/SIMD]'] >= twin['Occupancy [waves/SIMD]'], (n, r, twin)

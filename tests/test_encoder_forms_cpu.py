"""tests/encoder_form_checks.py on the CPU, the ops and the env replaced by their restatements (cpu_emulation): the host side of the
input encoders' forms -- which layers each form names, on which tensors, into which columns -- for every policy class."""
import numpy as np
import pytest

import encoder_form_checks as efc
from cpu_emulation import CpuCaccBatchEnv, cpu_ops
from helpers import cacc_config

T, E = efc.T, efc.E


def build(agent):
    """test_trainer_cpu.build's trainer at n_step = T (its episode of 30 steps is 15 batches then)."""
    from deeprl_network_amd.agents import models
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    cp = cacc_config(agent=agent, n_step=T, scenario='catchup', seed=12, reward_norm=800.0)
    cp['ENV_CONFIG']['episode_length_sec'] = '3'
    env = CpuCaccBatchEnv(cp['ENV_CONFIG'], num_envs=E)
    cls = {'ia2c': models.IA2C, 'ia2c_fp': models.IA2C_FP, 'ma2c_nc': models.MA2C_NC, 'ma2c_ic3': models.MA2C_IC3,
           'ma2c_cu': models.IA2C_CU, 'ma2c_dial': models.MA2C_DIAL}[agent]
    np.random.seed(12)
    model = cls(env.n_s_ls, env.n_a_ls, env.neighbor_mask, env.distance_mask, env.coop_gamma, 10 ** 6, cp['MODEL_CONFIG'], seed=12,
                num_envs=E, device='cpu')
    return env, model, BatchedTrainer(env, model, Counter(10 ** 6, 10 ** 7, 10 ** 4), use_graph=False)


ROLLOUT = [(c, lay) for c in efc.CASES for lay in efc.layouts(c)]


@pytest.mark.parametrize('case,layout', ROLLOUT, ids=['%s-%s' % (efc.case_id(c), lay) for c, lay in ROLLOUT])
def test_rollout_form_agrees_with_unroll(case, layout):
    from deeprl_network_amd import ops
    with cpu_ops():
        efc.check_rollout_against_unroll(ops, case, layout, 'cpu')


@pytest.mark.parametrize('case', efc.DESCRIPTION_CASES, ids=[efc.case_id(c) for c in efc.DESCRIPTION_CASES])
def test_kernel_descriptions_name_the_host_forms_tensors(case):
    from deeprl_network_amd import ops
    with cpu_ops():
        efc.check_descriptions(ops, case, 'cpu')


# (agent, environment switches, the batch has a sign image, CommNet's ENC slots)
SAVED = [('ia2c', {}, False, False), ('ia2c_fp', {}, True, False), ('ia2c_fp', {'NMARL_FC_BWD_PAIR': '0'}, False, False),
         ('ma2c_cu', {}, False, False), ('ma2c_nc', {}, True, False), ('ma2c_nc', {'NMARL_FC_BWD_PAIR': '0'}, False, False),
         ('ma2c_ic3', {}, False, True), ('ma2c_dial', {}, False, False)]


@pytest.mark.parametrize('agent,switches,bits,enc_slots', SAVED, ids=['%s%s' % (c[0], '-no-sign-image' if c[1] else '') for c in SAVED])
def test_saved_activations_give_the_gradients_of_unroll(agent, switches, bits, enc_slots, monkeypatch):
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    with cpu_ops():
        env, model, tr = build(agent)
        efc.check_saved_against_recomputed(model, tr, bits, enc_slots)

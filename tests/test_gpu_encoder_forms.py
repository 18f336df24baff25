"""tests/encoder_form_checks.py on the device: the encoders' forms on the fc kernels (one launch, a launch per layer, the plain GEMMs
past their widths), and the update's backward over what the lock-step kernels saved -- the sign image included, and on the 5 x 5
grid CommNet's ENC slots as the one-launch step with the observation encoder inside fills them."""
import pytest
import torch

import encoder_form_checks as efc
from test_gpu_trainer import build

pytestmark = pytest.mark.gpu

T, E = efc.T, efc.E
ROLLOUT = [(c, lay) for c in efc.CASES for lay in efc.layouts(c)]


@pytest.mark.parametrize('case,layout', ROLLOUT, ids=['%s-%s' % (efc.case_id(c), lay) for c, lay in ROLLOUT])
def test_rollout_form_agrees_with_unroll(case, layout):
    from deeprl_network_amd import ops
    efc.check_rollout_against_unroll(ops, case, layout, 'cuda:0')
    torch.cuda.synchronize()


@pytest.mark.parametrize('case', efc.DESCRIPTION_CASES, ids=[efc.case_id(c) for c in efc.DESCRIPTION_CASES])
def test_kernel_descriptions_name_the_host_forms_tensors(case):
    from deeprl_network_amd import ops
    efc.check_descriptions(ops, case, 'cuda:0')


# (agent, scenario, environment switches, the batch has a sign image, CommNet's ENC slots)
SAVED = [('ia2c', 'catchup', {}, False, False), ('ia2c_fp', 'catchup', {}, True, False),
         ('ia2c_fp', 'catchup', {'NMARL_FC_BWD_PAIR': '0'}, False, False), ('ma2c_cu', 'catchup', {}, False, False),
         ('ma2c_nc', 'catchup', {}, True, False), ('ma2c_nc', 'catchup', {'NMARL_FC_BWD_PAIR': '0'}, False, False),
         ('ma2c_nc', 'grid', {}, False, False), ('ma2c_ic3', 'catchup', {}, False, True), ('ma2c_ic3', 'grid', {}, False, True),
         ('ma2c_dial', 'catchup', {}, False, False)]


@pytest.mark.parametrize('agent,scenario,switches,bits,enc_slots', SAVED,
                         ids=['%s-%s%s' % (c[0], c[1], '-no-sign-image' if c[2] else '') for c in SAVED])
def test_saved_activations_give_the_gradients_of_unroll(agent, scenario, switches, bits, enc_slots, monkeypatch):
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    env, model, tr = build(agent, E, False, scenario=scenario, n_step=T, episode_sec=None if scenario == 'grid' else 3)
    efc.check_saved_against_recomputed(model, tr, bits, enc_slots)
    torch.cuda.synchronize()
    assert tr.handoff_fallbacks == 0

"""tests/lock_step_form_checks.py on the device: the forms that exist only there -- the env kernel's fused encode, the CACC env step
inside the lock-step launch, the grid env as a role of CommNet's launch (E = 130: two blocks per agent) -- beside the ones the CPU
runner has, and the per-batch flags a captured rollout and a captured update must leave as an eager batch does."""
import pytest
import torch

import lock_step_form_checks as lsf
from test_gpu_trainer import build

pytestmark = pytest.mark.gpu

T, E = lsf.T, lsf.E
# (id, agent, scenario, replicas, environment switches, the form `expected` is asked for, the trainer's (enc_in_kernel, env_in_kernel,
# fused_encode), the flags the update finds)
CASES = [
    ('both-encoders-and-env-inside-fp', 'ia2c_fp', 'catchup', E, {}, dict(enc='both', bits=True, env_in=True), (True, True, False), (False, False, T)),
    ('both-encoders-inside-fp', 'ia2c_fp', 'catchup', E, {'NMARL_INKERNEL_ENV': '0'}, dict(enc='both', bits=True), (True, False, False), (False, False, T)),
    ('fused-encode-fp', 'ia2c_fp', 'catchup', E, {'NMARL_INKERNEL_ENCODE': '0'}, dict(enc='pre'), (False, False, True), (False, False, 0)),
    ('enc-spec-nc', 'ma2c_nc', 'catchup', E, {}, dict(enc='both', bits=True, carry=True), (True, False, False), (False, False, T)),
    ('enc-spec-and-env-inside-nc', 'ma2c_nc', 'catchup', E, {'NMARL_NC_ENV_IN_KERNEL': '1'}, dict(enc='both', bits=True, carry=True, env_in=True),
     (True, True, False), (False, False, T)),
    ('fused-encode-nc', 'ma2c_nc', 'catchup', E, {'NMARL_NC_ONE_LAUNCH': '0'}, dict(enc='pre', carry=True), (False, False, True), (False, False, 0)),
    ('two-launches-nc', 'ma2c_nc', 'catchup', E, {'NMARL_INKERNEL_HANDOFF': '0'}, dict(enc='pre', launches=2), (False, False, True), (False, False, 0)),
    ('two-launches-dial', 'ma2c_dial', 'catchup', E, {}, dict(launches=2), (False, False, False), (False, False, 0)),
    ('ob-encoder-ic3-grid', 'ma2c_ic3', 'grid', E, {'NMARL_GRID_ENV_IN_KERNEL': '0'}, dict(enc='ob', carry=True), (False, False, False), (True, True, 0)),
    ('grid-env-role-ic3', 'ma2c_ic3', 'grid', E, {}, dict(enc='ob', carry=True, env_in=True), (False, True, False), (True, True, 0)),
    ('grid-env-role-ic3-two-blocks', 'ma2c_ic3', 'grid', 130, {}, dict(enc='ob', carry=True, env_in=True), (False, True, False), (True, True, 0)),
]


def _trainer(monkeypatch, agent, scenario, replicas, switches, use_graph=False):
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    return build(agent, replicas, use_graph, scenario=scenario, n_step=T, episode_sec=None if scenario == 'grid' else 3)


@pytest.mark.parametrize('name,agent,scenario,replicas,switches,form,trainer_form,flags', CASES, ids=[c[0] for c in CASES])
def test_one_batch_launches_the_form(name, agent, scenario, replicas, switches, form, trainer_form, flags, monkeypatch):
    from deeprl_network_amd import ops
    env, model, tr = _trainer(monkeypatch, agent, scenario, replicas, switches)
    if form.get('env_in') and scenario == 'grid' and not env.inkernel_step_supported():
        pytest.skip('the grid is not resident beside the LSTM blocks on this device')
    assert (bool(tr.enc_in_kernel), bool(tr.env_in_kernel), bool(tr.fused_encode)) == trainer_form
    assert lsf.check_batch(ops, model, env, tr, lsf.NETS[agent], **form) == flags
    torch.cuda.synchronize()
    assert tr.handoff_fallbacks == 0


@pytest.mark.parametrize('agent,scenario', [('ia2c_fp', 'catchup'), ('ma2c_nc', 'catchup'), ('ma2c_ic3', 'grid')])
def test_captured_batches_leave_the_flags_of_an_eager_batch(agent, scenario, monkeypatch):
    """A replayed rollout runs no Python and capturing the update runs it without a batch: after either, the flags read through
    policy.rollout_saved() are what an eager batch leaves at the same point."""
    found = {}
    for use_graph in (False, True):
        env, model, tr = _trainer(monkeypatch, agent, scenario, E, {}, use_graph=use_graph)
        seen = found[use_graph] = []
        rollout, update_end = tr.rollout, model.update_end

        def after_rollout(rollout=rollout, model=model, seen=seen):
            rollout()
            seen.append(('rollout', model.policy.rollout_saved()))

        def before_update_end(update_end=update_end, model=model, seen=seen):
            seen.append(('update', model.policy.rollout_saved()))            # (update_end clears them: the batch is consumed)
            update_end()

        tr.rollout, model.update_end = after_rollout, before_update_end
        for _ in range(3):                       # (the update is captured in the second batch and replayed in the third)
            tr.run_batch()
        torch.cuda.synchronize()
        assert model.policy.rollout_saved() == (False, False, 0) and len(seen) == 6
        if use_graph:
            assert tr.graph is not None and tr._upd is not None, tr.update_capture_error
    assert found[True] == found[False] and all(flags != (False, False, 0) for _, flags in found[False])

"""tests/lock_step_form_checks.py on the CPU, the ops and the env replaced by their restatements (cpu_emulation): every form of a
lock-step the host code can take without a device -- which launches one batch issues, in which order, on which buffer slots, with
which keys of the message description -- and the carry's invalidation with the state it describes."""
import numpy as np
import pytest

import lock_step_form_checks as lsf
from cpu_emulation import CpuCaccBatchEnv, cpu_ops
from helpers import cacc_config
from test_trainer_cpu import _Cpu8FeatureEnv

T, E = lsf.T, lsf.E


def build(agent, env_cls=CpuCaccBatchEnv, **trainer_kw):
    """test_trainer_cpu.build's trainer at n_step = 3 (its episode of 30 steps is 10 batches then), with the trainer's switches."""
    from deeprl_network_amd.agents import models
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    cp = cacc_config(agent=agent, n_step=T, scenario='catchup', seed=12, reward_norm=800.0)
    cp['ENV_CONFIG']['episode_length_sec'] = '3'
    env = env_cls(cp['ENV_CONFIG'], num_envs=E)
    cls = {'ia2c': models.IA2C, 'ia2c_fp': models.IA2C_FP, 'ma2c_nc': models.MA2C_NC, 'ma2c_ic3': models.MA2C_IC3,
           'ma2c_cu': models.IA2C_CU, 'ma2c_dial': models.MA2C_DIAL}[agent]
    np.random.seed(12)
    model = cls(env.n_s_ls, env.n_a_ls, env.neighbor_mask, env.distance_mask, env.coop_gamma, 10 ** 6, cp['MODEL_CONFIG'], seed=12,
                num_envs=E, device='cpu')
    return env, model, BatchedTrainer(env, model, Counter(10 ** 6, 10 ** 7, 10 ** 4), use_graph=False, **trainer_kw)


UNSAVED = dict(save_activations=False)
WIDE = dict(compact_obs=False)          # the env's gathered observation: an encoder launch per lock-step
# (id, agent, trainer switches, environment switches, env class, the form `expected` is asked for, the flags the update finds)
CASES = [
    ('unsaved-fused-ia2c', 'ia2c', UNSAVED, {}, None, dict(saved=False), (False, False, 0)),
    ('unsaved-fused-fp', 'ia2c_fp', UNSAVED, {}, None, dict(saved=False), (False, False, 0)),
    ('unsaved-fused-cu', 'ma2c_cu', UNSAVED, {}, None, dict(saved=False), (False, False, 0)),
    ('unsaved-pair-nc', 'ma2c_nc', UNSAVED, {}, None, dict(saved=False, launches=2), (False, False, 0)),
    ('unsaved-pair-dial', 'ma2c_dial', UNSAVED, {}, None, dict(saved=False, launches=2), (False, False, 0)),
    ('saved-both-encoders-fp', 'ia2c_fp', {}, {}, None, dict(enc='both', bits=True), (False, False, T)),
    ('saved-both-encoders-fp-no-sign-image', 'ia2c_fp', {}, {'NMARL_FC_BWD_PAIR': '0'}, None, dict(enc='both'), (False, False, 0)),
    ('saved-one-encoder-ia2c', 'ia2c', {}, {}, None, dict(enc='both'), (False, False, 0)),
    ('saved-one-encoder-cu', 'ma2c_cu', {}, {}, None, dict(enc='both'), (False, False, 0)),
    ('saved-encoder-launch-fp', 'ia2c_fp', WIDE, {}, None, dict(), (False, False, 0)),
    ('saved-encoder-launch-nc', 'ma2c_nc', WIDE, {}, None, dict(carry=True), (False, False, 0)),
    ('saved-encoder-launch-ic3', 'ma2c_ic3', WIDE, {}, None, dict(carry=True), (True, True, 0)),
    ('saved-carry-nc-enc-spec', 'ma2c_nc', {}, {}, None, dict(enc='both', bits=True, carry=True), (False, False, T)),
    ('saved-carry-ic3-encoder-launch', 'ma2c_ic3', {}, {}, None, dict(carry=True), (True, True, 0)),
    ('saved-carry-ic3-ob-encoder', 'ma2c_ic3', {}, {}, _Cpu8FeatureEnv, dict(enc='ob', carry=True), (True, True, 0)),
    ('saved-no-carry-nc', 'ma2c_nc', {}, {'NMARL_MSG_CARRY': '0'}, None, dict(enc='both', bits=True), (False, False, T)),
    ('saved-no-carry-ic3', 'ma2c_ic3', {}, {'NMARL_MSG_CARRY': '0'}, _Cpu8FeatureEnv, dict(enc='ob'), (True, True, 0)),
    ('saved-two-launches-nc', 'ma2c_nc', {}, {'NMARL_INKERNEL_HANDOFF': '0'}, None, dict(launches=2), (False, False, 0)),
    ('saved-two-launches-ic3', 'ma2c_ic3', {}, {'NMARL_INKERNEL_HANDOFF': '0'}, None, dict(launches=2), (True, True, 0)),
    ('saved-two-launches-dial', 'ma2c_dial', {}, {}, None, dict(launches=2), (False, False, 0)),
]
IDS = [c[0] for c in CASES]


def _trainer(monkeypatch, agent, kw, switches, env_cls):
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    return build(agent, **({} if env_cls is None else {'env_cls': env_cls}), **kw)


@pytest.mark.parametrize('name,agent,kw,switches,env_cls,form,flags', CASES, ids=IDS)
def test_one_batch_launches_the_form(name, agent, kw, switches, env_cls, form, flags, monkeypatch):
    """The whole sequence is the assertion of the form: one launch or two (the entries), the encoders inside (the keys of their
    description), the carry and the sign image (theirs) -- and what the update is told the rollout saved."""
    from deeprl_network_amd import ops
    with cpu_ops():
        env, model, tr = _trainer(monkeypatch, agent, kw, switches, env_cls)
        assert model.save_acts == form.get('saved', True) and model.compact_obs == ('compact_obs' not in kw)
        assert lsf.check_batch(ops, model, env, tr, lsf.NETS[agent], **form) == flags


@pytest.mark.parametrize('name,agent,kw,switches,env_cls,form,flags', CASES, ids=IDS)
def test_form_record_says_what_is_launched(name, agent, kw, switches, env_cls, form, flags, monkeypatch):
    """models.lock_step_form(): the one description `_lock_step`, `update_grads` and the trainer read, against the same table."""
    with cpu_ops():
        env, model, tr = _trainer(monkeypatch, agent, kw, switches, env_cls)
        model.policy.refresh_wimage()            # (a coupled net's one-launch form exists once its message image does: lock-step 0)
        enc = form.get('enc', 'launch')
        f = model.lock_step_form()
        assert (f.launches, f.encoders, f.carry, f.sign_image) == (form.get('launches', 1), 'none' if enc == 'launch' else enc,
                                                                   form.get('carry', False), form.get('bits', False))
        assert not (tr.enc_in_kernel or tr.env_in_kernel or tr.fused_encode)     # the trainer's forms need the device


# ------------------------------------------------------------------------------------------------------ the carry and its state
def _carry_spy(monkeypatch, model):
    seen = []

    def spy(self, t, orig=type(model)._msg_carry):
        d = orig(self, t)
        seen.append((t, d is not None and d.get('carry_in') is not None))
        return d

    monkeypatch.setattr(type(model), '_msg_carry', spy)
    return seen


def _act(model, tr, t):
    model.t = t
    model.act(tr.done_pre if t == 0 else tr.zero_done, seed=12, step=t, step_dev=tr.step_dev, done_is_zero=t > 0)


@pytest.mark.parametrize('agent', ['ma2c_nc', 'ma2c_ic3'])
@pytest.mark.parametrize('writer', ['reset_states', 'reset_states-masked', 'trainer-restore'])
def test_state_written_out_of_band_ends_the_carry(agent, writer, monkeypatch):
    """Lock-steps 0 and 1 hand their message term on; then the recurrent state is written behind the lock-steps' back; lock-step 2
    must compute its own (include/nmarl.h: carry_in = NULL after such a write) -- whatever order the caller keeps."""
    import torch
    with cpu_ops():
        env, model, tr = build(agent)
        seen = _carry_spy(monkeypatch, model)
        env.state_tensors = lambda: []           # (the restated env keeps its state on the host: the snapshot is the model's part)
        snap = tr._snapshot()
        _act(model, tr, 0)
        _act(model, tr, 1)
        assert seen == [(0, False), (1, True)]
        model.t = 2
        if writer == 'trainer-restore':
            tr._restore(snap)
        else:
            model.reset_states(mask=None if writer == 'reset_states' else torch.tensor([1.0, 0.0, 1.0]))
        _act(model, tr, 2)
        assert seen[2] == (2, False), 'lock-step 2 started from the message term of a state that is gone'

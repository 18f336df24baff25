"""IA2C / MA2C algorithm classes on MI355X -- the reference's `agents.models` surface
(models.py:15-309) over a batched, device-resident engine.

Each class keeps the reference's constructor and methods
    forward / add_transition / backward / reset / save / load
with the reference's E = 1, NumPy-in / NumPy-out semantics (so the reference's
Trainer and tests drive it unchanged), and adds the batched API the MI355X
Trainer uses for E >> 1 replicas with everything resident in HBM:
    act()  record()  bootstrap()  update()  reset_states()

Engine (per n_step batch, E replicas, N agents):
  rollout   2 recurrent steps per lock-step, reproducing the reference's quirk Q1
            (utils.py:129-151 + policies.py:119-134: `forward('v')` re-steps the LSTM
            from the state `forward('p')` just wrote);
  buffers   [T,...] device tensors replacing OnPolicyBuffer's Python lists
            (agents/utils.py:722-761, 819-835);
  update    rewards / reward_norm, clamped (opt-in reward_scale = return: nmarl_reward_scale, rewards over the running std of the
            discounted return) -> nmarl_nstep_return (opt-in gae_lambda < 1: nmarl_gae_return) [-> opt-in adv_norm: nmarl_standardize, the policy term's
            advantage per agent / over all agents to zero mean and unit std] -> autograd unroll -> A2C loss (policies.py:20-30,
            232-255; means over T*E, sum over agents) -> [RCCL all-reduce] ->
            nmarl_rmsprop_tf_clip (policies.py:32-39; opt-in optimizer = adam: nmarl_adam_clip)
            [-> opt-in ppo_epochs = K > 1: K - 1 more steps on the same batch, each the forward pass recomputed -> clipped surrogate
            against the behaviour policy's log-probabilities (nmarl_ppo_logp, nmarl_ppo_loss_*) -> all-reduce -> optimiser;
            opt-in ppo_vclip: the value term of those steps clipped around the behaviour critic's values (nmarl_ppo_loss_vclip_*);
            opt-in ppo_target_kl: the steps behind the first epoch whose pooled approx_kl exceeds it change nothing, decided on
            the device (nmarl_ppo_kl_sum -> all-reduce -> nmarl_ppo_kl_gate -> the optimiser's status word);
            opt-in ppo_minibatches = M > 1: every epoch k >= 2 permutes the replicas on the device (nmarl_minibatch_perm) and makes
            M such steps, each on the gathered rows of E / M whole sequences (nmarl_minibatch_gather)].
"""
import functools
import logging
import os

import numpy as np
import torch

from .. import ops, train_record
from .policies import (ConsensusPolicy, DIALMultiAgentPolicy, FPPolicy, IC3MultiAgentPolicy, LstmPolicy,
                       NCMultiAgentPolicy)
from .utils import Scheduler

F32 = torch.float32


class LockStepForm:
    """How a lock-step of `model` is launched (IA2C.lock_step_form).  Made anew per lock-step and per update, each field evaluated from the
    switches when it is read: a reader pays only for the predicates it asks (the eager rollout's host time; `encoders` is asked for thrice)."""
    def __init__(self, model):
        self.m, self.p = model, model.policy

    # 1: policy step and value re-step in one kernel (without saved activations a coupled net takes the pair); else 2
    launches = property(lambda f: 1 if (f.p.pv_one_launch(f.m.E) if f.m.save_acts else f.p.fused_pv) else 2)
    # the input encoders inside that launch: 'both', 'ob' (the observation encoder) or 'none'
    encoders = functools.cached_property(lambda f: 'none' if not f.m.save_acts else 'both' if f.p.enc_in_kernel(f.m.E, f.m.compact_obs) else
                                         'ob' if f.p.encodes_in_step(f.m.E, f.m.compact_obs) else 'none')
    # the re-step's message term goes on to the next lock-step's policy step (`_msg_carry`)
    carry = property(lambda f: bool(f.m.save_acts and f.launches == 1 and f.m._carries_msg()))
    # the launch writes the sign image of its encoders' output (`_relu_bits`)
    sign_image = property(lambda f: f.encoders == 'both' and f.p.enc_writes_bits and os.environ.get('NMARL_FC_BWD_PAIR', '1') != '0')


# Readers of the optional MODEL_CONFIG keys (absent: the default, so every reference ini runs unchanged)
def _cfg_choice(model_config, key, default, choices):
    value = model_config.get(key, fallback=default).strip().lower()
    if value not in choices:
        raise ValueError('%s = %r: must be %s' % (key, value, ' or '.join([', '.join(choices[:-1]), choices[-1]])))
    return value


def _cfg_float(model_config, key, default, ok, must):
    """A float that satisfies `ok` (written so that nan fails it), or ValueError '<key> = <value>: <must>'."""
    value = model_config.getfloat(key, fallback=default)
    if not ok(value):
        raise ValueError('%s = %r: %s' % (key, value, must))
    return value


def _cfg_positive(model_config, key):
    """An optional finite float > 0 (None: absent)."""
    raw = model_config.get(key, fallback=None)
    if raw is None:
        return None
    try:
        value = float(raw)
    except ValueError:
        value = float('nan')
    if not 0.0 < value < float('inf'):                   # (nan fails both comparisons)
        raise ValueError('%s = %r: must be finite and > 0' % (key, raw))
    return value


class IA2C:
    """Independent A2C with per-agent optimisers (models.py:15-158)."""

    policy_cls = LstmPolicy
    per_agent_optimizer = True       # IA2C: one RMSProp + one clip norm per agent (models.py:148-152)
    uses_fingerprint = False         # forward() receives neighbour policies `ps` (MA2C family)

    def __init__(self, n_s_ls, n_a_ls, neighbor_mask, distance_mask, coop_gamma, total_step, model_config,
                 seed=0, num_envs=1, device='cuda', dist_group=None, n_feat=None, n_feat_ls=None, obs_order=None):
        """The reference's constructor (models.py:20-24) + batching arguments.  obs_order (IA2C family): the env's
        `neighbor_order`, see BatchedPolicy.  n_feat_ls: per-agent OWN observation
        widths of heterogeneous systems (agents with different action counts, `identical_agent = False`,
        models.py:89-96).  MA2C envs report them as n_s_ls; the IA2C family's n_s_ls are the concatenated widths, from
        which the own widths are recovered when the system (I + neighbor_mask) x = n_s_ls determines them."""
        self.name = getattr(self, 'name', 'ia2c')
        self._init_algo(n_s_ls, n_a_ls, neighbor_mask, distance_mask, coop_gamma, total_step, seed,
                        model_config, num_envs, device, dist_group, n_feat, n_feat_ls, obs_order)

    # ------------------------------------------------------------------ construction
    def _init_algo(self, n_s_ls, n_a_ls, neighbor_mask, distance_mask, coop_gamma, total_step, seed,
                   model_config, num_envs, device, dist_group, n_feat, n_feat_ls=None, obs_order=None):
        self.n_s_ls, self.n_a_ls = [int(x) for x in n_s_ls], [int(x) for x in n_a_ls]
        self.n_a = max(self.n_a_ls)
        self.neighbor_mask = np.asarray(neighbor_mask)
        self.distance_mask = np.asarray(distance_mask)
        self.n_agent = len(self.neighbor_mask)
        self.identical_agent = max(self.n_a_ls) == min(self.n_a_ls)          # models.py:89-96
        # agents with equal action counts and UNEQUAL own observation widths (a network read from a file whose nodes all have,
        # say, two phases over different numbers of links; the reference's own networks have none): the reference's criterion
        # would build identical nets of agent 0's width.  They run as the padded heterogeneous network, like Monaco
        own = n_feat_ls if n_feat_ls is not None else (self.n_s_ls if self.name.startswith('ma2c') else None)
        if self.identical_agent and own is not None and max(own) != min(own):
            self.identical_agent = False
        self.n_feat_ls = None
        if not self.identical_agent:
            self.n_feat_ls = self._own_widths(n_feat_ls)
            n_feat = max(self.n_feat_ls)
        self.coop_gamma = float(coop_gamma)
        self.reward_clip = model_config.getfloat('reward_clip')
        self.reward_norm = model_config.getfloat('reward_norm')
        self.n_step = model_config.getint('batch_size')
        self.n_fc = model_config.getint('num_fc')
        self.n_lstm = model_config.getint('num_lstm')
        # optional (absent: 'fp32', so every reference ini runs unchanged): the rollout's LSTM product arithmetic, see
        # BatchedPolicy -- 'bf16x3' is opt-in and exists for the x-side uncoupled nets only
        self.lstm_precision = ops.check_precision(model_config.get('lstm_precision', fallback='fp32').strip(), 'lstm_precision')
        # optional (absent: 1.0 = the reference's plain n-step advantage, ops.nstep_return): lambda of GAE -- any other value in
        # [0, 1] sends the update's return scan through ops.gae_return (R becomes the lambda-return)
        self.gae_lambda = _cfg_float(model_config, 'gae_lambda', 1.0, lambda x: 0.0 <= x <= 1.0, 'must lie in [0, 1]')
        # optional (absent: 'rmsprop' = the reference's clip + TF-1.12 RMSProp, ops.rmsprop_tf_clip): 'adam' sends the optimiser
        # step through ops.adam_clip (the same clip, then bias-corrected Adam); rmsp_alpha / rmsp_epsilon are unused then
        self.optimizer = _cfg_choice(model_config, 'optimizer', 'rmsprop', ('rmsprop', 'adam'))
        self.adam_beta1 = _cfg_float(model_config, 'adam_beta1', 0.9, lambda x: 0.0 <= x < 1.0, 'must lie in [0, 1)')
        self.adam_beta2 = _cfg_float(model_config, 'adam_beta2', 0.999, lambda x: 0.0 <= x < 1.0, 'must lie in [0, 1)')
        self.adam_epsilon = _cfg_float(model_config, 'adam_epsilon', 1e-8, lambda x: x > 0.0, 'must be positive')
        # optional (absent: 'none' = the raw advantage in the policy-gradient term, as before): 'agent' standardises every agent's
        # T*E advantages of a batch to zero mean and unit std (each agent has its own critic), 'all' the N*T*E of all agents together
        # -- ops.standardize behind the return scan; the critic's target R is left alone
        self.adv_norm = _cfg_choice(model_config, 'adv_norm', 'none', ('none', 'agent', 'all'))
        self.adv_norm_epsilon = _cfg_float(model_config, 'adv_norm_epsilon', 1e-8, lambda x: x >= 0.0, 'must be >= 0')
        # optional (absent: 'none' = raw / reward_norm, as before): 'return' divides the rewards of a batch by the running standard
        # deviation of the discounted return over every sample seen so far (ops.reward_scale, in place of reward_norm)
        self.reward_scale = _cfg_choice(model_config, 'reward_scale', 'none', ('none', 'return'))
        self.reward_scale_epsilon = _cfg_float(model_config, 'reward_scale_epsilon', 1e-8, lambda x: x >= 0.0, 'must be >= 0')
        if self.reward_scale != 'none':
            logging.info('reward_scale = %s: rewards are divided by the running std of the discounted return; reward_norm = %r '
                         'is not applied' % (self.reward_scale, self.reward_norm))
        # optional (absent: 1 = one optimiser step per batch, as before): K > 1 makes K optimiser steps on every batch -- the first is the
        # A2C step as it is, epochs 2..K recompute the forward pass with the current weights and apply the clipped surrogate
        # (ops.ppo_loss) against the log-probabilities of the weights that produced the batch; ppo_clip is its epsilon
        raw = model_config.get('ppo_epochs', fallback='1').strip()
        try:
            self.ppo_epochs = int(raw)
        except ValueError:
            raise ValueError('ppo_epochs = %r: must be an integer >= 1' % raw)
        if self.ppo_epochs < 1:
            raise ValueError('ppo_epochs = %r: must be an integer >= 1' % raw)
        self.ppo_clip = _cfg_float(model_config, 'ppo_clip', 0.2, lambda x: 0.0 < x < float('inf'), 'must be finite and > 0')
        if self.ppo_epochs > 1:
            if self.policy_cls.coupled:
                # (as they refuse bf16x3) their in-launch hand-off guard and refused-batch rewind assume one optimiser step per batch
                raise ValueError('ppo_epochs = %d: not available for the coupled net %s (one optimiser step per batch)'
                                 % (self.ppo_epochs, self.policy_cls.name))
            if self.lstm_precision == 'bf16x3':
                raise ValueError('ppo_epochs = %d with lstm_precision = bf16x3: epochs >= 2 recompute the forward pass in fp32, the '
                                 'ratio would not start at 1' % self.ppo_epochs)
        # optional controls of epochs 2..K (absent: off, nothing allocated, the path of before).  ppo_vclip: the value loss clipped
        # around the critic's values under the weights that produced the batch (PPO2 form); ppo_target_kl: once the mean approx_kl of
        # an epoch exceeds it, the remaining optimiser steps of the update change nothing -- decided on the device
        self.ppo_vclip = _cfg_positive(model_config, 'ppo_vclip')
        self.ppo_target_kl = _cfg_positive(model_config, 'ppo_target_kl')
        for key in ('ppo_vclip', 'ppo_target_kl'):
            if getattr(self, key) is not None and self.ppo_epochs == 1:
                raise ValueError('%s = %r with ppo_epochs = 1: it acts on epochs 2..K only' % (key, model_config.get(key)))
        # optional (absent: 1 = every epoch is one full-batch step, as before): M > 1 splits the replicas of every epoch k >= 2 into M
        # groups of whole sequences along a permutation drawn on the device, one optimiser step per group
        raw = model_config.get('ppo_minibatches', fallback='1').strip()
        try:
            self.ppo_minibatches = int(raw)
        except ValueError:
            raise ValueError('ppo_minibatches = %r: must be an integer >= 1' % raw)
        if self.ppo_minibatches < 1:
            raise ValueError('ppo_minibatches = %r: must be an integer >= 1' % raw)
        if self.ppo_minibatches > 1:
            if self.ppo_epochs == 1:
                raise ValueError('ppo_minibatches = %d with ppo_epochs = 1: it splits epochs 2..K only' % self.ppo_minibatches)
            if self.ppo_minibatches > int(num_envs) or int(num_envs) % self.ppo_minibatches:
                raise ValueError('ppo_minibatches = %d does not divide the %d replica(s) of a rank into groups of whole sequences'
                                 % (self.ppo_minibatches, int(num_envs)))
        # test switch: M = 1 routed through the gather with the identity permutation (the plumbing must be lossless)
        self._mb_identity = self.ppo_minibatches == 1 and self.ppo_epochs > 1 and os.environ.get('NMARL_TEST_MINIBATCH_IDENTITY') == '1'
        self._mb_on = self.ppo_minibatches > 1 or self._mb_identity
        self.E = int(num_envs)
        self.device = torch.device(device)
        self.dist_group = dist_group
        self.world_size = 1
        if dist_group is not None:
            import torch.distributed as dist
            self.world_size = dist.get_world_size(dist_group)
        self.seed = seed
        m = self.neighbor_mask.sum(axis=1)
        if n_feat is None:
            # MA2C envs report the own-feature width; IA2C envs report n_feat*(1+m_i)
            n_feat = self.n_s_ls[0] if self._is_ma2c() else self.n_s_ls[0] // (1 + int(m[0]))
        self.n_feat = int(n_feat)
        self.policy = self.policy_cls(self.n_feat, self.n_a, self.neighbor_mask, n_fc=self.n_fc,
                                      n_h=self.n_lstm, device=self.device, n_feat_ls=self.n_feat_ls,
                                      n_a_ls=None if self.identical_agent else self.n_a_ls,
                                      obs_order=None if self._is_ma2c() else obs_order, precision=self.lstm_precision)
        if self.optimizer == 'adam':
            self.policy.params.enable_adam()
        self.policy.params.init_reference_order()       # consumes np.random like the reference's ortho_init
        self.n_s = self.n_s_ls[0]
        N, E, H, T = self.n_agent, self.E, self.n_lstm, self.n_step
        d = self.device
        z = lambda *s: torch.zeros(*s, dtype=F32, device=d)      # noqa: E731
        # recurrent state [c,h] of policies.py:151-154; static buffers (hipGraph-friendly), updated in place
        self.h_fw, self.c_fw, self.h_bw, self.c_bw = z(N, E, H), z(N, E, H), z(N, E, H), z(N, E, H)
        self._h2, self._c2 = z(N, E, H), z(N, E, H)        # scratch of the value re-step (quirk Q1)
        # a fresh episode's fingerprint: uniform over the agent's OWN actions (cacc_env.py:184, atsc_env.py:498-499)
        fp0 = np.zeros((N, 1, self.n_a), dtype=np.float32)
        for i in range(N):
            fp0[i, 0, :self.n_a_ls[i]] = 1.0 / self.n_a_ls[i]
        self.fp_uniform = torch.from_numpy(fp0).to(d)
        self._fp_eval = self.fp_uniform.expand(N, E, self.n_a).clone()
        self.t = 0
        self.total_step = total_step
        self.sess = None                                  # the reference Trainer reads model.sess (TF leak)
        if total_step:
            self._init_train(model_config, self.distance_mask, coop_gamma)

    def _is_ma2c(self):
        return self.name.startswith('ma2c')

    def _own_widths(self, n_feat_ls):
        """Own observation width of every agent of a heterogeneous system."""
        if n_feat_ls is not None:
            return [int(x) for x in n_feat_ls]
        if self._is_ma2c():
            return list(self.n_s_ls)                       # MA2C envs hand over the own features only
        a = np.eye(self.n_agent) + (self.neighbor_mask == 1)
        if abs(np.linalg.det(a)) < 1e-9:
            raise ValueError('heterogeneous IA2C: own observation widths are not determined by n_s_ls; pass n_feat_ls')
        x = np.linalg.solve(a, np.asarray(self.n_s_ls, dtype=np.float64))
        if np.abs(x - np.round(x)).max() > 1e-6 or x.min() < 1:
            raise ValueError('heterogeneous IA2C: n_s_ls is not a sum of own + neighbour widths; pass n_feat_ls')
        return [int(round(v)) for v in x]

    def _pad_policies(self, ps):
        """list of N probability vectors (ragged for heterogeneous agents, models.py:229-236) -> [N,1,A] f32."""
        out = np.zeros((self.n_agent, 1, self.n_a), dtype=np.float32)
        for i in range(self.n_agent):
            v = np.asarray(ps[i], dtype=np.float32).reshape(-1)
            out[i, 0, :len(v)] = v
        return torch.from_numpy(out).to(self.device)

    def _unpad_policies(self, pi):
        """[N,A] -> what the reference returns: an [N,A] array, or a list of ragged vectors (policies.py:314-316)."""
        if self.identical_agent:
            return pi
        return [pi[i, :self.n_a_ls[i]] for i in range(self.n_agent)]

    @property
    def fp(self):
        """Current fingerprints (previous-step policies) [N,E,A]: slot t of the rollout buffer while
        training, a standalone tensor for evaluation-only models (total_step = 0)."""
        return self.buf_fp[self.t] if self.total_step else self._fp_eval

    def _init_scheduler(self, model_config):
        lr_init = model_config.getfloat('lr_init')
        lr_decay = model_config.get('lr_decay')
        if lr_decay == 'constant':
            self.lr_scheduler = Scheduler(lr_init, decay=lr_decay)
        else:
            self.lr_scheduler = Scheduler(lr_init, model_config.getfloat('lr_min'), self.total_step, decay=lr_decay)

    def _init_train(self, model_config, distance_mask, coop_gamma):
        self._init_scheduler(model_config)
        self.v_coef = model_config.getfloat('value_coef')
        self.e_coef = model_config.getfloat('entropy_coef')
        self.max_grad_norm = model_config.getfloat('max_grad_norm')
        self.rmsp_alpha = model_config.getfloat('rmsp_alpha')
        self.rmsp_epsilon = model_config.getfloat('rmsp_epsilon')
        self.gamma = model_config.getfloat('gamma')
        N, E, T, d = self.n_agent, self.E, self.n_step, self.device
        p = self.policy
        # rollout buffers (replace OnPolicyBuffer's lists); every slot [t] is contiguous so kernels and
        # GEMMs write their results straight into it.  buf_x / buf_fp carry T+1 slots: slot t+1 receives
        # the observation / policy produced at lock-step t, slot T is the bootstrap input and becomes
        # slot 0 of the next batch.
        self.buf_x = torch.zeros(T + 1, E, N, p.n_obs, dtype=F32, device=d)
        self.buf_fp = self.fp_uniform.expand(T + 1, N, E, self.n_a).clone()
        self._pi_boot, self._v_boot = torch.zeros(N, E, self.n_a, dtype=F32, device=d), torch.zeros(N, E, dtype=F32, device=d)
        self.buf_act = torch.zeros(T, E, N, dtype=torch.uint8, device=d)
        self.buf_v = torch.zeros(T, N, E, dtype=F32, device=d)
        self.buf_done_pre = torch.zeros(T, E, dtype=F32, device=d)
        self.buf_done_post = torch.zeros(T, E, dtype=torch.uint8, device=d)
        spatial = self.coop_gamma >= 0
        self.buf_r = torch.zeros((T, E, N) if spatial else (T, E), dtype=F32, device=d)
        self.R = torch.zeros(N, T, E, dtype=F32, device=d)
        self.Adv = torch.zeros(N, T, E, dtype=F32, device=d)
        if self.adv_norm != 'none':
            # opt-in: the standardised advantage the policy-gradient term reads (Adv itself stays raw for every other reader), the
            # kernel's per-chunk moments and the (mean, std) of every group of the last update
            G = N if self.adv_norm == 'agent' else 1
            self.Adv_n = torch.zeros(N, T, E, dtype=F32, device=d)
            self._adv_partial = torch.zeros(G, ops.standardize_chunks(N * T * E // G, G), 3, dtype=torch.float64, device=d)
            self.adv_moments = torch.zeros(G, 2, dtype=torch.float64, device=d)
        if self.reward_scale != 'none':
            # opt-in: the discounted return carried across batches per reward stream, the pooled running moments, the kernel's
            # per-block moments, and the raw rewards of a batch of the one-replica path (`record` per step)
            S = self.buf_r[0].numel()
            self.rs_carry = torch.zeros(S, dtype=torch.float64, device=d)
            self.rs_state = torch.zeros(ops.REWARD_SCALE_STATE, dtype=torch.float64, device=d)
            self._rs_partial = torch.zeros(ops.reward_scale_chunks(S), 4, dtype=torch.float64, device=d)
            self._rs_raw = torch.zeros_like(self.buf_r)
            self._rs_pending = False
        if self.ppo_epochs > 1:
            # opt-in: the behaviour policy's log-probabilities of the actions taken (taken before the batch's first optimiser step)
            # and per epoch and agent (approx_kl, clip_frac) of the last update -- row 0, the A2C step, stays zero
            self.ppo_logp_old = torch.zeros(N, T * E, dtype=F32, device=d)
            self.ppo_stats = torch.zeros(self.ppo_epochs, N, 2, dtype=F32, device=d)
            if self.ppo_vclip is not None:
                # opt-in: the critic's values under the weights that produced the batch (taken with ppo_logp_old) and per epoch and
                # agent vclip_frac of the last update -- row 0 stays zero
                self.ppo_v_old = torch.zeros(N, T * E, dtype=F32, device=d)
                self.ppo_vclip_stats = torch.zeros(self.ppo_epochs, N, dtype=F32, device=d)
            if self.ppo_target_kl is not None:
                # opt-in: the KL stop's device words (ops.ppo_kl_gate: stop, steps refused, epochs applied, unused) and the values
                # every update starts them from
                self.ppo_gate = torch.tensor(ops.PPO_GATE_RESET, dtype=torch.int32, device=d)
                self._ppo_gate_reset = torch.tensor(ops.PPO_GATE_RESET, dtype=torch.int32, device=d)
                self._ppo_gate_pending = False
            if self._mb_on:
                # opt-in replica minibatches: the permutation of an epoch, its Philox keys, the count of updates made so far (what
                # the draw is keyed by, beside the epoch: advanced on the device once per update) and the dense operands of one
                # step -- every [.., E, ..] buffer of the update with E / M replicas in E's place (ops.minibatch_gather)
                Em, H = E // self.ppo_minibatches, self.n_lstm
                self.mb_env_id_base = 0              # (BatchedTrainer: the env's, so every rank permutes its shard with its own draws)
                self.mb_perm = torch.arange(E, dtype=torch.int32, device=d)
                self.mb_count = torch.zeros(1, dtype=torch.int32, device=d)
                self._mb = dict(keys=torch.zeros(E, dtype=torch.int32, device=d),
                                x=torch.zeros(T, Em, N, p.n_obs, dtype=F32, device=d), fp=torch.zeros(T, N, Em, self.n_a, dtype=F32, device=d),
                                act=torch.zeros(T, Em, N, dtype=torch.uint8, device=d), done=torch.zeros(T, Em, dtype=F32, device=d),
                                adv=torch.zeros(N, T * Em, dtype=F32, device=d), R=torch.zeros(N, T * Em, dtype=F32, device=d),
                                logp=torch.zeros(N, T * Em, dtype=F32, device=d), h=torch.zeros(N, Em, H, dtype=F32, device=d),
                                c=torch.zeros(N, Em, H, dtype=F32, device=d))
                if self.ppo_vclip is not None:
                    self._mb['v_old'] = torch.zeros(N, T * Em, dtype=F32, device=d)
        self.dist_dev =torch.from_numpy(self.distance_mask.astype(np.int32)).to(d)
        self.t = 0
        self.grad_norm = torch.zeros(N, dtype=F32, device=d)
        self.last_loss = None
        self._terms = None                # [N,3] terms tensor of the last update where a native loss produced one
        # steps whose pre-step done flag may be non-zero (None = any, the reference API); the batched trainer
        # sets (0,) because episodes start only at batch boundaries (quirk Q4)
        self.masked_steps = None
        self.save_acts = False

    def enable_saved_activations(self):
        """Batched engine, uncoupled nets: the rollout's policy steps ARE the forward pass of the update (on-policy
        A2C: same weights, same inputs, states_bw = the state the rollout started from), so the step kernel saves the
        LSTM inputs, gates and state sequences and update() runs the backward only.  The critic's neighbour-action
        term is added for all T lock-steps by one launch at update time.  Returns False if the policy cannot do it."""
        p = self.policy
        if not p.can_save_acts:
            return False
        N, E, T, H, d = self.n_agent, self.E, self.n_step, self.n_lstm, self.device
        KX = p.params[p.k_wx].shape[1]
        # one zero slab more than needed, so that [S | .] and the state sequences have the SAME (T + 1)-slab shape -- the
        # update's weight-gradient GEMMs then read the saved buffers in place (ops.seq_rows_pair / lstm_weight_grads)
        self.S_ext = torch.zeros(N, T + 1, E, KX, dtype=F32, device=d)
        self.S_buf = self.S_ext[:, :T]
        self.G_buf = torch.zeros(N, T, E, 4 * H, dtype=F32, device=d)
        self.H_all = torch.zeros(N, T + 1, E, H, dtype=F32, device=d)
        self.C_all = torch.zeros(N, T + 1, E, H, dtype=F32, device=d)
        self.buf_vn = torch.zeros(N, T, E, dtype=F32, device=d)          # agent-major values (critic's h part)
        # coupled nets: further per-step message terms the backward needs (policy.save_spec)
        # (`save_next` keys: one slab more -- the policy step of lock-step t fills slot t + 1, e.g. lstm_dial's message vectors)
        # (`save_pad` keys: one ZERO slab more, like S_ext -- the update's weight-gradient GEMM reads the (T + 1)-slab buffer in place)
        full = {k: torch.zeros(N, T + 1 if (k in p.save_next or k in p.save_pad) else T, E, w, dtype=F32, device=d) for k, w in p.save_spec().items()}
        p._extra = {k: v[:, :T] for k, v in full.items()}
        p._extra_full = full
        self.save_acts = True
        return True

    def enable_compact_obs(self):
        """Batched engine: the env writes compact observations [E,N,n_feat] (own features only); the rollout's encoder
        gathers the neighbours inside its kernels, forward (rollout) and backward (update)."""
        p = self.policy
        if p.hetero or p.n_obs == p.n_feat:
            return False
        if p.params[p.k_ob].shape[2] != ops.FC_J or p.n_obs > ops.FC_MAX_F:
            return False          # the gathering encoder kernel (nmarl_fc_fwd_multi) is 64 outputs wide, inputs <= 64
        T, E, N = self.n_step, self.E, self.n_agent
        self.buf_x = torch.zeros(T + 1, E, N, p.n_feat, dtype=F32, device=self.device)
        if self._mb_on:           # opt-in replica minibatches: the gathered slab follows the buffer it is gathered from
            self._mb['x'] = torch.zeros(T, E // self.ppo_minibatches, N, p.n_feat, dtype=F32, device=self.device)
        self.compact_obs = True
        return True

    compact_obs = False
    _enc_boot = None           # the bootstrap step's scratch LSTM input (encode_target)

    def _save_slots(self, t):
        """Slots of lock-step t in the saved activations, for the policy step of a coupled net."""
        p = self.policy
        d = {k: v[:, t] for k, v in p._extra.items()}
        d['S'] = self.S_buf[:, t]
        d.update({k + '_next': p._extra_full[k][:, t + 1] for k in p.save_next if k in p._extra_full})
        return d

    # ------------------------------------------------------------------ batched engine
    def reset_states(self, mask=None):
        """Policy._reset (policies.py:151-154, 334-336) for all replicas or those with mask != 0;
        also restores the uniform fingerprint of a fresh episode (cacc_env.py:184)."""
        self.invalidate_carried()
        if mask is None:
            for s in (self.h_fw, self.c_fw, self.h_bw, self.c_bw):
                s.zero_()
            self.fp.copy_(self.fp_uniform.expand_as(self.fp))
        else:
            keep = (mask == 0).to(F32).view(1, -1, 1)
            for s in (self.h_fw, self.c_fw, self.h_bw, self.c_bw):
                s.mul_(keep)
            self.fp.mul_(keep).add_((1.0 - keep) * self.fp_uniform)

    def invalidate_carried(self):
        """The recurrent state is written out of band (a reset, a restored snapshot, the batch hand-over's kernel): the next lock-step takes
        neither the carried message term (include/nmarl.h: carry_in = NULL after such a write) nor lstm_dial's cached message vectors."""
        self._carry_holds = -1
        self.policy.invalidate_cached_msg()

    def _policy_step(self, obs, done, done_is_zero=False):
        """forward('p'): advances states_fw (policies.py:119-134); returns the pi LOGITS' softmax."""
        self.policy.refresh_wimage()          # reference API: the weights may have changed since the last call
        self._enc = self.policy.encode(obs, self.fp)
        self.policy.step(self._enc, self.h_fw, self.c_fw, done, self.h_fw, self.c_fw, done_is_zero)
        with torch.no_grad():
            return self.policy.pi(self.h_fw)

    def _value_step(self, obs, done, na_onehot, done_is_zero=False, out=None, reuse_enc=False):
        """forward('v'): re-steps the LSTM from the state forward('p') wrote (quirk Q1), without
        storing the result (policies.py:124-133).  `reuse_enc`: obs / fingerprints are those of the
        preceding _policy_step, whose encoding is shared."""
        if not reuse_enc:
            self.policy.refresh_wimage()
        enc = self._enc if reuse_enc else self.policy.encode(obs, self.fp)
        self.policy.step(enc, self.h_fw, self.c_fw, done, self._h2, self._c2, done_is_zero, second=True)
        with torch.no_grad():
            return self.policy.value(self._h2, na_onehot, out=out)

    def encode_target(self, t):
        """Where lock-step t's LSTM input encoding lives when the env kernel produces it behind its step (fused encode):
        slot t of the saved activations, or a scratch buffer for the bootstrap step t = n_step (slab n_step of the saved
        inputs must stay zero: it pads the update's weight-gradient GEMMs)."""
        if t < self.n_step:
            return self.S_buf[:, t]
        if self._enc_boot is None:
            self._enc_boot = torch.zeros_like(self.S_buf[:, 0])
        return self._enc_boot

    def act(self, done, mode=ops.SAMPLE_PHILOX, u=None, seed=0, env_id_base=0, step=0, step_dev=None,
            done_is_zero=False, pre_encoded=False, env_step=None):
        """One lock-step decision for all replicas at buffer slot t: reads the observation buf_x[t]
        and fingerprints buf_fp[t]; writes the action into buf_act[t], the value into buf_v[t] and the
        new policy into buf_fp[t+1] (env.update_fingerprint, utils.py:173).  done [E] f32 is the pre-step
        flag.  Two kernels after the encoder when the heads fuse (H = 64).  Returns the action slot (input
        of the env kernel)."""
        return self._lock_step(self.t, done, dict(mode=mode, u=u, seed=seed, env_id_base=env_id_base, step=step, step_dev=step_dev),
                               done_is_zero, pre_encoded, env_step)[0]

    def bootstrap(self, done, action_scratch, mode=ops.SAMPLE_PHILOX, u=None, seed=0, env_id_base=0,
                  step=0, step_dev=None, done_is_zero=False, pre_encoded=False):
        """R for the unfinished replicas (utils.py:192-196) from buf_x[T] / buf_fp[T]: one more policy
        step (which advances states_fw -- quirk Q2) and the double-stepped value."""
        assert self.t == self.n_step
        return self._lock_step(self.n_step, done, dict(mode=mode, u=u, seed=seed, env_id_base=env_id_base, step=step, step_dev=step_dev),
                               done_is_zero, pre_encoded, None, act_out=action_scratch)[1]

    def lock_step_form(self):
        """The one description of a lock-step's launches: read by `_lock_step`, `update_grads` and BatchedTrainer (which adds the env's part)."""
        return LockStepForm(self)

    def _lstm_input(self, t, form, pre_encoded, env_step):
        """(enc, ob) of lock-step t.  enc: the LSTM input's h-independent part, shared by the policy step and the value re-step (Q1)
        -- or, with encoders inside the launch, the slot their output goes to.  ob: what those encoders read, else None."""
        p, boot, x = self.policy, t == self.n_step, self.buf_x[t]
        if pre_encoded:             # the env kernel of the previous lock-step already encoded buf_x[t] / fp[t] into its target
            return self.encode_target(t), None
        if form.encoders == 'both':
            # both encoders inside the launch, from the compact observation and the fingerprints of slot t (env_step: the CACC env step too).
            # Nothing of the bootstrap step is kept; a coupled net's encoders reach the K loop THROUGH the x slot, a scratch one there
            return (self.encode_target(t) if (p.coupled or not boot) else None), \
                dict(x=x, fp=self.fp, env=env_step, bits=self._relu_bits(t) if (form.sign_image and not boot) else None)
        slot = None
        if self.save_acts and not boot:
            slot = self.S_buf[:, t]
            if 'ENC' in p._extra:   # the encoder output is NOT the LSTM input itself (CommNet: s = enc + message term): kept per lock-step, so
                slot, p._enc_was_saved = p._extra['ENC'][:, t], True          # that the update's encoder backward needs no forward pass
        if form.encoders == 'ob':   # the observation encoder inside the launch, writing to `enc` (env_step: the grid env step as well)
            return (slot if slot is not None else self.encode_target(t)), dict(x=x, genv=env_step)
        return p.encode(x, self.fp, out=slot), None

    def _lock_step(self, t, done, draw, done_is_zero=False, pre_encoded=False, env_step=None, act_out=None):
        """Lock-step t = 0..n_step of a batch (t = n_step: the bootstrap step, whose action goes to the caller's scratch `act_out`):
        -> (action slot, value slot).  What varies with t is the table below; the launches are the same code."""
        p, T, saved = self.policy, self.n_step, self.save_acts
        if t == 0:
            p.refresh_wimage()                             # weights change between batches only (inside the hipGraph: one
            if saved:                                      # small node)
                self.H_all[:, 0].copy_(self.h_fw)
                self.C_all[:, 0].copy_(self.c_fw)
        form = self.lock_step_form()                       # (behind refresh_wimage: a coupled net's one-launch form needs its message image)
        one = form.launches == 1
        if env_step is not None and (pre_encoded or form.encoders == 'none'):
            raise ValueError('env_step needs the lock-step kernel that runs the input encoders itself (policy.enc_in_kernel / encodes_in_step)')
        enc, ob = self._lstm_input(t, form, pre_encoded, env_step)
        # saved activations: the policy step reads slot t of the state sequences; else the persistent state, advanced in place
        h, c = (self.H_all[:, t], self.C_all[:, t]) if saved else (self.h_fw, self.c_fw)
        if t < T:
            # ... and writes slot t + 1, gates into G[:, t]; in one launch the value (critic's h part) goes to the agent-major buffer, its
            # neighbour-action term is added in update().  Coupled nets: the POLICY step's message terms go to their save slots
            pi, act, v = self.buf_fp[t + 1], self.buf_act[t], (self.buf_vn[:, t] if (saved and one) else self.buf_v[t])
            h_out, c_out = (self.H_all[:, t + 1], self.C_all[:, t + 1]) if saved else (self.h_fw, self.c_fw)
            gates, save = (self.G_buf[:, t] if saved else None), (self._save_slots(t) if (saved and p.coupled) else None)
        else:
            # the bootstrap step: from slot T of the sequences into the persistent state; nothing of it is kept
            pi, act, v = self._pi_boot, act_out, self._v_boot
            h_out, c_out, gates, save = self.h_fw, self.c_fw, None, None
        if one:            # (without saved activations the fused step advances the state in place: no h_out / c_out)
            p.step_policy_value(enc, h, c, done, pi, act, v, h_out=h_out if saved else None, c_out=c_out if saved else None, gates=gates,
                                defer_action_term=saved and t < T, save=save, ob=ob,
                                carry=self._msg_carry(t) if (saved and p.coupled) else None, **draw)
        else:
            p.step_policy(enc, h, c, done, h_out, c_out, pi, act, done_is_zero, gates=gates, save=save, **draw)
            p.step_value(enc, h_out, c_out, done, self._h2, self._c2, act, v, done_is_zero)
        return act, v

    _carry_buf = None
    _carry_holds = -1          # the lock-step whose policy-step message term `_carry_buf` holds (written by the re-step of the one before)

    def _msg_carry(self, t):
        """Coupled nets, one-launch lock-step t (t = n_step: the bootstrap step): the re-step's message term -- computed from the
        neighbours' new, un-masked h (quirk Q3) -- IS lock-step t + 1's policy-step message term, so launch t leaves it in
        `_carry_buf` (and CommNet's mean rows in slot t + 1 of the saved means) and launch t + 1 starts from it: no neighbour rows,
        no product in front of its K loop.  Lock-step 0 computes its own (the batch boundary reset finished replicas' states)."""
        p = self.policy
        if not self._carries_msg():
            return None
        if self._carry_buf is None:
            self._carry_buf = torch.zeros(self.n_agent, self.E, self.n_lstm, dtype=F32, device=self.device)
        d = dict(carry_in=self._carry_buf if (t > 0 and self._carry_holds == t) else None,
                 carry_out=self._carry_buf if t < self.n_step else None)
        mm = p._extra_full.get('MM')
        if mm is not None and t + 1 < self.n_step and p.msg_kind == ops.MSG_MEAN_ADD:
            d['mean_next'] = mm[:, t + 1]
        self._carry_holds = t + 1 if t < self.n_step else -1
        return d

    def _carries_msg(self):
        """The one-launch lock-steps of this net hand the re-step's message term on (NMARL_MSG_CARRY=0: every step computes its own)."""
        return self.policy.msg_kind in (ops.MSG_GATHER_RELU, ops.MSG_MEAN_ADD) and os.environ.get('NMARL_MSG_CARRY', '1') != '0'

    S_bits = None

    def _relu_bits(self, t):
        """Slot t of the sign image of the saved LSTM inputs ([N,T,E,4] int32, ops.relu_bits_pack's layout): written by the lock-step kernel
        that runs the input encoders (`lock_step_form().sign_image`), read by the update's encoder backward instead of S itself."""
        if self.S_bits is None:
            self.S_bits = torch.zeros(self.n_agent, self.n_step, self.E, 4, dtype=torch.int32, device=self.device)
        self.policy._bits_steps = 1 if t == 0 else self.policy._bits_steps + 1
        return self.S_bits[:, t]

    def record(self, reward, done_post):
        """model.add_transition's reward path (models.py:26-32) for slot t: normalise, clip, store."""
        t = self.t
        if self.reward_scale != 'none':      # opt-in: keep the raw reward; update_grads scales the whole batch in front of the return scan
            self._rs_raw[t].copy_(reward)
            self._rs_pending = True
        else:
            self.buf_r[t].copy_(self._norm_reward(reward))
        self.buf_done_post[t].copy_(done_post)
        self.t = t + 1

    def _norm_reward(self, r):
        if self.reward_norm > 0:
            r = r / self.reward_norm
        if self.reward_clip > 0:
            r = torch.clamp(r, -self.reward_clip, self.reward_clip)
        return r

    def load_rewards(self, raw_rewards):
        """Batched path: the env kernel wrote raw rewards for all T slots (and done flags straight
        into buf_done_post); normalise them in one pass and mark the batch complete."""
        # (written in place: `buf_r.copy_(temporary)` is a memcpy node inside the captured update)
        if self.reward_scale != 'none':      # opt-in: the one native call in place of the division and the clamp
            self._scale_rewards(raw_rewards)
            self.t = self.n_step
            return
        if self.reward_norm > 0:
            torch.div(raw_rewards, self.reward_norm, out=self.buf_r)
        else:
            torch.mul(raw_rewards, 1.0, out=self.buf_r)
        if self.reward_clip > 0:
            self.buf_r.clamp_(-self.reward_clip, self.reward_clip)
        self.t = self.n_step

    def _scale_rewards(self, raw_rewards):
        """Opt-in reward_scale = return: advance the carried discounted returns and the pooled running moments by this batch's raw
        rewards and done flags, buf_r = raw / (running std + eps), clamped to reward_clip (reward_norm is not applied)."""
        ops.reward_scale(raw_rewards, self.buf_done_post, self.gamma, self.reward_scale_epsilon, max(self.reward_clip, 0.0),
                         self.rs_carry, self.rs_state, self._rs_partial, self.buf_r)
        self._rs_pending = False

    @property
    def reward_scale_std(self):
        """The running std of the discounted return the last update divided by (host read: synchronises); None with the key off."""
        return None if self.reward_scale == 'none' else float(self.rs_state[6])

    def _policy_adv(self):
        """The advantage of the policy-gradient term [N,T,E]: Adv, or under the opt-in adv_norm its standardised copy."""
        return self.Adv if self.adv_norm == 'none' else self.Adv_n

    def _loss_backward_fused(self, Hs):
        """`_loss(Hs).backward()` with the heads, the loss and the heads' backward as ONE pass over the h sequence
        (ops.heads_loss): this call is the root of the update's backward -- the head parameters receive their gradients here, the
        recurrence below Hs its dL/dh.  False: not available for this net (the caller takes the autograd chain)."""
        N, T, E = self.n_agent, self.n_step, self.E
        p = self.policy
        if Hs.dim() != 3 or not ops.heads_loss_supported(Hs, self.n_a, p.nbr_idx) or \
                (not self.identical_agent and not self.per_agent_optimizer) or Hs.stride(2) != 1 or Hs.stride(1) != Hs.shape[2]:
            return False
        prm = p.params
        action = self.buf_act.view(T * E, N)
        # the one-launch BPTT kernels take the heads' dL/dh as dy8 (32 bytes per row) and expand it themselves: no [N,T*E,64] tensor
        as_dy = self.save_acts and p.bptt_takes_head_dy and os.environ.get('NMARL_BPTT_HEAD_DY', '1') != '0'
        r = ops.heads_loss(Hs.detach(), prm['pi_w'], prm['pi_b'], prm['v_w'], prm['v_b'], action, p.nbr_idx, self.n_a,
                           self._policy_adv().view(N, T * E), self.R.view(N, T * E), self.v_coef, self.e_coef, want_dh=not as_dy)
        terms = self._terms = r['terms']
        self.last_loss = (terms[:, 0], terms[:, 1], terms[:, 2], terms.sum(dim=1))
        for k in ('pi_w', 'pi_b', 'v_w', 'v_b'):
            prm[k].grad = r[k].reshape(prm[k].shape)
        Hs.backward(gradient=ops.head_dy_placeholder(r['dy8'], r['hw'], Hs) if as_dy else r['dh'])
        if as_dy and ops._pending_head_dy.pop(Hs.device, None) is not None:
            raise RuntimeError('the recurrence below Hs did not take the heads\' dy8 (ops.take_head_dy): its gradient is wrong')
        return True

    def _loss(self, Hs):
        """policies.py:20-30 / 232-255 with the batch mean taken over T*E."""
        N, T, E = self.n_agent, self.n_step, self.E
        p = self.policy
        # the critic's neighbour one-hots (policies.py:66-68) are gathered from the action bytes inside the op
        action = self.buf_act.view(T * E, N)
        logits, v = p.heads(Hs, action)                                       # [N,T*E,A], [N,T*E]
        adv = self._loss_adv()
        R = self.R.view(N, T * E)
        if ops.a2c_loss_supported(self.n_a):
            per_agent, terms = ops.a2c_loss(logits, v, action, adv, R, self.v_coef, self.e_coef)
            self._terms = terms
            self.last_loss = (terms[:, 0], terms[:, 1], terms[:, 2], per_agent.detach())
            return per_agent.sum()
        per_agent, cols = self._loss_torch(logits, v, action, adv, R)
        self._terms = None
        self.last_loss = tuple(c.detach() for c in cols) + (per_agent.detach(),)
        return per_agent.sum()

    def _loss_torch(self, logits, v, action, adv, R, logp_old=None, v_old=None):
        """The loss where the native one does not reach (n_a > 8), in torch: -> per-agent total [N] (differentiable) and the terms as
        a list of [N] columns -- (policy, value, entropy) of the A2C loss; with logp_old the clipped surrogate of ops.ppo_loss and
        (approx_kl, clip_frac) behind the three; with v_old as well the clipped value term and vclip_frac, the sixth."""
        eps, vclip = self.ppo_clip, self.ppo_vclip
        pi = torch.softmax(logits, dim=-1)
        log_pi = torch.log(torch.clamp(pi, 1e-10, 1.0))
        entropy = -(pi * log_pi).sum(-1)
        logp_a = log_pi.gather(-1, action.t().long().unsqueeze(-1)).squeeze(-1)      # [N, T*E]
        if logp_old is None:
            policy_loss = -(logp_a * adv).mean(-1)                           # [N]
        else:
            dlp = logp_a - logp_old
            rho = torch.exp(dlp)
            policy_loss = -torch.min(rho * adv, torch.clamp(rho, 1.0 - eps, 1.0 + eps) * adv).mean(-1)
        if v_old is None:
            value_loss = (R - v).pow(2).mean(-1) * 0.5 * self.v_coef
        else:           # the clipped value loss; outside the clip range the gradient follows the larger of the two errors
            dvo = v - v_old
            inside = dvo.abs() <= vclip
            e1 = (R - v).pow(2)
            e2 = (R - (v_old + torch.clamp(dvo, -vclip, vclip))).pow(2).detach()
            value_loss = torch.where(inside | (e1 >= e2), e1, e2).mean(-1) * 0.5 * self.v_coef
        entropy_loss = -entropy.mean(-1) * self.e_coef
        per_agent = policy_loss + value_loss + entropy_loss
        cols = [policy_loss, value_loss, entropy_loss]
        if logp_old is not None:
            with torch.no_grad():
                cols += [(torch.expm1(dlp) - dlp).clamp_min(0.0).mean(-1), ((rho - 1.0).abs() > eps).to(F32).mean(-1)]
                if v_old is not None:
                    cols.append((dvo.abs() > vclip).to(F32).mean(-1))
        return per_agent, cols

    def loss_terms(self):
        """[N,3] contiguous (policy, value, entropy) loss terms of the last update: the `terms` tensor of ops.heads_loss /
        ops.a2c_loss itself on the two native paths (inside a captured update its address is the graph's), a stack on the
        torch path."""
        if self._terms is not None:
            return self._terms
        return torch.stack(self.last_loss[:3], dim=1).contiguous()

    def update(self, R_end, rotate=True):
        """model.backward (models.py:34-42 / 211-215) for all replicas: R_end [N,E].  rotate=False: the caller hands the
        states / slot T of the rollout buffers over to the next batch itself (BatchedTrainer: ops.batch_epilogue).
        = the four phases below back to back; BatchedTrainer captures `update_grads` and `update_apply` in hipGraphs and
        replays them around the (eager) gradient exchange, calling the two host-only phases itself.
        Opt-in ppo_epochs = K > 1: K - 1 further {update_ppo_grads, update_reduce, update_apply} on the same batch, `rotate` honoured
        on the last step only -- also where the opt-in KL stop (ppo_target_kl) refuses that step on the device."""
        lr = self.update_begin()
        K = self.ppo_epochs
        self.update_grads(R_end)
        self.update_reduce()
        self.update_apply(lr, rotate=rotate and K == 1)
        steps = self.ppo_steps()          # opt-in PPO epochs: the same batch, returns, advantages and lr; one all-reduce per step
        for i, step in enumerate(steps):
            self.update_ppo_grads(*step)
            self.update_reduce()
            self.update_apply(lr, rotate=rotate and i == len(steps) - 1)
        self.update_end()

    def ppo_steps(self):
        """The optimiser steps of an update behind the first, as the arguments of `update_ppo_grads` in order: (k,) for k = 2..K, or
        under the opt-in ppo_minibatches = M > 1 (k, j) for every epoch's groups j = 0..M-1."""
        K, M = self.ppo_epochs, self.ppo_minibatches
        if M == 1:
            return [(k,) for k in range(2, K + 1)]
        return [(k, j) for k in range(2, K + 1) for j in range(M)]

    def update_begin(self):
        """Host only: advance the lr schedule.  It counts lock-steps (environment steps per replica), the reference's
        get(n_step): the ini's total_step keeps its meaning for any number of replicas and ranks."""
        assert self.t == self.n_step, 'update() needs a full n_step batch (got %d)' % self.t
        self.cur_lr = self.lr_scheduler.get(self.n_step)
        return self.cur_lr

    @property
    def handoff_guarded(self):
        """This model launches in-launch hand-off kernels (one-launch coupled lock-step / BPTT): its optimiser step consults
        the device's hand-off status word and refuses a batch a timed-out wave contributed to (ops.rmsprop_tf_clip, ops.adam_clip)."""
        return bool(self.policy.coupled) and self.device.type == 'cuda'

    def update_grads(self, R_end):
        """Device work of one update up to the flat gradient: returns / advantages, loss, backward (no host
        synchronisation, static shapes and addresses: capturable)."""
        alpha = self.coop_gamma if self.coop_gamma >= 0 else -1.0
        T = self.n_step
        if self.ppo_target_kl is not None:
            # opt-in KL stop: every update starts with the stop down and one epoch applied (a kernel, so a replayed graph does it too)
            ops.copy_multi([(self.ppo_gate, self._ppo_gate_reset)])
            self._ppo_gate_pending = False
        if self.reward_scale != 'none' and self._rs_pending:
            # the one-replica path (`record` per step kept the raw rewards): the same one call the batched path makes in load_rewards
            self._scale_rewards(self._rs_raw)
        if self.save_acts and self.lock_step_form().launches == 1:
            # the critic's neighbour-action term of all T lock-steps in one launch (policies.py:59-77), then the values
            # in the [T,N,E] order the return scan reads
            with torch.no_grad():
                vn = self.buf_vn.view(self.n_agent, T * self.E)
                ops.nbr_action_value(self.buf_act.view(T * self.E, self.n_agent), self.policy.nbr_idx,
                                     self.policy.params['v_w'][:, self.n_lstm:], self.n_a, out=vn, accumulate=True)
                self.buf_v.copy_(self.buf_vn.permute(1, 0, 2))
        if self.gae_lambda == 1.0:
            ops.nstep_return(self.buf_r, self.buf_v, self.buf_done_post, R_end.contiguous(), self.gamma, alpha,
                             self.dist_dev, self.R, self.Adv)
        else:           # opt-in GAE(lambda): Adv = the lambda-weighted TD errors, R = Adv + v (the critic's target)
            ops.gae_return(self.buf_r, self.buf_v, self.buf_done_post, R_end.contiguous(), self.gamma, self.gae_lambda, alpha,
                           self.dist_dev, self.R, self.Adv)
        if self.adv_norm != 'none':     # opt-in: Adv_n = (Adv - mean) / (std + eps) per agent / over all agents; Adv and R stay as they are
            G = self.adv_moments.shape[0]
            ops.standardize(self.Adv.view(G, -1), self.adv_norm_epsilon, out=self.Adv_n.view(G, -1), partial=self._adv_partial,
                            moments=self.adv_moments)
        ps = self.policy.params
        ps.begin_backward()
        FP = self.buf_fp[:T].permute(1, 0, 2, 3).reshape(self.n_agent, T * self.E, self.n_a)
        X = self.buf_x[:T]            # compact [T,E,N,n_feat] slab: the encoders' kernels gather the neighbours themselves
        if self.save_acts:
            # (the sign image: only if every lock-step of this batch went through the kernel that writes it)
            bits = dict(S_bits=self.S_bits) if (self.S_bits is not None and self.policy._bits_steps == T) else {}
            Hs = self.policy.unroll_saved(X, FP, self.S_buf, self.G_buf, self.H_all, self.C_all,
                                          self.buf_done_pre, masked_steps=self.masked_steps, S_ext=self.S_ext, **bits)
        else:
            Hs = self.policy.unroll(X, FP, self.buf_done_pre, self.h_bw, self.c_bw, masked_steps=self.masked_steps)
        if self.ppo_epochs > 1:          # opt-in: the behaviour policy's log-probabilities, from the hidden states this epoch's loss reads
            self._take_logp_old(Hs)
        if not self._loss_backward_fused(Hs):
            loss = self._loss(Hs)
            loss.backward()
        self._end_grads()

    def _end_grads(self, kl_terms=None):
        """Close a gradient pass: the flat gradient, masked, and the float behind it that rides through the pass's ONE all-reduce --
        kl_terms (an epoch k >= 2 under the opt-in KL stop): that epoch's terms, whose approx_kl summed over agents goes there."""
        ps = self.policy.params
        ps.end_backward()
        if ps.mask is not None:          # entries of variables the reference does not create (heterogeneous nets)
            ps.grad.mul_(ps.mask)
        if kl_terms is not None:
            # free on these nets: only the coupled ones put their hand-off word there; `update_apply` decides on the sum
            ops.ppo_kl_sum(kl_terms, ps.grad_tail)
            self._ppo_gate_pending = True
        elif self._status_on_wire:
            # a rank whose in-launch hand-off timed out contributes invalid gradients: every rank must refuse the step (and recover
            # in lock-step, BatchedTrainer): the status word
            ps.grad_tail.copy_(ops.handoff_status(self.device)[:1])           # (int32 -> f32: an element-wise kernel)

    # ------------------------------------------------------------------ opt-in PPO epochs (MODEL_CONFIG ppo_epochs > 1)
    def _loss_adv(self):
        """The advantage the policy term reads, [N,T*E]."""
        N, T, E = self.n_agent, self.n_step, self.E
        adv = self._policy_adv().view(N, T * E)
        if not self.identical_agent and not self.per_agent_optimizer:
            # quirk Q6 (heterogeneous MA2C nets only, policies.py:241-254): the hetero branch builds prob_pi as
            # [N,1,T], so `prob_pi * ADV` broadcasts to [N,N,T] and every agent's log-probability is weighted by the
            # advantages of ALL agents: policy_loss = -sum_i mean_t(log pi_i[a] * sum_j ADV_j)
            adv = adv.sum(dim=0, keepdim=True).expand(N, T * E).contiguous()
        return adv

    def _take_logp_old(self, Hs):
        """ppo_logp_old = log(clip(softmax(logits_old)[a], 1e-10, 1)) of the actions taken, with the weights that produced the batch
        (called before the batch's first optimiser step; the clamp is the loss's)."""
        N, T, E = self.n_agent, self.n_step, self.E
        action = self.buf_act.view(T * E, N)
        with torch.no_grad():
            logits, v = self.policy.heads(Hs.detach(), action)
            if self.ppo_vclip is not None:       # opt-in: the same call's values, what the clipped value loss is clipped around
                ops.copy_multi([(self.ppo_v_old, v.contiguous())])           # (a kernel node in a captured update, not a memcpy node)
            if ops.ppo_loss_supported(self.n_a):
                ops.ppo_logp(logits, action, out=self.ppo_logp_old)
            else:
                log_pi = torch.log(torch.clamp(torch.softmax(logits, dim=-1), 1e-10, 1.0))
                self.ppo_logp_old.copy_(log_pi.gather(-1, action.t().long().unsqueeze(-1)).squeeze(-1))

    def _minibatch(self, k, j):
        """Step (k, j) under the opt-in replica minibatches: draw epoch k's permutation in front of its first group, then gather the
        rows of the replicas perm[j E/M .. (j + 1) E/M) of every operand of `update_ppo_grads` into the dense buffers `_mb` (whole
        sequences: all T steps of a replica and its own h_bw / c_bw).  Behind the update's last gather the count of updates moves."""
        N, T, E, M, mb = self.n_agent, self.n_step, self.E, self.ppo_minibatches, self._mb
        Em = E // M
        if j == 0 and not self._mb_identity:
            ops.minibatch_perm(int(self.seed or 0), self.mb_env_id_base, k, self.mb_count, mb['keys'], self.mb_perm)
        pairs = [(mb['x'], self.buf_x[:T], T), (mb['fp'], self.buf_fp[:T], T * N), (mb['act'], self.buf_act, T),
                 (mb['done'], self.buf_done_pre, T), (mb['adv'], self._loss_adv(), N * T), (mb['R'], self.R, N * T),
                 (mb['logp'], self.ppo_logp_old, N * T), (mb['h'], self.h_bw, N), (mb['c'], self.c_bw, N)]
        if self.ppo_vclip is not None:
            pairs.append((mb['v_old'], self.ppo_v_old, N * T))
        ops.minibatch_gather([(d_, s_) for d_, s_, _ in pairs], self.mb_perm[j * Em:(j + 1) * Em], outer_of=[o for _, _, o in pairs])
        if k == self.ppo_epochs and j == M - 1 and not self._mb_identity:
            ops.minibatch_count_advance(self.mb_count)

    def update_ppo_grads(self, k, j=0):
        """Epoch k = 2..K of an update up to the flat gradient: the forward pass recomputed with the current weights from the state
        the batch started from, the heads, the clipped surrogate against ppo_logp_old, backward.  R, Adv and the policy term's
        advantage are those of `update_grads`.  Capturable like it.  Under the opt-in ppo_minibatches = M > 1 this is step (k, j),
        j = 0..M-1: the same chain on the gathered tensors of the epoch's j-th group of replicas, its means over that group's rows;
        ppo_stats[k - 1] collects the mean of the epoch's M steps."""
        assert 2 <= k <= self.ppo_epochs and 0 <= j < self.ppo_minibatches
        N, T, E, M = self.n_agent, self.n_step, self.E, self.ppo_minibatches
        p = self.policy
        ps = p.params
        vclip = self.ppo_vclip
        if self._mb_on:
            self._minibatch(k, j)
            mb, E = self._mb, E // M
            X, FPs, done, h0, c0, action = mb['x'], mb['fp'], mb['done'], mb['h'], mb['c'], mb['act'].view(T * E, N)
            adv, R, logp_old, v_old = mb['adv'], mb['R'], mb['logp'], mb.get('v_old')
        else:
            X, FPs, done, h0, c0, action = self.buf_x[:T], self.buf_fp[:T], self.buf_done_pre, self.h_bw, self.c_bw, self.buf_act.view(T * E, N)
            logp_old, v_old = self.ppo_logp_old, (None if vclip is None else self.ppo_v_old)
        ps.begin_backward()
        FP = FPs.permute(1, 0, 2, 3).reshape(N, T * E, self.n_a)
        Hs = p.unroll(X, FP, done, h0, c0, masked_steps=self.masked_steps)
        logits, v = p.heads(Hs, action)
        if not self._mb_on:
            adv, R = self._loss_adv(), self.R.view(N, T * E)
        kw = {} if vclip is None else dict(v_old=v_old, vclip=vclip)
        if ops.ppo_loss_supported(self.n_a):
            per_agent, terms = ops.ppo_loss(logits, v, action, adv, R, logp_old, self.ppo_clip, self.v_coef, self.e_coef, **kw)
        else:
            per_agent, cols = self._loss_torch(logits, v, action, adv, R, logp_old, kw.get('v_old'))
            with torch.no_grad():
                terms = torch.stack(cols, dim=1)
        # (approx_kl, clip_frac) and vclip_frac of the epoch: the mean of its M steps, summed in step order
        stats = [(self.ppo_stats[k - 1], terms[:, 3:5])] + ([] if vclip is None else [(self.ppo_vclip_stats[k - 1], terms[:, 5])])
        for acc, t_ in stats:
            if j == 0:
                acc.copy_(t_)
            else:
                acc.add_(t_)
            if M > 1 and j == M - 1:
                acc.div_(M)
        t3 = self._terms = terms[:, :3].contiguous()
        self.last_loss = (t3[:, 0], t3[:, 1], t3[:, 2], per_agent.detach())
        per_agent.sum().backward()
        self._end_grads(kl_terms=None if self.ppo_target_kl is None else terms)

    @property
    def ppo_vclip_frac(self):
        """vclip_frac of the last update's last epoch, mean over agents (host read: synchronises); None with ppo_vclip off."""
        return None if not hasattr(self, 'ppo_vclip_stats') else float(self.ppo_vclip_stats[-1].mean())

    @property
    def ppo_epochs_done(self):
        """Optimiser steps the last update applied before the KL stop, 1..K (host read: synchronises); None with ppo_target_kl off."""
        if not hasattr(self, 'ppo_gate'):
            return None
        return 1 + (int(self.ppo_gate[2]) - 1) // self.ppo_minibatches      # (under minibatches: the epochs applied in full)

    @property
    def ppo_steps_done(self):
        """Optimiser steps the last update applied before the KL stop, 1..1 + (K - 1) M (host read: synchronises); None with
        ppo_target_kl off.  Without minibatches it equals ppo_epochs_done."""
        return None if not hasattr(self, 'ppo_gate') else int(self.ppo_gate[2])

    @property
    def ppo_kl(self):
        """approx_kl of the last update's last epoch, mean over agents (host read: synchronises); None with the key off."""
        return None if self.ppo_epochs == 1 or not hasattr(self, 'ppo_stats') else float(self.ppo_stats[-1, :, 0].mean())

    @property
    def ppo_clip_frac(self):
        """clip_frac of the last update's last epoch, mean over agents (host read: synchronises); None with the key off."""
        return None if self.ppo_epochs == 1 or not hasattr(self, 'ppo_stats') else float(self.ppo_stats[-1, :, 1].mean())

    @property
    def _status_on_wire(self):
        return self.dist_group is not None and self.handoff_guarded and self.save_acts

    def update_reduce(self):
        """The data-parallel exchange: ONE flat all-reduce per update (RCCL over xGMI) -- the gradient and, behind it, one float
        that is non-zero iff some rank's in-launch hand-off timed out in this batch (the reference has no collective)."""
        if self.dist_group is None:
            return
        import torch.distributed as dist
        dist.all_reduce(self.policy.params.grad_wire, group=self.dist_group)
        self.allreduce_calls = getattr(self, 'allreduce_calls', 0) + 1

    def update_apply(self, lr, rotate=True, lr_dev=None):
        """clip_by_global_norm + RMSProp on the flat buffers (policies.py:32-39, 257-264) -- under the opt-in optimizer = adam the same
        clip + Adam; lr_dev: device scalar that overrides `lr` (captured updates: the host refreshes it when the schedule moves)."""
        ps = self.policy.params
        scale = 1.0 / self.world_size
        guard = self.handoff_guarded
        if self._status_on_wire:             # some rank timed out (summed tail != 0): this rank's status word is raised as well
            st = ops.handoff_status(self.device)[:1]
            torch.maximum(st, (ps.grad_tail != 0).to(torch.int32), out=st)
        kw = {}
        if self.ppo_target_kl is not None:   # opt-in KL stop: the step consults the model's own word and changes nothing while it is up
            if self._ppo_gate_pending:       # (the step of an epoch k >= 2: its KL, summed over agents and ranks, against the target)
                ops.ppo_kl_gate(ps.grad_tail, self.world_size * self.n_agent, self.ppo_target_kl, self.ppo_gate)
                self._ppo_gate_pending = False
            kw['stop'] = self.ppo_gate
        # [G,P]: one group and one clip norm per agent (IA2C) or one over all agents
        shape = (self.n_agent, ps.P) if self.per_agent_optimizer else (1, self.n_agent * ps.P)
        w, g = ps.flat.view(shape), ps.grad.view(shape)
        if self.optimizer == 'adam':         # opt-in: the same clip, scale, guard and lr; Adam's slots and device counter
            ops.adam_clip(w, g, ps.adam_m.view(shape), ps.adam_v.view(shape), ps.scratch, ps.adam_t, lr, self.adam_beta1,
                          self.adam_beta2, self.adam_epsilon, self.max_grad_norm, scale, self.grad_norm, lr_dev=lr_dev, guard=guard, **kw)
        else:
            ops.rmsprop_tf_clip(w, g, ps.ms.view(shape), ps.scratch, lr, self.rmsp_alpha, self.rmsp_epsilon, self.max_grad_norm, scale,
                                self.grad_norm, lr_dev=lr_dev, guard=guard, **kw)
        self._after_apply()
        if rotate:
            T = self.n_step
            # states_bw <- states_fw (policies.py:115, 211)
            self.h_bw.copy_(self.h_fw)
            self.c_bw.copy_(self.c_fw)
            # slot T (bootstrap inputs) is slot 0 of the next batch
            self.buf_x[0].copy_(self.buf_x[T])
            self.buf_fp[0].copy_(self.buf_fp[T])

    def _after_apply(self):
        """Hook behind the optimiser step (ConseNet: the consensus averaging)."""

    def update_end(self):
        """Host only: the batch is consumed."""
        self.t = 0
        self.policy.set_rollout_saved((False, False, 0))     # what the rollout saved belonged to this batch (the next one sets it again)

    # ------------------------------------------------------------------ reference API (E = 1)
    def _obs_to_slab(self, obs):
        """list of N 1-D arrays (reference env) -> [1,N,n_obs] slab (+ fingerprints for ia2c_fp).  The slab has one
        n_feat-wide slot per (own, neighbour 1, ..): agents with narrower observations are zero padded inside their
        slots (heterogeneous systems), the reference's tightly concatenated vectors are scattered accordingly."""
        p = self.policy
        F, A = self.n_feat, self.n_a
        slab = np.zeros((1, self.n_agent, p.n_obs), dtype=np.float32)
        fp = None
        if not self._is_ma2c() and self.uses_fingerprint_obs():
            fp = np.zeros((self.n_agent, 1, p.n_na), dtype=np.float32)
        for i in range(self.n_agent):
            o = np.asarray(obs[i], dtype=np.float32)
            slab[0, i, :p.n_own[i]] = o[:p.n_own[i]]
            if self._is_ma2c():
                continue
            pos = p.n_own[i]
            for j in p.obs_order[i]:                     # the env's concatenation order -> the slab's ascending slots
                k = p.nbrs[i].index(j)
                slab[0, i, (k + 1) * F:(k + 1) * F + p.n_own[j]] = o[pos:pos + p.n_own[j]]
                pos += p.n_own[j]
            if fp is not None:
                for j in p.obs_order[i]:
                    k = p.nbrs[i].index(j)
                    fp[i, 0, k * A:k * A + p.n_a_ls[j]] = o[pos:pos + p.n_a_ls[j]]
                    pos += p.n_a_ls[j]
        slab = torch.from_numpy(slab).to(self.device)
        if self._is_ma2c():
            # MA2C envs hand over the own features only; neighbours are gathered here
            x = slab[:, :, :F].transpose(0, 1).contiguous()                   # [N,1,F]
            slab = torch.cat([x, ops.nbr_gather(x, p.nbr_idx)], dim=-1).transpose(0, 1).contiguous()
        return slab, fp

    def uses_fingerprint_obs(self):
        return False

    def _done_t(self, done):
        return torch.full((self.E,), float(bool(done)), dtype=F32, device=self.device)

    def _na_onehot_from_list(self, nactions):
        p = self.policy
        na = np.zeros((self.n_agent, 1, p.n_na), dtype=np.float32)
        for i in range(self.n_agent):
            for k, a in enumerate(np.asarray(nactions[i]).reshape(-1)):
                na[i, 0, k * self.n_a + int(a)] = 1.0
        return torch.from_numpy(na).to(self.device)

    def forward(self, obs, done, nactions=None, out_type='p'):
        """IA2C.forward (models.py:44-51): list of N pi arrays ('p') or N scalars ('v')."""
        slab, _ = self._obs_to_slab(obs)
        self._cur_slab = slab
        d = self._done_t(done)
        if out_type.startswith('p'):
            pi = self._policy_step(slab, d)
            return [x[:self.n_a_ls[i]] for i, x in enumerate(pi[:, 0].cpu().numpy())]
        v = self._value_step(slab, d, self._na_onehot_from_list(nactions))
        return [x for x in v[:, 0].cpu().numpy()]

    def add_transition(self, ob, naction, action, reward, value, done):
        """models.py:26-32 -> device buffers (slot t).  `naction` is not stored: it is
        env.get_neighbor_action(action) (utils.py:172, cacc_env.py:125-129), i.e. a function of `action`, and
        update() rebuilds the critic's one-hots from the action bytes."""
        t = self.t
        slab, fp = self._obs_to_slab(ob)
        self.buf_x[t].copy_(slab)
        self.buf_act[t].copy_(torch.as_tensor(np.asarray(action, dtype=np.uint8).reshape(1, -1)))
        self.buf_v[t].copy_(torch.as_tensor(np.asarray(value, dtype=np.float32).reshape(-1, 1)))
        self.buf_done_pre[t].fill_(float(self._prev_done))
        self._prev_done = bool(done)
        r = torch.as_tensor(np.asarray(reward, dtype=np.float32)).to(self.device)
        self.record(r.view(self.buf_r[t].shape), torch.full((self.E,), int(bool(done)), dtype=torch.uint8,
                                                           device=self.device))

    def backward(self, Rends, dt=0, summary_writer=None, global_step=None):
        R_end = torch.as_tensor(np.asarray(Rends, dtype=np.float32).reshape(self.n_agent, 1)).to(self.device)
        self.update(R_end)
        if self.handoff_guarded:
            # the reference API has no trainer that re-runs a batch: a timed-out in-launch hand-off (whose optimiser step the
            # device refused) is an error here, not a silent no-op (this path synchronises every lock-step anyway)
            ops.check_coupled_status(self.device)
        if summary_writer is not None:
            # the reference's six scalars of this update (policies.py:40-48, 116-117 / 212-213, 265-273) at global_step: plain
            # host reads, this path synchronises every lock-step anyway (the batched engine: train_record.TrainRecorder)
            train_record.write_scalars(summary_writer, self.policy.summary_name, self.per_agent_optimizer,
                                       [global_step], [train_record.host_row(self)], extras=False)

    def reset(self):
        self.reset_states()
        self._prev_done = True          # OnPolicyBuffer keeps the done BEFORE each step (agents/utils.py:732-739)

    _prev_done = True

    # ------------------------------------------------------------------ checkpoints (models.py:53-82)
    def save(self, model_dir, global_step):
        """`checkpoint-<step>.pt` (the reference writes TF Saver files `checkpoint-<step>.*`, models.py:53-58; the two
        formats are not interchangeable): a dict of plain tensors / numbers only, so it loads with
        torch.load(weights_only=True) -- variables under the reference's names and ragged shapes, the RMSProp slots,
        the lr schedule position.  'optimizer' names the slots that follow: 'rmsprop_ms', or under adam 'adam_m' / 'adam_v' and the
        step count 'adam_t' (a blob without the key is an RMSProp checkpoint of an earlier version)."""
        path = model_dir + 'checkpoint-%d.pt' % int(global_step)
        ps = self.policy.params
        sched = getattr(self, 'lr_scheduler', None)
        if self.optimizer == 'adam':
            slots = {'adam_m': ps.adam_m.detach().cpu(), 'adam_v': ps.adam_v.detach().cpu(), 'adam_t': ps.adam_t.detach().cpu()}
        else:
            slots = {'rmsprop_ms': ps.ms.detach().cpu()}
        if self.reward_scale != 'none' and hasattr(self, 'rs_state'):
            # opt-in reward scaling: the setting, the pooled running moments and the carried discounted returns (absent otherwise)
            slots.update({'reward_scale': self.reward_scale, 'reward_scale_state': self.rs_state.detach().cpu(),
                          'reward_scale_carry': self.rs_carry.detach().cpu()})
        if self.ppo_minibatches > 1 and hasattr(self, 'mb_count'):
            # opt-in replica minibatches: the updates made so far, what the next permutation is keyed by (absent otherwise)
            slots['ppo_minibatch_count'] = self.mb_count.detach().cpu()
        torch.save({'variables': {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in ps.ref_variables()},
                    'optimizer': self.optimizer, **slots, 'name': self.name, 'global_step': int(global_step),
                    'lr_n': float(sched.n) if sched is not None else -1.0}, path)
        # keep the 5 newest, like tf.train.Saver(max_to_keep=5)
        found = sorted(self._list_checkpoints(model_dir))
        for step, f in found[:-5]:
            os.remove(os.path.join(model_dir, f))

    @staticmethod
    def _list_checkpoints(model_dir):
        out = []
        for f in os.listdir(model_dir):
            if f.startswith('checkpoint'):
                tokens = f.split('.')[0].split('-')
                if len(tokens) == 2 and tokens[1].isdigit():
                    out.append((int(tokens[1]), f))
        return out

    def load(self, model_dir, checkpoint=None):
        """models.py:60-82: newest `checkpoint-<step>` of the directory, or the given step; False if there is none."""
        save_file = None
        if os.path.exists(model_dir):
            if checkpoint is None:
                found = sorted(self._list_checkpoints(model_dir))
                if found:
                    save_file = found[-1][1]
            else:
                save_file = 'checkpoint-%d.pt' % int(checkpoint)
        if save_file is not None and os.path.isfile(os.path.join(model_dir, save_file)):
            blob = torch.load(os.path.join(model_dir, save_file), weights_only=True, map_location='cpu')
            self.policy.params.load_ref_variables({k: v.numpy() for k, v in blob['variables'].items()})
            ps = self.policy.params
            saved_opt = blob.get('optimizer', 'rmsprop')
            if saved_opt != self.optimizer:
                # the variables are all `evaluate` needs; a run that trains on starts the other optimiser from fresh slots
                logging.warning('Checkpoint %s was written under optimizer = %s, this model uses %s: variables loaded, optimiser '
                                'slots left fresh' % (save_file, saved_opt, self.optimizer))
            elif self.optimizer == 'adam':
                ps.adam_m.copy_(blob['adam_m'])
                ps.adam_v.copy_(blob['adam_v'])
                ps.adam_t.copy_(blob['adam_t'])
            elif 'rmsprop_ms' in blob:
                ps.ms.copy_(blob['rmsprop_ms'])
            saved_rs = blob.get('reward_scale', 'none')
            if saved_rs != self.reward_scale:
                logging.warning('Checkpoint %s was written under reward_scale = %s, this model uses %s: variables loaded, the '
                                'reward-scale statistics left fresh' % (save_file, saved_rs, self.reward_scale))
            elif self.reward_scale != 'none' and hasattr(self, 'rs_state'):
                self.rs_state.copy_(blob['reward_scale_state'])
                if tuple(blob['reward_scale_carry'].shape) == tuple(self.rs_carry.shape):
                    self.rs_carry.copy_(blob['reward_scale_carry'])
                else:
                    logging.warning('Checkpoint %s carries %d discounted returns, this model %d (another num_envs): moments loaded, '
                                    'the carried returns left fresh' % (save_file, blob['reward_scale_carry'].numel(),
                                                                        self.rs_carry.numel()))
            if self.ppo_minibatches > 1 and hasattr(self, 'mb_count'):
                if 'ppo_minibatch_count' in blob:
                    self.mb_count.copy_(blob['ppo_minibatch_count'])
                else:
                    self.mb_count.zero_()
                    logging.warning('Checkpoint %s carries no ppo_minibatch_count (written without ppo_minibatches): the permutations '
                                    'start from count 0' % save_file)
            if blob.get('lr_n', -1.0) >= 0 and getattr(self, 'lr_scheduler', None) is not None:
                self.lr_scheduler.n = blob['lr_n']       # resume the lr decay where it stopped
            logging.info('Checkpoint loaded: %s' % save_file)
            return True
        logging.error('Can not find old checkpoint for %s' % model_dir)
        return False


class IA2C_FP(IA2C):
    """Fingerprint IA2C (models.py:161-188): neighbour policies appended to the observation."""
    policy_cls = FPPolicy
    name = 'ia2c_fp'

    def uses_fingerprint_obs(self):
        return True

    def forward(self, obs, done, nactions=None, out_type='p'):
        # the reference env delivers the neighbours' fingerprints inside `obs`; scatter them back
        # into the per-agent fingerprint table the batched policy gathers from
        _, fpg = self._obs_to_slab(obs)
        self.fp.copy_(self._ungather_fp(fpg))
        return super().forward(obs, done, nactions, out_type)

    def _ungather_fp(self, fpg):
        """[N,1,m_max*A] gathered neighbour fingerprints -> [N,1,A] table (every agent's
        fingerprint appears in at least one neighbour's slot)."""
        p = self.policy
        tab = self.fp_uniform.cpu().numpy().copy()
        idx = p.nbr_idx.cpu().numpy()
        for i in range(self.n_agent):
            for k in range(p.m_max):
                j = idx[i, k]
                if j >= 0:
                    tab[j, 0] = fpg[i, 0, k * self.n_a:(k + 1) * self.n_a]
        return torch.from_numpy(tab).to(self.device)

    def add_transition(self, ob, naction, action, reward, value, done):
        _, fpg = self._obs_to_slab(ob)
        self.buf_fp[self.t].copy_(self._ungather_fp(fpg))
        super().add_transition(ob, naction, action, reward, value, done)


class MA2C_NC(IA2C):
    """NeurComm (models.py:191-258): one optimiser over the whole meta-DNN."""
    policy_cls = NCMultiAgentPolicy
    per_agent_optimizer = False
    name = 'ma2c_nc'

    def forward(self, obs, done, ps, actions=None, out_type='p'):
        """MA2C_NC.forward (models.py:217-224): [N,A] ('p') or [N] ('v')."""
        slab, _ = self._obs_to_slab(obs)
        self.fp.copy_(self._pad_policies(ps))
        d = self._done_t(done)
        if out_type.startswith('p'):
            return self._unpad_policies(self._policy_step(slab, d)[:, 0].cpu().numpy())
        a = torch.as_tensor(np.asarray(actions, dtype=np.uint8).reshape(1, -1)).to(self.device)
        na = ops.nbr_onehot(a, self.policy.nbr_idx, self.n_a)
        return self._value_step(slab, d, na)[:, 0].cpu().numpy()

    def add_transition(self, ob, p, action, reward, value, done):
        t = self.t
        slab, _ = self._obs_to_slab(ob)
        self.buf_x[t].copy_(slab)
        self.buf_fp[t].copy_(self._pad_policies(p))
        a = torch.as_tensor(np.asarray(action, dtype=np.uint8).reshape(1, -1)).to(self.device)
        self.buf_act[t].copy_(a)
        self.buf_v[t].copy_(torch.as_tensor(np.asarray(value, dtype=np.float32).reshape(-1, 1)))
        self.buf_done_pre[t].fill_(float(self._prev_done))
        self._prev_done = bool(done)
        r = torch.as_tensor(np.asarray(reward, dtype=np.float32)).to(self.device)
        self.record(r.view(self.buf_r[t].shape), torch.full((self.E,), int(bool(done)), dtype=torch.uint8,
                                                           device=self.device))


class MA2C_IC3(MA2C_NC):
    """CommNet (models.py:278-292)."""
    policy_cls = IC3MultiAgentPolicy
    name = 'ma2c_ic3'


class IA2C_CU(MA2C_NC):
    """ConseNet (models.py:261-275): MA2C-style single optimiser + consensus averaging of the LSTM weights
    over each neighbourhood after every update (policies.py:351-364)."""
    policy_cls = ConsensusPolicy
    name = 'ma2c_cu'

    def _after_apply(self):
        # (under the opt-in KL stop a refused step must leave the weights as they are: the average is committed through the same word)
        if self.ppo_target_kl is None:
            self.policy.consensus_update()
        else:
            self.policy.consensus_update(skip_if=self.ppo_gate)


class MA2C_DIAL(MA2C_NC):
    """DIAL (models.py:295-309)."""
    policy_cls = DIALMultiAgentPolicy
    name = 'ma2c_dial'

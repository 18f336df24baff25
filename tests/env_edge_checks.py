"""Edge checks of the ATSC env step and reset kernels (csrc/grid.hip, csrc/grid_tile.h, csrc/realnet.hip), written as functions
of the implementation under test: the batch envs on the GPU (tests/test_gpu_env_edges.py), the float32 restatements or a
deliberately wrong variant of them on the CPU (tests/test_env_edges_cpu.py, which proves that the checks are sharp).

An implementation is an adapter `impl` with `impl.device`, `impl.limits` (the dispatch constants, below) and
`impl.make(family, E, **env_config)` -> an env with
    load(state)                 hand over any of q, tr, prev, t, xi, hw, episode (torch tensors on impl.device)
    step(actions, auto_reset)   one lock-step
    reset(mask=None, u0=None)
    state() / outputs()         dicts of tensors: q, tr, prev, t, xi, hw (None on `queue`), episode / obs, reward, done, greward
`family` is 'grid' (the 5x5 kernels), 'grid_rc' (rows, cols: the runtime-shape kernels) or 'net' (Monaco).  Every check forms its
expectation itself: the restatements oracle.grid_ref.GridBatchRef / grid_shape_ref.ShapeBatchRef / realnet_wait_ref.NetWaitRef in
float64 (`RefEnv`), fed the implementation's own float32 state in front of every step -- the hand-over protocol of
test_gpu_realnet_objectives.py::handed_over_step, so a threshold decision cannot drift over steps.

Tolerances: the project's single-step ones, unchanged (TOL: test_gpu_grid.py / test_gpu_grid_shape.py / test_gpu_realnet.py
::test_single_step_tight_from_random_state; TOL_WAIT: handed_over_step's rewards under `wait` / `hybrid`), applied through
`_close`, which prints the share of the bound used.  The per-node reward of the grid families, which no single-step test of the
grid compares, takes the network's bound for the same sum (rtol 1e-5, atol 1e-4).  The only entries a check leaves out are
head_wait decisions within 1e-5 of WAIT_EPS (`RefEnv.near_threshold`) and the rewards of the replicas holding one: at most 1e-3
of the valid entries of a check, asserted by `_finish`.  (A queue of exactly float32(WAIT_EPS) is asserted apart, against the
rule itself and not against another precision: check_saturation's threshold probe.)

A test cannot observe which kernel a host wrapper launched.  Every check of a launch branch therefore asserts the PRECONDITIONS
of that branch, computed from `impl.limits`: the GPU adapter declares the source's constants (GPU_LIMITS, each with file:line),
the CPU adapter scaled-down ones (CPU_LIMITS), so that "second round" and "tail group" stay meaningful at a few hundred replicas.

Large E without a large reference (check_large_E): a replica's step depends on nothing but its own rows.  K = 61 base states are
stepped as a K-batch and compared with the float64 expectation; the E-batch whose replica e holds base state e mod K (tiled on
the device) is stepped once and must have, replica by replica, the BITS of the K-batch in every state and output tensor -- the
K-batch runs the NT = 0 full-group kernel (REPS = 4 on the network), the E-batch the branch under test, the arithmetic is the
same.  61 is coprime to 8: every base state lands in every block slot, in the ragged tail and in each round.  A second step with
auto_reset at t = T - 1 checks, for all E, xi against oracle.philox with (env_id_base + e, episode), episode + 1, t = 0 and the
zeroed state.

Dispatch census: every hipLaunchKernelGGL of csrc/grid.hip and csrc/realnet.hip (and the env role of the lock-step launch).
NT = E * N * (160 compact | 352 slab) > 2^28 bytes (25 * 160 = 4000, 25 * 352 = 8800 at 5x5); C = p->compact_obs; W = objective != 0.
Test ids: [N] tests/test_gpu_env_edges.py, [G] test_gpu_grid.py, [S] test_gpu_grid_shape.py, [R] test_gpu_realnet.py,
[RO] test_gpu_realnet_objectives.py, [T] test_gpu_trainer.py.

  extern entry            kernel instantiation                 selected when (file:line)                              check, parameters
  ----------------------  -----------------------------------  -----------------------------------------------------  ------------------------------------------
  nmarl_grid_step         grid_step_kernel<0, false, false>    !NT (grid.hip:141), !C (:149), !W (:142, :147)         [G] test_trajectory_vs_oracle
                          grid_step_kernel<0, false, true>     !NT, !C, W                                             [G] test_wait_and_hybrid_objectives_vs_oracle
                          grid_step_kernel<0, true, false>     !NT, C (:148), !W                                      [N] test_large_E grid-compact-32773 (2 rounds);
                                                                                                                      [G] test_compact_observation_is_the_own_wave_block
                          grid_step_kernel<0, true, true>      !NT, C, W                                              [N] the K-batch of grid-compact-wait-67109;
                                                                                                                      [S] test_5x5_through_the_rc_entries_is_bit_identical
                          grid_step_kernel<1, true, false>     NT: E * 4000 > 2^28 (:141), C, !W                      [N] test_large_E grid-compact-queue-67109
                          grid_step_kernel<1, true, true>      NT, C, W                                               [N] test_large_E grid-compact-wait-67109
                          grid_step_kernel<1, false, false>    NT: E * 8800 > 2^28 (:141), !C, !W                     [N] test_large_E grid-slab-queue-30505
                          grid_step_kernel<1, false, true>     NT, !C, W                                              [N] test_large_E grid-slab-hybrid-30505
  nmarl_grid_step_rc      grid_step_rc_kernel<0, false, false> !NT (grid.hip:180), !C (:188), !W (:181, :186)         [S] test_trajectory_vs_restatement
                          grid_step_rc_kernel<0, false, true>  !NT, !C, W                                             [S] test_wait_and_hybrid_objectives_vs_restatement
                          grid_step_rc_kernel<0, true, false>  !NT, C (:187), !W                                      [N] test_large_E rc1x32-compact-32773 (2 rounds)
                          grid_step_rc_kernel<0, true, true>   !NT, C, W                                              [N] the K-batch of rc4x8-compact-hybrid-52429;
                                                                                                                      [S] test_5x5_through_the_rc_entries_is_bit_identical
                          grid_step_rc_kernel<1, true, false>  NT: E * 32 * 160 > 2^28 (:180), C, !W                  [N] test_large_E rc4x8-compact-queue-52429
                          grid_step_rc_kernel<1, true, true>   NT, C, W                                               [N] test_large_E rc4x8-compact-hybrid-52429
                          grid_step_rc_kernel<1, false, false> NT: E * 32 * 352 > 2^28 (:180), !C, !W                 [N] test_large_E rc4x8-slab-queue-23833
                          grid_step_rc_kernel<1, false, true>  NT, !C, W                                              [N] test_large_E rc4x8-slab-wait-23833
  (every grid step)       the grid-stride loop                 a second round: (E + 7) / 8 > 4096 (grid.hip:117-120,  [N] test_large_E: the E = 32773, 52429, 67109 rows
                                                               grid_tile.h:179); !full: E % 8 != 0 (grid_tile.h:184)  [N] every test_large_E row (E % 8 = 1 or 5)
  nmarl_grid_reset        grid_reset_kernel                    always (grid.hip:161)                                  [N] test_reset_forms grid; [G] test_episode_end_auto_reset_and_philox
  nmarl_grid_reset_rc     grid_reset_rc_kernel                 always (grid.hip:203)                                  [N] test_reset_forms grid_rc; [S] test_idle_and_tail_lanes_write_nothing
  nmarl_lstm_step_x       grid_step_groups<0, true, false, 16, genv given: the env role of the lock-step launch       [T] test_grid_env_step_as_a_role_of_the_lock_step_launch_
  (env role)                WORDS = true>                      (lstm_mfma.hip:454, :463)                                  is_the_env_kernel (not re-tested here)
  nmarl_net_step          net_step_kernel<4, false>            E <= 2048 (realnet.hip:394), objective 0 (:395-396)    [R] test_trajectory_vs_oracle; [N] every small-E check, net
                          net_step_kernel<4, true>             E <= 2048, objective != 0 (:398)                       [RO] test_handed_over_steps_vs_oracle
                          net_step_kernel<8, false>            E > 2048 (:394), objective 0                           [N] test_large_E net-queue-2049 (both coop_gamma), net-queue-32773
                          net_step_kernel<8, true>             E > 2048, objective != 0                               [N] test_large_E net-hybrid-32773 (rounds = 2, realnet.hip:108);
                                                                                                                      [RO] test_eight_replicas_per_block_form_with_a_ragged_last_block
                          net_step_kernel<2, false>            NMARL_NET_REPS=2 (realnet.hip:393-394), objective 0    [N] test_two_replicas_per_block_in_a_child_process (E = 1, 3, 8195)
                          net_step_kernel<2, true>             NMARL_NET_REPS=2, objective != 0                       [N] the same test, `wait`
  nmarl_net_reset         net_reset_kernel, hws NULL           always (realnet.hip:412 through :422)                  [N] test_reset_forms net queue; [R] test_episode_end_auto_reset_and_philox
  nmarl_net_reset_obj     net_reset_kernel, hws given or NULL  always (realnet.hip:412 through :429)                  [N] test_reset_forms net wait; [RO] test_resets_clear_head_wait
"""
import os
import sys

import numpy as np
import torch

import grid_shape_ref as S
from oracle import grid_ref as G
from oracle import philox
from oracle import realnet_ref as R
from realnet_wait_ref import NetWaitRef

F32 = np.float32
T_EPISODE = 720                     # episode_length_sec 3600 / control_interval_sec 5 of both shipped ATSC configs
Q_MAX, DET_CAP, WAIT_EPS = 26.0, 7.0, G.WAIT_EPS
K_BASE = 61                         # base states of check_large_E: coprime to the 8 (4, 2) replicas of a block
FAMILIES = ('grid', 'grid_rc', 'net')
RC_SHAPES = [(1, 2), (4, 8)]
SMALL_E = [1, 7, 8, 9]

# the dispatch constants of the kernels' host code
GPU_LIMITS = dict(
    name='gpu',
    group=8,                        # replicas per block of the grid kernels: grid.hip:41, grid_tile.h:174 (NREP = 8, grid.hip:47)
    max_blocks=4096,                # grid.hip:117-120 grid_blocks, realnet.hip:362-365 net_blocks
    nt_bytes=1 << 28,               # grid.hip:141, :180: (int64_t)256 << 20
    node_bytes=(352, 160),          # (slab, compact) per node: grid.hip:180; x 25 = 8800 / 4000 at 5x5: grid.hip:141
    net_switch=2048,                # realnet.hip:394: E <= 2048 ? 4 : 8
    net_reps=(4, 8),
)
CPU_LIMITS = dict(name='cpu', group=8, max_blocks=16, nt_bytes=1 << 20, node_bytes=(352, 160), net_switch=64, net_reps=(4, 8))

TOL = {
    'grid': dict(q=(1e-5, 1e-5), tr=(1e-5, 1e-6), obs=(1e-5, 1e-6), g=(1e-5, 1e-3), r=(1e-5, 1e-4)),
    'grid_rc': dict(q=(1e-5, 1e-5), tr=(1e-5, 1e-6), obs=(1e-5, 1e-6), g=(1e-5, 1e-3), r=(1e-5, 1e-4)),
    'net': dict(q=(1e-5, 1e-5), tr=(1e-5, 1e-6), obs=(1e-5, 1e-6), g=(1e-5, 2e-3), r=(1e-5, 1e-4)),
}
TOL_WAIT = dict(g=(2e-4, 5e-2), r=(2e-4, 5e-2))
EXCLUDED_CAP = 1e-3

DEFAULTS = {
    'grid': dict(objective='queue', coef_wait=0.2, coop_gamma=-1, norm_wave=5.0, clip_wave=2.0, compact=False, env_id_base=0, seed=12),
    'net': dict(objective='queue', coef_wait=0.2, coop_gamma=0.9, norm_wave=1.0, clip_wave=-1.0, compact=False, env_id_base=0, seed=12),
}


def full_config(family, cfg):
    c = dict(DEFAULTS['net' if family == 'net' else 'grid'])
    c.update(rows=5, cols=5)
    c.update(cfg)
    assert family in FAMILIES and c['objective'] in ('queue', 'wait', 'hybrid')
    assert family != 'grid' or (c['rows'], c['cols']) == (5, 5)
    assert family != 'net' or not c['compact']
    return c


# ------------------------------------------------------------------------------------------ the launch branches, from the limits
def grid_branch(limits, nn, compact, E):
    g = limits['group']
    blocks = (E + g - 1) // g
    return dict(nt=E * nn * limits['node_bytes'][1 if compact else 0] > limits['nt_bytes'],
                rounds=(blocks + limits['max_blocks'] - 1) // limits['max_blocks'], tail=E % g)


def net_branch(limits, E):
    reps = limits.get('net_reps_env') or (limits['net_reps'][0] if E <= limits['net_switch'] else limits['net_reps'][1])
    blocks = (E + reps - 1) // reps
    return dict(reps=reps, rounds=(blocks + limits['max_blocks'] - 1) // limits['max_blocks'], tail=E % reps)


# ------------------------------------------------------------------------------------------------ what is static about a family
class Fam:
    """N nodes, S lanes (grid) or links (network) per node, valid [N,S], n_a [N], green [N,A,S] (the lane / link discharges in
    phase a), entry [N,S] (the lane / link receives external demand)."""

    def __init__(self, family, rows=5, cols=5):
        self.family = family
        if family == 'net':
            tp = R.TOPO
            self.N, self.S = tp.N, tp.L
            self.valid = np.arange(tp.L)[None, :] < np.array(tp.n_s_ls)[:, None]
            self.n_a = np.array(tp.n_a_ls)
            self.green = tp.green != 0
            self.entry = tp.group >= 0
            self.interior = tp.fan > 0                                  # nodes that discharge into other links only
        else:
            self.rows, self.cols = rows, cols
            N = self.N = rows * cols
            self.S = G.N_LANE
            self.valid = np.ones((N, 6), dtype=bool)
            self.n_a = np.full(N, 5)
            gt = G.green_table() != 0                                   # [5,12]
            lane = np.stack([gt[:, G.LINK_LANE == l].any(axis=1) for l in range(6)], axis=1)      # [5,6]
            self.green = np.broadcast_to(lane[None], (N, 5, 6))
            self.entry = np.zeros((N, 6), dtype=bool)
            for node, ap, _ in S.entries(rows, cols):
                self.entry[node, G.LANE_APPROACH == ap] = True
            r, c = np.arange(N) // cols, np.arange(N) % cols
            self.interior = (r > 0) & (r < rows - 1) & (c > 0) & (c < cols - 1)

    def rand_actions(self, rng, E):
        return np.stack([rng.randint(0, self.n_a[i], size=E) for i in range(self.N)], axis=1)


def fam_of(family, cfg):
    c = full_config(family, cfg)
    return Fam(family, c['rows'], c['cols'])


# --------------------------------------------------------------------------------------------- the restatements behind one face
class RefEnv:
    """E replicas of a family on its restatement, in `dtype`: the float64 expectation of every check, and in float32 what the CPU
    adapter wraps.  Besides the restatement's own step it carries what the kernels add around it: the clamp of grid actions
    5..7 to 4 (grid_tile.h:230), the observation layout (compact or gathered), `episode`, and the fused / plain / masked
    re-initialisation with xi from oracle.philox (grid_tile.h:366-375, grid.hip:76-99, realnet.hip:290-298, :337-359)."""

    def __init__(self, family, E, dtype=np.float64, **cfg):
        c = self.cfg = full_config(family, cfg)
        self.family, self.E, self.f = family, E, dtype
        self.fam = Fam(family, c['rows'], c['cols'])
        self.objective = c['objective']
        if family == 'net':
            p = R.NetParams(norm_wave=c['norm_wave'], clip_wave=c['clip_wave'], flow_rate=325, coop_gamma=c['coop_gamma'])
            self.ref = NetWaitRef(p, E=E, dtype=dtype, objective=c['objective'], coef_wait=c['coef_wait'])
        else:
            p = G.GridParams(norm_wave=c['norm_wave'], clip_wave=c['clip_wave'], coop_gamma=c['coop_gamma'], objective=c['objective'],
                             coef_wait=c['coef_wait'])
            self.ref = (G.GridBatchRef(p, E=E, dtype=dtype) if family == 'grid' else
                        S.ShapeBatchRef(p, c['rows'], c['cols'], E=E, dtype=dtype))
        assert p.T == T_EPISODE
        self.T = p.T
        self.per_agent = c['coop_gamma'] >= 0
        self.ref.reset(np.ones((E, 4)))
        self.episode = np.zeros(E, dtype=np.int64)
        N = self.fam.N
        self.obs = np.zeros((E, N, self.obs_width()), dtype=dtype)
        self.reward = np.zeros((E, N) if self.per_agent else (E,), dtype=dtype)
        self.greward = np.zeros(E, dtype=dtype)
        self.done = np.zeros(E, dtype=np.uint8)
        self.last_q0 = self.last_served = None

    def obs_width(self):
        if self.family == 'net':
            return R.TOPO.L * (1 + R.TOPO.m_max)
        return 12 if self.cfg['compact'] else 60

    # -- state in and out (numpy)
    def load(self, st):
        r, f = self.ref, self.f
        for k, v in st.items():
            if v is None:
                continue
            v = np.asarray(v)
            if k == 'q':
                r.q = v.astype(f)
            elif k == 'tr':
                r.tr = v.astype(f)
            elif k == 'hw':
                r.hw = v.astype(f)
            elif k == 'xi':
                r.xi = v.astype(f)
            elif k == 'prev':
                r.prev = v.astype(np.int64)
            elif k == 't':
                r.t = v.astype(np.int64)
            elif k == 'episode':
                self.episode = v.astype(np.int64)
            else:
                raise KeyError(k)

    def state(self):
        r = self.ref
        return dict(q=r.q, tr=r.tr, prev=r.prev.astype(np.uint8), t=r.t.astype(np.int32), xi=r.xi,
                    hw=None if self.objective == 'queue' else r.hw, episode=self.episode.astype(np.int32))

    def outputs(self):
        return dict(obs=self.obs, reward=self.reward, done=self.done, greward=self.greward)

    # -- the step
    def _clamp(self, a):
        a = np.asarray(a).reshape(self.E, self.fam.N).astype(np.int64)
        return a if self.family == 'net' else np.minimum(a, 4)

    def _gather(self, ro):
        if self.family == 'net':
            return R.gather_net(ro)
        return ro.copy() if self.cfg['compact'] else G.gather_grid(ro, self.ref.nb)

    def _advance(self, a):
        r = self.ref
        q0, tr0 = r.q.copy(), r.tr.copy()
        ro, rew, done, g = r.step(a)
        if self.family == 'net':
            self.last_q0, self.last_served = r.last_q0, r.last_served
        else:                        # q' = q - served + transit: the served flow of the step, to rounding (float64: 1e-14)
            self.last_q0, self.last_served = q0, q0 + tr0 - r.q
        self.obs = self._gather(ro).astype(self.f)
        self.reward, self.greward, self.done = rew.astype(self.f), g.astype(self.f), np.asarray(done).astype(np.uint8)

    def step(self, a, auto_reset=False):
        self._advance(self._clamp(a))
        if auto_reset and self.done.any():
            self._reinit(self.done.astype(bool), None, fused=True)

    def draw_xi(self, ids=None, episode=None):
        """float32 [E,4]: 0.8 + 0.4 U of Philox (env_id_base + e, 0, episode, stream RESET), key = seed."""
        ids = np.arange(self.E) if ids is None else ids
        episode = self.episode if episode is None else episode
        seed = int(self.cfg['seed'])
        w = philox.philox4x32(self.cfg['env_id_base'] + ids, 0, episode, philox.STREAM_RESET, seed & 0xFFFFFFFF, seed >> 32)
        return F32(0.8) + F32(0.4) * philox.u01(np.stack(w, axis=-1))

    def _reinit(self, m, u0, fused=False):
        r = self.ref
        xi32 = self.draw_xi() if u0 is None else F32(0.8) + F32(0.4) * np.asarray(u0, dtype=F32).reshape(self.E, 4)
        r.reset(np.where(m[:, None], xi32.astype(self.f), r.xi), mask=m)
        if u0 is None:
            self.episode = self.episode + m.astype(np.int64)
        self.obs[m] = 0

    def reset(self, mask=None, u0=None):
        m = np.ones(self.E, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
        self._reinit(m, u0)

    def near_threshold(self, margin=1e-5):
        """[E,N,S] lanes / links whose head_wait decision of the LAST step sits within `margin` of WAIT_EPS (served, or the queue
        at the start of the step): NetWaitRef.near_threshold, for every family."""
        return (np.abs(self.last_served - WAIT_EPS) <= margin) | (np.abs(self.last_q0 - WAIT_EPS) <= margin)


# ------------------------------------------------------------------------------------------------------------- the adapters
def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class RefAdapterEnv:
    """A RefEnv (float32) behind the adapter face: tensors in, tensors out."""

    def __init__(self, model):
        self.m = model

    def load(self, st):
        self.m.load({k: _np(v) for k, v in st.items()})

    def step(self, a, auto_reset=False):
        self.m.step(_np(a), auto_reset)

    def reset(self, mask=None, u0=None):
        self.m.reset(_np(mask), _np(u0))

    def state(self):
        return {k: None if v is None else torch.from_numpy(np.ascontiguousarray(v)) for k, v in self.m.state().items()}

    def outputs(self):
        return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in self.m.outputs().items()}


class RefImpl:
    """The float32 restatements as the implementation under test, on scaled-down dispatch constants.  `model` builds the RefEnv:
    tests/test_env_edges_cpu.py passes subclasses with one mistake switched on."""
    device = 'cpu'

    def __init__(self, model=RefEnv, limits=CPU_LIMITS):
        self.model, self.limits = model, dict(limits)

    def make(self, family, E, **cfg):
        m = self.model(family, E, F32, **cfg)
        m.limits = self.limits
        return RefAdapterEnv(m)


class GpuEnv:
    """LargeGridBatchEnv / RealNetBatchEnv behind the adapter face."""

    def __init__(self, family, E, cfg):
        from helpers import grid_config, net_config
        c = full_config(family, cfg)
        if family == 'net':
            from deeprl_network_amd.envs.real_net_env import RealNetBatchEnv as Env
            cp = net_config(coop_gamma=c['coop_gamma'], seed=c['seed'])
            cp['ENV_CONFIG']['flow_rate'] = '325'
        else:
            from deeprl_network_amd.envs.large_grid_env import LargeGridBatchEnv as Env
            cp = grid_config(coop_gamma=c['coop_gamma'], seed=c['seed'])
            if family == 'grid_rc':
                cp['ENV_CONFIG']['grid_rows'], cp['ENV_CONFIG']['grid_cols'] = str(c['rows']), str(c['cols'])
        ec = cp['ENV_CONFIG']
        ec['objective'], ec['coef_wait'] = c['objective'], repr(float(c['coef_wait']))
        ec['norm_wave'], ec['clip_wave'] = repr(float(c['norm_wave'])), repr(float(c['clip_wave']))
        env = self.env = Env(ec, num_envs=E, env_id_base=c['env_id_base'], seed=c['seed'])
        assert env.T == T_EPISODE
        if family != 'net':
            assert env.fixed_shape == (family == 'grid') and (env.rows, env.cols) == (c['rows'], c['cols'])
            if c['compact']:
                assert env.set_compact_obs(True)
        self._names = dict(q='q', tr='transit', prev='prev_action', t='t', xi='xi', hw='head_wait', episode='episode')

    def load(self, st):
        for k, v in st.items():
            dst = getattr(self.env, self._names[k])
            if v is not None and dst is not None:
                dst.copy_(v.to(dst.device))

    def step(self, a, auto_reset=False):
        self.env.step(a.to(device=self.env.device, dtype=torch.uint8).contiguous(), auto_reset=auto_reset)

    def reset(self, mask=None, u0=None):
        dev = self.env.device
        self.env.reset(mask=None if mask is None else mask.to(device=dev, dtype=torch.uint8).contiguous(),
                       u0=None if u0 is None else u0.to(device=dev, dtype=torch.float32).contiguous())

    def state(self):
        return {k: getattr(self.env, n) for k, n in self._names.items()}

    def outputs(self):
        e = self.env
        return dict(obs=e.obs, reward=e.reward, done=e.done, greward=e.global_reward)


class GpuImpl:
    device = 'cuda'

    def __init__(self):
        self.limits = dict(GPU_LIMITS)
        ev = os.environ.get('NMARL_NET_REPS')                   # realnet.hip:393: read once per process
        self.limits['net_reps_env'] = int(ev) if ev else 0

    def make(self, family, E, **cfg):
        return GpuEnv(family, E, cfg)


# ------------------------------------------------------------------------------------------------------- comparing two sides
def new_stats():
    return dict(used={}, excluded=0, valid=0)


def _close(what, name, got, exp, tol, stats):
    """|got - exp| <= atol + rtol |exp| (numpy.testing.assert_allclose's criterion), the share of the bound printed and kept."""
    rtol, atol = tol
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (what, name, got.shape, exp.shape)
    u = 0.0
    if got.size:
        u = float(((np.abs(got - exp)) / (atol + rtol * np.abs(exp))).max()) if np.isfinite(got).all() else float('nan')
    print('%s %s: %.3g of its bound (rtol %g, atol %g)' % (what, name, u, rtol, atol))
    stats['used'][name] = max(stats['used'].get(name, 0.0), u)
    assert u <= 1.0, '%s %s: %.3g of its bound (rtol %g, atol %g)' % (what, name, u, rtol, atol)


def _finish(what, stats):
    share = stats['excluded'] / max(stats['valid'], 1)
    print('%s: worst shares %s; excluded %d of %d head_wait entries (%.2e, cap %g)'
          % (what, ', '.join('%s %.3g' % kv for kv in sorted(stats['used'].items())), stats['excluded'], stats['valid'], share, EXCLUDED_CAP))
    assert stats['excluded'] <= EXCLUDED_CAP * stats['valid'], '%s: excluded share %.2e above the cap' % (what, share)
    return stats


def compare(env, exp, what, stats):
    """Everything an implementation's env holds after a step against the float64 side `exp`.  -> the excluded entries [E,N,S]"""
    gs = {k: _np(v) for k, v in env.state().items()}
    go = {k: _np(v) for k, v in env.outputs().items()}
    es, eo = exp.state(), exp.outputs()
    tol = TOL[exp.family]
    valid = np.broadcast_to(exp.fam.valid, es['q'].shape)
    wait = exp.objective != 'queue'
    excl = np.zeros(valid.shape, dtype=bool)
    if wait:
        excl = exp.near_threshold(1e-5) & valid
        stats['excluded'] += int(excl.sum())
        stats['valid'] += int(valid.sum())
        cmp = valid & ~excl
        assert gs['hw'] is not None, '%s: no head_wait on a %s env' % (what, exp.objective)
        assert np.array_equal(gs['hw'][cmp], es['hw'][cmp]), '%s: head_wait differs in %d entries' % (what, (gs['hw'][cmp] != es['hw'][cmp]).sum())
        assert np.all(gs['hw'][~valid] == 0), '%s: head_wait on padding links' % what
    else:
        assert gs['hw'] is None, '%s: head_wait on a queue env' % what
    _close(what, 'q', gs['q'], es['q'], tol['q'], stats)
    _close(what, 'transit', gs['tr'], es['tr'], tol['tr'], stats)
    _close(what, 'obs', go['obs'], eo['obs'], tol['obs'], stats)
    ok = ~excl.any(axis=(1, 2))
    rt = TOL_WAIT if wait else tol
    _close(what, 'global reward', go['greward'][ok], eo['greward'][ok], rt['g'], stats)
    _close(what, 'reward', go['reward'][ok], eo['reward'][ok], rt['r'] if exp.per_agent else rt['g'], stats)
    for k in ('prev', 't', 'episode'):
        assert np.array_equal(gs[k], es[k]), '%s: %s differs' % (what, k)
    assert np.array_equal(gs['xi'], es['xi'].astype(F32)), '%s: xi differs' % what
    assert np.array_equal(go['done'].astype(bool), eo['done'].astype(bool)), '%s: done differs' % what
    return excl


def handed_over_step(impl, env, family, cfg, a, auto_reset, what, stats):
    """One step of `env` from its own state against the float64 restatement put into that state.  -> the float64 side"""
    exp = RefEnv(family, a.shape[0], np.float64, **cfg)
    exp.load({k: _np(v) for k, v in env.state().items()})
    env.step(_t(a.astype(np.uint8), impl.device), auto_reset)
    exp.step(a, auto_reset)
    exp.excluded = compare(env, exp, what, stats)
    return exp


def _bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 1: torch.uint8, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


# ------------------------------------------------------------------------------------------------------------------ states
SCHEDULE_T = sorted({0} | {60 * k - 1 for k in range(1, 12)} | {60 * k for k in range(1, 12)} | {T_EPISODE - 2, T_EPISODE - 1})
DESIGNS = ('gridlock', 'empty', 'overfull', 'eps', 'red_red')


def random_states(fam, E, rng, schedule_share=0.5):
    """The random mid-episode state of the single-step tests (test_gpu_grid.py, test_gpu_realnet_objectives.py::random_state): hw in
    multiples of 5, t partly from the schedule's piece boundaries; actions keep the phase with probability 0.6.  -> (state, a)"""
    N, Sx = fam.N, fam.S
    q = rng.uniform(0, 30, size=(E, N, Sx)) * (rng.rand(E, N, Sx) < 0.8)
    if fam.family == 'net':
        q = np.minimum(q, 26.0)
    t = rng.randint(0, 700, size=E)
    t = np.where(rng.rand(E) < schedule_share, np.array(SCHEDULE_T)[rng.randint(0, len(SCHEDULE_T), size=E)], t)
    prev = fam.rand_actions(rng, E)
    st = dict(q=(q * fam.valid).astype(F32), tr=(rng.uniform(0, 3, size=(E, N, Sx)) * fam.valid).astype(F32),
              prev=prev.astype(np.uint8), t=t.astype(np.int32),
              xi=F32(0.8) + F32(0.4) * rng.rand(E, 4).astype(F32),
              hw=(5.0 * rng.randint(0, 40, size=(E, N, Sx)) * fam.valid).astype(F32), episode=(np.arange(E) % 3).astype(np.int32))
    a = np.where(rng.rand(E, N) < 0.6, prev, fam.rand_actions(rng, E)).astype(np.uint8)
    return st, a


def apply_design(fam, st, a, e, kind):
    """Replica e of (st, a) becomes a designed state."""
    v = fam.valid
    one_approach = np.full(fam.N, 3) if fam.family != 'net' else fam.n_a - 1
    if kind == 'gridlock':          # every valid queue full, nothing in transit, a phase held that is green for one approach only
        st['q'][e], st['tr'][e], st['hw'][e] = Q_MAX * v, 0, 10.0 * v
        st['prev'][e] = a[e] = one_approach
        st['t'][e] = 100
    elif kind == 'empty':           # the empty network at t = 0
        st['q'][e], st['tr'][e], st['hw'][e], st['prev'][e], st['t'][e] = 0, 0, 0, 0, 0
    elif kind == 'overfull':        # q + transit > Q_MAX: the free space is negative before its clamp
        st['q'][e], st['tr'][e] = 25.0 * v, 3.0 * v
    elif kind == 'eps':             # queues of 5e-4 and 2e-3, either side of WAIT_EPS; the phase held
        lane = np.add.outer(np.arange(fam.N), np.arange(fam.S)) % 2
        st['q'][e], st['tr'][e], st['hw'][e] = np.where(lane == 0, F32(5e-4), F32(2e-3)) * v, 0, 15.0 * v
        st['prev'][e] = a[e] = 0
    elif kind == 'red_red':         # a change of phase between two phases that are both red for some lanes / links: 0 s of green
        st['q'][e], st['tr'][e], st['hw'][e] = 10.0 * v, 1.0 * v, 5.0 * v
        st['prev'][e], a[e] = (3, 4) if fam.family != 'net' else (0, 1)
    else:
        raise KeyError(kind)


def red_red_mask(fam):
    """[N,S] lanes / links that are red in both phases of the `red_red` design."""
    p, c = ((3, 4) if fam.family != 'net' else (0, 1))
    return ~fam.green[:, p] & ~fam.green[:, c] & fam.valid


def _fresh(impl, family, E, cfg, st):
    env = impl.make(family, E, **cfg)
    env.load({k: _t(v, impl.device) for k, v in st.items()})
    return env


# (id, family, env_config) of the small checks: both grid lattices asked for (1 x 2, 4 x 8), every objective, both reward forms,
# both observation layouts; a `queue` grid and a `queue` network among them (their masked resets)
SMALL_FAMILIES = [
    ('grid-queue', 'grid', dict()),
    ('grid-hybrid-compact', 'grid', dict(objective='hybrid', coop_gamma=0.9, compact=True)),
    ('rc1x2-wait', 'grid_rc', dict(rows=1, cols=2, objective='wait', coop_gamma=0.9)),
    ('rc4x8-queue-compact', 'grid_rc', dict(rows=4, cols=8, compact=True)),
    ('net-queue', 'net', dict()),
    ('net-wait-global', 'net', dict(objective='wait', coop_gamma=-1)),
]
# check_saturation asserts head_wait: `wait` / `hybrid` envs only
SATURATION_FAMILIES = [
    ('grid-hybrid', 'grid', dict(objective='hybrid', coop_gamma=0.9)),
    ('grid-wait-compact', 'grid', dict(objective='wait', compact=True)),
    ('rc1x2-wait', 'grid_rc', dict(rows=1, cols=2, objective='wait', coop_gamma=0.9)),
    ('rc4x8-hybrid-compact', 'grid_rc', dict(rows=4, cols=8, objective='hybrid', compact=True)),
    ('net-hybrid', 'net', dict(objective='hybrid')),
    ('net-wait-global', 'net', dict(objective='wait', coop_gamma=-1)),
]
SATURATION_RUNS = [(7, 0), (8, 0), (9, 0)] + [(1, rot) for rot in range(5)]          # (E, rot): E = 1 holds each design in turn
RESET_E = [9, 300]


# --------------------------------------------------------------------------------------------------------- A. large batches
def _case(cid, family, E_gpu, E_cpu, want, **cfg):
    return dict(id=cid, family=family, E=dict(gpu=E_gpu, cpu=E_cpu), want=want, cfg=cfg)


# want: nt / rounds of the grid kernels, reps / rounds of the network kernel; every row has a ragged last group (E % group != 0).
# E (gpu) is the smallest batch that reaches the branch: 32773 = 8 * 4096 + 5 (a second round of 5 live and 3 dead slots);
# 67109 * 4000 > 2^28 > 67108 * 4000; 30505 * 8800 > 2^28 > 30504 * 8800; 52429 * 32 * 160 > 2^28 > 52428 * 32 * 160;
# 23832 * 32 * 352 > 2^28 > 23831 * 32 * 352 and + 1 for E % 8 = 1; 2049 > 2048.  E (cpu): the same against CPU_LIMITS.
LARGE_CASES = [
    _case('grid-compact-queue-32773', 'grid', 32773, 133, dict(nt=False, rounds=2, dead=3), compact=True),
    _case('grid-compact-queue-67109', 'grid', 67109, 263, dict(nt=True, rounds=3), compact=True),
    _case('grid-compact-wait-67109', 'grid', 67109, 263, dict(nt=True, rounds=3), compact=True, objective='wait', coop_gamma=0.9),
    _case('grid-slab-queue-30505', 'grid', 30505, 121, dict(nt=True, rounds=1), coop_gamma=0.9),
    _case('grid-slab-hybrid-30505', 'grid', 30505, 121, dict(nt=True, rounds=1), objective='hybrid'),
    _case('rc4x8-compact-queue-52429', 'grid_rc', 52429, 205, dict(nt=True, rounds=2), rows=4, cols=8, compact=True),
    _case('rc4x8-compact-hybrid-52429', 'grid_rc', 52429, 205, dict(nt=True, rounds=2), rows=4, cols=8, compact=True, objective='hybrid',
          coop_gamma=0.9),
    _case('rc4x8-slab-queue-23833', 'grid_rc', 23833, 94, dict(nt=True, rounds=1), rows=4, cols=8, coop_gamma=0.9),
    _case('rc4x8-slab-wait-23833', 'grid_rc', 23833, 94, dict(nt=True, rounds=1), rows=4, cols=8, objective='wait'),
    _case('rc1x32-compact-queue-32773', 'grid_rc', 32773, 133, dict(nt=False, rounds=2, dead=3), rows=1, cols=32, compact=True),
    _case('net-queue-global-2049', 'net', 2049, 65, dict(reps=8, rounds=1), coop_gamma=-1),
    _case('net-queue-2049', 'net', 2049, 65, dict(reps=8, rounds=1), coop_gamma=0.9),
    _case('net-queue-32773', 'net', 32773, 133, dict(reps=8, rounds=2), coop_gamma=0.9),
    _case('net-hybrid-32773', 'net', 32773, 133, dict(reps=8, rounds=2), objective='hybrid'),
]
REPS2_CASES = [       # NMARL_NET_REPS=2: net_step_kernel<2, *>; 8195 = 2 * 4096 + 3: a second round at 2 replicas per block
    _case('net-reps2-queue-%d' % E, 'net', E, E, dict(reps=2, rounds=2 if E > 8192 else 1), coop_gamma=0.9) for E in (1, 3, 8195)
] + [
    _case('net-reps2-wait-%d' % E, 'net', E, E, dict(reps=2, rounds=2 if E > 8192 else 1), objective='wait') for E in (1, 3, 8195)
]


def base_states(fam, K, seed):
    """K distinct base states: random mid-episode ones mixed with the designed states."""
    rng = np.random.RandomState(seed)
    st, a = random_states(fam, K, rng)
    for e, kind in enumerate(DESIGNS):
        apply_design(fam, st, a, 7 * e + 3, kind)
    return st, a


def check_large_E(impl, case, keep=None, want=None):
    """See the module docstring, "Large E without a large reference".  keep: a dict that receives the E-batch's tensors after the
    first step (the child-process test compares them across two processes); want: the branch the batch must take, where it is
    not the case's own (the parent of that test runs the same states through the default dispatch)."""
    family, cfg, want = case['family'], dict(case['cfg'], env_id_base=1000), case['want'] if want is None else want
    E = case['E'][impl.limits['name']]
    lim, fam, K, dev = impl.limits, fam_of(family, case['cfg']), K_BASE, impl.device
    c = full_config(family, cfg)
    what = 'large E %s E=%d' % (case['id'], E)
    # ---- the preconditions of the branch, and of the plain branch for the K-batch
    if family == 'net':
        got, small = net_branch(lim, E), net_branch(lim, K)
        if not lim.get('net_reps_env'):
            assert small['reps'] == lim['net_reps'][0] and small['rounds'] == 1, small
        assert got['reps'] == want['reps'] and got['rounds'] == want['rounds'] and got['tail'] != 0, (what, got, want)
    else:
        got, small = grid_branch(lim, fam.N, c['compact'], E), grid_branch(lim, fam.N, c['compact'], K)
        assert not small['nt'] and small['rounds'] == 1, small
        assert got['nt'] == want['nt'] and got['rounds'] == want['rounds'] and got['tail'] != 0, (what, got, want)
        if 'dead' in want:          # the last round's only group mixes live and dead replica slots
            assert E - lim['group'] * lim['max_blocks'] == lim['group'] - want['dead'], (what, E)
    assert K % 2 == 1 and K % lim['group'] != 0
    # ---- K base states against the float64 expectation
    stats = new_stats()
    stK, aK = base_states(fam, K, seed=len(case['id']) * 1009 + fam.N)
    envK = _fresh(impl, family, K, cfg, stK)
    exp = handed_over_step(impl, envK, family, cfg, aK, False, what + ' K-batch', stats)
    assert float(exp.state()['q'].max()) > 20 and float(exp.outputs()['greward'].min()) < 0
    # ---- the E-batch: replica e = base state e mod K, tiled on the device
    idx = torch.arange(E, device=dev) % K
    envE = impl.make(family, E, **cfg)
    envE.load({k: _t(v, dev)[idx] for k, v in stK.items()})
    a_dev = _t(aK, dev)[idx].contiguous()
    envE.step(a_dev, False)
    tensors = dict(envE.state(), **envE.outputs())
    small_t = dict(envK.state(), **envK.outputs())
    for k, v in tensors.items():
        if v is None:
            assert small_t[k] is None
            continue
        assert same_bits(v, small_t[k].to(dev)[idx]), '%s: %s of the E-batch is not the K-batch\'s, replica by replica' % (what, k)
    if keep is not None:
        keep.update({k: v.clone() for k, v in tensors.items() if v is not None})
    # ---- the fused auto-reset of an episode's last step, on every replica
    ep0 = envE.state()['episode'].clone()
    for env, n in ((envE, E), (envK, K)):
        env.load(dict(t=torch.full((n,), T_EPISODE - 1, dtype=torch.int32, device=dev)))
    envE.step(a_dev, True)
    envK.step(_t(aK, dev), True)
    s, o, oK = envE.state(), envE.outputs(), envK.outputs()
    for k in ('reward', 'greward', 'done'):
        assert same_bits(o[k], oK[k].to(dev)[idx]), '%s: %s of the episode\'s last step' % (what, k)
    assert bool((o['done'] == 1).all()) and bool((s['t'] == 0).all()), what + ': done / t after the fused reset'
    for k in ('q', 'tr', 'prev', 'hw'):
        if s[k] is not None:
            assert bool((s[k] == 0).all()), '%s: %s is not cleared by the fused reset' % (what, k)
    assert bool((o['obs'] == 0).all()), what + ': the observation is not cleared by the fused reset'
    assert bool(torch.equal(s['episode'], ep0 + 1)), what + ': episode + 1'
    xi = RefEnv(family, 1, np.float64, **cfg).draw_xi(np.arange(E), _np(ep0).astype(np.int64))
    assert same_bits(s['xi'], _t(xi, dev)), '%s: xi is not Philox(env_id_base + e, episode)' % what
    assert len(np.unique(xi[:, 0])) > 0.9 * min(E, 1 << 20)
    return _finish(what, stats)


# ----------------------------------------------------------------------------------------------------- B. the small checks
def check_demand_schedule(impl, family, **cfg):
    """One handed-over step at every side of every 300-s piece boundary of the demand schedule (and at the episode's start and
    end), each t in its own replica, from a random state: an off-by-one of `piece` changes the arrivals."""
    fam = fam_of(family, cfg)
    ts = np.array(SCHEDULE_T)
    E = len(ts)
    # the set covers both sides of every step at which a group's rate changes value
    if family == 'net':
        rate = np.array([[R.activity(g, 5 * t) for g in range(4)] for t in range(T_EPISODE + 1)])
    else:
        rate = np.array([[G.demand_rate(g, 5 * t, 1100.0, 925.0) for g in range(4)] for t in range(T_EPISODE + 1)])
    change = np.nonzero((rate[1:] != rate[:-1]).any(axis=1))[0] + 1
    assert len(change) >= 10 and all(int(c) in ts and int(c) - 1 in ts for c in change if c < T_EPISODE), change
    rng = np.random.RandomState(11 + fam.N)
    st, a = random_states(fam, E, rng)
    st['t'] = ts.astype(np.int32)
    stats = new_stats()
    what = 'demand schedule %s' % family
    env = _fresh(impl, family, E, cfg, st)
    exp = handed_over_step(impl, env, family, cfg, a, False, what, stats)
    assert bool(exp.outputs()['done'][-1]) and not bool(exp.outputs()['done'][-2])
    return _finish(what, stats)


WAVE_CASES = [(1.0, -1.0), (1.0, 0.5), (5.0, -1.0), (5.0, 2.0), (0.5, 3.0)]


def check_wave_normalisation(impl, family, E, norm_wave, clip_wave, **cfg):
    """The observation min(q', 7) / norm_wave, clipped to [0, clip_wave] unless clip_wave < 0.  Replica 0 holds, on lanes / links
    that are red under a held phase (q' = q exactly), queues that put the wave below, at and above the clip."""
    cfg = dict(cfg, norm_wave=norm_wave, clip_wave=clip_wave)
    fam = fam_of(family, cfg)
    rng = np.random.RandomState(int(norm_wave * 10 + clip_wave * 3 + 7) + E)
    st, a = random_states(fam, E, rng)
    c = clip_wave * norm_wave if clip_wave > 0 else 3.5
    vals = np.array([0.5 * c, c, 1.5 * c, 7.5, 0.25], dtype=F32)
    st['q'][0] = vals[np.add.outer(np.arange(fam.N), np.arange(fam.S)) % 5] * fam.valid
    st['tr'][0] = 0
    st['prev'][0] = a[0] = 0
    stats = new_stats()
    what = 'wave norm=%g clip=%g %s E=%d' % (norm_wave, clip_wave, family, E)
    env = _fresh(impl, family, E, cfg, st)
    exp = handed_over_step(impl, env, family, cfg, a, False, what, stats)
    red = ~fam.green[:, 0] & fam.valid
    assert np.array_equal(exp.state()['q'][0][red], st['q'][0][red].astype(np.float64))          # q' = q on the red lanes
    pre = np.minimum(exp.state()['q'][0][red], DET_CAP) / norm_wave
    obs = exp.outputs()['obs']
    if clip_wave < 0:                # no clip: the full detector count shows (> 2 at norm_wave = 1)
        assert float(obs.max()) == DET_CAP / norm_wave and (norm_wave != 1.0 or float(obs.max()) > 2)
    elif clip_wave * norm_wave <= DET_CAP:
        assert (pre < clip_wave).any() and (pre == clip_wave).any() and (pre > clip_wave).any(), 'the queues do not straddle the clip'
        assert float(obs.max()) == clip_wave
    else:                            # the clip lies above the detector's range: it never binds
        assert float(obs.max()) == DET_CAP / norm_wave < clip_wave
    return _finish(what, stats)


def check_past_the_end(impl, family, E, **cfg):
    """auto_reset = 0: three steps from t = T - 1 -- done on all three, t counts on to T + 2, no demand, the traffic keeps
    evolving as the restatement says.  Then the same start with auto_reset = 1."""
    fam = fam_of(family, cfg)
    rng = np.random.RandomState(23 + E)
    st, a = random_states(fam, E, rng)
    st['t'][:] = T_EPISODE - 1
    stats = new_stats()
    what = 'past the end %s E=%d' % (family, E)
    env = _fresh(impl, family, E, cfg, st)
    for k in range(3):
        exp = handed_over_step(impl, env, family, cfg, a, False, '%s step %d' % (what, k), stats)
        assert bool(exp.outputs()['done'].all()) and bool((exp.state()['t'] == T_EPISODE + k).all())
        if k > 0:                    # t >= T: every rate of the schedule is 0, so nothing arrives on an entry that has no feeder
            got = _np(env.state()['tr'])
            alone = fam.entry if family == 'net' else fam.entry & ~_fed_lanes(fam)
            assert alone.any() and bool((got[:, alone] == 0).all()) and bool((exp.state()['tr'][:, alone] == 0).all())
        a = np.where(rng.rand(E, fam.N) < 0.6, a, fam.rand_actions(rng, E)).astype(np.uint8)
    env = _fresh(impl, family, E, cfg, st)
    exp = handed_over_step(impl, env, family, cfg, a, True, what + ' auto-reset', stats)
    s = exp.state()
    assert bool(exp.outputs()['done'].all()) and not s['t'].any() and not s['q'].any() and not s['prev'].any()
    assert np.array_equal(s['episode'], st['episode'] + 1) and not np.array_equal(s['xi'].astype(F32), st['xi'])
    return _finish(what, stats)


def _fed_lanes(fam):
    """[N,6] grid lanes whose approach has a neighbour inside the lattice feeding it."""
    fed = np.zeros((fam.N, 6), dtype=bool)
    for n in range(fam.N):
        r0, c0 = divmod(n, fam.cols)
        for ap, (dr, dc) in enumerate(G.APPROACH_FROM):
            if 0 <= r0 + dr < fam.rows and 0 <= c0 + dc < fam.cols:
                fed[n, G.LANE_APPROACH == ap] = True
    return fed


RESET_FORMS = ['plain', 'none', 'all', 'every third', 'last only']


def reset_mask(form, E):
    if form == 'plain':
        return None
    m = np.zeros(E, dtype=np.uint8)
    if form == 'all':
        m[:] = 1
    elif form == 'every third':
        m[::3] = 1
    elif form == 'last only':
        m[-1] = 1
    return m


def check_reset_forms(impl, family, E, form, with_u0, **cfg):
    """A plain or masked reset, with u0 or with the Philox draw, of an env that holds traffic: unselected replicas keep the bits
    of every state tensor, observation and episode included; selected ones take the restatement's reset; `episode` advances
    only without u0; head_wait is cleared on `wait` / `hybrid` and absent on `queue`."""
    cfg = dict(cfg, env_id_base=1000)
    fam = fam_of(family, cfg)
    rng = np.random.RandomState(31 + E)
    st, a = random_states(fam, E, rng)
    what = 'reset %s %s u0=%d E=%d' % (family, form, with_u0, E)
    env = _fresh(impl, family, E, cfg, st)
    env.step(_t(a, impl.device), False)                          # the observation holds traffic
    before = {k: None if v is None else v.clone() for k, v in dict(env.state(), **env.outputs()).items()}
    assert float(before['obs'].abs().max()) > 0 and float(before['q'].abs().max()) > 0
    exp = RefEnv(family, E, np.float64, **cfg)
    exp.load({k: _np(before[k]) for k in ('q', 'tr', 'prev', 't', 'xi', 'hw', 'episode')})
    exp.obs = _np(before['obs']).astype(np.float64)
    mask = reset_mask(form, E)
    u0 = rng.rand(E, 4).astype(F32) if with_u0 else None
    env.reset(mask=None if mask is None else _t(mask, impl.device), u0=None if u0 is None else _t(u0, impl.device))
    exp.reset(mask, u0)
    sel = np.ones(E, dtype=bool) if mask is None else mask.astype(bool)
    assert sel.sum() == {'plain': E, 'none': 0, 'all': E, 'every third': (E + 2) // 3, 'last only': 1}[form]
    gs = dict(env.state(), **env.outputs())
    wait = full_config(family, cfg)['objective'] != 'queue'
    assert (gs['hw'] is not None) == wait, what + ': head_wait must exist exactly on wait / hybrid'
    es = exp.state()
    for k in ('q', 'tr', 'prev', 't', 'xi', 'hw', 'episode', 'obs'):
        if gs[k] is None:
            continue
        g, b = _np(gs[k]), _np(before[k])
        assert np.array_equal(_np(_bits(gs[k]))[~sel], _np(_bits(before[k]))[~sel]), '%s: %s of an unselected replica changed' % (what, k)
        if k in ('q', 'tr', 'prev', 't', 'hw', 'obs'):
            assert not g[sel].any(), '%s: %s of a selected replica is not cleared' % (what, k)
        elif k == 'xi':
            assert np.array_equal(g[sel], es['xi'].astype(F32)[sel]), '%s: xi of the selected replicas' % what
            assert sel.sum() == 0 or not np.array_equal(g[sel], b[sel])
        else:
            assert np.array_equal(g, es['episode']), '%s: episode' % what
            assert np.array_equal(g[sel], b[sel] + (0 if with_u0 else 1)), '%s: episode advances only without u0' % what
    return sel


def check_action_clamp(impl, family, E, **cfg):
    """Grid actions 5, 6, 7 give the bits of action 4 (grid_tile.h:230; the hand-off words of the lock-step launch carry 3 bits),
    and the stored prev_action is 4."""
    assert family != 'net'
    fam = fam_of(family, cfg)
    rng = np.random.RandomState(41 + E)
    st, a = random_states(fam, E, rng)
    four = rng.rand(E, fam.N) < 0.4
    four.flat[0] = True
    a4 = np.where(four, 4, a).astype(np.uint8)
    big = a4.copy()
    big[four] = 5 + np.arange(int(four.sum())) % 3
    assert set(np.unique(big[four])) <= {5, 6, 7} and len(np.unique(big[four])) == min(3, int(four.sum()))
    stats = new_stats()
    what = 'action clamp %s E=%d' % (family, E)
    env4 = _fresh(impl, family, E, cfg, st)
    handed_over_step(impl, env4, family, cfg, a4, False, what, stats)
    envb = _fresh(impl, family, E, cfg, st)
    envb.step(_t(big, impl.device), False)
    t4, tb = dict(env4.state(), **env4.outputs()), dict(envb.state(), **envb.outputs())
    for k, v in t4.items():
        if v is not None:
            assert same_bits(v, tb[k]), '%s: %s differs between action 4 and actions 5..7' % (what, k)
    assert bool((_np(tb['prev'])[four] == 4).all()), what + ': prev_action must store 4'
    assert (st['prev'][four] != 4).any()                        # some of them change the phase: the yellow logic sees the 4 too
    return _finish(what, stats)


def check_saturation(impl, family, E, rot=0, **cfg):
    """The designed states (apply_design), design (e + rot) mod 6 in replica e (5: a random state), each against the expectation
    and against what it was designed to show."""
    cfg = dict(cfg)
    cfg.setdefault('objective', 'hybrid')
    fam = fam_of(family, cfg)
    rng = np.random.RandomState(53 + E + rot)
    st, a = random_states(fam, E, rng)
    kinds = [(DESIGNS + (None,))[(e + rot) % 6] for e in range(E)]
    for e, kind in enumerate(kinds):
        if kind is not None:
            apply_design(fam, st, a, e, kind)
    stats = new_stats()
    what = 'saturation %s E=%d rot=%d' % (family, E, rot)
    env = _fresh(impl, family, E, cfg, st)
    exp = handed_over_step(impl, env, family, cfg, a, False, what, stats)
    q1, hw1, tr1 = _np(env.state()['q']), _np(env.state()['hw']), _np(env.state()['tr'])
    v = fam.valid
    for e, kind in enumerate(kinds):
        if kind == 'gridlock':
            still = (exp.last_served[e] == 0) & v
            assert (still | ~v)[fam.interior].all(), what + ': an interior node of the gridlock serves'
            assert still.sum() > 0.5 * v.sum(), what + ': the gridlock moves'
            assert bool((q1[e][still] == Q_MAX).all()), what + ': gridlock, a blocked queue changed'
            assert bool((hw1[e][still] == 15.0).all()), what + ': gridlock, head_wait must grow by exactly 5'
        elif kind == 'empty':
            assert not q1[e].any() and not hw1[e].any() and float(_np(env.outputs()['greward'])[e]) == 0.0
            assert not tr1[e][~fam.entry].any() and float(tr1[e][fam.entry].sum()) > 0, what + ': the empty network receives its demand only'
        elif kind == 'overfull':
            assert bool((exp.state()['tr'][e] >= 0).all()) and bool((tr1[e] >= 0).all()), what + ': negative inflow'
            assert bool((st['q'][e] + st['tr'][e] > Q_MAX)[v].all())
        elif kind == 'eps':
            small = (st['q'][e] == F32(5e-4)) & v
            assert small.any() and not hw1[e][small].any(), what + ': a queue below WAIT_EPS keeps a waiting head vehicle'
            stand = (st['q'][e] == F32(2e-3)) & v & ~fam.green[:, 0]
            assert stand.any() and bool((hw1[e][stand] == 20.0).all()), what + ': a standing queue above WAIT_EPS'
            assert not exp.excluded[e].any()
        elif kind == 'red_red':
            rr = red_red_mask(fam)
            assert rr.any() and bool((q1[e][rr] == 11.0).all()) and bool((hw1[e][rr] == 10.0).all()), what + ': red to red serves'
    # ---- the threshold probe: a queue of exactly float32(WAIT_EPS) holds no standing queue ("at most WAIT_EPS", oracle/grid_ref.py
    # step 6: q <= WAIT_EPS in the env's own precision) -- asserted against the rule, not against float64
    pst, pa = random_states(fam, E, rng)
    pst['q'] = (F32(WAIT_EPS) * np.ones_like(pst['q']) * v).astype(F32)
    pst['tr'], pst['hw'] = np.zeros_like(pst['tr']), (15.0 * np.ones_like(pst['hw']) * v).astype(F32)
    assert bool((pst['q'][:, v] == F32(WAIT_EPS)).all())
    penv = _fresh(impl, family, E, cfg, pst)
    penv.step(_t(pa, impl.device), False)
    assert not _np(penv.state()['hw']).any(), what + ': a queue of exactly WAIT_EPS counts as standing'
    return _finish(what, stats)


# --------------------------------------------------------------------------- C. NMARL_NET_REPS=2, in a process of its own
def reps2_run(impl, out_path=None):
    """Every REPS2 case through check_large_E.  -> {case id: {tensor name: numpy bits}} of the E-batch after its first step."""
    out = {}
    for case in REPS2_CASES:
        keep = {}
        check_large_E(impl, case, keep=keep)
        for k, v in keep.items():
            out['%s/%s' % (case['id'], k)] = _np(_bits(v))
    if out_path is not None:
        np.savez(out_path, **out)
    return out


if __name__ == '__main__':           # the child of test_two_replicas_per_block_in_a_child_process
    assert sys.argv[1] == 'reps2' and os.environ.get('NMARL_NET_REPS') == '2'
    child = GpuImpl()
    assert child.limits['net_reps_env'] == 2
    reps2_run(child, sys.argv[2])
    print('reps2 child ok')

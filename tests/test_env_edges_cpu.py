"""The edge checks of tests/env_edge_checks.py are sharp: (a) the float32 restatements of the ATSC envs (oracle.grid_ref.GridBatchRef,
grid_shape_ref.ShapeBatchRef, realnet_wait_ref.NetWaitRef behind env_edge_checks.RefEnv) stay within every bound and within the
1e-3 cap of excluded head_wait decisions -- each check prints the share of every tolerance float32 uses against float64, and the
excluded share --, on dispatch constants scaled down so that "second round" and "tail group" mean something at a few hundred
replicas (env_edge_checks.CPU_LIMITS); (b) every named wrong variant of the adapter -- mistakes the env step and reset kernels of
csrc/grid.hip, csrc/grid_tile.h and csrc/realnet.hip could make without the older tests noticing -- fails the check listed
beside it in MUTANTS.

The wrong variants are `Wrong`, a RefEnv with one mistake switched on.  Most are a step before or behind the restatement's own
step; the two that sit inside it (the cap of the spill-back scale, the clamp of the free space) hand the restatement's module a
`np` whose minimum / maximum leaves that one call out."""
import contextlib

import numpy as np
import pytest

import env_edge_checks as eec
import grid_shape_ref
import realnet_wait_ref
from env_edge_checks import RefEnv, RefImpl
from oracle import grid_ref, realnet_ref

F32 = np.float32


# ------------------------------------------------------------------------------------------------------- the wrong variants
class _Numpy:
    """numpy with a few functions replaced."""

    def __init__(self, **over):
        self._over = over

    def __getattr__(self, k):
        over = self.__dict__['_over']
        return over[k] if k in over else getattr(np, k)


@contextlib.contextmanager
def _numpy_of(family, **over):
    mods = {'grid': [grid_ref], 'grid_rc': [grid_shape_ref], 'net': [realnet_ref, realnet_wait_ref]}[family] if over else []
    for m in mods:
        m.np = _Numpy(**over)
    try:
        yield
    finally:
        for m in mods:
            m.np = np


def _uncapped_minimum(a, b):
    """np.minimum, except the call `minimum(1, space / inflow)` of the restatements' spill-back scale."""
    return b if np.ndim(a) == 0 and float(a) == 1.0 else np.minimum(a, b)


def _unclamped_maximum(a, b):
    """np.maximum, except the call `maximum(Q_MAX - q - transit, 0)` of the restatements' free space."""
    return a if np.ndim(b) == 0 and float(b) == 0.0 and np.asarray(a).dtype.kind == 'f' else np.maximum(a, b)


class Wrong(RefEnv):
    variant = None

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        if self.variant == 'yellow charged when the phase did not change':
            inner = self.ref._eff_green

            def eff_green(prev, cur):          # a held green gets the 3 s of a red -> green change
                g = inner(prev, cur)
                return np.where((prev == cur)[..., None], g * 0.6, g).astype(g.dtype)
            self.ref._eff_green = eff_green

    def _per_round(self):
        lim = self.limits
        g = lim['group'] if self.family != 'net' else eec.net_branch(lim, self.E)['reps']
        return g, g * lim['max_blocks']

    def _snap(self):
        r = self.ref
        return dict(ref={k: getattr(r, k).copy() for k in ('q', 'tr', 'prev', 't', 'xi', 'hw')},
                    own={k: getattr(self, k).copy() for k in ('episode', 'obs', 'reward', 'greward', 'done')})

    def _restore(self, snap, sel):
        for k, v in snap['ref'].items():
            getattr(self.ref, k)[sel] = v[sel]
        for k, v in snap['own'].items():
            getattr(self, k)[sel] = v[sel]

    def step(self, a, auto_reset=False):
        v = self.variant
        g, per_round = self._per_round()
        if v in ('the tail group not stepped', 'replicas beyond the first round not stepped'):
            snap = self._snap()
            super().step(a, auto_reset)
            start = self.E // g * g if v.startswith('the tail') else per_round
            self._restore(snap, np.arange(self.E) >= start)
            return
        super().step(a, auto_reset)
        if v == 'dead slots of a mixed group written' and self.E % g:      # replica E - 1 stepped twice
            sub = RefEnv(self.family, 1, self.f, **dict(self.cfg, env_id_base=self.cfg['env_id_base'] + self.E - 1))
            st = {k: x[-1:] for k, x in self.state().items() if x is not None}
            st['hw'] = self.ref.hw[-1:]
            sub.load(st)
            sub.step(np.asarray(a).reshape(self.E, -1)[-1:], auto_reset)
            for k in ('q', 'tr', 'prev', 't', 'xi', 'hw'):
                getattr(self.ref, k)[-1] = getattr(sub.ref, k)[0]
            for k in ('episode', 'obs', 'reward', 'greward', 'done'):
                getattr(self, k)[-1] = getattr(sub, k)[0]

    def _clamp(self, a):
        if self.variant == 'action 5 taken as 0' and self.family != 'net':
            a = np.asarray(a).reshape(self.E, self.fam.N).astype(np.int64)
            return np.where(a > 4, 0, a)
        return super()._clamp(a)

    def _advance(self, a):
        v, r = self.variant, self.ref
        q0, hw0 = r.q.copy(), r.hw.copy()
        if v == 'piece computed from (t + 1) * 5':
            r.t = r.t + 1
        over = {'the spill-back scale not capped at 1': dict(minimum=_uncapped_minimum),
                'negative free space not clamped': dict(maximum=_unclamped_maximum)}.get(v, {})
        with _numpy_of(self.family, **over):
            super()._advance(a)
        if v == 'piece computed from (t + 1) * 5':
            r.t = r.t - 1
            self.done = (r.t >= self.T).astype(np.uint8)
        if v == 'done at t_new > T':
            self.done = (r.t > self.T).astype(np.uint8)
        if v == 'clip_wave < 0 treated as a clip at 0' and self.cfg['clip_wave'] < 0:
            self.obs[:] = 0
        if v == 'norm_wave ignored':
            keep, r.p.norm_wave = r.p.norm_wave, 1.0
            self.obs = self._gather(r.obs()).astype(self.f)
            r.p.norm_wave = keep
        if v == 'WAIT_EPS compared with >= on the queue side':             # q == WAIT_EPS counts as a standing queue
            sel = (q0 == self.f(eec.WAIT_EPS)) & (self.last_served <= self.f(eec.WAIT_EPS)) & self.fam.valid
            r.hw[sel] = hw0[sel] + self.f(5)
        if v == 'the per-agent reward written when coop_gamma < 0' and not self.per_agent:
            self.reward = (-(np.minimum(r.q[:, 0], self.f(eec.DET_CAP)) * self.fam.valid[0]).sum(axis=1)).astype(self.f)

    def _reinit(self, m, u0, fused=False):
        v, r = self.variant, self.ref
        prev0, hw0, ep0 = r.prev.copy(), r.hw.copy(), self.episode.copy()
        super()._reinit(m, u0, fused)
        if v == 'prev_action kept across auto-reset' and fused:
            r.prev[m] = prev0[m]
        if (v == 'head_wait kept across auto-reset' and fused) or (v == 'head_wait kept across masked reset' and not fused):
            r.hw[m] = hw0[m]
        if v == 'the last replica given the xi of its neighbour on auto-reset' and fused and m[-1] and self.E > 1:
            r.xi[-1] = self.draw_xi(np.array([self.E - 2]), ep0[-1:])[0]
        if v == 'episode advanced with u0' and u0 is not None:
            self.episode = self.episode + m.astype(np.int64)

    def reset(self, mask=None, u0=None):
        super().reset(mask, u0)
        if self.variant == 'masked reset zeroing an unselected replica\'s observation' and mask is not None:
            self.obs[:] = 0


def wrong(name):
    return RefImpl(model=type('Wrong_' + str(abs(hash(name))), (Wrong,), dict(variant=name)))


def _small(fid):
    return next((fam, cfg) for i, fam, cfg in eec.SMALL_FAMILIES + eec.SATURATION_FAMILIES if i == fid)


def _large(cid):
    return next(c for c in eec.LARGE_CASES if c['id'] == cid)


# ------------------------------------------------------------------------------------------ (a) the restatement passes
@pytest.mark.parametrize('case', eec.LARGE_CASES, ids=lambda c: c['id'])
def test_restatement_large_E(case):
    eec.check_large_E(RefImpl(), case)


@pytest.mark.parametrize('case', eec.REPS2_CASES, ids=lambda c: c['id'])
def test_restatement_two_replicas_per_block(case):
    """The states of the child-process test, on limits that say what NMARL_NET_REPS=2 says."""
    eec.check_large_E(RefImpl(limits=dict(eec.GPU_LIMITS, name='cpu', net_reps_env=2)), case)


@pytest.mark.parametrize('fid,family,cfg', eec.SMALL_FAMILIES, ids=[f[0] for f in eec.SMALL_FAMILIES])
def test_restatement_demand_schedule(fid, family, cfg):
    eec.check_demand_schedule(RefImpl(), family, **cfg)


@pytest.mark.parametrize('norm_wave,clip_wave', eec.WAVE_CASES)
@pytest.mark.parametrize('fid,family,cfg', eec.SMALL_FAMILIES, ids=[f[0] for f in eec.SMALL_FAMILIES])
def test_restatement_wave_normalisation(fid, family, cfg, norm_wave, clip_wave):
    for E in eec.SMALL_E:
        eec.check_wave_normalisation(RefImpl(), family, E, norm_wave, clip_wave, **cfg)


@pytest.mark.parametrize('fid,family,cfg', eec.SMALL_FAMILIES, ids=[f[0] for f in eec.SMALL_FAMILIES])
def test_restatement_past_the_end(fid, family, cfg):
    for E in eec.SMALL_E:
        eec.check_past_the_end(RefImpl(), family, E, **cfg)


@pytest.mark.parametrize('with_u0', [False, True])
@pytest.mark.parametrize('form', eec.RESET_FORMS)
@pytest.mark.parametrize('fid,family,cfg', eec.SMALL_FAMILIES, ids=[f[0] for f in eec.SMALL_FAMILIES])
def test_restatement_reset_forms(fid, family, cfg, form, with_u0):
    for E in eec.RESET_E:
        eec.check_reset_forms(RefImpl(), family, E, form, with_u0, **cfg)


@pytest.mark.parametrize('fid,family,cfg', [f for f in eec.SMALL_FAMILIES if f[1] != 'net'],
                         ids=[f[0] for f in eec.SMALL_FAMILIES if f[1] != 'net'])
def test_restatement_action_clamp(fid, family, cfg):
    for E in eec.SMALL_E:
        eec.check_action_clamp(RefImpl(), family, E, **cfg)


@pytest.mark.parametrize('fid,family,cfg', eec.SATURATION_FAMILIES, ids=[f[0] for f in eec.SATURATION_FAMILIES])
def test_restatement_saturation(fid, family, cfg):
    for E, rot in eec.SATURATION_RUNS:
        eec.check_saturation(RefImpl(), family, E, rot, **cfg)


def test_the_adapter_without_a_mistake_is_the_restatement():
    """`Wrong` with no variant switched on is RefEnv: the variants differ from the restatement by their one mistake alone."""
    for case in (_large('grid-slab-hybrid-30505'), _large('net-hybrid-32773')):
        eec.check_large_E(wrong(None), case)
    for fid in ('grid-hybrid', 'rc1x2-wait', 'net-hybrid'):
        family, cfg = _small(fid)
        eec.check_saturation(wrong(None), family, 9, 0, **cfg)


# ------------------------------------------------------------------------------------------ (b) the wrong variants fail
def _large_E(cid):
    return lambda impl: eec.check_large_E(impl, _large(cid))


def _on(check, fid, *args):
    def run(impl):
        family, cfg = _small(fid)
        return check(impl, family, *args, **cfg)
    return run


# variant -> the checks that must reject it (every family the mistake exists in)
MUTANTS = {
    'the tail group not stepped': [_large_E('grid-slab-queue-30505'), _large_E('rc4x8-slab-wait-23833'), _large_E('net-queue-2049')],
    'replicas beyond the first round not stepped': [_large_E('grid-compact-queue-32773'), _large_E('rc1x32-compact-queue-32773'),
                                                    _large_E('net-hybrid-32773')],
    'dead slots of a mixed group written': [_large_E('grid-compact-queue-32773'), _large_E('rc4x8-compact-hybrid-52429'),
                                            _large_E('net-queue-32773')],
    'the last replica given the xi of its neighbour on auto-reset': [_large_E('grid-compact-wait-67109'), _large_E('rc4x8-slab-queue-23833'),
                                                                     _large_E('net-queue-global-2049')],
    'piece computed from (t + 1) * 5': [_on(eec.check_demand_schedule, f) for f in ('grid-queue', 'rc1x2-wait', 'rc4x8-queue-compact', 'net-queue')],
    'yellow charged when the phase did not change': [_on(eec.check_demand_schedule, f) for f in ('grid-hybrid-compact', 'rc4x8-queue-compact',
                                                                                                  'net-wait-global')],
    'clip_wave < 0 treated as a clip at 0': [_on(eec.check_wave_normalisation, f, 8, 1.0, -1.0) for f in ('grid-queue', 'rc1x2-wait', 'net-queue')] +
                                            [_on(eec.check_wave_normalisation, 'grid-hybrid-compact', 1, 5.0, -1.0)],
    'norm_wave ignored': [_on(eec.check_wave_normalisation, f, 9, 5.0, 2.0) for f in ('grid-queue', 'rc4x8-queue-compact', 'net-wait-global')] +
                         [_on(eec.check_wave_normalisation, 'net-queue', 1, 0.5, 3.0)],
    'done at t_new > T': [_on(eec.check_past_the_end, f, 7) for f in ('grid-queue', 'rc1x2-wait', 'net-queue')],
    'prev_action kept across auto-reset': [_on(eec.check_past_the_end, f, 9) for f in ('grid-hybrid-compact', 'rc4x8-queue-compact', 'net-queue')],
    'head_wait kept across auto-reset': [_on(eec.check_past_the_end, f, 8) for f in ('grid-hybrid-compact', 'rc1x2-wait', 'net-wait-global')],
    'head_wait kept across masked reset': [_on(eec.check_reset_forms, f, 9, 'every third', True) for f in ('grid-hybrid-compact', 'rc1x2-wait',
                                                                                                           'net-wait-global')] +
                                          [_on(eec.check_reset_forms, 'net-wait-global', 300, 'last only', False)],
    'episode advanced with u0': [_on(eec.check_reset_forms, f, 9, form, True) for f in ('grid-queue', 'rc4x8-queue-compact', 'net-queue')
                                 for form in ('plain', 'last only')],
    'masked reset zeroing an unselected replica\'s observation': [_on(eec.check_reset_forms, f, 300, 'every third', False)
                                                                  for f in ('grid-queue', 'rc1x2-wait', 'net-queue')],
    'action 5 taken as 0': [_on(eec.check_action_clamp, f, E) for f in ('grid-queue', 'grid-hybrid-compact', 'rc1x2-wait', 'rc4x8-queue-compact')
                            for E in (1, 9)],
    'the spill-back scale not capped at 1': [_on(eec.check_saturation, f, 9, 0) for f in ('grid-hybrid', 'rc1x2-wait', 'rc4x8-hybrid-compact')] +
                                            [_on(eec.check_saturation, 'grid-wait-compact', 1, 4)],
    'negative free space not clamped': [_on(eec.check_saturation, f, 9, 0) for f in ('grid-hybrid', 'rc4x8-hybrid-compact', 'net-hybrid')] +
                                       [_on(eec.check_saturation, 'net-wait-global', 1, 2)],
    'WAIT_EPS compared with >= on the queue side': [_on(eec.check_saturation, f, 7, 0) for f in ('grid-wait-compact', 'rc1x2-wait', 'net-hybrid')],
    'the per-agent reward written when coop_gamma < 0': [_on(eec.check_demand_schedule, 'grid-queue'), _on(eec.check_demand_schedule, 'net-wait-global'),
                                                         _large_E('net-queue-global-2049')],
}


@pytest.mark.parametrize('name', list(MUTANTS))
def test_wrong_variant_is_rejected(name):
    assert MUTANTS[name]
    for run in MUTANTS[name]:
        with pytest.raises(AssertionError):
            run(wrong(name))
        run(wrong(None))                        # and the same call passes without the mistake


def test_every_variant_of_the_issue_has_a_check():
    assert len(MUTANTS) == 19                   # the 18 of the list; head_wait kept across auto-reset / across masked reset are two

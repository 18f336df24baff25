"""GPU: every launch branch and input edge of the ATSC env step and reset kernels (csrc/grid.hip, csrc/grid_tile.h, csrc/realnet.hip)
through LargeGridBatchEnv / RealNetBatchEnv, against the float64 restatements: the checks, their tolerances and the dispatch census
(which test reaches which hipLaunchKernelGGL) are in tests/env_edge_checks.py; tests/test_env_edges_cpu.py proves on the CPU that
every check rejects the mistake it is there for.  Comparisons of E-sized tensors stay on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import env_edge_checks as eec

pytestmark = pytest.mark.gpu

SMALL_IDS = [f[0] for f in eec.SMALL_FAMILIES]
GRID_FAMILIES = [f for f in eec.SMALL_FAMILIES if f[1] != 'net']


@pytest.fixture(scope='module')
def impl():
    impl = eec.GpuImpl()
    assert not impl.limits['net_reps_env'], 'NMARL_NET_REPS is set: the dispatch under test is overridden for this whole process'
    return impl


@pytest.mark.parametrize('case', eec.LARGE_CASES, ids=lambda c: c['id'])
def test_large_E(impl, case):
    """The non-temporal instantiations, the second and third round of the grid-stride loop with its mixed last group, the 8 replicas
    per block form of the network and its second round: the smallest batch that reaches each, bit for bit the K = 61 batch."""
    eec.check_large_E(impl, case)


def test_two_replicas_per_block_in_a_child_process(impl, tmp_path):
    """net_step_kernel<2, *> is selected by NMARL_NET_REPS alone, which the library reads once per process: a fresh child runs the
    checks (against the float64 expectation) with NMARL_NET_REPS=2 and writes its output bits; this process runs the same states
    through the default dispatch and asserts bit equality."""
    out = tmp_path / 'reps2.npz'
    tests = os.path.dirname(os.path.abspath(eec.__file__))
    paths = [os.path.dirname(tests), tests] + [p for p in os.environ.get('PYTHONPATH', '').split(os.pathsep) if p]
    env = dict(os.environ, NMARL_NET_REPS='2', PYTHONPATH=os.pathsep.join(paths))
    run = subprocess.run([sys.executable, os.path.abspath(eec.__file__), 'reps2', str(out)], env=env, timeout=300,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(run.stdout[-6000:])
    assert run.returncode == 0, 'the NMARL_NET_REPS=2 child failed (exit status %d)' % run.returncode
    with np.load(str(out)) as z:
        child = {k: z[k] for k in z.files}
    seen = 0
    for case in eec.REPS2_CASES:
        E, keep = case['E']['gpu'], {}
        eec.check_large_E(impl, case, keep=keep, want=dict(reps=4 if E <= 2048 else 8, rounds=1))
        for k, v in keep.items():
            assert np.array_equal(child['%s/%s' % (case['id'], k)], eec._np(eec._bits(v))), '%s: %s differs from the default dispatch' % (case['id'], k)
            seen += 1
    assert seen == len(child) and seen >= 10 * len(eec.REPS2_CASES)


@pytest.mark.parametrize('fid,family,cfg', eec.SMALL_FAMILIES, ids=SMALL_IDS)
def test_demand_schedule(impl, fid, family, cfg):
    eec.check_demand_schedule(impl, family, **cfg)


@pytest.mark.parametrize('norm_wave,clip_wave', eec.WAVE_CASES)
@pytest.mark.parametrize('fid,family,cfg', eec.SMALL_FAMILIES, ids=SMALL_IDS)
def test_wave_normalisation(impl, fid, family, cfg, norm_wave, clip_wave):
    for E in eec.SMALL_E:
        eec.check_wave_normalisation(impl, family, E, norm_wave, clip_wave, **cfg)


@pytest.mark.parametrize('fid,family,cfg', eec.SMALL_FAMILIES, ids=SMALL_IDS)
def test_past_the_end(impl, fid, family, cfg):
    for E in eec.SMALL_E:
        eec.check_past_the_end(impl, family, E, **cfg)


@pytest.mark.parametrize('with_u0', [False, True])
@pytest.mark.parametrize('form', eec.RESET_FORMS)
@pytest.mark.parametrize('fid,family,cfg', eec.SMALL_FAMILIES, ids=SMALL_IDS)
def test_reset_forms(impl, fid, family, cfg, form, with_u0):
    for E in eec.RESET_E:
        eec.check_reset_forms(impl, family, E, form, with_u0, **cfg)


@pytest.mark.parametrize('fid,family,cfg', GRID_FAMILIES, ids=[f[0] for f in GRID_FAMILIES])
def test_action_clamp(impl, fid, family, cfg):
    for E in eec.SMALL_E:
        eec.check_action_clamp(impl, family, E, **cfg)


@pytest.mark.parametrize('fid,family,cfg', eec.SATURATION_FAMILIES, ids=[f[0] for f in eec.SATURATION_FAMILIES])
def test_saturation(impl, fid, family, cfg):
    for E, rot in eec.SATURATION_RUNS:
        eec.check_saturation(impl, family, E, rot, **cfg)

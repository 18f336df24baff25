"""The `wait` / `hybrid` objectives and the rule-based `greedy` agent of the synthetic network, without a GPU: the
specification (tests/realnet_wait_ref.py), the controller's known answers, config parsing and the C-ABI."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import net_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nmarl.h')


def rand_actions(rng, E, tp):
    return np.stack([rng.randint(0, tp.n_a_ls[i], size=E) for i in range(tp.N)], axis=1)


def test_wait_and_hybrid_objectives_of_the_spec():
    """The grid's step 6 carried to links: the objective changes the reward and never the traffic, `wait` = -sum hw,
    `hybrid` = queue - coef * sum hw, a masked reset clears the masked replicas only, hw is a multiple of 5 s and 0 on
    padding links."""
    from oracle import realnet_ref as R
    from realnet_wait_ref import NetWaitRef
    E, tp = 3, R.TOPO
    refs = {o: NetWaitRef(R.NetParams(coop_gamma=0.9), E=E, objective=o, coef_wait=0.5) for o in ('queue', 'wait', 'hybrid')}
    xi = np.ones((E, 4))
    for r in refs.values():
        r.reset(xi)
        r.q[:] = 4.0 * r.valid                             # standing queues everywhere
    rng = np.random.RandomState(0)
    a = rand_actions(rng, E, tp)
    for t in range(40):
        if t % 8 == 7:                                     # hold a phase for 8 steps: the red links' front vehicles stand
            a = rand_actions(rng, E, tp)
        out = {o: r.step(a) for o, r in refs.items()}
        hw = refs['wait'].hw
        np.testing.assert_array_equal(hw, refs['hybrid'].hw)
        for o in ('wait', 'hybrid'):
            np.testing.assert_array_equal(refs[o].q, refs['queue'].q)
            np.testing.assert_array_equal(refs[o].tr, refs['queue'].tr)
            np.testing.assert_array_equal(out[o][0], out['queue'][0])
        wait = hw.sum(axis=2)
        np.testing.assert_allclose(out['wait'][1], -wait)                                   # per agent (coop_gamma >= 0)
        np.testing.assert_allclose(out['wait'][3], -wait.sum(axis=1))
        np.testing.assert_allclose(out['hybrid'][1], out['queue'][1] - 0.5 * wait)
        np.testing.assert_allclose(out['hybrid'][3], out['queue'][3] - 0.5 * wait.sum(axis=1))
        assert np.all(hw % 5.0 == 0) and np.all(hw >= 0) and np.all(hw[:, ~refs['wait'].valid] == 0)
    assert hw.max() >= 20.0 and (hw == 0).any()            # some links stood through red steps, served ones were cleared
    # a link that is red in both the previous and the new phase discharges nothing: it gains exactly 5 s
    r = refs['wait']
    before, prev = r.hw.copy(), r.prev.copy()
    r.step(prev)
    n = np.arange(tp.N)[None, :]
    red = (tp.green[n, prev] == 0) & r.valid & (r.last_q0 > 1.0)
    assert red.any()
    np.testing.assert_array_equal(r.hw[red], before[red] + 5.0)
    before = r.hw.copy()
    r.reset(xi, mask=[1, 0, 0])
    assert np.all(r.hw[0] == 0) and np.all(r.q[0] == 0) and np.array_equal(r.hw[1:], before[1:]) and before[1:].max() > 0
    # a global reward env (coop_gamma < 0) hands out the sum
    g = NetWaitRef(R.NetParams(coop_gamma=-1), E=E, objective='hybrid', coef_wait=0.5)
    g.reset(xi)
    g.q[:] = 4.0 * g.valid
    o = g.step(a)
    assert o[1].shape == (E,) and np.array_equal(o[1], o[3])


def test_greedy_controller_known_answers():
    """real_net_env.py:112-145: per node the phase whose 'G' links hold the most vehicles; a permitted 'g' does not count;
    np.argmax keeps the first maximum."""
    from deeprl_network_amd.envs.real_net_env import NODE_DEFS, PHASE_SETS, RealNetController
    names = sorted(n for n, _, _ in NODE_DEFS)
    ctl = RealNetController(names)
    assert ctl.name == 'greedy' and ctl.reset() is None and ctl.load('anywhere/') is True
    assert PHASE_SETS[dict((n, k) for n, k, _ in NODE_DEFS)['9433']] == ('Gg', 'rG')
    assert ctl.greedy([1, 3], '9433') == 1                 # 'Gg' counts link 0 (1), 'rG' link 1 (3)
    assert ctl.greedy([3, 1], '9433') == 0
    assert ctl.greedy([2, 2], '9433') == 0                 # a tie: the first maximum
    assert ctl.greedy([0, 0], '9433') == 0
    # node 8996 ('Grr', 'gGG'): link 0 is 'g' in phase 1 and never adds to it
    assert ctl.greedy([5, 1, 1], '8996') == 0 and ctl.greedy([100, 0, 0], '8996') == 0 and ctl.greedy([5, 3, 3], '8996') == 1
    # node 9153 ('GGrrr', 'ggGGG'): the two 'g' links of phase 1 do not count
    assert ctl.greedy([2, 2, 1, 1, 1], '9153') == 0 and ctl.greedy([2, 2, 2, 2, 1], '9153') == 1
    keys = dict((n, k) for n, k, _ in NODE_DEFS)
    rng = np.random.RandomState(1)
    obs = [rng.rand(len(PHASE_SETS[keys[n]][0])) * 7 for n in names]
    act = ctl.forward(obs)
    assert len(act) == 28 and all(isinstance(a, int) and 0 <= a < len(PHASE_SETS[keys[n]]) for a, n in zip(act, names))
    for a, ob, n in zip(act, obs, names):                  # against the definition written out
        flows = [sum(ob[k] for k, ch in enumerate(ph) if ch == 'G') for ph in PHASE_SETS[keys[n]]]
        assert a == int(np.argmax(flows))
    assert len(set(act)) > 1


def _lib_or_skip():
    """The binding; skipped only where the library has not been built at all.  A stale library, an ABI mismatch or a broken import
    of the package is an ImportError of the project's own and fails the test."""
    so = os.path.join(ROOT, 'deeprl_network_amd', 'libnmarl_hip.so')
    if not os.path.exists(so):
        pytest.skip('%s is not built' % so)
    from deeprl_network_amd import _lib
    return _lib


def test_config_parsing_of_the_objectives():
    _lib_or_skip()
    from deeprl_network_amd.envs.real_net_env import net_params_from_config
    for name, code in (('queue', 0), ('wait', 1), ('hybrid', 2)):
        cp = net_config()
        cp['ENV_CONFIG']['objective'] = name
        cp['ENV_CONFIG']['coef_wait'] = '0.2'
        p = net_params_from_config(cp['ENV_CONFIG'])
        assert p.objective == code and p.coef_wait == pytest.approx(0.2) and not p.head_wait
        assert p.T == 720 and p.per_agent_reward == 1 and p.flow_rate == 325
    cp = net_config()                                      # the shipped config: queue, coef_wait = 0
    p = net_params_from_config(cp['ENV_CONFIG'])
    assert p.objective == 0 and p.coef_wait == 0.0
    del cp['ENV_CONFIG']['coef_wait']
    cp['ENV_CONFIG']['objective'] = 'hybrid'
    assert net_params_from_config(cp['ENV_CONFIG']).coef_wait == 0.0
    cp['ENV_CONFIG']['objective'] = 'foo'
    with pytest.raises(ValueError, match='queue.*wait.*hybrid'):
        net_params_from_config(cp['ENV_CONFIG'])
    del cp['ENV_CONFIG']['objective']                      # the key is required, as before
    with pytest.raises(ValueError, match='queue.*wait.*hybrid'):
        net_params_from_config(cp['ENV_CONFIG'])


def test_net_params_layout_matches_c_compiler(tmp_path):
    """nmarl_net_params_t as gcc lays it out == _lib.NetParams, field by field (the method of
    test_abi.py::test_struct_layouts_match_c_compiler); the new fields follow the old ones in the grid's order."""
    _lib = _lib_or_skip()
    mirror = _lib.NetParams
    fields = [n for n, _ in mirror._fields_]
    assert fields == ['norm_wave', 'clip_wave', 'flow_rate', 'T', 'per_agent_reward', 'objective', 'coef_wait', 'head_wait']
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu", sizeof(nmarl_net_params_t));\n' % HEADER
    for f in fields:
        src += 'printf(" %%zu", offsetof(nmarl_net_params_t, %s));\n' % f
    src += 'return 0;}\n'
    c = tmp_path / 'off.c'
    c.write_text(src)
    exe = str(tmp_path / 'off')
    subprocess.check_call(['gcc', str(c), '-o', exe])
    nums = [int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert nums[0] == ctypes.sizeof(mirror) == 7 * 4 + 4 + 8           # (+ padding in front of the pointer)
    assert nums[1:] == [getattr(mirror, f).offset for f in fields]
    assert nums[1:6] == [0, 4, 8, 12, 16]                  # the fields of the `queue`-only struct keep their offsets


def test_reset_obj_is_declared_exported_and_bound():
    _lib = _lib_or_skip()
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    m = re.search(r'\bint\s+nmarl_net_reset_obj\s*\(([^;]*?)\)\s*;', src, flags=re.S)
    assert m, 'nmarl_net_reset_obj is not declared in include/nmarl.h'
    m0 = re.search(r'\bint\s+nmarl_net_reset\s*\(([^;]*?)\)\s*;', src, flags=re.S)
    norm = lambda s: re.sub(r'\s+', ' ', s).strip()
    assert norm(m.group(1)) == 'const nmarl_net_params_t* p, ' + norm(m0.group(1))      # nmarl_net_reset's arguments, params in front
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r' T nmarl_net_reset_obj$', nm, flags=re.M)
    sig = _lib.SIGNATURES['nmarl_net_reset_obj']
    assert sig[0]._type_ is _lib.NetParams and sig[1:] == _lib.SIGNATURES['nmarl_net_reset']
    assert list(_lib.lib.nmarl_net_reset_obj.argtypes) == sig
    assert _lib.lib.nmarl_abi_version() == _lib.ABI_VERSION

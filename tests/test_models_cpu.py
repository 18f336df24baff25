"""Host-logic parity of agents.models / agents.policies against the golden vectors produced by
the REAL reference model code on the fake-TF shim (tests/golden/nn_*.npz).  The HIP ops are
replaced by their oracle restatements (tests/cpu_emulation.py) because this container has no GPU;
tests/test_gpu_models.py runs the same comparison through the real kernels."""
import glob
import os

import numpy as np
import pytest
import torch

from cpu_emulation import cpu_ops
from helpers import GOLDEN, build_product_model, compare_scripted, drive_scripted, load_npz, var_stats_from_named

CASES = sorted(glob.glob(os.path.join(GOLDEN, 'nn_*.npz')))


@pytest.mark.parametrize('path', CASES, ids=[os.path.basename(c)[3:-4] for c in CASES])
def test_scripted_run_matches_reference(path):
    z = load_npz(path)
    with cpu_ops():
        model = build_product_model(z, 'cpu')
        named = model.policy.params.ref_variables()
        # initial weights: identical np.random draw order and shapes as the reference
        assert [n for n, _ in named] == [str(n) for n in z['names']]
        assert [str(a.shape) for _, a in named] == [str(s) for s in z['shapes']]
        np.testing.assert_allclose(var_stats_from_named(named), z['stats0'], rtol=1e-6, atol=1e-7)
        out = drive_scripted(model, z)
    compare_scripted(out, z)


def test_ortho_init_matches_reference():
    from deeprl_network_amd.agents.policies import ortho_init
    z = load_npz(os.path.join(GOLDEN, 'ortho_init.npz'))
    np.random.seed(12)
    for k, s in enumerate(z['shapes']):
        w = ortho_init(tuple(int(x) for x in s))
        assert w.dtype == np.float32 and np.array_equal(w, z['w%d' % k])
    assert np.random.rand() == float(z['after'])


@pytest.mark.parametrize('name', ['ma2c_nc_ragged', 'ia2c_fp_ragged', 'ma2c_ic3_ragged'])
def test_heterogeneous_checkpoint_roundtrip_and_layout(name, tmp_path):
    """Heterogeneous nets: variables are exported / re-imported under the reference's ragged shapes, padded entries
    keep their fill (0, -1e30 for absent actions), and the update mask covers exactly the exported entries."""
    import torch
    z = load_npz(os.path.join(GOLDEN, 'nn_%s.npz' % name))
    with cpu_ops():
        m1 = build_product_model(z, 'cpu')
        ps = m1.policy.params
        named = ps.ref_variables()
        assert [str(tuple(a.shape)) for _, a in named] == [str(s) for s in z['shapes']]
        n_exported = sum(a.size for _, a in named)
        if ps.mask is not None:
            # mask == 1 exactly on entries of existing variables; padded-but-existing tensors are larger than the export
            assert int(ps.mask.sum().item()) == n_exported
        m1.save(str(tmp_path) + '/', 7)
        m2 = build_product_model(z, 'cpu')
        with torch.no_grad():
            m2.policy.params.flat.add_(0.5)              # scramble, incl. the padding
        assert m2.load(str(tmp_path) + '/')
        for key in m1.policy.params.index:                   # every tensor incl. its padded entries (alignment gaps aside)
            assert torch.equal(m1.policy.params[key], m2.policy.params[key]), key
        pb = m2.policy.params['pi_b'].detach()
        for i, n in enumerate(m2.n_a_ls):
            assert (pb[i, n:] == -1e30).all() and (pb[i, :n] == 0).all()


BATCHED = sorted(glob.glob(os.path.join(GOLDEN, 'nnb_*.npz')))


@pytest.mark.parametrize('saved', [False, True], ids=['recompute', 'saved_acts'])
@pytest.mark.parametrize('path', BATCHED, ids=[os.path.basename(c)[4:-4] for c in BATCHED])
def test_batched_update_equals_mean_of_reference_replica_gradients(path, saved):
    """E = K = 4 replicas, n_step 60 / 120: the product's batched update == mean over K independent reference models'
    gradients -> clip -> one RMSProp step (tests/golden/make_golden_nn.py run_batched), host logic on CPU emulation.
    *_ragged: the reference's heterogeneous nets (n_step 12; one with spatial returns) + helpers.check_ragged_batched."""
    from helpers import build_product_batched, check_ragged_batched, compare_batched, drive_batched
    z = load_npz(path)
    with cpu_ops():
        model = build_product_batched(z, 'cpu')
        if saved and not model.policy.can_save_acts:
            pytest.skip('coupled net: the update recomputes its forward pass')
        np.testing.assert_allclose(var_stats_from_named(model.policy.params.ref_variables()), z['stats0'], rtol=1e-6, atol=1e-7)
        out = drive_batched(model, z, saved=saved)
        if str(z['topo']) == 'ragged':
            check_ragged_batched(model, z, out)
    compare_batched(out, z)


def test_batched_update_with_the_encoders_inside_the_lock_step():
    """BatchedTrainer's configuration for IA2C-FP on CACC: compact observations + saved activations, where the policy + value
    launch runs both input encoders itself (`enc_in_kernel`; on this CPU emulation: oracle/ops_ref.step_enc_forward) and no
    encoder launch exists -- against the K = 4 reference-replica golden."""
    from helpers import build_product_batched, compare_batched, drive_batched
    from oracle import ops_ref
    z = load_npz(os.path.join(GOLDEN, 'nnb_ia2c_fp_line.npz'))
    calls = {'n': 0}
    orig = ops_ref.step_enc_forward

    def counting(d):
        calls['n'] += 1
        return orig(d)
    ops_ref.step_enc_forward = counting
    try:
        with cpu_ops():
            model = build_product_batched(z, 'cpu')
            out = drive_batched(model, z, saved=True, compact=True)
            assert model.policy.enc_in_kernel(model.E, True)
    finally:
        ops_ref.step_enc_forward = orig
    assert calls['n'] == 2 * (int(z['n_step']) + 1)          # every lock-step and both bootstrap steps
    compare_batched(out, z)
    # the sign image of the saved LSTM inputs (what the update's one-pass encoder backward reads instead of S on the device): one
    # slot per lock-step, every slot written by the batch that was just consumed, packed as include/nmarl.h lays it out
    from deeprl_network_amd import ops
    assert model.S_bits is not None and tuple(model.S_bits.shape) == (model.n_agent, model.n_step, model.E, 4)
    assert torch.equal(model.S_bits, ops_ref.relu_bits_pack(model.S_buf)) and torch.equal(model.S_bits, ops.relu_bits_pack(model.S_buf))
    S = model.S_buf
    for t_, q, i in ((0, 0, 0), (3, 2, 1), (7, 3, 3)):
        bit = (model.S_bits[..., q].to(torch.int64) >> (4 * t_ + i)) & 1
        assert torch.equal(bit.bool(), S[..., 16 * t_ + 4 * q + i] > 0)


def test_ic3_encoder_inside_the_step_equals_separate_encoder():
    """CommNet on a compact observation with 16-byte feature pieces (the grid's shape): step_policy_value with `ob` (the
    one-launch step runs the observation encoder itself and writes its output to the enc slot) == encode() followed by
    the step on the encoder's output -- the host side of the in-kernel encoder (policies.IC3MultiAgentPolicy._ob_spec)."""
    from deeprl_network_amd import ops
    from deeprl_network_amd.agents.policies import IC3MultiAgentPolicy
    with cpu_ops():
        N, E, F, A = 6, 5, 8, 4
        mask = np.zeros((N, N), dtype=int)
        for i in range(N - 1):                                  # a line: ragged neighbour counts (1 or 2)
            mask[i, i + 1] = mask[i + 1, i] = 1
        np.random.seed(3)
        pol = IC3MultiAgentPolicy(F, A, mask, device='cpu')
        pol.params.init_reference_order()
        pol.refresh_wimage()
        assert pol.encodes_in_step(E, True) and not pol.encodes_in_step(E, False)
        g = torch.Generator().manual_seed(1)
        x = torch.randn(E, N, F, generator=g)
        h, c = torch.randn(N, E, 64, generator=g) * 0.5, torch.randn(N, E, 64, generator=g) * 0.5
        done = (torch.rand(E, generator=g) < 0.4).float()
        outs = []
        for in_step in (True, False):
            enc = torch.full((N, E, 64), 3.0)
            if not in_step:
                pol.encode(x, None, out=enc)
            pi, act, v = torch.zeros(N, E, A), torch.zeros(E, N, dtype=torch.uint8), torch.zeros(N, E)
            ho, co, gates, S = torch.zeros_like(h), torch.zeros_like(c), torch.zeros(N, E, 256), torch.zeros(N, E, 64)
            pol.step_policy_value(enc, h, c, done, pi, act, v, h_out=ho, c_out=co, gates=gates, defer_action_term=True,
                                  save={'S': S}, mode=ops.SAMPLE_PHILOX, seed=4, env_id_base=0, step=2,
                                  **(dict(ob=x) if in_step else {}))
            outs.append((enc, pi, act, v, ho, co, gates, S))
        for a, b in zip(*outs):
            assert torch.equal(a, b)


@pytest.mark.parametrize('agent', ['ia2c', 'ia2c_fp'])
def test_ia2c_on_the_grid_consumes_the_reference_neighbour_order(agent):
    """ATSC envs concatenate an IA2C agent's observation in the order of the reference's `neighbor_map` lists (north, east,
    south, west: atsc_env.py:263-271, large_grid_env.py:58-85), not in ascending node index.  The product given
    `obs_order` must compute, from the env's vectors, the reference's function with the reference's variables (same
    np.random draws under the same names, same values after an update): checked against oracle/nn_ref.py, for which an
    observation is an opaque vector (the critic's neighbour ACTIONS stay in mask order, atsc_env.py:132-136)."""
    from helpers import cacc_config
    from deeprl_network_amd.agents import models
    from deeprl_network_amd.envs.large_grid_env import grid_masks, grid_neighbor_order
    from oracle.nn_ref import REF_MODELS
    nb, dist = grid_masks()
    order = grid_neighbor_order()
    assert order[0] == [5, 1] and order[24] == [19, 23] and order[12] == [17, 13, 7, 11] and order[9] == [14, 4, 8]
    assert any(o != sorted(o) for o in order)
    N, F, A, T = 25, 12, 5, 4
    cp = cacc_config(agent=agent, n_step=T, reward_norm=2000.0, coop_gamma=-1)
    n_s_prod = [F * (1 + len(order[i])) for i in range(N)]
    np.random.seed(5)
    ref = REF_MODELS[agent](n_s_prod, [A] * N, nb, dist, -1.0, cp['MODEL_CONFIG'], dtype=torch.float64)
    rng = np.random.RandomState(0)
    X = rng.rand(T + 1, N, F)
    ACT = rng.randint(0, A, size=(T + 1, N))
    with cpu_ops():
        np.random.seed(5)
        cls = {'ia2c': models.IA2C, 'ia2c_fp': models.IA2C_FP}[agent]
        m = cls(n_s_prod, [A] * N, nb, dist, -1.0, 10000, cp['MODEL_CONFIG'], seed=5, num_envs=1, device='cpu', obs_order=order)
        named0 = m.policy.params.ref_variables()
        assert [k for k, _ in named0] == list(ref.vars.v.keys())
        for (k, a), (_, b) in zip(named0, ref.vars.v.items()):
            np.testing.assert_allclose(a, b.detach().numpy(), rtol=1e-6, atol=1e-7, err_msg=k)
        out = {}
        for name, mod in (('ref', ref), ('prod', m)):
            fp = [np.ones(A) / A for _ in range(N)]
            mod.reset()
            done, PI, V = True, [], []
            for t in range(T + 1):
                ob = [np.concatenate([X[t, i]] + [X[t, j] for j in order[i]] +
                                     ([fp[j] for j in order[i]] if agent == 'ia2c_fp' else [])) for i in range(N)]
                pi = mod.forward(ob, done)
                na = [ACT[t][nb[i] == 1] for i in range(N)]
                v = np.array(mod.forward(ob, done, na, 'v'), dtype=np.float64)
                fp = [np.asarray(p, dtype=np.float64).reshape(-1) for p in pi]
                PI.append(np.stack(fp)); V.append(v)
                if t < T:
                    mod.add_transition(ob, na, ACT[t], -1.0 - 0.1 * t, v, False)
                    done = False
            mod.backward(V[-1], 0)
            out[name] = (np.array(PI), np.array(V))
        np.testing.assert_allclose(out['prod'][0], out['ref'][0], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(out['prod'][1], out['ref'][1], rtol=1e-4, atol=2e-5)
        for (k, a), (_, b) in zip(m.policy.params.ref_variables(), ref.vars.v.items()):
            np.testing.assert_allclose(a, b.detach().numpy(), rtol=1e-3, atol=2e-6, err_msg=k)


def test_greedy_grid_controller_is_the_reference_rule():
    """LargeGridController: the reference's five lane sums (large_grid_env.py:41-45) on a 6-lane vector, and on this env's
    12-link wave vector read at the first link of each physical lane."""
    from deeprl_network_amd.envs.large_grid_env import LargeGridController
    from oracle.grid_ref import LINK_LANE
    rng = np.random.RandomState(3)
    ctl = LargeGridController()
    for _ in range(200):
        lanes = rng.rand(6)
        flows = [lanes[0] + lanes[3], lanes[2] + lanes[5], lanes[1] + lanes[4], lanes[1] + lanes[2], lanes[4] + lanes[5]]
        assert ctl.greedy(lanes) == int(np.argmax(flows))
        assert ctl.greedy(lanes[LINK_LANE]) == int(np.argmax(flows))          # the 12-link form of the same state
    assert ctl.forward([np.zeros(12)] * 25) == [0] * 25

"""Training record on the GPU (csrc/train_record.hip, deeprl_network_amd/train_record.py): the op against its float64
restatement (tests/train_record_ref.py), the ring and the skip_if contract, the record inside the batched trainer -- eager, captured,
guarded -- against the restatement on the trainer's own tensors, the captured update staying kernel-only, and `main.py train`.

Tolerance: rtol = atol = 1e-6 -- float64 sums rounded once to float32 (2^-24 = 6e-8 relative), the traffic record's bound; with
|mean| < 10 std the one-pass variance loses under 1e-13 in float64.  The copied columns (0-2, 4, 5, 13) are compared exactly."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from helpers import cacc_config
from test_train_record_cpu import SIX, WriterStub
from train_record_ref import train_record_ref

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-6, atol=1e-6)
EXACT = [0, 1, 2, 4, 5, 13]


def _inputs(N, rows, A, n_a=None, seed=0, G=None):
    g = np.random.default_rng(seed)
    R = g.normal(-3.0, 2.0, (N, rows)).astype(np.float32)
    V = g.normal(-2.5, 1.5, (N, rows)).astype(np.float32)
    own = np.full(N, A) if n_a is None else np.asarray(n_a)
    return dict(terms=g.normal(0.0, 1.0, (N, 3)).astype(np.float32), gn=g.uniform(0.5, 40.0, N if G is None else G).astype(np.float32),
                R=R, Adv=(R - V).astype(np.float32), act=(g.integers(0, 1 << 30, (rows, N)) % own[None, :]).astype(np.uint8),
                n_a=None if n_a is None else np.asarray(n_a, dtype=np.int32))


def _dev(d):
    return {k: None if v is None else torch.from_numpy(v).cuda() for k, v in d.items()}


def _state(N, rows, K):
    from deeprl_network_amd import ops
    return (torch.zeros(K, N, 24, device='cuda'), torch.zeros(1, dtype=torch.int64, device='cuda'), ops.train_record_ws(N, rows, 'cuda'))


def _call(d, A, ring, count, ws, lr=5e-4, e_coef=0.01, **kw):
    from deeprl_network_amd import ops
    ops.train_record(d['terms'], d['gn'], lr, e_coef, d['R'], d['Adv'], d['act'], ring, count, ws, n_a=d['n_a'], A=A, **kw)


def _check(got, ref):
    got = np.asarray(got, dtype=np.float64)
    print('max abs diff per column:', np.abs(got - ref).max(axis=0).round(10).tolist())
    np.testing.assert_array_equal(got[:, EXACT], ref[:, EXACT])
    np.testing.assert_allclose(got, ref, **TOL)


RAGGED = [2 + (3 * i) % 5 for i in range(28)]            # 2..6


@pytest.mark.parametrize('N,rows,A,n_a', [(1, 1, 2, None), (3, 5, 4, None), (8, 63, 4, None), (8, 64, 4, None), (8, 65, 5, None),
                                          (25, 469, 5, None), (28, 4099, 6, RAGGED)])
def test_op_matches_the_restatement_and_is_reproducible(N, rows, A, n_a):
    assert n_a is None or (min(n_a), max(n_a)) == (2, 6)
    h = _inputs(N, rows, A, n_a, seed=N * 1000 + rows)
    d = _dev(h)
    ring, count, ws = _state(N, rows, 2)
    _call(d, A, ring, count, ws)
    _call(d, A, ring, count, ws)
    torch.cuda.synchronize()
    assert int(count) == 2
    ref = train_record_ref(h['terms'], h['gn'], 5e-4, 0.01, h['R'], h['Adv'], h['act'], h['n_a'] if n_a is not None else [A] * N)
    _check(ring[0].cpu().numpy(), ref)
    assert torch.equal(ring[0], ring[1]), 'two calls on the same inputs differ'
    assert (ring[:, :, 14:16] == 0).all() and (ring[:, :, 16 + A:] == 0).all()
    np.testing.assert_allclose(ring[0, :, 16:].sum(dim=1).cpu().numpy(), 1.0, atol=1e-6)


def test_ring_wraps_and_broadcasts_one_grad_norm_and_lr_dev_overrides_lr():
    N, rows, A, K = 3, 5, 4, 4
    ring, count, ws = _state(N, rows, K)
    lr_dev = torch.full((1,), 2.5e-4, device='cuda')
    hs = [_inputs(N, rows, A, seed=100 + c, G=1) for c in range(6)]
    for h in hs:
        _call(_dev(h), A, ring, count, ws, lr=1.0, lr_dev=lr_dev)
    torch.cuda.synchronize()
    assert int(count) == 6
    got = ring.cpu().numpy()
    for slot, c in enumerate([4, 5, 2, 3]):
        h = hs[c]
        _check(got[slot], train_record_ref(h['terms'], h['gn'], 2.5e-4, 0.01, h['R'], h['Adv'], h['act'], [A] * N))
        assert (got[slot][:, 5] == h['gn'][0]).all() and (got[slot][:, 4] == np.float32(2.5e-4)).all()


def test_skip_if_leaves_ring_and_count_alone():
    N, rows, A, K = 8, 65, 4, 4
    ring, count, ws = _state(N, rows, K)
    word = torch.zeros(1, dtype=torch.int32, device='cuda')          # the test's own word: no fault is injected anywhere
    hs = [_inputs(N, rows, A, seed=200 + c) for c in range(3)]
    _call(_dev(hs[0]), A, ring, count, ws, skip_if=word)
    torch.cuda.synchronize()
    before = (ring.clone(), count.clone())
    assert int(count) == 1 and bool((ring[0] != 0).any()) and not bool((ring[1:] != 0).any())
    word.fill_(1)
    _call(_dev(hs[1]), A, ring, count, ws, skip_if=word)
    torch.cuda.synchronize()
    assert torch.equal(ring, before[0]) and torch.equal(count, before[1])
    word.zero_()
    _call(_dev(hs[2]), A, ring, count, ws, skip_if=word)
    torch.cuda.synchronize()
    assert int(count) == 2 and torch.equal(ring[0], before[0][0]) and not bool((ring[2:] != 0).any())
    h = hs[2]
    _check(ring[1].cpu().numpy(), train_record_ref(h['terms'], h['gn'], 5e-4, 0.01, h['R'], h['Adv'], h['act'], [A] * N))


def test_bad_arguments_are_refused_without_a_launch():
    from deeprl_network_amd import _lib
    d = _dev(_inputs(3, 5, 4))
    ring, count, ws = _state(3, 5, 2)
    with pytest.raises(_lib.NmarlError):
        _call(d, 9, ring, count, ws)                                  # A > 8
    with pytest.raises(_lib.NmarlError):
        _call(d, 4, ring, count, ws[:1])                              # workspace too small
    with pytest.raises(_lib.NmarlError):
        _call(d, 4, ring[:, :2], count, ws)                           # ring of another N
    torch.cuda.synchronize()
    assert int(count) == 0 and not bool((ring != 0).any())


# ------------------------------------------------------------------ inside the trainer
def _build(agent, scenario, E, use_graph, record, **kw):
    if scenario != 'grid2x2':
        from test_gpu_trainer import build
        return build(agent, E, use_graph, scenario=scenario, n_step=20, summary_writer=WriterStub() if record else None,
                     record=record, **kw)
    from deeprl_network_amd.envs import make_batch_env
    from deeprl_network_amd.main import init_agent
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    from test_gpu_grid_shape import shape_config
    cp = shape_config(2, 2, agent=agent, n_step=20)
    env = make_batch_env(cp['ENV_CONFIG'], num_envs=E)
    np.random.seed(12)
    model = init_agent(env, cp['MODEL_CONFIG'], 10 ** 9, 12, num_envs=E)
    return env, model, BatchedTrainer(env, model, Counter(10 ** 12, 10 ** 12, 10 ** 12), use_graph=use_graph,
                                      summary_writer=WriterStub() if record else None, record=record, **kw)


def _row_from_model(model):
    N, n = model.n_agent, model.n_step * model.E
    c = lambda t: t.clone().cpu().numpy()                    # noqa: E731
    gn = c(model.grad_norm)
    return train_record_ref(c(model.loss_terms()), gn if model.per_agent_optimizer else gn[:1], model.cur_lr, model.e_coef,
                            c(model.R).reshape(N, n), c(model.Adv).reshape(N, n), c(model.buf_act).reshape(n, N), model.n_a_ls)


@pytest.mark.parametrize('agent,scenario,E,guarded', [('ia2c_fp', 'catchup', 64, False), ('ma2c_nc', 'slowdown', 64, True),
                                                      ('ma2c_ic3', 'grid2x2', 16, None)])
def test_trainer_records_every_update_and_only_reads(agent, scenario, E, guarded):
    """4 batches, eager and with hipGraphs (an eager first batch, then captured updates): after every batch the ring's newest row
    == the restatement on clones of the model's R, Adv, actions, loss terms, grad_norm and lr; the eager and the graph rings are
    bit-identical; weights, RMSProp slots and actions equal a run with record=False bit for bit."""
    rings, finals = [], []
    for use_graph, record in ((False, True), (True, True), (True, False)):
        env, model, tr = _build(agent, scenario, E, use_graph, record)
        assert (tr.recorder is not None) == record
        if guarded is not None:
            assert tr.handoff_guard == guarded
        for b in range(4):
            tr.run_batch()
            torch.cuda.synchronize()
            if record:
                assert int(tr.recorder.count) == b + 1
                _check(tr.recorder.ring[b].cpu().numpy(), _row_from_model(model))
        assert tr.handoff_fallbacks == 0 and tr.update_capture_error is None and (tr._upd is not None) == use_graph
        if record:
            tr.flush()
            steps, rows = tr.recorder.rows()
            assert steps == [20, 40, 60, 80] and rows.shape == (4, model.n_agent, 24) and np.isfinite(rows).all()
            assert np.array_equal(rows, tr.recorder.ring[:4].cpu().numpy())
            assert tr.recorder.rows()[1].shape[0] == 0                       # drained
            assert (rows[:, :, 13] == 20 * E).all() and (rows[:, :, 7] > 0).all() and (rows[:, :, 12] > 0).all()
            rings.append(rows)
        finals.append((model.policy.params.flat.clone(), model.policy.params.ms.clone(), model.buf_act.clone()))
        del env, model, tr
    assert np.array_equal(rings[0], rings[1]), 'the captured record differs from the eager one'
    for k, (a, b, c) in enumerate(zip(*finals)):
        assert torch.equal(a, c) and torch.equal(b, c), 'the record changed what the update computes (item %d)' % k


def test_recorder_refuses_an_overrun_and_a_step_mismatch():
    from deeprl_network_amd import _lib
    env, model, tr = _build('ia2c_fp', 'catchup', 16, False, True, record_slots=2)
    for _ in range(2):
        tr.run_batch()
    assert len(tr.recorder.rows()[0]) == 2
    tr.run_batch()
    tr.recorder.steps.pop()
    with pytest.raises(_lib.NmarlError, match='out of step'):
        tr.recorder.rows()
    tr.recorder.steps = [1, 2, 3]
    for _ in range(2):
        tr.run_batch()
    with pytest.raises(_lib.NmarlError, match='overrun'):
        tr.recorder.rows()
    with pytest.raises(AssertionError):
        tr.run(log_every=3)


def test_captured_update_with_the_record_holds_kernel_nodes_only():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import graph_nodes as G
    counts = {}
    for record in (True, False):
        env, model, tr = _build('ia2c_fp', 'catchup', 64, True, record, keep_graphs=True)
        for _ in range(3):
            tr.run_batch()
        torch.cuda.synchronize()
        assert tr._upd is not None and tr._upd['apply'] is None and tr.update_capture_error is None
        c = G.census(tr._upd['grads'])
        assert set(c) == {'kernel'}, c
        counts[record] = c['kernel']
        del env, model, tr
    assert 1 <= counts[True] - counts[False] <= 2, counts


def test_cli_train_writes_the_scalars_and_the_summary_table(tmp_path):
    import pandas as pd
    from deeprl_network_amd.main import main
    cp = cacc_config(agent='ia2c_fp', n_step=20, reward_norm=800.0, total_step=120)
    cp['ENV_CONFIG']['episode_length_sec'] = '6'
    ini = tmp_path / 'config_ia2c_fp_catchup.ini'
    with open(ini, 'w') as f:
        cp.write(f)
    base = str(tmp_path / 'run')
    main(['--base-dir', base, 'train', '--config-dir', str(ini), '--num-envs', '16'])
    df = pd.read_csv(base + '/data/train_summary.csv')
    assert list(df.columns) == ['step', 'agent_id', 'policy_loss', 'value_loss', 'entropy_loss', 'total_loss', 'lr', 'gradnorm', 'ret_mean',
                                'ret_std', 'value_mean', 'explained_var', 'adv_mean', 'adv_std', 'entropy', 'share_0', 'share_1', 'share_2',
                                'share_3']
    assert len(df) == 6 * 8 and np.isfinite(df.to_numpy(dtype=np.float64)).all()
    assert list(df['step']) == [s for s in range(20, 121, 20) for _ in range(8)] and list(df['agent_id']) == list(range(8)) * 6
    rows = [json.loads(line) for line in open(base + '/log/scalars.jsonl')]
    for tag in SIX:
        steps = [r['step'] for r in rows if r['tag'] == tag % 'lstm_0']
        assert steps == list(range(20, 121, 20)), (tag, steps)
    a0 = df[df['agent_id'] == 0]
    assert [r['value'] for r in rows if r['tag'] == 'loss/lstm_0_policy_loss'] == pytest.approx(list(a0['policy_loss']), rel=1e-6)
    reward = pd.read_csv(base + '/data/train_reward.csv')
    assert list(reward.columns) == ['Unnamed: 0', 'agent', 'step', 'test_id', 'avg_reward', 'std_reward', 'train_avg_reward',
                                    'train_std_reward', 'episodes', 'collisions', 'env_steps', 'wall_s', 'test_collisions', 'evaluated']
    assert sum(r['tag'] == 'train_reward' for r in rows) == len(reward)

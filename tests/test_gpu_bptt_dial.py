"""nmarl_lstm_bptt_dial: the whole reverse recurrence of lstm_dial (agents/utils.py:561-593, policies.py:479-525) in one launch,
the message adjoint handed between the agents' blocks inside the kernel -- against a float64 reference composed from the
restatements that exist (oracle/ops_ref.py: bptt_step for the cell backward and the transposed product, dial_msg_adjoint for the
message path, per reverse step), its two forms against each other, and the engine's dial branch against the step-wise pair it
replaces."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 64


def _forward_cells(gates, c0, done):
    """c[t + 1] = gf * (c[t] * keep_t) + gi * gu in float32, operation for operation what the forward kernels compute: the
    one-launch BPTT kernels recompute c_t from the gates, so their inputs must be a consistent forward trace."""
    N, T, E, H4 = gates.shape
    call = torch.empty(N, T + 1, E, H)
    call[:, 0] = c0
    for t in range(T):
        keep = (1.0 - done[t]).view(1, E, 1)
        call[:, t + 1] = gates[:, t, :, H:2 * H] * (call[:, t] * keep) + gates[:, t, :, :H] * gates[:, t, :, 3 * H:]
    return call


def _table(N, topo):
    """line: the CACC neighbour table (m_max = 2; N = 2: m_max = 1).  ragged: the asymmetric -1 padded 6-agent table of
    test_dial_msg_adjoint with the fan-in capped at 2 (agent 3 keeps two of its four sources; agent 5 has none at all)."""
    from deeprl_network_amd import ops
    if topo == 'ragged':
        assert N == 6
        idx = -torch.ones(N, 2, dtype=torch.int32)
        idx[0, 0], idx[1, 0], idx[1, 1], idx[2, 0], idx[4, 0], idx[4, 1] = 3, 0, 3, 1, 1, 2
        return idx
    nm = np.zeros((N, N), dtype=int)
    for i in range(N - 1):
        nm[i, i + 1] = nm[i + 1, i] = 1
    return ops.neighbor_table(nm, 'cpu')[0]


def _inputs(N, T, E, topo, seed, O=None):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                         # noqa: E731
    idx = _table(N, topo)
    m_max = idx.shape[1]
    d = dict(idx=idx, m_max=m_max)
    d['gates'] = torch.cat([torch.sigmoid(r(N, T, E, 3 * H)), torch.tanh(r(N, T, E, H))], dim=-1)
    d['done'] = (torch.rand(T, E, generator=g) < 0.2).float()
    d['call'] = _forward_cells(d['gates'], r(N, E, H) * 0.8, d['done'])
    if O is None:
        d['dhs'] = r(N, T, E, H)
    else:
        d['dy8'] = torch.zeros(N, T * E, 8)
        d['dy8'][:, :, :O] = r(N, T * E, O)
        d['hw'] = r(N, H, O) * 0.3
        d['dhs'] = torch.bmm(d['dy8'][:, :, :O].double(), d['hw'].double().transpose(1, 2)).float().view(N, T, E, H)
    d['wx'], d['wh'] = r(N, H, 4 * H) * 0.1, r(N, H, 4 * H) * 0.1
    d['w_msg'], d['mfc_w'] = r(N, H * m_max, H) * 0.15, r(N, H, H) * 0.2
    d['hm'], d['msg'] = torch.relu(r(N, T, E, H)), torch.relu(r(N, T, E, H))
    return d


def _reference(d):
    """float64, per reverse step: ops_ref.bptt_step (cell backward, [ds | dh] = dz [wx; wh]^T, dh * keep) then
    ops_ref.dial_msg_adjoint (both relu masks, gather adjoint, dh + d2 mfc_w^T) -- the loop of agents/sequence.py, composed in
    oracle/ops_ref.py as bptt_dial."""
    from oracle import ops_ref
    f = lambda t: t.double()                                                            # noqa: E731
    N, T, E, _ = d['gates'].shape
    dZ = torch.zeros(N, T, E, 4 * H, dtype=torch.float64)
    DS, D1, D2 = (torch.zeros(N, T, E, H, dtype=torch.float64) for _ in range(3))
    db, dbm, dbf, dh0, dc0 = ops_ref.bptt_dial(ops_ref.reverse_neighbor_table(d['idx'], ops_ref.COUPLED_NC), d['m_max'], f(d['gates']),
                                               f(d['call']), f(d['done']), f(d['dhs']), (f(d['wx']), f(d['wh']), None),
                                               (f(d['w_msg']), None), f(d['mfc_w']), f(d['hm']), f(d['msg']), dZ, DS, D1, D2,
                                               want_state_grad=True)
    return dict(dZ=dZ, DS=DS, D1=D1, D2=D2, db=db, dbm=dbm, dbf=dbf, dh0=dh0, dc0=dc0)


def _run(d, mode, head_dy=False):
    """ops.bptt_dial on slots of wider allocations (guard slabs around every sequence operand)."""
    from deeprl_network_amd import ops
    N, T, E, _ = d['gates'].shape
    cu = lambda t: t.cuda()                                                             # noqa: E731
    G = torch.zeros(N, T + 2, E, 4 * H, device='cuda'); G[:, 1:T + 1].copy_(d['gates'])             # noqa: E702
    C = torch.zeros(N, T + 3, E, H, device='cuda'); C[:, 1:T + 2].copy_(d['call'])                  # noqa: E702
    D = torch.zeros(N, T + 1, E, H, device='cuda'); D[:, :T].copy_(d['dhs'])                        # noqa: E702
    HM = torch.zeros(N, T, E, 3 * H, device='cuda'); HM[..., H:2 * H].copy_(d['hm'])                # noqa: E702
    MSG = torch.zeros(N, T + 1, E, H, device='cuda'); MSG[:, :T].copy_(d['msg'])                    # noqa: E702
    wx, wh, w_msg, mfc_w = cu(d['wx']), cu(d['wh']), cu(d['w_msg']), cu(d['mfc_w'])
    ws = (wx, wh, ops.lstm_bptt_wimage(wx, wh))
    wm = (w_msg, ops.lstm_bptt_msg_wimage(w_msg))
    img_f = ops.lstm_bptt_msg_wimage(mfc_w)
    rev = ops.reverse_neighbor_table(cu(d['idx']), ops.COUPLED_NC)
    assert ops.bptt_dial_supported(d['m_max'], H, rev=rev)
    dZ = torch.zeros(N, T + 2, E, 4 * H, device='cuda')
    DS, D1, D2 = (torch.zeros(N, T + 2, E, H, device='cuda') for _ in range(3))
    hd = (cu(d['dy8']), cu(d['hw'])) if head_dy else None
    db, dbm, dbf, dh0, dc0 = ops.bptt_dial(rev, d['m_max'], G[:, 1:T + 1], C[:, 1:T + 2], cu(d['done']), None if head_dy else D[:, :T], ws, wm,
                                           img_f, HM[..., H:2 * H], MSG, dZ[:, 1:T + 1], DS[:, 1:T + 1], D1[:, 1:T + 1], D2[:, 1:T + 1],
                                           mode=mode, head_dy=hd, want_state_grad=True)
    torch.cuda.synchronize()
    ops.check_coupled_status()
    for x in (dZ, DS, D1, D2):
        assert torch.all(x[:, 0] == 0) and torch.all(x[:, T + 1] == 0), 'a guard slab was written'
    return dict(dZ=dZ[:, 1:T + 1].clone(), DS=DS[:, 1:T + 1].clone(), D1=D1[:, 1:T + 1].clone(), D2=D2[:, 1:T + 1].clone(), db=db, dbm=dbm,
                dbf=dbf, dh0=dh0, dc0=dc0)


def _resident(N, E):
    return N * -(-E // 128) <= torch.cuda.get_device_properties(0).multi_processor_count


SHAPES = [(8, 12, 4096, 'line'), (8, 60, 300, 'line'), (3, 5, 127, 'line'), (2, 3, 1, 'line'), (6, 4, 77, 'ragged')]


@pytest.mark.parametrize('N,T,E,topo', SHAPES)
def test_bptt_dial_against_float64(N, T, E, topo):
    """dZ, DS, D1, D2, the three bias gradients and the final dL/dh0, dL/dc0 of ops.bptt_dial against the float64 composition of
    ops_ref.bptt_step + ops_ref.dial_msg_adjoint per step (tolerances of test_lstm_bptt_coupled_one_launch); D1 / D2 exactly zero
    where their relu masks are; the one-launch form is forced (mode 1) where the grid is resident, so the in-kernel hand-off runs."""
    d = _inputs(N, T, E, topo, N * 131 + T * 7 + E)
    ref = _reference(d)
    got = _run(d, 1 if _resident(N, E) else 0)
    for k in ('dZ', 'DS', 'D1', 'D2', 'dh0', 'dc0'):
        err = (got[k].cpu().double() - ref[k]).abs().max().item()
        print('%s: max |diff| %.3e (|ref| max %.3e)' % (k, err, ref[k].abs().max().item()))
        torch.testing.assert_close(got[k].cpu().double(), ref[k], rtol=2e-4, atol=5e-5, msg=lambda m, k=k: '%s: %s' % (k, m))
    for k in ('db', 'dbm', 'dbf'):
        print('%s: max |diff| %.3e' % (k, (got[k].cpu().double() - ref[k]).abs().max().item()))
        torch.testing.assert_close(got[k].cpu().double(), ref[k], rtol=1e-4, atol=1e-4 * max(1.0, float(ref[k].abs().max())),
                                   msg=lambda m, k=k: '%s: %s' % (k, m))
    assert torch.all(got['D1'].cpu()[d['hm'] <= 0] == 0)
    assert torch.all(got['D2'].cpu()[d['msg'] <= 0] == 0)


@pytest.mark.parametrize('N,T,E,topo', SHAPES)
def test_bptt_dial_forms_agree(N, T, E, topo):
    """One launch (mode 1) and T + 1 step-wise launches (mode 2) of the same kernel: dZ, DS, D1, D2 bit for bit, bias sums within
    summation order; the status word clean after each (checked in _run).  The dy8 form against the tensor form dy8 @ hw^T in both
    modes at the tolerance of test_lstm_bptt_coupled_expands_the_heads_gradient_itself."""
    if not _resident(N, E):
        pytest.skip('the grid is not resident at once on this device')
    d = _inputs(N, T, E, topo, N * 31 + T * 5 + E, O=5)
    out = {(form, mode): _run(d, mode, head_dy=form == 'dy8') for form in ('tensor', 'dy8') for mode in (1, 2)}
    for form in ('tensor', 'dy8'):
        a, b = out[form, 1], out[form, 2]
        for k in ('dZ', 'DS', 'D1', 'D2'):
            n = (a[k] != b[k]).sum().item()
            assert n == 0, '%s form, %s: one launch and step-wise launches differ in %d entries' % (form, k, n)
        for k in ('db', 'dbm', 'dbf'):
            torch.testing.assert_close(a[k], b[k], rtol=1e-5, atol=1e-5 * (T * E) ** 0.5)
        assert torch.equal(a['dh0'], b['dh0']) and torch.equal(a['dc0'], b['dc0'])
    for mode in (1, 2):
        for k in ('dZ', 'DS', 'D1', 'D2', 'db', 'dbm', 'dbf'):
            x, y = out['dy8', mode][k], out['tensor', mode][k]
            torch.testing.assert_close(x, y, rtol=5e-5, atol=5e-6 * float(y.abs().max()), msg=lambda m, k=k: '%s: %s' % (k, m))


@pytest.mark.parametrize('E', [300, 4096])
def test_sequence_new_op_equals_step_wise_pair(E, monkeypatch):
    """coupled_sequence_saved for lstm_dial through nmarl_lstm_bptt_dial and, with the predicate patched to False, through the
    step-wise pair it replaces: the gradients of every parameter and of enc at the bounds of test_gpu_sequence.py (relative
    L2 <= 1e-3, max entry <= 2e-2 * scale: its docstring explains why relu kinks forbid tighter ones).  coupled_sequence_saved has no
    h0 / c0 inputs (the rollout owns the state), so dL/dh0 and dL/dc0 are compared where they exist: at the op, in
    test_bptt_dial_against_float64."""
    from deeprl_network_amd import ops
    from deeprl_network_amd.agents import sequence
    N, T = 8, 6
    d = _inputs(N, T, E, 'line', 77 + E)
    g = torch.Generator().manual_seed(E)
    cu = lambda t: t.cuda()                                                             # noqa: E731
    idx = cu(d['idx'])
    Hall = cu(torch.randn(N, T + 1, E, H, generator=g) * 0.3)
    S = cu(torch.randn(N, T, E, H, generator=g))
    w = cu(torch.randn(N, T, E, H, generator=g))
    done = d['done'].clone()
    done[1:] = 0.0                                                     # masked_steps = (0,): later steps carry no done by contract
    call = _forward_cells(d['gates'], d['call'][:, 0], done)
    calls = []
    real = ops.bptt_dial

    def run(new):
        if not new:
            monkeypatch.setattr(ops, 'bptt_dial_supported', lambda *a, **k: False)
        monkeypatch.setattr(ops, 'bptt_dial', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
        prm = [cu(d[k]).clone().requires_grad_(True) for k in ('wx', 'wh', 'w_msg', 'mfc_w')]
        wx, wh, w_msg, mfc_w = prm
        b, b_msg, mfc_b = (torch.zeros(N, n, device='cuda', requires_grad=True) for n in (4 * H, H, H))
        enc = torch.zeros(N, T, E, H, device='cuda', requires_grad=True)
        Hs = sequence.coupled_sequence_saved('dial', idx, (0,), enc, cu(done), wx, wh, b, w_msg, b_msg, mfc_w, mfc_b, cu(d['gates']),
                                             Hall.clone(), cu(call), S, dict(A1=cu(d['hm']), A2=cu(d['msg'])))
        (Hs * w).sum().backward()
        torch.cuda.synchronize()
        ops.check_coupled_status()
        return [t.grad.detach().cpu() for t in prm + [b, b_msg, mfc_b, enc]]
    got = run(True)
    assert calls == [1], 'the dial branch did not take nmarl_lstm_bptt_dial'
    want = run(False)
    assert calls == [1]
    for a, b_, name in zip(got, want, ['wx', 'wh', 'w_msg', 'mfc_w', 'b', 'b_msg', 'mfc_b', 'enc']):
        rel_l2 = ((a - b_).norm() / b_.norm().clamp_min(1e-12)).item()
        err, scale = (a - b_).abs().max().item(), b_.abs().max().item()
        print('%s: rel L2 %.3e, max |diff| %.3e, scale %.3e' % (name, rel_l2, err, scale))
        assert rel_l2 <= 1e-3, '%s: relative L2 error %.3e' % (name, rel_l2)
        assert err <= 2e-2 * max(scale, 1.0), '%s: max |diff| %.3e vs scale %.3e' % (name, err, scale)


def _trainer(E, use_graph, n_step=20, **kw):
    from test_gpu_trainer import build
    return build('ma2c_dial', E, use_graph, scenario='catchup', n_step=n_step, **kw)


def _two_batches(E, use_graph, **kw):
    from deeprl_network_amd import ops
    env, model, tr = _trainer(E, use_graph, **kw)
    for _ in range(2):
        tr.run_batch()
    tr.flush()
    torch.cuda.synchronize()
    ops.check_coupled_status()
    assert tr.handoff_fallbacks == 0
    return env, model, tr


@pytest.mark.parametrize('E', [512, 4096])
def test_trainer_one_launch_bptt(E, monkeypatch):
    """DIAL catch-up, n_step 20, two batches: hipGraph == eager bit for bit and two runs identical; every captured graph is kernel
    nodes only; weights equal the old path's (predicate patched to False) within the bound of
    test_coupled_one_launch_step_equals_two_launches; the update graph lost at least 2 (n_step - 1) kernel nodes; the heads'
    gradient travels as dy8 on the new path."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import graph_nodes as G
    from deeprl_network_amd import ops
    T = 20
    runs, nodes = [], {}
    for use_graph in (True, False, True):
        env, model, tr = _two_batches(E, use_graph, keep_graphs=True)
        assert model.policy.bptt_takes_head_dy is True
        runs.append((model.policy.params.flat.clone(), env.state_tensors()[0].clone(), model.buf_act.clone()))
        if use_graph:
            assert tr.graph is not None and tr._upd is not None and tr.update_capture_error is None
            graphs = {'rollout': tr.graph, 'update': tr._upd['grads']}
            if tr._upd['apply'] is not None:
                graphs['apply'] = tr._upd['apply']
            for what, g in graphs.items():
                c = G.census(g)
                assert c.get('kernel', 0) > 0 and set(c) == {'kernel'}, '%s graph holds non-kernel nodes: %s' % (what, c)
            nodes['new'] = G.census(tr._upd['grads'])['kernel']
        del env, model, tr
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b), 'hipGraph replay differs from eager launches'
    for a, b in zip(runs[0], runs[2]):
        assert torch.equal(a, b), 'two identical runs differ'
    monkeypatch.setattr(ops, 'bptt_dial_supported', lambda *a, **k: False)
    env, model, tr = _two_batches(E, True, keep_graphs=True)
    assert model.policy.bptt_takes_head_dy is False
    nodes['old'] = G.census(tr._upd['grads'])['kernel']
    print('update graph kernel nodes: old path %d, new path %d' % (nodes['old'], nodes['new']))
    torch.testing.assert_close(runs[0][0], model.policy.params.flat, rtol=1e-4, atol=2e-6)
    assert nodes['old'] - nodes['new'] >= 2 * (T - 1)


def test_trainer_picks_the_step_wise_form_on_a_smaller_device(monkeypatch):
    """NMARL_TEST_FAKE_CUS=16 at E = 512 (8 x 4 blocks > 16 CUs): the engine takes the step-wise form of the same kernel by itself and
    the batches finish clean."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import graph_nodes as G
    from deeprl_network_amd import _lib
    T = 20
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert _lib.lib.nmarl_handoff_capacity(3, 128) == cus and _lib.lib.nmarl_handoff_capacity(3, 64) == cus
    env, model, tr = _two_batches(512, True, keep_graphs=True)
    one = G.census(tr._upd['grads'])['kernel']
    w_one = model.policy.params.flat.clone()
    del env, model, tr
    monkeypatch.setenv('NMARL_TEST_FAKE_CUS', '16')
    assert _lib.lib.nmarl_handoff_capacity(3, 128) == 16 and _lib.lib.nmarl_handoff_capacity(3, 64) == 16
    env, model, tr = _two_batches(512, True, keep_graphs=True)
    step = G.census(tr._upd['grads'])['kernel']
    print('update graph kernel nodes: one launch %d, step-wise %d' % (one, step))
    assert step - one == T, 'the step-wise form is T + 1 launches of the kernel where the one-launch form is 1'
    assert torch.isfinite(model.policy.params.flat).all()
    torch.testing.assert_close(model.policy.params.flat, w_one, rtol=1e-4, atol=2e-6)       # same kernel; the bias sums' order differs


@pytest.fixture
def handoff_switch():
    """The recovery pins the launch-per-step kernels process-wide: give the following tests the one-launch forms back."""
    from deeprl_network_amd import _lib, ops
    yield
    ops._handoff_off[0] = False
    _lib.lib.nmarl_test_handoff_fault(0)
    for st in ops._handoff_status.values():
        st.zero_()


def test_dial_bptt_handoff_timeout_fails_closed(handoff_switch, monkeypatch):
    """test_handoff_timeout_fails_closed for the DIAL BPTT launch (the only in-launch hand-off of a DIAL batch, so the first hand-off
    launch after arming): a bounded time-out injected once; the refused batches change no weight and no optimiser slot, the trainer
    notices one batch late and recovers onto the step-wise form; after three batches weights, slots and env state equal bit for bit
    a run with NMARL_INKERNEL_HANDOFF=0."""
    from deeprl_network_amd import _lib, ops
    from deeprl_network_amd.utils import BatchedTrainer
    E, T = 256, 10
    monkeypatch.setenv('NMARL_INKERNEL_HANDOFF', '0')
    env, model, tr = _trainer(E, False, n_step=T)
    assert not tr.handoff_guard
    for _ in range(3):
        tr.run_batch()
    torch.cuda.synchronize()
    ref = (model.policy.params.flat.clone(), model.policy.params.ms.clone(), env.state_tensors()[0].clone(), model.buf_act.clone())
    del env, model, tr
    monkeypatch.delenv('NMARL_INKERNEL_HANDOFF')
    env, model, tr = _trainer(E, False, n_step=T)
    assert tr.handoff_guard
    w0, ms0 = model.policy.params.flat.clone(), model.policy.params.ms.clone()
    seen = {}
    orig = BatchedTrainer._recover_from_handoff_timeout

    def spy(self, batches=1):
        torch.cuda.synchronize()
        seen['w'], seen['ms'], seen['batches'] = self.model.policy.params.flat.clone(), self.model.policy.params.ms.clone(), batches
        orig(self, batches)
    monkeypatch.setattr(BatchedTrainer, '_recover_from_handoff_timeout', spy)
    _lib.check(_lib.lib.nmarl_test_handoff_fault(1), 'nmarl_test_handoff_fault')
    tr.run_batch()
    assert tr.handoff_fallbacks == 0 and not seen, 'the host looked at the status word of the batch it had just launched'
    tr.run_batch()
    assert tr.handoff_fallbacks == 1 and not ops.handoff_enabled() and not tr.handoff_guard
    assert seen['batches'] == 2
    assert torch.equal(seen['w'], w0) and torch.equal(seen['ms'], ms0), 'a refused batch reached the weights'
    tr.run_batch()
    tr.flush()
    torch.cuda.synchronize()
    ops.check_coupled_status()
    got = (model.policy.params.flat, model.policy.params.ms, env.state_tensors()[0], model.buf_act)
    for name, a, b in zip(('weights', 'rmsprop slots', 'env state', 'actions'), got, ref):
        assert torch.equal(a, b), '%s differ from the launch-per-step run' % name
    assert tr.n_batches == 3

"""The kernels that heterogeneous nets (the reference's identical=False nets: agents with different action counts) reach through
the padded arrangement of agents/policies.py -- absent actions carry zero weight columns and a -1e30 logit bias, absent critic
inputs zero weight rows -- at the row counts where the kernels' row handling changes, against float64 restatements of the
REFERENCE's own definition: a softmax / loss over each agent's first n_a_i logits only (policies.py:241-254 with n_a_ls), the
critic's one-hots n_a_j wide per neighbour (policies.py:59-77 with na_dim_ls).  Deliberately not the padded formula.

N = 5 agents on the neighbourhood of tests/golden/make_golden_nn.ragged_graph() (agent 2 has three neighbours, agent 4 none);
(A, n_a) are the three instantiations of the step kernel's actor head (csrc/lstm_mfma.hip head_policy_lds: <4>, <8,5>, <8>)."""
import functools

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

H = 64
N = 5
NBR = [[1, 2], [0, 2], [0, 1, 3], [2], []]
M_MAX = 3
SHAPES = {4: [2, 3, 4, 4, 3], 5: [2, 3, 4, 2, 5], 8: [2, 5, 8, 7, 6]}
U_BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))


def _nbr_idx():
    idx = -torch.ones(N, M_MAX, dtype=torch.int32)
    for i, js in enumerate(NBR):
        idx[i, :len(js)] = torch.tensor(js, dtype=torch.int32)
    return idx


def _padded_heads(A, g):
    """Head parameters as ParamStore pads them (policies._head_phase): the reference's ragged variables -- pi/w [H,n_a_i],
    pi/b [n_a_i], v/w [H + sum_j n_a_j, 1] -- in float32, and the padded tensors built from them."""
    n_a = SHAPES[A]
    r = lambda *s: torch.randn(*s, generator=g)                                         # noqa: E731
    rag = dict(pi_w=[r(H, n_a[i]) * 0.5 for i in range(N)], pi_b=[r(n_a[i]) * 0.3 for i in range(N)],
               v_h=[r(H) * 0.3 for i in range(N)], v_nb=[[r(n_a[j]) for j in NBR[i]] for i in range(N)], v_b=[r(1) for i in range(N)])
    pi_w, pi_b = torch.zeros(N, H, A), torch.full((N, A), -1e30)
    v_w, v_b = torch.zeros(N, H + M_MAX * A, 1), torch.zeros(N, 1)
    for i in range(N):
        pi_w[i, :, :n_a[i]] = rag['pi_w'][i]
        pi_b[i, :n_a[i]] = rag['pi_b'][i]
        v_w[i, :H, 0] = rag['v_h'][i]
        for k, j in enumerate(NBR[i]):
            v_w[i, H + k * A:H + k * A + n_a[j], 0] = rag['v_nb'][i][k]
        v_b[i] = rag['v_b'][i]
    return rag, dict(pi_w=pi_w, pi_b=pi_b, v_w=v_w, v_b=v_b)


# --------------------------------------------------------------------------- the lock-step kernel's actor head and draw
@functools.lru_cache(maxsize=None)
def _step_case(A, E, mode):
    """Inputs and the float64 reference of one policy step (computed once, shared by the tests below, never written to)."""
    from oracle import ops_ref
    n_a = SHAPES[A]
    g = torch.Generator().manual_seed(1000 * A + 10 * E + mode)
    r = lambda *s: torch.randn(*s, generator=g)                                         # noqa: E731
    h, c, z1 = r(N, E, H) * 0.7, r(N, E, H), r(N, E, 4 * H)
    done = (torch.rand(E, generator=g) < 0.3).float()
    wh, b = r(N, H, 4 * H) * 0.2, r(N, 4 * H) * 0.1
    rag, pad = _padded_heads(A, g)
    u = torch.rand(E, N, generator=g)
    u[0::3] = 0.0                                            # the CDF's two edges: np.random.random_sample() is in [0, 1)
    u[1::3] = U_BELOW_ONE
    assert float(u.max()) < 1.0
    draw = dict(mode=mode, u=u if mode == 0 else None, seed=77, env_id_base=1000, step=5)
    d = lambda t: t.double()                                                            # noqa: E731
    hr, cr = torch.empty(N, E, H, dtype=torch.float64), torch.empty(N, E, H, dtype=torch.float64)
    ops_ref.lstm_step_fused(d(h), d(wh), d(b), d(z1), None, d(c), d(done), None, cr, hr)
    pir = torch.zeros(N, E, A, dtype=torch.float64)
    for i in range(N):                                       # the reference's actor head: n_a_i outputs, nothing else exists
        pir[i, :, :n_a[i]] = torch.softmax(hr[i] @ d(rag['pi_w'][i]) + d(rag['pi_b'][i]), dim=-1)
    actr = torch.zeros(E, N, dtype=torch.uint8)
    ops_ref.sample_actions(pir, actr, **draw)
    return dict(A=A, E=E, n_a=n_a, h=h, c=c, z1=z1, done=done, wh=wh, b=b, rag=rag, pad=pad, draw=draw, hr=hr, cr=cr, pir=pir,
                actr=actr)


def _value_ref(case, act):
    """forward('v') in float64 from the reference's ragged critic weights: the re-step from (h', c') with the same addend
    (quirk Q1), then v = h'' . w_h + sum_k w_k[a_{j_k}] + b with one n_a_j-wide one-hot block per neighbour."""
    from oracle import ops_ref
    d = lambda t: t.double()                                                            # noqa: E731
    E, rag = case['E'], case['rag']
    h2, c2 = torch.empty_like(case['hr']), torch.empty_like(case['cr'])
    ops_ref.lstm_step_fused(case['hr'], d(case['wh']), d(case['b']), d(case['z1']), None, case['cr'], d(case['done']), None, c2, h2)
    v = torch.zeros(N, E, dtype=torch.float64)
    for i in range(N):
        v[i] = h2[i] @ d(rag['v_h'][i]) + d(rag['v_b'][i])
        for k, j in enumerate(NBR[i]):
            assert int(act[:, j].max()) < case['n_a'][j]
            v[i] += d(rag['v_nb'][i][k])[act[:, j].long()]
    return v


STEP_CASES = [(A, E, mode) for A in (4, 5, 8) for E in (1, 17, 130) for mode in (0, 2)]


@pytest.mark.parametrize('A,E,mode', STEP_CASES)
def test_float64_side_of_the_step_cases_is_exact(A, E, mode):
    """(CPU) The reference side alone meets the exact conditions for the chosen seeds: its draws never leave an agent's own
    action set -- at u = 0 and at the largest float32 below 1 in particular -- its padded columns are exactly 0, and the padded
    float64 formula (what the oracle restatement computes from the padded parameters) gives the same probabilities and draws."""
    from oracle import ops_ref
    case = _step_case(A, E, mode)
    n_a, pir, actr = case['n_a'], case['pir'], case['actr']
    for i in range(N):
        assert int(actr[:, i].max()) < n_a[i]
        assert torch.all(pir[i, :, n_a[i]:] == 0) and torch.all(pir[i, :, :n_a[i]] > 0)
    torch.testing.assert_close(pir.sum(-1), torch.ones(N, E, dtype=torch.float64), rtol=0, atol=1e-12)
    pad = case['pad']
    pip = torch.softmax(torch.bmm(case['hr'], pad['pi_w'].double()) + pad['pi_b'].double().unsqueeze(1), dim=-1)
    torch.testing.assert_close(pip, pir, rtol=1e-12, atol=0)
    actp = torch.zeros(E, N, dtype=torch.uint8)
    ops_ref.sample_actions(pip, actp, **case['draw'])
    assert torch.equal(actp, actr)
    if mode == 0:                                            # the edges themselves: the first action, and the agent's LAST one
        u = case['draw']['u']
        assert torch.all(actr[u == 0] == 0)
        last = torch.tensor(n_a, dtype=torch.uint8).view(1, N).expand(E, N) - 1
        assert torch.equal(actr[u == U_BELOW_ONE], last[u == U_BELOW_ONE])


def _check_policy_half(case, hg, cg, pig, actg):
    from oracle import ops_ref
    A, E, n_a = case['A'], case['E'], case['n_a']
    torch.testing.assert_close(hg.cpu().double(), case['hr'], rtol=2e-5, atol=2e-6)
    torch.testing.assert_close(cg.cpu().double(), case['cr'], rtol=2e-5, atol=2e-6)
    pi, act = pig.cpu(), actg.cpu()
    for i in range(N):
        torch.testing.assert_close(pi[i, :, :n_a[i]].double(), case['pir'][i, :, :n_a[i]], rtol=2e-5, atol=2e-6)
        assert torch.all(pi[i, :, n_a[i]:] == 0), 'agent %d: probability in a padded column' % i
        assert int(act[:, i].max()) < n_a[i], 'agent %d drew an action it does not have' % i
    # the draw, bit for bit given the kernel's own probabilities; against the float64 softmax' draw a CDF boundary within an
    # ulp of u may differ (the cap of test_gpu_ops.test_lstm_step_fused_heads)
    chk = torch.zeros(E, N, dtype=torch.uint8)
    ops_ref.sample_actions(pi, chk, **case['draw'])
    assert torch.equal(act, chk)
    assert (act != case['actr']).float().mean() < 1e-3
    return act


@gpu
@pytest.mark.parametrize('A,E,mode', STEP_CASES)
def test_step_policy_on_padded_action_sets(A, E, mode):
    """ops.lstm_step_policy, KX = 0 form with one addend, in place: E = 1 / 17 / 130 rows = a partial 16-row strip, a strip plus
    one row, a 128-row block plus two rows."""
    from deeprl_network_amd import ops
    case = _step_case(A, E, mode)
    cu = lambda t: None if t is None else t.cuda()                                      # noqa: E731
    pad = case['pad']
    hg, cg = cu(case['h']), cu(case['c'])
    pig = torch.full((N, E, A), 7.0, device='cuda')
    actg = torch.full((E, N), 255, dtype=torch.uint8, device='cuda')
    ops.lstm_step_policy(hg, cu(case['wh']), cu(case['b']), cu(case['z1']), None, cg, cu(case['done']), cg, hg, cu(pad['pi_w']),
                         cu(pad['pi_b']), pig, actg, **dict(case['draw'], u=cu(case['draw']['u'])))
    _check_policy_half(case, hg, cg, pig, actg)


@gpu
@pytest.mark.parametrize('A,E,mode', STEP_CASES)
def test_step_policy_value_on_padded_action_sets(A, E, mode):
    """ops.lstm_step_policy_value (the fused policy + value launch `act` / `bootstrap` run): the policy half as above, and v from
    the re-step with the neighbours' one-hots at the padded width A == the reference's critic on n_a_j-wide one-hots."""
    from deeprl_network_amd import ops
    case = _step_case(A, E, mode)
    cu = lambda t: None if t is None else t.cuda()                                      # noqa: E731
    pad = case['pad']
    hg, cg = cu(case['h']), cu(case['c'])
    pig = torch.full((N, E, A), 7.0, device='cuda')
    actg = torch.full((E, N), 255, dtype=torch.uint8, device='cuda')
    vg = torch.zeros(N, E, device='cuda')
    ops.lstm_step_policy_value(hg, cu(case['wh']), cu(case['b']), cu(case['z1']), None, cg, cu(case['done']), cu(pad['pi_w']),
                               cu(pad['pi_b']), pig, actg, cu(pad['v_w']), cu(pad['v_b']), _nbr_idx().cuda(), A, vg,
                               **dict(case['draw'], u=cu(case['draw']['u'])))
    act = _check_policy_half(case, hg, cg, pig, actg)
    torch.testing.assert_close(vg.cpu().double(), _value_ref(case, act), rtol=1e-4, atol=2e-5)


# --------------------------------------------------------------------------- the update's heads and loss
@functools.lru_cache(maxsize=None)
def _loss_case(A, rows):
    """Inputs of the update's heads + loss and the float64 autograd chain of policies.py:20-30 / 241-254 over each agent's own
    columns: terms [N,3], and the gradients of the ragged head variables, of h, of the own logits and of v."""
    n_a = SHAPES[A]
    g = torch.Generator().manual_seed(100 * A + rows)
    r = lambda *s: torch.randn(*s, generator=g)                                         # noqa: E731
    h = torch.tanh(r(N, rows, H))
    rag, pad = _padded_heads(A, g)
    action = torch.stack([torch.randint(0, n_a[i], (rows,), generator=g) for i in range(N)], dim=1).to(torch.uint8)
    adv, R = r(N, rows), r(N, rows)
    v_coef, e_coef = 0.5, 0.01
    hd = h.double().requires_grad_(True)
    leaf = lambda t: t.double().requires_grad_(True)                                    # noqa: E731
    L = dict(pi_w=[leaf(t) for t in rag['pi_w']], pi_b=[leaf(t) for t in rag['pi_b']], v_h=[leaf(t) for t in rag['v_h']],
             v_nb=[[leaf(t) for t in ts] for ts in rag['v_nb']], v_b=[leaf(t) for t in rag['v_b']])
    terms, logits, vs = [], [], []
    for i in range(N):
        lg = hd[i] @ L['pi_w'][i] + L['pi_b'][i]                                  # [rows, n_a_i]
        v = hd[i] @ L['v_h'][i] + L['v_b'][i]
        for k, j in enumerate(NBR[i]):
            v = v + L['v_nb'][i][k][action[:, j].long()]
        lg.retain_grad(); v.retain_grad()
        pi = torch.softmax(lg, dim=-1)
        log_pi = torch.log(torch.clamp(pi, 1e-10, 1.0))
        ent = -(pi * log_pi).sum(-1)
        logp_a = log_pi.gather(-1, action[:, i].long().unsqueeze(-1)).squeeze(-1)
        terms.append(torch.stack([-(logp_a * adv[i].double()).mean(), (R[i].double() - v).pow(2).mean() * 0.5 * v_coef,
                                  -ent.mean() * e_coef]))
        logits.append(lg); vs.append(v)
    terms = torch.stack(terms)
    terms.sum().backward()
    return dict(A=A, rows=rows, n_a=n_a, h=h, pad=pad, action=action, adv=adv, R=R, v_coef=v_coef, e_coef=e_coef, terms=terms.detach(),
                dh=hd.grad, dlogits=[t.grad for t in logits], dv=torch.stack([t.grad for t in vs]), L=L)


@gpu
@pytest.mark.parametrize('want_dh', [True, False])
@pytest.mark.parametrize('rows', [1, 129, 1003])
@pytest.mark.parametrize('A', [4, 5, 8])
def test_heads_loss_on_padded_action_sets(A, rows, want_dh):
    """ops.heads_loss (what the per-agent-optimiser heterogeneous nets' update runs) on padded parameters, tolerances of
    test_gpu_ops.test_heads_loss_one_pass_vs_torch; gradient entries of padded columns / rows exactly 0.  A = 8: the one-pass
    kernel has 8 outputs (A + 1 <= 8) -- ops.heads_loss_supported says so, models take heads + ops.a2c_loss (tested below), and
    the entry point must refuse rather than compute something."""
    from deeprl_network_amd import _lib, ops
    case = _loss_case(A, rows)
    n_a, pad, L = case['n_a'], case['pad'], case['L']
    c = lambda t: t.cuda()                                                              # noqa: E731
    args = (c(case['h']), c(pad['pi_w']), c(pad['pi_b']), c(pad['v_w']), c(pad['v_b']), c(case['action']), _nbr_idx().cuda(), A,
            c(case['adv']), c(case['R']), case['v_coef'], case['e_coef'])
    if A + 1 > ops.THIN_MAX_O:
        assert not ops.heads_loss_supported(args[0], A, args[6])
        with pytest.raises(_lib.NmarlError):
            ops.heads_loss(*args, want_dh=want_dh)
        return
    assert ops.heads_loss_supported(args[0], A, args[6])
    out = ops.heads_loss(*args, want_dh=want_dh)
    torch.testing.assert_close(out['terms'].cpu().double(), case['terms'], rtol=2e-5, atol=1e-7)
    dy8 = out['dy8'].cpu().double()
    scale = max(float(t.abs().max()) for t in case['dlogits'])
    for i in range(N):
        torch.testing.assert_close(dy8[i, :, :n_a[i]], case['dlogits'][i], rtol=2e-4, atol=2e-6 * scale)
        assert torch.all(dy8[i, :, n_a[i]:A] == 0), 'agent %d: d logits of a padded column' % i
    torch.testing.assert_close(dy8[:, :, A], case['dv'], rtol=2e-4, atol=2e-6 * float(case['dv'].abs().max()))
    assert float(dy8[:, :, A + 1:].abs().max() if A + 1 < 8 else 0.0) == 0.0
    assert (out['dh'] is not None) == want_dh
    if want_dh:
        torch.testing.assert_close(out['dh'].cpu().double(), case['dh'], rtol=2e-4, atol=2e-6 * float(case['dh'].abs().max()))
    gw, gb, gv, gvb = (out[k].cpu().double() for k in ('pi_w', 'pi_b', 'v_w', 'v_b'))
    gv = gv.reshape(N, H + M_MAX * A)

    def close(got, ref, what, ref_max):
        torch.testing.assert_close(got, ref, rtol=2e-4, atol=3e-6 * ref_max + 1e-9, msg=lambda m: '%s: %s' % (what, m))
    mx = lambda ts: max(float(t.grad.abs().max()) for t in ts)                          # noqa: E731
    for i in range(N):
        close(gw[i, :, :n_a[i]], L['pi_w'][i].grad, 'pi_w[%d]' % i, mx(L['pi_w']))
        close(gb[i, :n_a[i]], L['pi_b'][i].grad, 'pi_b[%d]' % i, mx(L['pi_b']))
        assert torch.all(gw[i, :, n_a[i]:] == 0) and torch.all(gb[i, n_a[i]:] == 0), 'agent %d: gradient of a padded actor column' % i
        close(gv[i, :H], L['v_h'][i].grad, 'v_w[%d] (h part)' % i, mx(L['v_h']))
        close(gvb[i].reshape(1), L['v_b'][i].grad, 'v_b[%d]' % i, mx(L['v_b']))
        live = torch.zeros(M_MAX * A, dtype=torch.bool)
        for k, j in enumerate(NBR[i]):
            close(gv[i, H + k * A:H + k * A + n_a[j]], L['v_nb'][i][k].grad, 'v_w[%d] (neighbour %d)' % (i, j),
                  max(mx(ts) for ts in L['v_nb'] if ts))
            live[k * A:k * A + n_a[j]] = True
        assert torch.all(gv[i, H:][~live] == 0), 'agent %d: gradient of a padded critic row' % i


@gpu
@pytest.mark.parametrize('q6', [False, True], ids=['own_adv', 'q6_summed_adv'])
@pytest.mark.parametrize('rows', [1, 129, 1003])
@pytest.mark.parametrize('A', [4, 5, 8])
def test_a2c_loss_on_padded_logits(A, rows, q6):
    """ops.a2c_loss (what the shared-optimiser heterogeneous nets' update runs behind the heads) on logits whose padded columns hold
    -1e30, some own probabilities below the 1e-10 clip, tolerances of test_gpu_ops.test_a2c_loss_fused.  q6: the advantage of
    every agent is the per-row sum over agents (models._loss, quirk Q6 of the reference's heterogeneous branch)."""
    from deeprl_network_amd import ops
    n_a = SHAPES[A]
    g = torch.Generator().manual_seed(7 * A + rows + int(q6))
    out = torch.randn(N, rows, A + 1, generator=g) * 2.0          # logits handed over as a column block, like the heads' output
    out[:, ::7, 0] = -60.0                                        # pi_0 ~ 1e-26 < 1e-10: clipped, gradient blocked ...
    action = torch.stack([torch.randint(0, n_a[i], (rows,), generator=g) for i in range(N)], dim=1).to(torch.uint8)
    action[::7] = 0                                               # ... and it is the action taken on those rows
    for i in range(N):
        out[i, :, n_a[i]:A] = -1e30
    v, adv, R = (torch.randn(N, rows, generator=g) for _ in range(3))
    if q6:
        adv = adv.sum(dim=0, keepdim=True).expand(N, rows).contiguous()
    w = torch.rand(N, generator=g) + 0.5                          # per-agent upstream factors
    v_coef, e_coef = 0.5, 0.05
    # float64, the reference's definition: agent i has n_a_i logits
    od, vd = out.double().requires_grad_(True), v.double().requires_grad_(True)
    terms_r = []
    for i in range(N):
        pi = torch.softmax(od[i, :, :n_a[i]], dim=-1)
        log_pi = torch.log(torch.clamp(pi, 1e-10, 1.0))
        ent = -(pi * log_pi).sum(-1)
        logp_a = log_pi.gather(-1, action[:, i].long().unsqueeze(-1)).squeeze(-1)
        terms_r.append(torch.stack([-(logp_a * adv[i].double()).mean(), (R[i].double() - vd[i]).pow(2).mean() * 0.5 * v_coef,
                                    -ent.mean() * e_coef]))
    terms_r = torch.stack(terms_r)
    (terms_r.sum(dim=1) * w.double()).sum().backward()
    og = out.cuda().requires_grad_(True)
    vg = v.cuda().requires_grad_(True)
    tot, terms = ops.a2c_loss(og[..., :A], vg, action.cuda(), adv.cuda(), R.cuda(), v_coef, e_coef)
    (tot * w.cuda()).sum().backward()
    torch.testing.assert_close(tot.detach().cpu().double(), terms_r.detach().sum(dim=1), rtol=2e-5, atol=1e-6)
    torch.testing.assert_close(terms.cpu().double(), terms_r.detach(), rtol=2e-5, atol=1e-6)
    dog = og.grad.cpu()
    for i in range(N):
        torch.testing.assert_close(dog[i, :, :n_a[i]].double(), od.grad[i, :, :n_a[i]], rtol=1e-4, atol=1e-9)
        assert torch.all(dog[i, :, n_a[i]:] == 0), 'agent %d: d logits of a padded column' % i
    torch.testing.assert_close(vg.grad.cpu().double(), vd.grad, rtol=1e-4, atol=1e-9)


# --------------------------------------------------------------------------- the stand-alone draw
def _sparse_pi(E, A, g):
    """pi [N,E,A] with exact zeros: a trailing block (an agent's padded columns), one in the middle of the own set, and on
    every fifth row dyadic probabilities, so that a uniform can sit exactly on a CDF step."""
    n_a = SHAPES[A]
    pi = torch.zeros(N, E, A)
    for i in range(N):
        p = torch.rand(E, n_a[i], generator=g) + 0.05
        if n_a[i] >= 3:
            p[:, 1] = 0.0                                         # middle of the row
        if n_a[i] >= 4:
            p[1::2, 0] = 0.0                                      # and a leading one on every other row
        pi[i, :, :n_a[i]] = p / p.sum(-1, keepdim=True)
        if n_a[i] >= 3:
            pi[i, ::5, :n_a[i]] = 0.0
            pi[i, ::5, 0] = 0.5
            pi[i, ::5, n_a[i] - 1] = 0.5
    return pi


@functools.lru_cache(maxsize=None)
def _sample_case(A, E):
    g = torch.Generator().manual_seed(31 * A + E)
    pi = _sparse_pi(E, A, g)
    u = torch.rand(E, N, generator=g)
    u[0::3] = 0.0
    u[1::3] = U_BELOW_ONE
    u[5::10] = 0.5                                                # exactly on the step of the dyadic rows' CDF
    return pi, u


SAMPLE_CASES = [(A, E) for A in (4, 5, 8) for E in (1, 17, 130)]


def _sample_modes(u):
    from oracle import ops_ref
    return [(ops_ref.SAMPLE_UNIFORM, dict(u=u)), (ops_ref.SAMPLE_PHILOX, dict(seed=12345678901, env_id_base=777, step=4242)),
            (ops_ref.SAMPLE_ARGMAX, {})]


@pytest.mark.parametrize('A,E', SAMPLE_CASES)
def test_float64_side_of_the_draw_never_picks_a_zero(A, E):
    """(CPU) np.random.choice's rule (searchsorted(cdf, u, 'right')) never returns an action of probability exactly 0 for
    u in [0, 1) -- the property the kernel is held to below."""
    from oracle import ops_ref
    pi, u = _sample_case(A, E)
    for mode, kw in _sample_modes(u):
        ref = torch.zeros(E, N, dtype=torch.uint8)
        ops_ref.sample_actions(pi, ref, mode, **kw)
        p = pi.gather(-1, ref.t().long().unsqueeze(-1)).squeeze(-1)
        assert torch.all(p > 0), mode


@gpu
@pytest.mark.parametrize('A,E', SAMPLE_CASES)
def test_sample_actions_with_exact_zero_probabilities(A, E):
    """ops.sample_actions on probabilities with exact zeros in the middle and at the end of a row, uniforms at 0, at the largest
    float32 below 1 and exactly on a CDF step: the oracle's draw, and never an action of probability 0."""
    from deeprl_network_amd import ops
    from oracle import ops_ref
    pi, u = _sample_case(A, E)
    for mode, kw in _sample_modes(u):
        out = torch.full((E, N), 255, dtype=torch.uint8, device='cuda')
        ref = torch.zeros(E, N, dtype=torch.uint8)
        ops.sample_actions(pi.cuda(), out, mode, **{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()})
        ops_ref.sample_actions(pi, ref, mode, **kw)
        assert torch.equal(out.cpu(), ref), mode
        p = pi.gather(-1, out.cpu().t().long().unsqueeze(-1)).squeeze(-1)
        assert torch.all(p > 0), 'mode %d drew an action of probability 0' % mode

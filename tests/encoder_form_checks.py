"""The input encoders of the six policy classes, form by form (run by test_encoder_forms_cpu.py on the restated ops and by
test_gpu_encoder_forms.py on the kernels).  A net's observation layer over [own | neighbours] and, for some nets, its fingerprint layer
are described to five consumers -- the update's autograd forward (`unroll`), its backward over what the rollout saved (`unroll_saved`),
the rollout (`encode`), the env kernel (`fused_env_encode`) and the lock-step kernel (`_enc_spec`, `_ob_spec`) -- and these checks
hold the five against each other: the same layers, the same tensors, the same values.

Everything is asked through names the policies have had all along (encode, `_enc(xv, fp)` = the call `unroll` makes, unroll,
unroll_saved, fused_env_encode, `_enc_spec`, `_ob_spec`, enc_in_kernel, encodes_in_step, enc_writes_bits): the checks pin what the
forms compute, not how the host code derives them.

Shapes: the smallest at which a form can go wrong -- T = 2 lock-steps of E = 3 replicas (6 rows per agent: no multiple of a 64-row
tile), the 8-agent CACC line (m_max = 2, 5 features, 4 actions), a 3 x 3 ATSC grid (m_max = 4, 12 features, 5 actions, the env's
north-east-south-west neighbour order: not ascending), four heterogeneous agents, and the widths at which a form takes another path
(n_fc = 32: no fc kernel; 24 features x 3 slots = 72 inputs: no one-launch pair)."""
import numpy as np
import torch

T, E = 2, 3

# tests/fc_edge_checks.py, "Two encoder layers in one launch == act(x w + b) per layer in float64 (rtol 1e-5, atol 1e-5)": the bound of
# these layers' forward wherever two forms do not reach the same kernel
FWD_TOL = dict(rtol=1e-5, atol=1e-5)
# ... and of their gradients (fc_edge_checks: dw, db rtol 1e-4, atol 2e-5 sqrt(rows)), rows = T * E
GRAD_TOL = dict(rtol=1e-4, atol=2e-5 * float(T * E) ** 0.5)

CLASSES = ('LstmPolicy', 'FPPolicy', 'ConsensusPolicy', 'NCMultiAgentPolicy', 'IC3MultiAgentPolicy', 'DIALMultiAgentPolicy')
TWO_LAYER = ('FPPolicy', 'NCMultiAgentPolicy')
IA2C_FAMILY = ('LstmPolicy', 'FPPolicy', 'ConsensusPolicy')        # observations are concatenated by the env: `obs_order` applies
# the encoders' (weight, bias) keys per class: the reference's variable names, fixed by the checkpoints
KEYS = {'LstmPolicy': (('fc_w', 'fc_b'),), 'ConsensusPolicy': (('fc_w', 'fc_b'),), 'FPPolicy': (('fcs_w', 'fcs_b'), ('fcp_w', 'fcp_b')),
        'NCMultiAgentPolicy': (('w_ob', 'w_ob_b'), ('w_fp', 'w_fp_b')), 'IC3MultiAgentPolicy': (('w_ob', 'w_ob_b'),),
        'DIALMultiAgentPolicy': (('w_ob', 'w_ob_b'),)}


def _line(n):
    m = np.zeros((n, n), dtype=np.int64)
    for i in range(n - 1):
        m[i, i + 1] = m[i + 1, i] = 1
    return m


def _grid(rows, cols):
    """-> (neighbour mask, per agent the neighbours north, east, south, west)."""
    n = rows * cols
    m, order = np.zeros((n, n), dtype=np.int64), []
    for i in range(n):
        r, c = divmod(i, cols)
        nesw = [(r + 1, c), (r, c + 1), (r - 1, c), (r, c - 1)]
        order.append([rr * cols + cc for rr, cc in nesw if 0 <= rr < rows and 0 <= cc < cols])
        for j in order[-1]:
            m[i, j] = 1
    return m, order


_GRID_MASK, _GRID_ORDER = _grid(3, 3)
TOPOLOGIES = {
    'cacc-line': dict(mask=_line(8), n_feat=5, n_a=4),
    'grid-m4': dict(mask=_GRID_MASK, n_feat=12, n_a=5, obs_order=_GRID_ORDER),
    'hetero': dict(mask=_line(4), n_feat=5, n_a=4, n_feat_ls=[5, 3, 5, 4], n_a_ls=[4, 3, 4, 2]),
    'wide-line': dict(mask=_line(8), n_feat=24, n_a=4),             # 72 observation inputs: past the fc kernels' 64
}
# (class, topology, n_fc, n_h): every class on the three systems, and the widths at which the forms leave the fc kernels
CASES = [(c, t, 64, 64) for t in ('cacc-line', 'grid-m4', 'hetero') for c in CLASSES] + \
        [('LstmPolicy', 'cacc-line', 32, 64), ('FPPolicy', 'cacc-line', 32, 64), ('FPPolicy', 'wide-line', 64, 64),
         ('NCMultiAgentPolicy', 'wide-line', 64, 64)]
# widths asked of the descriptions only (no launch): NeurComm and ConseNet have no n_fc-wide layer, yet num_fc is asked
DESCRIPTION_CASES = CASES + [('NCMultiAgentPolicy', 'cacc-line', 32, 64), ('ConsensusPolicy', 'cacc-line', 32, 64),
                             ('NCMultiAgentPolicy', 'cacc-line', 64, 32), ('IC3MultiAgentPolicy', 'grid-m4', 64, 32)]


def case_id(case):
    return '%s-%s-fc%d-h%d' % case


def make_policy(case, dev):
    """The policy of a case, initialised like the reference (np.random stream), the encoders' biases moved off zero."""
    from deeprl_network_amd.agents import policies
    name, topo, n_fc, n_h = case
    tp = TOPOLOGIES[topo]
    np.random.seed(12)
    p = getattr(policies, name)(tp['n_feat'], tp['n_a'], tp['mask'], n_fc=n_fc, n_h=n_h, device=dev, n_feat_ls=tp.get('n_feat_ls'),
                                n_a_ls=tp.get('n_a_ls'), obs_order=tp.get('obs_order') if name in IA2C_FAMILY else None)
    p.params.init_reference_order()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for _, b in KEYS[name]:
            p.params[b].add_((0.2 * torch.randn(p.params[b].shape, generator=g)).to(p.device))
    return p


def make_inputs(p):
    """-> (Xc [T,E,N,n_feat] the compact observation, X [T,E,N,n_obs] the gathered slab, FP [N,T,E,A] previous policies): features an
    agent does not have are 0, actions it does not have have probability 0."""
    g = torch.Generator().manual_seed(5)
    Xc = torch.randn(T, E, p.N, p.n_feat, generator=g)
    logits = torch.randn(p.N, T, E, p.n_a, generator=g)
    for i in range(p.N):
        Xc[:, :, i, p.n_own[i]:] = 0.0
        logits[i, :, :, p.n_a_ls[i]:] = -float('inf')
    Xc, FP = Xc.to(p.device), torch.softmax(logits, dim=-1).to(p.device)
    return Xc, p.expand_obs(Xc), FP


def _ident(t):
    return None if t is None else (t.data_ptr(), tuple(t.shape))


def unroll_layers(ops, p, X, FP):
    """What `unroll`'s encoder computes on (X [T,E,N,*], FP [N,T,E,A]): -> (the layers' output [N,T*E,64 * layers], the `parts` it
    handed ops.fc_concat) -- `_enc(Xv, FP)` is the call unroll makes, on unroll's own views."""
    seen = []
    orig = ops.fc_concat

    def spy(parts, act, saved=None, bits=None):
        out = orig(parts, act, saved=saved, bits=bits)
        seen.append((out.detach(), [tuple(pt) + (None,) * (4 - len(pt)) for pt in parts], act))
        return out

    ops.fc_concat = spy
    try:
        Xv = X.reshape(T * E, p.N, X.shape[-1]).transpose(0, 1)
        p._enc(Xv, FP.reshape(p.N, T * E, p.n_a))
    finally:
        ops.fc_concat = orig
    assert len(seen) == 1, 'the encoder forward is %d fc_concat calls' % len(seen)
    return seen[0]


def _same_kernel(p, name, X):
    """fc_concat and the rollout form reach the same kernel: the layers fit the fc kernels (64 outputs, <= 64 inputs)."""
    w = p.params[KEYS[name][0][0]]
    return w.shape[2] == 64 and w.shape[1] <= 64 and p.n_na <= 64


def _agree(what, got, exp, exact):
    err = float((got - exp).abs().max())
    print('%s: max |difference| %.3g (%s)' % (what, err, 'bit for bit' if exact else 'rtol %(rtol)g, atol %(atol)g' % FWD_TOL))
    if exact:
        assert torch.equal(got, exp), '%s: differs (max %.3g) where both forms reach the same kernel' % (what, err)
    else:
        torch.testing.assert_close(got, exp, **FWD_TOL)


def layouts(case):
    """The observation layouts a case is asked in: the gathered slab always; the compact observation where the engine offers it
    (models.enable_compact_obs: no heterogeneous system, a gathering kernel that fits)."""
    name, topo, n_fc, n_h = case
    return ('slab',) if topo in ('hetero', 'wide-line') or n_fc != 64 else ('slab', 'compact')


# ------------------------------------------------------------------------------------------------------ rollout against unroll
def check_rollout_against_unroll(ops, case, layout, dev):
    """encode(x, fp) and encode(x, fp, out=slot) of every lock-step == the forward value of unroll's encoder on the same rows."""
    name = case[0]
    p = make_policy(case, dev)
    Xc, Xs, FP = make_inputs(p)
    X = Xc if layout == 'compact' else Xs
    with torch.no_grad():
        L, _, _ = unroll_layers(ops, p, X, FP)
    exact = _same_kernel(p, name, X)
    H = p.n_h
    KX = p.params[p.k_wx].shape[1]
    slots = torch.zeros(p.N, T, E, KX, device=p.device)
    for t in range(T):
        want = L[:, t * E:(t + 1) * E]
        fp_t = FP[:, t]
        if name == 'DIALMultiAgentPolicy':                 # + the own-action one-hot (a constant of the layers)
            want = want + p._own_action_onehot(fp_t)
        elif not p.xside:                                  # the x-side pre-activation: the layers' output times Wx
            wx = p.params[p.k_wx]
            want = torch.bmm(want, wx[:, :want.shape[2]]).detach()
        fresh = p.encode(X[t], fp_t)
        if p.xside:
            kept = p.encode(X[t], fp_t, out=slots[:, t])
            if name != 'DIALMultiAgentPolicy':             # (lstm_dial's slot is written by the step: S = enc + hm)
                assert _ident(kept) == _ident(slots[:, t]), 'encode(out=) did not write the slot it was given'
        else:
            kept = fresh
        for what, got in (('encode', fresh), ('encode(out=)', kept)):
            if name == 'NCMultiAgentPolicy' and p.xside:   # [hx | hp | room for the message third]
                assert got.shape[2] == 3 * H
                got = got[:, :, :2 * H]
            _agree('%s %s %s t=%d' % (case_id(case), layout, what, t), got, want, exact and p.xside)
    return p


# ------------------------------------------------------------------------------------------------------ the descriptions
def check_descriptions(ops, case, dev):
    """fused_env_encode, `_enc_spec` / `_ob_spec` name exactly the tensors the host forms' `parts` use, and say None / unsupported
    where the layers do not have the kernels' shape: heterogeneous agents, n_feat != 5 for the env kernel, widths other than 64."""
    name, topo, n_fc, n_h = case
    p = make_policy(case, dev)
    Xc, Xs, FP = make_inputs(p)
    with torch.no_grad():
        _, parts, act = unroll_layers(ops, p, Xs, FP)
    p.refresh_wimage()
    two = name in TWO_LAYER
    # (the sign image: asked of a net whose launch runs both encoders -- the one-layer coupled nets need not have the attribute)
    assert len(parts) == (2 if two else 1) and bool(getattr(p, 'enc_writes_bits', False)) == two
    ob, fpl = parts[0], (parts[1] if two else None)
    for (wk, bk), pt in zip(KEYS[name], parts):
        assert _ident(pt[1]) == _ident(p.params[wk]) and _ident(pt[2]) == _ident(p.params[bk])
    fits64 = n_fc == 64 and n_h == 64
    layer64 = (n_fc if name in ('LstmPolicy', 'FPPolicy') else n_h) == 64           # the width of the class's encoder layers
    x, fp, fp_next = Xc[0], FP[:, 0], FP[:, 1]
    out = torch.zeros(p.N, E, 128 if two else 64, device=p.device)
    bits = torch.zeros(p.N, E, 4, dtype=torch.int32, device=p.device)

    # the env kernel: relu layers over the compact CACC observation, written as they are into the LSTM input
    d = p.fused_env_encode(fp_next, out)
    env_fused = name in ('LstmPolicy', 'FPPolicy', 'NCMultiAgentPolicy') and topo == 'cacc-line' and layer64 and n_h == 64
    assert (d is not None) == env_fused, 'fused_env_encode answers %r' % (d,)
    if d is not None:
        assert _ident(d['w_ob']) == _ident(ob[1]) and _ident(d['b_ob']) == _ident(ob[2]) and d['act'] == act == ops.BIAS_RELU
        assert d['nbr_idx'] is p.nbr_idx and d['out'] is out
        assert ('w_fp' in d) == two
        if two:
            assert _ident(d['w_fp']) == _ident(fpl[1]) and _ident(d['b_fp']) == _ident(fpl[2]) and d['fp'] is fp_next

    # the lock-step kernel's pre-phase
    if name in ('LstmPolicy', 'FPPolicy', 'ConsensusPolicy', 'NCMultiAgentPolicy'):
        s = p._enc_spec(x, fp, out, None, bits)
        # (`env`: the product's op alone has the key -- the in-launch env step exists on the device only)
        assert set(s) - {'env'} == {'ob', 'fp', 'w_ob', 'b_ob', 'w_fp', 'b_fp', 'nbrs', 'out', 'bits'}
        assert s['ob'] is x and s['fp'] is fp and s['out'] is out and s.get('env') is None and s['nbrs'] == p.nbrs
        assert _ident(s['w_ob']) == _ident(ob[1]) and _ident(s['b_ob']) == _ident(ob[2])
        assert _ident(s['w_fp']) == _ident(fpl and fpl[1]) and _ident(s['b_fp']) == _ident(fpl and fpl[2])
        assert (s['bits'] is bits) if two else (s['bits'] is None)                   # the sign image: the two-layer encodings'
        assert (p._enc_spec(x, fp, None).get('w_fp') is not None) == two
    if name == 'IC3MultiAgentPolicy':
        s = p._ob_spec(x)
        assert set(s) == {'x', 'nbr', 'img', 'b', 'w'} and s['x'] is x and s['nbr'] is p.nbr_self and s['img'] is p._ob_img
        assert _ident(s['w']) == _ident(ob[1]) and _ident(s['b']) == _ident(ob[2])

    # which net's launch runs its encoders, and at which shapes
    homog = topo != 'hetero'
    assert not p.enc_in_kernel(E, False) and not p.encodes_in_step(E, False)
    if name in IA2C_FAMILY:
        # (the input layouts the pre-phase has are the op's to say: the restated ops know the CACC one alone)
        if two:
            layout = ops.step_enc_supported(p.n_feat, p.n_a, p.m_max, 64, 64, p.N)
        else:
            layout = ops.step_enc1_supported(p.n_feat, 0 if name == 'ConsensusPolicy' else p.m_max, 64, 64, p.N)
        want = homog and fits64 and bool(layout)
        assert layout == (topo != 'wide-line') or p.device.type == 'cpu'      # the kernels: every layout here but the 72-input one
        assert bool(p.enc_in_kernel(E, True)) == want, 'enc_in_kernel: %r' % (p.enc_in_kernel(E, True),)
    elif name == 'NCMultiAgentPolicy':
        want = topo == 'cacc-line' and fits64 and bool(p.pv_one_launch(E))
        assert bool(p.enc_in_kernel(E, True)) == want
    else:
        assert not p.enc_in_kernel(E, True)
    if name == 'IC3MultiAgentPolicy':
        assert bool(p.encodes_in_step(E, True)) == (topo == 'grid-m4' and n_h == 64 and bool(p.pv_one_launch(E)))
    else:
        assert not p.encodes_in_step(E, True)
    return p


# ------------------------------------------------------------------------------------------------------ saved against recomputed
def _param_grads(p, fn, W):
    ps = p.params
    ps.begin_backward()
    Hs = fn()
    (Hs * W).sum().backward()
    ps.end_backward()
    return ps.grad.clone()


def check_saved_against_recomputed(model, tr, bits, enc_slots):
    """One eager batch of a small trainer (the second: the recurrent state is not zero), stopped where the update starts:
    `unroll_saved` over what the rollout's lock-steps saved -- with the sign image and without it; CommNet: from the ENC slots and
    recomputed -- sets up the parameter gradients of `unroll` on the same batch.  bits / enc_slots: the batch must have them."""
    p = model.policy
    seen = {}
    grads = model.update_grads

    def update_grads(R_end):
        if tr_batches[0] == 2:
            seen.update(_saved_and_recomputed(model))
        return grads(R_end)

    tr_batches = [0]
    model.update_grads = update_grads
    try:
        for _ in range(2):
            tr_batches[0] += 1
            tr.run_batch()
    finally:
        del model.update_grads
    assert model.save_acts and 'unroll' in seen
    assert ('unroll_saved, sign image' in seen) == bits and ('unroll_saved, ENC slots not filled' in seen) == enc_slots, sorted(seen)
    ref = seen.pop('unroll')
    assert float(ref.abs().max()) > 0.0
    for what, g in sorted(seen.items()):
        err = float((g - ref).abs().max())
        print('%s %s: max |difference| %.3g of max |gradient| %.3g (rtol %g, atol %.3g)'
              % (type(p).__name__, what, err, float(ref.abs().max()), GRAD_TOL['rtol'], GRAD_TOL['atol']))
        torch.testing.assert_close(g, ref, **GRAD_TOL)
    return seen


def _saved_and_recomputed(model):
    p = model.policy
    T, E, N = model.n_step, model.E, model.n_agent
    FP = model.buf_fp[:T].permute(1, 0, 2, 3).reshape(N, T * E, model.n_a)
    X = model.buf_x[:T]
    W = torch.randn(N, T * E, p.n_h, generator=torch.Generator().manual_seed(9)).to(p.device)
    out = {'unroll': _param_grads(p, lambda: p.unroll(X, FP, model.buf_done_pre, model.h_bw, model.c_bw,
                                                      masked_steps=model.masked_steps), W)}

    def saved(**kw):
        return _param_grads(p, lambda: p.unroll_saved(X, FP, model.S_buf, model.G_buf, model.H_all, model.C_all, model.buf_done_pre,
                                                      masked_steps=model.masked_steps, S_ext=model.S_ext, **kw), W)

    out['unroll_saved'] = saved()
    if model.S_bits is not None and p._bits_steps == T:
        out['unroll_saved, sign image'] = saved(S_bits=model.S_bits)
    if getattr(p, '_enc_was_saved', False):
        p._enc_was_saved = False
        try:
            out['unroll_saved, ENC slots not filled'] = saved()
        finally:
            p._enc_was_saved = True
    return out

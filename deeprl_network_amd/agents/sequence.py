"""Fused n_step recurrences with CROSS-AGENT coupling (NeurComm, CommNet, DIAL) for the update: manual BPTT as one
torch.autograd.Function instead of ~15 autograd nodes per step.

Reference recurrences (agents/utils.py): lstm_comm 182-208, lstm_ic3 385-408, lstm_dial 561-593.  Per step t, with
h = h_{t-1} (un-masked for the messages, quirk Q3), `enc_t` the h-independent part computed for all T beforehand:

  nc    hm = relu(gather(h) W_msg + b_msg);                     z = enc_t + hm Wx[2H:3H] + (h keep) Wh
  ic3   s  = enc_t + mean_nbr(h) W_msg + b_msg;                 z = s Wx + (h keep) Wh
  dial  hm = relu(gather(relu(h W_mfc + b_mfc)) W_msg + b_msg); z = (enc_t + hm) Wx + (h keep) Wh

followed by the cell (fused MFMA step kernel when H = 64).  Backward, in three parts: choose the tier of the reverse recurrence
(`_choose_tier`: a one-launch kernel, the step kernel per step, or torch), run it (`_run_tier`: it fills dZ and the message layers'
D1 / D2 / DS), then every weight gradient as a SINGLE GEMM over all rows and every bias gradient as a single reduction
(`_weight_grads`, one rule for flat and (T + 1)-slab operands: ops.seq_rows_pair).
"""
import torch

from .. import ops

F32 = torch.float32


def _stack_rows(w_top, w_bot):
    """[w_top; w_bot] as one [N, rows, 4H] view when the two tensors are adjacent rows of the flat buffer."""
    if (w_top.stride() == w_bot.stride() and w_top.shape[2] == w_bot.shape[2] and w_top.stride(2) == 1 and
            w_top.stride(1) == w_top.shape[2] and
            w_top.data_ptr() + w_top.shape[1] * w_top.shape[2] * 4 == w_bot.data_ptr()):
        return torch.as_strided(w_top, (w_top.shape[0], w_top.shape[1] + w_bot.shape[1], w_top.shape[2]), w_top.stride())
    return None


def _panels(w):
    return w.stride(2) == 1 and w.stride(1) == w.shape[2]


def _choose_tier(kind, nbr_idx, G, Call, done, dHs, wxm, wh, w_msg, mfc_w, hm, A2):
    """Which form of the reverse recurrence applies, and in which form it takes the heads' dL/dh -> (tier, rev, dHs, head_dy):
      'dial'     lstm_dial, the whole recurrence in one launch (rev: ops.dial_bptt_table)
      'coupled'  lstm_comm / lstm_ic3, the whole recurrence in one launch (rev: the kind's reverse table)
      'step'     cell backward + dgrad in one MFMA kernel per step; rev: the table of lstm_dial's adjoint kernel, None: torch adjoint
      'torch'    ops.bptt_loop
    The one-launch kernels expand the heads' dy8 themselves (head_dy = (dy8, hw), dHs unused); every other tier gets the tensor."""
    N, T, E, H4 = G.shape
    H, m_max = H4 // 4, nbr_idx.shape[1]
    head_dy = ops.take_head_dy(dHs)
    dHs = None if head_dy is not None else dHs.contiguous()
    tier, rev = 'torch', None
    if ops.bptt_supported(H) and _panels(wxm) and _panels(wh):
        tier = 'step'
        if kind == 'dial':
            if ops.bptt_dial_operands_ok(G, Call, done, dHs, wxm, wh, w_msg, mfc_w, hm, A2):
                rev = ops.dial_bptt_table(nbr_idx, H)        # None: m_max > 2, more than 2 sources per agent, no GPU
            if rev is not None:
                tier = 'dial'
            elif _panels(w_msg):
                rev = ops.reverse_table(nbr_idx, ops.COUPLED_NC)
                if not ops.dial_adjoint_supported(m_max, H, rev):
                    rev = None
        else:
            ckind = ops.COUPLED_NC if kind == 'nc' else ops.COUPLED_IC3
            if ops.bptt_coupled_supported(ckind, m_max, H) and _panels(w_msg):
                rev = ops.reverse_table(nbr_idx, ckind)
                if rev is not None and ops.bptt_coupled_supported(ckind, m_max, H, rev=rev):
                    tier = 'coupled'
                else:
                    rev = None                    # e.g. lstm_comm with more than 2 sources per agent
    if head_dy is not None and tier not in ('dial', 'coupled'):
        dHs, head_dy = ops.head_dy_to_dh(*head_dy, (N, T, E, H)), None
    return tier, rev, dHs, head_dy


def _message_adjoint(kind, D1, msg, D2, wmsg_t, mfc_w, nbr_idx, add=None):
    """One step's message adjoint from D1 = dL/d(the receiver layer's pre-activation; ic3: ds) -> the message part of dL/dh_{t-1}
    (+ add, in the last launch's own pass): the adjoint of the neighbour gather / mean; lstm_dial: then the senders' relu mask (into
    D2) and the sender layer's product."""
    H = D1.shape[-1]
    if add is not None and not add.is_contiguous():
        add = add.contiguous()
    if kind == 'nc':
        return ops.nbr_gather_bwd(torch.bmm(D1, wmsg_t), nbr_idx, H, add=add)
    if kind == 'ic3':
        return ops.nbr_mean_bwd(torch.bmm(D1, wmsg_t), nbr_idx, add=add)
    dmsg = ops.nbr_gather_bwd(torch.bmm(D1, wmsg_t), nbr_idx, H)
    torch.mul(dmsg, (msg > 0), out=D2)
    mfc_t = mfc_w.transpose(1, 2)
    return torch.bmm(D2, mfc_t) if add is None else torch.baddbmm(add, D2, mfc_t)


def _torch_adjoint(kind, nbr_idx, w_msg, mfc_w, hm, A2, D1, D2, DS, fold):
    """ops.bptt_loop's per-step callback for the coupled nets: D1 (and lstm_dial's DS) from dx, then _message_adjoint.  fold: the
    recurrent part dhd is added inside the adjoint's last launch (the saved path), else by an addition of its own (the recompute
    path)."""
    wmsg_t = w_msg.transpose(1, 2)

    def adjoint(t, dx, dhd):
        if kind == 'ic3':
            D1[:, t].copy_(dx)
        else:
            if kind == 'dial':
                DS[:, t].copy_(dx)
            torch.mul(dx, (hm[:, t] > 0), out=D1[:, t])
        msg, d2 = (A2[:, t], D2[:, t]) if kind == 'dial' else (None, None)
        if fold:
            return _message_adjoint(kind, D1[:, t], msg, d2, wmsg_t, mfc_w, nbr_idx, add=dhd)
        return _message_adjoint(kind, D1[:, t], msg, d2, wmsg_t, mfc_w, nbr_idx) + dhd
    return adjoint


def _run_tier(tier, rev, kind, nbr_idx, masked, keep, G, Call, done, dHs, head_dy, wxm, wh, w_msg, mfc_w, hm, A2, dZ, D1, D2, DS):
    """The reverse recurrence in the chosen form: fills dZ [N,T,E,4H], D1 (nc / dial: d(pre-relu of hm); ic3: ds) and, for lstm_dial,
    D2 (d(pre-relu of msg)) and DS (ds) -> the bias gradients it summed on the way, {'b' | 'msg' | 'mfc': [N, .]} (the others are
    row sums of dZ / D1 / D2)."""
    N, T, E, H4 = G.shape
    H, m_max, dev = H4 // 4, nbr_idx.shape[1], G.device
    if tier == 'torch':
        w2 = _stack_rows(wxm, wh)                 # [N, 2H, 4H]: one dgrad GEMM gives [d(wx input) | d(h keep)]
        ops.bptt_loop(G, Call, done, keep, dHs, masked, dZ, wh.transpose(1, 2), wx_t=wxm.transpose(1, 2),
                      w2_t=None if w2 is None else w2.transpose(1, 2),
                      adjoint=_torch_adjoint(kind, nbr_idx, w_msg, mfc_w, hm, A2, D1, D2, DS, fold=True))
        return {}
    # dL/dc carried between the step-wise launches.  (The one-launch kernels keep theirs inside and do not read it; it is zeroed
    # before every fused tier, as it always was: the captured update's launches are pinned to its predecessor's.)
    dc = torch.zeros(N, E, H, dtype=F32, device=dev)
    dc_next = torch.empty_like(dc)
    ws = (wxm, wh, ops.lstm_bptt_wimage(wxm, wh))
    if tier == 'dial':
        # cell backward, [ds | dh] = dz @ [wx; wh]^T, both relu masks, the message adjoint handed between the agents' blocks, the
        # sender layer's product, the three bias gradients on the way
        wm = (w_msg, ops.lstm_bptt_msg_wimage(w_msg))
        db, dbmsg, dbmfc, _, _ = ops.bptt_dial(rev, m_max, G, Call, done, dHs, ws, wm, ops.lstm_bptt_msg_wimage(mfc_w), hm, A2, dZ, DS, D1,
                                               D2, head_dy=head_dy)
        return dict(b=db, msg=dbmsg, mfc=dbmfc)
    if tier == 'coupled':
        # cell backward, [dx | dh] = dz @ [wxm; wh]^T, relu mask, the message adjoint D1 @ w_msg^T handed between the agents' blocks
        # inside the kernel, both bias gradients on the way
        wm = (w_msg, ops.lstm_bptt_msg_wimage(w_msg))
        db, dbmsg = ops.bptt_coupled(ops.COUPLED_NC if kind == 'nc' else ops.COUPLED_IC3, rev, m_max, G, Call, done, dHs, ws, wm,
                                     hm if kind == 'nc' else None, dZ, D1, head_dy=head_dy)
        return dict(b=db, msg=dbmsg)
    # step-wise: cell backward + [dx | dh] = dz @ [wxm; wh]^T (+ relu mask, + done mask, + db) in one MFMA kernel per step; lstm_dial with
    # `rev`: the whole message adjoint of a step (both relu masks, gather adjoint, both products, both bias sums) in ONE more launch
    dhd = torch.empty(N, E, H, dtype=F32, device=dev)
    if rev is not None:
        imgs, dh_adj, parts = ops.dial_adjoint_images(w_msg, mfc_w), torch.empty(N, E, H, dtype=F32, device=dev), ops.dial_adjoint_bias_parts(N, E, dev)
    dbp = ops.bptt_step_db_parts(N, E, H, dev)
    wmsg_t = w_msg.transpose(1, 2)
    dh_rec = None
    for t in range(T - 1, -1, -1):
        ops.bptt_step(G[:, t], Call[:, t], Call[:, t + 1], done[t], dHs[:, t], dh_rec, dc, ws, dZ[:, t], dc_next, dhd, t in masked,
                      dx=DS[:, t] if kind == 'dial' else D1[:, t], mask=hm[:, t] if kind == 'nc' else None, db_part=dbp)
        dc, dc_next = dc_next, dc
        if rev is not None:
            dh_rec = ops.dial_msg_adjoint(DS[:, t], hm[:, t], A2[:, t], dhd, w_msg, mfc_w, nbr_idx, imgs, rev, D1[:, t], D2[:, t], dh_adj,
                                          bias_parts=parts)
        elif kind == 'dial':
            torch.mul(DS[:, t], (hm[:, t] > 0), out=D1[:, t])
            dh_rec = _message_adjoint(kind, D1[:, t], A2[:, t], D2[:, t], wmsg_t, mfc_w, nbr_idx, add=dhd)
        else:
            dh_rec = _message_adjoint(kind, D1[:, t], None, None, wmsg_t, mfc_w, nbr_idx, add=dhd)
    sums = dict(b=dbp.sum(dim=1))
    if rev is not None:
        sums.update(msg=parts[0].sum(dim=1), mfc=parts[1].sum(dim=1))
    return sums


def _weight_grads(kind, nbr_idx, masked, keep, X, Hall, M, dZ, D1, D2, sums):
    """Every weight and bias gradient from what the tier left; X, M, dZ, D1, D2 sequence operands (ops.seq_buffer): X the LSTM
    inputs, M the message layer's saved input -- None: the un-masked state sequence itself (nc, ic3), lstm_dial: the senders'
    vectors, lstm_ic3 optionally the mean_nbr(h_{t-1}) rows the rollout kept.  Each product reads its two operands in place iff both
    are (T + 1)-slab buffers; a bias gradient is the tier's own sum if it made one, else the row sum.
    -> (dwx, dwh, db, dwmsg, dbmsg, dmfc_w, dmfc_b)."""
    H = Hall.shape[-1]
    Hs = ops.seq_operand(Hall, Hall.shape[1] - 1)

    def row_sum(name, op):
        return sums[name] if name in sums else ops.seq_rows(op[0] if op[0] is not None else op[1]).sum(dim=1)
    # the message layers first: their input is the UN-masked h_{t-1} (quirk Q3), which lstm_weight_grads may mask in place
    src, d1 = ops.seq_rows_pair(Hs if M is None else M, D1)
    if kind == 'ic3':
        dwmsg = ops.wgrad(ops.nbr_mean(src, nbr_idx) if M is None else src, d1)
    elif D1[0] is not None and (Hs if M is None else M)[0] is not None:
        dwmsg = _dwmsg_by_runs(src, d1, nbr_idx, H)          # both in place: per run of agents, no gathered copy
    else:
        dwmsg = ops.wgrad(ops.nbr_gather(src, nbr_idx), d1)
    dmfc_w = dmfc_b = None
    if kind == 'dial':                                       # the sender layer, on the un-masked h_{t-1}
        dmfc_w = ops.wgrad(*ops.seq_rows_pair(Hs, D2))
        dmfc_b = row_sum('mfc', D2)
    db, dbmsg = row_sum('b', dZ), row_sum('msg', D1)
    dwx, dwh = ops.lstm_weight_grads(X, Hall, dZ, keep, masked)
    return dwx, dwh, db, dwmsg, dbmsg, dmfc_w, dmfc_b


class CoupledSequence(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kind, nbr_idx, masked_steps, enc, h0, c0, done, wx, wh, b, w_msg, b_msg, mfc_w, mfc_b):
        N, T, E, _ = enc.shape
        H = h0.shape[-1]
        dev = enc.device
        G = torch.empty(N, T, E, 4 * H, dtype=F32, device=dev)
        Hall = torch.empty(N, T + 1, E, H, dtype=F32, device=dev)
        Call = torch.empty(N, T + 1, E, H, dtype=F32, device=dev)
        Hall[:, 0].copy_(h0)
        Call[:, 0].copy_(c0)
        A1 = torch.empty(N, T, E, H, dtype=F32, device=dev)          # nc/dial: hm (post-relu); ic3: s
        A2 = torch.empty(N, T, E, H, dtype=F32, device=dev) if kind == 'dial' else None   # dial: msg (post-relu)
        S = torch.empty(N, T, E, H, dtype=F32, device=dev) if kind == 'dial' else None    # dial: enc + hm
        masked = set(range(T)) if masked_steps is None else set(masked_steps)
        fused = H == ops.FUSED_H
        xs = (None, None, ops.lstm_wimage(None, wh)) if fused else None      # (KX = 0: wh alone, the x-side part as addends)
        keep = 1.0 - done
        for t in range(T):
            hp = Hall[:, t].contiguous()
            if kind == 'nc':
                ops.bias_act_(torch.bmm(ops.nbr_gather(hp, nbr_idx), w_msg), b_msg, ops.BIAS_RELU, out=A1[:, t])
                z1, z2 = enc[:, t], torch.bmm(A1[:, t], wx)
            elif kind == 'ic3':
                s = ops.bias_act_(torch.bmm(ops.nbr_mean(hp, nbr_idx), w_msg), b_msg, ops.BIAS_NONE)
                torch.add(s, enc[:, t], out=A1[:, t])
                z1, z2 = torch.bmm(A1[:, t], wx), None
            else:
                ops.bias_act_(torch.bmm(hp, mfc_w), mfc_b, ops.BIAS_RELU, out=A2[:, t])
                ops.bias_act_(torch.bmm(ops.nbr_gather(A2[:, t].contiguous(), nbr_idx), w_msg), b_msg, ops.BIAS_RELU,
                              out=A1[:, t])
                torch.add(A1[:, t], enc[:, t], out=S[:, t])
                z1, z2 = torch.bmm(S[:, t], wx), None
            if fused:
                ops.lstm_step_fused(Hall[:, t], wh, b, z1, z2, Call[:, t], done[t], G[:, t], Call[:, t + 1], Hall[:, t + 1], xs=xs)
            else:
                hk = hp * keep[t].view(1, E, 1) if t in masked else hp
                z = torch.bmm(hk, wh) if z2 is None else torch.baddbmm(z2, hk, wh)
                ops.cell_fwd(z, b, Call[:, t], done[t], G[:, t], Call[:, t + 1], Hall[:, t + 1], z2=z1)
        ctx.save_for_backward(G, Hall, Call, A1, A2 if A2 is not None else G.new_empty(0), S if S is not None else G.new_empty(0),
                              done, wx, wh, w_msg, mfc_w if mfc_w is not None else G.new_empty(0), nbr_idx)
        ctx.kind, ctx.masked = kind, masked
        return Hall[:, 1:]

    @staticmethod
    def backward(ctx, dHs):
        G, Hall, Call, A1, A2, S, done, wx, wh, w_msg, mfc_w, nbr_idx = ctx.saved_tensors
        kind, masked = ctx.kind, ctx.masked
        N, T, E, H4 = G.shape
        H = H4 // 4
        dZ = ops.seq_buffer(N, T, E, H4, G.device, False)
        D1 = ops.seq_buffer(N, T, E, H, G.device, False)      # nc/dial: d(pre-relu of hm); ic3: ds
        D2 = DS = (None, None)                                # dial: d(pre-relu of msg), ds
        if kind == 'dial':
            D2, DS = ops.seq_buffer(N, T, E, H, G.device, False), ops.seq_buffer(N, T, E, H, G.device, False)
        keep = 1.0 - done
        w2 = _stack_rows(wx, wh)                              # [N, 2H, 4H]: one dgrad GEMM gives [d(wx input) | d(h keep)]
        dh_rec, dc = ops.bptt_loop(G, Call, done, keep, dHs.contiguous(), masked, dZ[1], wh.transpose(1, 2), wx_t=wx.transpose(1, 2),
                                   w2_t=None if w2 is None else w2.transpose(1, 2),
                                   adjoint=_torch_adjoint(kind, nbr_idx, w_msg, mfc_w, A1, A2, D1[1], D2[1], DS[1], fold=False))
        # the LSTM's input: hm (nc: enc enters z directly), s (ic3), enc + hm (dial)
        dwx, dwh, db, dwmsg, dbmsg, dmfc_w, dmfc_b = _weight_grads(kind, nbr_idx, masked, keep, (None, S if kind == 'dial' else A1), Hall,
                                                                    (None, A2) if kind == 'dial' else None, dZ, D1, D2, {})
        denc = {'nc': dZ, 'ic3': D1, 'dial': DS}[kind][1]
        return None, None, None, denc, dh_rec, dc, None, dwx, dwh, db, dwmsg, dbmsg, dmfc_w, dmfc_b


class CoupledSequenceSaved(torch.autograd.Function):
    """The coupled recurrences of the update WITHOUT a forward pass: the rollout's policy steps (x-side step kernel,
    agents/policies.py `_recur_addends`) evaluated exactly this sequence with exactly these weights and saved
    S [N,T,E,KX] (the LSTM inputs: nc [hx | hp | hm], ic3 s, dial enc + hm), the gates G, the state sequences Hall /
    Call and, for dial, the post-relu message terms A1 (hm) / A2 (msg); for ic3 A1 may be the (T + 1)-slab buffer of the
    mean_nbr(h_{t-1}) rows the step kernel kept (the message layer's input: no averaging pass over the h sequence here).
    forward = hand out Hall[:, 1:]; backward = the manual BPTT of CoupledSequence with the x-side weight as ONE matrix:
      nc    `enc` = [hx | hp] (autograd-connected, = S[..., :2H]); wx = the full [3H,4H]:
            d enc = dZ @ wx[:2H]^T, d wx = S^T dZ (one GEMM over all T*E rows, all three thirds at once)
      ic3 / dial as in CoupledSequence (their `enc` enters the LSTM input additively)."""

    @staticmethod
    def forward(ctx, kind, nbr_idx, masked_steps, enc, done, wx, wh, b, w_msg, b_msg, mfc_w, mfc_b, G, Hall, Call, S, A1, A2,
                s_ext=None):
        T = G.shape[1]
        ctx.s_ext = s_ext
        e = G.new_empty(0)
        ctx.save_for_backward(G, Hall, Call, S, A1 if A1 is not None else e, A2 if A2 is not None else e, done, wx, wh, w_msg,
                              mfc_w if mfc_w is not None else e, nbr_idx)
        ctx.kind = kind
        ctx.masked = set(range(T)) if masked_steps is None else set(masked_steps)
        return Hall[:, 1:]

    @staticmethod
    def backward(ctx, dHs):
        G, Hall, Call, S, A1, A2, done, wx, wh, w_msg, mfc_w, nbr_idx = ctx.saved_tensors
        kind, masked = ctx.kind, ctx.masked
        N, T, E, H4 = G.shape
        H = H4 // 4
        dial = kind == 'dial'
        wxm = wx[:, 2 * H:] if kind == 'nc' else wx           # the rows of wx the h-dependent part of the input meets
        hm = S[..., 2 * H:] if kind == 'nc' else A1           # post-relu message term (nc: last third of the input)
        # 1. the tier
        tier, rev, dHs, head_dy = _choose_tier(kind, nbr_idx, G, Call, done, dHs, wxm, wh, w_msg, mfc_w, hm, A2)
        # 2. run it.  Layout: with the LSTM inputs handed over as the first T slabs of a (T + 1)-slab buffer (and lstm_dial's senders'
        # vectors A2 likewise) dZ, D1, D2 are allocated the same way, and every weight gradient reads its operands in place; lstm_dial
        # with A2 alone padded: D1 follows it (the message-weight gradient in place), the rest stays flat
        M = ops.seq_operand(A2, T) if dial else ops.seq_operand(A1, T) if (kind == 'ic3' and A1.numel() and A1.shape[1] == T + 1) else None
        padded = ops.seq_input_in_place(S, ctx.s_ext, Hall) and (not dial or M[0] is not None)
        dZ = ops.seq_buffer(N, T, E, H4, G.device, padded)
        D1 = ops.seq_buffer(N, T, E, H, G.device, padded or (dial and M[0] is not None))      # nc/dial: d(pre-relu of hm); ic3: ds
        D2 = DS = (None, None)                                # dial: d(pre-relu of msg), ds
        if dial:
            D2, DS = ops.seq_buffer(N, T, E, H, G.device, padded), ops.seq_buffer(N, T, E, H, G.device, False)
        keep = 1.0 - done
        sums = _run_tier(tier, rev, kind, nbr_idx, masked, keep, G, Call, done, dHs, head_dy, wxm, wh, w_msg, mfc_w, hm, A2, dZ[1], D1[1],
                         D2[1], DS[1])
        # 3. the weight gradients
        dwx, dwh, db, dwmsg, dbmsg, dmfc_w, dmfc_b = _weight_grads(kind, nbr_idx, masked, keep, (ctx.s_ext if padded else None, S), Hall, M,
                                                                    dZ, D1, D2, sums)
        if kind == 'nc':
            denc = None
            if ctx.needs_input_grad[3]:
                denc = torch.bmm(ops.seq_rows(dZ[1]), wx[:, :2 * H].transpose(1, 2)).view(N, T, E, 2 * H)
        else:
            denc = DS[1] if dial else D1[1]
        return (None, None, None, denc, None, dwx, dwh, db, dwmsg, dbmsg, dmfc_w, dmfc_b, None, None, None, None, None, None, None)


def _gather_runs(nbr_idx):
    """[(i0, i1, k, d)]: the maximal runs of consecutive agents i0 .. i1 - 1 whose k-th neighbour sits at the constant index offset d."""
    tab = nbr_idx.cpu().numpy()
    runs = []
    for k in range(tab.shape[1]):
        i = 0
        while i < tab.shape[0]:
            if tab[i, k] < 0:
                i += 1
                continue
            d, i0 = int(tab[i, k]) - i, i
            while i < tab.shape[0] and tab[i, k] >= 0 and int(tab[i, k]) - i == d:
                i += 1
            runs.append((i0, i, k, d))
    return runs


def _dwmsg_by_runs(Hx, D1x, nbr_idx, H):
    """lstm_comm's message-weight gradient  gather(h)^T D1  without the gathered copy: block (agent i, slot k) of it is
    h[nbr(i, k)]^T D1[i], and over a run of consecutive agents whose k-th neighbour sits at a constant index offset both
    operands are plain slices -- one row-split GEMM per run (3 on the line graph).  Hx / D1x [N,rows,H] contiguous."""
    N, m = nbr_idx.shape
    out = torch.zeros(N, m * H, H, dtype=F32, device=Hx.device)      # slots an agent does not have: zero gradient
    for i0, i1, k, d in ops.nbr_derived(nbr_idx, 'gather runs', lambda: _gather_runs(nbr_idx)):
        ops.wgrad(Hx[i0 + d:i1 + d], D1x[i0:i1], out=out[i0:i1, k * H:(k + 1) * H])
    return out


def coupled_sequence_saved(kind, nbr_idx, masked_steps, enc, done, wx, wh, b, w_msg, b_msg, mfc_w, mfc_b, G, Hall, Call, S,
                           extra, s_ext=None):
    """enc [N,T,E,W] (autograd-connected h-independent part), saved activations of the rollout -> Hs [N,T,E,H].
    s_ext (optional): the [N,T+1,E,KX] buffer S is the first T slabs of (last slab zero): in-place weight gradients."""
    return CoupledSequenceSaved.apply(kind, nbr_idx, masked_steps, enc, done, wx, wh, b, w_msg, b_msg, mfc_w, mfc_b, G, Hall,
                                      Call, S, extra.get('A1'), extra.get('A2'), s_ext)


def coupled_sequence(kind, nbr_idx, masked_steps, enc, h0, c0, done, wx, wh, b, w_msg, b_msg, mfc_w=None, mfc_b=None):
    """enc [N,T,E,W] -> Hs [N,T,E,H]; see the module docstring."""
    return CoupledSequence.apply(kind, nbr_idx, masked_steps, enc, h0, c0, done, wx, wh, b, w_msg, b_msg, mfc_w, mfc_b)

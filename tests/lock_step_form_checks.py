"""The launches of one rollout batch, form by form (run by test_lock_step_forms_cpu.py on the restated ops and by
test_gpu_lock_step_forms.py on the kernels): ONE eager batch of a small trainer with the step ops, the encoder launch and the env step
wrapped; every call is recorded as (entry, {operand: buffer slot}, non-None keys of the message dict, non-None keys of the in-launch
encoders' description, defer_action_term, the draw's step) and compared with the sequence written out below.  An operand is named by
its address, shape and strides against the model's rollout buffers, so a launch that reads or writes another slot -- or the same slot
through another view -- is a difference.

The expected sequences are written per form from what a lock-step IS, not from the host code: they hold for any host
code that issues the parent's launches."""
import contextlib

import torch

T = 3           # lock-steps per batch; t = T is the bootstrap step
E = 3


# ------------------------------------------------------------------------------------------------------ naming operands
def _slots(model, tr):
    """[(name, tensor)]: every slot of the rollout buffers a lock-step launch may touch."""
    p = model.policy
    out = [('h_fw', model.h_fw), ('c_fw', model.c_fw), ('_h2', model._h2), ('_c2', model._c2), ('_pi_boot', model._pi_boot),
           ('_v_boot', model._v_boot), ('action_boot', tr.action_boot), ('done_pre', tr.done_pre), ('zero_done', tr.zero_done)]
    if model._carry_buf is not None:
        out.append(('carry', model._carry_buf))
    if getattr(model, '_enc_boot', None) is not None:
        out.append(('enc_boot', model._enc_boot))
    for (name, _, _), buf in getattr(p, '_scratch_pool', {}).items():
        out.append((name, buf))
    n = model.n_step
    for t in range(n + 1):
        out += [('x[%d]' % t, model.buf_x[t]), ('fp[%d]' % t, model.buf_fp[t])]
        if model.save_acts:
            out += [('H[%d]' % t, model.H_all[:, t]), ('C[%d]' % t, model.C_all[:, t]), ('S[%d]' % t, model.S_ext[:, t])]
            out += [('%s[%d]' % (k, t), v[:, t]) for k, v in p._extra_full.items() if t < v.shape[1]]
    for t in range(n):
        out += [('act[%d]' % t, model.buf_act[t]), ('v[%d]' % t, model.buf_v[t])]
        if model.save_acts:
            out += [('G[%d]' % t, model.G_buf[:, t]), ('vn[%d]' % t, model.buf_vn[:, t])]
            if model.S_bits is not None:
                out.append(('bits[%d]' % t, model.S_bits[:, t]))
    return out


def _key(t):
    return (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.element_size())


def _name(key, slots):
    """The slot a recorded operand is: the whole slot, or columns [a:b] of its rows."""
    ptr, shape, stride, es = key
    for name, s in slots:
        if s.element_size() != es or s.dim() != len(shape) or tuple(s.shape[:-1]) != shape[:-1] or tuple(s.stride()) != stride:
            continue
        off = (ptr - s.data_ptr()) // es
        if (ptr - s.data_ptr()) % es == 0 and 0 <= off and off + shape[-1] <= s.shape[-1]:
            return name if shape[-1] == s.shape[-1] else '%s[%d:%d]' % (name, off, off + shape[-1])
    return '?%s' % (shape,)


# ------------------------------------------------------------------------------------------------------ recording
def _msg_keys(msg):
    """The non-None keys of a message dict a form adds or fills (the weights, `kind` and `img` are always there)."""
    own = ('enc', 'out', 'mean_out', 'sync', 'carry_in', 'carry_out', 'mean_next', 'ob', 'enc_spec', 'genv', 'src', 'out2', 'next')
    return tuple(k for k in own if msg.get(k) is not None)


def _spec_keys(spec):
    return tuple(k for k in ('out', 'env', 'bits') if spec.get(k) is not None)


@contextlib.contextmanager
def recorded(ops, model, env):
    """-> list of [entry, {operand: tensor}, msg keys, encoder keys, defer_action_term, step] in call order.  (The tensors themselves
    are kept until they are named: a temporary's address is not handed out again while the batch runs.)"""
    calls = []
    p = model.policy

    def operands(rec, xs, **named):
        for k, v in named.items():
            if torch.is_tensor(v):
                rec[1][k] = v
        if xs is None:
            return
        x = xs[0]
        if isinstance(x, dict):             # the in-launch encoders' description (uncoupled nets)
            rec[3] = _spec_keys(x)
            rec[1].update({'enc.' + k: x[k] for k in ('ob', 'fp', 'out', 'bits') if x.get(k) is not None})
        elif x is not None:
            rec[1]['x'] = x
        if len(xs) > 3 and xs[3] is not None:
            rec[1]['x2'] = xs[3]
        msg = xs[4] if len(xs) > 4 else None
        if msg is not None:
            rec[2] = _msg_keys(msg)
            rec[1].update({'msg.' + k: msg[k] for k in ('enc', 'out', 'mean_out', 'carry_in', 'carry_out', 'mean_next')
                           if msg.get(k) is not None})
            if msg.get('ob') is not None:
                rec[1]['msg.ob.x'] = msg['ob']['x']
            if msg.get('enc_spec') is not None:
                spec = msg['enc_spec']
                rec[3] = _spec_keys(spec)
                rec[1].update({'enc.' + k: spec[k] for k in ('ob', 'fp', 'out', 'bits') if spec.get(k) is not None})

    o_p, o_v, o_pv, o_enc, o_step = ops.lstm_step_policy, ops.lstm_step_value, ops.lstm_step_policy_value, p.encode, env.step
    o_in = getattr(env, 'inkernel_step', None)

    def policy(h, wh, b, z1, z2, c, done, c_out, h_out, pi_w, pi_b, pi_out, act_out, xs=None, gates=None, **kw):
        rec = ['policy', {}, (), (), None, kw.get('step')]
        operands(rec, xs, h=h, c=c, done=done, h_out=h_out, c_out=c_out, pi=pi_out, act=act_out, gates=gates)
        calls.append(rec)
        return o_p(h, wh, b, z1, z2, c, done, c_out, h_out, pi_w, pi_b, pi_out, act_out, xs=xs, gates=gates, **kw)

    def value(h, wh, b, z1, z2, c, done, c_out, h_out, v_w, v_b, action, nbr_idx, n_a, v_out, xs=None, **kw):
        rec = ['value', {}, (), (), None, None]
        operands(rec, xs, h=h, c=c, done=done, h_out=h_out, c_out=c_out, act=action, v=v_out)
        calls.append(rec)
        return o_v(h, wh, b, z1, z2, c, done, c_out, h_out, v_w, v_b, action, nbr_idx, n_a, v_out, xs=xs, **kw)

    def policy_value(h, wh, b, z1, z2, c, done, pi_w, pi_b, pi_out, act_out, v_w, v_b, nbr_idx, n_a, v_out, xs=None, h_out=None,
                     c_out=None, gates=None, defer_action_term=False, **kw):
        rec = ['policy_value', {}, (), (), bool(defer_action_term), kw.get('step')]
        operands(rec, xs, h=h, c=c, done=done, h_out=h_out, c_out=c_out, pi=pi_out, act=act_out, v=v_out, gates=gates)
        calls.append(rec)
        return o_pv(h, wh, b, z1, z2, c, done, pi_w, pi_b, pi_out, act_out, v_w, v_b, nbr_idx, n_a, v_out, xs=xs, h_out=h_out,
                    c_out=c_out, gates=gates, defer_action_term=defer_action_term, **kw)

    def encode(x, fp, out=None):
        rec = ['encode', {}, (), (), None, None]
        operands(rec, None, x=x, fp=fp, out=out)
        calls.append(rec)
        return o_enc(x, fp) if out is None else o_enc(x, fp, out=out)

    def step(action, **kw):
        rec = ['env.step', {}, (), (), None, None]
        operands(rec, None, act=action, obs_out=kw.get('obs_out'))
        if kw.get('encode') is not None:
            rec[3] = ('encode',)
            rec[1]['enc.out'] = kw['encode']['out']
        calls.append(rec)
        return o_step(action, **kw)

    def inkernel_step(**kw):
        rec = ['env.inkernel_step', {}, (), (), None, None]
        operands(rec, None, obs_out=kw.get('obs_out'))
        calls.append(rec)
        return o_in(**kw)

    ops.lstm_step_policy, ops.lstm_step_value, ops.lstm_step_policy_value, p.encode, env.step = policy, value, policy_value, encode, step
    if o_in is not None:
        env.inkernel_step = inkernel_step
    try:
        yield calls
    finally:
        ops.lstm_step_policy, ops.lstm_step_value, ops.lstm_step_policy_value = o_p, o_v, o_pv
        del p.encode, env.step
        if o_in is not None:
            del env.inkernel_step


def run_one_batch(ops, model, env, tr):
    """One eager batch -> ([(entry, {operand: slot name}, msg keys, encoder keys, defer_action_term, step)], the policy's
    rollout_saved() flags as the update found them)."""
    flags = []
    grads, p = model.update_grads, model.policy

    def update_grads(R_end):
        # (the three attributes themselves, not policy.rollout_saved(): the sequences are also checked against code without it)
        flags.append((getattr(p, '_enc_was_saved', False), getattr(p, '_mm_was_saved', False), p._bits_steps))
        return grads(R_end)

    model.update_grads = update_grads
    try:
        with recorded(ops, model, env) as calls:
            tr.run_batch()
    finally:
        del model.update_grads
    slots = _slots(model, tr)
    named = [(c[0], {k: _name(_key(v), slots) for k, v in sorted(c[1].items())}, c[2], c[3], c[4], c[5]) for c in calls]
    return named, flags[0]


# ------------------------------------------------------------------------------------------------------ what a batch launches
NETS = {'ia2c': 'x64', 'ma2c_cu': 'x64', 'ia2c_fp': 'x128', 'ma2c_nc': 'nc', 'ma2c_ic3': 'ic3', 'ma2c_dial': 'dial'}


def expected(net, N, E, n_step, saved=True, launches=1, enc='launch', carry=False, bits=False, env_in=False):
    """The launches of one batch, lock-step by lock-step (t = n_step: the bootstrap step).
    net: NETS' kinds -- 'x64' / 'x128' uncoupled, the LSTM input 64 / 128 wide; 'nc': [hx | hp | hm], the message third written by
    the step; 'ic3': enc + message term, the encoder output kept in the ENC slots; 'dial'.
    enc: where lock-step t's LSTM input comes from -- 'launch': an encoder launch; 'both' / 'ob': encoders inside the step's launch;
    'pre': the env kernel encoded it behind the step of lock-step t - 1 (lock-step 0: an encoder launch).
    env_in: the env step is inside the step's launch too (announced by env.inkernel_step in front of it)."""
    T = n_step
    tmp = lambda w: '?(%d, %d, %d)' % (N, E, w)
    seq = []
    for t in range(T + 1):
        boot = t == T
        done = 'done_pre' if t == 0 else 'zero_done'
        pi, act = ('_pi_boot', 'action_boot') if boot else ('fp[%d]' % (t + 1), 'act[%d]' % t)
        src = 'launch' if (enc == 'pre' and t == 0) else enc
        keep = saved and not boot                      # the step's results go to slot t / t + 1 of the saved activations
        if src == 'launch':
            o = {'x': 'x[%d]' % t, 'fp': 'fp[%d]' % t}
            if keep:
                o['out'] = ('ENC[%d]' if net == 'ic3' else 'S[%d]') % t
            seq.append(('encode', o, (), (), None, None))
        if env_in and not boot:
            seq.append(('env.inkernel_step', {'obs_out': 'x[%d]' % (t + 1)}, (), (), None, None))
        # the state: slot t -> slot t + 1 of the sequences (bootstrap: -> the persistent state), or the persistent state in place
        o = {'h': 'H[%d]' % t, 'c': 'C[%d]' % t} if saved else {'h': 'h_fw', 'c': 'c_fw'}
        o.update(done=done, pi=pi, act=act)
        h_out, c_out = ('H[%d]' % (t + 1), 'C[%d]' % (t + 1)) if keep else ('h_fw', 'c_fw')
        if keep:
            o['gates'] = 'G[%d]' % t
        one = launches == 1
        if one:
            o['v'] = '_v_boot' if boot else ('vn[%d]' if saved else 'v[%d]') % t
        if saved or not one:
            o.update(h_out=h_out, c_out=c_out)
        # the input slot: slot t of the saved inputs, the bootstrap scratch where something outside `encode` writes it, a temporary
        slot = 'S[%d]' % t if keep else ('enc_boot' if (saved and src != 'launch') else None)
        msg, spec = [], []
        if src == 'both':
            o.update({'enc.ob': 'x[%d]' % t, 'enc.fp': 'fp[%d]' % t})
            if keep and net != 'nc':                   # (a coupled net's encoders write through the step's x slot)
                o['enc.out'] = slot
                spec.append('out')
            if env_in and not boot:
                spec.append('env')
            if bits and keep:
                o['enc.bits'] = 'bits[%d]' % t
                spec.append('bits')
        value = None                                   # the second launch's operands, where there is one
        if not one:
            value = dict(h=h_out, c=c_out, h_out='_h2', c_out='_c2', done=done, act=act, v='_v_boot' if boot else 'v[%d]' % t)
        vmsg = []
        if net in ('x64', 'x128'):
            if src != 'both':
                o['x'] = slot or tmp(64 if net == 'x64' else 128)
        elif net == 'nc':
            if not saved:                              # the pair, in place: the step's message term comes from a launch in front of it
                o['x'], value['x'] = tmp(192), tmp(128)
            else:
                o['x'], o['msg.out'] = (slot + '[0:128]', slot + '[128:192]') if slot else (tmp(128), tmp(64))
                msg.append('out')
                if not one:
                    value['x'] = o['x']
        elif net == 'ic3':
            o['msg.enc'] = 'ENC[%d]' % t if keep else (slot or tmp(64))
            msg.append('enc')
            if keep:
                o.update({'msg.out': 'S[%d]' % t, 'msg.mean_out': 'MM[%d]' % t})
                msg += ['out', 'mean_out']
            if not one:
                value['msg.enc'] = o['msg.enc']
                vmsg = ['enc']
        elif net == 'dial':                            # (msg.enc, the sender layer's cached output, is not a rollout buffer: not compared)
            msg += ['enc', 'out', 'src', 'out2', 'next'] if keep else ['enc', 'src', 'next']
            if keep:
                o['msg.out'] = 'S[%d]' % t
            vmsg = ['enc', 'src']
        if one and net in ('nc', 'ic3'):
            msg.append('sync')
            if carry and t > 0:
                o['msg.carry_in'] = 'carry'
                msg.append('carry_in')
            if carry and not boot:
                o['msg.carry_out'] = 'carry'
                msg.append('carry_out')
            if carry and net == 'ic3' and t + 1 < T:
                o['msg.mean_next'] = 'MM[%d]' % (t + 1)
                msg.append('mean_next')
            if src == 'ob':
                o['msg.ob.x'] = 'x[%d]' % t
                msg.append('ob')
            if src == 'both':
                msg.append('enc_spec')
            if src == 'ob' and env_in and not boot:
                msg.append('genv')
        if one:
            seq.append(('policy_value', o, tuple(msg), tuple(spec), keep, t))
        else:
            seq.append(('policy', o, tuple(msg), (), None, t))
            seq.append(('value', value, tuple(vmsg), (), None, None))
        if not boot and not env_in:
            o = {'act': act, 'obs_out': 'x[%d]' % (t + 1)}
            if enc == 'pre':                           # ... and lock-step t + 1's input encoders behind it
                o['enc.out'] = 'S[%d]' % (t + 1) if t + 1 < T else 'enc_boot'
            seq.append(('env.step', o, (), ('encode',) if enc == 'pre' else (), None, None))
    return seq


def check_batch(ops, model, env, tr, net, **form):
    """One eager batch of `tr` launches exactly `expected(net, **form)`; -> the flags the update found."""
    got, flags = run_one_batch(ops, model, env, tr)
    want = expected(net, model.n_agent, model.E, model.n_step, **form)
    if net == 'dial':
        got = [(c[0], {k: v for k, v in c[1].items() if k != 'msg.enc'}) + c[2:] for c in got]
    assert [c[0] for c in got] == [c[0] for c in want], 'the order of launches differs: %s' % ([c[0] for c in got],)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, 'launch %d (%s):\n  got      %r\n  expected %r' % (k, g[0], g, w)
    return flags

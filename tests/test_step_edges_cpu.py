"""The edge checks of tests/step_edge_checks.py are sharp: (a) the restatement oracle/ops_ref (fp32 on the CPU) stays within every
bound, (b) every named wrong variant of it -- mistakes the lock-step kernel of csrc/lstm_mfma.hip could make without the older
tests noticing -- makes the check that targets it raise.

The variants of the two-piece input, of the split product and of the row edges wrap the restatement's entry points (or replace
one helper of it for the duration of a call); the variants of the done mask need the mask taken out of single operands, so
`_Steps` below restates the plain forms (no message term, no encoders) with one switch per mask --
test_steps_without_a_mistake_are_the_restatement shows that with every switch off it is ops_ref bit for bit."""
import contextlib
import types

import pytest
import torch

import step_edge_checks as sec
from oracle import ops_ref

H = sec.H
_NAMES = ('lstm_wimage', 'lstm_msg_wimage', 'lstm_step_fused', 'lstm_step_policy', 'lstm_step_value', 'lstm_step_policy_value',
          'step_enc_spec', 'check_precision')
_STEPS = ('lstm_step_fused', 'lstm_step_policy', 'lstm_step_value', 'lstm_step_policy_value')


def _impl(**replaced):
    ns = types.SimpleNamespace(**{k: getattr(ops_ref, k) for k in _NAMES})
    for k, v in replaced.items():
        setattr(ns, k, v)
    return ns


def _wrap_steps(pre=None, post=None, patch=None):
    """An implementation whose four step entry points are ops_ref's with `pre(kwargs-of-xs)` applied to xs, `post(name, args, kw)`
    run behind the call, and `patch` = (attribute of ops_ref, replacement) in force during it."""
    def make(name):
        fn = getattr(ops_ref, name)

        def f(*args, **kw):
            if pre is not None and kw.get('xs') is not None:
                kw['xs'] = pre(kw['xs'])
            with _patched(patch):
                out = fn(*args, **kw)
            if post is not None:
                post(name, args, kw)
            return out
        return f
    return _impl(**{n: make(n) for n in _STEPS})


@contextlib.contextmanager
def _patched(patch):
    if patch is None:
        yield
        return
    name, repl = patch
    orig = getattr(ops_ref, name)
    setattr(ops_ref, name, repl)
    try:
        yield
    finally:
        setattr(ops_ref, name, orig)


# ------------------------------------------------------------------------------------------ (a) the restatement passes
@pytest.mark.parametrize('split,precision', [(s, 'fp32') for s in sec.TWO_PIECE_SPLITS] + [(s, 'bf16x3') for s in sec.TWO_PIECE_X3_SPLITS])
@pytest.mark.parametrize('E', sec.TWO_PIECE_E)
def test_restatement_two_piece(E, split, precision):
    for pitch in sec.TWO_PIECE_PITCH:
        for head in sec.TWO_PIECE_HEADS:
            for addends in (0, 1):
                sec.check_two_piece(_impl(), 'cpu', 3, E, split[0], split[1], pitch, head, addends, precision)


@pytest.mark.parametrize('form', sec.X3_FORMS)
@pytest.mark.parametrize('E', sec.X3_E)
def test_restatement_bf16x3_form(E, form):
    for KX, addends in ([(128 if form == 'enc_pair' else 64, 0)] if form.startswith('enc') else sec.X3_KX):
        sec.check_bf16x3_form(_impl(), 'cpu', form, 3, E, KX, addends)


@pytest.mark.parametrize('form', sec.ROW_EDGE_HEAD_FORMS)
@pytest.mark.parametrize('E', sec.ROW_EDGE_E)
def test_restatement_row_edges(E, form):
    for KX, addends in sec.ROW_EDGE_KX:
        for A in ((1, 8) if form in ('head1', 'head3') else (4,)):
            sec.check_row_edges(_impl(), 'cpu', form, E, KX=KX, addends=addends, A=A)
        if form == 'head2':
            sec.check_row_edges(_impl(), 'cpu', form, E, KX=KX, addends=addends, m_max=0)


@pytest.mark.parametrize('form', sec.ROW_EDGE_MSG_FORMS)
@pytest.mark.parametrize('E', sec.ROW_EDGE_E)
def test_restatement_row_edges_message_forms(E, form):
    sec.check_row_edges(_impl(), 'cpu', form, E)


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('head', sec.DONE_HEADS)
def test_restatement_done_mask(head, precision):
    sec.check_done_mask(_impl(), 'cpu', head, precision)


# ------------------------------------------------------------------------------------------ (b) the wrong variants fail
def _reread(t, sn, row, col0, K):
    """What a kernel reads that takes t's pointer but walks it with the agent stride `sn` and the row pitch `row`, K columns from
    column col0 (indices past t's allocation read its last element: the CPU has no wild reads)."""
    base = t if t._base is None else t._base
    flat = base.reshape(-1)
    N, E, _ = t.shape
    idx = (t.storage_offset() - base.storage_offset() + torch.arange(N).view(N, 1, 1) * sn + torch.arange(E).view(1, E, 1) * row
           + col0 + torch.arange(K).view(1, 1, K)).clamp(max=flat.numel() - 1)
    return flat[idx]


def _x2_variant(kind):
    def pre(xs):
        if len(xs) < 4 or xs[3] is None:
            return xs
        x, wx, img, x2 = xs[:4]
        if kind == 'x2 in front of x':
            return (x2, wx, img, x) if x is not None else xs
        if kind == 'x2 read with the row pitch of x':
            x2 = _reread(x2, x2.stride(0), x.stride(1), 0, x2.shape[2])
        elif kind == 'x2 read with the agent stride of x':
            x2 = _reread(x2, x.stride(0), x2.stride(1), 0, x2.shape[2])
        elif kind == 'the last chunk of x2 dropped':
            x2 = x2.clone()
            x2[..., -32:] = 0.0
        elif kind == 'chunk nx1 taken from x':
            x2 = x2.clone()
            x2[..., :32] = _reread(x, x.stride(0), x.stride(1), x.shape[2], 32)
        else:
            raise KeyError(kind)
        return (x, wx, img, x2)
    return _wrap_steps(pre=pre)


TWO_PIECE_MUTANTS = ['x2 in front of x', 'x2 read with the row pitch of x', 'x2 read with the agent stride of x', 'the last chunk of x2 dropped',
                     'chunk nx1 taken from x']


@pytest.mark.parametrize('pitch', sec.TWO_PIECE_PITCH)
@pytest.mark.parametrize('head', sec.TWO_PIECE_HEADS)
@pytest.mark.parametrize('name', TWO_PIECE_MUTANTS)
def test_two_piece_mutant_fails(name, head, pitch):
    for split in ((128, 64), (224, 32)):
        with pytest.raises(AssertionError, match=r'^\[bits\]'):
            sec.check_two_piece(_x2_variant(name), 'cpu', 3, 17, split[0], split[1], pitch, head, 0, 'fp32')
    with pytest.raises(AssertionError, match=r'^\[bits\]'):
        sec.check_two_piece(_x2_variant(name), 'cpu', 3, 129, 128, 64, pitch, head, 1, 'bf16x3')


def _split_trunc(a):
    """bf16_split with lo TRUNCATED (toward zero) instead of rounded to nearest even."""
    a32 = a.float()
    hi = a32.to(torch.bfloat16).float()
    lo = ((a32 - hi).view(torch.int32) & -65536).view(torch.float32)
    return hi.to(a.dtype), lo.to(a.dtype)


def _product_variant(kind):
    def f(a, w, precision='fp32'):
        if precision == 'fp32' or kind == 'the fp32 product under the bf16x3 label':
            return torch.bmm(a, w)
        split = _split_trunc if kind == 'lo truncated instead of rounded' else ops_ref.bf16_split
        ah, al = split(a)
        wh, wl = split(w)
        if kind == 'the lo_a hi_b term left out':
            return torch.bmm(ah, wh) + torch.bmm(ah, wl)
        return torch.bmm(ah, wh) + torch.bmm(ah, wl) + torch.bmm(al, wh)
    return f


def _restep_fp32(h, wh, bias, zadd1, zadd2, c, done, pi_w, pi_b, pi_out, act_out, v_w, v_b, nbr_idx, n_a, v_out, mode, u=None, seed=0,
                 env_id_base=0, step=0, step_dev=None, xs=None, h_out=None, c_out=None, gates=None, defer_action_term=False, precision='fp32'):
    """ops_ref.lstm_step_policy_value (action term deferred) whose value re-step runs the fp32 product whatever the precision."""
    assert defer_action_term
    if isinstance(xs[0], dict):
        xs = (ops_ref.step_enc_forward(xs[0]),) + tuple(xs[1:])
    ops_ref.lstm_step_fused(h, wh, bias, zadd1, zadd2, c, done, gates, torch.empty_like(c), torch.empty_like(h), xs=xs, precision=precision)
    ops_ref.lstm_step_policy(h, wh, bias, zadd1, zadd2, c, done, c_out, h_out, pi_w, pi_b, pi_out, act_out, mode, u=u, seed=seed,
                             env_id_base=env_id_base, step=step, step_dev=step_dev, xs=xs, precision=precision)
    hv, cv = torch.empty_like(h), torch.empty_like(c)
    ops_ref.lstm_step_fused(h_out, wh, bias, zadd1, zadd2, c_out, done, None, cv, hv, xs=xs, precision='fp32')
    v_out.copy_((torch.bmm(hv, v_w[:, :H]) + v_b.unsqueeze(1)).squeeze(-1))
    return pi_out, act_out, v_out


X3_MUTANTS = {
    'the lo_a hi_b term left out': None,
    'lo truncated instead of rounded': None,
    'the fp32 product under the bf16x3 label': None,
    'the value re-step in fp32 while the policy step is split': None,
}


def _x3_variant(name):
    if name == 'the value re-step in fp32 while the policy step is split':
        return _impl(lstm_step_policy_value=_restep_fp32)
    return _wrap_steps(patch=('step_product', _product_variant(name)))


@pytest.mark.parametrize('name', list(X3_MUTANTS))
def test_bf16x3_mutant_fails(name):
    forms = ['head3', 'enc_pair', 'enc_single_m2'] if name.startswith('the value re-step') else sec.X3_FORMS
    for form in forms:
        cases = [(128 if form == 'enc_pair' else 64, 0)] if form.startswith('enc') else [(0, 1), (128, 1)]
        for KX, addends in cases:
            with pytest.raises(AssertionError, match=r'^\[(x3|x3-pi|x3-v|discriminate|restep-x3)\]'):
                sec.check_bf16x3_form(_x3_variant(name), 'cpu', form, 3, 129, KX, addends)


def test_bf16x3_variants_without_a_mistake_pass():
    sec.check_bf16x3_form(_wrap_steps(patch=('step_product', _product_variant(None))), 'cpu', 'head3', 3, 129, 128, 1)


def _row_variant(kind):
    def post(name, args, kw):
        h_out = kw['h_out'] if name == 'lstm_step_policy_value' else args[9] if name == 'lstm_step_fused' else args[8]
        N, E, W = h_out.shape
        if kind == 'row E - 1 left unwritten':
            h_out[:, E - 1] = sec.SENTINEL
        else:
            h_out._base.view(N, 3, E, W)[:, 2, 0] = 0.0            # row E of slot 1 is row 0 of slot 2
    if kind in ('row E - 1 left unwritten', 'row E written'):
        return _wrap_steps(post=post)
    if kind == 'the agent without neighbours given the rows of agent 0':
        def pre(xs):
            if len(xs) < 5 or xs[4] is None:
                return xs
            tab = xs[4]['nbr_idx'].clone()
            tab[(tab < 0).all(dim=1), 0] = 0
            return tuple(xs[:4]) + (dict(xs[4], nbr_idx=tab),)
        return _wrap_steps(pre=pre)
    assert kind == 'the mean divided by m_max'
    return _wrap_steps(patch=('nbr_mean', lambda x, tab: ops_ref.nbr_gather(x, tab).view(*x.shape[:2], tab.shape[1], x.shape[2]).sum(2) / tab.shape[1]))


ROW_MUTANTS = {
    'row E - 1 left unwritten': (sec.ROW_EDGE_HEAD_FORMS + sec.ROW_EDGE_MSG_FORMS, r'^\[written\]'),
    'row E written': (sec.ROW_EDGE_HEAD_FORMS + sec.ROW_EDGE_MSG_FORMS, r'^\[slots\]'),
    'the agent without neighbours given the rows of agent 0': (sec.ROW_EDGE_MSG_FORMS, r'^\[(msg|close)\]'),
    'the mean divided by m_max': (['msg2+head1', 'msg2+head2'], r'^\[(msg|close)\]'),
}


@pytest.mark.parametrize('E', [16, 129])
@pytest.mark.parametrize('name', list(ROW_MUTANTS))
def test_row_edge_mutant_fails(name, E):
    forms, tag = ROW_MUTANTS[name]
    for form in forms:
        with pytest.raises(AssertionError, match=tag):
            sec.check_row_edges(_row_variant(name), 'cpu', form, E)


class _Steps:
    """The plain forms (no message term, no encoders) of the four step entry points, the (1 - done) masks switchable one by one."""

    def __init__(self, mask_h=True, mask_c=True, restep_mask_h=True, restep_mask_c=True, shifted=False):
        self.mask_h, self.mask_c, self.restep_mask_h, self.restep_mask_c, self.shifted = mask_h, mask_c, restep_mask_h, restep_mask_c, shifted
        self.lstm_wimage, self.check_precision = ops_ref.lstm_wimage, ops_ref.check_precision

    def _keep(self, done):
        keep = (1.0 - done).view(1, -1, 1)
        return torch.cat([keep[:, :1], keep[:, :-1]], dim=1) if self.shifted else keep        # the mask of row e taken from row e - 1

    def _step(self, h, wh, bias, zadd1, zadd2, c_prev, done, xs, precision, mask_h, mask_c):
        keep = self._keep(done)
        z = ops_ref.step_product(h * keep if mask_h else h, wh, precision)
        if xs[0] is not None:
            z = z + ops_ref.step_product(xs[0], xs[1], precision)
        for zz in (zadd1, zadd2):
            if zz is not None:
                z = z + zz
        zb = z + bias.unsqueeze(1)
        i, f, o, u = zb.split(H, dim=-1)
        i, f, o, u = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(u)
        c = f * (c_prev * keep if mask_c else c_prev) + i * u
        return torch.cat([i, f, o, u], dim=-1), c, o * torch.tanh(c)

    def lstm_step_fused(self, h, wh, bias, zadd1, zadd2, c_prev, done, gates, c_out, h_out, xs=None, precision='fp32'):
        g, c, hn = self._step(h, wh, bias, zadd1, zadd2, c_prev, done, xs, precision, self.mask_h, self.mask_c)
        if gates is not None:
            gates.copy_(g)
        c_out.copy_(c)
        h_out.copy_(hn)
        return h_out, c_out

    def lstm_step_value(self, h, wh, bias, zadd1, zadd2, c_prev, done, c_out, h_out, v_w, v_b, action, nbr_idx, n_a, v_out, xs=None,
                        precision='fp32'):
        self.lstm_step_fused(h, wh, bias, zadd1, zadd2, c_prev, done, None, c_out, h_out, xs=xs, precision=precision)
        na = ops_ref.nbr_onehot(action, nbr_idx, n_a)
        v_out.copy_((torch.bmm(torch.cat([h_out, na], dim=-1), v_w) + v_b.unsqueeze(1)).squeeze(-1))
        return v_out

    def lstm_step_policy_value(self, h, wh, bias, zadd1, zadd2, c, done, pi_w, pi_b, pi_out, act_out, v_w, v_b, nbr_idx, n_a, v_out, mode,
                               u=None, seed=0, env_id_base=0, step=0, step_dev=None, xs=None, h_out=None, c_out=None, gates=None,
                               defer_action_term=False, precision='fp32'):
        assert defer_action_term
        g, cn, hn = self._step(h, wh, bias, zadd1, zadd2, c, done, xs, precision, self.mask_h, self.mask_c)
        if gates is not None:
            gates.copy_(g)
        c_out.copy_(cn)
        h_out.copy_(hn)
        pi_out.copy_(torch.softmax(torch.bmm(h_out, pi_w) + pi_b.unsqueeze(1), dim=-1))
        ops_ref.sample_actions(pi_out, act_out, mode, u=u, seed=seed, env_id_base=env_id_base, step=step, step_dev=step_dev)
        _, _, hv = self._step(h_out, wh, bias, zadd1, zadd2, c_out, done, xs, precision, self.restep_mask_h, self.restep_mask_c)
        v_out.copy_((torch.bmm(hv, v_w[:, :H]) + v_b.unsqueeze(1)).squeeze(-1))
        return pi_out, act_out, v_out


DONE_MUTANTS = {
    'no mask on c_prev': (dict(mask_c=False), sec.DONE_HEADS),
    'no mask on h_in': (dict(mask_h=False), sec.DONE_HEADS),
    'the re-step without the mask on h\'': (dict(restep_mask_h=False), [3]),
    'the re-step without the mask on c\'': (dict(restep_mask_c=False), [3]),
    'the mask of row e taken from row e - 1': (dict(shifted=True), sec.DONE_HEADS),
}


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('name', list(DONE_MUTANTS))
def test_done_mask_mutant_fails(name, precision):
    flags, heads = DONE_MUTANTS[name]
    for head in heads:
        with pytest.raises(AssertionError, match=r'^\[(bits|close|restep|x3-v|x3)\]'):
            sec.check_done_mask(_Steps(**flags), 'cpu', head, precision)


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('head', sec.DONE_HEADS)
def test_steps_without_a_mistake_are_the_restatement(head, precision):
    """_Steps with every switch off == ops_ref bit for bit (the variants differ from the restatement by their one mistake alone),
    and passes the check."""
    d = sec._done_inputs(head, precision, False)
    a = sec.run_step(_Steps(), 'cpu', d, head, x=d['x'], precision=precision)
    b = sec.run_step(_impl(), 'cpu', d, head, x=d['x'], precision=precision)
    sec.same_outputs(a, b, head, 'the switchable restatement')
    sec.check_done_mask(_Steps(), 'cpu', head, precision)


def test_every_named_variant_is_there():
    """The issue names 5 + 4 + 4 + 5 wrong variants; none is silently dropped."""
    assert len(TWO_PIECE_MUTANTS) == 5 and len(X3_MUTANTS) == 4 and len(ROW_MUTANTS) == 4 and len(DONE_MUTANTS) == 5

"""Opt-in replica minibatches of the PPO epochs (MODEL_CONFIG ppo_minibatches), without a GPU: the restated permutation, the literal
update against its wrong variants, the config / CLI layers and the call order of an update on the torch path (the HIP-op wrappers
replaced by the restatements of tests/ppo_minibatch_checks.py)."""
import configparser
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import ppo_minibatch_checks as mc
from cpu_emulation import cpu_ops
from helpers import cacc_config
from test_ppo_vclip_kl_cpu import _build, spied_ops


# ------------------------------------------------------------------------------------------------------------------ permutation
@pytest.mark.parametrize('E', [1, 2, 3, 64, 77, 1000])
def test_restated_permutation_is_a_permutation(E):
    p = mc.perm(E, 2, 0, 12)
    assert p.dtype == np.int32 and sorted(p.tolist()) == list(range(E))
    assert np.array_equal(p, mc.perm(E, 2, 0, 12))
    if E <= 77:
        assert np.array_equal(p, mc.rank_literal(mc.keys(E, 2, 0, 12)))
    if E >= 64:         # (E! orderings: two independent draws of 64 or more agree with probability < 1e-89)
        assert not np.array_equal(p, mc.perm(E, 3, 0, 12)) and not np.array_equal(p, mc.perm(E, 2, 1, 12))
        assert not np.array_equal(p, mc.perm(E, 2, 0, 13)) and not np.array_equal(p, mc.perm(E, 2, 0, 12, env_id_base=E))
        assert not np.array_equal(p, np.arange(E))


def test_a_shard_draws_the_keys_of_its_global_replicas():
    whole = mc.keys(24, 2, 5, 12)
    assert np.array_equal(mc.keys(12, 2, 5, 12, env_id_base=12), whole[12:])
    assert np.array_equal(mc.keys(12, 2, 5, 12 + (7 << 32)), mc.keys(12, 2, 5, 12 + (7 << 32))) and \
        not np.array_equal(mc.keys(12, 2, 5, 12 + (7 << 32)), whole[:12])          # the seed's high word is part of the key


def test_forced_key_ties_fall_back_to_index_order():
    k = np.array([5, 1, 5, 1, 1, 9, 0], dtype=np.uint32)
    assert mc.perm_of_keys(k).tolist() == [6, 1, 3, 4, 0, 2, 5] == mc.rank_literal(k).tolist()
    assert mc.perm_of_keys(np.zeros(9, dtype=np.uint32)).tolist() == list(range(9))
    assert mc.perm_of_keys(np.array([0xFFFFFFFF, 0x80000000, 0x7FFFFFFF], dtype=np.uint32)).tolist() == [2, 1, 0]     # unsigned order


def test_gather_is_fancy_indexing():
    src = torch.arange(3 * 5 * 2, dtype=torch.float32).reshape(3, 5, 2)
    got = mc.gather_rows(src, [4, 0], 3, 5)
    assert torch.equal(got, src[:, [4, 0]]) and got.is_contiguous()


# ------------------------------------------------------------------------------------------------------------------ literal update
def _toy_perm(k):
    return mc.perm(mc.Toy.E, k, 0, 12)


def test_literal_update_equals_itself_and_its_one_group_form_is_plain_ppo():
    toy = mc.Toy()
    a, b = toy.update(3, 2, _toy_perm), toy.update(3, 2, _toy_perm)
    assert not mc.differs(a, b, tol=0.0)
    # M = 1: the grouping does not matter (one group of every replica, a mean over all rows) up to the order of the sums
    one = toy.update(3, 1, _toy_perm)
    assert not mc.differs(one, toy.update(3, 1, lambda k: np.arange(mc.Toy.E)), tol=1e-12)
    assert mc.differs(a, one)


@pytest.mark.parametrize('name', mc.WRONG)
def test_wrong_variant_is_told_apart(name):
    toy = mc.Toy()
    good = toy.update(3, 2, _toy_perm)
    assert mc.differs(good, toy.update(3, 2, _toy_perm, wrong=name)), name


# ------------------------------------------------------------------------------------------------------------------ host layers
@contextlib.contextmanager
def minibatch_ops():
    """spied_ops() with the three minibatch ops replaced by the restatement, recording."""
    from deeprl_network_amd import ops
    names = ('minibatch_perm', 'minibatch_gather', 'minibatch_count_advance')
    saved = {k: getattr(ops, k) for k in names}
    with spied_ops() as calls:
        calls['perm'], calls['gather'] = [], []

        def perm(seed, env_id_base, epoch, count, keys, out):
            calls['order'].append('perm')
            calls['perm'].append((seed, env_id_base, epoch, int(count)))
            out.copy_(torch.from_numpy(mc.perm(out.numel(), epoch, int(count), seed, env_id_base)))
            return out

        def gather(pairs, idx, outer_of=None):
            calls['order'].append('gather')
            calls['gather'].append(idx.tolist())
            pairs = list(pairs)
            E = None
            for (d, s), outer in zip(pairs, outer_of):
                e = s.numel() * len(idx) // d.numel()
                assert E in (None, e)
                E = e
                d.copy_(mc.gather_rows(s, idx.tolist(), outer, E).reshape(d.shape))

        def advance(count):
            calls['order'].append('count')
            count += 1

        ops.minibatch_perm, ops.minibatch_gather, ops.minibatch_count_advance = perm, gather, advance
        try:
            yield calls
        finally:
            for k, f in saved.items():
                setattr(ops, k, f)


@pytest.mark.parametrize('keys,match', [(dict(ppo_epochs='2', ppo_minibatches='0'), 'ppo_minibatches'),
                                        (dict(ppo_epochs='2', ppo_minibatches='-2'), 'ppo_minibatches'),
                                        (dict(ppo_epochs='2', ppo_minibatches='1.5'), 'ppo_minibatches'),
                                        (dict(ppo_epochs='2', ppo_minibatches='two'), 'ppo_minibatches'),
                                        (dict(ppo_epochs='2', ppo_minibatches='2'), 'does not divide'),        # E = 3
                                        (dict(ppo_epochs='2', ppo_minibatches='6'), 'does not divide'),        # M > E
                                        (dict(ppo_minibatches='3'), 'ppo_epochs = 1'),
                                        (dict(ppo_epochs='1', ppo_minibatches='3'), 'ppo_epochs = 1')])
def test_config_refusals_name_the_key(keys, match):
    with cpu_ops():
        with pytest.raises(ValueError, match=match):
            _build(trainer=False, **keys)


def test_one_replica_and_coupled_nets_are_refused():
    with cpu_ops():
        with pytest.raises(ValueError, match='ppo_minibatches'):
            _build(trainer=False, E=1, ppo_epochs='2', ppo_minibatches='2')
        with pytest.raises(ValueError, match='ppo_epochs'):
            _build('ma2c_nc', trainer=False, E=4, ppo_epochs='2', ppo_minibatches='2')


@pytest.mark.parametrize('M', [None, '1'])
def test_absent_or_one_allocates_nothing_and_runs_the_path_of_before(M):
    with minibatch_ops() as calls:
        _, model, tr = _build(E=4, ppo_epochs='2', ppo_minibatches=M)
        assert model.ppo_minibatches == 1 and model.ppo_steps() == [(2,)]
        for name in ('mb_perm', 'mb_count', '_mb', 'mb_env_id_base'):
            assert not hasattr(model, name), name
        tr.run_batch()
        assert calls['order'] == ['logp', 'apply', 'ppo_loss', 'apply']


def test_call_order_of_one_update_with_three_epochs_of_two_groups():
    """K = 3, M = 2 on E = 4 replicas: 1 + 2 * 2 optimiser steps; a permutation in front of every epoch's first gather, keyed by
    (epoch, updates made so far); the groups are the two halves of it; the count moves once, behind the last gather; the rotation
    is the last step's; ppo_stats holds the mean of an epoch's two steps."""
    with minibatch_ops() as calls:
        _, model, tr = _build(E=4, ppo_epochs='3', ppo_minibatches='2', ppo_target_kl='1e30')
        N, T = model.n_agent, model.n_step
        assert model.ppo_steps() == [(2, 0), (2, 1), (3, 0), (3, 1)]
        assert model.mb_perm.dtype == torch.int32 and int(model.mb_count) == 0 and tuple(model._mb['x'].shape)[:3] == (T, 2, N)
        assert tuple(model._mb['h'].shape) == (N, 2, model.n_lstm) and tuple(model._mb['logp'].shape) == (N, T * 2)
        tr.rollout()
        model.load_rewards(tr.buf_rraw)
        rotations = []
        inner_apply = model.update_apply
        model.update_apply = lambda lr, rotate=True, lr_dev=None: rotations.append(rotate) or inner_apply(lr, rotate=rotate, lr_dev=lr_dev)
        lr_n = model.lr_scheduler.n
        model.update(tr.R_end)
        tail = ['ppo_loss', 'kl_sum', 'kl_gate', 'apply']
        assert calls['order'] == ['logp', 'apply'] + ['perm', 'gather'] + tail + ['gather'] + tail + \
            ['perm', 'gather'] + tail + ['gather', 'count'] + tail, calls['order']
        assert rotations == [False] * 4 + [True]
        assert calls['perm'] == [(12, 0, 2, 0), (12, 0, 3, 0)] and int(model.mb_count) == 1
        p2, p3 = mc.perm(4, 2, 0, 12).tolist(), mc.perm(4, 3, 0, 12).tolist()
        assert calls['gather'] == [p2[:2], p2[2:], p3[:2], p3[2:]]
        assert model.ppo_steps_done == 5 and model.ppo_epochs_done == 3
        assert model.lr_scheduler.n == lr_n + T                       # the schedule moves once per update
        assert tuple(model.ppo_stats.shape) == (3, N, 2) and not model.ppo_stats[0].any()
        # the second update draws under count 1
        tr.rollout()
        model.load_rewards(tr.buf_rraw)
        model.update(tr.R_end)
        assert calls['perm'][2:] == [(12, 0, 2, 1), (12, 0, 3, 1)] and int(model.mb_count) == 2


def test_epoch_stats_are_the_mean_of_the_steps_in_step_order():
    with minibatch_ops() as calls:
        _, model, tr = _build(E=4, ppo_epochs='2', ppo_minibatches='2', ppo_vclip='0.5')
        from deeprl_network_amd import ops
        seen = []
        inner = ops.ppo_loss

        def loss(*a, **kw):
            tot, terms = inner(*a, **kw)
            seen.append(terms.detach().clone())
            return tot, terms
        ops.ppo_loss = loss
        try:
            tr.run_batch()
        finally:
            ops.ppo_loss = inner
        assert len(seen) == 2 and all(kw['v_old'] is model._mb['v_old'] for kw in calls['loss'])
        assert torch.equal(model.ppo_stats[1], (seen[0][:, 3:5] + seen[1][:, 3:5]) / 2)
        assert torch.equal(model.ppo_vclip_stats[1], (seen[0][:, 5] + seen[1][:, 5]) / 2)


def test_a_stop_inside_an_epoch_refuses_the_rest_of_the_update():
    """K = 3, M = 2, target 0.03; the steps report 0.01, 0.05, ..: step (2, 1) and everything behind it is refused."""
    with minibatch_ops() as calls:
        _, model, tr = _build(E=4, ppo_epochs='3', ppo_minibatches='2', ppo_target_kl='0.03')
        calls_script = [0.01, 0.05, 0.0, 0.0]
        from deeprl_network_amd import ops
        inner = ops.ppo_loss

        def loss(*a, **kw):
            tot, terms = inner(*a, **kw)
            terms = terms.clone()
            terms[:, 3] = calls_script.pop(0)
            return tot, terms
        ops.ppo_loss = loss
        try:
            tr.run_batch()
        finally:
            ops.ppo_loss = inner
        assert [c for c in calls['order'] if c in ('apply', 'refused')] == ['apply', 'apply', 'refused', 'refused', 'refused']
        assert model.ppo_steps_done == 2 and model.ppo_epochs_done == 1 and int(model.mb_count) == 1


def test_the_counter_travels_in_the_checkpoint_only_with_the_key_on(tmp_path, caplog):
    with minibatch_ops():
        _, model, tr = _build(E=4, ppo_epochs='2', ppo_minibatches='2')
        tr.run_batch()
        tr.run_batch()
        d = str(tmp_path) + '/'
        model.save(d, 7)
        blob = torch.load(d + 'checkpoint-7.pt', weights_only=True)
        assert int(blob['ppo_minibatch_count']) == 2
        _, fresh, _ = _build(E=4, ppo_epochs='2', ppo_minibatches='2')
        assert fresh.load(d) and int(fresh.mb_count) == 2
        _, plain, tr1 = _build(E=4, ppo_epochs='2')
        tr1.run_batch()
        plain.save(d, 9)
        assert 'ppo_minibatch_count' not in torch.load(d + 'checkpoint-9.pt', weights_only=True)
        fresh.mb_count.fill_(5)
        with caplog.at_level('WARNING'):
            assert fresh.load(d, checkpoint=9)
        assert int(fresh.mb_count) == 0 and 'ppo_minibatch_count' in caplog.text


def test_cli_flag_reaches_the_run_ini(tmp_path):
    from deeprl_network_amd.main import apply_overrides, parse_args
    a0 = parse_args(['train'])
    assert a0.ppo_minibatches is None
    args = parse_args(['train', '--ppo-epochs', '3', '--ppo-minibatches', '4'])
    assert args.ppo_minibatches == 4
    with pytest.raises(SystemExit):
        parse_args(['train', '--ppo-minibatches', '2.5'])
    cp = cacc_config(agent='ia2c_fp', n_step=5)
    run_ini = tmp_path / 'config.ini'
    with open(run_ini, 'w') as f:
        cp.write(f)
    before = open(run_ini, 'rb').read()
    assert not apply_overrides(cp, a0, str(run_ini)) and open(run_ini, 'rb').read() == before
    assert apply_overrides(cp, args, str(run_ini))
    back = configparser.ConfigParser()
    back.read(str(run_ini))
    assert back['MODEL_CONFIG'].getint('ppo_minibatches') == 4 and back['MODEL_CONFIG'].getint('ppo_epochs') == 3


def test_scalar_is_written_only_with_minibatches_and_a_target():
    from deeprl_network_amd.utils import SummaryWriter, _write_ppo_scalars
    with minibatch_ops():
        for keys, want in ((dict(ppo_minibatches='2', ppo_target_kl='10'), True), (dict(ppo_minibatches='2'), False),
                           (dict(ppo_target_kl='10'), False)):
            _, model, tr = _build(E=4, ppo_epochs='2', **keys)
            tr.run_batch()
            w = SummaryWriter()
            _write_ppo_scalars(w, model, 7)
            rows = ' '.join(str(r) for r in w._rows)
            assert ('train/%s_ppo_steps_done' % model.policy.summary_name in rows) == want


def test_descriptor_layout_matches_the_header():
    from deeprl_network_amd import _lib
    assert ctypes.sizeof(_lib.GatherDesc) == 32
    assert [(_lib.GatherDesc.src.offset, _lib.GatherDesc.dst.offset, _lib.GatherDesc.outer.offset, _lib.GatherDesc.inner_bytes.offset)] == \
        [(0, 8, 16, 24)]
    from deeprl_network_amd import ops
    assert ops.GATHER_MAX == 16 and ops.MINIBATCH_MAX_E == 65536 and ops.STREAM_MINIBATCH == mc.STREAM_MINIBATCH == 3


def test_new_kernels_use_no_scratch():
    """The permutation, count and gather kernels as compiled for gfx950: no scratch, no spills; the rank pass stages keys in LDS."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'tools'))
    import resource_usage
    rows = {r['name']: r for r in resource_usage.usage(os.path.join(root, 'deeprl_network_amd', 'csrc', 'minibatch.hip'))}
    for want in ('minibatch_keys_kernel', 'minibatch_rank_kernel', 'minibatch_count_advance_kernel', 'minibatch_gather_kernel'):
        assert any(want in n for n in rows), (want, sorted(rows))
    for n, g in rows.items():
        assert g['ScratchSize [bytes/lane]'] == 0 and g['VGPRs Spill'] == 0 and g['SGPRs Spill'] == 0, (n, g)
        print(n, {k: g[k] for k in g if 'GPR' in k or 'LDS' in k or 'Scratch' in k})
        if 'rank' in n:
            assert g['LDS Size [bytes/block]'] == 1024

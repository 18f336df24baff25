"""Training record without a GPU: the float64 restatement of the row (tests/train_record_ref.py) on hand-computed cases, the
tags and the aggregation of the writers (deeprl_network_amd/train_record.py) on a fabricated record, the binding, and the E = 1
reference path -- `model.backward(..., summary_writer, global_step)` emits the reference's six scalars (agents/policies.py:40-48,
265-273) -- on the CPU emulation of the HIP ops."""
import ctypes

import numpy as np
import pytest

from helpers import cacc_config
from train_record_ref import train_record_ref

SIX = ('loss/%s_entropy_loss', 'loss/%s_policy_loss', 'loss/%s_value_loss', 'loss/%s_total_loss', 'train/%s_lr', 'train/%s_gradnorm')


class WriterStub:
    def __init__(self):
        self.rows, self.flushed = [], 0

    def add_scalar(self, tag, value, global_step):
        self.rows.append((tag, float(value), int(global_step)))

    def flush(self):
        self.flushed += 1


# ------------------------------------------------------------------ the restatement on hand-computed cases
def test_ref_single_row():
    """rows = 1: every moment is the entry itself, both variances are 0 -> std 0 and explained_var 0 (var_R <= 0)."""
    r = train_record_ref([[0.5, 0.25, -0.125]], [3.0], 5e-4, 0.5, [[2.0]], [[0.5]], [[1]], [2])
    assert r.shape == (1, 24)
    np.testing.assert_array_equal(r[0, :4], [0.5, 0.25, -0.125, 0.625])
    assert r[0, 4] == np.float32(5e-4) and r[0, 5] == 3.0
    np.testing.assert_array_equal(r[0, 6:14], [2.0, 0.0, 1.5, 0.0, 0.5, 0.0, 0.25, 1.0])
    np.testing.assert_array_equal(r[0, 14:], [0, 0, 0.0, 1.0, 0, 0, 0, 0, 0, 0])


def test_ref_constant_return_and_zero_advantage():
    """Agent 0: constant R -> ret_std 0, explained_var 0 whatever the advantages are.  Agent 1: Adv == 0 (V == R) ->
    explained_var 1, value_mean == ret_mean.  R = (1, 3, 1, 3): mean 2, variance 1."""
    R = np.array([[2.0, 2.0, 2.0, 2.0], [1.0, 3.0, 1.0, 3.0]], dtype=np.float32)
    Adv = np.array([[1.0, -1.0, 1.0, -1.0], [0.0, 0.0, 0.0, 0.0]], dtype=np.float32)
    act = np.array([[0, 3], [1, 3], [1, 2], [1, 3]], dtype=np.uint8)
    r = train_record_ref(np.zeros((2, 3)), [7.0], 1e-3, 0.0, R, Adv, act, [2, 4])
    np.testing.assert_array_equal(r[0, 6:12], [2.0, 0.0, 2.0, 0.0, 0.0, 1.0])     # ret_mean, ret_std, value_mean, ev, adv_mean, adv_std
    np.testing.assert_array_equal(r[1, 6:12], [2.0, 1.0, 2.0, 1.0, 0.0, 0.0])
    np.testing.assert_array_equal(r[:, 5], [7.0, 7.0])                             # G = 1: broadcast
    np.testing.assert_array_equal(r[:, 12], [0.0, 0.0])                            # e_coef == 0 -> entropy 0
    np.testing.assert_array_equal(r[:, 13], [4.0, 4.0])
    np.testing.assert_array_equal(r[0, 16:], [0.25, 0.75, 0, 0, 0, 0, 0, 0])
    np.testing.assert_array_equal(r[1, 16:], [0, 0, 0.25, 0.75, 0, 0, 0, 0])


def test_ref_partial_explained_variance_entropy_and_ragged_actions():
    """R = (0, 2, 4, 6) (variance 5), Adv = (1, -1, 1, -1) (variance 1) -> explained_var 0.8; entropy = -c2 / e_coef; an agent
    with n_a = 2 < A gets no share beyond its own actions even if a stray byte is there; a per-agent grad_norm is read per agent."""
    R = np.array([[0.0, 2.0, 4.0, 6.0]] * 2, dtype=np.float32)
    Adv = np.array([[1.0, -1.0, 1.0, -1.0]] * 2, dtype=np.float32)
    act = np.array([[0, 0], [1, 1], [2, 2], [0, 3]], dtype=np.uint8)
    r = train_record_ref([[1.0, 2.0, -0.5], [0.0, 0.0, -0.25]], [1.5, 2.5], 1e-3, 0.25, R, Adv, act, [2, 4])
    np.testing.assert_allclose(r[:, 9], [0.8, 0.8], rtol=1e-15)
    np.testing.assert_allclose(r[:, 7], [np.sqrt(5.0)] * 2, rtol=1e-15)
    np.testing.assert_array_equal(r[:, 8], [3.0, 3.0])                             # mean of R - Adv = (-1, 3, 3, 7)
    np.testing.assert_array_equal(r[:, 12], [2.0, 1.0])
    np.testing.assert_array_equal(r[:, 5], [1.5, 2.5])
    np.testing.assert_array_equal(r[0, 16:], [0.5, 0.25, 0, 0, 0, 0, 0, 0])
    np.testing.assert_array_equal(r[1, 16:], [0.25, 0.25, 0.25, 0.25, 0, 0, 0, 0])


# ------------------------------------------------------------------ tags and aggregation
def _fabricated(n=3, N=4):
    rows = np.zeros((n, N, 24), dtype=np.float32)
    for u in range(n):
        for i in range(N):
            rows[u, i, :14] = [1 + i + 10 * u, 2 + i, -0.5 - i, 2.5 + i + 10 * u, 1e-3 * (u + 1), 5.0 + i, 0, 0, 0.5 * i, 0.25 * i, 0, 0,
                               1.0 + i, 60]
            rows[u, i, 16:20] = 0.25
    return rows


def test_per_agent_model_logs_agent_zero_under_lstm_0():
    from deeprl_network_amd import train_record as TR
    from deeprl_network_amd.agents import policies
    assert policies.LstmPolicy.summary_name == policies.FPPolicy.summary_name == 'lstm_0'
    rows, w = _fabricated(), WriterStub()
    TR.write_scalars(w, 'lstm_0', True, [60, 120, 180], rows)
    assert len(w.rows) == 3 * 9
    for u, step in enumerate((60, 120, 180)):
        got = {t: v for t, v, s in w.rows if s == step}
        assert list(got)[:6] == [t % 'lstm_0' for t in SIX]                       # the reference's order
        assert got['loss/lstm_0_policy_loss'] == 1 + 10 * u and got['loss/lstm_0_value_loss'] == 2
        assert got['loss/lstm_0_entropy_loss'] == -0.5 and got['loss/lstm_0_total_loss'] == 2.5 + 10 * u
        assert got['train/lstm_0_lr'] == pytest.approx(1e-3 * (u + 1)) and got['train/lstm_0_gradnorm'] == 5.0
        assert got['train/lstm_0_explained_var'] == pytest.approx(0.25 * 1.5) and got['train/lstm_0_entropy'] == 2.5
        assert got['train/lstm_0_value_mean'] == pytest.approx(0.75)


@pytest.mark.parametrize('cls,name', [('NCMultiAgentPolicy', 'nc'), ('IC3MultiAgentPolicy', 'ic3'), ('ConsensusPolicy', 'cu'),
                                      ('DIALMultiAgentPolicy', 'dial')])
def test_single_policy_model_sums_the_losses_over_agents(cls, name):
    from deeprl_network_amd import train_record as TR
    from deeprl_network_amd.agents import policies
    assert getattr(policies, cls).summary_name == name
    rows = _fabricated()
    got = dict(TR.scalars(name, False, rows[1]))
    assert got['loss/%s_policy_loss' % name] == sum(1 + i + 10 for i in range(4))
    assert got['loss/%s_value_loss' % name] == sum(2 + i for i in range(4))
    assert got['loss/%s_entropy_loss' % name] == sum(-0.5 - i for i in range(4))
    assert got['loss/%s_total_loss' % name] == sum(2.5 + i + 10 for i in range(4))
    assert got['train/%s_lr' % name] == pytest.approx(2e-3) and got['train/%s_gradnorm' % name] == 5.0      # row 0
    assert got['train/%s_entropy' % name] == 2.5
    assert [t for t, _ in TR.scalars(name, False, rows[1], extras=False)] == [t % name for t in SIX]


def test_csv_rows_and_columns():
    from deeprl_network_amd import train_record as TR
    rows = _fabricated(n=2, N=3)
    data = TR.csv_rows([20, 40], rows, 4)
    cols = ['step', 'agent_id', 'policy_loss', 'value_loss', 'entropy_loss', 'total_loss', 'lr', 'gradnorm', 'ret_mean', 'ret_std',
            'value_mean', 'explained_var', 'adv_mean', 'adv_std', 'entropy', 'share_0', 'share_1', 'share_2', 'share_3']
    assert TR.csv_columns(4) == cols and len(data) == 6 and all(list(d) == cols for d in data)
    assert [(d['step'], d['agent_id']) for d in data] == [(20, 0), (20, 1), (20, 2), (40, 0), (40, 1), (40, 2)]
    assert data[4]['policy_loss'] == 12.0 and data[4]['entropy'] == 2.0 and data[4]['share_3'] == 0.25


def test_binding_of_the_entry_points():
    from deeprl_network_amd import _lib
    assert ctypes.sizeof(_lib.TrainRecord) == 8 + 4 * 4 + 2 * 4 + 11 * 8 and _lib.TrainRecord.n_a.offset == 32
    assert _lib.lib.nmarl_train_record_ws_bytes(8, 60 * 4096) == 256 * 8 * 72          # 256 chunks x N x (5 f64 + 8 u32)
    assert _lib.lib.nmarl_train_record_ws_bytes(28, 4099) == 17 * 28 * 72
    assert _lib.lib.nmarl_train_record_ws_bytes(33, 10) < 0 and _lib.lib.nmarl_train_record_ws_bytes(8, 0) < 0
    assert _lib.lib.nmarl_train_record(None, None) == -1


def test_struct_layout_matches_the_c_compiler(tmp_path):
    """nmarl_train_record_t as gcc lays it out == its ctypes mirror, field by field (tests/test_abi.py does this for the others)."""
    import os
    import subprocess
    from deeprl_network_amd import _lib
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'nmarl.h')
    fields = [n for n, _ in _lib.TrainRecord._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu", sizeof(nmarl_train_record_t));\n' % header
    for f in fields:
        src += 'printf(" %%zu", offsetof(nmarl_train_record_t, %s));\n' % f
    src += 'return 0;}\n'
    (tmp_path / 'off.c').write_text(src)
    exe = str(tmp_path / 'off')
    subprocess.check_call(['gcc', str(tmp_path / 'off.c'), '-o', exe])
    nums = [int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert nums[0] == ctypes.sizeof(_lib.TrainRecord)
    assert nums[1:] == [getattr(_lib.TrainRecord, f).offset for f in fields]


def test_recorder_needs_a_device():
    from types import SimpleNamespace
    from deeprl_network_amd import _lib, train_record as TR
    with pytest.raises(_lib.NmarlError):
        TR.TrainRecorder(SimpleNamespace(device='cpu'))


# ------------------------------------------------------------------ the E = 1 reference path
@pytest.mark.parametrize('agent,name', [('ia2c_fp', 'lstm_0'), ('ma2c_nc', 'nc')])
def test_backward_with_a_writer_emits_the_six_reference_scalars(agent, name):
    """Trainer-style drive of the E = 1 model on the CPU emulation: explore one n_step batch, backward with a writer.  The six
    tags come out once, at the global step, with the reference's aggregation of the model's own last_loss / grad_norm / cur_lr;
    a backward without a writer writes nothing and moves the weights the same way."""
    import torch
    from cpu_emulation import cpu_ops
    from deeprl_network_amd.agents import models
    from deeprl_network_amd.utils import Counter, Trainer
    from oracle import trainer_ref
    cls = {'ia2c_fp': models.IA2C_FP, 'ma2c_nc': models.MA2C_NC}[agent]
    flats = []
    for with_writer in (True, False):
        cp = cacc_config(agent=agent, n_step=5, reward_norm=800.0, total_step=10 ** 6)
        env = trainer_ref.RefCaccEnv(cp['ENV_CONFIG'])
        w = WriterStub()
        with cpu_ops():
            model = cls(env.n_s_ls, env.n_a_ls, env.neighbor_mask, env.distance_mask, env.coop_gamma, 10 ** 6, cp['MODEL_CONFIG'],
                        seed=12, num_envs=1, device='cpu')
            tr = Trainer(env, model, Counter(10 ** 6, 10 ** 7, 10 ** 7), w if with_writer else None)
            ob = env.reset()
            model.reset()
            ob, done, R = tr.explore(ob, True)
            model.backward(R, 0, w if with_writer else None, 5)
            terms = model.loss_terms()
        flats.append(model.policy.params.flat.clone())
        if not with_writer:
            assert w.rows == []
            continue
        assert [t for t, _, _ in w.rows] == [t % name for t in SIX] and all(s == 5 for _, _, s in w.rows)
        got = {t: v for t, v, _ in w.rows}
        pl, vl, el, _ = (x.detach().numpy().astype(np.float64) for x in model.last_loss)
        assert terms.shape == (8, 3) and terms.is_contiguous()
        np.testing.assert_array_equal(terms.detach().numpy(), np.stack([pl, vl, el], axis=1).astype(np.float32))
        agg = (lambda x: x[0]) if agent == 'ia2c_fp' else (lambda x: x.sum())
        assert got['loss/%s_policy_loss' % name] == pytest.approx(agg(pl), rel=1e-6)
        assert got['loss/%s_value_loss' % name] == pytest.approx(agg(vl), rel=1e-6)
        assert got['loss/%s_entropy_loss' % name] == pytest.approx(agg(el), rel=1e-6)
        assert got['loss/%s_total_loss' % name] == pytest.approx(agg(pl + vl + el), rel=1e-6)
        assert got['train/%s_lr' % name] == pytest.approx(model.cur_lr, rel=1e-6) and model.cur_lr == 5e-4
        assert got['train/%s_gradnorm' % name] == pytest.approx(float(model.grad_norm[0]), rel=1e-6) and got['train/%s_gradnorm' % name] > 0
        assert all(np.isfinite(v) for v in got.values())
    assert torch.equal(flats[0], flats[1])

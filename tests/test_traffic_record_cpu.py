"""The traffic record of an ATSC evaluation without a GPU: the claims its definition rests on (both synthetic models conserve
vehicles, so what is missing from the network has left it), the queue statistics against NumPy's on the reference's detector view,
and the host-built static tables (deeprl_network_amd/envs/traffic_record.py) against the oracles."""
import types

import numpy as np
import pytest

from helpers import grid_config, net_config
from traffic_record_ref import TrafficRecordRef

E, STEPS = 3, 150          # 750 s from an episode's start; `test_both_demand_waves_are_reached` moves the clock to 600 s


def _grid():
    from deeprl_network_amd.envs import traffic_record as TR
    from oracle import grid_ref as G
    p = G.GridParams(config=grid_config()['ENV_CONFIG'])
    return G, p, TR.grid_mult(), TR.grid_demand(p.peak1, p.peak2)


def _net():
    from deeprl_network_amd.envs import traffic_record as TR
    from oracle import realnet_ref as R
    p = R.NetParams(config=net_config()['ENV_CONFIG'])
    return R, p, TR.net_mult(R.TOPO.n_s_ls, R.TOPO.L), TR.net_demand(p.flow_rate)


def _drive(scenario, t0=0):
    """Seeded random actions through the float64 oracle and the restatement.  -> per step (rows, arrived before the clamp, q),
    the restatement.  t0: the oracle's clock at the start (the record does not care where an episode's clock stands)."""
    rng = np.random.RandomState(7)
    if scenario == 'grid':
        G, p, mult, demand = _grid()
        ref = G.GridBatchRef(p, E=E, dtype=np.float64)
        n_a = [5] * 25
    else:
        R, p, mult, demand = _net()
        ref = R.NetBatchRef(p, E=E, dtype=np.float64)
        n_a = R.TOPO.n_a_ls
    ref.reset(0.8 + 0.4 * rng.rand(E, 4))
    ref.t = ref.t + t0
    rec = TrafficRecordRef(mult, demand, E)
    rec.begin()
    out = []
    for _ in range(STEPS):
        a = np.stack([rng.randint(0, n, size=E) for n in n_a], axis=1)
        ref.step(a)
        rows = rec.step(ref.q, ref.tr, ref.t, ref.xi)
        out.append((rows, rec.arrived_raw.copy(), ref.q.copy()))
    return out, rec


@pytest.fixture(scope='module', params=['grid', 'net'])
def run(request):
    return (request.param,) + _drive(request.param)


@pytest.fixture(scope='module')
def grid_run():
    return _drive('grid')


def test_vehicles_are_conserved(run):
    """arrived >= 0 BEFORE the clamp, at every step: the models create no vehicle, so the clamp only removes rounding."""
    _, out, _ = run
    worst = min(raw.min() for _, raw, _ in out)
    assert worst >= -1e-9, 'the model created %.3e vehicles in one step' % -worst
    assert max(rows[:, 2].max() for rows, _, _ in out) > 0.1           # and vehicles do leave


def test_departed_minus_arrived_is_what_is_in_the_network(run):
    _, out, rec = run
    total = out[-1][0][:, 0]
    assert (total > 10).all()
    np.testing.assert_allclose(rec.cum[:, 0] - rec.cum[:, 1], total, rtol=1e-9, atol=0)
    np.testing.assert_allclose(sum(rows[:, 1] for rows, _, _ in out), rec.cum[:, 0], rtol=1e-12)


def test_both_demand_waves_are_reached():
    """150 steps from an episode's start end at 750 s, and the second wave of either scenario (flow groups 2, 3) starts at 900 s:
    the same drive with the clock started at 600 s covers the change of piece and the second wave's onset."""
    for scenario, (_, p, mult, demand) in (('grid', _grid()), ('net', _net())):
        out, rec = _drive(scenario, t0=120)                            # 600 s .. 1350 s: pieces 2..4
        assert min(raw.min() for _, raw, _ in out) >= -1e-9, scenario
        dep = np.array([rows[:, 1] for rows, _, _ in out])
        assert (dep > 0).all()
        # before 900 s only groups 0, 1 feed the network, afterwards all four: every replica's departures jump
        assert (dep[60:].min(axis=0) > dep[:60].max(axis=0)).all(), scenario
        np.testing.assert_allclose(rec.cum[:, 0] - rec.cum[:, 1], out[-1][0][:, 0], rtol=1e-9, atol=0)


def test_grid_queue_statistics_are_numpys_over_the_link_view(grid_run):
    out, _ = grid_run
    from oracle.grid_ref import LINK_LANE
    for rows, _, q in out[::7]:
        view = q[:, :, LINK_LANE].reshape(E, -1)                       # the reference's `queues` list: one entry per ilds_in
        np.testing.assert_allclose(rows[:, 6], view.mean(axis=1), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(rows[:, 5], view.std(axis=1), rtol=1e-10, atol=1e-12)
    assert out[-1][0][:, 5].min() > 0


def test_row_relations(run):
    """Speeds within [0, V_FREE], the mean wait bounded by half the time recorded so far, time_sec = 5 t, the trip row's order."""
    _, out, rec = run
    for k, (rows, _, _) in enumerate(out):
        assert (rows[:, 0] >= 0).all() and (rows[:, 4] >= 0).all() and (rows[:, 4] <= 13.89 + 1e-12).all()
        assert (rows[:, 3] >= 0).all() and (rows[:, 3] <= 5.0 * (k + 1) / 2).all()
        assert (rows[:, 7] == 5.0 * (k + 1)).all()
    trip = rec.trip(STEPS)
    assert (trip['duration_sec'] >= trip['wait_sec']).all() and (trip['wait_sec'] >= 0).all()
    np.testing.assert_allclose(trip['wait_step'] * 5.0, trip['wait_sec'], rtol=1e-15)
    assert (trip['arrival_sec'] == 5.0 * STEPS).all()


def test_demand_tables():
    G, p, _, demand = _grid()
    for g in range(4):
        for piece in range(12):
            for sec in (piece * 300, piece * 300 + 299):
                assert demand[g, piece] == 3 * G.demand_rate(g, sec, p.peak1, p.peak2), (g, piece)
    R, p, _, demand = _net()
    for g in range(4):
        for piece in range(12):
            for sec in (piece * 300, piece * 300 + 299):
                assert demand[g, piece] == p.flow_rate * R.activity(g, sec), (g, piece)
    assert demand.dtype == np.float64 and demand.shape == (4, 12) and demand[:, 11].max() == 0


def test_mult_tables():
    G, _, mult, _ = _grid()
    assert mult.shape == (25, 6) and mult.dtype == np.int32
    want = np.bincount(G.LINK_LANE, minlength=6)
    assert (mult == want[None]).all() and tuple(want) == (3, 2, 1, 3, 2, 1) and mult.sum() == 25 * 12
    R, _, mult, _ = _net()
    tp = R.TOPO
    assert mult.shape == (tp.N, tp.L) and mult.dtype == np.int32
    assert mult.sum() == sum(tp.n_s_ls) and set(np.unique(mult)) == {0, 1}
    for i, n in enumerate(tp.n_s_ls):
        assert (mult[i, :n] == 1).all() and (mult[i, n:] == 0).all()


def test_invalid_slots_never_contribute():
    R, p, mult, demand = _net()
    rng = np.random.RandomState(1)
    q = rng.uniform(0, 9, size=(2,) + mult.shape) * (mult > 0)
    tr = rng.uniform(0, 2, size=q.shape) * (mult > 0)
    a, b = TrafficRecordRef(mult, demand, 2), TrafficRecordRef(mult, demand, 2)
    dirty = np.where(mult > 0, q, 1e6)
    np.testing.assert_array_equal(a.step(q, tr, [3, 3], np.ones((2, 4))), b.step(dirty, np.where(mult > 0, tr, 1e6), [3, 3], np.ones((2, 4))))
    assert (b.stand[:, mult == 0] == 0).all()


def test_recorder_refuses_other_envs_and_the_cpu():
    from deeprl_network_amd import _lib
    from deeprl_network_amd.envs.traffic_record import TrafficRecorder
    with pytest.raises(_lib.NmarlError):
        TrafficRecorder(types.SimpleNamespace(device='cpu', E=1), 4)             # neither ATSC env (a CACC env lands here too)
    from deeprl_network_amd.envs.large_grid_env import LargeGridBatchEnv
    fake = LargeGridBatchEnv.__new__(LargeGridBatchEnv)                            # a grid env that somehow sits on the CPU
    fake.device, fake.E, fake.n_agent = 'cpu', 1, 25
    fake.params = types.SimpleNamespace(peak1=1100.0, peak2=925.0)
    with pytest.raises(_lib.NmarlError, match='HIP device'):
        TrafficRecorder(fake, 4)

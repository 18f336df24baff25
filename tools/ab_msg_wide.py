"""Same-box A/B of lstm_comm's in-kernel message term at four neighbour slots (NeurComm on the 5 x 5 ATSC grid), and the check that
the two-slot path did not move.
    python tools/ab_msg_wide.py grid [RUNS=3] [BATCHES=6]
        config_ma2c_cnet_grid.ini with agent = ma2c_nc (= the reference's config_ma2c_nc_grid.ini) at 25 x 1024 replicas, one process,
        arms alternating: A = ops.msg_supported held to the 128-float bound (gather + fc launches: the previous commit's path, whose
        code this commit does not touch), B = this tree (the message term inside lstm_step_x_kernel<1,1> / <2,1>).  Per run: ms per
        batch, ms per rollout graph alone, kernel nodes of the rollout graph (tools/graph_nodes.py).
    NMARL_INKERNEL_HANDOFF=0 [NMARL_LIB_AB=tools/dbg/libnmarl_prev.so] python tools/ab_msg_wide.py line
        config_ma2c_nc_catchup.ini (m_max = 2) at 8 x 1024 on the launch-per-step forms <1,1> / <2,1>: 3 batches, a hash of the weights,
        then ms per batch over 5 more.  Run once per library (tools/ab_build.sh <parent> builds the other one), alternating."""
import configparser
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import graph_nodes as GN  # noqa: E402
from deeprl_network_amd import _lib, ops  # noqa: E402
from deeprl_network_amd.envs import make_batch_env  # noqa: E402
from deeprl_network_amd.main import init_agent  # noqa: E402
from deeprl_network_amd.utils import BatchedTrainer, Counter  # noqa: E402

E = 1024
ORIG = ops.msg_supported


def narrow(kind, m_max, n_h):
    return ORIG(kind, m_max, n_h) and (n_h if kind == ops.MSG_MEAN_ADD else n_h * m_max) <= 128


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def trainer(ini, agent=None, **kw):
    cp = configparser.ConfigParser()
    cp.read(os.path.join(ROOT, 'config', ini))
    if agent:
        cp['ENV_CONFIG']['agent'] = agent
    env = make_batch_env(cp['ENV_CONFIG'], num_envs=E)
    np.random.seed(12)
    model = init_agent(env, cp['MODEL_CONFIG'], 10 ** 9, 12, num_envs=E)
    return env, model, BatchedTrainer(env, model, Counter(10 ** 12, 10 ** 12, 10 ** 12), use_graph=True, **kw)


def grid_run(arm, batches):
    ops.msg_supported = narrow if arm == 'A' else ORIG
    env, model, tr = trainer('config_ma2c_cnet_grid.ini', 'ma2c_nc', keep_graphs=True)
    for _ in range(3):
        tr.run_batch()
    assert (model.policy._msg() is not None) == (arm == 'B') and not model.policy.pv_one_launch(E)
    ms = timed(tr.run_batch, batches)
    tr.flush()
    snap = tr._snapshot()
    roll = timed(tr.graph.replay, 5)
    tr._restore(snap)
    T = model.n_step
    k_roll = GN.census(tr.graph)['kernel']
    print('arm %s  batch %.3f ms  rollout graph alone %.3f ms  rollout kernel nodes %d = %.2f per lock-step (%d lock-steps)' %
          (arm, ms, roll, k_roll, k_roll / (T + 1), T + 1), flush=True)
    del tr, model, env
    torch.cuda.empty_cache()


def line_run():
    env, model, tr = trainer('config_ma2c_nc_catchup.ini')
    assert not model.policy.pv_one_launch(E), 'run with NMARL_INKERNEL_HANDOFF=0: the launch-per-step forms'
    for _ in range(3):
        tr.run_batch()
    tr.flush()
    torch.cuda.synchronize()
    assert model.policy._msg() is not None
    w = model.policy.params.flat.detach().cpu().numpy()
    print('lib %s  weights after 3 batches sha256 %s  finite %s' %
          (os.path.relpath(_lib.LIB_PATH, ROOT), hashlib.sha256(w.tobytes()).hexdigest()[:16], bool(np.isfinite(w).all())), flush=True)
    print('    batch %.3f ms' % timed(tr.run_batch, 5), flush=True)


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else 'grid'
    if what == 'grid':
        runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
        batches = int(sys.argv[3]) if len(sys.argv) > 3 else 6
        print('ma2c_nc on the 5 x 5 grid, 25 x %d replicas, n_step 120, %s' % (E, torch.cuda.get_device_name(0)), flush=True)
        for _ in range(runs):
            for arm in ('A', 'B'):
                grid_run(arm, batches)
    else:
        line_run()

"""Generate tests/golden/platoon_*.npz: the REAL reference environment (envs/cacc_env.py of the reference checkout,
imported unmodified) with platoons of other lengths than 8 -- `n_vehicle` is an ordinary ENV_CONFIG key (cacc_env.py:320-343).

    python tests/golden/make_golden_platoon.py [--out DIR]

Same keys as the cacc_*.npz fixtures of make_golden_env.py (whose ini text and action tapes are reused) plus `n_vehicle`;
every run stops at the first `done`.  The 32-vehicle case stores its observations as float32 (`obs32`): in float64 the file
would exceed the size limit of a committed fixture; its state, rewards and done flags stay float64.  The files are NOT named
cacc_*: the tests of the 8-vehicle kernels glob that prefix.
"""
import configparser
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_env import INI, REF, tape  # noqa: E402

OUT = HERE

# name, n_vehicle, scenario, agent, seed, tape, coop_gamma, train_mode[, obs32]
CASES = [
    ('n2_catchup_cyclic', 2, 'catchup', 'ma2c_nc', 41, 'cyclic', -1, True),
    ('n3_catchup_ia2c_mild', 3, 'catchup', 'ia2c', 42, 'mild', -1, True),
    ('n5_slowdown_fp_random', 5, 'slowdown', 'ia2c_fp', 43, 'random', -1, True),
    ('n12_catchup_mild', 12, 'catchup', 'ma2c_nc', 44, 'mild', -1, True),
    ('n12_catchup_const1', 12, 'catchup', 'ma2c_nc', 48, 'const1', -1, True),
    ('n16_slowdown_spatial_mild', 16, 'slowdown', 'ma2c_nc', 45, 'mild', 0.9, True),
    ('n25_catchup_test_const3', 25, 'catchup', 'ma2c_nc', 46, 'const3', -1, False),
    ('n32_slowdown_const3', 32, 'slowdown', 'ma2c_nc', 47, 'const3', -1, True, True),
]


def run_case(name, n_vehicle, scenario, agent, seed, kind, coop_gamma=-1, train_mode=True, obs32=False):
    sys.path.insert(0, REF)
    from envs.cacc_env import CACCEnv  # the reference, unmodified
    ini = INI.format(agent=agent, scenario=scenario, seed=seed, coop_gamma=coop_gamma)
    assert 'n_vehicle = 8\n' in ini
    cp = configparser.ConfigParser()
    cp.read_file(io.StringIO(ini.replace('n_vehicle = 8\n', 'n_vehicle = %d\n' % n_vehicle)))
    env = CACCEnv(cp['ENV_CONFIG'])
    env.train_mode = train_mode
    rng = np.random.RandomState(1234 + seed)
    T, N = env.T, env.n_agent
    assert N == n_vehicle
    acts = tape(kind, T, N, rng)
    used_seed = env.seed if train_mode else env.seed - 1      # cacc_env.py:169-176 (test_ind < 0)
    np.random.seed(used_seed)
    U = np.random.rand()
    ob = env.reset()
    fps = rng.dirichlet(np.ones(4), size=(T + 1, N))          # synthetic fingerprints for ia2c_fp
    if agent == 'ia2c_fp':
        env.update_fingerprint(fps[0])
        ob = env._get_state()
    n_s = [len(o) for o in ob]
    obs = np.zeros((T + 1, N, max(n_s)))
    for i, o in enumerate(ob):
        obs[0, i, :len(o)] = o
    hs, vs, us = [env.hs_cur.copy()], [env.vs_cur.copy()], [env.us_cur.copy()]
    rew, grew, dones = [], [], []
    v0s = env.v0s.copy()
    steps = 0
    for t in range(T):
        if agent == 'ia2c_fp':
            env.update_fingerprint(fps[t + 1])
        ob, r, d, g = env.step(acts[t])
        steps += 1
        for i, o in enumerate(ob):
            obs[t + 1, i, :len(o)] = o
        hs.append(np.array(env.hs_cur, dtype=np.float64))
        vs.append(np.array(env.vs_cur, dtype=np.float64))
        us.append(np.array(env.us_cur, dtype=np.float64))
        rew.append(np.broadcast_to(np.asarray(r, dtype=np.float64), (N,)).copy())
        grew.append(g)
        dones.append(d)
        if d:
            break
    out = dict(U=U, used_seed=used_seed, acts=acts[:steps], h=np.array(hs), v=np.array(vs), u=np.array(us),
               reward=np.array(rew), global_reward=np.array(grew), done=np.array(dones),
               obs=obs[:steps + 1].astype(np.float32 if obs32 else np.float64), n_s=np.array(n_s), v0s=v0s, fps=fps[:steps + 1],
               scenario=scenario, agent=agent, seed=seed, train_mode=train_mode,
               coop_gamma=coop_gamma, neighbor_mask=env.neighbor_mask, distance_mask=env.distance_mask,
               n_vehicle=n_vehicle)
    np.savez_compressed(os.path.join(OUT, 'platoon_%s.npz' % name), **out)
    print('%-28s N=%2d steps=%3d collided=%s sum_g=%.10f' % (name, N, steps, env.collision, float(np.sum(grew))))


if __name__ == '__main__':
    if '--out' in sys.argv:
        OUT = sys.argv[sys.argv.index('--out') + 1]
    for case in CASES:
        run_case(*case)

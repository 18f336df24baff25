"""Fixture networks of the `net_file` tests and their independent restatement.  TEST HELPER, not a test.

SMALL (5 nodes): link counts {6, 5, 3, 2, 1}, phase counts 2 and 3, m_max = 2; n4 lists no neighbour; n2 is listed (by n0) but feeds
no link (fan 0); permitted `g` in n0, n1, n2; every `links` list differs from the rule; external links in all four groups; a
non-integer activity table that is non-zero in piece 11.  LIMITS (32 nodes): x01 has 24 links and 8 phases, x00 lists 4 neighbours,
no `links` (the rule applies), Monaco's activity.  UNIFORM (3 nodes): every node has 2 phases, over 4 / 6 / 2 links, m_max = 2 -- equal action
counts over unequal observation widths.

`Topo(obj)` computes every static array from the description on its own (nothing of deeprl_network_amd is imported): it is the
`topo` of oracle.realnet_ref.NetBatchRef and of tests/realnet_wait_ref.NetWaitRef.  `with_activity(cls)` restates the arrival term
for a general table: oracle.realnet_ref.activity is Monaco's."""
import configparser
import json
import os

import numpy as np

from oracle import realnet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MONACO_ACTIVITY = [[1, 2, 4, 4, 4, 4, 2, 1, 0, 0, 0, 0]] * 2 + [[0, 0, 0, 1, 2, 4, 4, 4, 4, 2, 1, 0]] * 2

SMALL = {
    'nodes': {
        'n0': {'phases': ['GGgrrr', 'rrrGGg', 'GrGrGr'], 'neighbors': ['n1', 'n2'], 'links': ['n1', 'n1', 'n1', 0, 1, 'n1']},
        'n1': {'phases': ['GGgrr', 'rrrGG'], 'neighbors': ['n3', 'n0'], 'links': ['n0', 'n3', 'n3', 2, 'n0']},
        'n2': {'phases': ['Grr', 'gGG'], 'neighbors': ['n0'], 'links': ['n0', 'n0', 3]},
        'n3': {'phases': ['Gr', 'rG', 'GG'], 'neighbors': ['n1', 'n4'], 'links': ['n4', 'n1']},
        'n4': {'phases': ['G', 'r'], 'neighbors': [], 'links': [2]},
    },
    'activity': [[0.5, 1.25, 2.5, 3.75, 4, 4, 2.5, 1.25, 0.5, 0.25, 0.125, 0.75],
                 [1.5, 1.5, 1.5, 1.5, 1.5, 1.5, 1.5, 1.5, 1.5, 1.5, 1.5, 1.5],
                 [0, 0.3, 0.6, 1.2, 2.4, 3.3, 3.3, 2.4, 1.2, 0.6, 0.3, 0.1],
                 [2.2, 0, 2.2, 0, 2.2, 0, 2.2, 0, 2.2, 0, 2.2, 1.1]],
}


UNIFORM = {
    'nodes': {
        'u0': {'phases': ['GGrr', 'rrGG'], 'neighbors': ['u1']},
        'u1': {'phases': ['GGgrrr', 'rrrGGg'], 'neighbors': ['u0', 'u2']},
        'u2': {'phases': ['Gr', 'rG'], 'neighbors': ['u1'], 'links': ['u1', 0]},
    },
}


def _limits():
    nodes = {}
    for i in range(32):
        n_s, n_a = (24, 8) if i == 1 else (2 + i % 5, 2 + i % 3)
        phases = [''.join('G' if (k + a) % 3 == 0 else 'g' if (k + 2 * a) % 7 == 3 else 'r' for k in range(n_s)) for a in range(n_a)]
        nbrs = ['x01', 'x02', 'x03', 'x31'] if i == 0 else ['x%02d' % ((i + 1) % 32)] + (['x%02d' % (i - 1)] if i % 4 == 2 else [])
        nodes['x%02d' % i] = {'phases': phases, 'neighbors': nbrs}
    return {'nodes': nodes}


LIMITS = _limits()


class Topo:
    """The static arrays of a description, computed here from the JSON object alone."""

    def __init__(self, obj):
        nodes = obj['nodes']
        self.names = sorted(nodes)
        N = self.N = len(self.names)
        idx = {n: i for i, n in enumerate(self.names)}
        self.phases = [list(nodes[n]['phases']) for n in self.names]
        self.n_a_ls = [len(p) for p in self.phases]
        self.n_s_ls = [len(p[0]) for p in self.phases]
        self.A, self.L = max(self.n_a_ls), max(self.n_s_ls)
        self.nbrs_listed = [[idx[m] for m in nodes[n]['neighbors']] for n in self.names]
        self.nbrs = [sorted(js) for js in self.nbrs_listed]
        self.m_max = max(len(js) for js in self.nbrs)
        self.neighbor_mask = np.zeros((N, N), dtype=int)
        for i, js in enumerate(self.nbrs_listed):
            for j in js:
                self.neighbor_mask[i, j] = 1
        # shortest directed path lengths over the listed neighbours by repeated relaxation (Bellman-Ford on unit edges)
        INF = 10 ** 6
        dist = np.full((N, N), INF, dtype=int)
        np.fill_diagonal(dist, 0)
        for _ in range(N):
            for u in range(N):
                for v in self.nbrs_listed[u]:
                    dist[:, v] = np.minimum(dist[:, v], dist[:, u] + 1)
        self.distance_mask = np.where(dist >= INF, -1, dist)
        self.green = np.zeros((N, self.A, self.L), dtype=np.int32)
        self.src = -np.ones((N, self.L), dtype=np.int32)
        self.group = -np.ones((N, self.L), dtype=np.int32)
        for i, n in enumerate(self.names):
            for a, s in enumerate(self.phases[i]):
                for k, ch in enumerate(s):
                    self.green[i, a, k] = 'rGg'.index(ch)
            links = nodes[n].get('links')
            for k in range(self.n_s_ls[i]):
                if links is None:
                    m = len(self.nbrs[i])
                    if k % (m + 1) < m:
                        self.src[i, k] = self.nbrs[i][k % (m + 1)]
                    else:
                        self.group[i, k] = (i + k) % 4
                elif isinstance(links[k], str):
                    self.src[i, k] = idx[links[k]]
                else:
                    self.group[i, k] = links[k]
        self.fan = np.array([(self.src == j).sum() for j in range(N)], dtype=np.int32)
        n_ext = [int((self.group == g).sum()) for g in range(4)]
        self.ext_share = np.zeros((N, self.L))
        for i in range(N):
            for k in range(self.L):
                if self.group[i, k] >= 0:
                    self.ext_share[i, k] = 1.0 / n_ext[self.group[i, k]]
        self.dn = [[(i, k) for i in range(N) for k in range(self.n_s_ls[i]) if self.src[i, k] == j] for j in range(N)]
        self.activity = np.array(obj.get('activity', MONACO_ACTIVITY), dtype=np.float64)


def with_activity(cls):
    """cls (NetBatchRef or a subclass) -> the same model whose arrival term reads the topology's own [4,12] activity table:
    a_g = activity[g][sec // 300] below piece 12, else 0 -- oracle.realnet_ref.activity(group, sec) is Monaco's table."""
    class WithActivity(cls):
        def _activity(self, group, sec):
            piece = int(sec) // 300
            return float(self.tp.activity[group, piece]) if piece < 12 else 0.0

        def step(self, action):
            monaco, R.activity = R.activity, self._activity
            try:
                return super().step(action)
            finally:
                R.activity = monaco
    WithActivity.__name__ = cls.__name__ + 'WithActivity'
    return WithActivity


def write(directory, obj, name='net.json'):
    path = os.path.join(str(directory), name)
    with open(path, 'w') as f:
        json.dump(obj, f)
    return path


def config(net_path, agent='ma2c_nc', coop_gamma=0.9, seed=12, n_step=120, objective='queue', coef_wait=0.0, **env_keys):
    """config_ma2c_nc_net.ini with `net_file` (an absolute path; None = the built-in network) and the given keys."""
    cp = configparser.ConfigParser()
    cp.read(os.path.join(ROOT, 'config', 'config_ma2c_nc_net.ini'))
    e = cp['ENV_CONFIG']
    e['agent'], e['coop_gamma'], e['seed'] = agent, str(coop_gamma), str(seed)
    e['objective'], e['coef_wait'] = objective, str(coef_wait)
    if net_path is not None:
        e['net_file'] = str(net_path)
    for k, v in env_keys.items():
        e[k] = str(v)
    cp['MODEL_CONFIG']['batch_size'] = str(n_step)
    return cp


def rand_actions(rng, E, tp):
    return np.stack([rng.randint(0, tp.n_a_ls[i], size=E) for i in range(tp.N)], axis=1)


class CpuFileNetBatchEnv:
    """TEST-ONLY stand-in for RealNetBatchEnv with a `net_file` on CPU tensors (tests/cpu_emulation.py CpuRealNetBatchEnv on
    the description `obj` instead of the oracle's Monaco): the restatement above steps it, the host attributes are computed here."""

    def __new__(cls, obj, config, num_envs=1):
        import torch
        from cpu_emulation import CpuRealNetBatchEnv

        class Env(CpuRealNetBatchEnv):
            def __init__(self):
                tp = self.topo = Topo(obj)
                self.config, self.E, self.device = config, num_envs, torch.device('cpu')
                self.p = R.NetParams(config=config)
                self.ref = with_activity(R.NetBatchRef)(self.p, E=num_envs, dtype=np.float32, topo=tp)
                self.name, self.agent, self.coop_gamma, self.T = config.get('scenario'), self.p.agent, self.p.coop_gamma, self.p.T
                self.seed, self.env_id_base = self.p.seed, 0
                self.n_agent, self.n_a, self.n_a_ls = tp.N, tp.A, list(tp.n_a_ls)
                self.n_feat, self.n_feat_ls = tp.L, list(tp.n_s_ls)
                self.neighbor_mask, self.distance_mask = tp.neighbor_mask, tp.distance_mask
                self.n_s_ls = list(tp.n_s_ls) if self.agent.startswith('ma2c') else \
                    [tp.n_s_ls[i] + sum(tp.n_s_ls[j] for j in tp.nbrs[i]) for i in range(tp.N)]
                self.batch_size, self.train_mode = None, True
                self.episode = torch.zeros(num_envs, dtype=torch.int32)
                self.obs = torch.zeros(num_envs, tp.N, tp.L * (1 + tp.m_max))
                self.done = torch.zeros(num_envs, dtype=torch.uint8)
                self.reward = torch.zeros((num_envs, tp.N) if self.coop_gamma >= 0 else (num_envs,))
                self.global_reward = torch.zeros(num_envs)

            def _emit(self):
                self.obs.copy_(torch.from_numpy(R.gather_net(self.ref.obs(), self.topo)))
                return self.obs
        return Env()

"""Synthetic (SUMO-free) Monaco-like ATSC network on MI355X -- host mirror of the reference's
envs/real_net_env.py + envs/atsc_env.py for the `atsc_real_net` scenario: 28 HETEROGENEOUS agents (2..6 phases over
2..22 signal links, 0..4 listed neighbours).

The reference drives an external SUMO process on a net file that is not in its repository; this path keeps the
reference's *contract* -- node set, directed neighbour lists, phase sets (real_net_env.py:21-69), node order and
neighbour / BFS distance masks (152-195), 5 s control / 2 s yellow, 720-step episodes, `wave` observation, queue
reward with per-agent spatial discount (or the `wait` / `hybrid` objectives of atsc_env.py:383-418 over one more state
array, head_wait: csrc/realnet.hip header), the flow_rate demand schedule (real_net_data/build_file.py:70-96), the rule-based
`greedy` agent (real_net_env.py:112-145) -- and replaces the microsimulation by the store-and-forward link-graph model specified in oracle/realnet_ref.py, stepped
by csrc/realnet.hip for E lock-stepped replicas.  Observations come out already padded to the widest node and
gathered over the listed neighbours: the input layout of the heterogeneous (identical=False) nets.

The network is a description (envs/net_file.py): the built-in Monaco one made from NODE_DEFS / PHASE_SETS below, or the file that
ENV_CONFIG `net_file` names (2..32 nodes), which also carries the demand's activity table (nmarl_net_step_dem).
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from .atsc import N_GROUP, OBJECTIVES, RULE_AGENTS, AtscBatchEnv, AtscEnv, RuleController, atsc_params_from_config  # noqa: F401
from . import net_file
from .traffic_record import net_mult

# (node, phase-set key, listed neighbours): real_net_env.py:21-49
NODE_DEFS = (
    ('10026', '6.0', ('9431', '9561', 'cluster_9563_9597', '9531')),
    ('8794', '4.0', ('cluster_8985_9609', '9837', '9058', 'cluster_9563_9597')),
    ('8940', '2.1', ('9007', '9429')),
    ('8996', '2.2', ()),
    ('9007', '2.3', ('9309', '8940')),
    ('9058', '4.0', ('cluster_8985_9609', '8794', 'joinedS_0')),
    ('9153', '2.0', ('9643',)),
    ('9309', '4.0', ('9466', '9007', 'cluster_9043_9052')),
    ('9413', '2.3', ('9721', '9837')),
    ('9429', '5.0', ('cluster_9043_9052', '8940')),
    ('9431', '2.4', ('9721', '9884', '9561', '10026')),
    ('9433', '2.5', ()),
    ('9466', '4.0', ('9309', 'joinedS_0')),
    ('9480', '2.3', ()),
    ('9531', '2.6', ('joinedS_1',)),
    ('9561', '4.0', ('cluster_9389_9689', '10026')),
    ('9643', '2.3', ('9153',)),
    ('9713', '3.0', ('9721',)),
    ('9721', '6.0', ('9431', '9713', '9413')),
    ('9837', '3.1', ('9413', '8794', 'cluster_8985_9609')),
    ('9884', '2.7', ('9713', 'cluster_9389_9689')),
    ('cluster_8751_9630', '4.0', ()),
    ('cluster_8985_9609', '4.0', ('9837', '8794', '9058')),
    ('cluster_9043_9052', '4.1', ('cluster_9563_9597', '10026', 'joinedS_1')),
    ('cluster_9389_9689', '4.0', ('cluster_8751_9630', '9884', '9561', '8996')),
    ('cluster_9563_9597', '4.2', ('10026', '8794', 'joinedS_0', 'cluster_9043_9052')),
    ('joinedS_0', '6.1', ('9058', 'cluster_9563_9597', '9466')),
    ('joinedS_1', '3.2', ('9531', '9429')),
)
# phase sets over the node's signal links: real_net_env.py:51-69
PHASE_SETS = {
    '2.0': ('GGrrr', 'ggGGG'), '2.1': ('GGGrrr', 'rrGGGg'), '2.2': ('Grr', 'gGG'), '2.3': ('GGGgrr', 'GrrrGG'),
    '2.4': ('GGGGrr', 'rrrrGG'), '2.5': ('Gg', 'rG'), '2.6': ('GGGg', 'rrrG'), '2.7': ('GGg', 'rrG'),
    '3.0': ('GGgrrrGGg', 'rrGrrrrrG', 'rrrGGGGrr'), '3.1': ('GgrrGG', 'rGrrrr', 'rrGGGr'),
    '3.2': ('GGGGrrrGG', 'rrrrGGGGr', 'GGGGrrGGr'),
    '4.0': ('GGgrrrGGgrrr', 'rrrGGgrrrGGg', 'rrGrrrrrGrrr', 'rrrrrGrrrrrG'),
    '4.1': ('GGgrrGGGrrr', 'rrGrrrrrrrr', 'rrrGgrrrGGg', 'rrrrGrrrrrG'),
    '4.2': ('GGGGrrrrrrrr', 'GGggrrGGggrr', 'rrrGGGGrrrrr', 'grrGGggrrGGg'),
    '5.0': ('GGGGgrrrrGGGggrrrr', 'grrrGrrrrgrrGGrrrr', 'GGGGGrrrrrrrrrrrrr', 'rrrrrrrrrGGGGGrrrr', 'rrrrrGGggrrrrrggGg'),
    '6.0': ('GGGgrrrGGGgrrr', 'rrrGrrrrrrGrrr', 'GGGGrrrrrrrrrr', 'rrrrrrrrrrGGGG', 'rrrrGGgrrrrGGg', 'rrrrrrGrrrrrrG'),
    '6.1': ('GGgrrGGGrrrGGGgrrrGGGg', 'rrGrrrrrrrrrrrGrrrrrrG', 'GGGrrrrrGGgrrrrGGgrrrr', 'GGGrrrrrrrGrrrrrrGrrrr',
            'rrrGGGrrrrrrrrrrrrGGGG', 'rrrGGGrrrrrGGGgrrrGGGg'),
}


def builtin_description():
    """The built-in Monaco network (NODE_DEFS / PHASE_SETS, links by the rule, Monaco's activity) as a checked description."""
    return net_file.parse({'nodes': {name: {'phases': list(PHASE_SETS[key]), 'neighbors': list(nbrs)} for name, key, nbrs in NODE_DEFS}})


def _phases_of(node_names, phases):
    """Per node of `node_names` its phase strings: `phases` (a topology's, in that order), or -- None -- the built-in network's by
    name; a name the built-in network does not have is refused (a file-described network hands over its own phases)."""
    if phases is not None:
        if len(phases) != len(node_names):
            raise ValueError('phases: one entry per node (%d nodes, %d entries)' % (len(node_names), len(phases)))
        return [tuple(p) for p in phases]
    key = {name: k for name, k, _ in NODE_DEFS}
    unknown = [name for name in node_names if name not in key]
    if unknown:
        raise ValueError('node %r is not a node of the built-in network: pass the phases of the network (NetTopology.phases)' % unknown[0])
    return [PHASE_SETS[key[name]] for name in node_names]


class RealNetController(RuleController):
    """The reference's rule-based `greedy` agent (real_net_env.py:112-145): per node the phase whose green links hold the most
    vehicles.  A link counts for a phase where its signal is the capital 'G' (the reference tests `signal == 'G'`: a permitted
    'g' does not count); the reference adds every incoming lane once per phase, and in the synthetic network every link is its
    own lane, so nothing is de-duplicated.  `ob` is the node's own wave vector, one entry per link.  `phases`: the nodes' phase
    strings in the order of `node_names` (NetTopology.phases); None = the built-in network's.  Same `forward(obs) -> actions`
    duck-type as LargeGridController."""
    name = 'greedy'

    def __init__(self, node_names, phases=None):
        self.node_names = list(node_names)
        self._phases = dict(zip(self.node_names, _phases_of(self.node_names, phases)))

    def greedy(self, ob, node_name):
        flows = [sum(ob[k] for k, signal in enumerate(phase) if signal == 'G') for phase in self._phases[node_name]]
        return int(np.argmax(np.array(flows)))               # the first maximum

    def forward(self, obs):
        return [self.greedy(ob, node_name) for ob, node_name in zip(obs, self.node_names)]


def net_greedy_table(node_names, phases=None):
    """(n_a [N] i32, mask [N,8] u32) of nmarl_atsc_greedy for the network's nodes in the given order: bit k of mask[i][a] is set
    where link k of node i shows the capital 'G' in phase a -- the links RealNetController.greedy adds.  `phases` as there."""
    n_a = np.zeros(len(node_names), dtype=np.int32)
    mask = np.zeros((len(node_names), 8), dtype=np.uint32)
    for i, node_phases in enumerate(_phases_of(node_names, phases)):
        n_a[i] = len(node_phases)
        for a, phase in enumerate(node_phases):
            mask[i, a] = sum(1 << k for k, signal in enumerate(phase) if signal == 'G')
    return n_a, mask


class NetTopology:
    """Static arrays of the network (host NumPy + device copies + the nmarl_net_topo_t handed to the kernels)."""

    def __init__(self, device, desc=None):
        """desc: a net_file.NetDescription (a parsed `net_file`); None = the built-in Monaco network."""
        self.builtin = desc is None
        desc = self.desc = builtin_description() if desc is None else desc
        self.node_names = list(desc.names)                               # sorted: real_net_env.py:189
        N = self.N = len(self.node_names)
        self.phases = [tuple(p) for p in desc.phases]
        self.activity = np.array(desc.activity, dtype=np.float64)        # [4,12]: x flow_rate = veh/h of a flow group in a piece
        self.n_a_ls = [len(p) for p in self.phases]
        self.n_s_ls = [len(p[0]) for p in self.phases]                   # one `wave` entry per signal link
        self.A, self.L = max(self.n_a_ls), max(self.n_s_ls)
        listed = [list(js) for js in desc.listed]
        self.neighbor_mask = np.zeros((N, N), dtype=int)                 # real_net_env.py:175-181 (directed)
        for i, js in enumerate(listed):
            self.neighbor_mask[i, js] = 1
        self.distance_mask = -np.ones((N, N), dtype=int)                 # BFS, -1 = unreachable (152-187)
        for i in range(N):
            self.distance_mask[i, i] = 0
            frontier, d = [i], 0
            while frontier:
                d += 1
                nxt = []
                for u in frontier:
                    for v in listed[u]:
                        if self.distance_mask[i, v] < 0:
                            self.distance_mask[i, v] = d
                            nxt.append(v)
                frontier = nxt
        self.nbrs = [sorted(js) for js in listed]
        self.m_max = max(len(js) for js in self.nbrs)
        code = {'r': 0, 'G': 1, 'g': 2}
        green = np.zeros((N, self.A, self.L), dtype=np.uint8)
        for i, p in enumerate(self.phases):
            for a, s in enumerate(p):
                green[i, a, :len(s)] = [code[ch] for ch in s]
        src = -np.ones((N, self.L), dtype=np.int32)                      # the description's feeders and flow groups (net_file.parse:
        group = -np.ones((N, self.L), dtype=np.int32)                    # the file's `links`, or the rule of oracle/realnet_ref.py)
        for i in range(N):
            src[i, :self.n_s_ls[i]] = desc.feeder[i]
            group[i, :self.n_s_ls[i]] = desc.group[i]
        fan = np.array([(src == j).sum() for j in range(N)], dtype=np.int32)
        n_ext = np.array([(group == g).sum() for g in range(N_GROUP)])   # a group without an entry has no share: nothing is divided by 0
        ext_share = np.where(group >= 0, 1.0 / np.maximum(n_ext, 1)[np.maximum(group, 0)], 0.0).astype(np.float32)
        dn_ptr, dn_pair = [0], []
        for j in range(N):
            for i in range(N):
                for k in range(self.n_s_ls[i]):
                    if src[i, k] == j:
                        dn_pair.append((i << 8) | k)
            dn_ptr.append(len(dn_pair))
        nbr_idx = -np.ones((N, self.m_max), dtype=np.int32)
        for i, js in enumerate(self.nbrs):
            nbr_idx[i, :len(js)] = js
        self.host = dict(n_s=np.array(self.n_s_ls, dtype=np.int32), green=green, src=src, fan=fan, group=group,
                         ext_share=ext_share, dn_ptr=np.array(dn_ptr, dtype=np.int32),
                         dn_pair=np.array(dn_pair if dn_pair else [0], dtype=np.int32), nbr_idx=nbr_idx)
        # the packed image the step kernel copies into LDS (include/nmarl.h NMARL_NET_OFF_*: rows padded to 24 links)
        NM, LM, AM = 32, 24, 8
        if N > NM or self.L > LM or self.A > AM or self.m_max > 8:
            raise _lib.NmarlError('network exceeds the kernel limits (32 nodes, 24 links, 8 phases, 8 neighbours)')
        img = np.zeros(_lib.NET_IMAGE_BYTES, dtype=np.uint8)
        off = _lib.NET_OFF

        def put(name, arr):
            b = np.ascontiguousarray(arr).view(np.uint8).ravel()
            img[off[name]:off[name] + b.size] = b
        g = np.zeros((NM, AM, LM), dtype=np.uint8)
        g[:N, :self.A, :self.L] = green
        put('green', g)
        a16 = -np.ones((NM, LM), dtype=np.int16)
        a16[:N, :self.L] = src
        put('src', a16)
        a8 = -np.ones((NM, LM), dtype=np.int8)
        a8[:N, :self.L] = group
        put('group', a8)
        f = np.zeros((NM, LM), dtype=np.float32)
        f[:N, :self.L] = ext_share
        put('share', f)
        ff = np.zeros(NM, dtype=np.float32)
        ff[:N] = fan
        put('fan', ff)
        put('dnptr', np.array(dn_ptr + [dn_ptr[-1]] * (NM + 1 - len(dn_ptr)), dtype=np.int16))
        pairs = np.zeros(NM * LM, dtype=np.int16)
        pairs[:len(dn_pair)] = [(v >> 8) * LM + (v & 255) for v in dn_pair]
        put('dnpair', pairs)
        nb8 = -np.ones((NM, 8), dtype=np.int8)
        nb8[:N, :self.m_max] = nbr_idx
        put('nbr', nb8)
        self.host['image'] = img
        self.dev = {'n_s': torch.from_numpy(self.host['n_s']).to(device), 'image': torch.from_numpy(img).to(device),
                    'nbr_idx': torch.from_numpy(nbr_idx).to(device)}
        t = self.c = _lib.NetTopo()
        t.N, t.L, t.A, t.m_max = N, self.L, self.A, self.m_max
        t.n_s, t.image = self.dev['n_s'].data_ptr(), self.dev['image'].data_ptr()
        # a file-described network hands its activity table to the step kernel (nmarl_net_step_dem); the built-in one keeps the
        # kernel's own arithmetic (nmarl_net_step)
        self.dem = None if self.builtin else _lib.NetDemand()
        if self.dem is not None:
            for g in range(N_GROUP):
                for piece in range(net_file.N_PIECE):
                    self.dem.act[g][piece] = self.activity[g, piece]


def net_topology_from_config(config, device):
    """ENV_CONFIG section -> NetTopology: the network of the file `net_file` names (an absolute path, or one relative to the working
    directory: `net_file.read_ini` has resolved the ini's own against the ini's directory), or the built-in one."""
    path = config.get('net_file', fallback=None)
    return NetTopology(device, net_file.load(path) if path else None)


def net_params_from_config(config):
    """ENV_CONFIG section -> nmarl_net_params_t; keys of atsc_env.py:79-99 + real_net_env.py:147."""
    p = atsc_params_from_config(config, _lib.NetParams(), 'network', config.get('objective'), ValueError)
    p.flow_rate = config.getfloat('flow_rate')
    return p


class RealNetBatchEnv(AtscBatchEnv):
    def _scenario(self, config):
        self.params = net_params_from_config(config)
        tp = self.topo = net_topology_from_config(config, self.device)
        self.n_agent, self.n_a, self.n_a_ls = tp.N, tp.A, list(tp.n_a_ls)
        self.n_feat, self.n_feat_ls = tp.L, list(tp.n_s_ls)               # own observation widths (heterogeneous)
        self.neighbor_mask, self.distance_mask = tp.neighbor_mask, tp.distance_mask
        if self.agent.startswith('ma2c') or self.agent in RULE_AGENTS:   # (greedy: atsc_env.py:256-257)
            self.n_s_ls = list(tp.n_s_ls)
        else:                                                            # own + listed neighbours' (atsc_env.py:263-269)
            self.n_s_ls = [tp.n_s_ls[i] + sum(tp.n_s_ls[j] for j in tp.nbrs[i]) for i in range(tp.N)]
        return tp.L, tp.L * (1 + tp.m_max)

    def traffic_model(self):
        """(mult [N,L] i32, demand [4,12] f64) of the traffic record (envs/traffic_record.py)."""
        return net_mult(self.topo.n_s_ls, self.topo.L), float(self.params.flow_rate) * self.topo.activity

    def greedy_rule(self):
        """(host controller, own observation width, n_a, mask) of the batched greedy agent (envs/greedy.py)."""
        names, phases = self.topo.node_names, self.topo.phases
        return (RealNetController(names, phases), int(self.topo.L)) + net_greedy_table(names, phases)

    def pressure_table(self):
        from .maxpressure import net_pressure_table
        return net_pressure_table(self.topo)

    def _reset_call(self, params, args):
        topo = ctypes.byref(self.topo.c)
        if self.head_wait is None:
            _lib.check(_lib.lib.nmarl_net_reset(topo, *args), 'nmarl_net_reset')
        else:                                                            # the same reset, which also clears head_wait
            _lib.check(_lib.lib.nmarl_net_reset_obj(ctypes.byref(params), topo, *args), 'nmarl_net_reset_obj')

    def _step_call(self, args):
        p, topo = ctypes.byref(self.params), ctypes.byref(self.topo.c)
        if self.topo.dem is None:
            _lib.check(_lib.lib.nmarl_net_step(p, topo, *args), 'nmarl_net_step')
        else:                                                            # the same step with the demand's activity table as data
            _lib.check(_lib.lib.nmarl_net_step_dem(p, topo, *args, ctypes.byref(self.topo.dem)), 'nmarl_net_step_dem')


class RealNetEnv(AtscEnv):
    """Reference duck-type (atsc_env.py:77-524 / real_net_env.py:145-198) for ONE replica: ragged observation lists
    (`ma2c*` / `greedy` / `maxpressure`: the node's own links; `ia2c*`: own + listed neighbours' in ascending node index, + their fingerprints
    for ia2c_fp), ragged fingerprints, per-agent rewards."""
    batch_class = RealNetBatchEnv

    def __init__(self, config, port=0, device='cuda', **_):
        super().__init__(config, port, device)
        self.n_feat_ls = self.batch.n_feat_ls
        self.node_names = self.batch.topo.node_names
        self._nbr = self.batch.topo.nbrs

    def _state_list(self):
        L = self.batch.n_feat
        x = self.batch.obs[0].cpu().numpy().astype(np.float64)          # [N, L*(1+m_max)], slots L wide
        out = []
        for i in range(self.n_agent):
            cur = [x[i, :self.n_feat_ls[i]]]
            if self.agent.startswith('ia2c'):
                cur += [x[i, (k + 1) * L:(k + 1) * L + self.n_feat_ls[j]] for k, j in enumerate(self._nbr[i])]
            if self.agent == 'ia2c_fp':
                cur += [np.asarray(self.fp[j]) for j in self._nbr[i]]
            out.append(np.concatenate(cur))
        return out

"""The description of a signalised network for `scenario = atsc_real_net` (ENV_CONFIG `net_file`): a JSON file

    {"nodes": {"a": {"phases": ["GGgrr", "rrrGG"], "neighbors": ["b", "c"], "links": ["b", 0, "c", "b", 2]}, ...},
     "activity": [[...12...], [...12...], [...12...], [...12...]]}

`phases`: 2..8 strings over r / G / g of one length, the node's number of signal links (1..24).  `neighbors`: the node's LISTED
neighbours (directed, as real_net_env.py:21-49 lists them): at most 4, no repeats, not the node itself.  `links` (optional), one
entry per signal link: a string names the listed neighbour that feeds the link, an integer 0..3 makes it an external entry of that
flow group; absent = the rule of oracle/realnet_ref.py (neighbour number k mod (m+1) in ascending node index, external where that
equals m, group (i + k) mod 4).  `activity` (optional): 4 flow groups x 12 pieces of 300 s, the factor of `flow_rate` veh/h the
group carries in the piece; absent = Monaco's profile (real_net_data/build_file.py:70-72).  Node order is the sorted names.

`parse` checks a description against the limits of the kernels (csrc/realnet.hip NMAX, LMAX, AMAX; 4 listed neighbours: the
policy kernels) and resolves it: every link gets its feeder or its flow group.  Pure Python + NumPy: no device is touched."""
import collections
import json
import math

import numpy as np

N_GROUP, N_PIECE = 4, 12
N_MAX, L_MAX, A_MAX, M_MAX = 32, 24, 8, 4
F32_MAX = float(np.finfo(np.float32).max)
# number of active flows per 5-minute piece, groups 0, 1 and 2, 3 (real_net_data/build_file.py:70-72): the host's one copy of
# Monaco's profile (traffic_record.net_demand reads it; csrc/realnet.hip activity_a / activity_b evaluate it)
MONACO_ACTIVITY = ((1, 2, 4, 4, 4, 4, 2, 1, 0, 0, 0, 0),) * 2 + ((0, 0, 0, 1, 2, 4, 4, 4, 4, 2, 1, 0),) * 2

NetDescription = collections.namedtuple('NetDescription', 'names phases listed feeder group activity')
NetDescription.__doc__ = """A checked, resolved network: names (sorted), and per node in that order phases (tuple of strings), listed (the
listed neighbours' indices, in the file's order), feeder (per link the feeding node's index or -1), group (per link the flow group of
an external entry or -1); activity [4,12] f64."""


def _fail(where, what):
    raise ValueError('net_file: %s: %s' % (where, what))


def _activity(raw):
    if raw is None:
        return np.array(MONACO_ACTIVITY, dtype=np.float64)
    ok = isinstance(raw, (list, tuple)) and len(raw) == N_GROUP and \
        all(isinstance(row, (list, tuple)) and len(row) == N_PIECE for row in raw)
    if not ok:
        _fail('activity', 'must be %d groups x %d pieces of 300 s' % (N_GROUP, N_PIECE))
    for g, row in enumerate(raw):
        for p, v in enumerate(row):
            # (finite as the float32 the kernel reads, too: 1e39 is a finite float64 and an infinite float32)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0 or v > F32_MAX:
                _fail('activity', 'entry [%d][%d] = %r is not a finite (float32) number >= 0' % (g, p, v))
    return np.array(raw, dtype=np.float64)


def parse(obj):
    """The parsed JSON object (or an equal dict) -> NetDescription; a ValueError names the offending node or field."""
    if not isinstance(obj, dict) or not isinstance(obj.get('nodes'), dict):
        _fail('nodes', 'the file must be an object with a "nodes" object')
    unknown = set(obj) - {'nodes', 'activity'}
    if unknown:
        _fail('field %r' % sorted(unknown)[0], 'unknown top-level field')
    nodes = obj['nodes']
    if not 2 <= len(nodes) <= N_MAX:
        _fail('nodes', '%d nodes, the kernels take 2..%d' % (len(nodes), N_MAX))
    names = sorted(nodes)
    pos = {name: i for i, name in enumerate(names)}
    phases, listed = [], []
    for name in names:
        nd, at = nodes[name], 'node %r' % name
        if not isinstance(nd, dict):
            _fail(at, 'must be an object')
        unknown = set(nd) - {'phases', 'neighbors', 'links'}
        if unknown:
            _fail(at, 'unknown field %r' % sorted(unknown)[0])
        ph = nd.get('phases')
        if not isinstance(ph, (list, tuple)) or not all(isinstance(s, str) for s in ph):
            _fail(at + ' phases', 'must be a list of strings')
        if not 2 <= len(ph) <= A_MAX:
            _fail(at + ' phases', '%d phases, a node has 2..%d' % (len(ph), A_MAX))
        if len({len(s) for s in ph}) != 1:
            _fail(at + ' phases', 'phase strings of unequal length')
        if any(ch not in 'rGg' for s in ph for ch in s):
            _fail(at + ' phases', 'a phase string holds a character other than r, G, g')
        if not 1 <= len(ph[0]) <= L_MAX:
            _fail(at + ' phases', '%d signal links, a node has 1..%d' % (len(ph[0]), L_MAX))
        nb = nd.get('neighbors', [])
        if not isinstance(nb, (list, tuple)) or not all(isinstance(s, str) for s in nb):
            _fail(at + ' neighbors', 'must be a list of node names')
        if len(nb) > M_MAX:
            _fail(at + ' neighbors', '%d neighbours, a node lists at most %d' % (len(nb), M_MAX))
        for m in nb:
            if m not in pos:
                _fail(at + ' neighbors', 'unknown neighbour %r' % m)
            if m == name:
                _fail(at + ' neighbors', 'a node cannot list itself')
        if len(set(nb)) != len(nb):
            _fail(at + ' neighbors', 'repeated neighbour')
        phases.append(tuple(ph))
        listed.append([pos[m] for m in nb])
    if max(len(js) for js in listed) < 1:
        _fail('nodes', 'no node lists a neighbour (the kernels need m_max >= 1)')
    feeder, group = [], []
    for i, name in enumerate(names):
        at, n_s, asc = 'node %r links' % name, len(phases[i][0]), sorted(listed[i])
        links = nodes[name].get('links')
        if links is None:                                    # the rule of oracle/realnet_ref.py
            m = len(asc)
            fd = [asc[k % (m + 1)] if k % (m + 1) < m else -1 for k in range(n_s)]
            gr = [(i + k) % N_GROUP if fd[k] < 0 else -1 for k in range(n_s)]
        else:
            if not isinstance(links, (list, tuple)) or len(links) != n_s:
                _fail(at, 'must list one entry per signal link (%d)' % n_s)
            fd, gr = [], []
            for k, v in enumerate(links):
                if isinstance(v, str):
                    if v not in pos or pos[v] not in listed[i]:
                        _fail(at, 'link %d: feeder %r is not one of the node\'s listed neighbours' % (k, v))
                    fd.append(pos[v])
                    gr.append(-1)
                elif isinstance(v, int) and not isinstance(v, bool):
                    if not 0 <= v < N_GROUP:
                        _fail(at, 'link %d: flow group %d outside 0..%d' % (k, v, N_GROUP - 1))
                    fd.append(-1)
                    gr.append(v)
                else:
                    _fail(at, 'link %d: %r is neither a neighbour\'s name nor a flow group 0..%d' % (k, v, N_GROUP - 1))
        feeder.append(fd)
        group.append(gr)
    activity = _activity(obj.get('activity'))
    for g in range(N_GROUP):
        if activity[g].max() > 0 and not any(g in gr for gr in group):
            _fail('activity', 'flow group %d has positive activity and no external link' % g)
    return NetDescription(names, phases, listed, feeder, group, activity)


def load(path):
    """The file at `path` -> NetDescription."""
    with open(path) as f:
        try:
            obj = json.load(f)
        except ValueError as e:
            raise ValueError('net_file: %s is not JSON: %s' % (path, e))
    return parse(obj)


def check_scenario(env_config):
    """`net_file` belongs to the signalised network alone: any other scenario that carries the key is refused."""
    if env_config.get('net_file', fallback=None) and env_config.get('scenario') != 'atsc_real_net':
        _fail('ENV_CONFIG net_file', 'valid only with scenario = atsc_real_net, not %r' % env_config.get('scenario'))


def read_ini(path):
    """The ini at `path` -> ConfigParser whose ENV_CONFIG net_file, where relative, is resolved against the ini's directory."""
    import configparser
    import os
    config = configparser.ConfigParser()
    config.read(path)
    if config.has_section('ENV_CONFIG'):
        check_scenario(config['ENV_CONFIG'])
        name = config['ENV_CONFIG'].get('net_file', fallback=None)
        if name and not os.path.isabs(name):
            config.set('ENV_CONFIG', 'net_file', os.path.join(os.path.dirname(os.path.abspath(path)), name))
    return config


def copy_into_run(config, data_dir, run_ini):
    """What `main.py train` does with a `net_file`: the file is copied into the run's data directory and the run's ini
    `run_ini` is rewritten to name that copy (by its bare name: relative to the ini beside it, so the run directory can move).
    `config` -- as `read_ini` returned it -- keeps the resolved path.  -> whether there was a file."""
    import os
    import shutil
    path = config.get('ENV_CONFIG', 'net_file', fallback=None) if config.has_section('ENV_CONFIG') else None
    if not path:
        return False
    shutil.copy(path, os.path.join(data_dir, os.path.basename(path)))
    config.set('ENV_CONFIG', 'net_file', os.path.basename(path))
    with open(run_ini, 'w') as f:
        config.write(f)
    config.set('ENV_CONFIG', 'net_file', path)
    return True


def explicit(desc):
    """NetDescription -> the JSON object that describes it with `links` and `activity` written out."""
    nodes = {}
    for i, name in enumerate(desc.names):
        links = [desc.names[f] if f >= 0 else int(g) for f, g in zip(desc.feeder[i], desc.group[i])]
        nodes[name] = {'phases': list(desc.phases[i]), 'neighbors': [desc.names[j] for j in desc.listed[i]], 'links': links}
    act = [[int(v) if float(v).is_integer() else float(v) for v in row] for row in desc.activity.tolist()]
    return {'nodes': nodes, 'activity': act}

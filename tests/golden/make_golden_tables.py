"""Generate tests/golden/reference_tables.json: the reference's static tables that the oracle / product are pinned to,
read from a reference checkout, so that the pinning tests run without one.

    python tests/golden/make_golden_tables.py --ref <reference checkout> [--out DIR]

Stores
  configs     every config/*.ini of the reference, section -> key -> raw string (configparser, no interpolation);
  large_grid  the LargeGridPhase phase list (envs/large_grid_env.py), the two demand ratio vectors and the external
              origin edges of the four flow groups (envs/large_grid_data/build_file.py, get_external_od run unmodified);
  real_net    NODES / PHASES (envs/real_net_env.py) as sorted node names, phase strings and listed neighbour indices,
              and the neighbour / distance masks RealNetEnv builds from them (its map builders run without SUMO).
"""
import argparse
import ast
import configparser
import glob
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))


def literal_assign(path, name, cls=None):
    """The literal value assigned to `name` (inside class `cls` if given); np.array([...]) -> the list."""
    tree = ast.parse(open(path).read())
    scope = tree
    if cls is not None:
        scope = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == cls)
    for n in ast.walk(scope):
        if isinstance(n, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in n.targets):
            v = n.value
            if isinstance(v, ast.Call):
                v = v.args[0]
            return ast.literal_eval(v)
    raise KeyError('%s not assigned in %s' % (name, path))


def configs(ref):
    out = {}
    for f in sorted(glob.glob(os.path.join(ref, 'config', '*.ini'))):
        cp = configparser.ConfigParser()
        cp.read(f)
        out[os.path.basename(f)] = {s: dict(cp.items(s, raw=True)) for s in cp.sections()}
    return out


def large_grid(ref):
    env = os.path.join(ref, 'envs', 'large_grid_env.py')
    bf = os.path.join(ref, 'envs', 'large_grid_data', 'build_file.py')
    sys.path.insert(0, os.path.dirname(bf))
    try:
        import build_file
        srcs = [build_file.get_external_od(x, dest=False) for x in ([12, 13, 14], [16, 18, 20], [2, 3, 4], [6, 8, 10])]
    finally:
        sys.path.remove(os.path.dirname(bf))
    return {'phases': literal_assign(env, 'phases', cls='LargeGridPhase'),
            'ratios1': literal_assign(bf, 'ratios1'), 'ratios2': literal_assign(bf, 'ratios2'),
            'external_origins': srcs}


def real_net(ref):
    saved = dict(sys.modules)
    try:
        for m in ('seaborn', 'matplotlib', 'matplotlib.pyplot', 'traci', 'traci.exceptions', 'sumolib'):
            sys.modules[m] = types.ModuleType(m)
        sys.modules['seaborn'].set_color_codes = lambda *a, **k: None
        sys.modules['sumolib'].checkBinary = lambda x: x
        sys.modules['traci'].exceptions = types.SimpleNamespace(FatalTraCIError=Exception)
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), 'oracle', 'tf1_shim'))
        sys.path.insert(0, ref)
        from envs.real_net_env import NODES, PHASES, RealNetEnv
        names = sorted(NODES)
        env = RealNetEnv.__new__(RealNetEnv)                     # no SUMO: run only the pure map builders
        env.node_names, env.n_node = names, len(names)
        env._init_neighbor_map()
        env._init_distance_map()
        return {'names': names, 'phases': [list(PHASES[NODES[n][0]]) for n in names],
                'nbrs_listed': [[names.index(x) for x in NODES[n][1]] for n in names],
                'neighbor_mask': env.neighbor_mask.astype(int).tolist(), 'distance_mask': env.distance_mask.astype(int).tolist()}
    finally:
        sys.path[:] = [p for p in sys.path if p != ref and not p.endswith('tf1_shim')]
        for k in [k for k in sys.modules if k not in saved]:
            del sys.modules[k]
        sys.modules.update(saved)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='the reference checkout')
    ap.add_argument('--out', default=HERE)
    a = ap.parse_args()
    ref = os.path.abspath(a.ref)
    tables = {'configs': configs(ref), 'large_grid': large_grid(ref), 'real_net': real_net(ref)}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'reference_tables.json'), 'w') as f:
        json.dump(tables, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()

"""Bit-for-bit record of small trainers, for comparing two checkouts of this repository (a host-code refactor against its parent).

    python tools/state_hashes.py out.json             run the 28 cases in this checkout -> out.json
    python tools/state_hashes.py --compare a.json b.json

28 cases = 7 nets x {saved activations, recompute} x {eager, captured}: trainers as tests/test_gpu_trainer.build makes them (n_step 10,
E = 64 on the CACC line, 32 on the 5 x 5 grid), three batches each.  Per case: a hash of the bytes of the rollout buffers, the recurrent
state, the weights, the optimiser slots, the env's state tensors and -- with saved activations -- of everything the rollout saved
(S, gates, state sequences, every `_extra_full` entry, the sign image); the trainer's (enc_in_kernel, env_in_kernel, fused_encode,
handoff_fallbacks); the node census (tools/graph_nodes.census) of the rollout graph and of the update graphs.  Run each checkout in a
fresh process of its own; --compare prints one line per case and exits 1 if any differs."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = [('ia2c', 'catchup'), ('ia2c_fp', 'catchup'), ('ma2c_cu', 'catchup'), ('ma2c_dial', 'catchup'), ('ma2c_ic3', 'grid'),
        ('ma2c_nc', 'catchup'), ('ma2c_nc', 'grid')]
N_STEP, BATCHES = 10, 3


def _hash(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def run_case(agent, scenario, saved, captured):
    import torch
    from test_gpu_trainer import build
    import graph_nodes
    kw = dict(keep_graphs=True) if captured else {}
    if not saved:
        kw['save_activations'] = False
    env, model, tr = build(agent, 32 if scenario == 'grid' else 64, captured, scenario=scenario, n_step=N_STEP, **kw)
    for _ in range(BATCHES):
        tr.run_batch()
    torch.cuda.synchronize()
    p = model.policy
    tensors = {'buf_act': model.buf_act, 'buf_v': model.buf_v, 'buf_fp': model.buf_fp, 'h_fw': model.h_fw, 'c_fw': model.c_fw,
               'R_end': tr.R_end, 'weights': p.params.flat, 'rmsprop': p.params.ms}
    tensors.update({'env[%d]' % k: t for k, t in enumerate(env.state_tensors())})
    if model.save_acts:
        tensors.update(buf_vn=model.buf_vn, S_ext=model.S_ext, G_buf=model.G_buf, H_all=model.H_all, C_all=model.C_all)
        tensors.update({'extra.' + k: v for k, v in p._extra_full.items()})
        if model.S_bits is not None:
            tensors['S_bits'] = model.S_bits
    assert bool(model.save_acts) == saved, 'the trainer did not take the %s form' % ('saved' if saved else 'recompute')
    out = {'tensors': {k: _hash(v) for k, v in sorted(tensors.items())},
           'form': [bool(tr.enc_in_kernel), bool(tr.env_in_kernel), bool(tr.fused_encode), int(tr.handoff_fallbacks)],
           'rollout_nodes': None, 'update_nodes': None}
    if captured:
        assert tr.graph is not None and tr._upd is not None, tr.update_capture_error
        out['rollout_nodes'] = graph_nodes.census(tr.graph)
        out['update_nodes'] = {k: graph_nodes.census(g) for k, g in sorted(tr._upd.items()) if isinstance(g, torch.cuda.CUDAGraph)}
    return out


def record(path):
    for d in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
        if d not in sys.path:
            sys.path.insert(0, d)
    cases = {}
    for agent, scenario in NETS:
        for saved in (True, False):
            for captured in (False, True):
                name = '%s/%s %s %s' % (agent, scenario, 'saved' if saved else 'recompute', 'captured' if captured else 'eager')
                cases[name] = run_case(agent, scenario, saved, captured)
                print(name, 'tensors %d' % len(cases[name]['tensors']), cases[name]['form'], cases[name]['rollout_nodes'], flush=True)
                with open(path, 'w') as f:        # (written case by case: a run that is cut short leaves what it reached)
                    json.dump(cases, f, indent=1, sort_keys=True)


def compare(a_path, b_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    differ = 0
    for name in sorted(set(a) | set(b)):
        x, y = a.get(name), b.get(name)
        if x == y:
            print('%-40s equal  tensors %d  form %s  rollout nodes %s  update nodes %s'
                  % (name, len(x['tensors']), x['form'], x['rollout_nodes'], x['update_nodes']))
            continue
        differ += 1
        if x is None or y is None:
            print('%-40s only in %s' % (name, b_path if x is None else a_path))
            continue
        what = [k for k in sorted(set(x['tensors']) | set(y['tensors'])) if x['tensors'].get(k) != y['tensors'].get(k)]
        what += [k for k in ('form', 'rollout_nodes', 'update_nodes') if x[k] != y[k]]
        print('%-40s DIFFER in %s' % (name, ', '.join(what)))
    print('%d cases, %d differ' % (len(set(a) | set(b)), differ))
    return 1 if differ else 0


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == '--compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2 or sys.argv[1].startswith('-'):
        sys.exit(__doc__)
    record(sys.argv[1])

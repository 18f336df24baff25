"""The opt-in replica minibatches of the PPO epochs under data parallelism ON THE GPU: two ranks on one device (gloo carries the
device tensors; with two visible devices RCCL, one rank each), as tests/test_gpu_ppo_dist.py.  1 + (K - 1) M optimiser steps per
batch are as many all-reduces per batch -- the first batch eager, the second through the chain of captured graphs split at every
all-reduce --, both ranks hold the same weights, and under ppo_target_kl both stop at the same step (the KL rides through the
all-reduce)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
K, M, BATCHES, E = 2, 2, 2, 8
STEPS = 1 + (K - 1) * M


def _run(E, env_id_base, group, device, target_kl=None):
    sys.path.insert(0, HERE)
    sys.path.insert(0, ROOT)
    from helpers import cacc_config
    from deeprl_network_amd.agents import models
    from deeprl_network_amd.envs.cacc_env import CACCBatchEnv
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    cp = cacc_config(agent='ia2c_fp', n_step=10, reward_norm=800.0)
    cp['ENV_CONFIG']['episode_length_sec'] = '2'                   # T = 20 = 2 batches: episode ends + auto-reset inside
    cp['MODEL_CONFIG']['ppo_epochs'] = str(K)
    cp['MODEL_CONFIG']['ppo_minibatches'] = str(M)
    if target_kl is not None:
        cp['MODEL_CONFIG']['ppo_target_kl'] = target_kl
    env = CACCBatchEnv(cp['ENV_CONFIG'], num_envs=E, device=device, env_id_base=env_id_base)
    np.random.seed(12)
    model = models.IA2C_FP(env.n_s_ls, env.n_a_ls, env.neighbor_mask, env.distance_mask, env.coop_gamma, 10 ** 6,
                           cp['MODEL_CONFIG'], seed=12, num_envs=E, device=device, dist_group=group)
    tr = BatchedTrainer(env, model, Counter(10 ** 9, 10 ** 9, 10 ** 9), use_graph=True, rank=dist.get_rank(group), world_size=2)
    for _ in range(BATCHES):
        tr.run_batch()
    torch.cuda.synchronize()
    chain = None if tr._upd is None else len(tr._upd.get('chain', ()))
    return dict(flat=model.policy.params.flat.detach().cpu().clone(), allreduces=getattr(model, 'allreduce_calls', 0), chain=chain,
                error=tr.update_capture_error, perm=model.mb_perm.cpu().clone(), base=model.mb_env_id_base,
                gate=None if target_kl is None else model.ppo_gate.cpu().tolist(), steps_done=model.ppo_steps_done)


def _worker(rank, world, port, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    if torch.cuda.device_count() >= 2:
        backend, dev = 'nccl', rank
    else:
        backend, dev = 'gloo', 0
    torch.cuda.set_device(dev)
    device = torch.device('cuda', dev)
    if backend == 'nccl':
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=device)
    else:
        dist.init_process_group('gloo', rank=rank, world_size=world)
    res = dict(plain=_run(E, rank * E, dist.group.WORLD, device), stop=_run(E, rank * E, dist.group.WORLD, device, target_kl='1e-12'),
               backend=backend)
    torch.save(res, os.path.join(out, 'rank%d.pt' % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_make_one_all_reduce_per_step_and_stop_together(tmp_path):
    import ppo_minibatch_checks as mc
    port = 29100 + (os.getpid() % 1500)
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / 'rank0.pt'), torch.load(tmp_path / 'rank1.pt')
    for r in (r0, r1):
        p = r['plain']
        assert p['error'] is None and p['allreduces'] == STEPS * BATCHES        # one all-reduce per optimiser step
        assert p['chain'] == (K - 1) * M                                          # the captured update: 2 + (K - 1) M graphs
    assert torch.equal(r0['plain']['flat'], r1['plain']['flat']), 'ranks diverged (%s)' % r0['backend']
    # every rank permutes its own shard, its replicas' keys drawn under their global ids
    for rank, r in enumerate((r0, r1)):
        assert r['plain']['base'] == rank * E
        assert np.array_equal(r['plain']['perm'].numpy(), mc.perm(E, K, BATCHES - 1, 12, rank * E))
    # a target below every step's KL: both ranks refuse every step behind the first, at the same step
    s0, s1 = r0['stop'], r1['stop']
    assert s0['error'] is None and s1['error'] is None and s0['allreduces'] == STEPS * BATCHES
    assert s0['gate'] == s1['gate'] and s0['steps_done'] == s1['steps_done'] == 1 and s0['gate'][0] == 1
    assert torch.equal(s0['flat'], s1['flat']) and not torch.equal(s0['flat'], r0['plain']['flat'])

"""The opt-in PPO epochs under data parallelism ON THE GPU: two ranks on one device (gloo carries the device tensors; with two visible
devices RCCL, one rank each), as tests/test_gpu_dist.py::test_two_ranks_equal_one_process_on_gpu.  K optimiser steps per batch are
K all-reduces per batch -- the first batch eager, the second through the chain of K + 1 captured graphs split at every all-reduce --
and 2 ranks x E replicas == one process x 2 E replicas."""
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
K, BATCHES = 2, 2


def _run(E, env_id_base, group, device):
    sys.path.insert(0, HERE)
    sys.path.insert(0, ROOT)
    from helpers import cacc_config
    from deeprl_network_amd.agents import models
    from deeprl_network_amd.envs.cacc_env import CACCBatchEnv
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    cp = cacc_config(agent='ia2c_fp', n_step=10, reward_norm=800.0)
    cp['ENV_CONFIG']['episode_length_sec'] = '2'                   # T = 20 = 2 batches: episode ends + auto-reset inside
    cp['MODEL_CONFIG']['ppo_epochs'] = str(K)
    env = CACCBatchEnv(cp['ENV_CONFIG'], num_envs=E, device=device, env_id_base=env_id_base)
    np.random.seed(12)
    model = models.IA2C_FP(env.n_s_ls, env.n_a_ls, env.neighbor_mask, env.distance_mask, env.coop_gamma, 10 ** 6,
                           cp['MODEL_CONFIG'], seed=12, num_envs=E, device=device, dist_group=group)
    world = 1 if group is None else dist.get_world_size(group)
    tr = BatchedTrainer(env, model, Counter(10 ** 9, 10 ** 9, 10 ** 9), use_graph=True,
                        rank=0 if group is None else dist.get_rank(group), world_size=world)
    for _ in range(BATCHES):
        tr.run_batch()
    torch.cuda.synchronize()
    chain = None if tr._upd is None else len(tr._upd.get('chain', ()))
    return model.policy.params.flat.detach().cpu().clone(), getattr(model, 'allreduce_calls', 0), chain, tr.update_capture_error


def _worker(rank, world, port, E, out):
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
    res = _run(E, rank * E, dist.group.WORLD, device)
    torch.save(res + (backend,), os.path.join(out, 'rank%d.pt' % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_with_two_epochs_equal_one_process(tmp_path):
    E = 64
    port = 29100 + (os.getpid() % 1500)
    mp.spawn(_worker, args=(2, port, E, str(tmp_path)), nprocs=2, join=True)
    w0, n0, chain0, err0, be = torch.load(tmp_path / 'rank0.pt')
    w1, n1, chain1, err1, _ = torch.load(tmp_path / 'rank1.pt')
    assert err0 is None and err1 is None
    assert n0 == n1 == K * BATCHES == 4                       # K all-reduces per update
    assert chain0 == chain1 == K - 1                          # the captured update: K + 1 graphs, K - 1 of them [apply k | grads k + 1]
    assert torch.equal(w0, w1), 'ranks diverged (%s)' % be
    single, n, chain, err = _run(2 * E, 0, None, torch.device('cuda', 0))
    assert n == 0 and chain == 0 and err is None
    torch.testing.assert_close(w0, single, rtol=2e-4, atol=2e-6)

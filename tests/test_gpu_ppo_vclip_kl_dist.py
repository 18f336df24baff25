"""The KL stop of the PPO epochs under data parallelism ON THE GPU: two ranks on one device (gloo carries the device tensors; with two
visible devices RCCL, one rank each), as tests/test_gpu_ppo_dist.py.  The sum of approx_kl rides in the float behind the gradient, so
there are still K all-reduces per update, both ranks compare the same pooled KL with the target and stop at the same epoch -- the
first batch eager, the second through the chain of captured graphs split at every all-reduce."""
import math
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
K, BATCHES, E = 4, 2, 16


def _run(group, device, rank, keys):
    from helpers import cacc_config
    from deeprl_network_amd.agents import models
    from deeprl_network_amd.envs.cacc_env import CACCBatchEnv
    from deeprl_network_amd.utils import BatchedTrainer, Counter
    cp = cacc_config(agent='ia2c_fp', n_step=5, reward_norm=800.0)
    cp['ENV_CONFIG']['episode_length_sec'] = '1'                   # T = 10 = 2 batches
    cp['MODEL_CONFIG']['ppo_epochs'] = str(K)
    for k, v in keys.items():
        cp['MODEL_CONFIG'][k] = v
    env = CACCBatchEnv(cp['ENV_CONFIG'], num_envs=E, device=device, env_id_base=rank * E)
    np.random.seed(12)
    model = models.IA2C_FP(env.n_s_ls, env.n_a_ls, env.neighbor_mask, env.distance_mask, env.coop_gamma, 10 ** 6,
                           cp['MODEL_CONFIG'], seed=12, num_envs=E, device=device, dist_group=group)
    tr = BatchedTrainer(env, model, Counter(10 ** 9, 10 ** 9, 10 ** 9), use_graph=True, rank=rank, world_size=dist.get_world_size(group))
    per = []
    for _ in range(BATCHES):
        tr.run_batch()
        per.append((model.ppo_stats[:, :, 0].detach().cpu().clone(), model.ppo_epochs_done))
    torch.cuda.synchronize()
    return dict(flat=model.policy.params.flat.detach().cpu().clone(), ms=model.policy.params.ms.detach().cpu().clone(), per=per,
                calls=getattr(model, 'allreduce_calls', 0), chain=None if tr._upd is None else len(tr._upd.get('chain', ())),
                err=tr.update_capture_error)


def _worker(rank, world, port, out):
    sys.path.insert(0, HERE)
    sys.path.insert(0, ROOT)
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
    group = dist.group.WORLD
    # the target-off run: the KL of the first update's epochs, pooled over agents and ranks as the gate pools it
    off = _run(group, device, rank, {})
    kl = off['per'][0][0][1:].double().sum(dim=1).to(device)       # [K - 1] sums over this rank's agents
    local = kl.cpu().clone()
    dist.all_reduce(kl, group=group)
    n_agent = off['per'][0][0].shape[1]
    pooled = (kl.cpu() / (world * n_agent)).tolist()
    ks = [k for k in range(3, K + 1) if pooled[k - 2] > 1.5 * max(pooled[:k - 2])]
    res = dict(off=off, local=local, pooled=pooled, backend=backend, ks=ks)
    if ks:
        kappa = math.sqrt(pooled[ks[0] - 2] * max(pooled[:ks[0] - 2]))
        res['kappa'] = kappa
        res['on'] = _run(group, device, rank, dict(ppo_target_kl=repr(kappa)))
    torch.save(res, os.path.join(out, 'rank%d.pt' % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_stop_at_the_same_epoch(tmp_path):
    sys.path.insert(0, HERE)
    import ppo_vclip_checks as vc
    port = 29100 + (os.getpid() % 1500)
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / ('rank%d.pt' % r), weights_only=False) for r in (0, 1))
    print('pooled kl_2..kl_K:', r0['pooled'], 'rank-local sums:', r0['local'].tolist(), r1['local'].tolist())
    assert r0['pooled'] == r1['pooled'] and r0['ks'] == r1['ks']
    assert not torch.equal(r0['local'], r1['local'])             # the ranks see different replicas: only the pooled KL can agree
    assert r0['ks'], 'precondition: some k* >= 3 with kl_k* > 1.5 max(kl_2..kl_{k*-1}); got %r' % (r0['pooled'],)
    k_star = r0['ks'][0]
    a, b = r0['on'], r1['on']
    for r in (a, b, r0['off'], r1['off']):
        assert r['err'] is None and r['calls'] == K * BATCHES and r['chain'] == K - 1          # still K all-reduces per update
    assert [d for _, d in a['per']] == [d for _, d in b['per']], 'the ranks stopped at different epochs'
    assert a['per'][0][1] == k_star - 1
    assert torch.equal(a['flat'], b['flat']) and torch.equal(a['ms'], b['ms']), 'ranks diverged (%s)' % r0['backend']
    assert not torch.equal(a['flat'], r0['off']['flat'])
    # every update, the replayed one included, follows the definition on the KL pooled over both ranks
    n_agent = a['per'][0][0].shape[1]
    for (sa, done), (sb, _) in zip(a['per'], b['per']):
        sums = (sa[1:].double().sum(dim=1) + sb[1:].double().sum(dim=1)).tolist()
        kls = [s / (2 * n_agent) for s in sums]
        if all(abs(x / r0['kappa'] - 1.0) > 1e-3 for x in kls):   # (the host's float64 pooling decides like the device's fp32 one)
            assert done == vc.gate_sequence(sums, r0['kappa'], 2 * n_agent)[1]

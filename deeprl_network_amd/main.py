"""train / evaluate drivers -- the reference's main.py (21-163) on the MI355X path."""
import argparse
import logging
import os

import numpy as np
import torch

from .agents.models import IA2C, IA2C_CU, IA2C_FP, MA2C_DIAL, MA2C_IC3, MA2C_NC
from .envs import init_env, make_batch_env, net_file
from .envs.atsc import RULE_AGENTS
from .envs.greedy import GreedyBatchController
from .envs.maxpressure import MaxPressureBatchController
from .utils import (BatchedEvaluator, BatchedTrainer, Counter, Evaluator, SummaryWriter, Trainer, check_dir, copy_file, find_file,
                    init_dir, init_log)

AGENTS = {'ia2c': IA2C, 'ia2c_fp': IA2C_FP, 'ma2c_nc': MA2C_NC, 'ma2c_ic3': MA2C_IC3, 'ma2c_cu': IA2C_CU,
          'ma2c_dial': MA2C_DIAL}


# The MODEL_CONFIG keys `train` overrides from the command line: (flag, key, how the parsed value is written into the ini, argparse's
# type or choices of the flag, its help)
OVERRIDES = (
    ('--lstm-precision', 'lstm_precision', str, dict(choices=('fp32', 'bf16x3')),
     'arithmetic of the rollout\'s LSTM products (overrides MODEL_CONFIG lstm_precision; default fp32). '
     'bf16x3: opt-in split-bf16 form, IA2C / IA2C-FP / ConseNet only; the update stays fp32'),
    ('--gae-lambda', 'gae_lambda', repr, dict(type=float),
     'lambda of generalised advantage estimation in [0, 1] (overrides MODEL_CONFIG gae_lambda; default 1 = the '
     'reference\'s n-step advantage).  Below 1 the critic\'s target is the lambda-return'),
    ('--optimizer', 'optimizer', str, dict(choices=('rmsprop', 'adam')),
     'optimiser behind the gradient clip (overrides MODEL_CONFIG optimizer; default rmsprop = the reference\'s '
     'TF-1.12 RMSProp).  adam: opt-in bias-corrected Adam (MODEL_CONFIG adam_beta1 / adam_beta2 / adam_epsilon)'),
    ('--adv-norm', 'adv_norm', str, dict(choices=('none', 'agent', 'all')),
     'per-batch standardisation of the advantage in the policy-gradient term (overrides MODEL_CONFIG adv_norm; '
     'default none).  agent: zero mean and unit std per agent; all: over all agents together.  The critic\'s '
     'target is not touched (MODEL_CONFIG adv_norm_epsilon, default 1e-8, is added to the std)'),
    ('--reward-scale', 'reward_scale', str, dict(choices=('none', 'return')),
     'scale of the training rewards (overrides MODEL_CONFIG reward_scale; default none = raw / reward_norm).  '
     'return: divide by the running std of the discounted return over everything seen so far, in place of '
     'reward_norm (MODEL_CONFIG reward_scale_epsilon, default 1e-8, is added to the std); evaluation is untouched'),
    ('--ppo-epochs', 'ppo_epochs', str, dict(type=int),
     'optimiser steps per batch (overrides MODEL_CONFIG ppo_epochs; default 1 = one A2C step).  K > 1: the first '
     'step is the A2C step, steps 2..K recompute the forward pass and apply the clipped surrogate against the '
     'policy that produced the batch; IA2C / IA2C-FP / ConseNet only, fp32 only'),
    ('--ppo-clip', 'ppo_clip', repr, dict(type=float),
     'epsilon of the clipped surrogate (overrides MODEL_CONFIG ppo_clip; default 0.2; finite and > 0)'),
    ('--ppo-vclip', 'ppo_vclip', repr, dict(type=float),
     'clip range of the value loss in steps 2..K (overrides MODEL_CONFIG ppo_vclip; default absent = unclipped).  '
     'The critic\'s error is the larger of (R - v)^2 and (R - v_clipped)^2, v_clipped within +-this of the value '
     'under the weights that produced the batch; finite and > 0, needs --ppo-epochs / ppo_epochs > 1'),
    ('--ppo-target-kl', 'ppo_target_kl', repr, dict(type=float),
     'KL stop of steps 2..K (overrides MODEL_CONFIG ppo_target_kl; default absent = no stop).  Once the mean '
     'approx_kl of a step exceeds this, that step and the rest of the update change nothing; decided on the '
     'device, the remaining passes still run (it buys stability, not time); finite and > 0, needs ppo_epochs > 1'),
    ('--ppo-minibatches', 'ppo_minibatches', str, dict(type=int),
     'replica minibatches of epochs 2..K (overrides MODEL_CONFIG ppo_minibatches; default 1 = one full-batch step '
     'per epoch).  M > 1: every epoch permutes the replicas on the device and makes M optimiser steps, each on '
     'E / M whole sequences; M must divide the replicas per rank, needs ppo_epochs > 1'),
)


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--base-dir', type=str, required=False, default='./runs/default', help='experiment base dir')
    subparsers = parser.add_subparsers(dest='option', help='train or evaluate')
    sp = subparsers.add_parser('train', help='train a single agent under base dir')
    sp.add_argument('--config-dir', type=str, required=False, default='./config/config_ia2c_fp_catchup.ini',
                    help='experiment config path')
    sp.add_argument('--num-envs', type=int, default=None, help='replicas per GPU (overrides ENV_CONFIG num_envs)')
    sp.add_argument('--no-graph', action='store_true', help='do not capture the rollout in a hipGraph')
    sp.add_argument('--no-train-record', action='store_true',
                    help='batched training: no per-update loss / lr / gradnorm scalars and no train_summary.csv')
    for flag, _, _, kw, text in OVERRIDES:
        sp.add_argument(flag, default=None, help=text, **kw)
    sp = subparsers.add_parser('evaluate', help='evaluate and compare agents under base dir')
    sp.add_argument('--evaluation-seeds', type=str, required=False,
                    default=','.join([str(i) for i in range(2000, 2500, 10)]),
                    help='random seeds for evaluation, split by ,')
    sp.add_argument('--batched', action='store_true',
                    help='all evaluation seeds as the replicas of one device-resident batch (BatchedEvaluator); same CSVs')
    sp.add_argument('--demo', action='store_true', help='kept for CLI compatibility (no SUMO gui here)')
    args = parser.parse_args(argv)
    if not args.option:
        parser.print_help()
        raise SystemExit(1)
    return args


def init_agent(env, config, total_step, seed, **kw):
    if env.agent in RULE_AGENTS:               # the rule-based baselines: the ATSC envs know theirs (envs/atsc.py), no other env has one
        host_controller = getattr(env, 'host_controller', None)
        return host_controller() if host_controller is not None else None
    cls = AGENTS.get(env.agent)
    if cls is None:
        return None
    return cls(env.n_s_ls, env.n_a_ls, env.neighbor_mask, env.distance_mask, env.coop_gamma, total_step, config,
               seed=seed, n_feat_ls=getattr(env, 'n_feat_ls', None), obs_order=getattr(env, 'neighbor_order', None), **kw)


def _dist():
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    group = None
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(local)
        dist.init_process_group('nccl', device_id=torch.device('cuda', local))
        group = dist.group.WORLD
    return world, rank, local, group


def apply_overrides(config, args, run_ini=None):
    """The MODEL_CONFIG keys the command line overrides (OVERRIDES), set
    on every rank; run_ini (rank 0): the run's copy of the ini, rewritten with them -- `evaluate` rebuilds the policy from that file."""
    given = {key: render(getattr(args, key)) for _, key, render, _, _ in OVERRIDES if getattr(args, key, None) is not None}
    for k, v in given.items():
        config.set('MODEL_CONFIG', k, v)
    if given and run_ini is not None:
        with open(run_ini, 'w') as f:
            config.write(f)
    return bool(given)


def train(args):
    world, rank, local, group = _dist()
    dirs = init_dir(args.base_dir)
    init_log(dirs['log'], rank)
    config = net_file.read_ini(args.config_dir)           # (an ENV_CONFIG net_file resolves against the ini's directory)
    if rank == 0:
        copy_file(args.config_dir, dirs['data'])
    run_ini = os.path.join(dirs['data'], os.path.basename(args.config_dir))
    apply_overrides(config, args, run_ini if rank == 0 else None)
    if rank == 0:                                         # the network's file travels with the run: `evaluate` needs nothing else
        net_file.copy_into_run(config, dirs['data'], run_ini)
    env_cfg = config['ENV_CONFIG']
    if env_cfg.get('agent') in RULE_AGENTS:
        # the rule-based ATSC baselines have nothing to train (no add_transition / backward / save): say so instead of dying on an
        # AttributeError after the first env step with a half-initialised run directory -- `main.py evaluate` is their mode
        # (asked before TRAIN_CONFIG is read: their inis have neither that section nor MODEL_CONFIG)
        logging.error('Training: agent "%s" is a rule-based controller; run `main.py evaluate` on it' % env_cfg.get('agent'))
        return
    total_step = int(config.getfloat('TRAIN_CONFIG', 'total_step'))
    test_step = int(config.getfloat('TRAIN_CONFIG', 'test_interval'))
    log_step = int(config.getfloat('TRAIN_CONFIG', 'log_interval'))
    counter = Counter(total_step, test_step, log_step)
    seed = config.getint('ENV_CONFIG', 'seed')
    num_envs = args.num_envs if args.num_envs is not None else env_cfg.getint('num_envs', fallback=1)
    device = torch.device('cuda', local)
    writer = SummaryWriter(dirs['log']) if rank == 0 else None
    if num_envs <= 1 and world == 1:
        env = init_env(env_cfg, device=device)                       # seeds np.random (cacc_env.py:22)
        logging.info('Training: a dim %r, agent dim: %d' % (env.n_a_ls, env.n_agent))
        model = init_agent(env, config['MODEL_CONFIG'], total_step, seed, device=device)
        trainer = Trainer(env, model, counter, writer, output_path=dirs['data'])
        trainer.run()
    else:
        env = make_batch_env(env_cfg, num_envs=num_envs, device=device, env_id_base=rank * num_envs)
        np.random.seed(seed)                                         # same initial weights on every rank
        model = init_agent(env, config['MODEL_CONFIG'], total_step, seed, num_envs=num_envs, device=device,
                           dist_group=group)
        trainer = BatchedTrainer(env, model, counter, writer, output_path=dirs['data'],
                                 use_graph=not args.no_graph, rank=rank, world_size=world,
                                 record=False if args.no_train_record else None)
        trainer.run()
    if rank == 0:
        final_step = counter.cur_step
        logging.info('Training: save final model at step %d ...' % final_step)
        model.save(dirs['model'], final_step)


def _open_run(run_dir):
    """A finished training run on disk -> the parsed ini `train` left under <run>/data/ (main.py:112-123 of the reference finds it
    the same way), or None with the reason logged."""
    if not check_dir(run_dir):
        logging.error('Evaluation: %s does not exist!' % os.path.basename(run_dir.rstrip('/')))
        return None
    ini = find_file(os.path.join(run_dir, 'data') + '/')
    if not ini:
        return None
    return net_file.read_ini(ini)


def model_config(cfg):
    """The run's MODEL_CONFIG section; None where the ini has none (config_greedy.ini, config_maxpressure*.ini: a rule-based agent reads no model keys)."""
    return cfg['MODEL_CONFIG'] if cfg.has_section('MODEL_CONFIG') else None


def evaluate(args):
    """`main.py evaluate` (reference main.py:112-155): the run under --base-dir is rebuilt from its own ini, its newest checkpoint
    loaded, and the Evaluator replays the test seeds into <run>/eva_data (port 1, no GUI: the synthetic envs have neither)."""
    run_dir = args.base_dir
    out = init_dir(run_dir, pathes=['eva_data', 'eva_log'])
    init_log(out['eva_log'])
    logging.info('Evaluation: random seeds: %s' % args.evaluation_seeds)
    seeds = [int(tok) for tok in args.evaluation_seeds.split(',')] if args.evaluation_seeds else []
    cfg = _open_run(run_dir)
    if cfg is None:
        return
    if args.batched:
        return evaluate_batched(cfg, seeds, run_dir, out['eva_data'])
    env = init_env(cfg['ENV_CONFIG'], port=1)
    env.init_test_seeds(seeds)
    model = init_agent(env, model_config(cfg), 0, 0)
    if model is None or not model.load(os.path.join(run_dir, 'model') + '/'):
        return
    Evaluator(env, model, out['eva_data'], gui=False).run()


def evaluate_batched(cfg, seeds, run_dir, output_path):
    """`main.py evaluate --batched`: the seeds are the replicas of one batch env, the policy is built for that many replicas (or
    is the batched greedy / max-pressure controller), and BatchedEvaluator writes the CSVs the loop above writes.  A scenario / agent pair the
    batch engine cannot build raises the engine's own error."""
    E = len(seeds)
    if E < 1:
        logging.error('Evaluation: no evaluation seeds')
        return None
    env_cfg = cfg['ENV_CONFIG']
    env = make_batch_env(env_cfg, num_envs=E)
    if env.agent == 'greedy':
        model = GreedyBatchController(env)
    elif env.agent == 'maxpressure':
        model = MaxPressureBatchController(env)
    else:
        model = init_agent(env, model_config(cfg), 0, 0, num_envs=E)
    if model is None or not model.load(os.path.join(run_dir, 'model') + '/'):
        return None
    return BatchedEvaluator(env, model, seeds, output_path).run()


def main(argv=None):
    args = parse_args(argv)
    if args.option == 'train':
        train(args)
    else:
        evaluate(args)

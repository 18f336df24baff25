"""What the synthetic ATSC scenarios share on the host -- the part of the reference's envs/atsc_env.py that does not depend on
the road network: the objectives and the rule-based agents' names, the common ENV_CONFIG keys, the state and output buffers of
E lock-stepped replicas with their reset / step calling convention (`AtscBatchEnv`), the one-replica reference duck-type on top
of such a batch (`AtscEnv`), and what every rule-based controller answers to Trainer.perform / main.py evaluate
(`RuleController`).  A scenario module (large_grid_env.py, real_net_env.py) adds its topology, its parameter keys, the library
entry points it calls and how an observation list is cut out of the observation buffer."""
import numpy as np
import torch

from .. import _lib

OBJECTIVES = {'queue': 0, 'wait': 1, 'hybrid': 2}
RULE_AGENTS = ('greedy', 'maxpressure')      # rule-based controllers: own-row observations, the global reward
N_GROUP = 4                                  # demand flow groups: one multiplier xi per replica and group


def atsc_params_from_config(config, p, what, objective, error):
    """The ENV_CONFIG keys of atsc_env.py:79-99 into the scenario's params struct p.  `what` names the scenario in the
    message, `objective` is the key's value as the scenario reads it, `error` the exception a bad one raises.  -> p"""
    if config.getint('control_interval_sec') != 5 or config.getint('yellow_interval_sec') != 2:
        raise _lib.NmarlError('the synthetic %s is specified for control 5 s / yellow 2 s' % what)
    if objective not in OBJECTIVES:
        raise error('objective must be one of queue, wait, hybrid (atsc_env.py:87, 411-416), got %r' % objective)
    p.objective = OBJECTIVES[objective]
    p.coef_wait = config.getfloat('coef_wait', fallback=0.0)
    p.norm_wave = config.getfloat('norm_wave')
    p.clip_wave = config.getfloat('clip_wave')
    p.T = int(np.ceil(config.getint('episode_length_sec') / config.getint('control_interval_sec')))
    p.per_agent_reward = 0 if config.getfloat('coop_gamma') < 0 else 1
    return p


def described(env, method, what):
    """env.<method>() -- `traffic_model`, `greedy_rule`, `pressure_table`: how an ATSC batch env describes itself to the traffic
    record and the rule-based agents.  Any other object is refused."""
    describe = getattr(env, method, None)
    if describe is None:
        raise _lib.NmarlError('the %s is defined for the ATSC grid and network envs, not for %s' % (what, type(env).__name__))
    return describe()


class RuleController:
    """What a rule-based controller shares with a trained agent's duck-type besides `forward(obs) -> actions`: `reset` / `load`
    exist so that Trainer.perform / main.py evaluate drive it."""
    n_step = 1

    def reset(self):
        return

    def load(self, model_dir, checkpoint=None):
        return True


class AtscBatchEnv:
    """E lock-stepped replicas of one scenario, all state on the device.  The subclass supplies `_scenario(config)` -- which
    sets `params`, `n_agent`, `n_a`, `n_a_ls`, `n_s_ls` and the masks and returns (lane or link width, observation width) --,
    the library calls `_reset_call(params, args)` / `_step_call(args)`, and `traffic_model` / `greedy_rule` / `pressure_table`."""

    def __init__(self, config, num_envs=1, device='cuda', env_id_base=0, seed=None):
        self.config = config
        self.E = int(num_envs)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.NmarlError('%s needs a HIP device; there is no CPU path' % type(self).__name__)
        self.name = config.get('scenario')
        self.agent = config.get('agent')
        self.coop_gamma = config.getfloat('coop_gamma')
        self.seed = config.getint('seed') if seed is None else int(seed)
        self.env_id_base = int(env_id_base)
        S, n_obs = self._scenario(config)
        p, E, N, d = self.params, self.E, self.n_agent, self.device
        self.T = p.T
        self.train_mode = True
        f32 = dict(dtype=torch.float32, device=d)
        self.q = torch.zeros(E, N, S, **f32)
        self.transit = torch.zeros(E, N, S, **f32)
        self.prev_action = torch.zeros(E, N, dtype=torch.uint8, device=d)
        self.t = torch.zeros(E, dtype=torch.int32, device=d)
        self.xi = torch.ones(E, N_GROUP, **f32)
        # `wait` / `hybrid` objectives: the front vehicle's standing time per lane or link (oracle/grid_ref.py step 6,
        # csrc/realnet.hip header)
        self.head_wait = torch.zeros(E, N, S, **f32) if p.objective else None
        if self.head_wait is not None:
            p.head_wait = self.head_wait.data_ptr()
        self.obs = torch.zeros(E, N, n_obs, **f32)
        self.reward = torch.zeros((E, N) if p.per_agent_reward else (E,), **f32)
        self.done = torch.zeros(E, dtype=torch.uint8, device=d)
        self.global_reward = torch.zeros(E, **f32)
        self.episode = torch.zeros(E, dtype=torch.int32, device=d)
        self.batch_size = None     # episodes end at T only; any n_step dividing T works

    def state_tensors(self):
        return [self.q, self.transit, self.prev_action, self.t, self.xi, self.obs, self.episode, self.done] + \
            ([self.head_wait] if self.head_wait is not None else [])

    def _outputs(self, obs_out, reward_out, done_out, greward_out):
        """The buffers a step writes: the caller's, the env's own where it names none."""
        return (self.obs if obs_out is None else obs_out, self.reward if reward_out is None else reward_out,
                self.done if done_out is None else done_out, self.global_reward if greward_out is None else greward_out)

    def _reset(self, params, E, mask, u0, seed, env_id_base, s=None):
        """The scenario's reset entry point on all replicas (s None) or on the contiguous slices s of the state."""
        P = _lib.ptr
        state = (self.episode, self.q, self.transit, self.prev_action, self.t, self.xi, self.obs)
        if s is not None:
            state = [x[s] for x in state]
        self._reset_call(params, (E, P(mask, torch.uint8), P(u0, torch.float32), seed, env_id_base, *[P(x) for x in state],
                                  _lib.stream()))

    def reset(self, mask=None, u0=None):
        self._reset(self.params, self.E, mask, u0, self.seed, self.env_id_base)
        return self.obs

    def reset_replica(self, e, seed):
        """Replica e alone, to the state the one-replica env takes for this seed (`AtscEnv.reset`: Philox key = seed, env id 0,
        episode 0): the reset entry point on the replica's contiguous slices, E = 1.  A batch whose replicas are the test seeds
        of an evaluation starts every one of them where the E = 1 path starts it, whatever its position in the batch."""
        s = slice(e, e + 1)
        p = type(self.params).from_buffer_copy(self.params)
        if self.head_wait is not None:
            p.head_wait = self.head_wait[s].data_ptr()
        self.episode[s].zero_()
        self._reset(p, 1, None, None, int(seed), 0, s)

    def step(self, action, auto_reset=False, obs_out=None, reward_out=None, done_out=None, greward_out=None):
        P = _lib.ptr
        out = obs, reward, done, greward = self._outputs(obs_out, reward_out, done_out, greward_out)
        self._step_call((self.E, P(action, torch.uint8), P(self.q), P(self.transit), P(self.prev_action), P(self.t), P(self.xi),
                         P(obs, torch.float32), P(reward, torch.float32), P(done, torch.uint8), P(greward, torch.float32),
                         1 if auto_reset else 0, self.seed, self.env_id_base, P(self.episode), _lib.stream()))
        return out

    def host_controller(self):
        """The host rule of the env's rule-based `agent` for one replica (what main.py's init_agent hands the Evaluator)."""
        if self.agent == 'greedy':                 # large_grid_env.py:30-45, real_net_env.py:112-145
            return self.greedy_rule()[0]
        from .maxpressure import MaxPressureController
        return MaxPressureController(self.pressure_table())


class AtscEnv:
    """Reference duck-type (atsc_env.py:77-524) for ONE replica on top of `batch_class(config, num_envs=1)`.  The subclass sets
    `node_names` and `_nbr` (per node its neighbours, ascending) and cuts the observation lists out of `batch.obs`
    (`_state_list`).  Neighbour actions come in mask order (ascending, atsc_env.py:132-136)."""
    batch_class = None

    def __init__(self, config, port=0, device='cuda', **_):
        b = self.batch = self.batch_class(config, num_envs=1, device=device)
        self.name, self.agent, self.coop_gamma, self.T = b.name, b.agent, b.coop_gamma, b.T
        self.n_agent, self.n_a, self.n_a_ls, self.n_s_ls = b.n_agent, b.n_a, b.n_a_ls, b.n_s_ls
        self.neighbor_mask, self.distance_mask = b.neighbor_mask, b.distance_mask
        self.seed = config.getint('seed')
        self.control_interval_sec = config.getint('control_interval_sec')
        self.init_test_seeds([int(s) for s in config.get('test_seeds').split(',')])
        self.cur_episode = 0
        self.train_mode = True
        self.is_record = False
        self.record = None           # the traffic / trip tables of an evaluation (envs/traffic_record.py): init_data(is_record=True)

    def init_data(self, is_record, record_stats, output_path):
        self.is_record, self.output_path = is_record, output_path
        if is_record:                                                    # atsc_env.py:142-145
            from .traffic_record import EpisodeRecord
            self.control_data, self.traffic_data, self.trip_data = [], [], []
            self.record = EpisodeRecord(self)
        else:
            self.record = None

    def init_test_seeds(self, test_seeds):
        self.test_num, self.test_seeds = len(test_seeds), test_seeds

    def get_neighbor_action(self, action):
        action = np.asarray(action)
        return [action[self.neighbor_mask[i] == 1] for i in range(self.n_agent)]

    def get_fingerprint(self):
        return self.fp

    def update_fingerprint(self, policy):
        self.fp = policy

    def terminate(self):
        return

    def collect_tripinfo(self):
        """The finished episode's rows of `_traffic.csv` and its row of `_trip.csv` (atsc_env.py:107-124, 464-499)."""
        if self.record is not None:
            self.record.collect(self.traffic_data, self.trip_data)

    def output_data(self):
        if self.is_record:
            from .traffic_record import write_tables
            write_tables(self)

    def host_controller(self):
        ctl = self.batch.host_controller()
        ctl.node_names = self.node_names
        return ctl

    def reset(self, gui=False, test_ind=0):
        seed = self.seed if self.train_mode else self.test_seeds[test_ind]      # atsc_env.py:167-170
        self.batch.seed = seed
        self.batch.episode.zero_()
        self.batch.reset()
        if self.record is not None:
            self.record.begin()
        self.cur_episode += 1
        self.fp = [np.ones(a) / a for a in self.n_a_ls]                  # atsc_env.py:498-499
        self.seed += 1
        return self._state_list()

    def step(self, action):
        a = torch.as_tensor(np.asarray(action, dtype=np.uint8).reshape(1, -1), device=self.batch.device)
        _, reward, done, g = self.batch.step(a)
        if self.record is not None:
            self.record.step()                                         # one launch behind the step, nothing read back here
        global_reward = float(g.item())
        done = bool(done.item())
        if self.agent in RULE_AGENTS or self.coop_gamma < 0:             # atsc_env.py:205-206
            reward = global_reward
        else:
            reward = reward[0].cpu().numpy().astype(np.float64)
        if self.is_record:
            sec = int(self.batch.t.item()) * self.control_interval_sec
            self.control_data.append({'episode': self.cur_episode, 'time_sec': sec,
                                      'step': sec / self.control_interval_sec,
                                      'action': ','.join('%d' % x for x in action), 'reward': global_reward})
        return self._state_list(), reward, done, global_reward

"""The rule-based `greedy` ATSC agent for a batch of replicas: csrc/greedy.hip behind the duck-type of the host controllers."""
import torch

from .. import ops
from .atsc import RuleController, described


class GreedyBatchController(RuleController):
    """`LargeGridController` / `RealNetController` for E lock-stepped replicas.  `forward_batch(obs, out)` decides every
    (replica, node) with one launch of nmarl_atsc_greedy on the env's observation buffer -- nothing is read back --; `forward`
    is the host controller's, so the object also drives the one-replica loops.  The scenario is the table (n_a, mask) its env
    hands over (`greedy_rule`); the rule is DESIGN.md 6."""
    name = 'greedy'

    def __init__(self, batch_env):
        self.host, self.n_own, n_a, mask = described(batch_env, 'greedy_rule', 'greedy agent')
        self.node_names = self.host.node_names
        self.n_a_host, self.mask_host, self.a_max = n_a, mask, int(n_a.max())
        dev = torch.device(batch_env.device)
        self.n_a = torch.from_numpy(n_a).to(dev)
        self.mask = torch.from_numpy(mask.view('int32')).to(dev)

    def forward_batch(self, obs_tensor, out_actions):
        """obs_tensor [E,N,row] f32 (rows lead with the node's own wave vector) -> out_actions [E,N] u8.  The kernel reads rows of
        whole 16-byte pieces (nmarl_atsc_greedy refuses any other row); the network env's rows are 22 (1 + m_max) = 110 floats, so its
        own vectors -- the leading 22 floats, no neighbour's feature -- are staged into zero-padded rows of 24 floats first: one
        strided device copy (a torch elementwise kernel, not a launch of this library) per lock-step, nothing read back.  The grid
        env's buffers (12 or 60 floats per row) are handed over as they are."""
        E, N, row = obs_tensor.shape
        if row % 4:
            own = min(row, self.n_own)
            if self._own is None or self._own.shape[0] != E:
                self._own = torch.zeros(E, N, 24, dtype=torch.float32, device=obs_tensor.device)
            self._own[:, :, :own].copy_(obs_tensor[:, :, :own])
            obs_tensor = self._own
        return ops.atsc_greedy(self.n_a, self.mask, obs_tensor, out_actions, a_max=self.a_max)

    _own = None

    def forward(self, obs):
        return self.host.forward(obs)

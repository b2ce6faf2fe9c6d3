"""Off-policy collection: the replay ring `BatchedCarEnv.collect_transitions` fills and the torch actor a learner trains.

The reference's strongest drivers are SAC agents, and four of its six SB3 trainers are off-policy (learn/sac.py,
learn/td3.py, learn/td3_n.py, learn/ddpg.py): OffPolicyAlgorithm.collect_rollouts samples an exploring action, steps the
vec env and stores (obs, next_obs, action, reward, done, timeout) in a ReplayBuffer, from which the learner draws uniform
minibatches.  `BatchedCarEnv.set_explorer` / `collect_transitions` do the first three on the device
(csrc/nascar_actor.h: the explorer's epilogues of mlp_field_kernel; csrc/nascar_replay.h: replay_store_kernel), into the
device tensors of a `ReplayBuffer`, and `ReplayBuffer.sample` is ReplayBuffer.sample as one launch
(replay_sample_kernel).  `SquashedActorNet` is SB3's SAC Actor for this observation and action space as a plain torch
module, built from and exported to a `policy.SquashedActor` record: collect -> sample -> update the module ->
`update_explorer(net.export())`.

There is no trainer, critic or optimiser here: those are the learner's.
"""
import ctypes
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from . import policy as P

OBS_DIM = 38
BYTES_PER_TRANSITION = 2 * 4 * OBS_DIM + 8 + 4 + 3     # 319: obs, next_obs, action, reward, done / timeout / live


class ReplaySamples(NamedTuple):
    """ReplayBuffer.sample(): SB3's ReplayBufferSamples (observations, actions, next_observations, dones, rewards) plus
    `live`.  obs / next_obs [batch, 38], actions [batch, 2] (scaled, as the buffer keeps them), dones [batch] float32 =
    done * (1 - timeout), rewards [batch] float32, live [batch] uint8 (0: the car was already disabled before the step)."""
    obs: torch.Tensor
    actions: torch.Tensor
    next_obs: torch.Tensor
    dones: torch.Tensor
    rewards: torch.Tensor
    live: torch.Tensor


class ReplayBuffer:
    """A device replay ring of `capacity_steps` step slots x N = E * C cars for `env` (319 bytes per transition, so
    319 * N bytes per step slot).  `pos` is the slot the next step writes, `size` the filled slots, `full` whether the
    ring has wrapped -- SB3's ReplayBuffer bookkeeping, advanced by BatchedCarEnv.collect_transitions."""

    def __init__(self, env, capacity_steps: int):
        cap = int(capacity_steps)
        if cap < 1:
            raise ValueError("capacity_steps must be >= 1")
        self.env, self.E, self.C, self.N, self.device = env, env.E, env.C, env.N, env.device
        self.capacity, self.pos, self.full = cap, 0, False
        f32, u8, dev = torch.float32, torch.uint8, env.device
        self.obs = torch.zeros(cap, env.E, env.C, OBS_DIM, dtype=f32, device=dev)
        self.next_obs = torch.zeros_like(self.obs)
        self.actions = torch.zeros(cap, env.E, env.C, 2, dtype=f32, device=dev)
        self.rewards = torch.zeros(cap, env.E, env.C, dtype=f32, device=dev)
        self.dones = torch.zeros(cap, env.E, env.C, dtype=u8, device=dev)
        self.timeouts = torch.zeros_like(self.dones)
        self.live = torch.zeros_like(self.dones)

    @property
    def size(self) -> int:
        return self.capacity if self.full else self.pos

    @property
    def bytes_per_step(self) -> int:
        return BYTES_PER_TRANSITION * self.N

    def advance(self, steps: int):
        """the bookkeeping of `steps` ReplayBuffer.add calls"""
        p = self.pos + int(steps)
        self.full = self.full or p >= self.capacity
        self.pos = p % self.capacity

    def struct(self) -> _lib.NascarReplay:
        return _lib.NascarReplay(*[t.data_ptr() for t in (self.obs, self.next_obs, self.actions, self.rewards, self.dones,
                                                           self.timeouts, self.live)], self.capacity)

    def sample(self, batch: int, seed: int = 0, draw: int = 0, out: ReplaySamples = None) -> ReplaySamples:
        """`batch` transitions drawn uniformly over the filled slots x cars, as one gather launch on the current stream.
        Sample i of (seed, draw) is a counter hash (include/nascar.h), so a call is reproducible; a learner passes its
        update counter as `draw`.  `out`: a ReplaySamples of caller-owned buffers of at least `batch` rows."""
        B = int(batch)
        if B < 0:
            raise ValueError("batch must be >= 0")
        if self.size < 1:
            raise ValueError("the replay buffer is empty")
        dev, f32 = self.device, torch.float32
        if out is None:
            out = ReplaySamples(torch.empty(B, OBS_DIM, dtype=f32, device=dev), torch.empty(B, 2, dtype=f32, device=dev),
                                torch.empty(B, OBS_DIM, dtype=f32, device=dev), torch.empty(B, dtype=f32, device=dev),
                                torch.empty(B, dtype=f32, device=dev), torch.empty(B, dtype=torch.uint8, device=dev))
        else:
            want = ((OBS_DIM,), (2,), (OBS_DIM,), (), (), ())
            for name, t, inner in zip(ReplaySamples._fields, out, want):
                dt = torch.uint8 if name == "live" else f32
                if (t.device != dev or t.dtype != dt or tuple(t.shape[1:]) != inner or t.shape[0] < B
                        or not t.is_contiguous()):
                    raise ValueError(f"out {name}: need a contiguous {dt} tensor [>= {B}{''.join(', %d' % i for i in inner)}] "
                                     f"on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device}")
        r = self.struct()
        vp = ctypes.c_void_p
        with torch.cuda.device(dev):
            stream = vp(torch.cuda.current_stream().cuda_stream)
            _lib.check(_lib.lib().nascar_replay_sample(self.env.h, ctypes.byref(r), self.size, int(seed), int(draw), B,
                                                       vp(out.obs.data_ptr()), vp(out.next_obs.data_ptr()),
                                                       vp(out.actions.data_ptr()), vp(out.rewards.data_ptr()),
                                                       vp(out.dones.data_ptr()), vp(out.live.data_ptr()), stream))
        return out


class SquashedActorNet(torch.nn.Module):
    """SB3's SAC Actor (sac/policies.py) for Box(38) -> Box(-1, 1)^2 with two hidden layers, with SB3's parameter names
    (latent_pi.{0,2}, mu, log_std): its state_dict loads into, and from, the `actor` of an SB3 SAC policy of the same
    net_arch (the checkpoint's ``actor.*`` keys without the prefix)."""

    def __init__(self, actor: P.SquashedActor):
        super().__init__()
        act = {P.RELU: torch.nn.ReLU, P.TANH: torch.nn.Tanh}[int(actor.activation)]
        self.activation = int(actor.activation)
        L = torch.nn.Linear
        self.latent_pi = torch.nn.Sequential(L(OBS_DIM, actor.h1), act(), L(actor.h1, actor.h2), act())
        self.mu = L(actor.h2, 2)
        self.log_std = L(actor.h2, 2)
        self.load_record(actor)

    def load_record(self, actor: P.SquashedActor):
        w1, b1, w2, b2, w3, b3 = [torch.from_numpy(np.asarray(a, np.float32)) for a in actor.arrays]
        with torch.no_grad():
            for lin, w, b in ((self.latent_pi[0], w1, b1), (self.latent_pi[2], w2, b2), (self.mu, w3[:2], b3[:2]),
                              (self.log_std, w3[2:], b3[2:])):
                lin.weight.copy_(w)
                lin.bias.copy_(b)

    def export(self) -> P.SquashedActor:
        """the current parameters as a float32 SquashedActor record (for BatchedCarEnv.update_explorer)"""
        g = lambda t: t.detach().float().cpu().numpy()
        return P.make_squashed_actor([g(self.latent_pi[0].weight), g(self.latent_pi[0].bias), g(self.latent_pi[2].weight),
                                      g(self.latent_pi[2].bias), np.concatenate([g(self.mu.weight), g(self.log_std.weight)]),
                                      np.concatenate([g(self.mu.bias), g(self.log_std.bias)])], self.activation, "sac")

    def get_action_dist_params(self, obs):
        """(mean_actions, log_std) [n, 2], log_std clamped to [-20, 2] as Actor.get_action_dist_params does"""
        h = self.latent_pi(obs.reshape(-1, OBS_DIM))
        return self.mu(h), torch.clamp(self.log_std(h), P.LOG_STD_MIN, P.LOG_STD_MAX)

    def forward(self, obs, deterministic: bool = False, eps=None):
        """the squashed action tanh(mu) or tanh(mu + std * eps) (eps: standard normal [n, 2], drawn when None)"""
        mu, ls = self.get_action_dist_params(obs)
        if deterministic:
            return torch.tanh(mu)
        e = torch.randn_like(mu) if eps is None else eps.reshape(-1, 2)
        return torch.tanh(mu + ls.exp() * e)

    def action_log_prob(self, obs, eps=None):
        """Actor.action_log_prob: (action [n, 2], log_prob [n]) of a reparametrised sample -- the Gaussian's log-density
        of the unsquashed sample minus the tanh correction sum_j log(1 - a_j^2 + 1e-6) (SquashedDiagGaussianDistribution)."""
        mu, ls = self.get_action_dist_params(obs)
        e = torch.randn_like(mu) if eps is None else eps.reshape(-1, 2)
        g = mu + ls.exp() * e
        a = torch.tanh(g)
        logp = (-((g - mu) ** 2) / (2 * (ls.exp() ** 2)) - ls - 0.5 * math.log(2 * math.pi)).sum(dim=1)
        return a, logp - torch.log(1 - a ** 2 + 1e-6).sum(dim=1)

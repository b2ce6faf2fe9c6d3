"""On-policy collection: the buffer `BatchedCarEnv.collect` fills and the torch module a learner trains.

The reference trains its drivers with Stable-Baselines3's on-policy algorithms (learn/ppo.py:65-107, learn/a2c.py):
OnPolicyAlgorithm.collect_rollouts samples an action from the Gaussian actor, steps the vec env and stores observation,
action, log-probability, value, reward and episode start; RolloutBuffer.compute_returns_and_advantage then runs GAE.
`BatchedCarEnv.collect` does all of that on the device (csrc/nascar_actor.h: the MLP_OUT_SAMPLE / MLP_OUT_VALUE
epilogues of mlp_field_kernel and gae_kernel) and returns a `RolloutBatch`.  `ActorCriticNet` is SB3's
ActorCriticPolicy for this observation and action space as a plain torch module, built from and exported to a
`policy.ActorCritic` record, which closes the loop: collect -> update the module -> `update_actor_critic(net.export())`.

There is no trainer, logger or checkpoint writer here: the loss and the optimiser are the learner's.
"""
from typing import NamedTuple

import numpy as np
import torch

from . import policy as P

OBS_DIM = 38


class FlatBatch(NamedTuple):
    """RolloutBatch.flatten(): views [K * E * C, ...] of the K collected records, as SB3's RolloutBufferSamples"""
    obs: torch.Tensor
    actions: torch.Tensor
    log_probs: torch.Tensor
    values: torch.Tensor
    advantages: torch.Tensor
    returns: torch.Tensor


class RolloutBatch(NamedTuple):
    """One collected rollout of K steps over E envs x C cars (device tensors, written by the kernels in place).
    obs [K + 1, E, C, 38]: record k the observation the action of step k was sampled on, record K the one after the last
    step; actions [K, E, C, 2]: the unclipped samples (what SB3's buffer keeps; the envs were stepped with their clip to
    [-1, 1]); log_probs [K, E, C]; values [K + 1, E, C]: V(obs[k]); rewards [K, E, C]: the raw step rewards;
    timeout_values [K, E, C]: V(terminal observation) for the cars of envs a time limit cut at step k (truncated and not
    terminated), 0 elsewhere -- SB3 adds gamma times it to the reward; car_flags [K, E, C], env_flags [K, E] uint8;
    advantages, returns [K, E, C]: GAE of these records."""
    obs: torch.Tensor
    actions: torch.Tensor
    log_probs: torch.Tensor
    values: torch.Tensor
    rewards: torch.Tensor
    timeout_values: torch.Tensor
    car_flags: torch.Tensor
    env_flags: torch.Tensor
    advantages: torch.Tensor
    returns: torch.Tensor

    @staticmethod
    def spec(E, C):
        """(field, dtype, per-record shape, records beyond K) in field order"""
        f32, u8 = torch.float32, torch.uint8
        return [("obs", f32, (E, C, OBS_DIM), 1), ("actions", f32, (E, C, 2), 0), ("log_probs", f32, (E, C), 0),
                ("values", f32, (E, C), 1), ("rewards", f32, (E, C), 0), ("timeout_values", f32, (E, C), 0),
                ("car_flags", u8, (E, C), 0), ("env_flags", u8, (E,), 0), ("advantages", f32, (E, C), 0),
                ("returns", f32, (E, C), 0)]

    @property
    def steps(self) -> int:
        return int(self.actions.shape[0])

    def flatten(self) -> FlatBatch:
        K = self.steps
        return FlatBatch(self.obs[:K].reshape(-1, OBS_DIM), self.actions.reshape(-1, 2), self.log_probs.reshape(-1),
                         self.values[:K].reshape(-1), self.advantages.reshape(-1), self.returns.reshape(-1))

    def minibatches(self, n: int, seed: int = 0):
        """the K * E * C samples in n minibatches of a seeded random permutation (the last one takes the remainder)"""
        flat = self.flatten()
        total = flat.actions.shape[0]
        g = torch.Generator(device="cpu")
        g.manual_seed(int(seed))
        perm = torch.randperm(total, generator=g).to(flat.actions.device)
        size = -(-total // int(n))
        for i in range(0, total, size):
            idx = perm[i:i + size]
            yield FlatBatch(*[t[idx] for t in flat])


class NormalizedRolloutBatch(NamedTuple):
    """`BatchedCarEnv.collect` under `set_normalize`: RolloutBatch's fields -- obs and rewards the NORMALISED ones the
    actor-critic and GAE saw, timeout_values V of the normalised terminal observation -- plus raw_rewards [K, E, C], the
    step rewards before normalisation (what an episode-return monitor sums)."""
    obs: torch.Tensor
    actions: torch.Tensor
    log_probs: torch.Tensor
    values: torch.Tensor
    rewards: torch.Tensor
    timeout_values: torch.Tensor
    car_flags: torch.Tensor
    env_flags: torch.Tensor
    advantages: torch.Tensor
    returns: torch.Tensor
    raw_rewards: torch.Tensor

    @staticmethod
    def spec(E, C):
        """RolloutBatch.spec plus raw_rewards"""
        return RolloutBatch.spec(E, C) + [("raw_rewards", torch.float32, (E, C), 0)]

    steps = RolloutBatch.steps
    flatten = RolloutBatch.flatten
    minibatches = RolloutBatch.minibatches


class _Extractor(torch.nn.Module):
    def __init__(self, h1, h2, v1, v2, act, vact):
        super().__init__()
        L = torch.nn.Linear
        self.policy_net = torch.nn.Sequential(L(OBS_DIM, h1), act(), L(h1, h2), act())
        self.value_net = torch.nn.Sequential(L(OBS_DIM, v1), vact(), L(v1, v2), vact())


class ActorCriticNet(torch.nn.Module):
    """SB3's ActorCriticPolicy for Box(38) -> Box(-1, 1)^2 with an MlpExtractor of two hidden layers per branch and a
    state-independent log_std, with SB3's parameter names (mlp_extractor.policy_net.{0,2}, mlp_extractor.value_net.{0,2},
    action_net, value_net, log_std): its state_dict loads into, and from, an SB3 policy of the same net_arch."""

    def __init__(self, ac: P.ActorCritic):
        super().__init__()
        acts = {P.RELU: torch.nn.ReLU, P.TANH: torch.nn.Tanh}
        self.activation, self.vf_activation = int(ac.pi.activation), int(ac.vf.activation)
        self.mlp_extractor = _Extractor(ac.pi.h1, ac.pi.h2, ac.vf.h1, ac.vf.h2, acts[self.activation], acts[self.vf_activation])
        self.action_net = torch.nn.Linear(ac.pi.h2, 2)
        self.value_net = torch.nn.Linear(ac.vf.h2, 1)
        self.log_std = torch.nn.Parameter(torch.zeros(2))
        self.load_record(ac)

    def _layers(self):
        pn, vn = self.mlp_extractor.policy_net, self.mlp_extractor.value_net
        return (pn[0], pn[2], self.action_net), (vn[0], vn[2], self.value_net)

    def load_record(self, ac: P.ActorCritic):
        with torch.no_grad():
            for layers, arrays in zip(self._layers(), (ac.pi.arrays, ac.vf.arrays)):
                for i, lin in enumerate(layers):
                    lin.weight.copy_(torch.from_numpy(np.asarray(arrays[2 * i])))
                    lin.bias.copy_(torch.from_numpy(np.asarray(arrays[2 * i + 1])))
            self.log_std.copy_(torch.from_numpy(np.asarray(ac.log_std, np.float32)))

    def export(self) -> P.ActorCritic:
        """the current parameters as a float32 ActorCritic record (for BatchedCarEnv.update_actor_critic)"""
        pi, vf = [[a.detach().float().cpu().numpy() for lin in layers for a in (lin.weight, lin.bias)]
                  for layers in self._layers()]
        return P.ActorCritic(P.make_controller(pi, self.activation, P.OUT_RAW, "actor_critic"),
                             P.make_value_net(vf, self.vf_activation), self.log_std.detach().float().cpu().numpy().copy())

    def forward(self, obs):
        """(mu [n, 2], values [n, 1])"""
        x = obs.reshape(-1, OBS_DIM)
        return self.action_net(self.mlp_extractor.policy_net(x)), self.value_net(self.mlp_extractor.value_net(x))

    def evaluate_actions(self, obs, actions):
        """ActorCriticPolicy.evaluate_actions: (values [n, 1], log_prob [n], entropy [n]) of `actions` [n, 2] under the
        current policy on `obs` [n, 38] (DiagGaussianDistribution: independent normals, summed over the components)."""
        mu, values = self.forward(obs)
        dist = torch.distributions.Normal(mu, torch.ones_like(mu) * self.log_std.exp())
        return values, dist.log_prob(actions.reshape(-1, 2)).sum(dim=1), dist.entropy().sum(dim=1)


# ------------------------------------------------------------------ the categorical actor-critic (Discrete(5))
class DiscreteRolloutBatch(NamedTuple):
    """`BatchedCarEnv.collect` with a policy.DiscreteActorCritic: RolloutBatch's fields with actions int32 [K, E, C], the
    sampled action index in 0..4 (what SB3's buffer keeps for a Discrete space; the envs were stepped with it)."""
    obs: torch.Tensor
    actions: torch.Tensor
    log_probs: torch.Tensor
    values: torch.Tensor
    rewards: torch.Tensor
    timeout_values: torch.Tensor
    car_flags: torch.Tensor
    env_flags: torch.Tensor
    advantages: torch.Tensor
    returns: torch.Tensor

    @staticmethod
    def spec(E, C):
        """RolloutBatch.spec with the actions record int32 [E, C]"""
        return [("actions", torch.int32, (E, C), 0) if s[0] == "actions" else s for s in RolloutBatch.spec(E, C)]

    steps = RolloutBatch.steps
    minibatches = RolloutBatch.minibatches

    def flatten(self) -> FlatBatch:
        K = self.steps
        return FlatBatch(self.obs[:K].reshape(-1, OBS_DIM), self.actions.reshape(-1), self.log_probs.reshape(-1),
                         self.values[:K].reshape(-1), self.advantages.reshape(-1), self.returns.reshape(-1))


class NormalizedDiscreteRolloutBatch(NamedTuple):
    """DiscreteRolloutBatch under `set_normalize`: obs and rewards normalised, raw_rewards beside them (as
    NormalizedRolloutBatch)."""
    obs: torch.Tensor
    actions: torch.Tensor
    log_probs: torch.Tensor
    values: torch.Tensor
    rewards: torch.Tensor
    timeout_values: torch.Tensor
    car_flags: torch.Tensor
    env_flags: torch.Tensor
    advantages: torch.Tensor
    returns: torch.Tensor
    raw_rewards: torch.Tensor

    @staticmethod
    def spec(E, C):
        """DiscreteRolloutBatch.spec plus raw_rewards"""
        return DiscreteRolloutBatch.spec(E, C) + [("raw_rewards", torch.float32, (E, C), 0)]

    steps = RolloutBatch.steps
    flatten = DiscreteRolloutBatch.flatten
    minibatches = RolloutBatch.minibatches


class CategoricalActorCriticNet(torch.nn.Module):
    """SB3's ActorCriticPolicy for Box(38) -> Discrete(5) with an MlpExtractor of two hidden layers per branch, with SB3's
    parameter names (mlp_extractor.policy_net.{0,2}, mlp_extractor.value_net.{0,2}, action_net = Linear(h2, 5), value_net;
    no log_std): its state_dict loads into, and from, an SB3 policy of the same net_arch."""

    def __init__(self, ac: P.DiscreteActorCritic):
        super().__init__()
        acts = {P.RELU: torch.nn.ReLU, P.TANH: torch.nn.Tanh}
        self.activation, self.vf_activation = int(ac.pi.activation), int(ac.vf.activation)
        self.mlp_extractor = _Extractor(ac.pi.h1, ac.pi.h2, ac.vf.h1, ac.vf.h2, acts[self.activation], acts[self.vf_activation])
        self.action_net = torch.nn.Linear(ac.pi.h2, P.N_DISCRETE)
        self.value_net = torch.nn.Linear(ac.vf.h2, 1)
        self.load_record(ac)

    _layers = ActorCriticNet._layers

    def load_record(self, ac: P.DiscreteActorCritic):
        with torch.no_grad():
            for layers, arrays in zip(self._layers(), (ac.pi.arrays, ac.vf.arrays)):
                for i, lin in enumerate(layers):
                    lin.weight.copy_(torch.from_numpy(np.asarray(arrays[2 * i])))
                    lin.bias.copy_(torch.from_numpy(np.asarray(arrays[2 * i + 1])))

    def export(self) -> P.DiscreteActorCritic:
        """the current parameters as a float32 DiscreteActorCritic record (for BatchedCarEnv.update_actor_critic)"""
        pi, vf = [[a.detach().float().cpu().numpy() for lin in layers for a in (lin.weight, lin.bias)]
                  for layers in self._layers()]
        return P.make_discrete_actor_critic(pi, vf, self.activation, "actor_critic", self.vf_activation)

    def forward(self, obs):
        """(logits [n, 5], values [n, 1])"""
        x = obs.reshape(-1, OBS_DIM)
        return self.action_net(self.mlp_extractor.policy_net(x)), self.value_net(self.mlp_extractor.value_net(x))

    def evaluate_actions(self, obs, actions):
        """ActorCriticPolicy.evaluate_actions: (values [n, 1], log_prob [n], entropy [n]) of the action indices `actions` [n]
        under the current policy on `obs` [n, 38] (CategoricalDistribution: torch's Categorical(logits=...))."""
        logits, values = self.forward(obs)
        dist = torch.distributions.Categorical(logits=logits)
        return values, dist.log_prob(actions.reshape(-1).long()), dist.entropy()

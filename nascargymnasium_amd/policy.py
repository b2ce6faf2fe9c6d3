"""Controller weights for the fused device policies.

The reference's SACController loads a Stable-Baselines3 checkpoint with ``SAC.load``
(game/control/sac_control_class.py:48-76) and calls ``model.predict(obs, deterministic=True)``.
Here the checkpoint zip is opened with ``zipfile`` and ``policy.pth`` with
``torch.load(weights_only=True)`` -- nothing in the file is executed -- and only the actor
tensors are kept; inference runs in ``actor_kernel`` (csrc/nascar_actor.h).

The reference's race modes (game/competition.py:150-212) put a different controller in every car: SAC, PPO and
A2C checkpoints beside the rule driver.  ``load_sb3_policy`` reads any of the three kinds into a ``Controller``
record -- a two-hidden-layer MLP 38 -> h1 -> h2 -> 2 with its activation and output transform -- for
``BatchedCarEnv.add_controller`` / ``set_car_controllers`` (policy 4, ``mlp_field_kernel``).

The reference's trainers (learn/ppo.py, learn/a2c.py) need the rest of such a checkpoint: ``load_sb3_actor_critic`` reads
policy net, value net and ``log_std`` into an ``ActorCritic`` record for ``BatchedCarEnv.set_actor_critic`` / ``collect``
(policy 6: the sampled Gaussian actor and the critic, the same kernel's MLP_OUT_SAMPLE / MLP_OUT_VALUE epilogues).
"""
import io
import json
import zipfile
from typing import NamedTuple

import numpy as np

ACTOR_KEYS = ("actor.latent_pi.0.weight", "actor.latent_pi.0.bias", "actor.latent_pi.2.weight",
              "actor.latent_pi.2.bias", "actor.mu.weight", "actor.mu.bias")
SHAPES = ((256, 38), (256,), (256, 256), (256,), (2, 256), (2,))


def load_sb3_actor(zip_path: str) -> dict:
    """Actor tensors of an SB3 SAC checkpoint (MlpPolicy, net_arch [256, 256])."""
    import torch
    with zipfile.ZipFile(zip_path) as z:
        sd = torch.load(io.BytesIO(z.read("policy.pth")), weights_only=True, map_location="cpu")
    missing = [k for k in ACTOR_KEYS if k not in sd]
    if missing:
        raise ValueError(f"{zip_path}: not an SB3 SAC MlpPolicy checkpoint (missing {missing})")
    return {k: sd[k].float().numpy() for k in ACTOR_KEYS}


def random_actor(seed: int = 0) -> dict:
    """Random-init actor of the reference architecture (PyTorch nn.Linear default init)."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, shp in zip(ACTOR_KEYS, SHAPES):
        fan_in = 38 if "latent_pi.0" in k else 256
        bound = 1.0 / np.sqrt(fan_in)
        out[k] = rng.uniform(-bound, bound, shp).astype(np.float32)
    return out


def actor_arrays(weights: dict):
    arrs = []
    for k, shp in zip(ACTOR_KEYS, SHAPES):
        a = np.ascontiguousarray(np.asarray(weights[k], np.float32))
        if a.shape != shp:
            raise ValueError(f"{k}: shape {a.shape}, expected {shp}")
        arrs.append(a)
    return arrs


# ------------------------------------------------------------------ per-car controllers (policy 4)
RELU, TANH = 0, 1                       # NascarMlp.activation
OUT_RAW, OUT_CLIP, OUT_SQUASH = 0, 1, 2  # NascarMlp.output
OUT_VALUE, OUT_SAMPLE = 3, 4            # a critic's value head / the sampled Gaussian actor (policy 6: ActorCritic)
MLP_SHAPES = ((256, 256), (256, 128), (256, 32), (128, 128), (64, 64), (32, 256))   # csrc/nascar_actor.h MLP_SHAPES
WIDE_SHAPES = ((512, 512),)             # csrc/nascar_actor.h MLP_WIDE_SHAPES (mlp_wide_kernel): ReLU only, no explorer head
OUT_CATEGORICAL, OUT_MODE = 6, 7        # the categorical actor of Discrete(5), sampled (DiscreteActorCritic) / its arg max
SAC_KEYS = ACTOR_KEYS
AC_KEYS = ("mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias", "mlp_extractor.policy_net.2.weight",
           "mlp_extractor.policy_net.2.bias", "action_net.weight", "action_net.bias")


class Controller(NamedTuple):
    """One MLP controller: PyTorch layouts w1 [h1, 38], b1 [h1], w2 [h2, h1], b2 [h2], w3 [2, h2], b3 [2] (float32).
    activation: RELU / TANH on both hidden layers.  output: OUT_RAW (mu = W3 h + b3), OUT_CLIP (np.clip(mu, -1, 1):
    SB3 predict for an unsquashed Box policy, PPO / A2C) or OUT_SQUASH (tanh(mu) then unscale_action: SAC).
    A five-row head (w3 [5, h2], b3 [5]: the logits of the env's Discrete(5)) takes OUT_CATEGORICAL (sampled: the actor of a
    DiscreteActorCritic) or OUT_MODE (the arg max, SB3's deterministic predict: a driver of the field).
    kind: "sac", "actor_critic" or "random"."""
    w1: np.ndarray
    b1: np.ndarray
    w2: np.ndarray
    b2: np.ndarray
    w3: np.ndarray
    b3: np.ndarray
    h1: int
    h2: int
    activation: int
    output: int
    kind: str

    @property
    def arrays(self):
        return (self.w1, self.b1, self.w2, self.b2, self.w3, self.b3)


def make_controller(arrays, activation: int, output: int, kind: str = "random") -> Controller:
    """A Controller from six arrays (PyTorch layouts), checked for a consistent 38 -> h1 -> h2 -> 2 shape.  Which
    (h1, h2) the device kernels hold is a separate question: BatchedCarEnv.check_controller / add_controller."""
    w1, b1, w2, b2, w3, b3 = [np.ascontiguousarray(np.asarray(a, np.float32)) for a in arrays]
    if w1.ndim != 2 or w2.ndim != 2 or w3.ndim != 2:
        raise ValueError("controller weights must be 2-D")
    h1, h2 = int(w1.shape[0]), int(w2.shape[0])
    rows = 5 if output in (OUT_CATEGORICAL, OUT_MODE) else 2        # the five logits of Discrete(5), or the two actions
    want = ((h1, 38), (h1,), (h2, h1), (h2,), (rows, h2), (rows,))
    got = tuple(a.shape for a in (w1, b1, w2, b2, w3, b3))
    if got != want:
        raise ValueError(f"controller shapes {got}, expected {want} (obs 38 -> h1 -> h2 -> " +
                         ("5 logits)" if rows == 5 else "2 actions)"))
    if activation not in (RELU, TANH) or output not in (OUT_RAW, OUT_CLIP, OUT_SQUASH, OUT_CATEGORICAL, OUT_MODE):
        raise ValueError(f"activation {activation} / output {output} unknown")
    return Controller(w1, b1, w2, b2, w3, b3, h1, h2, int(activation), int(output), kind)


def load_sb3_policy(zip_path: str) -> Controller:
    """The deterministic policy branch of an SB3 checkpoint zip, whichever of the reference's kinds it is
    (game/control/models/):
      * SAC (``actor.latent_pi.*`` + ``actor.mu.*``): ReLU, tanh-squashed -- SACController.control;
      * actor-critic, PPO / A2C (``mlp_extractor.policy_net.*`` + ``action_net.*``): the action is the Gaussian's
        mean clipped to the Box(-1, 1) (ActorCriticPolicy._predict + BasePolicy.predict's np.clip); the activation
        comes from the ``data`` JSON's ``policy_kwargs.activation_fn`` (a class name holding ReLU or Tanh; Tanh,
        SB3's default, when absent).  The value net and the optimizer are not read.
    ``policy.pth`` is read with torch.load(weights_only=True) and ``data`` as JSON whose ``:serialized:`` fields are
    ignored: nothing is unpickled.  The reference's A2C checkpoint was trained under VecNormalize, but
    A2CController.control (game/control/a2c_control_class.py:104-111) predicts on the raw observation; this restates
    what the controller does -- no normalisation.  Anything else raises ValueError."""
    import torch
    with zipfile.ZipFile(zip_path) as z:
        sd = torch.load(io.BytesIO(z.read("policy.pth")), weights_only=True, map_location="cpu")
        data = json.loads(z.read("data")) if "data" in z.namelist() else {}
    if all(k in sd for k in SAC_KEYS):
        keys, act, out, kind = SAC_KEYS, RELU, OUT_SQUASH, "sac"
    elif all(k in sd for k in AC_KEYS):
        kw = data.get("policy_kwargs") or {}
        fn = str(kw.get("activation_fn", "Tanh")) if isinstance(kw, dict) else "Tanh"
        if "ReLU" in fn:
            act = RELU
        elif "Tanh" in fn:
            act = TANH
        else:
            raise ValueError(f"{zip_path}: activation_fn {fn!r} is neither ReLU nor Tanh")
        keys, out, kind = AC_KEYS, OUT_CLIP, "actor_critic"
    else:
        raise ValueError(f"{zip_path}: neither an SB3 SAC actor (actor.latent_pi.* + actor.mu.*) nor an actor-critic "
                         f"policy (mlp_extractor.policy_net.* + action_net.*); keys: {sorted(sd)[:8]}")
    return make_controller([sd[k].float().numpy() for k in keys], act, out, kind)


def _sb3_activation(zip_path, data) -> int:
    kw = data.get("policy_kwargs") or {}
    fn = str(kw.get("activation_fn", "Tanh")) if isinstance(kw, dict) else "Tanh"
    if "ReLU" in fn:
        return RELU
    if "Tanh" in fn:
        return TANH
    raise ValueError(f"{zip_path}: activation_fn {fn!r} is neither ReLU nor Tanh")


# ------------------------------------------------------------------ the sampled actor-critic (policy 6, collect)
VF_KEYS = ("mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.0.bias", "mlp_extractor.value_net.2.weight",
           "mlp_extractor.value_net.2.bias", "value_net.weight", "value_net.bias")


class ValueNet(NamedTuple):
    """A critic 38 -> h1 -> h2 -> 1 in PyTorch layouts: w3 [1, h2], b3 [1]; `activation` on both hidden layers."""
    w1: np.ndarray
    b1: np.ndarray
    w2: np.ndarray
    b2: np.ndarray
    w3: np.ndarray
    b3: np.ndarray
    h1: int
    h2: int
    activation: int

    @property
    def arrays(self):
        return (self.w1, self.b1, self.w2, self.b2, self.w3, self.b3)

    output = OUT_VALUE


class ActorCritic(NamedTuple):
    """What SB3's on-policy algorithms (PPO, A2C) train: the Gaussian policy's mean net `pi` (a Controller with OUT_RAW),
    the critic `vf` and the state-independent `log_std` [2] (float32).  BatchedCarEnv.set_actor_critic / collect."""
    pi: Controller
    vf: ValueNet
    log_std: np.ndarray


def make_value_net(arrays, activation: int) -> ValueNet:
    """A ValueNet from six arrays (PyTorch layouts), checked for a 38 -> h1 -> h2 -> 1 shape the kernels hold: any other
    (h1, h2) raises, the message naming it."""
    w1, b1, w2, b2, w3, b3 = [np.ascontiguousarray(np.asarray(a, np.float32)) for a in arrays]
    if w1.ndim != 2 or w2.ndim != 2 or w3.ndim != 2:
        raise ValueError("value net weights must be 2-D")
    h1, h2 = int(w1.shape[0]), int(w2.shape[0])
    want = ((h1, 38), (h1,), (h2, h1), (h2,), (1, h2), (1,))
    got = tuple(a.shape for a in (w1, b1, w2, b2, w3, b3))
    if got != want:
        raise ValueError(f"value net shapes {got}, expected {want} (obs 38 -> h1 -> h2 -> 1 value)")
    if activation not in (RELU, TANH):
        raise ValueError(f"activation {activation} unknown")
    if (h1, h2) not in MLP_SHAPES and not ((h1, h2) in WIDE_SHAPES and activation == RELU):
        raise ValueError(f"value net shape 38 -> {h1} -> {h2} -> 1 ({'ReLU' if activation == RELU else 'Tanh'}) unsupported: "
                         f"the kernels hold hidden layers {', '.join('%d-%d' % s for s in MLP_SHAPES)}, and "
                         f"{', '.join('%d-%d' % s for s in WIDE_SHAPES)} with ReLU")
    return ValueNet(w1, b1, w2, b2, w3, b3, h1, h2, int(activation))


def make_actor_critic(pi_arrays, vf_arrays, activation: int, log_std, kind: str = "random") -> ActorCritic:
    ls = np.ascontiguousarray(np.asarray(log_std, np.float32))
    if ls.shape != (2,) or not np.all(np.isfinite(ls)):
        raise ValueError(f"log_std must be 2 finite values, got {ls!r}")
    return ActorCritic(make_controller(pi_arrays, activation, OUT_RAW, kind), make_value_net(vf_arrays, activation), ls)


def load_sb3_actor_critic(zip_path: str) -> ActorCritic:
    """Policy net, value net and log_std of an SB3 PPO / A2C checkpoint zip (ActorCriticPolicy with an MlpExtractor of
    two hidden layers per branch: ``mlp_extractor.policy_net.*`` + ``action_net.*``, ``mlp_extractor.value_net.{0,2}.*`` +
    ``value_net.*``, ``log_std``); the activation as load_sb3_policy reads it.  ``policy.pth`` is read with
    torch.load(weights_only=True): nothing is unpickled; the optimizer is not read.  A SAC zip, or anything else without
    these tensors, raises ValueError, as does a value net of a shape the kernels do not hold."""
    import torch
    with zipfile.ZipFile(zip_path) as z:
        sd = torch.load(io.BytesIO(z.read("policy.pth")), weights_only=True, map_location="cpu")
        data = json.loads(z.read("data")) if "data" in z.namelist() else {}
    missing = [k for k in AC_KEYS + VF_KEYS + ("log_std",) if k not in sd]
    if missing:
        what = "an SB3 SAC checkpoint (no value net, no log_std)" if all(k in sd for k in SAC_KEYS) else "no actor-critic"
        if missing == ["log_std"] and tuple(sd["action_net.weight"].shape)[:1] == (5,):
            what = "a Discrete(5) policy (no log_std) -- use load_sb3_discrete_actor_critic"
        raise ValueError(f"{zip_path}: {what}: missing {missing[:4]}")
    act = _sb3_activation(zip_path, data)
    return make_actor_critic([sd[k].float().numpy() for k in AC_KEYS], [sd[k].float().numpy() for k in VF_KEYS], act,
                             sd["log_std"].float().numpy(), "actor_critic")


def random_actor_critic(h1: int, h2: int, activation: int = TANH, log_std=(0.0, 0.0), seed: int = 0,
                        vf_shape=None, vf_activation=None) -> ActorCritic:
    """Random-init actor-critic (PyTorch nn.Linear default init): pi 38 -> h1 -> h2 -> 2, vf 38 -> h1 -> h2 -> 1, or
    `vf_shape` = (h1, h2) / `vf_activation` for a critic of another shape (it then runs in a launch of its own)."""
    pi = random_mlp(h1, h2, activation, OUT_RAW, seed)
    v1, v2 = vf_shape or (h1, h2)
    rng = np.random.default_rng(seed + 7919)
    arrs = []
    for shp, fan_in in (((v1, 38), 38), ((v1,), 38), ((v2, v1), v1), ((v2,), v1), ((1, v2), v2), ((1,), v2)):
        bound = 1.0 / np.sqrt(fan_in)
        arrs.append(rng.uniform(-bound, bound, shp).astype(np.float32))
    ls = np.ascontiguousarray(np.asarray(log_std, np.float32))
    return ActorCritic(pi, make_value_net(arrs, activation if vf_activation is None else vf_activation), ls)


def actor_critic_numpy(ac: ActorCritic, obs, dtype=np.float64):
    """Host restatement of the actor-critic's forward in `dtype` arithmetic: (mu [n, 2], value [n])."""
    dt = np.dtype(dtype).type
    mu = mlp_forward_numpy(ac.pi, obs, dtype, output=OUT_RAW)
    f = (lambda v: np.maximum(v, dt(0))) if ac.vf.activation == RELU else np.tanh
    x = np.asarray(obs, dtype=dt).reshape(-1, 38)
    w1, b1, w2, b2, w3, b3 = [a.astype(dt) for a in ac.vf.arrays]
    h = f(x @ w1.T + b1)
    h = f(h @ w2.T + b2)
    return mu, (h @ w3.T + b3)[:, 0]


def random_mlp(h1: int, h2: int, activation: int = RELU, output: int = OUT_RAW, seed: int = 0) -> Controller:
    """Random-init controller 38 -> h1 -> h2 -> 2 (PyTorch nn.Linear default init)."""
    rng = np.random.default_rng(seed)
    arrs = []
    for shp, fan_in in (((h1, 38), 38), ((h1,), 38), ((h2, h1), h1), ((h2,), h1), ((2, h2), h2), ((2,), h2)):
        bound = 1.0 / np.sqrt(fan_in)
        arrs.append(rng.uniform(-bound, bound, shp).astype(np.float32))
    return make_controller(arrs, activation, output, "random")


def mlp_forward_numpy(ctrl: Controller, obs, dtype=np.float64, output=None):
    """Host restatement of a controller's forward in `dtype` arithmetic (`output`: override ctrl.output).  OUT_SQUASH
    ends with BasePolicy.unscale_action for the Box(-1, 1): low + 0.5 * (a + 1) * (high - low)."""
    dt = np.dtype(dtype).type
    f = (lambda v: np.maximum(v, dt(0))) if ctrl.activation == RELU else np.tanh
    x = np.asarray(obs, dtype=dt).reshape(-1, 38)
    w1, b1, w2, b2, w3, b3 = [a.astype(dt) for a in ctrl.arrays]
    h = f(x @ w1.T + b1)
    h = f(h @ w2.T + b2)
    mu = h @ w3.T + b3
    out = ctrl.output if output is None else output
    if out == OUT_CLIP:
        return np.clip(mu, dt(-1), dt(1))
    if out == OUT_SQUASH:
        return dt(-1) + (dt(0.5) * (np.tanh(mu) + dt(1))) * dt(2)
    return mu


# ------------------------------------------------------------------ the sampled SAC actor (policy 7, collect_transitions)
OUT_SQUASH_SAMPLE = 5                    # NascarMlp.output: SB3's SAC Actor with deterministic=False (act_dim 4)
LOG_STD_KEYS = ("actor.log_std.weight", "actor.log_std.bias")
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0    # stable_baselines3/sac/policies.py


class SquashedActor(NamedTuple):
    """SB3's SAC actor with its log_std head: a Controller whose w3 is [4, h2] -- rows 0-1 actor.mu.weight, rows 2-3
    actor.log_std.weight -- and b3 [4] likewise.  output is OUT_SQUASH_SAMPLE: a = tanh(mu + exp(clip(log_std, -20, 2)) *
    eps), then unscale_action; BatchedCarEnv.set_explorer / collect_transitions."""
    w1: np.ndarray
    b1: np.ndarray
    w2: np.ndarray
    b2: np.ndarray
    w3: np.ndarray
    b3: np.ndarray
    h1: int
    h2: int
    activation: int
    kind: str = "sac"

    output = OUT_SQUASH_SAMPLE

    @property
    def arrays(self):
        return (self.w1, self.b1, self.w2, self.b2, self.w3, self.b3)

    def deterministic(self) -> Controller:
        """the mean branch alone: the OUT_SQUASH Controller load_sb3_policy reads from the same checkpoint"""
        return Controller(self.w1, self.b1, self.w2, self.b2, np.ascontiguousarray(self.w3[:2]),
                          np.ascontiguousarray(self.b3[:2]), self.h1, self.h2, self.activation, OUT_SQUASH, self.kind)


def make_squashed_actor(arrays, activation: int = RELU, kind: str = "random") -> SquashedActor:
    """A SquashedActor from six arrays (PyTorch layouts; w3 [4, h2], b3 [4]), checked for a 38 -> h1 -> h2 -> 4 shape."""
    w1, b1, w2, b2, w3, b3 = [np.ascontiguousarray(np.asarray(a, np.float32)) for a in arrays]
    if w1.ndim != 2 or w2.ndim != 2 or w3.ndim != 2:
        raise ValueError("squashed actor weights must be 2-D")
    h1, h2 = int(w1.shape[0]), int(w2.shape[0])
    want = ((h1, 38), (h1,), (h2, h1), (h2,), (4, h2), (4,))
    got = tuple(a.shape for a in (w1, b1, w2, b2, w3, b3))
    if got != want:
        raise ValueError(f"squashed actor shapes {got}, expected {want} (obs 38 -> h1 -> h2 -> mu [2] + log_std [2])")
    if activation not in (RELU, TANH):
        raise ValueError(f"activation {activation} unknown")
    return SquashedActor(w1, b1, w2, b2, w3, b3, h1, h2, int(activation), kind)


def load_sb3_sac_actor(zip_path: str) -> SquashedActor:
    """The stochastic actor of an SB3 SAC checkpoint zip: ``actor.latent_pi.*``, ``actor.mu.*`` and ``actor.log_std.*``
    (the head load_sb3_actor leaves out), ReLU as SAC's MlpPolicy.  ``policy.pth`` is read with
    torch.load(weights_only=True): nothing is unpickled.  A ``use_sde`` checkpoint (its log_std is a [h2, 2] parameter,
    not a layer) and an actor-critic (PPO / A2C) zip raise ValueError."""
    import torch
    with zipfile.ZipFile(zip_path) as z:
        sd = torch.load(io.BytesIO(z.read("policy.pth")), weights_only=True, map_location="cpu")
    if "actor.log_std" in sd or any(k.startswith("actor.") and "sde" in k for k in sd):
        raise ValueError(f"{zip_path}: a use_sde SAC checkpoint (state-dependent exploration) is not supported")
    missing = [k for k in SAC_KEYS + LOG_STD_KEYS if k not in sd]
    if missing:
        what = ("an actor-critic (PPO / A2C) checkpoint, no SAC actor" if all(k in sd for k in AC_KEYS)
                else "no SB3 SAC MlpPolicy checkpoint")
        raise ValueError(f"{zip_path}: {what}: missing {missing[:4]}")
    a = [sd[k].float().numpy() for k in SAC_KEYS]
    lw, lb = [sd[k].float().numpy() for k in LOG_STD_KEYS]
    return make_squashed_actor(a[:4] + [np.concatenate([a[4], lw]), np.concatenate([a[5], lb])], RELU, "sac")


def random_squashed_actor(h1: int, h2: int, seed: int = 0, activation: int = RELU) -> SquashedActor:
    """Random-init squashed actor 38 -> h1 -> h2 -> mu [2] + log_std [2] (PyTorch nn.Linear default init)."""
    rng = np.random.default_rng(seed)
    arrs = []
    for shp, fan_in in (((h1, 38), 38), ((h1,), 38), ((h2, h1), h1), ((h2,), h1), ((4, h2), h2), ((4,), h2)):
        bound = 1.0 / np.sqrt(fan_in)
        arrs.append(rng.uniform(-bound, bound, shp).astype(np.float32))
    return make_squashed_actor(arrs, activation, "random")


def squashed_actor_numpy(actor: SquashedActor, obs, eps, dtype=np.float64):
    """Host restatement of the sampled SAC actor in `dtype` arithmetic on obs [n, 38] and standard normal pairs eps
    [n, 2]: (u, s) -- u = unscale_action(tanh(mu + exp(clip(log_std, -20, 2)) * eps)) steps the env, s = scale_action(u)
    is what the replay buffer keeps."""
    dt = np.dtype(dtype).type
    f = (lambda v: np.maximum(v, dt(0))) if actor.activation == RELU else np.tanh
    x = np.asarray(obs, dtype=dt).reshape(-1, 38)
    w1, b1, w2, b2, w3, b3 = [a.astype(dt) for a in actor.arrays]
    h = f(x @ w1.T + b1)
    h = f(h @ w2.T + b2)
    out = h @ w3.T + b3
    mu, ls = out[:, :2], np.clip(out[:, 2:], dt(LOG_STD_MIN), dt(LOG_STD_MAX))
    t = np.tanh(mu + np.exp(ls) * np.asarray(eps, dt))
    u = dt(-1) + (dt(0.5) * (t + dt(1))) * dt(2)
    return u, dt(2) * ((u + dt(1)) / dt(2)) - dt(1)


# ------------------------------------------------------------------ the categorical actor-critic (policy 6 for Discrete(5))
N_DISCRETE = 5
# CarEnv(discrete_action_space=True): action index -> (throttle / brake, steering), BaseEnv._discrete_to_continuous
DISCRETE_PAIRS = np.array([[0, 0], [1, 0], [-1, 0], [0, -1], [0, 1]], np.float32)


class DiscreteActorCritic(NamedTuple):
    """What SB3's on-policy algorithms train on CarEnv(discrete_action_space=True) (learn/a2c.py): the categorical policy's
    logit net `pi` (a five-row Controller with OUT_CATEGORICAL) and the critic `vf`; a Discrete(5) policy has no log_std.
    BatchedCarEnv.set_actor_critic / collect take it like an ActorCritic."""
    pi: Controller
    vf: ValueNet

    def deterministic(self) -> Controller:
        """the arg-max driver (SB3's predict(deterministic=True)): an OUT_MODE Controller for add_controller /
        set_car_controllers"""
        return self.pi._replace(output=OUT_MODE)


def make_discrete_actor_critic(pi_arrays, vf_arrays, activation: int, kind: str = "random", vf_activation=None) -> DiscreteActorCritic:
    """A DiscreteActorCritic from the six arrays of each net (PyTorch layouts; the policy head w3 [5, h2], b3 [5])."""
    return DiscreteActorCritic(make_controller(pi_arrays, activation, OUT_CATEGORICAL, kind),
                               make_value_net(vf_arrays, activation if vf_activation is None else vf_activation))


def load_sb3_discrete_actor_critic(zip_path: str) -> DiscreteActorCritic:
    """Policy net and value net of an SB3 PPO / A2C checkpoint zip trained on a Discrete(5) action space: the keys of
    load_sb3_actor_critic without ``log_std``, ``action_net.weight`` [5, h2].  A Box checkpoint (a [2, h2] head) raises
    ValueError naming load_sb3_actor_critic.  ``policy.pth`` is read with torch.load(weights_only=True): nothing is
    unpickled; the optimizer is not read."""
    import torch
    with zipfile.ZipFile(zip_path) as z:
        sd = torch.load(io.BytesIO(z.read("policy.pth")), weights_only=True, map_location="cpu")
        data = json.loads(z.read("data")) if "data" in z.namelist() else {}
    missing = [k for k in AC_KEYS + VF_KEYS if k not in sd]
    if missing:
        what = "an SB3 SAC checkpoint (no value net)" if all(k in sd for k in SAC_KEYS) else "no actor-critic"
        raise ValueError(f"{zip_path}: {what}: missing {missing[:4]}")
    head = tuple(sd["action_net.weight"].shape)
    if len(head) != 2 or head[0] != N_DISCRETE:
        raise ValueError(f"{zip_path}: action_net.weight is {list(head)}, not [5, h2]: " +
                         ("a Box(-1, 1)^2 policy -- use load_sb3_actor_critic" if head[:1] == (2,) else
                          "no Discrete(5) policy"))
    act = _sb3_activation(zip_path, data)
    return make_discrete_actor_critic([sd[k].float().numpy() for k in AC_KEYS], [sd[k].float().numpy() for k in VF_KEYS], act,
                                      "actor_critic")


def random_discrete_actor_critic(h1: int, h2: int, activation: int = TANH, seed: int = 0, vf_shape=None,
                                 vf_activation=None) -> DiscreteActorCritic:
    """Random-init categorical actor-critic (PyTorch nn.Linear default init): pi 38 -> h1 -> h2 -> 5, vf 38 -> h1 -> h2 -> 1,
    or `vf_shape` = (h1, h2) / `vf_activation` for a critic of another shape (it then runs in a launch of its own)."""
    def nets(rng, dims):
        out = []
        for shp, fan_in in dims:
            bound = 1.0 / np.sqrt(fan_in)
            out.append(rng.uniform(-bound, bound, shp).astype(np.float32))
        return out
    pi = nets(np.random.default_rng(seed), (((h1, 38), 38), ((h1,), 38), ((h2, h1), h1), ((h2,), h1),
                                            ((N_DISCRETE, h2), h2), ((N_DISCRETE,), h2)))
    v1, v2 = vf_shape or (h1, h2)
    vf = nets(np.random.default_rng(seed + 7919), (((v1, 38), 38), ((v1,), 38), ((v2, v1), v1), ((v2,), v1), ((1, v2), v2),
                                                   ((1,), v2)))
    return make_discrete_actor_critic(pi, vf, activation, "random", vf_activation)


def discrete_actor_critic_numpy(ac: DiscreteActorCritic, obs, dtype=np.float64):
    """Host restatement of the categorical actor-critic's forward in `dtype` arithmetic: (logits [n, 5], value [n])."""
    dt = np.dtype(dtype).type
    x = np.asarray(obs, dtype=dt).reshape(-1, 38)
    out = []
    for net in (ac.pi, ac.vf):
        f = (lambda v: np.maximum(v, dt(0))) if net.activation == RELU else np.tanh
        w1, b1, w2, b2, w3, b3 = [a.astype(dt) for a in net.arrays]
        h = f(x @ w1.T + b1)
        h = f(h @ w2.T + b2)
        out.append(h @ w3.T + b3)
    return out[0], out[1][:, 0]

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
SAC_KEYS = ACTOR_KEYS
AC_KEYS = ("mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias", "mlp_extractor.policy_net.2.weight",
           "mlp_extractor.policy_net.2.bias", "action_net.weight", "action_net.bias")


class Controller(NamedTuple):
    """One MLP controller: PyTorch layouts w1 [h1, 38], b1 [h1], w2 [h2, h1], b2 [h2], w3 [2, h2], b3 [2] (float32).
    activation: RELU / TANH on both hidden layers.  output: OUT_RAW (mu = W3 h + b3), OUT_CLIP (np.clip(mu, -1, 1):
    SB3 predict for an unsquashed Box policy, PPO / A2C) or OUT_SQUASH (tanh(mu) then unscale_action: SAC).
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
    want = ((h1, 38), (h1,), (h2, h1), (h2,), (2, h2), (2,))
    got = tuple(a.shape for a in (w1, b1, w2, b2, w3, b3))
    if got != want:
        raise ValueError(f"controller shapes {got}, expected {want} (obs 38 -> h1 -> h2 -> 2 actions)")
    if activation not in (RELU, TANH) or output not in (OUT_RAW, OUT_CLIP, OUT_SQUASH):
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

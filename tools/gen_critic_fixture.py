"""Fixture for the sampled actor-critic (policy 6): the value net and log_std of the reference's PPO checkpoint
(game/control/models/ppo_849.zip) plus its values on the 2236 observations already stored as `obs` in
tests/golden/sac_1235_actor.npz (not stored again); the policy branch is tests/golden/ppo_849_actor.npz.
TEST INFRASTRUCTURE: runs only where the reference checkout exists; the npz file travels, the reference does not.

The zip is read by nascargymnasium_amd.policy.load_sb3_actor_critic (zipfile + torch.load(weights_only=True) + JSON):
nothing in it is executed, stable_baselines3 is not needed.  ActorCriticPolicy.predict_values is
mlp_extractor.value_net (Linear-act-Linear-act) followed by value_net (Linear), restated here in PyTorch once in float64
(`value_f64`) and once in float32 (`value_f32`).

    python tools/gen_critic_fixture.py --ref REFERENCE_CHECKOUT   ->  tests/golden/ppo_849_critic.npz
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_value(vf, obs, dtype):
    import torch
    from nascargymnasium_amd.policy import RELU
    act = torch.relu if vf.activation == RELU else torch.tanh
    w1, b1, w2, b2, w3, b3 = [torch.from_numpy(a).to(dtype) for a in vf.arrays]
    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(obs, np.float32)).to(dtype)
        h = act(torch.nn.functional.linear(x, w1, b1))
        h = act(torch.nn.functional.linear(h, w2, b2))
        return torch.nn.functional.linear(h, w3, b3).numpy()[:, 0]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a checkout of the reference project")
    a = ap.parse_args()
    if not os.path.isdir(a.ref):
        sys.exit(f"{a.ref}: no reference checkout here (the committed fixture under tests/golden is its output)")
    from nascargymnasium_amd.policy import load_sb3_actor_critic
    gold = os.path.join(ROOT, "tests", "golden")
    obs = np.load(os.path.join(gold, "sac_1235_actor.npz"))["obs"]
    ac = load_sb3_actor_critic(os.path.join(a.ref, "game", "control", "models", "ppo_849.zip"))
    pi = np.load(os.path.join(gold, "ppo_849_actor.npz"))
    assert all(np.array_equal(pi[k], v) for k, v in zip(("w1", "b1", "w2", "b2", "w3", "b3"), ac.pi.arrays))
    v = ac.vf
    v64, v32 = torch_value(v, obs, torch.float64), torch_value(v, obs, torch.float32)
    out = os.path.join(gold, "ppo_849_critic.npz")
    np.savez_compressed(out, w1=v.w1, b1=v.b1, w2=v.w2, b2=v.b2, w3=v.w3, b3=v.b3, h1=np.int32(v.h1), h2=np.int32(v.h2),
                        activation=np.int32(v.activation), log_std=ac.log_std, value_f64=v64, value_f32=v32)
    print(out, os.path.getsize(out), "bytes; h", v.h1, v.h2, "act", v.activation, "log_std", ac.log_std, "value range",
          v64.min(), v64.max(), "max |f32 - f64|", np.abs(v32 - v64).max())


if __name__ == "__main__":
    main()

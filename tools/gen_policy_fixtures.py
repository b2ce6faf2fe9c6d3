"""Fixtures for the per-car controllers (policy 4): the policy branch of the reference's PPO and A2C checkpoints
(game/control/models/ppo_849.zip, a2c_best_model3.zip) plus their pre-clip action means on the 2236 observations
already stored as `obs` in tests/golden/sac_1235_actor.npz (not stored again).
TEST INFRASTRUCTURE: runs only where the reference checkout exists; the npz files travel, the reference does not.

The zips are opened with zipfile, policy.pth with torch.load(weights_only=True) and `data` as JSON
(nascargymnasium_amd.policy.load_sb3_policy) -- nothing in them is executed.  stable_baselines3 is not needed:
ActorCriticPolicy._predict(deterministic=True) is mlp_extractor.policy_net (Linear-act-Linear-act) followed by
action_net (Linear), the Gaussian's mean; BasePolicy.predict then clips it to the Box(-1, 1).  That mean is restated
here in PyTorch, once in float64 (`mean_f64`) and once in float32 (`mean_f32`).  The value net, log_std and the
optimizer state are left out.

    python tools/gen_policy_fixtures.py [--ref REFERENCE_CHECKOUT]
        ->  tests/golden/ppo_849_actor.npz, tests/golden/a2c_best_model3_actor.npz
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_mean(ctrl, obs, dtype):
    import torch
    from nascargymnasium_amd.policy import RELU
    act = torch.relu if ctrl.activation == RELU else torch.tanh
    w1, b1, w2, b2, w3, b3 = [torch.from_numpy(a).to(dtype) for a in ctrl.arrays]
    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(obs, np.float32)).to(dtype)
        h = act(torch.nn.functional.linear(x, w1, b1))
        h = act(torch.nn.functional.linear(h, w2, b2))
        return torch.nn.functional.linear(h, w3, b3).numpy()


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    if not os.path.isdir(a.ref):
        sys.exit(f"{a.ref}: no reference checkout here (the committed fixtures under tests/golden are its output)")
    from nascargymnasium_amd.policy import load_sb3_policy
    gold = os.path.join(ROOT, "tests", "golden")
    obs = np.load(os.path.join(gold, "sac_1235_actor.npz"))["obs"]
    for name in ("ppo_849", "a2c_best_model3"):
        c = load_sb3_policy(os.path.join(a.ref, "game", "control", "models", name + ".zip"))
        m64 = torch_mean(c, obs, torch.float64)
        m32 = torch_mean(c, obs, torch.float32)
        out = os.path.join(gold, name + "_actor.npz")
        np.savez_compressed(out, w1=c.w1, b1=c.b1, w2=c.w2, b2=c.b2, w3=c.w3, b3=c.b3, h1=np.int32(c.h1),
                            h2=np.int32(c.h2), activation=np.int32(c.activation), output=np.int32(c.output),
                            mean_f64=m64, mean_f32=m32)
        print(out, os.path.getsize(out), "bytes; h", c.h1, c.h2, "act", c.activation, "mean range", m64.min(), m64.max(),
              "max |f32 - f64|", np.abs(m32 - m64).max(), "inside (-1, 1):", (np.abs(m64) < 1).mean(0))


if __name__ == "__main__":
    main()

"""Fixture for the sampled SAC actor (policy 7): the log_std head of the reference's SAC checkpoint
(game/control/models/sac_1235.zip), ``actor.log_std.weight`` [2, 256] and ``actor.log_std.bias`` [2].  The rest of the
actor is already stored in tests/golden/sac_1235_actor.npz (not stored again).
TEST INFRASTRUCTURE: runs only where the reference checkout exists; the npz file travels, the reference does not.

The zip is read by nascargymnasium_amd.policy.load_sb3_sac_actor (zipfile + torch.load(weights_only=True)): nothing in it
is executed, stable_baselines3 is not needed.

    python tools/gen_sac_head_fixture.py --ref REFERENCE_CHECKOUT   ->  tests/golden/sac_1235_log_std.npz
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a checkout of the reference project")
    a = ap.parse_args()
    if not os.path.isdir(a.ref):
        sys.exit(f"{a.ref}: no reference checkout here (the committed fixture under tests/golden is its output)")
    from nascargymnasium_amd.policy import ACTOR_KEYS, load_sb3_sac_actor
    gold = os.path.join(ROOT, "tests", "golden")
    act = load_sb3_sac_actor(os.path.join(a.ref, "game", "control", "models", "sac_1235.zip"))
    d = np.load(os.path.join(gold, "sac_1235_actor.npz"))
    stored = [d[k.replace(".", "__")] for k in ACTOR_KEYS]
    mean = (act.w1, act.b1, act.w2, act.b2, act.w3[:2], act.b3[:2])
    assert all(np.array_equal(x, y) for x, y in zip(stored, mean)), "the stored actor is not this checkpoint's"
    out = os.path.join(gold, "sac_1235_log_std.npz")
    np.savez_compressed(out, weight=act.w3[2:], bias=act.b3[2:])
    print(out, os.path.getsize(out), "bytes; log_std.weight", act.w3[2:].shape, "bias", act.b3[2:])


if __name__ == "__main__":
    main()

"""Time one step's action computation and the closed-loop rollout for the per-car controllers (policy 4) against the
single SAC actor (policy 2, float32), from a saved steady state:  python tools/field_bench.py [--envs 8192] [--cars 10]
[--track daytona] [--out FILE.json] [--tag NAME]

  policy2_fp32   nascar_policy_actions(2): sac_1235 through set_actor(precision="fp32")
  field_sac      policy 4, every slot the same sac_1235 controller
  field_mixed    policy 4, 4 x SAC, 2 x PPO (ppo_849), 2 x A2C (a2c_best_model3), 2 x rule (needs 10 cars)
Launches go straight through the C ABI on preallocated buffers; each figure is the median of --rounds windows of --iters
launches (HIP events), the variants alternating inside every round.  A library without the controller entry points
(--root pointing at an older checkout) measures policy2_fp32 only.  The weights are the committed fixtures under
tests/golden (the reference's own checkpoints)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --root DIR: import the package (and its built library) from another checkout, e.g. the parent commit's for an A/B
PKG_ROOT = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else ROOT
sys.path.insert(0, PKG_ROOT)
from nascargymnasium_amd import policy as P  # noqa: E402
from nascargymnasium_amd.batched import BatchedCarEnv  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def fixture(name):
    d = np.load(os.path.join(GOLD, name + "_actor.npz"))
    return P.make_controller([d[k] for k in ("w1", "b1", "w2", "b2", "w3", "b3")], int(d["activation"]), int(d["output"]))


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters      # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--cars", type=int, default=10)
    ap.add_argument("--track", default="daytona")
    ap.add_argument("--warm", type=int, default=600, help="noisy-rule-driver steps before the state is saved")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rollout-steps", type=int, default=300)
    ap.add_argument("--root", default=ROOT, help="checkout to import nascargymnasium_amd from")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    E, C = a.envs, a.cars
    env = BatchedCarEnv(E, C, a.track, device="cuda:0")
    d = np.load(os.path.join(GOLD, "sac_1235_actor.npz"))
    w = {k: d[k.replace(".", "__")] for k in P.ACTOR_KEYS}
    env.set_actor(w, precision="fp32")
    have_field = hasattr(env, "add_controller")
    env.reset()
    env.rollout(3, a.warm, seed=1, step0=0, auto_reset=True)
    state, obs0 = env.get_state(), env.obs.clone()
    fields = {}
    if have_field:
        sac = env.add_controller(P.make_controller([w[k] for k in P.ACTOR_KEYS], P.RELU, P.OUT_SQUASH, "sac"))
        fields["field_sac"] = [sac] * C
        if C == 10:
            ppo, a2c = env.add_controller(fixture("ppo_849")), env.add_controller(fixture("a2c_best_model3"))
            fields["field_mixed"] = [sac] * 4 + [ppo] * 2 + [a2c] * 2 + ["rule"] * 2
    L, h = env.L, env.h
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    po, pa = ctypes.c_void_p(env.obs.data_ptr()), ctypes.c_void_p(env._actions.data_ptr())

    def actions(policy):
        return lambda: L.nascar_policy_actions(h, policy, 0, 0, po, pa, st)

    variants = [("policy2_fp32", 2, None)] + [(k, 4, v) for k, v in fields.items()]
    act_us = {k: [] for k, _, _ in variants}
    for r in range(a.rounds + 1):                 # round 0 warms every shape up
        for name, pol, field in variants:
            if field is not None:
                env.set_car_controllers(field)
            us = timed(actions(pol), a.iters if r else 20)
            if r:
                act_us[name].append(us)
    ro = {k: [] for k, _, _ in variants}
    K = a.rollout_steps
    for r in range(4):
        for name, pol, field in variants:
            if field is not None:
                env.set_car_controllers(field)
            env.set_state(state); env.obs.copy_(obs0)
            torch.cuda.synchronize()
            us = timed(lambda: env.rollout(pol, K if r else 20, seed=2, step0=a.warm, auto_reset=True), 1)
            if r:
                ro[name].append(E * C * K / (us * 1e-6))
    res = {"tag": a.tag, "root": os.path.relpath(os.path.abspath(a.root), ROOT), "envs": E, "cars": C,
           "track": a.track, "warm_steps": a.warm, "iters": a.iters, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0),
           "action_us": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in act_us.items()},
           "rollout_steps": K, "rollout_streams": env.rollout_streams,
           "rollout_car_steps_per_s": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ro.items()}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    env.close()


if __name__ == "__main__":
    main()

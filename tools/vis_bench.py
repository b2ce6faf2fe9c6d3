"""Cost of the opponent-aware sensors (nascar_set_car_visibility), from a saved steady state:
  python tools/vis_bench.py [--envs 8192] [--cars 10] [--track talladega] [--contact] [--root DIR] [--tag NAME] [--out FILE.json]

Per variant (switch off; switch on where the library has it) the figures are medians of --rounds windows, the variants
alternating inside every round and every window starting from the same saved state and observation:
  sensor_us    the sensor launch of a whole-grid step (nascar_step_driven, policy 3, auto-reset: pass A + pass B),
               between the step events after the logic and after the sensor launch; median over a window's steps
  step_us      the whole step of the same launches (first to last step event)
  rollout_us   per step of a sharded nascar_rollout of --rollout-steps steps (the schedule bench.py times)
A library without the entry point (--root pointing at the parent commit's checkout) measures `off` only: run the two
checkouts alternately in one session and compare their `off` figures with the spread each shows against itself."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_ROOT = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else ROOT
sys.path.insert(0, os.path.abspath(PKG_ROOT))
from nascargymnasium_amd.batched import BatchedCarEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--cars", type=int, default=10)
    ap.add_argument("--track", default="talladega")
    ap.add_argument("--contact", action="store_true", help="car-car contact on (cfg3)")
    ap.add_argument("--warm", type=int, default=1200, help="noisy-rule-driver steps before the state is saved")
    ap.add_argument("--steps", type=int, default=100, help="steps per window")
    ap.add_argument("--rollout-steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--root", default=ROOT, help="checkout to import nascargymnasium_amd from")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    E, C = a.envs, a.cars
    env = BatchedCarEnv(E, C, a.track, device="cuda:0")
    if a.contact:
        env.set_car_contact(True)
    have = hasattr(env, "set_car_visibility")
    env.reset()
    env.rollout(3, a.warm, seed=1, step0=0, auto_reset=True)     # the steady state is the walls-only one for every variant
    state, obs0 = env.get_state(), env.obs.clone()
    variants = ["off"] + (["on"] if have else [])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    res = {v: {"sensor_us": [], "step_us": [], "rollout_us": []} for v in variants}

    def restore(v):
        if have:
            env.set_car_visibility(v == "on")
        env.set_state(state)
        env.obs.copy_(obs0)
        torch.cuda.synchronize()

    for r in range(a.rounds + 1):                 # round 0 warms up
        for v in variants:
            restore(v)
            env.set_step_events(ev)
            sens, step = [], []
            for k in range(a.steps if r else 10):
                env.step_driven(3, seed=2, step=a.warm + k, auto_reset=True)
                torch.cuda.synchronize()
                sens.append(ev[2].elapsed_time(ev[3]) * 1e3)
                step.append(ev[0].elapsed_time(ev[3]) * 1e3)
            env.set_step_events(None)
            restore(v)
            K = a.rollout_steps if r else 20
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            env.rollout(3, K, seed=2, step0=a.warm, auto_reset=True)
            e.record()
            torch.cuda.synchronize()
            if r:
                res[v]["sensor_us"].append(statistics.median(sens))
                res[v]["step_us"].append(statistics.median(step))
                res[v]["rollout_us"].append(s.elapsed_time(e) * 1e3 / K)
    summ = {v: {k: {"median": statistics.median(x), "min": min(x), "max": max(x)} for k, x in d.items()}
            for v, d in res.items()}
    out = {"tag": a.tag, "root": os.path.relpath(os.path.abspath(a.root), ROOT), "envs": E, "cars": C, "track": a.track,
           "car_contact": bool(a.contact), "warm_steps": a.warm, "steps": a.steps, "rollout_steps": a.rollout_steps,
           "rounds": a.rounds, "rollout_streams": env.rollout_streams, "device": torch.cuda.get_device_name(0),
           "variants": summ}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    env.close()


if __name__ == "__main__":
    main()

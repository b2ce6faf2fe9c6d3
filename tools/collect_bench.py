"""Time the on-policy collection against what a learner had before it, from a saved steady state:

    python tools/collect_bench.py [--parent DIR] [--shapes 8192x1,8192x10] [--steps 128] [--rounds 7] [--out FILE.json]

Per shape (daytona, E envs x C cars; 8192 x 1 is learn/ppo.py's) the driver starts one child process per measurement
window, alternating the parent commit's checkout (--parent: a built checkout of the commit before the collection, which
runs the rollout4 leg only) with this tree's, --rounds times each, and reports the medians.  Legs (ms per env step):

  rollout4      rollout(4, K, trajectory=True, obs_trajectory=True), the ppo_849 policy net clipped in every car slot:
                what the device could run before (no sampling, no values)                              [parent and new]
  collect       collect(K): sampled actor + critic in one launch, timeout values, values[K], GAE        [new]
  forward_1x / forward_2x   the policy net's forward on the E * C rows and on twice as many rows: the like-for-like
                cost of a second net slot in the launch (us per launch)                                 [new]
  vec_env       K x VecCarEnv.step (return_tensors) with the PyTorch forward and sample of ActorCriticNet in between:
                the path a learner has without collect                                                  [new]
  gae / gae_torch   gae() at K = 128 against the same reverse loop in PyTorch ops on the device (us)    [new]

Each child warms up with --warm noisy-rule-driver steps from reset, saves that state, runs each leg once untimed and
once timed from the saved state (HIP events around the whole window).  The weights are the committed fixtures under
tests/golden."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
KEYS = ("w1", "b1", "w2", "b2", "w3", "b3")


def child(a):
    sys.path.insert(0, a.root)
    import numpy as np
    import torch
    from nascargymnasium_amd import policy as P
    from nascargymnasium_amd.batched import BatchedCarEnv
    E, C, K = a.envs, a.cars, a.steps
    pi = np.load(os.path.join(GOLD, "ppo_849_actor.npz"))
    env = BatchedCarEnv(E, C, "daytona", device="cuda:0")
    env.reset()
    env.rollout(3, a.warm, seed=1, step0=0, auto_reset=True)
    state, obs0 = env.get_state(), env.obs.clone()

    def window(fn):
        out = None
        for timed in (False, True):
            env.set_state(state); env.obs.copy_(obs0)
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            out = s.elapsed_time(e)
        return out                                                     # ms per window

    res = {}
    clip = env.add_controller(P.make_controller([pi[k] for k in KEYS], int(pi["activation"]), P.OUT_CLIP))
    env.set_car_controllers([clip] * C)
    bufs = (torch.empty(K + 1, E, C, 38, device="cuda:0"), torch.empty(K, E, C, device="cuda:0"),
            torch.empty(K, E, C, dtype=torch.uint8, device="cuda:0"), torch.empty(K, E, dtype=torch.uint8, device="cuda:0"))
    res["rollout4"] = window(lambda: env.rollout(4, K, seed=2, step0=a.warm, auto_reset=True, trajectory=True,
                                                 obs_trajectory=True, out=bufs)) / K
    if hasattr(env, "collect"):
        from nascargymnasium_amd.onpolicy import ActorCriticNet, RolloutBatch
        vf = np.load(os.path.join(GOLD, "ppo_849_critic.npz"))
        ac = P.make_actor_critic([pi[k] for k in KEYS], [vf[k] for k in KEYS], int(vf["activation"]), vf["log_std"])
        env.set_actor_critic(ac)
        out = RolloutBatch(*[torch.empty((K + extra, *inner), dtype=dt, device="cuda:0")
                             for _n, dt, inner, extra in RolloutBatch.spec(E, C)])
        res["collect"] = window(lambda: env.collect(K, seed=2, step0=a.warm, out=out)) / K
        x1 = torch.randn(E * C, 38, device="cuda:0")
        x2 = torch.randn(2 * E * C, 38, device="cuda:0")
        for name, x in (("forward_1x", x1), ("forward_2x", x2)):
            res[name] = window(lambda: [env.controller_forward(clip, x) for _ in range(50)]) * 1e3 / 50
        KG = 128
        rew, val = torch.randn(KG, E, C, device="cuda:0"), torch.randn(KG + 1, E, C, device="cuda:0")
        ef = (torch.rand(KG, E, device="cuda:0") < 0.01).to(torch.uint8)
        tv = torch.zeros(KG, E, C, device="cuda:0")
        res["gae"] = window(lambda: [env.gae(rew, val, tv, ef, 0.99, 0.95) for _ in range(20)]) * 1e3 / 20

        def gae_torch():
            nnt = 1.0 - (ef & 3 != 0).float()[:, :, None]
            adv, last = torch.empty_like(rew), torch.zeros(E, C, device="cuda:0")
            r = rew + 0.99 * tv
            for k in reversed(range(KG)):
                delta = r[k] + 0.99 * val[k + 1] * nnt[k] - val[k]
                last = delta + 0.99 * 0.95 * nnt[k] * last
                adv[k] = last
            return adv, adv + val[:KG]
        res["gae_torch"] = window(gae_torch) * 1e3
        env.close()
        # the path a learner has without collect: VecCarEnv.step with the PyTorch forward and sample in between
        from nascargymnasium_amd.vec_env import VecCarEnv
        venv = VecCarEnv(E, "daytona", num_cars=C, return_tensors=True)
        net = ActorCriticNet(ac).cuda()
        venv.reset()
        venv.engine.set_state(state); venv.engine.obs.copy_(obs0)      # the same steady state as the other legs
        obs = obs0

        def vec_window(n):
            o = obs
            with torch.no_grad():
                for _ in range(n):
                    mu, v = net(o)
                    std = net.log_std.exp()
                    act = mu + std * torch.randn_like(mu)
                    lp = (-((act - mu) ** 2) / (2 * std * std) - net.log_std - 0.9189385332046727).sum(1)   # noqa: F841
                    o, _r, _d, _i = venv.step(torch.clamp(act, -1, 1).reshape(E, C, 2))
        vec_window(10)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        vec_window(K)
        e.record()
        torch.cuda.synchronize()
        res["vec_env"] = s.elapsed_time(e) / K
        venv.close()
    else:
        env.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="", help="built checkout of the parent commit (its rollout4 leg alternates with this tree's)")
    ap.add_argument("--shapes", default="8192x1,8192x10")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warm", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--cars", type=int, default=1)
    a = ap.parse_args()
    if a.child:
        return child(a)
    roots = ([("parent", os.path.abspath(a.parent))] if a.parent else []) + [("new", ROOT)]
    report = {"steps": a.steps, "warm_steps": a.warm, "rounds": a.rounds, "track": "daytona", "shapes": {}}
    for shape in a.shapes.split(","):
        E, C = [int(x) for x in shape.split("x")]
        runs = {name: [] for name, _ in roots}
        for _ in range(a.rounds):
            for name, root in roots:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--envs", str(E), "--cars", str(C),
                       "--steps", str(a.steps), "--warm", str(a.warm)]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    sys.exit(f"{name} child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")   # nothing more starts
                runs[name].append(json.loads(line[0][7:]))
        med = {name: {k: statistics.median(r[k] for r in rs) for k in rs[0]} for name, rs in runs.items()}
        new = med["new"]
        ratios = {"collect_over_rollout4_new": new["collect"] / new["rollout4"],
                  "vec_env_over_collect": new["vec_env"] / new["collect"],
                  "second_slot_forward_us": new["forward_2x"] - new["forward_1x"],
                  "gae_torch_over_gae": new["gae_torch"] / new["gae"]}
        if "parent" in med:
            ratios["collect_over_rollout4_parent"] = new["collect"] / med["parent"]["rollout4"]
            ratios["rollout4_new_over_parent"] = new["rollout4"] / med["parent"]["rollout4"]
        report["shapes"][shape] = {"median": med, "ratios": ratios, "windows": runs}
        print(shape, json.dumps({"median": med, "ratios": ratios}), flush=True)
    try:
        import torch
        report["device"] = torch.cuda.get_device_name(0)
    except Exception:
        pass
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

"""Time the categorical and the wide (512-512) on-policy collection, from a saved steady state:

    python tools/discrete_bench.py [--parent DIR] [--shapes 8192x1,8192x10] [--steps 128] [--rounds 5] [--out FILE.json]

Per shape (daytona, E envs x C cars) the driver starts one child process per measurement window, alternating the parent
commit's checkout (--parent: a built checkout of the commit before this feature, which runs the gauss leg only) with this
tree's, --rounds times each, and reports medians, every window and the parent's own spread.  Legs (ms per env step):

  gauss       collect(K) with a Gaussian 64-64 Tanh pair (random_actor_critic, seed 11)                   [parent and new]
  cat         collect(K) with a categorical 64-64 Tanh pair (random_discrete_actor_critic, seed 11)        [new]
  cat512      collect(K) with the categorical 512-512 ReLU pair: the wide kernel                           [new]
  vec_env512  K x VecCarEnv(discrete_action_space=True).step (return_tensors) with the PyTorch forward of the same
              512-512 nets and a torch Categorical sample in between: the path a learner has without collect  [new]

Comparisons: (a) cat over the parent's gauss, (b) vec_env512 over cat512, (c) this build's gauss over the parent's, against
the parent's run-to-run spread (max - min over median of its own windows).  Each child warms up with --warm
noisy-rule-driver steps from reset, saves that state, and runs each leg once untimed and once timed from the saved state
(HIP events around the whole window)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    sys.path.insert(0, a.root)
    import torch
    from nascargymnasium_amd import policy as P
    from nascargymnasium_amd.batched import BatchedCarEnv
    from nascargymnasium_amd import onpolicy as O
    E, C, K = a.envs, a.cars, a.steps
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

    def collect_leg(ac, Batch):
        env.set_actor_critic(ac)
        out = Batch(*[torch.empty((K + extra, *inner), dtype=dt, device="cuda:0") for _n, dt, inner, extra in Batch.spec(E, C)])
        return window(lambda: env.collect(K, seed=2, step0=a.warm, out=out)) / K

    res = {"gauss": collect_leg(P.random_actor_critic(64, 64, P.TANH, log_std=(-0.3, 0.2), seed=11), O.RolloutBatch)}
    if hasattr(P, "random_discrete_actor_critic"):
        res["cat"] = collect_leg(P.random_discrete_actor_critic(64, 64, P.TANH, seed=11), O.DiscreteRolloutBatch)
        wide = P.random_discrete_actor_critic(512, 512, P.RELU, seed=11)
        res["cat512"] = collect_leg(wide, O.DiscreteRolloutBatch)
        env.close()
        from nascargymnasium_amd.vec_env import VecCarEnv
        venv = VecCarEnv(E, "daytona", num_cars=C, return_tensors=True, discrete_action_space=True)
        net = O.CategoricalActorCriticNet(wide).cuda()
        venv.reset()
        venv.engine.set_state(state); venv.engine.obs.copy_(obs0)      # the same steady state as the other legs

        def vec_window(n):
            o = obs0
            with torch.no_grad():
                for _ in range(n):
                    logits, v = net(o)
                    dist = torch.distributions.Categorical(logits=logits)
                    act = dist.sample()
                    lp = dist.log_prob(act)                            # noqa: F841
                    o, _r, _d, _i = venv.step(act.reshape(E, C))
        vec_window(10)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        vec_window(K)
        e.record()
        torch.cuda.synchronize()
        res["vec_env512"] = s.elapsed_time(e) / K
        venv.close()
    else:
        env.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="", help="built checkout of the parent commit (its gauss leg alternates with this tree's)")
    ap.add_argument("--shapes", default="8192x1,8192x10")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warm", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--cars", type=int, default=1)
    a = ap.parse_args()
    if a.child:
        return child(a)
    roots = ([("parent", os.path.abspath(a.parent))] if a.parent else []) + [("new", ROOT)]
    report = {"steps": a.steps, "warm_steps": a.warm, "rounds": a.rounds, "track": "daytona", "unit": "ms per env step",
              "shapes": {}}
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
                print(shape, name, line[0][7:], flush=True)
        med = {name: {k: statistics.median(r[k] for r in rs) for k in rs[0]} for name, rs in runs.items()}
        new = med["new"]
        ratios = {"b_vec_env512_over_cat512": new["vec_env512"] / new["cat512"], "cat_over_gauss_new": new["cat"] / new["gauss"],
                  "cat512_over_cat": new["cat512"] / new["cat"]}
        if "parent" in med:
            pg = [r["gauss"] for r in runs["parent"]]
            ratios["a_cat_over_gauss_parent"] = new["cat"] / med["parent"]["gauss"]
            ratios["c_gauss_new_over_parent"] = new["gauss"] / med["parent"]["gauss"]
            ratios["parent_gauss_spread"] = (max(pg) - min(pg)) / med["parent"]["gauss"]
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

"""Time `collect` under the running normalisation (set_normalize) against `collect` without it, against the parent
commit's `collect`, and against the route a learner had before it, from a saved steady state:

    python tools/normalize_bench.py [--parent DIR] [--shapes 8192x1,8192x10] [--steps 128] [--rounds 5] [--out FILE.json]

Per shape (daytona, E envs x C cars) the driver starts one child process per measurement window, alternating the parent
commit's checkout (--parent: a built checkout of the commit before this feature, which runs the collect leg only) with
this tree's, --rounds times each, and reports the medians and the parent leg's own spread.  Legs (ms per env step):

  collect            collect(K) without normalisation                                              [parent and new]
  collect_frozen     collect(K) under set_normalize(training=False): row-local, the shards stay unsynchronised   [new]
  collect_training   collect(K) under set_normalize(training=True): one shard, statistics updated every step     [new]
  vec_env_norm       K x VecCarEnv.step (return_tensors) with ActorCriticNet's forward and sample, and VecNormalize in
                     PyTorch ops on the device (float64 mean / var of the batch, the update, normalise, returns): the
                     route a learner had                                                                          [new]
  step_wait_training / step_wait_frozen   normalize_step alone, 50 launches back to back (us): their difference is the
                     moments launch plus the one-workgroup statistics update                                      [new]
  copy               a plain device copy of the same [N, 38] float32 batch (us): its read rate prices the moments
                     launch's one pass over the batch                                                             [new]

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
NORM = dict(clip_obs=1.0, gamma=0.99)         # learn/a2c.py:94-100


def child(a):
    sys.path.insert(0, a.root)
    import numpy as np
    import torch
    from nascargymnasium_amd import policy as P
    from nascargymnasium_amd.batched import BatchedCarEnv
    from nascargymnasium_amd.onpolicy import ActorCriticNet, RolloutBatch
    E, C, K = a.envs, a.cars, a.steps
    pi, vf = np.load(os.path.join(GOLD, "ppo_849_actor.npz")), np.load(os.path.join(GOLD, "ppo_849_critic.npz"))
    ac = P.make_actor_critic([pi[k] for k in KEYS], [vf[k] for k in KEYS], int(vf["activation"]), vf["log_std"])
    env = BatchedCarEnv(E, C, "daytona", device="cuda:0")
    env.set_actor_critic(ac)
    env.reset()
    env.rollout(3, a.warm, seed=1, step0=0, auto_reset=True)
    state, obs0 = env.get_state(), env.obs.clone()

    def window(fn, before=None):
        out = None
        for timed in (False, True):
            env.set_state(state); env.obs.copy_(obs0)
            if before:
                before()
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            out = s.elapsed_time(e)
        return out                                                     # ms per window

    def bufs(batch):
        return batch(*[torch.empty((K + extra, *inner), dtype=dt, device="cuda:0") for _n, dt, inner, extra in batch.spec(E, C)])

    res = {}
    out = bufs(RolloutBatch)
    res["collect"] = window(lambda: env.collect(K, seed=2, step0=a.warm, out=out)) / K
    if not hasattr(env, "set_normalize"):
        env.close()
        print("RESULT " + json.dumps(res))
        return
    from nascargymnasium_amd.onpolicy import NormalizedRolloutBatch
    nout = bufs(NormalizedRolloutBatch)
    # statistics of a few hundred steps, so that the frozen leg normalises with something a learner would have
    env.set_normalize(**NORM)
    env.normalize_step()
    env.collect(K, seed=5, step0=0, out=nout)
    stats = env.norm_stats()

    def start(training):
        def f():
            env.set_normalize(training=training, **NORM)
            env.load_norm_stats(stats)
            env.normalize_step()
        return f
    res["collect_frozen"] = window(lambda: env.collect(K, seed=2, step0=a.warm, out=nout), start(False)) / K
    res["collect_training"] = window(lambda: env.collect(K, seed=2, step0=a.warm, out=nout), start(True)) / K
    res["step_wait_frozen"] = window(lambda: [env.normalize_step() for _ in range(50)], start(False)) * 1e3 / 50
    res["step_wait_training"] = window(lambda: [env.normalize_step() for _ in range(50)], start(True)) * 1e3 / 50
    src, dst = env.obs.clone(), torch.empty_like(env.obs)
    res["copy"] = window(lambda: [dst.copy_(src) for _ in range(50)]) * 1e3 / 50
    res["batch_bytes"] = int(src.numel() * 4)
    env.set_normalize(False)
    env.close()
    # the route a learner had: VecCarEnv.step, the PyTorch forward and sample, VecNormalize in PyTorch ops
    from nascargymnasium_amd.vec_env import VecCarEnv
    venv = VecCarEnv(E, "daytona", num_cars=C, return_tensors=True)
    net = ActorCriticNet(ac).cuda()
    venv.reset()
    venv.engine.set_state(state); venv.engine.obs.copy_(obs0)
    N = E * C
    f64 = torch.float64

    class Rms:
        def __init__(self, shape):
            self.mean, self.var, self.count = torch.zeros(shape, dtype=f64, device="cuda:0"), torch.ones(shape, dtype=f64, device="cuda:0"), 1e-4

        def update(self, x):
            x = x.to(f64)
            bm, bv, bc = x.mean(0), x.var(0, unbiased=False), x.shape[0]
            delta, tot = bm - self.mean, self.count + bc
            m2 = self.var * self.count + bv * bc + delta * delta * self.count * bc / tot
            self.mean, self.var, self.count = self.mean + delta * bc / tot, m2 / tot, tot
    obs_rms, ret_rms = Rms((38,)), Rms(())
    returns = torch.zeros(N, dtype=f64, device="cuda:0")

    def norm_obs(o):
        return torch.clamp((o.to(f64) - obs_rms.mean) / torch.sqrt(obs_rms.var + 1e-8), -1.0, 1.0).float()

    def vec_window(n, o):
        nonlocal returns
        with torch.no_grad():
            for _ in range(n):
                mu, v = net(o)
                std = net.log_std.exp()
                act = mu + std * torch.randn_like(mu)
                lp = (-((act - mu) ** 2) / (2 * std * std) - net.log_std - 0.9189385332046727).sum(1)   # noqa: F841
                raw, r, d, _i = venv.step(torch.clamp(act, -1, 1).reshape(E, C, 2))
                raw, r = raw.reshape(N, 38), r.reshape(N)
                obs_rms.update(raw)
                o = norm_obs(raw)
                returns = returns * 0.99 + r
                ret_rms.update(returns)
                nr = torch.clamp(r.to(f64) / torch.sqrt(ret_rms.var + 1e-8), -10.0, 10.0).float()   # noqa: F841
                returns = torch.where(d.reshape(E, 1).expand(E, C).reshape(N).bool(), torch.zeros_like(returns), returns)
        return o
    o = vec_window(10, norm_obs(obs0.reshape(N, 38)))
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    vec_window(K, o)
    e.record()
    torch.cuda.synchronize()
    res["vec_env_norm"] = s.elapsed_time(e) / K
    venv.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="", help="built checkout of the parent commit (its collect leg alternates with this tree's)")
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
    report = {"steps": a.steps, "warm_steps": a.warm, "rounds": a.rounds, "track": "daytona", "normalize": NORM, "shapes": {}}
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
        moments_us = new["step_wait_training"] - new["step_wait_frozen"]
        read_us = new["copy"]          # the copy reads the batch once (and writes it once): its time prices one streamed read
        ratios = {"frozen_over_off": new["collect_frozen"] / new["collect"],
                  "training_over_off": new["collect_training"] / new["collect"],
                  "vec_env_norm_over_training": new["vec_env_norm"] / new["collect_training"],
                  "moments_and_update_us": moments_us,
                  "copy_read_GBps": new["batch_bytes"] / (read_us * 1e-6) / 1e9,
                  "moments_and_update_over_copy": moments_us / read_us}
        if "parent" in med:
            pw = [r["collect"] for r in runs["parent"]]
            ratios["off_over_parent"] = new["collect"] / med["parent"]["collect"]
            ratios["parent_spread"] = {"min": min(pw), "max": max(pw), "max_over_min": max(pw) / min(pw)}
            ratios["off_within_parent_spread"] = bool(min(pw) <= new["collect"] <= max(pw))
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

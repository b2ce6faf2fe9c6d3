"""Time the off-policy collection and the replay sampler against what a learner had before them, from a saved steady
state:

    python tools/replay_bench.py [--parent DIR] [--shapes 8192x1,8192x10] [--steps 128] [--rounds 5] [--out FILE.json]

Per shape (daytona, E envs x C cars) the driver starts one child process per measurement window, alternating the parent
commit's checkout (--parent: a built checkout of the commit before the off-policy collection, which runs the rollout2 leg
only) with this tree's, --rounds times each, and reports the medians and the parent leg's run-to-run spread.  Legs:

  rollout2      rollout(2, K): the deterministic sac_1235 actor (float32) in the sharded rollout, ms per step: what the
                device could run before (no sampling, no buffer)                                        [parent and new]
  collect       collect_transitions(ring, K, source=7): sac_1235 with its log_std head sampled, the transitions written
                into a ring of K step slots, ms per step                                                 [new]
  host          K x (SquashedActorNet forward and sample in PyTorch + VecCarEnv.step (return_tensors) + the seven buffer
                writes in PyTorch ops): the route a SAC learner has without collect_transitions, ms per step   [new]
  sample_512 / sample_65536       ReplayBuffer.sample(batch) on the ring the collect leg filled, us per call  [new]
  torch_512 / torch_65536         the same gather in PyTorch ops on the same tensors (randint x 2 and the six indexed
                reads), us per call                                                                       [new]

Each child warms up with --warm noisy-rule-driver steps from reset, saves that state, runs each leg once untimed and once
timed from the saved state (HIP events around the whole window; the sampler legs around 200 calls).  Clocks as found.  The
weights are the committed fixtures under tests/golden."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def child(a):
    sys.path.insert(0, a.root)
    import numpy as np
    import torch
    from nascargymnasium_amd import policy as P
    from nascargymnasium_amd.batched import BatchedCarEnv
    E, C, K = a.envs, a.cars, a.steps
    d = np.load(os.path.join(GOLD, "sac_1235_actor.npz"))
    w = {k: d[k.replace(".", "__")] for k in P.ACTOR_KEYS}
    env = BatchedCarEnv(E, C, "daytona", device="cuda:0")
    env.reset()
    env.rollout(3, a.warm, seed=1, step0=0, auto_reset=True)
    state, obs0 = env.get_state(), env.obs.clone()

    def window(fn, restore=True):
        out = None
        for _timed in (False, True):
            if restore:
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
    env.set_actor(w, precision="fp32")
    res["rollout2"] = window(lambda: env.rollout(2, K, seed=2, step0=a.warm, auto_reset=True)) / K
    if not hasattr(env, "collect_transitions"):
        env.close()
        print("RESULT " + json.dumps(res))
        return
    from nascargymnasium_amd.offpolicy import ReplayBuffer, SquashedActorNet
    h = np.load(os.path.join(GOLD, "sac_1235_log_std.npz"))
    keys = list(P.ACTOR_KEYS)
    actor = P.make_squashed_actor([w[k] for k in keys[:4]] + [np.concatenate([w[keys[4]], h["weight"]]),
                                                               np.concatenate([w[keys[5]], h["bias"]])], P.RELU, "sac")
    env.set_explorer(actor)
    rb = ReplayBuffer(env, K)

    def collect():
        rb.pos, rb.full = 0, False
        env.collect_transitions(rb, K, seed=2, step0=a.warm)
    res["collect"] = window(collect) / K
    res["ring_bytes_per_step"] = rb.bytes_per_step
    if a.sampler:
        N, reps = E * C, 200
        for B in (512, 65536):
            res[f"sample_{B}"] = window(lambda: [rb.sample(B, seed=3, draw=i) for i in range(reps)], restore=False) * 1e3 / reps
            flat = [t.reshape(rb.capacity * N, *t.shape[3:]) for t in (rb.obs, rb.actions, rb.next_obs, rb.dones,
                                                                       rb.timeouts, rb.rewards)]

            def gather():
                for _ in range(reps):
                    slot = torch.randint(0, rb.size, (B,), device="cuda:0")
                    car = torch.randint(0, N, (B,), device="cuda:0")
                    i = slot * N + car
                    o, ac, no, dn, to, rw = [t[i] for t in flat]
                    dn = dn.float() * (1 - to.float())                  # noqa: F841
            res[f"torch_{B}"] = window(gather, restore=False) * 1e3 / reps
    env.close()
    # the route a learner has without collect_transitions
    from nascargymnasium_amd.vec_env import VecCarEnv
    venv = VecCarEnv(E, "daytona", num_cars=C, return_tensors=True)
    net = SquashedActorNet(actor).cuda()
    venv.reset()
    venv.engine.set_state(state); venv.engine.obs.copy_(obs0)          # the same steady state as the other legs
    hb = ReplayBuffer(venv.engine, K)

    def host_window(n):
        o = obs0
        with torch.no_grad():
            for k in range(n):
                t = net(o)                                              # tanh(mu + std * randn)
                nxt, r, dn, _i = venv.step(t.reshape(E, C, 2))          # Box(-1, 1): unscale_action is the identity
                p = k % hb.capacity
                hb.obs[p].copy_(o.reshape(E, C, 38)); hb.next_obs[p].copy_(nxt.reshape(E, C, 38))
                hb.actions[p].copy_(t.reshape(E, C, 2)); hb.rewards[p].copy_(r.reshape(E, C))
                dd = dn.reshape(E, 1).expand(E, C)
                hb.dones[p].copy_(dd); hb.timeouts[p].zero_(); hb.live[p].fill_(1)
                o = nxt
    host_window(10)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    host_window(K)
    e.record()
    torch.cuda.synchronize()
    res["host"] = s.elapsed_time(e) / K
    venv.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="", help="built checkout of the parent commit (its rollout2 leg alternates with this tree's)")
    ap.add_argument("--shapes", default="8192x1,8192x10")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warm", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--sampler", type=int, default=0)
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
                       "--steps", str(a.steps), "--warm", str(a.warm), "--sampler", str(int(E * C >= 81920))]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    sys.exit(f"{name} child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")   # nothing more starts
                runs[name].append(json.loads(line[0][7:]))
        med = {name: {k: statistics.median(r[k] for r in rs) for k in rs[0]} for name, rs in runs.items()}
        new = med["new"]
        base = runs.get("parent", runs["new"])
        r2 = [r["rollout2"] for r in base]
        ratios = {"collect_over_rollout2_new": new["collect"] / new["rollout2"],
                  "host_over_collect": new["host"] / new["collect"],
                  "rollout2_spread": (max(r2) - min(r2)) / statistics.median(r2)}
        if "parent" in med:
            ratios["collect_over_rollout2_parent"] = new["collect"] / med["parent"]["rollout2"]
            ratios["rollout2_new_over_parent"] = new["rollout2"] / med["parent"]["rollout2"]
        for B in (512, 65536):
            if f"sample_{B}" in new:
                ratios[f"torch_over_sample_{B}"] = new[f"torch_{B}"] / new[f"sample_{B}"]
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

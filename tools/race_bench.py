#!/usr/bin/env python
"""What the race ledger costs (nascar_set_race): rollout(4, K, auto_reset=False) with race mode off / 1 / 2 against the
same rollout of a parent build of the library, and against fitness accumulation as the comparable per-step accumulator;
the host loop the ledger replaces; the rank kernel.  Writes one JSON file (default profiles/race.json).

    python tools/race_bench.py --parent-tree ab/parent [--out profiles/race.json]

The parent tree is a built checkout of the commit before the race modes (`git archive HEAD~ | tar -x -C ab/parent`, then
its own build()): its package and library run in processes of their own.  Parent and new processes alternate, and which
of the two runs first alternates from round to round (--rounds).  Every process warms each configuration up, keeps that state, and then times
--windows windows of --reps rollouts of K steps, each window starting from the kept state (so every window of every variant and library steps the same cars through the
same steps) and ending in a device synchronise; the parent's window-to-window
spread (min .. max over all its windows) is the yardstick for "race mode off costs nothing": the summary says whether the new
library's mode-off median lies inside it, and the run exits 1 when it lies above it.  One process holds the GPU at a time; a child that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(8192, 1), (8192, 10)]
K = 128


def child(args):
    sys.path.insert(0, os.path.abspath(args.root))     # the tree under test: this one, or the parent's
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from nascargymnasium_amd import _lib, policy as P
    from nascargymnasium_amd.batched import BatchedCarEnv
    new = hasattr(BatchedCarEnv, "set_race")
    d = np.load(os.path.join(ROOT, "tests", "golden", "sac_1235_actor.npz"))
    w = {k: d[k.replace(".", "__")] for k in P.ACTOR_KEYS}
    sac = P.make_controller([w[k] for k in P.ACTOR_KEYS], P.RELU, P.OUT_SQUASH, "sac")
    out = []

    def timed(fn, n, prep=None):
        ts = []
        for _ in range(n):
            if prep:
                prep()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    for E, C in SIZES:
        for field in ("rule", "sac"):
            env = BatchedCarEnv(E, C, "daytona", device="cuda:0")
            env.set_car_controllers([env.add_controller(sac)] * C if field == "sac" else ["rule"] * C)
            env.reset()
            env.rollout(4, args.warmup, auto_reset=True)          # the steady state: envs spread over their episodes
            state0, obs0 = env.get_state(), env.obs.clone()

            def restore():      # every window steps the same cars through the same steps, whatever ran before it
                env.set_state(state0)
                env.obs.copy_(obs0)
                if env_race[0] == "fitness":
                    env.set_fitness(True)       # (zeroes the accumulators and the ended bytes)
                elif env_race[0]:
                    env.race_begin(False)
            env_race = [None]
            variants = ["off", "fitness"] + (["race1", "race2"] if new else [])
            step0 = args.warmup
            for v in variants:
                if v == "fitness":
                    env.set_fitness(True)
                if v.startswith("race"):
                    env.set_race(int(v[-1]))
                env_race[0] = v if v != "off" else None
                run = lambda: [env.rollout(4, K, step0=step0, auto_reset=False) for _ in range(args.reps)]
                timed(run, 2, restore)                              # this variant's launches, warm
                ts = timed(run, args.windows, restore)
                if v == "fitness":
                    env.set_fitness(False)
                if v.startswith("race"):
                    env.set_race(0)
                env_race[0] = None
                out.append({"E": E, "C": C, "field": field, "variant": v, "K": K * args.reps, "window_ms": ts})
            if new and field == "rule":
                import race_ref
                # what a user does today: actions, step, the info tensor to the host, the reference's loop in Python
                restore()
                races = [race_ref.EnvRace(C, 1) for _ in range(E)]
                I = _lib.INFO_INDEX

                def host_step():
                    env.step(env.policy_actions(4, 0, 0), auto_reset=False)
                    rew, info = env.reward.cpu().numpy(), env.info_tensor().cpu().numpy()
                    done = (env.env_flags.cpu().numpy() & 3) != 0
                    laps, last = info[..., I["lap_count"]], info[..., I["last_lap_time"]]
                    dis, st = info[..., I["disabled"]] != 0, info[..., I["simulation_time"]]
                    for e, r in enumerate(races):
                        r.step(rew[e], laps[e].tolist(), [race_ref.none_if_nan(x) for x in last[e]], dis[e].tolist(),
                               float(st[e, 0]), bool(done[e]))
                host_step()
                out.append({"E": E, "C": C, "field": field, "variant": "host_loop", "K": 1, "window_ms": timed(host_step, 3)})
                env.set_race(1)
                env.rollout(4, 4, auto_reset=False)
                env.race_rank(1)
                rank = lambda: [env.race_rank(1) for _ in range(20)]
                out.append({"E": E, "C": C, "field": field, "variant": "race_rank_x20", "K": 20, "window_ms": timed(rank, 5)})
                env.set_race(0)
            env.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "race.json"))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--reps", type=int, default=4, help="rollouts of K steps per timed window")
    ap.add_argument("--warmup", type=int, default=512)
    ap.add_argument("--child-timeout", type=int, default=420, help="seconds a child process may take")
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = {"parent": [], "new": []}
    order = []
    for r in range(args.rounds):      # parent first in even rounds, new first in odd ones
        order += (["parent", "new"][::1 if r % 2 == 0 else -1] if args.parent_tree else ["new"])
    for tag in order:
        env = dict(os.environ)
        env.pop("NASCAR_LIB", None)
        env.pop("PYTHONPATH", None)
        root = os.path.abspath(args.parent_tree) if tag == "parent" else ROOT
        try:      # (a child took 12 s on an MI355X with the defaults)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--windows",
                                str(args.windows), "--reps", str(args.reps), "--warmup", str(args.warmup)], env=env,
                               cwd=root, capture_output=True, text=True, timeout=args.child_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{tag} child ran past {args.child_timeout} s: nothing more is started")
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"{tag} child failed (exit {r.returncode}): nothing more is started")
        runs[tag].append(json.loads(line[0][7:]))
        print(tag, "done", flush=True)
    rows, procs = {}, {}
    for tag, rr in runs.items():
        for res in rr:
            for x in res:
                key = (x["E"], x["C"], x["field"], x["variant"], tag)
                per = [t / x["K"] for t in x["window_ms"]]
                rows.setdefault(key, []).extend(per)
                procs.setdefault(key, []).append(statistics.median(per))
    table = []
    for (E, C, field, variant, tag), per in sorted(rows.items()):
        table.append({"E": E, "C": C, "field": field, "variant": variant, "lib": tag, "windows": len(per),
                      "process_medians_ms_per_step": procs[(E, C, field, variant, tag)],
                      "ms_per_step_median": statistics.median(per), "ms_per_step_min": min(per), "ms_per_step_max": max(per)})
    get = lambda E, C, f, v, t: next((x for x in table if (x["E"], x["C"], x["field"], x["variant"], x["lib"]) == (E, C, f, v, t)), None)
    summary = []
    for E, C in SIZES:
        for field in ("rule", "sac"):
            p, pf = get(E, C, field, "off", "parent"), get(E, C, field, "fitness", "parent")
            s = {"E": E, "C": C, "field": field}
            for v in ("off", "fitness", "race1", "race2"):
                n = get(E, C, field, v, "new")
                if n and p:
                    s[v + "_over_parent_off"] = n["ms_per_step_median"] / p["ms_per_step_median"]
                if n and pf and v.startswith("race"):
                    s[v + "_over_parent_fitness"] = n["ms_per_step_median"] / pf["ms_per_step_median"]
            if p:
                off = get(E, C, field, "off", "new")
                s["parent_off_window_spread_ms_per_step"] = [p["ms_per_step_min"], p["ms_per_step_max"]]
                s["new_off_median_inside_parent_spread"] = bool(p["ms_per_step_min"] <= off["ms_per_step_median"] <= p["ms_per_step_max"])
                s["new_off_median_above_parent_spread"] = bool(off["ms_per_step_median"] > p["ms_per_step_max"])
            summary.append(s)
    doc = {"what": "rollout(4, K=128, auto_reset=False) on daytona after a 512-step auto-reset warm-up; ms per step per "
                   "window of `rollouts_per_window` rollouts, each window starting from the state kept after the warm-up and ending in a device synchronise; parent = a built checkout of the parent commit, "
                   "run in alternating processes in `process_order`; host_loop = policy_actions + step + info_tensor().cpu() "
                   "+ the reference's Python loop, per step; race_rank_x20 = per race_rank call",
           "rounds": args.rounds, "windows_per_round": args.windows, "rollouts_per_window": args.reps,
           "process_order": order, "table": table, "summary": summary}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(summary, indent=1))
    above = [(x["E"], x["C"], x["field"]) for x in summary if x.get("new_off_median_above_parent_spread")]
    if above:
        raise SystemExit(f"race mode off is slower than the parent's slowest window at {above}")


if __name__ == "__main__":
    main()

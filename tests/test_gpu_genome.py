"""Genome drivers (device action source 5, NASCAR_CTRL_GENOME) and the on-device fitness accumulators against their
host oracles (tests/genome_ref.py): the driver alone on directed observation sequences, its identity with the rule
driver, genome slots in a mixed field, a whole evaluation rollout against the host loop it replaces, the library's
error messages, and nascargymnasium_amd.genetic's evaluate / GeneticTrainer.  Every comparison is bit for bit."""
import os

import numpy as np
import pytest

from genome_ref import FitnessLoop, GenomeDriver, drive, synthetic_case
from golden_replay import GOLDEN, TRACKS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from nascargymnasium_amd import _lib, genetic as G   # noqa: E402
from nascargymnasium_amd import policy as P          # noqa: E402

# Evaluation scene: env IDLE_ENV's ten cars have g[2] = g[3] = 0, so their throttle never leaves 0; they stand on the
# grid until the stuck rule disables them and the env terminates with all cars disabled at step TERMINAL_STEP (found
# with the engine and asserted below; the golden trace env_martinsville_all_idle ends at the same step).  K is the
# smallest count with 50 further steps after it.
IDLE_ENV = 5
TERMINAL_STEP = 600
K = TERMINAL_STEP + 50


def _track(name):
    return os.path.join(TRACKS, name + ".track")


def _engine(E, C, tracks):
    from nascargymnasium_amd.batched import BatchedCarEnv
    files = [_track(t) for t in tracks] if not isinstance(tracks, str) else _track(tracks)
    return BatchedCarEnv(E, C, files, device="cuda:0")


def _ctl(env):
    """the drivers' per-car state [N, 4] float64: the last region of the state arena"""
    n = 32 * env.N
    tail = (n + 255) // 256 * 256
    return env.get_state().cpu().numpy()[-tail:][:n].view(np.float64).reshape(env.N, 4)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _bits_t(t):
    return t.view(torch.int32)


def test_driver_on_directed_sequences():
    """130 cars (two waves and two lanes: the only block is partial), 64 steps, genomes from the bounds: actions and
    the control state equal the restatement bit for bit at every step"""
    g, obs, counts = synthetic_case(130, 64, 3, G.GENOME_BOUNDS)
    assert all(v > 0 for v in counts.values()), counts
    env = _engine(13, 10, "martinsville")
    env.set_genomes(g)
    ref = [GenomeDriver(x) for x in g]
    dev = torch.from_numpy(obs).cuda()
    for k in range(len(obs)):
        got = env.policy_actions(5, obs=dev[k]).cpu().numpy().reshape(130, 2)
        want = drive(ref, obs[k])
        assert np.array_equal(_bits(got), _bits(want)), (k, np.argwhere(_bits(got) != _bits(want))[:4])
        ctl = np.stack([d.ctl() for d in ref])
        assert np.array_equal(_bits(_ctl(env)), _bits(ctl)), (k, np.argwhere(_bits(_ctl(env)) != _bits(ctl))[:4])
    # [E, C, 12] is accepted as well, and a new table starts the controllers afresh
    env.set_genomes(g.reshape(13, 10, 12))
    assert not _ctl(env).any()
    got = env.policy_actions(5, obs=dev[0]).cpu().numpy().reshape(130, 2)
    assert np.array_equal(_bits(got), _bits(drive([GenomeDriver(x) for x in g], obs[0])))
    env.close()


def test_rule_genome_is_policy_1():
    """26 x 10 daytona, 300 steps: policy 5 with a RULE_GENOME table, and a field whose slots alternate "genome" and
    "rule", equal policy 1 in observations, rewards, flags and the state arena (control state included)"""
    E, C, S = 26, 10, 300
    table = np.tile(np.asarray(G.RULE_GENOME, np.float64), (E * C, 1))
    outs = []
    for mode in ("rule", "genome", "field"):
        env = _engine(E, C, "daytona")
        env.reset()
        if mode != "rule":
            env.set_genomes(table)
        if mode == "field":
            env.set_car_controllers(["genome", "rule"] * 5)
        obs, rew, cf, ef = env.rollout({"rule": 1, "genome": 5, "field": 4}[mode], S, trajectory=True)
        outs.append((obs.clone(), rew, cf, ef, env.get_state()))
        env.close()
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)
    assert outs[0][1].abs().sum() > 0


def test_genome_slots_in_a_mixed_field():
    """C = 4: ["genome", "rule", "noisy", sac].  The genome column of policy_actions(4) is policy 5's for those cars,
    the other columns are their own sources' (each twin sees the same observations, so its per-car state follows)."""
    d = np.load(os.path.join(GOLDEN, "sac_1235_actor.npz"))
    w = {k: d[k.replace(".", "__")] for k in P.ACTOR_KEYS}
    sac = P.make_controller([w[k] for k in P.ACTOR_KEYS], P.RELU, P.OUT_SQUASH, "sac")
    E, C, seed = 37, 4, 11
    g = G.random_genomes(np.random.default_rng(2), E * C)
    env = _engine(E, C, "martinsville")
    twins = {p: _engine(E, C, "martinsville") for p in (5, 1, 3)}
    cid = env.add_controller(sac)
    env.set_genomes(g)
    twins[5].set_genomes(g)
    env.set_car_controllers(["genome", "rule", "noisy", cid])
    env.reset()
    for k in range(40):
        a = env.policy_actions(4, seed, k).clone()
        for slot, p in enumerate((5, 1, 3)):
            want = twins[p].policy_actions(p, seed, k, obs=env.obs)
            assert torch.equal(a[:, slot], want[:, slot]), (k, slot)
        assert torch.equal(a[:, 3], env.controller_forward(cid, env.obs[:, 3]))
        env.step(a)
    assert torch.equal(torch.from_numpy(_ctl(env)).view(E, C, 4)[:, 0], torch.from_numpy(_ctl(twins[5])).view(E, C, 4)[:, 0])
    for e in [env] + list(twins.values()):
        e.close()


def test_evaluation_rollout_equals_the_host_loop():
    """13 envs on daytona + 13 on martinsville, 10 cars each (one full 12-env workgroup and one 1-env workgroup per
    track, 4 shards): rollout(5, K) with fitness on equals policy_actions(5) + step + info_tensor + the trainer's
    Python accumulation on a twin engine, all 8 fields of every car bit for bit; the idle env ends inside K and its
    accumulators stay at their terminal-step values; a second set_fitness(True) zeroes them."""
    E, C = 26, 10
    tracks = ["daytona"] * 13 + ["martinsville"] * 13
    g = G.random_genomes(np.random.default_rng(7), E * C).reshape(E, C, 12)
    g[IDLE_ENV, :, 2] = 0.0
    g[IDLE_ENV, :, 3] = 0.0
    a, b = _engine(E, C, tracks), _engine(E, C, tracks)
    for env in (a, b):
        env.set_rollout_streams(4)
        env.set_genomes(g)
        env.reset()
    a.set_envs_per_block(12)        # the twin keeps the automatic layout (1 env per workgroup at this size)
    bt, _ = a.block_map()
    assert len(bt) == 4 and sorted(bt.tolist()) == [0, 0, 1, 1]
    a.set_fitness(True)
    a.rollout(5, K, auto_reset=False)
    dev = a.fitness().cpu().numpy().reshape(E * C, 8)

    loop = FitnessLoop(E, C)
    ended_at = {}
    at_terminal = None
    for k in range(K):
        b.step(b.policy_actions(5), auto_reset=False)
        done = ((b.env_flags & (_lib.EF_TERMINATED | _lib.EF_TRUNCATED)) != 0).cpu().numpy()
        loop.update(b.reward.cpu().numpy(), b.info_tensor().cpu().numpy(), done, _lib.INFO_INDEX)
        for e in np.nonzero(done)[0]:
            ended_at.setdefault(int(e), k + 1)
        if at_terminal is None and IDLE_ENV in ended_at:
            at_terminal = loop.rows()[IDLE_ENV * C:(IDLE_ENV + 1) * C].copy()
    host = loop.rows()
    print("envs ended at", ended_at)
    assert torch.equal(a.obs, b.obs) and torch.equal(a.get_state(), b.get_state())
    # at least one env ends inside K with 50 steps to spare, at least one does not end
    assert ended_at.get(IDLE_ENV) == TERMINAL_STEP and K - TERMINAL_STEP >= 50
    assert len(ended_at) < E
    assert _lib.FITNESS_FIELDS == a.FITNESS_FIELDS and len(_lib.FITNESS_FIELDS) == 8
    for f, name in enumerate(_lib.FITNESS_FIELDS):
        assert np.array_equal(_bits(dev[:, f]), _bits(host[:, f])), (name, np.argwhere(_bits(dev[:, f]) != _bits(host[:, f]))[:4])
    idle = dev[IDLE_ENV * C:(IDLE_ENV + 1) * C]
    assert np.array_equal(_bits(idle), _bits(at_terminal))
    steps = dev[:, _lib.FITNESS_FIELDS.index("steps")].reshape(E, C)
    assert np.all(steps[IDLE_ENV] == TERMINAL_STEP)
    assert np.all(steps[[e for e in range(E) if e not in ended_at]] == K)
    dis = idle[:, _lib.FITNESS_FIELDS.index("disabled_at_step")]
    assert np.all(dis > 0) and np.all(dis <= TERMINAL_STEP)
    assert dev[:, _lib.FITNESS_FIELDS.index("total_reward")].std() > 0

    a.set_fitness(True)
    z = a.fitness().cpu().numpy().reshape(E * C, 8)
    lt, da = _lib.FITNESS_FIELDS.index("lap_time"), _lib.FITNESS_FIELDS.index("disabled_at_step")
    assert np.all(np.isnan(z[:, lt])) and np.all(z[:, da] == -1)
    assert not np.delete(z, [lt, da], axis=1).any()
    a.close(); b.close()


def test_back_to_back_genome_uploads_keep_their_order():
    """Two set_genomes calls with nothing between them share one pinned staging buffer: the second waits for the
    first upload to leave it, and the table the driver reads is the second one, as in an engine given only that."""
    E, C = 2, 2
    rng = np.random.default_rng(7)
    ga, gb = G.random_genomes(rng, E * C), G.random_genomes(rng, E * C)
    env, fresh = _engine(E, C, "martinsville"), _engine(E, C, "martinsville")
    env.reset(); fresh.reset()
    env.set_genomes(ga)
    only_a = env.policy_actions(5).clone()
    env.set_genomes(ga)
    env.set_genomes(gb)
    fresh.set_genomes(gb)
    assert not torch.equal(env.policy_actions(5), only_a)       # the two tables drive differently from the grid
    fresh.policy_actions(5)
    for k in range(5):
        assert torch.equal(_bits_t(env._actions), _bits_t(fresh._actions)), k
        env.step(env._actions); fresh.step(fresh._actions)
        env.policy_actions(5); fresh.policy_actions(5)
    assert np.array_equal(_bits(_ctl(env)), _bits(_ctl(fresh)))
    env.close(); fresh.close()


def test_errors_carry_the_library_message():
    env = _engine(2, 3, "martinsville")
    env.reset()
    with pytest.raises(RuntimeError, match=r"policy 5 needs a genome table \(nascar_set_genomes\)"):
        env.policy_actions(5)
    with pytest.raises(RuntimeError, match=r"policy 5 needs a genome table \(nascar_set_genomes\)"):
        env.rollout(5, 2)
    with pytest.raises(RuntimeError, match=r"unknown controller id -4 .*once a genome table is set"):
        env.set_car_controllers(["genome", "rule", "rule"])         # a genome slot before any table
    g = G.random_genomes(np.random.default_rng(0), 6)
    bad = g.copy()
    bad[4, 7] = np.inf
    with pytest.raises(RuntimeError, match=r"genome of car 4: gene 7 is not finite"):
        env.set_genomes(bad)
    with pytest.raises(ValueError, match="genomes must be"):
        env.set_genomes(g[:5])
    env.set_genomes(g)
    with pytest.raises(RuntimeError, match=r"driven step: policy 5 \(genome drivers\) runs in a launch of its own"):
        env.step_driven(5)
    env.set_rollout_streams(0)
    with pytest.raises(RuntimeError, match=r"the fused rollout kernel has no genome drivers \(policy 5\)"):
        env.rollout(5, 2)
    env.set_rollout_streams(4)
    env.set_rollout_pipe(2)
    with pytest.raises(RuntimeError, match=r"the pipelined rollout has no genome drivers \(policy 5\)"):
        env.rollout(5, 2)
    env.set_rollout_pipe(0)
    env.set_car_controllers(["genome", "rule", "rule"])
    env.set_genomes(None)
    with pytest.raises(RuntimeError, match=r"a genome slot of the field needs a genome table"):
        env.policy_actions(4)
    with pytest.raises(RuntimeError, match=r"no fitness accumulators"):
        env.fitness()
    env.set_fitness(True)
    with pytest.raises(RuntimeError, match=r"fitness accumulation \(nascar_set_fitness\) needs auto_reset = 0"):
        env.rollout(1, 2, auto_reset=True)
    env.set_fitness(False)
    env.rollout(1, 2, auto_reset=True)        # off again: nothing changes for existing callers
    env.close()


def test_evaluate_equals_per_track_evaluation():
    """25 genomes (not a multiple of 10) on two tracks in one engine == one engine per track, padding dropped"""
    tracks, S = ["daytona", "martinsville"], 400
    g = G.random_genomes(np.random.default_rng(12), 25)
    res = G.evaluate(g, [_track(t) for t in tracks], max_steps=S, device="cuda:0")
    assert res["per_track"].shape == (2, 25, 8) and res["fitness"].shape == (25,) and res["tracks"] == tracks
    per, table = G.layout(g, 1)
    fitness = np.zeros(25)
    for t, name in enumerate(tracks):
        env = _engine(per, 10, name)
        env.set_genomes(table)
        env.reset()
        env.set_fitness(True)
        env.rollout(5, S, auto_reset=False)
        rows = env.fitness().cpu().numpy().reshape(per * 10, 8)[:25]
        env.close()
        assert np.array_equal(_bits(res["per_track"][t]), _bits(rows)), name
        fitness = fitness + rows[:, 0] * G.TRACK_MULTIPLIERS[name] if t else rows[:, 0] * G.TRACK_MULTIPLIERS[name]
    assert np.array_equal(_bits(res["fitness"]), _bits(fitness))
    assert np.all(res["steps"] == 2 * S) and res["fitness"].std() > 0


def test_trainer_runs_and_is_deterministic():
    def run():
        t = G.GeneticTrainer(population_size=20, generations=2, seed=1, max_steps=300, device="cuda:0",
                             tracks=("daytona", "martinsville", "michigan"))
        best, fit = t.train()
        return t, best, fit
    t, best, fit = run()
    assert len(t.evaluated) == 2 and len(t.fitness_history) == 2 and best.shape == (12,)
    assert fit == max(f.max() for f in t.evaluated) == max(h["best_fitness"] for h in t.fitness_history)
    t2, best2, fit2 = run()
    assert fit2 == fit and np.array_equal(best, best2) and np.array_equal(t.population, t2.population)
    assert all(np.array_equal(x, y) for x, y in zip(t.evaluated, t2.evaluated))

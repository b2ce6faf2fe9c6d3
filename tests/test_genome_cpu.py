"""Genome driver and GA operators on the host (no GPU): the restatement tests/genome_ref.py against the suite's rule
driver, the one numeric case policy 1 can never reach (a steering the clamp turned into a Python int), the vectorised
operators of nascargymnasium_amd/genetic.py, and the three new ABI symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

from drivers import RuleDriver
from genome_ref import Float32GenomeDriver, GenomeDriver, drive, synthetic_case
from golden_replay import GOLDEN

from nascargymnasium_amd import genetic as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("nascar_set_genomes", "nascar_set_fitness", "nascar_get_fitness")


def test_constants_restate_the_reference():
    assert len(G.GENOME_NAMES) == 12 and G.GENOME_BOUNDS.shape == (12, 2)
    assert G.DEFAULT_GENOME[10] == 0.8 and G.RULE_GENOME[10] == 1.0
    assert G.DEFAULT_GENOME[:10] == G.RULE_GENOME[:10] and G.DEFAULT_GENOME[11] == G.RULE_GENOME[11]
    for g in (G.DEFAULT_GENOME, G.RULE_GENOME):
        assert np.all(np.asarray(g) >= G.GENOME_BOUNDS[:, 0]) and np.all(np.asarray(g) <= G.GENOME_BOUNDS[:, 1])
    assert sorted(G.TRACK_MULTIPLIERS) == sorted(G.TRACKS) and len(G.TRACKS) == 8
    from nascargymnasium_amd import available_tracks
    assert sorted(G.track_name(t) for t in available_tracks()) == sorted(G.TRACKS)


@pytest.mark.parametrize("trace", ["env_talladega_10car", "env_martinsville_lap"])
def test_rule_genome_is_the_rule_driver(trace):
    """RULE_GENOME turns the restatement into BaseController._fallback_control: equal to the suite's RuleDriver on every
    step's observations of a golden trace -- actions and all four state values, bit for bit."""
    d = np.load(os.path.join(GOLDEN, trace + ".npz"))
    obs = np.concatenate([d["obs0"][None], d["obs"]])
    assert len(d["obs_steps"]) == len(d["rewards"])          # every step's observation is in the fixture
    C = obs.shape[1]
    rule = RuleDriver(C)
    gen = [GenomeDriver(G.RULE_GENOME) for _ in range(C)]
    for k in range(len(obs)):
        a = rule(obs[k])
        b = drive(gen, obs[k])
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), k
        ctl = np.stack([g.ctl() for g in gen])
        want = np.stack([rule.tb, rule.steer.astype(np.float64), rule.last.astype(np.float64),
                         rule.lim.astype(np.float64)], 1)
        assert np.array_equal(ctl.view(np.uint64), want.view(np.uint64)), k


def _obs(speed, forward, left, right):
    o = np.zeros(38, np.float32)
    o[4], o[22], o[23], o[37] = speed, forward, left, right
    return o


def test_saturated_steering_is_a_python_number_on_the_next_tie():
    """g[4] = 3 saturates the clamp (steering becomes the int 1); on the following exact tie steering *= g[6] is a
    float64 product compared with the float64 g[7].  The directed genome has g[6] one float64 ulp above g[7]: float64
    sees 1 * g[6] > g[7] and halves the throttle; an all-float32 evaluation rounds both to the same float32 and does
    not."""
    g7 = 0.3
    g6 = float(np.nextafter(np.float64(g7), 1.0))            # > g7 in float64, == g7 after rounding to float32
    assert g6 > g7 and np.float32(g6) == np.float32(g7)
    genome = [0.95, 1.05, 0.1, 0.1, 3.0, 0.5, g6, g7, 1, 1, 1.0, 0.3]
    seq = [_obs(0.0, 1.0, 0.01, 0.9),      # (1 - l/r) * 3 > 1: the clamp returns the int 1
           _obs(0.0, 1.0, 0.5, 0.5)]       # exact tie
    ref, f32 = GenomeDriver(genome), Float32GenomeDriver(genome)
    a0, b0 = ref.control(seq[0]), f32.control(seq[0])
    assert ref.control_state["steering"] == 1 and isinstance(ref.control_state["steering"], int)
    assert np.array_equal(a0, b0) and a0[1] == 1.0
    a1, b1 = ref.control(seq[1]), f32.control(seq[1])
    assert isinstance(ref.control_state["steering"], float) and ref.control_state["steering"] == g6
    # float64: |steering| > g[7] halves the throttle; float32: it does not
    assert ref.control_state["throttle_brake"] != f32.control_state["throttle_brake"]
    assert a1[0] != b1[0]
    # a step that is no tie makes the steering float32 again
    ref.control(_obs(0.0, 1.0, 0.4, 0.5))
    assert isinstance(ref.control_state["steering"], np.float32)


def test_python_number_path_changes_actions_within_the_bounds():
    """within GENOME_BOUNDS too: on the directed sequences of the GPU test the all-float32 driver differs from the
    restatement in some action, and every edge the sequences aim at is hit"""
    g, obs, counts = synthetic_case(130, 64, 3, G.GENOME_BOUNDS)
    assert np.all(g >= G.GENOME_BOUNDS[:, 0]) and np.all(g <= G.GENOME_BOUNDS[:, 1])
    assert all(v > 0 for v in counts.values()), counts
    ref = [GenomeDriver(x) for x in g]
    f32 = [Float32GenomeDriver(x) for x in g]
    differ = 0
    for k in range(len(obs)):
        differ += int((drive(ref, obs[k]).view(np.uint32) != drive(f32, obs[k]).view(np.uint32)).sum())
    assert differ > 0


def test_operators_bounds_and_determinism():
    lo, hi = G.GENOME_BOUNDS[:, 0], G.GENOME_BOUNDS[:, 1]
    pop = G.random_genomes(np.random.default_rng(4), 200)
    assert pop.shape == (200, 12) and pop.dtype == np.float64 and np.all(pop >= lo) and np.all(pop <= hi)
    m = G.mutate(np.random.default_rng(5), pop, rate=0.5, strength=2.0)     # strength 2: most moves leave the bounds
    assert np.all(m >= lo) and np.all(m <= hi)
    moved = m != pop
    assert 0.3 < moved.mean() < 0.6                     # ~rate of the genes moved, the others untouched
    assert np.array_equal(G.mutate(np.random.default_rng(5), pop, rate=0.0, strength=2.0), pop)
    c1, c2 = G.crossover(np.random.default_rng(6), pop[:100], pop[100:], rate=0.5)
    took_b = c1 == pop[100:]
    assert np.array_equal(np.where(took_b, pop[100:], pop[:100]), c1)
    assert np.array_equal(np.where(took_b, pop[:100], pop[100:]), c2) and 0.4 < took_b.mean() < 0.6
    k1, k2 = G.crossover(np.random.default_rng(6), pop[:100], pop[100:], rate=0.0)
    assert np.array_equal(k1, pop[:100]) and np.array_equal(k2, pop[100:])
    for f, args in ((G.random_genomes, (50,)), (G.mutate, (pop, 0.3, 0.2))):
        assert np.array_equal(f(np.random.default_rng(9), *args), f(np.random.default_rng(9), *args))


def test_generation_step_keeps_the_elite_and_is_deterministic():
    def run(seed):
        t = G.GeneticTrainer(population_size=23, generations=1, seed=seed)
        pop = t.population.copy()
        fit = np.random.default_rng(1).normal(size=23)
        return t, pop, fit, t.evolve(fit).copy()
    t, pop, fit, new = run(3)
    assert t.elite_count == 4 and new.shape == pop.shape
    elite = pop[np.argsort(fit)[-4:]]
    assert np.array_equal(new[:4], elite)
    assert t.best_fitness == fit.max() and np.array_equal(t.best_individual, pop[np.argmax(fit)])
    assert t.fitness_history == [{"generation": 0, "best_fitness": float(fit.max()), "avg_fitness": float(fit.mean()),
                                  "std_fitness": float(fit.std())}]
    assert np.all(new >= G.GENOME_BOUNDS[:, 0]) and np.all(new <= G.GENOME_BOUNDS[:, 1])
    assert np.array_equal(run(3)[3], new) and not np.array_equal(run(4)[3], new)


def test_layout_pads_with_the_rule_genome():
    g = G.random_genomes(np.random.default_rng(0), 25)
    per, table = G.layout(g, 2)
    assert per == 3 and table.shape == (60, 12)
    for t in range(2):
        assert np.array_equal(table[30 * t:30 * t + 25], g)
        assert np.array_equal(table[30 * t + 25:30 * t + 30], np.tile(np.asarray(G.RULE_GENOME, np.float64), (5, 1)))


def test_header_binding_and_library_agree_on_the_new_symbols():
    from nascargymnasium_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    hdr = open(os.path.join(ROOT, "include", "nascar.h")).read()
    declared = set(re.findall(r"\b(nascar_[a-z0-9_]+)\s*\(", hdr))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for sym in NEW_SYMBOLS:
        assert sym in declared and sym in _lib.EXPORTED and hasattr(L, sym), sym
    assert re.search(r"#define\s+NASCAR_CTRL_GENOME\s+\(-4\)", hdr) and _lib.CTRL_BUILTIN["genome"] == -4
    assert _lib.FITNESS_FIELDS == ["total_reward", "distance_traveled", "max_speed", "time_on_track", "lap_completed",
                                   "lap_time", "steps", "disabled_at_step"]

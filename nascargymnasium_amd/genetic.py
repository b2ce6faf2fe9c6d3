"""Genetic-algorithm training of the rule driver on the device: the reference's learn/genetic_trainer.py and the
genome operators of game/control/genetic_controller.py, with the evaluation of a whole population as ONE rollout.

The reference evaluates 10 individuals per CarEnv, one env at a time, with a Python `control()` per car and step and a
Python metrics loop over `info`.  Here P genomes become ceil(P / 10) envs of 10 cars per track, all tracks of the pair
in one engine; the genome driver is device action source 5 (BatchedCarEnv.set_genomes) and the per-individual metrics
are accumulated on the device during the rollout (BatchedCarEnv.set_fitness), so an evaluation is one reset, one
`rollout(5, max_steps, auto_reset=False)` and one `fitness()` read.

The driver's semantics are BaseController._fallback_control with its constants replaced by genes (include/nascar.h):
GeneticController.control itself cannot run as written.  Genes 8, 9 and 11 are carried through the operators and
unused by the driver.

No plotting, no checkpoint files, no prints.
"""
import numpy as np

from . import _lib

# GeneticController.default_genome's order (game/control/genetic_controller.py:32-45, 162-175)
GENOME_NAMES = ("speed_lower_multiplier", "speed_upper_multiplier", "throttle_increment", "brake_increment",
                "steering_sensitivity", "throttle_reduction_when_steering", "steering_decay_rate",
                "max_steering_for_throttle_reduction", "left_sensor_weight", "right_sensor_weight",
                "collision_avoidance_threshold", "emergency_brake_threshold")
GENOME_BOUNDS = np.array([(0.70, 0.99), (1.01, 1.30), (0.01, 0.30), (0.01, 0.30), (0.10, 3.00), (0.10, 0.90),
                          (0.70, 0.99), (0.10, 0.50), (0.50, 2.00), (0.50, 2.00), (0.50, 1.00), (0.05, 0.50)], np.float64)
DEFAULT_GENOME = (0.95, 1.05, 0.10, 0.10, 1.00, 0.50, 0.90, 0.25, 1.00, 1.00, 0.80, 0.30)
# the genome under which the driver IS BaseController._fallback_control (device policy 1), bit for bit: the default
# genome with collision_avoidance_threshold 1.0
RULE_GENOME = (0.95, 1.05, 0.1, 0.1, 1.0, 0.5, 0.9, 0.25, 1, 1, 1.0, 0.3)
# GeneticTrainer._calculate_fitness (learn/genetic_trainer.py:98-107)
TRACK_MULTIPLIERS = {"daytona": 0.79, "talladega": 0.74, "martinsville": 2.07, "michigan": 0.77, "trioval": 0.98,
                     "nascar_banked": 0.74, "nascar2": 1.0, "nascar": 0.8}
TRACKS = ("daytona", "martinsville", "michigan", "trioval", "nascar2", "nascar_banked", "nascar", "talladega")
CARS_PER_ENV = 10          # evaluate_population's batch size
N_GENES = len(GENOME_NAMES)


def random_genomes(rng: np.random.Generator, n: int) -> np.ndarray:
    """GeneticController.random_genome x n: uniform within the bounds, [n, 12] float64."""
    return rng.uniform(GENOME_BOUNDS[:, 0], GENOME_BOUNDS[:, 1], size=(int(n), N_GENES))


def crossover(rng: np.random.Generator, a, b, rate: float = 0.5):
    """GeneticController.crossover, vectorised over pairs: every gene swaps between the parents with probability
    `rate`.  a, b: [..., 12]; returns the two children."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    swap = rng.random(a.shape) < rate
    return np.where(swap, b, a), np.where(swap, a, b)


def mutate(rng: np.random.Generator, g, rate: float = 0.1, strength: float = 0.1) -> np.ndarray:
    """GeneticController.mutate, vectorised: with probability `rate` per gene, gene += U(-strength, strength) * gene,
    clamped to the gene's bounds (only mutated genes are clamped, as in the reference)."""
    g = np.asarray(g, np.float64)
    hit = rng.random(g.shape) < rate
    noise = rng.uniform(-strength, strength, size=g.shape) * g
    moved = np.clip(g + noise, GENOME_BOUNDS[:, 0], GENOME_BOUNDS[:, 1])
    return np.where(hit, moved, g)


def track_name(track: str) -> str:
    return str(track).split("/")[-1].replace(".track", "")


def layout(genomes, n_tracks: int):
    """(envs per track, the engine's genome table [n_tracks * envs * 10, 12]): the P genomes fill the first P car slots
    of each track's envs; the slots past P get RULE_GENOME."""
    g = np.asarray(genomes, np.float64).reshape(-1, N_GENES)
    per = -(-g.shape[0] // CARS_PER_ENV)
    pad = np.tile(np.asarray(RULE_GENOME, np.float64), (per * CARS_PER_ENV, 1))
    pad[:g.shape[0]] = g
    return per, np.tile(pad, (n_tracks, 1))


def evaluate(genomes, tracks, max_steps: int = 9999, device="cuda", env=None):
    """GeneticTrainer._evaluate_batch for a whole population at once.  genomes [P, 12]; tracks: the track names (the
    reference uses a pair).  One engine of len(tracks) * ceil(P / 10) envs x 10 cars (`env`: one of that shape to reuse,
    e.g. across generations), one reset, one rollout of `max_steps` steps without auto-reset, one fitness read.
    Returns a dict of numpy arrays per individual, combined over the tracks as _evaluate_batch combines them
    (fitness = sum of total_reward x TRACK_MULTIPLIERS[track]; rewards, distances, times and steps summed, max_speed
    the maximum, lap_time the running pairwise mean), plus "per_track" [len(tracks), P, 8] (BatchedCarEnv.FITNESS_FIELDS)."""
    from .batched import BatchedCarEnv
    g = np.asarray(genomes, np.float64).reshape(-1, N_GENES)
    P, T = g.shape[0], len(tracks)
    if P < 1 or T < 1:
        raise ValueError("need at least one genome and one track")
    per, table = layout(g, T)
    files = [t for t in tracks for _ in range(per)]
    own = env is None
    if own:
        env = BatchedCarEnv(T * per, CARS_PER_ENV, files, device=device)
    elif (env.E, env.C) != (T * per, CARS_PER_ENV):
        raise ValueError(f"env must be {T * per} x {CARS_PER_ENV}, got {env.E} x {env.C}")
    else:
        env.set_env_tracks(files)
    try:
        env.set_genomes(table)
        env.reset()
        env.set_fitness(True)
        env.rollout(5, int(max_steps), auto_reset=False)
        fit = env.fitness().cpu().numpy().reshape(T, per * CARS_PER_ENV, _lib.N_FITNESS)[:, :P]
        env.set_fitness(False)
    finally:
        if own:
            env.close()
    return combine(fit, tracks)


def combine(fit, tracks):
    """per-track fitness rows [T, P, 8] -> the per-individual result of GeneticTrainer._evaluate_batch"""
    F = {f: i for i, f in enumerate(_lib.FITNESS_FIELDS)}
    mult = np.array([TRACK_MULTIPLIERS.get(track_name(t), 1.0) for t in tracks], np.float64)
    out = {"total_reward": fit[0, :, F["total_reward"]].copy(),
           "distance_traveled": fit[0, :, F["distance_traveled"]].copy(),
           "max_speed": fit[0, :, F["max_speed"]].copy(),
           "time_on_track": fit[0, :, F["time_on_track"]].copy(),
           "lap_completed": fit[0, :, F["lap_completed"]] != 0,
           "lap_time": fit[0, :, F["lap_time"]].copy(),
           "steps": fit[0, :, F["steps"]].astype(np.int64),
           "fitness": fit[0, :, F["total_reward"]] * mult[0]}
    for t in range(1, fit.shape[0]):
        out["total_reward"] += fit[t, :, F["total_reward"]]
        out["distance_traveled"] += fit[t, :, F["distance_traveled"]]
        out["max_speed"] = np.maximum(out["max_speed"], fit[t, :, F["max_speed"]])
        out["time_on_track"] += fit[t, :, F["time_on_track"]]
        out["lap_completed"] |= fit[t, :, F["lap_completed"]] != 0
        a, b = out["lap_time"], fit[t, :, F["lap_time"]]
        out["lap_time"] = np.where(np.isnan(a), b, np.where(np.isnan(b), a, (a + b) / 2.0))
        out["steps"] += fit[t, :, F["steps"]].astype(np.int64)
        out["fitness"] += fit[t, :, F["total_reward"]] * mult[t]
    out["per_track"] = fit.copy()
    out["tracks"] = [track_name(t) for t in tracks]
    return out


class GeneticTrainer:
    """learn/genetic_trainer.py GeneticTrainer with the reference's defaults and generation step (elite, tournament of
    3, crossover, mutation), evaluating each generation with `evaluate` on two distinct bundled tracks drawn for that
    generation.  All randomness comes from one np.random.Generator(seed)."""

    def __init__(self, population_size: int = 50, generations: int = 100, mutation_rate: float = 0.15,
                 mutation_strength: float = 0.2, crossover_rate: float = 0.7, elite_ratio: float = 0.2, seed: int = 0,
                 max_steps: int = 9999, device="cuda", tracks=TRACKS):
        self.population_size, self.generations = int(population_size), int(generations)
        self.mutation_rate, self.mutation_strength = float(mutation_rate), float(mutation_strength)
        self.crossover_rate, self.elite_ratio = float(crossover_rate), float(elite_ratio)
        self.elite_count = max(1, int(self.population_size * self.elite_ratio))
        self.max_steps, self.device = int(max_steps), device
        self.tracks = tuple(tracks)              # the pool each generation's pair is drawn from (default: all 8)
        if len(self.tracks) < 2:
            raise ValueError("need at least two tracks to draw a pair from")
        self.rng = np.random.default_rng(seed)
        self.population = random_genomes(self.rng, self.population_size)
        self.fitness_history = []
        self.best_individual, self.best_fitness = None, -np.inf
        self.generation = 0
        self.last_results = None
        self.evaluated = []          # per generation: the fitness array that generation's population was given

    def selection(self, fitness) -> np.ndarray:
        """population_size - elite_count tournament winners (3 distinct candidates each)"""
        n = self.population_size - self.elite_count
        k = min(3, len(fitness))
        winners = np.empty(n, np.int64)
        for i in range(n):
            cand = self.rng.choice(len(fitness), k, replace=False)
            winners[i] = cand[np.argmax(fitness[cand])]
        return winners

    def evolve(self, fitness) -> np.ndarray:
        """GeneticTrainer.evolve_generation: records the best, keeps the elite, fills up with mutated children"""
        fitness = np.asarray(fitness, np.float64)
        best = int(np.argmax(fitness))
        if fitness[best] > self.best_fitness:
            self.best_fitness = float(fitness[best])
            self.best_individual = self.population[best].copy()
        self.fitness_history.append({"generation": int(self.generation), "best_fitness": float(fitness.max()),
                                     "avg_fitness": float(fitness.mean()), "std_fitness": float(fitness.std())})
        new = [self.population[i].copy() for i in np.argsort(fitness, kind="stable")[-self.elite_count:]]
        parents = self.selection(fitness)
        while len(new) < self.population_size:
            p1, p2 = self.population[self.rng.choice(parents)], self.population[self.rng.choice(parents)]
            if self.rng.random() < self.crossover_rate:
                c1, c2 = crossover(self.rng, p1, p2)
            else:
                c1, c2 = p1.copy(), p2.copy()
            new.append(mutate(self.rng, c1, self.mutation_rate, self.mutation_strength))
            if len(new) < self.population_size:
                new.append(mutate(self.rng, c2, self.mutation_rate, self.mutation_strength))
        self.population = np.stack(new[:self.population_size])
        return self.population

    def train(self):
        """`generations` x (draw two tracks, evaluate, evolve); returns (best_genome, best_fitness)"""
        from .batched import BatchedCarEnv
        per = -(-self.population_size // CARS_PER_ENV)
        env = None
        try:
            for self.generation in range(self.generations):
                pair = [self.tracks[i] for i in self.rng.choice(len(self.tracks), 2, replace=False)]
                if env is None:
                    env = BatchedCarEnv(2 * per, CARS_PER_ENV, [t for t in pair for _ in range(per)], device=self.device)
                self.last_results = evaluate(self.population, pair, self.max_steps, env=env)
                self.evaluated.append(self.last_results["fitness"].copy())
                self.evolve(self.last_results["fitness"])
        finally:
            if env is not None:
                env.close()
        return self.best_individual, self.best_fitness

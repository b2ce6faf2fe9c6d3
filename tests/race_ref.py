"""CPU restatement of the reference's race modes, line by line, for the tests of the device race ledger.

The reference's game/*.py needs pygame, Box2D and SB3 to import, so its loops are restated here on plain Python values:
  competition.py:37-81    calculate_finishing_order   (championship.py:200-246 is the same function)
  competition.py:319-388  the per-step reward and lap loop of a race      (championship.py:505-560)
  competition.py:395-424  the race ends after the step with terminated or truncated; final_lap_counts from that info
  time_trial.py:246-388   an attempt: parked cars, the lap loop, disabled cars finish, all finished ends it
  championship.py:28-29   TIME_TRIAL_POINTS, COMPETITION_POINTS, FASTEST_LAP_BONUS
  championship.py:44-134  ChampionshipManager
Python's own sorted() on the reference's key tuples gives the order; rewards are np.float32 sums (car_rewards[i] = 0.0;
car_rewards[i] += reward[i] is np.float32 from the first add under NumPy 2); lap times and simulation_time stay floats.
None is None here; the ledger rows of the device (BatchedCarEnv.RACE_FIELDS) hold NaN for it.
"""
import math

import numpy as np

TIME_TRIAL_POINTS = [15, 7, 3]
COMPETITION_POINTS = [0, 1, 2, 3, 5, 8, 13, 21, 24, 45]
FASTEST_LAP_BONUS = 15
RACE_FIELDS = ["lap_count", "laps_timed", "attempt_laps", "best_lap", "last_lap", "finish_time", "total_reward",
               "disabled", "parked", "steps"]
F = {f: i for i, f in enumerate(RACE_FIELDS)}


def none_if_nan(x):
    x = float(x)
    return None if math.isnan(x) else x


def competition_order(laps, finish_time, best_time, reward, disabled):
    """calculate_finishing_order (competition.py:37-81): the car indices in finishing order"""
    results = [(i, laps[i], best_time[i], finish_time[i], reward[i], bool(disabled[i])) for i in range(len(laps))]

    def sort_key(result):
        _, laps_, best, finish, rew, dis = result
        return (-laps_, finish if finish else 999999, best if best else 999999, -rew, dis)

    results.sort(key=sort_key)
    return [r[0] for r in results]


def competition_points(order, fastest_lap_car):
    """calculate_competition_points (championship.py:89-120): points per car index"""
    pts = {}
    for position, car in enumerate(order):
        idx = min(position, len(COMPETITION_POINTS) - 1)
        pts[car] = COMPETITION_POINTS[-(idx + 1)]
    if fastest_lap_car is not None:
        pts[fastest_lap_car] = pts.get(fastest_lap_car, 0) + FASTEST_LAP_BONUS
    return [pts[c] for c in range(len(order))]


def time_trial_order(best_time):
    """the time trial's order: sorted by `best or 999999` (championship.py:68 with the competition's truthiness, so a 0.0
    best counts as none as everywhere else in the reference's keys).  championship.py:68 itself tests `is not None`, and
    ChampionshipDict below restates it so; the two agree on every ledger a race can produce, because a best lap is only
    ever taken from a truthy last_lap_time and so is never 0.0.  They differ only on a hand-made best of 0.0, which the
    device ranks as this function does (include/nascar.h says so)."""
    return sorted(range(len(best_time)), key=lambda i: best_time[i] if best_time[i] else 999999)


def time_trial_points(order, best_time):
    """calculate_time_trial_points (championship.py:65-87): positions 0-2 that have a best lap"""
    pts = [0] * len(order)
    for position, car in enumerate(order):
        if position < len(TIME_TRIAL_POINTS) and best_time[car]:
            pts[car] = TIME_TRIAL_POINTS[position]
    return pts


def rank_ledger(ledger, fastest_car, mode):
    """order, position, points [E, C] int32 of ledger rows [E, C, 10] (NaN: None), fastest_car [E] (-1 or None: none)"""
    ledger = np.asarray(ledger, np.float64)
    E, C = ledger.shape[:2]
    order = np.zeros((E, C), np.int32)
    position = np.zeros((E, C), np.int32)
    points = np.zeros((E, C), np.int32)
    for e in range(E):
        row = ledger[e]
        best = [none_if_nan(x) for x in row[:, F["best_lap"]]]
        if mode == 1:
            o = competition_order([float(x) for x in row[:, F["lap_count"]]], [none_if_nan(x) for x in row[:, F["finish_time"]]],
                                  best, [float(x) for x in row[:, F["total_reward"]]], row[:, F["disabled"]] != 0)
            fc = None if fastest_car is None or int(fastest_car[e]) < 0 else int(fastest_car[e])
            p = competition_points(o, fc)
        else:
            o = time_trial_order(best)
            p = time_trial_points(o, best)
        order[e] = o
        position[e, o] = np.arange(C)
        points[e] = p
    return order, position, points


class EnvRace:
    """The reference's per-step bookkeeping of one env of C cars.  step() takes what env.step returned: reward [C], the
    cars' (lap_count, last_lap_time or None, disabled, simulation_time) and terminated-or-truncated."""

    def __init__(self, C, mode, laps_per_attempt=2):
        self.C, self.mode, self.laps_per_attempt = C, mode, laps_per_attempt
        self.best = [None] * C
        self.laps_timed = [0] * C
        self.overall_best, self.fastest_car = None, None
        self.begin(False)

    def begin(self, keep_records):
        C = self.C
        if not keep_records:
            self.best = [None] * C
            self.laps_timed = [0] * C
            self.overall_best, self.fastest_car = None, None
        self.rewards = [0.0] * C          # car_rewards[i] = 0.0
        self.prev = [0] * C
        self.attempt_laps = [0] * C
        self.last = [None] * C
        self.finish = [None] * C
        self.lap_count = [0] * C
        self.disabled = [False] * C
        self.finished = set()             # cars_finished_attempt
        self.steps = [0] * C
        self.ended = False

    def parked(self):
        """the cars whose controller the time trial does not call this step (time_trial.py:278-280)"""
        return [c in self.finished for c in range(self.C)]

    def step(self, reward, lap_count, last_lap, disabled, sim_time, env_done):
        if self.ended:
            return
        C = self.C
        for c in range(C):
            self.rewards[c] += np.float32(reward[c])
            self.steps[c] += 1
        for c in range(C):
            if self.mode == 2 and c in self.finished:
                continue
            self.lap_count[c] = int(lap_count[c])
            self.disabled[c] = bool(disabled[c])
            if lap_count[c] > self.prev[c]:
                t = last_lap[c]
                if t:
                    self.last[c] = t
                    self.laps_timed[c] += 1
                    self.attempt_laps[c] += 1
                    self.finish[c] = sim_time
                    if self.best[c] is None or t < self.best[c]:
                        self.best[c] = t
                    if self.overall_best is None or t < self.overall_best:
                        self.overall_best, self.fastest_car = t, c
                    if self.mode == 2 and self.attempt_laps[c] >= self.laps_per_attempt:
                        self.finished.add(c)
                self.prev[c] = int(lap_count[c])
        if self.mode == 2:
            for c in range(C):
                if disabled[c] and c not in self.finished:
                    self.finished.add(c)
            self.ended = len(self.finished) >= C
        else:
            self.ended = bool(env_done)

    def rows(self):
        """the env's ledger rows [C, 10] (NaN: None)"""
        nan = lambda x: float("nan") if x is None else float(x)
        out = np.zeros((self.C, len(RACE_FIELDS)), np.float64)
        for c in range(self.C):
            out[c] = [self.lap_count[c], self.laps_timed[c], self.attempt_laps[c], nan(self.best[c]), nan(self.last[c]),
                      nan(self.finish[c]), float(self.rewards[c]), float(self.disabled[c]), float(c in self.finished),
                      self.steps[c]]
        return out


class ChampionshipDict:
    """ChampionshipManager (championship.py:44-134) on plain dicts, for one replica"""

    def __init__(self, num_cars):
        self.num_cars = num_cars
        self.championship_points = {i: 0 for i in range(num_cars)}
        self.stats = {"time_trial_wins": {i: 0 for i in range(num_cars)},
                      "competition_wins": {i: 0 for i in range(num_cars)},
                      "time_trial_podiums": {i: {"2nd": 0, "3rd": 0} for i in range(num_cars)},
                      "competition_podiums": {i: {"2nd": 0, "3rd": 0} for i in range(num_cars)},
                      "fastest_laps": {i: 0 for i in range(num_cars)}}

    def calculate_time_trial_points(self, best_times):
        results = [(i, best_times[i]) for i in range(self.num_cars)]
        sorted_results = sorted(results, key=lambda x: x[1] if x[1] is not None else 999999)
        for position, (car, best) in enumerate(sorted_results):
            if position < len(TIME_TRIAL_POINTS) and best is not None:
                self.championship_points[car] += TIME_TRIAL_POINTS[position]
                if position == 0:
                    self.stats["time_trial_wins"][car] += 1
                elif position == 1:
                    self.stats["time_trial_podiums"][car]["2nd"] += 1
                elif position == 2:
                    self.stats["time_trial_podiums"][car]["3rd"] += 1
        return [c for c, _ in sorted_results]

    def calculate_competition_points(self, finishing_order, fastest_lap_car):
        for position, car in enumerate(finishing_order):
            idx = min(position, len(COMPETITION_POINTS) - 1)
            self.championship_points[car] += COMPETITION_POINTS[-(idx + 1)]
            if position == 0:
                self.stats["competition_wins"][car] += 1
            elif position == 1:
                self.stats["competition_podiums"][car]["2nd"] += 1
            elif position == 2:
                self.stats["competition_podiums"][car]["3rd"] += 1
        if fastest_lap_car is not None:
            self.championship_points[fastest_lap_car] += FASTEST_LAP_BONUS
            self.stats["fastest_laps"][fastest_lap_car] += 1

    def get_championship_standings(self):
        standings = [(c, self.championship_points[c]) for c in range(self.num_cars)]
        standings.sort(key=lambda x: x[1], reverse=True)
        return standings

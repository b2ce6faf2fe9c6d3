"""The reference's race modes (game/time_trial.py, game/competition.py, game/championship.py) on the device.

The field is whatever the engine's action source drives (policy 4: `set_car_controllers`, with per-env genomes for its
genome slots; policy 2 / 5 likewise).  The per-step bookkeeping the reference's loops do on the host -- reward sums, lap
events, best and fastest laps, finishing times, parked cars -- is the engine's race ledger (`BatchedCarEnv.set_race`),
the finishing order and points its rank kernel (`race_rank`), so a stage is a handful of `rollout` calls and one read:

    competition(env)     one race per env, until the env terminates or truncates       (game/competition.py:239-424)
    time_trial(env)      `attempts` x (reset, every car times `laps` laps or is disabled)  (game/time_trial.py:222-420)
    championship(env, tracks)   per track a time-trial stage, then a competition stage (game/championship.py:721-748),
                         T tracks x R replicas of the field in one engine, points added up in a ChampionshipTable

Results are numpy arrays per env.  No rendering, no printing, no files.  Every function begins its own race
(`race_begin`), so whatever the env's ledger held before is overwritten; the race mode the env had on entry (off, by
default) is set again on return.
"""
import numpy as np

from . import _lib

TIME_TRIAL_POINTS = [15, 7, 3]                           # game/championship.py:28
COMPETITION_POINTS = [0, 1, 2, 3, 5, 8, 13, 21, 24, 45]  # game/championship.py:29, last place to first
FASTEST_LAP_BONUS = 15
TOTAL_ATTEMPTS, LAPS_PER_ATTEMPT = 3, 2                  # game/time_trial.py
PARKING_POLICIES = (2, 4, 5)                             # the rollout's action sources that write an action buffer
DEFAULT_CHUNK = 512

_F = {f: i for i, f in enumerate(_lib.RACE_FIELDS)}


def _check_run(policy, max_steps, chunk, parking):
    if int(max_steps) < 1:
        raise ValueError(f"max_steps must be >= 1, got {max_steps}")
    if int(chunk) < 1:
        raise ValueError(f"chunk must be >= 1, got {chunk}")
    if parking and int(policy) not in PARKING_POLICIES:
        raise ValueError(f"a time trial parks cars through the rollout's action buffer: policy must be one of "
                         f"{PARKING_POLICIES}, got {policy}")
    if int(policy) not in (0, 1, 2, 3, 4, 5):
        raise ValueError(f"policy must be a rollout action source (0-5), got {policy}")


def _run(env, policy, max_steps, chunk, seed, step0):
    """rollout in chunks until no env is racing (one device count per chunk) or the step cap; returns the steps run"""
    done = 0
    while done < max_steps:
        k = min(int(chunk), max_steps - done)
        env.rollout(policy, k, seed=seed, step0=step0 + done, auto_reset=False)
        done += k
        if env.race_racing() == 0:
            break
    return done


def _result(env, mode, steps):
    led, fastest_car, ended = env.race()
    rank = env.race_rank(mode)
    led = led.cpu().numpy()
    out = {"order": rank.order.cpu().numpy(), "position": rank.position.cpu().numpy(), "points": rank.points.cpu().numpy(),
           "best_lap": led[:, :, _F["best_lap"]], "laps": led[:, :, _F["lap_count"]].astype(np.int64),
           "laps_timed": led[:, :, _F["laps_timed"]].astype(np.int64), "finish_time": led[:, :, _F["finish_time"]],
           "total_reward": led[:, :, _F["total_reward"]].astype(np.float32), "disabled": led[:, :, _F["disabled"]] != 0,
           "fastest_car": fastest_car.cpu().numpy(), "ended": ended.cpu().numpy() != 0, "steps": steps, "ledger": led}
    return out


def competition(env, policy=4, max_steps=100000, chunk=DEFAULT_CHUNK, seed=0):
    """One race per env (game/competition.py:239-424): reset, then steps until every env has terminated or truncated
    (its last step counted) or `max_steps`.  Returns a dict of numpy arrays: order [E, C] (the car at position p),
    position, points [E, C] (COMPETITION_POINTS by position, +15 for the env's fastest lap), best_lap, finish_time (NaN:
    none), laps (the final lap_count), laps_timed, total_reward (float32), disabled [E, C], fastest_car [E] (-1: none),
    ended [E], steps (run), ledger [E, C, 10] (BatchedCarEnv.RACE_FIELDS)."""
    _check_run(policy, max_steps, chunk, False)
    before = env.race_mode()
    env.set_race(_lib.RACE_COMPETITION)
    try:
        env.race_begin(False)
        env.reset()
        steps = _run(env, int(policy), int(max_steps), chunk, seed, 0)
        return _result(env, _lib.RACE_COMPETITION, steps)
    finally:
        env.set_race(*before)


def time_trial(env, policy=4, attempts=TOTAL_ATTEMPTS, laps=LAPS_PER_ATTEMPT, max_steps=50000, chunk=DEFAULT_CHUNK, seed=0):
    """`attempts` attempts (game/time_trial.py:222-420): each resets the envs and runs until every car of every env has
    timed `laps` laps in the attempt or is disabled -- such cars are parked: action (0, 0), controller not run -- or
    `max_steps`.  Best laps and lap totals persist across the attempts; the env's terminated / truncated flags are
    ignored.  Attempt a steps with step0 = a * max_steps.  Returns competition's dict: order by best lap, points
    [15, 7, 3] for the first three with a lap; steps is a list per attempt."""
    _check_run(policy, max_steps, chunk, True)
    if int(attempts) < 1 or int(laps) < 1:
        raise ValueError(f"attempts and laps must be >= 1, got {attempts} and {laps}")
    before = env.race_mode()
    env.set_race(_lib.RACE_TIME_TRIAL, int(laps))
    try:
        steps = []
        for a in range(int(attempts)):
            env.race_begin(keep_records=a > 0)
            env.reset()
            steps.append(_run(env, int(policy), int(max_steps), chunk, seed, a * int(max_steps)))
        return _result(env, _lib.RACE_TIME_TRIAL, steps)
    finally:
        env.set_race(*before)


class ChampionshipTable:
    """ChampionshipManager (game/championship.py:44-134) for R replicas of a field of C cars at once: points and the
    per-stage statistics as [R, C] integer arrays."""

    def __init__(self, replicas, cars):
        self.R, self.C = int(replicas), int(cars)
        z = lambda: np.zeros((self.R, self.C), np.int64)
        self.points = z()
        self.stats = {"time_trial_wins": z(), "time_trial_2nd": z(), "time_trial_3rd": z(), "competition_wins": z(),
                      "competition_2nd": z(), "competition_3rd": z(), "fastest_laps": z()}

    def _stage(self, order, points):
        order, points = np.asarray(order), np.asarray(points)
        if order.shape != (self.R, self.C) or points.shape != (self.R, self.C):
            raise ValueError(f"stage results must be [{self.R}, {self.C}], got {order.shape} and {points.shape}")
        return order, points

    def _podium(self, stage, order, awarded):
        r = np.arange(self.R)
        for p, name in enumerate(("wins", "2nd", "3rd")[:self.C]):
            np.add.at(self.stats[f"{stage}_{name}"], (r, order[:, p]), awarded[:, p].astype(np.int64))

    def add_time_trial(self, order, points):
        """calculate_time_trial_points (championship.py:65-87): a podium place counts only with a best lap, i.e. where
        the position scored"""
        order, points = self._stage(order, points)
        self.points += points
        self._podium("time_trial", order, np.take_along_axis(points, order, 1) > 0)

    def add_competition(self, order, points, fastest_car):
        """calculate_competition_points (championship.py:89-120); `points` already holds the fastest-lap bonus"""
        order, points = self._stage(order, points)
        fastest_car = np.asarray(fastest_car)
        if fastest_car.shape != (self.R,):
            raise ValueError(f"fastest_car must be [{self.R}], got {fastest_car.shape}")
        self.points += points
        self._podium("competition", order, np.ones((self.R, self.C), bool))
        has = fastest_car >= 0
        np.add.at(self.stats["fastest_laps"], (np.arange(self.R)[has], fastest_car[has]), 1)

    def standings(self):
        """get_championship_standings (championship.py:122-134): (cars [R, C], their points [R, C]) by points,
        descending and stable (equal points keep car order, as list.sort(reverse=True) does)"""
        cars = np.argsort(-self.points, axis=1, kind="stable")
        return cars, np.take_along_axis(self.points, cars, 1)


def championship_layout(tracks, replicas):
    """the track file of each env: track t's replicas are envs [t * replicas, (t + 1) * replicas)"""
    tracks = list(tracks)
    if not tracks or int(replicas) < 1:
        raise ValueError("need at least one track and one replica")
    return [t for t in tracks for _ in range(int(replicas))]


def championship(env, tracks, policy=4, attempts=TOTAL_ATTEMPTS, laps=LAPS_PER_ATTEMPT, time_trial_steps=50000,
                 competition_steps=100000, chunk=DEFAULT_CHUNK, seed=0):
    """game/championship.py:721-748 as a batch: `env` holds len(tracks) * R envs; track t is given to envs
    [t * R, (t + 1) * R) (set_env_tracks), so all tracks' time-trial stages run as one time_trial and all competition
    stages as one competition.  Replica r of every track adds into row r of the table, track by track, time trial
    before competition.  Per-env genomes, noisy slots and car contact / visibility are the env's own settings.
    Returns (ChampionshipTable, time-trial result, competition result), the results per env as above."""
    tracks = list(tracks)
    T = len(tracks)
    if T < 1 or env.E % T:
        raise ValueError(f"the env's {env.E} envs do not split over {T} tracks")
    _check_run(policy, time_trial_steps, chunk, True)
    _check_run(policy, competition_steps, chunk, False)
    R = env.E // T
    env.set_env_tracks(championship_layout(tracks, R))
    tt = time_trial(env, policy, attempts, laps, time_trial_steps, chunk, seed)
    comp = competition(env, policy, competition_steps, chunk, seed)
    table = ChampionshipTable(R, env.C)
    for t in range(T):
        e = slice(t * R, (t + 1) * R)
        table.add_time_trial(tt["order"][e], tt["points"][e])
        table.add_competition(comp["order"][e], comp["points"][e], comp["fastest_car"][e])
    return table, tt, comp

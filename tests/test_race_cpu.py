"""The race modes' CPU reference (tests/race_ref.py) on hand-made ledgers, ChampionshipTable against a plain-dict
ChampionshipManager, and the argument errors of nascargymnasium_amd.race that need no device."""
import numpy as np
import pytest

import race_ref
from race_ref import F

NAN = float("nan")


def _ledger(rows):
    """rows: per car (lap_count, finish_time, best_lap, total_reward, disabled) -> ledger [1, C, 10]"""
    led = np.zeros((1, len(rows), len(race_ref.RACE_FIELDS)))
    for c, (laps, fin, best, rew, dis) in enumerate(rows):
        led[0, c, F["lap_count"]] = laps
        led[0, c, F["finish_time"]] = NAN if fin is None else fin
        led[0, c, F["best_lap"]] = NAN if best is None else best
        led[0, c, F["total_reward"]] = rew
        led[0, c, F["disabled"]] = dis
    return led


def test_competition_key_depths():
    """Six cars, all with 2 laps except car 5 (3 laps, so first whatever else).  Cars 0-4 tie on laps:
      car 0 finish 50.0 best 20.0 reward 5 -> second key: 50.0
      car 1 finish 40.0                    -> earliest finish of the tied: position 1
      car 2 finish 50.0 best 19.0          -> ties car 0 on finish, better best: before car 0
      car 3 finish 50.0 best 20.0 reward 9 -> ties car 0 on finish and best, higher reward: before car 0
      car 4 finish 50.0 best 20.0 reward 5, disabled -> ties car 0 down to the reward, disabled: after car 0
    Order: 5, 1, 2, 3, 0, 4.  Points 45, 24, 21, 13, 8, 5 by position; fastest lap car 2 gets +15."""
    led = _ledger([(2, 50.0, 20.0, 5.0, 0), (2, 40.0, 30.0, 0.0, 0), (2, 50.0, 19.0, 0.0, 0), (2, 50.0, 20.0, 9.0, 0),
                   (2, 50.0, 20.0, 5.0, 1), (3, 99.0, 33.0, -7.0, 0)])
    order, position, points = race_ref.rank_ledger(led, [2], 1)
    assert order[0].tolist() == [5, 1, 2, 3, 0, 4]
    assert position[0].tolist() == [4, 1, 2, 3, 5, 0]
    assert points[0].tolist() == [8, 24, 21 + 15, 13, 5, 45]


def test_competition_zero_time_is_none_and_full_tie_keeps_index_order():
    """`x or 999999` maps 0.0 like None: car 0 (finish 0.0) and car 1 (finish None) share the key 999999 and every other
    key, so they keep index order; car 2 with a real finish time is ahead of both.  Car 3 ties car 2 on everything: index
    order.  Order 2, 3, 0, 1."""
    led = _ledger([(1, 0.0, 0.0, 1.0, 0), (1, None, None, 1.0, 0), (1, 30.0, 25.0, 1.0, 0), (1, 30.0, 25.0, 1.0, 0)])
    order, _, points = race_ref.rank_ledger(led, [-1], 1)
    assert order[0].tolist() == [2, 3, 0, 1]
    assert points[0].tolist() == [21, 13, 45, 24]


def test_competition_more_than_ten_cars():
    """12 cars with laps 12, 11, ..., 1: the order is the index order; positions 0-9 score 45 ... 0 and every position
    past 9 scores COMPETITION_POINTS[-10] = 0 too."""
    led = _ledger([(12 - c, None, None, 0.0, 0) for c in range(12)])
    order, _, points = race_ref.rank_ledger(led, None, 1)
    assert order[0].tolist() == list(range(12))
    assert points[0].tolist() == [45, 24, 21, 13, 8, 5, 3, 2, 1, 0, 0, 0]


def test_time_trial_fewer_than_three_laps():
    """Four cars, only cars 3 (21.5) and 1 (22.0) have a best lap, car 2's 0.0 counts as none: order 3, 1, then 0, 2 in
    index order; points 15 and 7, position 2 has no lap and scores 0."""
    led = _ledger([(0, None, None, 0.0, 0), (2, 44.0, 22.0, 0.0, 0), (1, 9.0, 0.0, 0.0, 0), (2, 43.0, 21.5, 0.0, 1)])
    order, position, points = race_ref.rank_ledger(led, None, 2)
    assert order[0].tolist() == [3, 1, 0, 2]
    assert position[0].tolist() == [2, 1, 3, 0]
    assert points[0].tolist() == [0, 7, 0, 15]


def _lap_step(r, laps, last, t, done=False, disabled=None):
    C = r.C
    r.step([0.25] * C, laps, last, disabled or [False] * C, t, done)


def test_strict_fastest_lap_rule_and_lap_events():
    """Three cars.  Step 1: cars 1 and 2 both complete a lap in 20.0 -> car 1 (lower index) holds the fastest lap.
    Step 2: car 0 laps in 20.0 too -> not strictly lower, car 1 keeps it.  Step 3: car 2 laps with last_lap_time 0.0 ->
    not truthy: no lap recorded, but previous_lap_count follows, so step 4 (same lap_count) is no event.  Step 5: car 0
    laps in 19.5 -> takes the fastest lap; its finish time is overwritten, its best improves.  The race ends with step 5
    (counted); step 6 changes nothing."""
    r = race_ref.EnvRace(3, 1)
    _lap_step(r, [0, 1, 1], [None, 20.0, 20.0], 1.0)
    assert (r.fastest_car, r.overall_best) == (1, 20.0)
    _lap_step(r, [1, 1, 1], [20.0, 20.0, 20.0], 2.0)
    assert r.fastest_car == 1
    _lap_step(r, [1, 1, 2], [20.0, 20.0, 0.0], 3.0)
    _lap_step(r, [1, 1, 2], [20.0, 20.0, 18.0], 4.0)
    assert r.laps_timed == [1, 1, 1] and r.prev == [1, 1, 2] and r.best[2] == 20.0
    _lap_step(r, [2, 1, 2], [19.5, 20.0, 18.0], 5.0, done=True)
    assert (r.fastest_car, r.overall_best) == (0, 19.5)
    assert r.finish == [5.0, 1.0, 1.0] and r.best == [19.5, 20.0, 20.0] and r.ended
    _lap_step(r, [3, 2, 3], [1.0, 1.0, 1.0], 6.0)
    rows = r.rows()
    assert rows[:, F["lap_count"]].tolist() == [2, 1, 2] and rows[:, F["steps"]].tolist() == [5, 5, 5]
    # five float32 adds of 0.25 are exact
    assert rows[:, F["total_reward"]].tolist() == [1.25] * 3 and isinstance(r.rewards[0], np.float32)


def test_reward_sum_is_float32():
    r = race_ref.EnvRace(1, 1)
    acc = np.float32(0.0)
    for k in range(50):
        x = np.float32(0.1) * np.float32(k)
        r.step([x], [0], [None], [False], k / 60.0, False)
        acc = np.float32(acc + x)
    assert isinstance(r.rewards[0], np.float32) and r.rewards[0] == acc
    assert float(r.rewards[0]) != sum(float(np.float32(0.1) * np.float32(k)) for k in range(50))


def test_time_trial_parking_and_persistence():
    """Two cars, one lap per attempt.  Attempt 1: car 0 laps in 30.0 at step 2 and is parked; its later lap events are
    ignored (step 3 shows lap_count 2 with 10.0: not recorded).  Car 1 is disabled at step 4 and parks; the attempt ends
    there.  Attempt 2 (records kept): car 0 laps in 31.0 -> best stays 30.0, laps_timed 2; car 1 laps in 29.0 and takes
    the fastest lap.  begin(False) clears all of it."""
    r = race_ref.EnvRace(2, 2, laps_per_attempt=1)
    _lap_step(r, [0, 0], [None, None], 1.0)
    assert r.parked() == [False, False]
    _lap_step(r, [1, 0], [30.0, None], 2.0)
    assert r.parked() == [True, False] and not r.ended
    _lap_step(r, [2, 0], [10.0, None], 3.0)
    assert r.best[0] == 30.0 and r.lap_count[0] == 1
    _lap_step(r, [2, 0], [10.0, None], 4.0, disabled=[False, True])
    assert r.ended and r.parked() == [True, True] and r.fastest_car == 0
    r.begin(True)
    assert r.parked() == [False, False] and r.best == [30.0, None] and not r.ended
    _lap_step(r, [1, 1], [31.0, 29.0], 5.0)
    assert r.best == [30.0, 29.0] and r.laps_timed == [2, 1] and r.attempt_laps == [1, 1] and r.ended
    assert (r.fastest_car, r.overall_best) == (1, 29.0)
    r.begin(False)
    assert r.best == [None, None] and r.fastest_car is None and r.laps_timed == [0, 0]


def test_championship_table_against_dicts():
    from nascargymnasium_amd.race import ChampionshipTable
    rng = np.random.default_rng(7)
    R, C, stages = 5, 12, 6
    table = ChampionshipTable(R, C)
    dicts = [race_ref.ChampionshipDict(C) for _ in range(R)]
    for _ in range(stages):
        # time trial: bests from a small set (ties) with Nones; some replicas with fewer than 3 laps
        best = rng.choice([NAN, NAN, 20.0, 21.0, 22.5], size=(R, C))
        best[0] = NAN
        best[1, 2:] = NAN
        led = np.zeros((R, C, len(race_ref.RACE_FIELDS)))
        led[:, :, F["best_lap"]] = best
        order, _, points = race_ref.rank_ledger(led, None, 2)
        table.add_time_trial(order, points)
        for r in range(R):
            got = dicts[r].calculate_time_trial_points([race_ref.none_if_nan(x) for x in best[r]])
            assert got == order[r].tolist()
        # competition
        led[:, :, F["lap_count"]] = rng.integers(0, 3, size=(R, C))
        led[:, :, F["finish_time"]] = rng.choice([NAN, 50.0, 60.0], size=(R, C))
        led[:, :, F["total_reward"]] = rng.choice([-1.0, 0.0, 2.5], size=(R, C))
        fastest = rng.integers(-1, C, size=R)
        order, _, points = race_ref.rank_ledger(led, fastest, 1)
        table.add_competition(order, points, fastest)
        for r in range(R):
            dicts[r].calculate_competition_points(order[r].tolist(), None if fastest[r] < 0 else int(fastest[r]))
    cars, pts = table.standings()
    for r in range(R):
        d = dicts[r]
        assert table.points[r].tolist() == [d.championship_points[c] for c in range(C)]
        assert list(zip(cars[r].tolist(), pts[r].tolist())) == d.get_championship_standings()
        for key, sub in (("time_trial_wins", None), ("competition_wins", None), ("fastest_laps", None),
                         ("time_trial_2nd", ("time_trial_podiums", "2nd")), ("time_trial_3rd", ("time_trial_podiums", "3rd")),
                         ("competition_2nd", ("competition_podiums", "2nd")), ("competition_3rd", ("competition_podiums", "3rd"))):
            want = [d.stats[key][c] if sub is None else d.stats[sub[0]][c][sub[1]] for c in range(C)]
            assert table.stats[key][r].tolist() == want, key
    assert (pts[:, :-1] >= pts[:, 1:]).all() and table.stats["time_trial_wins"][0].sum() == 0


def test_race_argument_errors():
    from nascargymnasium_amd import race

    class NoDevice:
        E, C = 4, 2

        def __getattr__(self, name):
            raise AssertionError(f"argument errors come before any device call ({name})")

    env = NoDevice()
    with pytest.raises(ValueError, match="policy must be one of"):
        race.time_trial(env, policy=1)
    with pytest.raises(ValueError, match="max_steps must be >= 1"):
        race.competition(env, max_steps=0)
    with pytest.raises(ValueError, match="chunk must be >= 1"):
        race.competition(env, chunk=0)
    with pytest.raises(ValueError, match="rollout action source"):
        race.competition(env, policy=6)
    with pytest.raises(ValueError, match="attempts and laps"):
        race.time_trial(env, attempts=0)
    with pytest.raises(ValueError, match="do not split over 3 tracks"):
        race.championship(env, ["daytona", "martinsville", "michigan"])
    with pytest.raises(ValueError, match="at least one track"):
        race.championship_layout([], 2)
    assert race.championship_layout(["a", "b"], 2) == ["a", "a", "b", "b"]
    with pytest.raises(ValueError, match=r"stage results must be \[2, 3\]"):
        race.ChampionshipTable(2, 3).add_time_trial(np.zeros((2, 2), int), np.zeros((2, 2), int))

"""The opponent-aware sensors' expected values, proved on the CPU (no GPU): tests/opponents.py's float32 restatement
of b2PolygonShape::RayCast is pinned to the oracle's ray cast, and the scenes tests/test_gpu_opponents.py holds the
device to are shown to exercise every class of ray (floors at most half the measured counts)."""
import math
import os

import numpy as np
import pytest

import opponents as op
from oracle_lib import OracleEnv


def _random_rays(rng, wf, n):
    """n rays p1 -> p2 (float32) around the walls `wf` (or_walls' float records): origins within N(0, 12 m) of a wall
    or uniform over the track, 250 m long or shorter, every 9th exactly axis-aligned"""
    j = rng.integers(0, len(wf), n)
    p1 = np.stack([wf[j, 0], wf[j, 1]], 1).astype(np.float64) + rng.normal(0, 12.0, (n, 2))
    lo, hi = wf[:, :2].min(0) - 50, wf[:, :2].max(0) + 50
    p1[::4] = rng.uniform(lo, hi, (len(p1[::4]), 2))
    ang = rng.uniform(-math.pi, math.pi, n)
    ln = np.where(rng.random(n) < 0.7, 250.0, rng.uniform(1.0, 250.0, n))
    p1 = p1.astype(np.float32)
    p2 = (p1.astype(np.float64) + np.stack([np.cos(ang), np.sin(ang)], 1) * ln[:, None]).astype(np.float32)
    k = np.arange(0, n, 9)              # exactly vertical / horizontal rays: one coordinate of p2 is p1's
    axis = rng.integers(0, 2, len(k))
    p2[k, axis] = p1[k, axis]
    return p1, p2


@pytest.mark.parametrize("track", ["martinsville.track", "daytona.track"])
def test_box_cast_equals_the_oracle_ray_cast(track):
    """fed the track's own wall records, the restatement's minimum over the walls equals or_raycast (ob_raycast:
    b2PolygonShape::RayCast per wall, closest hit) on 4 000 random rays, bit for bit -- hits, misses and rays that
    start inside a wall alike"""
    orc = OracleEnv(os.path.join(op.TRACKS, track), 1, 1)
    _, wf = orc.walls()
    rng = np.random.default_rng(5)
    p1, p2 = _random_rays(rng, wf, 4000)
    want = np.array([orc.L.or_raycast(orc.h, float(a[0]), float(a[1]), float(b[0]), float(b[1]))
                     for a, b in zip(p1, p2)], np.float32)
    orc.close()
    got = op.min_cast(p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1], (wf[:, 0], wf[:, 1], wf[:, 5], wf[:, 6], wf[:, 3], wf[:, 4]))
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, f"{len(bad)} rays differ, first {bad[0]}: {got[bad[0]]!r} vs oracle {want[bad[0]]!r}"
    assert (want >= 0).sum() > 1000 and (want < 0).sum() > 100     # hits and misses
    aligned = (p1[:, 0] == p2[:, 0]) | (p1[:, 1] == p2[:, 1])
    assert aligned.sum() > 100 and (want[aligned] >= 0).any()


def test_sensor_value_is_monotonic_and_equals_the_walls_only_rows():
    """min(wall value, car value) is the value of the min fraction only because the value arithmetic is monotonic;
    and with no other car (C = 1) the expected rows are the oracle's rows"""
    fr = np.sort(np.random.default_rng(0).uniform(0, 1.2, 20000).astype(np.float32))
    v = op.sensor_value(fr)
    assert (np.diff(v) >= 0).all() and v[0] >= 0 and v[-1] == 1.0
    assert op.sensor_value(np.float32(-1.0)) == 1.0
    poses = op.cluster_poses("martinsville.track", 16, 1)
    orc = OracleEnv(os.path.join(op.TRACKS, "martinsville.track"), 1, 1)
    walls = op.wall_rows(orc, poses).reshape(16, 1, 16)
    orc.close()
    rows, st = op.expected_rows(poses, walls)
    assert np.array_equal(rows.view(np.uint32), walls.view(np.uint32)) and not st["car"].any()


@pytest.mark.parametrize("track", ["martinsville.track", "daytona.track"])
def test_cluster_scene_exercises_every_class(track):
    """64 envs x 10 cars = 10 240 rays: a car is the nearest hit / a car is hit behind a nearer wall / no car is hit /
    the origin lies inside another car's box.  Measured (seed 11): see DESIGN 4.7; floors at most half."""
    poses, walls, rows, st = op.cluster_expected(track, 64, 10)
    near, behind, none = st["near"].sum(), (st["car"] & ~st["near"]).sum(), (~st["car"]).sum()
    inside = st["inside"].sum()
    print(f"{track}: near {near} behind {behind} none {none} inside {inside}")
    assert near + behind + none == 64 * 10 * 16
    assert near >= op.CLUSTER_FLOOR["near"] and behind >= op.CLUSTER_FLOOR["behind"]
    assert none >= op.CLUSTER_FLOOR["none"] and inside >= op.CLUSTER_FLOOR["inside"]
    assert (rows[st["near"]] < walls[st["near"]]).all() and np.array_equal(rows[~st["near"]], walls[~st["near"]])
    # a ray that starts inside a box gets no hit from that box: with two cars on one spot neither sees the other
    two = np.zeros((1, 2, 3), np.float32)
    two[0, :, :2] = poses[0, 0, :2]
    two[0, 1, 2] = 0.3
    r2, s2 = op.expected_rows(two, np.ones((1, 2, 16), np.float32))
    assert s2["inside"].all() and not s2["car"].any() and (r2 == 1.0).all()


def test_throttle_scene_cars_see_each_other():
    """daytona 4 x 10, contact off, each car its own throttle for 600 steps: none of the stacked cars sees another at
    the reset; sampled every 5th step, thousands of rays see a car nearer than the wall"""
    R = op.throttle_run()
    assert not R["near"][0].any(), "stacked at the start pose every origin is inside every other box"
    n = int(R["near"][::5].sum())
    print(f"throttle scene: {n} of {R['near'][::5].size} sampled rays see a car nearer than the wall")
    assert n >= op.THROTTLE_FLOOR_NEAR
    assert np.array_equal(R["rows"][~R["near"]], R["obs"][..., 22:][~R["near"]])

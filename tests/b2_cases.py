"""Hand-made cases for the Box2D step's primitives (b2TimeOfImpact, its exact cull, b2CollidePolygons).  TEST
INFRASTRUCTURE.

A TOI case is 12 float32: the car's sweep c0x c0y cx cy a0 a alpha0, then the static wall box wx wy wang whx why
(nascar_debug_toi / or_toi).  A manifold case is 8 float32: the car's pose x y angle and the same wall
(nascar_debug_collide / or_collide).  Every class aims at an edge of csrc/nascar_device.h's restatement; what each
reaches is counted by tests/test_b2_cases_cpu.py on the oracle and compared by tests/test_gpu_b2_prims.py on the device.

The classes (walls: half extents 0.5 .. 6 m x 0.05 .. 0.6 m; the car's end pose at a signed core gap off the wall's
long side, the start pose back along a direction; one case in seven with whole turns on both car angles):
  approach  gap -1 .. 0.3 m, 0.2 .. 2 m from the wall's outside, da +-0.1: TOUCHING with 0 < beta < 1, the root finder
  scrape    gap 6 .. 30 mm, parallel +-0.05 rad, 0 .. 1 m along the wall, da +-10 mrad: the second-order cull's regime
  far       gap 0.05 .. 3 m, 0 .. 2 m any direction, da +-0.3 (a tenth to +-pi/2, a slice 0.09 .. 0.11): the cull's bulk
  overlap0  gap -0.5 .. 0.02 m, 0 .. 0.3 m, da +-0.05: the OVERLAPPED / FAILED exits
  corner    gaps +-0.3 m past the wall's end, any angle, 0 .. 2 m, da +-0.2: vertex-vertex separation, 1-point manifolds
  alpha0    gap -0.3 .. 0.1 m, 0.05 .. 1 m, da +-0.05, alpha0 in (0.05, 0.95): sweeps after an event
  gate      |da| 0.05 .. 0.1 turning towards parallel, the second-order bound near its threshold (TOI and cull only)
  captured  the product's own computed jobs, tools/data/toi_jobs_r05.npy (TOI only)
  ties      manifolds only: car angle = wall angle + k pi / 2, gaps of 0 and the two radii +- 1 ulp

Also the float64 restatement of the cull's two bounds (toi_far / toi_far_rot2), shared with tests/test_toi_cull_cpu.py.
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPTURED = os.path.join(ROOT, "tools", "data", "toi_jobs_r05.npy")

CAR_HX, CAR_HY = 5.042 / 2.0, 1.996 / 2.0
R_CAR = 2.80389
CULL_T = 0.00925           # TOI_CULL_DIST: target + tolerance + the 3 mm rounding margin
CULL_MARGIN = 0.003
TOI_FAILED, TOI_OVERLAPPED, TOI_TOUCHING, TOI_SEPARATED = 1, 2, 3, 4
POSE_CLASSES = ("approach", "scrape", "far", "overlap0", "corner", "alpha0")
TOI_CLASSES = POSE_CLASSES + ("gate",)        # + "captured" (the TOI comparison only)
MANI_CLASSES = POSE_CLASSES + ("ties",)       # the end poses of the six, and the exact ties
SEEDS = {name: 1000 + i for i, name in enumerate(POSE_CLASSES + ("ties", "gate"))}
N_GPU = 100003             # cases per class in the GPU test: odd, so the last wave is partial


def rot(a):
    return np.stack([np.cos(a), np.sin(a)], -1)


def perp(u):
    return np.stack([-u[..., 1], u[..., 0]], -1)


def ext(u, ax, ay, hx, hy):
    return hx * np.abs((u * ax).sum(-1)) + hy * np.abs((u * ay).sum(-1))


def bounds(c0, a0, c1, a1, w, wa, whx, why):
    """(first-order bound, second-order bound) as toi_far / toi_far_rot2 compute them (float64 here)."""
    q1 = rot(a1)
    cx1, cy1 = q1, np.stack([-q1[:, 1], q1[:, 0]], -1)
    q0 = rot(a0)
    cx0, cy0 = q0, np.stack([-q0[:, 1], q0[:, 0]], -1)
    wx = rot(wa)
    wy = np.stack([-wx[:, 1], wx[:, 0]], -1)
    d1, d0, dc = c1 - w, c0 - w, c1 - c0
    b1 = np.full(len(a0), -np.inf)
    b2 = np.full(len(a0), -np.inf)
    for u in (wx, wy, cx1, cy1):
        s1, s0 = (u * d1).sum(-1), (u * d0).sum(-1)
        we = ext(u, wx, wy, whx, why)
        g1 = np.abs(s1) - ext(u, cx1, cy1, CAR_HX, CAR_HY) - we
        away = np.where(s1 >= 0, (u * dc).sum(-1), -(u * dc).sum(-1))
        b1 = np.maximum(b1, g1 - np.maximum(0.0, away))
        g0 = np.where(s1 >= 0, s0, -s0) - ext(u, cx0, cy0, CAR_HX, CAR_HY) - we
        b2 = np.maximum(b2, np.minimum(g0, g1))
    da = np.abs(a1 - a0)
    return b1 - da * R_CAR, b2 - da * da * (R_CAR / 8.0)


def case_bounds(cases):
    """(b1, b2, |da|) of TOI cases [n, 12]: the float64 bounds on the float32 inputs widened to double"""
    k = np.asarray(cases, np.float32).astype(np.float64)
    b1, b2 = bounds(k[:, 0:2], k[:, 4], k[:, 2:4], k[:, 5], k[:, 7:9], k[:, 9], k[:, 10], k[:, 11])
    return b1, b2, np.abs(k[:, 5] - k[:, 4])


def cull_decision(cases):
    """(far64, near): the cull's decision from the float64 bounds, and the cases within the device's float32 rounding
    budget (3 mm) of a threshold -- or of the |da| <= 0.1 gate -- where float32 may decide either way"""
    b1, b2, da = case_bounds(cases)
    gate = da <= 0.1
    far = (b1 > CULL_T) | (gate & (b2 > CULL_T))
    near = (np.abs(b1 - CULL_T) <= CULL_MARGIN) | (gate & (np.abs(b2 - CULL_T) <= CULL_MARGIN)) | \
           (np.abs(da - 0.1) <= 1e-6)
    return far, near


def _walls(rng, n):
    """wall centres (two thirds in +-500 m, one third in +-1500 m: the tracks' extent, the largest float32 ulps),
    angles (about 5 % beyond +-2 pi: their b2Sweep::Normalize changes the angle, so the device cannot reuse the
    body's rotation) and half extents"""
    span = np.where(rng.random(n) < 1.0 / 3.0, 1500.0, 500.0)
    w = rng.uniform(-1.0, 1.0, (n, 2)) * span[:, None]
    wa = rng.uniform(-np.pi, np.pi, n)
    big = rng.random(n) < 0.05
    wa = np.where(big, np.where(rng.random(n) < 0.5, 1.0, -1.0) * rng.uniform(2 * np.pi, 4 * np.pi, n), wa)
    return w, wa, rng.uniform(0.5, 6.0, n), rng.uniform(0.05, 0.6, n)


def _parallel(rng, n, wa, spread):
    """car angles within +-spread of the wall's direction, either way round"""
    return wa + rng.uniform(-spread, spread, n) + np.where(rng.random(n) < 0.5, 0.0, np.pi)


def _place(w, wa, whx, why, a1, side, along, gap):
    """car centre at signed core gap `gap` off the wall's long side `side`, `along` metres along it"""
    wx = rot(wa)
    wy = perp(wx)
    q1 = rot(a1)
    e_car = ext(wy, q1, perp(q1), CAR_HX, CAR_HY)
    return w + along[:, None] * wx + (side * (why + e_car + gap))[:, None] * wy


def _pack(c0, a0, c1, a1, alpha0, w, wa, whx, why):
    return np.concatenate([c0, c1, a0[:, None], a1[:, None], alpha0[:, None], w, wa[:, None], whx[:, None],
                           why[:, None]], 1).astype(np.float32)


def _from_outside(rng, n, wa, side, lo, hi, gap_lo, gap_hi):
    """a translation of lo .. hi metres that comes from the wall's outside (within 1.2 rad of its inward normal), and
    an end-pose gap in gap_lo .. gap_hi that leaves the start pose's centre at least 2 cm further out than a touching
    one: (translation vector, gap)"""
    L = rng.uniform(lo, hi, n)
    th = rng.uniform(-1.2, 1.2, n)
    out = perp(rot(wa)) * side[:, None]                       # outward normal of the car's side
    dirn = np.cos(th)[:, None] * out + np.sin(th)[:, None] * perp(out)
    gap = rng.uniform(np.maximum(gap_lo, 0.02 - L * np.cos(th)), gap_hi)
    return -L[:, None] * dirn, gap                            # c1 - c0: towards the wall


def toi_cases(name, n, seed=None):
    """[n, 12] float32 TOI cases of class `name` (seeded: the same cases in every process)"""
    if name == "captured":
        j = np.load(CAPTURED).astype(np.float32)               # sw0, sw1, (px py qs qc), (hx hy ang key)
        return np.ascontiguousarray(np.concatenate([j[:, 0:7], j[:, 8:10], j[:, 14:15], j[:, 12:14]], 1))
    rng = np.random.default_rng(SEEDS[name] if seed is None else seed)
    w, wa, whx, why = _walls(rng, n)
    side = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    anyang = rng.uniform(-np.pi, np.pi, n)
    alpha0 = np.zeros(n)
    along = rng.uniform(-1.0, 1.0, n) * (whx + CAR_HX)
    anydir = rot(rng.uniform(-np.pi, np.pi, n))
    if name == "approach":
        a1 = np.where(rng.random(n) < 0.5, _parallel(rng, n, wa, 0.2), anyang)
        dc, gap = _from_outside(rng, n, wa, side, 0.2, 2.0, -1.0, 0.3)
        da = rng.uniform(-0.1, 0.1, n)
    elif name == "scrape":
        a1 = _parallel(rng, n, wa, 0.05)
        # a quarter of the gaps from the upper half of the range: decided by the second-order bound alone, and clear
        # of the threshold by more than the float32 budget (the margin test cannot use the cases within it)
        gap = np.where(rng.random(n) < 0.25, rng.uniform(0.018, 0.030, n), rng.uniform(0.006, 0.030, n))
        # along the wall as a car drives along it: forwards or backwards on its own heading
        dc = (rng.uniform(0.0, 1.0, n) * np.where(rng.random(n) < 0.5, 1.0, -1.0))[:, None] * rot(a1)
        da = rng.uniform(-0.010, 0.010, n)
    elif name == "far":
        a1 = np.where(rng.random(n) < 0.5, _parallel(rng, n, wa, 0.2), anyang)
        gap = rng.uniform(0.05, 3.0, n)
        dc = rng.uniform(0.0, 2.0, n)[:, None] * anydir
        u = rng.random(n)
        sign = np.where(rng.random(n) < 0.5, 1.0, -1.0)
        da = np.where(u < 0.1, rng.uniform(-np.pi / 2, np.pi / 2, n),
                      np.where(u < 0.25, sign * rng.uniform(0.09, 0.11, n), rng.uniform(-0.3, 0.3, n)))
    elif name == "overlap0":
        a1 = np.where(rng.random(n) < 0.5, _parallel(rng, n, wa, 0.2), anyang)
        gap = rng.uniform(-0.5, 0.02, n)
        dc = rng.uniform(0.0, 0.3, n)[:, None] * anydir
        da = rng.uniform(-0.05, 0.05, n)
    elif name == "corner":
        a1 = anyang
        gap = rng.uniform(-0.3, 0.3, n)
        q1 = rot(a1)
        e_along = ext(rot(wa), q1, perp(q1), CAR_HX, CAR_HY)
        along = np.where(rng.random(n) < 0.5, 1.0, -1.0) * (whx + e_along + rng.uniform(-0.3, 0.3, n))
        dc = rng.uniform(0.0, 2.0, n)[:, None] * anydir
        da = rng.uniform(-0.2, 0.2, n)
    elif name == "alpha0":
        a1 = np.where(rng.random(n) < 0.5, _parallel(rng, n, wa, 0.2), anyang)
        dc, gap = _from_outside(rng, n, wa, side, 0.05, 1.0, -0.3, 0.1)
        da = rng.uniform(-0.05, 0.05, n)
        alpha0 = rng.uniform(0.05, 0.95, n)
    elif name == "gate":
        # The second-order bound where its start-pose rotation decides: a car alongside the wall turning 0.05 .. 0.1
        # rad (up to the |da| <= 0.1 gate) towards parallel, so the start pose's gap across the wall is the smaller one
        # by the change of the car's extent; 12 % of the gaps put that bound within 1 mm of the threshold (where a
        # rotation of too low an order, off by |da|^3 / 6 x 3.5 m, decides otherwise), the rest within 60 mm.
        phi = rng.uniform(-0.05, 0.05, n)
        a1 = wa + phi + np.where(rng.random(n) < 0.5, 0.0, np.pi)
        da = -np.where(phi >= 0, 1.0, -1.0) * rng.uniform(0.05, 0.1, n)
        wy = perp(rot(wa))
        q1, q0 = rot(a1), rot(a1 - da)
        shrink = ext(wy, q0, perp(q0), CAR_HX, CAR_HY) - ext(wy, q1, perp(q1), CAR_HX, CAR_HY)
        off = np.where(rng.random(n) < 0.12, rng.uniform(-0.001, 0.001, n), rng.uniform(-0.06, 0.06, n))
        gap = CULL_T + R_CAR * da * da / 8.0 + shrink + off
        along = rng.uniform(-0.8, 0.8, n) * whx
        dc = rng.uniform(-0.3, 0.3, n)[:, None] * rot(wa)
    else:
        raise KeyError(name)
    c1 = _place(w, wa, whx, why, a1, side, along, gap)
    # one case in seven: whole turns on both car angles (b2Sweep::Normalize takes them off again)
    turns = np.where(rng.random(n) < 1.0 / 7.0, rng.integers(1, 10, n) * np.where(rng.random(n) < 0.5, 1.0, -1.0), 0.0)
    a1 = a1 + turns * (2 * np.pi)
    return _pack(c1 - dc, a1 - da, c1, a1, alpha0, w, wa, whx, why)


def _ties(rng, n):
    """exact ties of b2CollidePolygons: car angle = wall angle + k pi / 2 (float32 sums), core gaps of 0, 0.02 m (the
    two polygon radii: the `separation <= totalRadius` point test) and one ulp of the car's coordinates either side;
    parallel boxes have equal face separations, the `separationB > separationA + 0.1 slop` choice (e_faceA unless the
    difference passes the bias; a third of the cars are tilted by up to 0.3 mrad so that it does).  Half of the walls
    are axis-aligned at coordinates that are multiples of 1/8, so the sums are exact."""
    w, wa, whx, why = _walls(rng, n)
    exact = rng.random(n) < 0.5
    w = np.where(exact[:, None], np.round(w * 8.0) / 8.0, w)
    wa = np.where(exact, 0.0, wa).astype(np.float32)
    whx, why = whx.astype(np.float32), why.astype(np.float32)
    k = rng.integers(0, 4, n)
    a1 = (wa + (k * np.float32(np.pi / 2)).astype(np.float32)).astype(np.float32)
    # a third of them a hair off parallel: the wall's far end dips by up to 6 m x 3e-4 = 1.8 mm under the car's face,
    # so separationB - separationA straddles the 0.5 mm bias and both manifold types come out
    a1 = (a1 + np.where(rng.random(n) < 1.0 / 3.0, rng.uniform(-3e-4, 3e-4, n), 0.0).astype(np.float32)).astype(np.float32)
    side = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    gap = np.where(rng.random(n) < 0.5, 0.0, 0.02)
    # half of the cars lie along the wall, half past its end (clip points cut off, 1-point manifolds)
    along = np.where(rng.random(n) < 0.5, rng.uniform(-1.0, 1.0, n) * whx,
                     np.where(rng.random(n) < 0.5, 1.0, -1.0) * (whx + np.where(k % 2 == 0, CAR_HX, CAR_HY) +
                                                                   rng.uniform(-0.05, 0.02, n)))
    # the car's extent across the wall in float32, as the device's boxes have it
    e_car = np.where(k % 2 == 0, np.float32(CAR_HY), np.float32(CAR_HX)).astype(np.float32)
    off = ((why + e_car).astype(np.float32) + gap.astype(np.float32)).astype(np.float32)
    wa64 = wa.astype(np.float64)
    wx, wy = rot(wa64), perp(rot(wa64))
    c = (w + along[:, None] * wx + (side * off.astype(np.float64))[:, None] * wy).astype(np.float32)
    nudge = rng.integers(-1, 2, n)
    # one ulp either way on the coordinate across the wall (for the axis-aligned half: exactly across)
    axis = np.where(np.abs(wy[:, 1]) >= np.abs(wy[:, 0]), 1, 0)
    for i in (0, 1):
        sel = axis == i
        col = c[:, i].copy()
        col[sel & (nudge > 0)] = np.nextafter(col[sel & (nudge > 0)], np.float32(np.inf))
        col[sel & (nudge < 0)] = np.nextafter(col[sel & (nudge < 0)], np.float32(-np.inf))
        c[:, i] = col
    return np.concatenate([c, a1[:, None], w.astype(np.float32), wa[:, None], whx[:, None], why[:, None]], 1) \
        .astype(np.float32)


def mani_cases(name, n, seed=None):
    """[n, 8] float32 manifold cases: the end poses of the TOI class `name`, or the exact ties"""
    if name == "ties":
        return np.ascontiguousarray(_ties(np.random.default_rng(SEEDS[name] if seed is None else seed), n))
    k = toi_cases(name, n, seed)
    return np.ascontiguousarray(np.concatenate([k[:, 2:4], k[:, 5:6], k[:, 7:12]], 1))


def shuffled(parts, seed=99):
    """the classes' cases in one buffer, shuffled, so that the lanes of a wave take different paths; returns
    (cases, the permutation: row i is row perm[i] of the concatenation)"""
    allc = np.concatenate(parts, 0)
    perm = np.random.default_rng(seed).permutation(len(allc))
    return np.ascontiguousarray(allc[perm]), perm


def mani_decode_oracle(o):
    """or_collide rows -> (stage, point count, type) as the device derives them from the same sentinels: stage 2 when
    localNormal.x was written (no longer the NaN 0x7fc0dead), else 1 when the type was, else 0"""
    o = np.ascontiguousarray(o, np.float32)
    written = o[:, 2].copy().view(np.uint32) != 0x7FC0DEAD
    typ = o[:, 0].astype(np.int64)
    stage = np.where(written, 2, np.where(typ >= 0, 1, 0))
    return stage, o[:, 1].astype(np.int64), typ


def mani_decode_device(r):
    """raw ManiRes rows [n, 12] -> (stage, point count, type) as contact_apply unpacks word 0"""
    h = np.ascontiguousarray(r, np.float32)[:, 0].copy().view(np.int32).astype(np.int64)
    return h & 3, (h >> 2) & 3, (h >> 4) & 3


_cache = {}


def gpu_toi(name):
    """class `name`'s N_GPU TOI cases with the oracle's (beta, state) and the float64 cull decision (far64, near):
    computed once per process, read-only"""
    if ("toi", name) not in _cache:
        import oracle_lib
        k = toi_cases(name, N_GPU)
        beta, state = oracle_lib.toi(k)
        far64, near = cull_decision(k)
        for a in (k, beta, state, far64, near):
            a.setflags(write=False)
        _cache["toi", name] = (k, beta, state, far64, near)
    return _cache["toi", name]


def gpu_mani(name):
    """class `name`'s N_GPU manifold cases with or_collide's rows: computed once per process, read-only"""
    if ("mani", name) not in _cache:
        import oracle_lib
        k = mani_cases(name, N_GPU)
        o = oracle_lib.collide(k)
        for a in (k, o):
            a.setflags(write=False)
        _cache["mani", name] = (k, o)
    return _cache["mani", name]

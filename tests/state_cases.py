"""Whole-state cases for single-step parity of the device against the oracle.  TEST INFRASTRUCTURE, CPU only.

A case set is one state arena of an E x C engine (the blob nascar_get_state returns, oracle_lib.gpu_arena's layout)
plus one action per car: tests/test_gpu_state_parity.py loads it into the device (set_state) and into the oracle
(oracle_lib.inject_gpu_state), steps both once and compares every field; tests/test_state_cases_cpu.py pins on the
oracle alone that the sets reach what they are built for.

Base states are harvested from oracle runs (noisy rule driver on daytona -- banked -- and martinsville -- short,
tight --, throttle-heavy random actions on the crowded POCKET(40) scene of tests/crowded.py, whose cars carry live
contact records and listener entries).  A class overlays crafted fields on them: values exactly at a gate's threshold
and at nextafter on either side, in the arithmetic the gate uses (a speed gate compares the float32 b2Vec2 length
widened to double, so the velocity is axis-aligned with a float32 component next to the threshold: sqrtf(s * s) == s).
Where the gate's operand is computed during the step (the progress difference, the lap distance), the builder first
steps the oracle once (`probe`) and places the injected field relative to what the step will add.

Every class records, per car or env, the side of each gate it was built for (`want`); predicate() recomputes the sides
from the blob's fields alone, in the gate's arithmetic, and the two must agree for every case.

Gates with no reachable other side (kept out on purpose, so that nobody looks for them):
  * weight_transfer's deficit redistribution (raw < 50.0): the front axle keeps at least 5 % of its load (the
    longitudinal transfer is capped at 95 %), i.e. >= 367.9 N, and the lateral transfer is capped at half the axle load
    minus 200 N (or zero), so no wheel's raw load is under min(ft / 4 + 100, ft / 2) >= 183.9 N for any finite input;
  * lat_g > 2.0 needs a mean lateral acceleration over 19.62 m/s^2 where each sample is clipped to 12: reachable only
    through an injected ring (the `tyres` class does that), as are the saturated transfers of `weight_transfer` (+-40).
"""
import atexit
import math
import os
import shutil
import tempfile

import numpy as np

import crowded
import track_gen
from drivers import NoisyRuleDriver
from gpu_state import F32, F64, I32
from oracle_lib import GPU_MAXC, OracleEnv, gpu_arena, inject_gpu_state, oracle_arena, pack_arena

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACKS = os.path.join(ROOT, "nascargymnasium_amd", "tracks")
N_CARS = 2400                       # cars per case set: divisible by every layout's C
LAYOUTS = {1: (1, 128), 3: (1, 42), 10: (1, 12)}    # C -> envs per workgroup (1, the fullest)
DT = 1.0 / 60.0
STEER_K = 45.0 * (np.pi / 180.0)    # c.steer = str_in * (45.0 * RAD_PER_DEG)
SPEED_GATES = (0.05, 0.1, 1.0, 2.0, 3.0, 5.0, 12.0, 25.0, 50.0)
f32i, f64i, i32i = ({f: k for k, f in enumerate(L)} for L in (F32, F64, I32))

_tmp = None
_pools = {}
_built = {}


def track_path(name):
    """daytona / martinsville: the bundled files; pocket: crowded.POCKET(40), written once per process; the names of
    track_gen.FAMILY: the generated tracks, likewise"""
    global _tmp
    if name == "pocket" or name in track_gen.FAMILY:
        if _tmp is None:
            _tmp = tempfile.mkdtemp(prefix="state_cases_")
            atexit.register(shutil.rmtree, _tmp, True)
            crowded.write_pocket(_tmp, 40)
        if name == "pocket":
            return os.path.join(_tmp, "pocket40.track")
        path = os.path.join(_tmp, name + ".track")
        return path if os.path.exists(path) else track_gen.write(_tmp, name)
    return os.path.join(TRACKS, name + ".track")


# ---------------------------------------------------------------- base states
def _cat(parts):
    """per-car sections of several oracle_arena() snapshots joined along the car axis, with each car's env time"""
    out = {}
    for k in ("f32", "f64", "i32", "acc"):
        out[k] = np.concatenate([p[k] for p in parts], 1)
    for k in ("ct", "key", "n"):
        out[k] = np.concatenate([p[k] for p in parts], 0)
    out["time"] = np.concatenate([np.repeat(p["time"], p["f32"].shape[1] // len(p["time"])) for p in parts])
    return out


STARTS = (0, 3, 4, 5)     # the segments whose start points the harvest runs begin at (0: the track's own start)


GEN_STARTS = {"seg64": (0, 10, 20, 40), "seg17": (0, 3, 8, 13), "ring4": (0, 2), "degenerate": (0, 10), "nostart": (0, 2)}


def start_poses(name):
    """[(x, y, angle)] of track `name`: the start of segment k for k in STARTS (GEN_STARTS[name] on a generated
    track), heading along the track there"""
    starts = GEN_STARTS.get(name, STARTS)
    orc = OracleEnv(track_path(name), 1, 1)
    seg = orc.segments()
    orc.close()
    head = 0.0
    out = []
    for k, r in enumerate(seg):
        if r[0] != 4.0:                                   # not a curve: the heading of its own chord
            head = float(np.arctan2(r[5] - r[3], r[4] - r[2]))
        if k in starts:
            out.append((float(r[2]), float(r[3]), head))
        if r[0] == 4.0:                                   # a curve turns by its angle (degrees), to the left if r[9]
            head += float(np.radians(r[7])) * (1.0 if r[9] else -1.0)
    return out


def pool(name):
    """The harvested base states of track `name`, one record per car (sections as gpu_arena's, car axis P), computed
    once per process.  daytona / martinsville: from each of start_poses(), 3 x 10 cars under the noisy rule driver
    (seed 5; done envs reset), harvested right after the reset and at steps 3, 40, 100, 160 -- cars on both
    straights and in both banked curves; pocket: the crowded 12 x 10 scene's actions, harvested at steps 295, 310 and
    330 (57 of its 120 cars hold more than 4 contacts after 300).  The first call runs all the harvests in parallel
    host threads (the C step releases the GIL inside ctypes)."""
    if name not in _pools and name in GEN_STARTS:     # a generated track: its own harvest, from each of start_poses()
        from concurrent.futures import ThreadPoolExecutor
        poses = start_poses(name)
        with ThreadPoolExecutor(len(poses)) as ex:
            parts = list(ex.map(lambda p: _harvest(name, p), poses))
        P = _cat([q for pp in parts for q in pp])
        for a in P.values():
            a.setflags(write=False)
        _pools[name] = P
    if name not in _pools:
        from concurrent.futures import ThreadPoolExecutor
        track_path("pocket")
        jobs = [("pocket", None)] + [(t, p) for t in ("daytona", "martinsville") for p in start_poses(t)]
        with ThreadPoolExecutor(len(jobs)) as ex:
            parts = list(ex.map(lambda j: _harvest(*j), jobs))
        for t in ("daytona", "martinsville", "pocket"):
            P = _cat([q for (tt, _), pp in zip(jobs, parts) if tt == t for q in pp])
            for a in P.values():
                a.setflags(write=False)
            _pools[t] = P
    return _pools[name]


def _harvest(name, pose):
    path = track_path(name)
    parts = []
    if name == "pocket":
        E, C = 12, 10
        orc = OracleEnv(path, E, C)
        orc.reset()
        rng = np.random.default_rng(crowded.SEED)
        for k in range(331):
            orc.step(crowded.actions(rng, E, C))
            if k + 1 in (295, 310, 330):
                parts.append(oracle_arena(orc))
    else:
        E, C = 3, 10
        orc = OracleEnv(path, E, C, start_position=pose[:2], start_angle=pose[2])
        obs = orc.reset()[0]
        parts.append(oracle_arena(orc))
        drv = NoisyRuleDriver(E * C, seed=5)
        for k in range(160):
            obs, _, _, ef = orc.step(drv.actions(obs, k))
            done = (ef[:, 0] != 0) | (ef[:, 1] != 0)
            for e in np.flatnonzero(done):
                orc.reset(int(e))
            if done.any():
                obs = orc.outputs()[0]
            if k + 1 in (3, 40, 100, 160):
                parts.append(oracle_arena(orc))
    orc.close()
    return parts


def speed32(f32):
    """the float32 b2Vec2::Length of the body velocity, widened to double as every speed gate reads it"""
    vx, vy = f32[f32i["vx"]], f32[f32i["vy"]]
    return np.sqrt(vx * vx + vy * vy, dtype=np.float32).astype(np.float64)


class Cases:
    """one case set: `A` the arena sections of an E x C engine (views of `blob`), `actions` [E, C, 2] float32,
    `want` the gate sides the builder aimed at (per car [N] or per env [E])"""

    def __init__(self, name, track, C, reset_on_lap=False):
        self.name, self.track, self.path, self.C, self.reset_on_lap = name, track, track_path(track), C, reset_on_lap
        self.N, self.E = N_CARS, N_CARS // C
        self.blob = np.zeros(len(pack_arena({}, self.E, C)), np.uint8)
        self.A = gpu_arena(self.blob, self.E, C)
        self.actions = np.zeros((self.E, C, 2), np.float32)
        self.want = {}
        self.mask = None     # reset_dirty: the envs to reset instead of stepping
        self.meta = {}       # what the builder probed on the oracle (predicate() reads it)

    def fill(self, sel=None, stride=7):
        """base states: car n takes pool record sel[(n * stride) % len(sel)] (sel: indices allowed, default all);
        env words: created, nothing pending; each env's time is the largest of its cars' harvest times"""
        P = pool(self.track)
        sel = np.arange(P["f32"].shape[1]) if sel is None else np.asarray(sel)
        assert len(sel) > 0, (self.name, "no base state qualifies")
        src = sel[(np.arange(self.N) * stride) % len(sel)]
        for k in ("f32", "f64", "i32", "acc"):
            self.A[k][...] = P[k][:, src]
        for k in ("ct", "key", "n"):
            self.A[k][...] = P[k][src]
        self.A["time"][...] = P["time"][src].reshape(self.E, self.C).max(1)
        self.A["ei32"][...] = 0
        self.A["ei32"][0] = 1
        self.src = src
        return self

    def f32(self, f):
        return self.A["f32"][f32i[f]]

    def f64(self, f):
        return self.A["f64"][f64i[f]]

    def i32(self, f):
        return self.A["i32"][i32i[f]]

    def set_velocity(self, vx, vy, idx=slice(None)):
        """the body's linear velocity (b2Body::SetLinearVelocity: a moving body is awake)"""
        self.f32("vx")[idx], self.f32("vy")[idx] = vx, vy
        self.i32("awake")[idx] = 1

    def act(self):
        return self.actions.reshape(self.N, 2)

    def oracle(self):
        """a fresh OracleEnv holding this state"""
        orc = OracleEnv(self.path, self.E, self.C, reset_on_lap=self.reset_on_lap)
        inject_gpu_state(orc, self.blob, self.E, self.C, list(range(self.E)))
        return orc

    def probe(self):
        """the oracle's state one step on (sections as gpu_arena's), without touching this set"""
        orc = self.oracle()
        orc.step(self.actions)
        A = oracle_arena(orc)
        orc.close()
        return A

    def check_bounds(self):
        """everything the device indexes with stays inside its arrays (csrc/nascar_layout.h MAXC, the 10-slot ring,
        the track's walls)"""
        orc = OracleEnv(self.path, 1, 1)
        nw = orc.L.or_num_walls(orc.h)
        keys = int(orc.walls()[1][:, 11].max())
        orc.close()
        nct, nact = self.i32("nct"), self.i32("nact")
        assert (0 <= nct).all() and (nct <= GPU_MAXC).all() and (0 <= nact).all() and (nact <= GPU_MAXC).all()
        assert (0 <= self.i32("acc_len")).all() and (self.i32("acc_len") <= 10).all()
        assert (0 <= self.i32("acc_head")).all() and (self.i32("acc_head") < 10).all()
        ct = self.A["ct"].reshape(self.N, GPU_MAXC, 20)
        slot = np.arange(GPU_MAXC)[None, :] < nct[:, None]
        assert ((ct[:, :, 0] >= 0) & (ct[:, :, 0] < nw))[slot].all() and ((ct[:, :, 3] >= 0) & (ct[:, :, 3] <= 2))[slot].all()
        act = np.arange(GPU_MAXC)[None, :] < nact[:, None]
        assert ((self.A["key"] >= 0) & (self.A["key"] <= keys))[act].all()
        assert np.isfinite(self.A["f32"]).all() and np.isfinite(self.A["f64"]).all() and np.isfinite(self.A["acc"]).all()
        assert np.isfinite(self.actions).all() and np.isfinite(self.A["time"]).all()
        assert (np.abs(self.A["f32"][:6]) < 1e5).all()

    def done(self):
        self.check_bounds()
        self.blob.setflags(write=False)
        self.actions.setflags(write=False)
        return self


def around(t, dtype=np.float64):
    """[nextafter(t, -inf), t, nextafter(t, +inf)] in dtype (t rounded to dtype first)"""
    t = dtype(t)
    return np.array([np.nextafter(t, dtype(-np.inf)), t, np.nextafter(t, dtype(np.inf))], dtype)


def _moving(P, lo=5.0):
    """pool records of enabled, awake cars faster than `lo` m/s"""
    return np.flatnonzero((P["i32"][i32i["disabled"]] == 0) & (P["i32"][i32i["awake"]] == 1) & (speed32(P["f32"]) > lo))


def _free(P):
    """enabled cars with no touching contact and no listener entry"""
    return np.flatnonzero((P["i32"][i32i["disabled"]] == 0) & (P["i32"][i32i["nact"]] == 0) &
                          ((P["ct"].reshape(len(P["ct"]), GPU_MAXC, 20)[:, :, 1] & 1).sum(1) == 0))


def _pre_sum(target, add):
    """x [3, n] with fl(x + add) just below / at / just above `target` (float64), for gates that compare a field after
    the step added `add` to it"""
    add = np.asarray(add, np.float64).ravel()
    cand = [target - add]
    for _ in range(4):
        cand.insert(0, np.nextafter(cand[0], -np.inf))
        cand.append(np.nextafter(cand[-1], np.inf))
    cand = np.stack(cand)                     # ascending, 9 candidates
    s = cand + add
    lo = (s < target).sum(0) - 1              # the last candidate whose sum is below
    hi = len(cand) - (s > target).sum(0)      # the first candidate whose sum is above
    at = np.argmax(s == target, 0)
    assert (lo >= 0).all() and (hi < len(cand)).all() and (s == target).any(0).all()
    cols = np.arange(add.size)
    return np.stack([cand[j, cols] for j in (lo, at, hi)])


# ---------------------------------------------------------------- classes
def _speed_gates(c):
    """all nine speed gates x (below, at, above) x 4 axis directions x (throttle, brake, coast), steering varied"""
    c.fill(_moving(pool(c.track)))
    n = np.arange(c.N)
    g, side, d, a = n % 9, (n // 9) % 3, (n // 27) % 4, (n // 108) % 3
    s = np.stack([around(t, np.float32) for t in SPEED_GATES])[g, side]
    # the float32 neighbours of a threshold that float32 does not hold (0.05, 0.1) lie on either side of it
    c.set_velocity(np.where(d == 0, s, np.where(d == 2, -s, 0)).astype(np.float32),
                   np.where(d == 1, s, np.where(d == 3, -s, 0)).astype(np.float32))
    c.act()[:, 0] = np.array([1.0, -1.0, 0.0], np.float32)[a]
    c.act()[:, 1] = np.array([0.3, -0.5, 0.0, 1.0], np.float32)[(n // 324) % 4]
    thr = np.array(SPEED_GATES)[g]
    sd = s.astype(np.float64)
    c.want = dict(gate=g, above=sd > thr, below=sd < thr)
    c.meta = dict(side=side)


def _input_gates(c):
    """throttle, brake and steering next to 0.01 (the steering gate reads str_in * 45 deg), out-of-range actions that
    the clip catches, and disabled cars, whose actions the step zeroes"""
    c.fill(_moving(pool(c.track)))
    n = np.arange(c.N)
    tb = np.concatenate([around(0.01, np.float32), -around(0.01, np.float32), np.float32([0.0, 1.0, -1.0, 1.5, -1.5, 0.5])])
    s0 = np.float32(0.01 / STEER_K)
    st = [s0]
    for _ in range(2):
        st.insert(0, np.nextafter(st[0], np.float32(-1)))
        st.append(np.nextafter(st[-1], np.float32(1)))
    st = np.float32(st)
    st = np.concatenate([st, -st, np.float32([0.0, 1.0, -1.0, 1.25, -1.25])])
    c.act()[:, 0] = tb[n % len(tb)]
    c.act()[:, 1] = st[(n // len(tb)) % len(st)]
    dis = (n // (len(tb) * len(st))) % 3 == 2
    c.i32("disabled")[dis] = 1
    a = c.act().astype(np.float64)
    a[dis] = 0.0
    c.want = dict(thr_on=np.clip(a[:, 0], 0, 1) > 0.01, brk_on=np.clip(-a[:, 0], 0, 1) > 0.01,
                  steer_on=np.abs(np.clip(a[:, 1], -1, 1) * STEER_K) > 0.01, disabled=dis)


def rpm_next(rpm, thr):
    """Car._update_engine_rpm in numpy: (new rpm, the min() took 1.0, low clamp, high clamp)"""
    with np.errstate(divide="ignore"):
        diff = (1000.0 + 800.0 * thr) - rpm
        k = DT * 3000.0 / np.abs(diff + 0.1)
        unit = ~(k < 1.0)
        r = rpm + diff * np.where(unit, 1.0, k)
    return np.maximum(600.0, np.minimum(9500.0, r)), unit, r < 600.0, r > 9500.0


def rpm_edge(target, level, lo, hi):
    """adjacent doubles (a, b), lo <= a < b <= hi, between which the unclamped new rpm crosses `level` (bisection; the
    update is increasing in rpm there)"""
    raw = lambda r: r + (target - r) * np.minimum(1.0, DT * 3000.0 / np.abs((target - r) + 0.1))
    a, b = np.full_like(target, lo), np.full_like(target, hi)
    assert (raw(a) < level).all() and (raw(b) >= level).all()
    while True:
        m = a + (b - a) / 2
        if ((m == a) | (m == b)).all():
            return a, b
        up = raw(m) >= level
        a, b = np.where(up, a, m), np.where(up, m, b)


def _rpm(c):
    """both clamps (the adjacent doubles near 550 / 9550 rpm between which the new value crosses 600 / 9500, and values
    200 rpm to either side), the denominator diff + 0.1 within a few
    1e-14 of zero on either side (exactly zero it cannot be: next to 1000 rpm the differences are multiples of 2^-43,
    which 0.1 is not), and |diff + 0.1| next to 50, where min(1.0, ...) changes hands"""
    c.fill(_moving(pool(c.track)))
    n = np.arange(c.N)
    thr = np.array([0.0, 0.5, 1.0])[n % 3]
    target = 1000.0 + 800.0 * thr
    vals = []
    for level, lo, hi in ((600.0, 500.0, 600.0), (9500.0, 9500.0, 9600.0)):
        a, b = rpm_edge(target, level, lo, hi)
        vals += [a, b, a - 200.0, b + 200.0, a - 4.0 * np.spacing(a), b + 4.0 * np.spacing(b)]
    z = target + 0.1            # diff = target - rpm = -0.1 (+- rounding): diff + 0.1 = 0 or a few 1e-14
    zs = [z]
    for _ in range(3):
        zs.insert(0, np.nextafter(zs[0], -np.inf))
        zs.append(np.nextafter(zs[-1], np.inf))
    vals += zs
    for d in (49.9, -50.1):     # diff + 0.1 = +-50: dt * 3000 / 50 = 1.0
        r0 = target - d
        vals += [np.nextafter(r0, -np.inf), r0, np.nextafter(r0, np.inf)]
    vals = np.stack(vals)
    c.f64("rpm")[:] = vals[(n // 3) % len(vals), n]
    c.act()[:, 0] = thr.astype(np.float32)
    c.act()[:, 1] = np.float32(0.1)
    _, unit, lo, hi = rpm_next(c.f64("rpm"), thr)
    den = (target - c.f64("rpm")) + 0.1
    c.want = dict(unit=unit, lo=lo, hi=hi, tiny_den=np.sign(den) * (np.abs(den) < 1e-12))


def _tyres(c):
    """tyre temperatures at 85 / 105 (the grip band) and 25 / 120 (the clamps; 20 and 130 lie outside them), wear up
    to 100, the slip angle at 5 (lateral heating), 17.04 (its cap of 8) and 45 (the wear factor's cap), and a ring
    whose mean lateral acceleration lies on either side of 2 g"""
    c.fill(_moving(pool(c.track), 10.0))
    n = np.arange(c.N)
    T = np.concatenate([around(85.0), around(105.0), around(25.0), around(120.0), [20.0, 130.0, 95.0, 60.0]])
    for i in range(4):
        c.f64("temp%d" % i)[:] = T[(n + 5 * i) % len(T)]
    Wr = np.concatenate([around(100.0)[:2], [99.99999, 0.0, 37.5]])
    for i in range(4):
        c.f64("wear%d" % i)[:] = Wr[(n // len(T) + i) % len(Wr)]
    cap = 5.0 + np.sqrt((8.0 - 2.2) / 0.04)
    S = np.concatenate([around(5.0), around(45.0), around(cap), [0.0, 2.0, 30.0, 90.0]])
    c.f64("slip")[:] = S[(n // 3) % len(S)]
    c.f64("lfm")[:] = np.array([0.0, 3000.0, 14000.0])[(n // 7) % 3]
    hot = (n // 11) % 4
    sel = hot >= 2                 # a full ring of lateral samples 20.0 (mean under 19.62 whatever the new one) / 23.5
    c.i32("acc_len")[sel] = 10
    c.A["acc"][1::2, sel] = np.where(hot[sel] == 2, 20.0, 23.5)
    c.act()[:, 0] = np.float32([1.0, 0.4, -0.6])[n % 3]
    c.act()[:, 1] = np.float32([0.4, -0.4, 0.0])[(n // 3) % 3]
    t0 = c.f64("temp0")
    c.want = dict(band0=np.where(t0 < 85.0, -1, np.where(t0 > 105.0, 1, 0)), slip_gt5=c.f64("slip") > 5.0,
                  worn0=c.f64("wear0") >= 100.0, latg=np.where(hot == 3, 1, np.where(hot == 2, -1, 0)))


def _weight_transfer(c):
    """a full ring of +-12 (the clip of every sample) and of +-40 (reachable by injection only: saturates the 95 %
    longitudinal cap and zeroes the lateral one), the new sample saturated too, below and above the aero gate"""
    c.fill(_moving(pool(c.track), 10.0))
    n = np.arange(c.N)
    sl, st = np.array([1.0, -1.0, 0.0])[n % 3], np.array([1.0, -1.0, 0.0])[(n // 3) % 3]
    mag = np.array([12.0, 40.0])[(n // 9) % 2]
    fast = (n // 18) % 2 == 1
    c.i32("acc_len")[:] = 10
    c.i32("acc_head")[:] = n % 10
    c.A["acc"][0::2] = sl * mag
    c.A["acc"][1::2] = st * mag
    qs, qc = c.f32("qs").astype(np.float64), c.f32("qc").astype(np.float64)
    s = np.where(fast, 70.0, 30.0)
    vx, vy = (qc * s).astype(np.float32), (qs * s).astype(np.float32)
    c.set_velocity(vx, vy)
    # previous velocity: the new sample is (v - pv) / dt projected on the heading and its normal, clipped to +-12
    c.f64("pvx")[:] = vx - (sl * qc - st * qs) * 1.0
    c.f64("pvy")[:] = vy - (sl * qs + st * qc) * 1.0
    c.act()[:, 0] = np.float32([1.0, -1.0])[(n // 36) % 2]
    c.want = dict(aero=speed32(c.A["f32"]) > 50.0, lon=sl * mag, lat=st * mag)


def _ring(c):
    """every (acc_len, acc_head): 11 x 10, the ring's slots holding distinct values"""
    c.fill(_moving(pool(c.track)))
    n = np.arange(c.N)
    c.i32("acc_len")[:] = n % 11
    c.i32("acc_head")[:] = (n // 11) % 10
    k = np.arange(20)[:, None] * 2400 + n[None, :]
    c.A["acc"][...] = ((k * 2654435761 % 4096) / 4096.0 - 0.5) * 24.0
    c.act()[:, 0] = np.float32([0.8, -0.8])[n % 2]
    c.act()[:, 1] = np.float32(0.2)
    c.want = dict(acc_len=n % 11, acc_head=(n // 11) % 10)


def bank_table(c):
    """the banking angles of the track's segments"""
    orc = OracleEnv(c.path, 1, 1)
    b = np.unique(orc.segments()[:, 12])
    orc.close()
    return b


def _bank(c):
    """every banking angle of the track's table (both sides of 0.1 degrees) x the gates of the banking force: speed
    at 1.0 and at 5.0"""
    c.fill(_moving(pool(c.track)))
    n = np.arange(c.N)
    tab = bank_table(c)
    assert (np.abs(tab) < 0.1).any() and (np.abs(tab) >= 0.1).any()
    c.f64("bank")[:] = tab[n % len(tab)]
    j = (n // len(tab)) % 8
    s = np.concatenate([around(1.0, np.float32), around(5.0, np.float32), np.float32([0.0, 40.0])])[j]
    free = j < 7                     # the last: the base state's own velocity
    d = (n // (8 * len(tab))) % 4
    vx = np.where(d == 0, s, np.where(d == 2, -s, 0)).astype(np.float32)
    vy = np.where(d == 1, s, np.where(d == 3, -s, 0)).astype(np.float32)
    c.set_velocity(vx[free], vy[free], free)
    c.act()[:, 0] = np.float32(0.7)
    sp = speed32(c.A["f32"])
    c.want = dict(banked=~(np.abs(c.f64("bank")) < 0.1), ge1=~(sp < 1.0), gt5=sp > 5.0)


def _stuck(c):
    """cars at rest (coasting: they stay where they are) with stuck_dur + dt next to 10 and 15 and the distance from
    the stuck start next to 1.0; cars moving at speeds next to 0.5 with and without a stuck start"""
    c.fill(_free(pool(c.track)))
    n = np.arange(c.N)
    rest = n % 2 == 0
    c.f32("vx")[rest] = 0.0; c.f32("vy")[rest] = 0.0; c.f32("w")[rest] = 0.0
    c.f64("pvx")[rest] = 0.0; c.f64("pvy")[rest] = 0.0
    k = n // 2
    dur = np.concatenate([_pre_sum(10.0, np.array([DT]))[:, 0], _pre_sum(15.0, np.array([DT]))[:, 0], [3.0, 12.0, 0.0]])
    c.f64("stuck_dur")[:] = dur[k % len(dur)]
    px = c.f32("xpx").astype(np.float64)
    m = np.concatenate([around(1.0), [0.0, 0.5, 2.0]])[(k // len(dur)) % 6]
    sx = px - 1.0                                       # exact: px is a float32
    j = (k // len(dur)) % 6
    sx = np.where(j == 0, np.nextafter(sx, np.inf), np.where(j == 2, np.nextafter(sx, -np.inf), np.where(j < 3, sx, px - m)))
    c.f64("stuck_sx")[:] = sx
    c.f64("stuck_sy")[:] = c.f32("xpy").astype(np.float64)
    c.i32("has_stuck_start")[:] = np.where((k // (6 * len(dur))) % 3 == 2, 0, 1)
    mv = ~rest
    s = np.concatenate([around(0.5, np.float32), np.float32([0.2, 0.8])])[k % 5]
    d = (k // 5) % 4
    c.set_velocity(np.where(d == 0, s, np.where(d == 2, -s, 0)).astype(np.float32)[mv],
                   np.where(d == 1, s, np.where(d == 3, -s, 0)).astype(np.float32)[mv], mv)
    c.f64("stuck_dur")[mv] = np.array([0.0, 1.0, 11.0])[(k // 20) % 3][mv]
    c.act()[:, 0] = 0.0
    c.act()[:, 1] = 0.0
    dx = px - c.f64("stuck_sx")
    c.want = dict(rest=rest, dur10=(c.f64("stuck_dur") + DT) > 10.0, dur15=(c.f64("stuck_dur") + DT) > 15.0,
                  moved_lt1=np.sqrt(dx * dx) < 1.0, slow=speed32(c.A["f32"]) < 0.5)


def _backward(c):
    """prog_hist placed relative to the progress the step will find (probe): going forwards, backwards with `back`
    reaching 25 and 200 exactly / next to them, and the two wraps at +-L / 2"""
    c.fill(_moving(pool(c.track)))
    c.i32("first_step")[:] = 0
    c.act()[:, 0] = np.float32(0.6)
    prog = c.probe()["f64"][f64i["prog_hist"]]          # the progress at the end of this step, whatever prog_hist is
    orc = OracleEnv(c.path, 1, 1)
    L = orc.total_length()
    orc.close()
    n = np.arange(c.N)
    kind = n % 12
    ph = np.where(kind < 7, prog + 3.0, prog - 2.0)     # pd = -3 (backwards) / +2 (forwards)
    half = np.where(prog < L / 2, prog + L / 2, prog - L / 2)    # pd = -+L / 2: next to the wrap
    for j in (9, 10, 11):
        ph = np.where(kind == j, half, ph)
    eps = 8.0 * np.spacing(L)       # a few ulps of the difference's own size
    ph = np.where(kind == 9, half - eps, np.where(kind == 11, half + eps, ph))
    pd = prog - ph
    c.f64("prog_hist")[:] = ph
    add = np.abs(pd)
    b25, b200 = (_pre_sum(t, np.where(kind < 7, add, 3.0)) for t in (25.0, 200.0))
    back = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5, kind == 6],
                     [b25[0], b25[1], b25[2], b200[0], b200[1], b200[2], np.full(c.N, 60.0)], 10.0)
    c.f64("back")[:] = back
    c.f64("prev_back")[:] = np.where(n // 12 % 2 == 0, back, np.minimum(back, 24.0))
    wrapped = np.where(pd > L / 2, pd - L, np.where(pd < -L / 2, pd + L, pd))
    newback = np.where(wrapped < 0, back + np.abs(wrapped), 0.0)
    c.want = dict(kind=kind, backwards=wrapped < 0, gt25=newback > 25.0, gt200=newback > 200.0,
                  wrap=(pd > L / 2) | (pd < -L / 2))
    c.meta = dict(prog=prog, L=L)


def _impact(c):
    """cars with no touching contact (the listener leaves `imp` alone): imp next to 100 and 50000 with imp_present 0 /
    1, cum_impact reaching 250000 exactly / next to it with and without this step's impulse; on the crowded scene also
    cars in contact, whose step impulses add to a cum_impact just under the limit"""
    P = pool(c.track)
    free = _free(P)
    c.fill(free)
    n = np.arange(c.N)
    imp = np.concatenate([around(100.0), around(50000.0), [0.0, 200.0, 200.0, 200.0, 50.0, 50.0, 50.0]])
    j = n % len(imp)
    c.f64("imp")[:] = imp[j]
    pres = (n // len(imp)) % 2
    c.i32("imp_present")[:] = pres
    cum = np.full(c.N, 1000.0)
    s = _pre_sum(250000.0, np.array([200.0]))[:, 0]
    for q in range(3):
        cum[j == 7 + q] = s[q]                  # + 200 -> next to the limit
        cum[j == 10 + q] = around(250000.0)[q]  # imp 50 is not added: cum_impact itself next to the limit
    c.f64("cum_impact")[:] = cum
    c.act()[:, 0] = np.float32(0.5)
    eff = np.where(pres == 1, c.f64("imp"), 0.0)
    cum2 = np.where(eff > 100.0, cum + eff, cum)
    c.want = dict(gt50000=eff > 50000.0, gt100=eff > 100.0, cum_gt=cum2 > 250000.0)
    c.meta = dict(live=np.zeros(c.N, bool))
    if c.track == "pocket":     # every third car: a base state in contact, as harvested
        touching = np.flatnonzero((P["i32"][i32i["nact"]] > 0) & (P["i32"][i32i["disabled"]] == 0))
        assert len(touching) > 20
        live = n % 3 == 2
        src = touching[(n * 5) % len(touching)]
        for k in ("f32", "f64", "i32", "acc"):
            c.A[k][:, live] = P[k][:, src[live]]
        for k in ("ct", "key", "n"):
            c.A[k][live] = P[k][src[live]]
        c.f64("cum_impact")[live] = np.array([249000.0, 249900.0, 0.0])[(n // 3) % 3][live]
        for k in c.want:
            c.want[k] = np.where(live, False, c.want[k])
        c.meta["live"] = live


def _lap_gate(c):
    """cars one step short of the start line's capsule, driving onto it: lt_cur next to 10 (sim - lt_start at sim =
    20), the lap distance after this step's move next to 0.95 L (probe), lt_crossed / lt_timing 0 / 1"""
    P = pool(c.track)
    fresh = np.flatnonzero((P["time"] == 0.0) & (P["f32"][f32i["xpx"]] == 0.0) & (P["f32"][f32i["xpy"]] == 0.0) &
                           (P["f32"][f32i["a"]] == 0.0))          # right after a reset at the track's own start
    c.fill(fresh)
    orc = OracleEnv(c.path, 1, 1)
    seg, L = orc.segments(), orc.total_length()
    orc.close()
    sl = seg[seg[:, 0] == 1.0][0]
    sx, sy, w = sl[2], sl[3], sl[6]
    assert sl[4] > sx and sl[5] == sy, "the start line is expected to run along +x"
    n = np.arange(c.N)
    v = np.float32(30.0)
    x = np.float32(sx - w / 2.0 - 0.25) - np.float32(0.001) * (n % 7).astype(np.float32)   # 0.25 m short; 0.5 m a step
    dx = x - c.f32("xpx")
    for f in ("cx", "xpx", "flox", "fhix"):
        c.f32(f)[:] = c.f32(f) + dx
    c.f32("cy")[:] = np.float32(sy); c.f32("xpy")[:] = np.float32(sy)
    c.set_velocity(np.full(c.N, v), np.zeros(c.N, np.float32))
    c.f64("pvx")[:] = 30.0
    c.f64("lt_px")[:] = c.f32("xpx").astype(np.float64) - 0.5
    c.f64("lt_py")[:] = sy
    c.i32("lt_has_pos")[:] = 1
    c.i32("first_step")[:] = 0
    c.f64("prev_px")[:] = c.f64("lt_px"); c.f64("prev_py")[:] = sy
    c.A["time"][:] = 20.0
    c.act()[:, 0] = np.float32(0.3)
    k = n // 7
    cr, tm = k % 2, (k // 2) % 2
    c.i32("lt_crossed")[:] = cr
    c.i32("lt_timing")[:] = tm
    cur = np.concatenate([around(10.0), [30.0, 30.0, 30.0, 30.0]])
    jc = (k // 4) % len(cur)
    c.f64("lt_start")[:] = 20.0 - cur[jc]          # exact
    c.f64("lt_cur")[:] = np.where(tm == 1, cur[jc], 0.0)
    c.f64("lt_dist")[:] = 0.0
    c.i32("lt_laps")[:] = (k // 28) % 2
    moved = c.probe()["f64"][f64i["lt_dist"]]      # from 0: this step's own move
    d = _pre_sum(0.95 * L, moved)
    jd = np.where(jc < 3, 3, jc - 3)               # lt_cur at the edge: far over the distance; else the distance's edge
    c.f64("lt_dist")[:] = np.where(jd == 0, d[0], np.where(jd == 1, d[1], np.where(jd == 2, d[2], L)))
    cur_now = np.where(tm == 1, 20.0 - c.f64("lt_start"), c.f64("lt_cur"))
    lap = (cr == 1) & (tm == 1) & ~(cur_now < 10.0) & ~((c.f64("lt_dist") + moved) < 0.95 * L)
    c.want = dict(lap=lap, first=cr == 0, cur_lt10=cur_now < 10.0, short=(c.f64("lt_dist") + moved) < 0.95 * L)
    c.meta = dict(moved=moved)


def termination_expect(c):
    """(terminated, truncated, reason) [E] of CarEnv._check_termination from the blob alone, for cars the step itself
    does not disable: the priority all-disabled > all-low-reward > time limit (reset_on_lap) > truncation, with a
    pending lap reset terminating on top"""
    dis = c.i32("disabled").reshape(c.E, c.C) != 0
    low = c.f32("cum_reward").reshape(c.E, c.C) < np.float32(-250.0)
    st = c.A["time"] + DT
    alld = dis.all(1)
    active = (~dis).sum(1)
    allow = (active > 0) & ((low & ~dis).sum(1) == active)
    reason = np.where(alld, 1, np.where(allow, 2, np.where(c.reset_on_lap & (st > 60.0), 3, np.where(st > 180.0, 4, 0))))
    term = (reason == 1) | (reason == 2) | (reason == 3) | (c.A["ei32"][1] != 0)
    return term, reason == 4, reason


def _termination(c):
    """C = 3.  Which cars are disabled (none, one, two, all) x the enabled cars' cum_reward (all under -250.0f, one at
    it, one over it by an ulp, all over) x the env's time (5 s; sim + dt next to 60 and to 180) x a pending lap reset"""
    assert c.C == 3
    c.fill(_moving(pool(c.track)))
    e = np.arange(c.E)
    dp, rp, tp, pend = e % 4, (e // 4) % 4, (e // 16) % 7, (e // 112) % 2
    dis = np.zeros((c.E, 3), np.int32)
    dis[dp >= 1, 0] = 1; dis[dp >= 2, 1] = 1; dis[dp == 3, 2] = 1
    c.i32("disabled")[:] = dis.ravel()
    lo, at, hi = around(-250.0, np.float32)
    cr = np.full((c.E, 3), lo, np.float32)
    cr[rp == 1, 2] = at; cr[rp == 2, 2] = hi; cr[rp == 3] = np.float32(-3.5)
    c.f32("cum_reward")[:] = cr.ravel()
    t60, t180 = _pre_sum(60.0, np.array([DT]))[:, 0], _pre_sum(180.0, np.array([DT]))[:, 0]
    c.A["time"][:] = np.concatenate([[5.0], t60, t180])[tp]
    c.A["ei32"][1] = pend
    c.act()[:, 0] = np.float32(0.5)
    term, trunc, reason = termination_expect(c)
    c.want = dict(term=term, trunc=trunc, reason=reason)


def _reset_dirty(c):
    """arbitrary harvested states (contacts, listener entries, laps, disabled cars and all); two envs in three are
    reset through the mask and none is stepped.  The banking angle survives a reset (Car.reset does not clear it)."""
    c.fill()
    c.mask = (np.arange(c.E) % 3 != 1).astype(np.uint8)
    c.want = dict(reset=c.mask != 0)


# ---------------------------------------------------------------- the track lookups, on the generated tracks
_pow = np.frompyfunc(math.pow, 2, 1)
_tracks = {}


def P2(x):
    """Python's x ** 2 as the reference and the oracle compute it: glibc's pow(x, 2.0)"""
    return _pow(np.asarray(x, np.float64), 2.0).astype(np.float64)


def track_tables(name):
    """(segments [S, 13], walls [nw, 4] centre / angle / half length, total length) of track `name`, from the oracle"""
    if name not in _tracks:
        orc = OracleEnv(track_path(name), 1, 1)
        _tracks[name] = (orc.segments(), orc.walls()[0], orc.total_length())
        orc.close()
    return _tracks[name]


def screen_eps(x, y):
    """the chord screen's bound (csrc/nascar_kernels.hip), in float64"""
    return 0.05 + 4e-6 * (np.abs(x) + np.abs(y))


def _clamp01(tt):
    tt = np.where(tt < 1.0, tt, 1.0)          # pymin(1, tt)
    return np.where(tt > 0.0, tt, 0.0)        # pymax(0, .)


def chord_search(seg, px, py):
    """Both nearest-chord searches of the step for positions px, py [N] (float64), each in its own arithmetic:
    d2 [N, S] and its first minimiser pbi (CarEnv._calculate_track_progress: squared distances, chords with ll < 1e-6
    stand for their start point), d [N, S] and bbi (CarPhysics.get_banking_angle_at_position: distances, only ll == 0
    is a point), and clamp [N]: -1 / +1 where the progress search's projection on its nearest chord was clamped at
    0 / at 1 (0: inside the chord, or a point chord)."""
    sx, sy, ex, ey = (seg[None, :, k] for k in (2, 3, 4, 5))
    px, py = np.asarray(px, np.float64)[:, None], np.asarray(py, np.float64)[:, None]
    dx, dy = ex - sx, ey - sy
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ll = dx * dx + dy * dy
        raw = ((px - sx) * dx + (py - sy) * dy) / ll
        tt = _clamp01(raw)
        point = ll < 1e-6
        qx, qy = np.where(point, sx, sx + tt * dx), np.where(point, sy, sy + tt * dy)
        d2 = P2(px - qx) + P2(py - qy)
        llb = P2(dx) + P2(dy)
        tb = _clamp01(((px - sx) * dx + (py - sy) * dy) / llb)
        zero = llb == 0
        bx, by = np.where(zero, sx, sx + tb * dx), np.where(zero, sy, sy + tb * dy)
        d = np.sqrt(P2(px - bx) + P2(py - by))
    pbi, bbi = np.argmin(d2, 1), np.argmin(d, 1)       # the first minimiser: the reference's strict '<' in index order
    n = np.arange(len(pbi))
    r = raw[n, pbi]
    clamp = np.where(point[0, pbi], 0, np.where(~(r > 0.0), -1, np.where(~(r < 1.0), 1, 0)))
    return dict(d2=d2, d=d, pbi=pbi, bbi=bbi, clamp=clamp)


def lookup_stats(seg, px, py):
    """what a set of positions reaches in the two searches (the counts tests/test_state_cases_cpu.py puts floors
    under): per car, the nearest chord of either search, whether a second chord lies within 2 screen_eps of the nearest,
    whether the two smallest distances of either search are equal or 1 ulp apart, whether the banking search's
    runner-up carries another banking than its winner, and the clamp"""
    s = chord_search(seg, px, py)
    n = np.arange(len(px))
    out = dict(pbi=s["pbi"], bbi=s["bbi"], clamp=s["clamp"])
    if seg.shape[0] == 1:
        z = np.zeros(len(px), bool)
        out.update(close=z, tie=z, bank_differs=z)
        return out
    od = np.argsort(s["d"], 1, kind="stable")
    d0, d1 = s["d"][n, od[:, 0]], s["d"][n, od[:, 1]]
    e0, e1 = np.sort(s["d2"], 1)[:, :2].T
    out["close"] = (d1 - d0) <= 2.0 * screen_eps(px, py)
    out["tie"] = ((d1 - d0) <= np.spacing(d0)) | ((e1 - e0) <= np.spacing(e0))
    out["bank_differs"] = seg[od[:, 0], 12] != seg[od[:, 1], 12]
    return out


def _unit(vx, vy):
    n = np.hypot(vx, vy)
    n = np.where(n > 0, n, 1.0)
    return vx / n, vy / n


def _steps32(v, k):
    """float32 v moved by k float32 neighbours (k an int array), as float64"""
    v = np.asarray(v, np.float32).copy()
    k = np.broadcast_to(np.asarray(k), v.shape)
    for _ in range(int(np.abs(k).max()) if k.size else 0):
        v = np.where(k > 0, np.nextafter(v, np.float32(np.inf)), np.where(k < 0, np.nextafter(v, np.float32(-np.inf)), v))
        k = k - np.sign(k)
    return v.astype(np.float64)


TIE_DIST = (0.0, 0.02, 0.5, 3.0, 7.0, 12.0, 40.0, 100.0, 200.0)


def tie_targets(name):
    """The positions of chord_ties on track `name`, by category ({category: [k, 2] float64}):
      wedge     beyond the joint of consecutive chords, on the outer side of the turn, where both projections clamp to
                the joint itself: exact ties (the lower index wins), at TIE_DIST from the joint over three directions;
      bisector  on the inner side, on the line equidistant from both chords' lines at TIE_DIST, and -2 .. 2 float32
                neighbours across it;
      ends      beyond either end of every chord along its own line, 0.5 .. 60 m out and up to 3 m aside;
      along     beside every chord, up to 6 m to either side;
      points    at and around the start points of the chords shorter than 1e-3 m (degenerate), and the centre of the
                four chords' square (ring4) with its float32 neighbours;
      far       |x| + |y| from 1e3 to 8e4 m over 16 directions."""
    seg = track_tables(name)[0]
    S = len(seg)
    sx, sy, ex, ey = seg[:, 2], seg[:, 3], seg[:, 4], seg[:, 5]
    ll = (ex - sx) ** 2 + (ey - sy) ** 2
    hd = np.radians(seg[:, 10])                         # a point chord: the heading the segment starts with
    ux = np.where(ll > 1e-6, (ex - sx) / np.sqrt(np.maximum(ll, 1e-300)), np.cos(hd))
    uy = np.where(ll > 1e-6, (ey - sy) / np.sqrt(np.maximum(ll, 1e-300)), np.sin(hd))
    cat = {k: [] for k in ("wedge", "bisector", "ends", "along", "points", "far")}
    closed = np.hypot(ex[-1] - sx[0], ey[-1] - sy[0]) < 1e-6
    for k in range(S if closed else S - 1):
        j = (k + 1) % S
        J = np.array([sx[j], sy[j]])
        bx, by = _unit(ux[j] - ux[k], uy[j] - uy[k])    # towards the inside of the turn
        if np.hypot(ux[j] - ux[k], uy[j] - uy[k]) < 1e-9:
            bx, by = -uy[k], ux[k]                      # collinear chords: the normal; both sides are "wedges"
            for t in TIE_DIST:
                for sgn in (1.0, -1.0):
                    cat["wedge"].append(J + sgn * t * np.array([bx, by]))
            continue
        for t in TIE_DIST:
            for rot in (-0.3, 0.0, 0.3):                # the wedge opens by the turn's angle about its centre line
                a = rot * 0.5 * np.arccos(np.clip(ux[j] * ux[k] + uy[j] * uy[k], -1, 1))
                ox, oy = -bx * np.cos(a) + by * np.sin(a), -bx * np.sin(a) - by * np.cos(a)
                cat["wedge"].append(J + t * np.array([ox, oy]))
            p = J + t * np.array([bx, by])
            for m in (-2, -1, 0, 1, 2):
                cat["bisector"].append(np.array([_steps32(p[0], m), p[1]]) if abs(by) > abs(bx) else
                                       np.array([p[0], _steps32(p[1], m)]))
    for k in range(S):
        for out in (0.5, 5.0, 25.0, 60.0):
            for side in (-3.0, 0.0, 3.0):
                cat["ends"].append(np.array([sx[k] - out * ux[k] - side * uy[k], sy[k] - out * uy[k] + side * ux[k]]))
                cat["ends"].append(np.array([ex[k] + out * ux[k] - side * uy[k], ey[k] + out * uy[k] + side * ux[k]]))
        for t in (0.1, 0.35, 0.65, 0.9):
            for side in (-6.0, -1.0, 0.0, 2.5):
                cat["along"].append(np.array([sx[k] + t * (ex[k] - sx[k]) - side * uy[k], sy[k] + t * (ey[k] - sy[k]) + side * ux[k]]))
    pts = [np.array([sx[k], sy[k]]) for k in range(S) if ll[k] < 1e-6]
    if name == "ring4":
        pts.append(np.array([sx.mean(), sy.mean()]))
    for p in pts:
        for r in (0.0, 1e-4, 1e-3, 0.3, 4.0):
            for a in range(8 if r else 1):
                cat["points"].append(p + r * np.array([np.cos(a * np.pi / 4), np.sin(a * np.pi / 4)]))
        for mx in (-1, 0, 1):
            for my in (-1, 0, 1):
                cat["points"].append(np.array([_steps32(p[0], mx), _steps32(p[1], my)]))
    mid = np.array([0.5 * (sx.min() + sx.max()), 0.5 * (sy.min() + sy.max())])
    for r in (1e3, 3e3, 1e4, 3e4, 6e4):
        for a in range(16):
            th = a * np.pi / 8 + 0.1
            cat["far"].append(mid + r * np.array([np.cos(th), np.sin(th)]))
    return {k: np.array(v, np.float64).reshape(-1, 2) for k, v in cat.items()}


TIE_SHARES = dict(wedge=7, bisector=7, ends=3, along=4, points=1, far=2)     # of 24 cars


def _deal(cat, N):
    """N targets dealt from the categories in the proportions TIE_SHARES (an empty category's share goes to `along`),
    each category cycled through with a stride that spreads the cars over the track"""
    order = [k for k, w in TIE_SHARES.items() for _ in range(w)]
    count = {k: 0 for k in cat}
    out = np.zeros((N, 2))
    for n in range(N):
        k = order[n % len(order)]
        if len(cat[k]) == 0:
            k = "along"
        out[n] = cat[k][(count[k] * 7) % len(cat[k])]
        count[k] += 1
    return out


def _calm(P, lo=None):
    """enabled cars that hold no contact record at all (so that moving them elsewhere leaves nothing stale); lo: and
    faster than `lo` m/s"""
    m = (P["i32"][i32i["disabled"]] == 0) & (P["i32"][i32i["nct"]] == 0) & (P["i32"][i32i["nact"]] == 0)
    if lo is not None:
        m &= (P["i32"][i32i["awake"]] == 1) & (speed32(P["f32"]) > lo)
    if m.sum() < 50:      # ring4 is all curve: every car's fat AABB meets a wall's.  Then: no touching contact
        free = _free(P)
        return free if lo is None else np.intersect1d(free, _moving(P, lo))
    return np.flatnonzero(m)


def _place(c, x, y):
    """every car's body moved to (x, y) (rounded to float32): sweep centre, transform and fat AABB alike"""
    for f, g, lo, hi, v in (("cx", "xpx", "flox", "fhix", x), ("cy", "xpy", "floy", "fhiy", y)):
        v = np.asarray(v, np.float64).astype(np.float32)
        d = v - c.f32(g)
        c.f32(lo)[:] = c.f32(lo) + d
        c.f32(hi)[:] = c.f32(hi) + d
        c.f32(f)[:] = v
        c.f32(g)[:] = v


def _rest(c, idx):
    """cars `idx` at rest, coasting: the step leaves a free body where it is"""
    for f in ("vx", "vy", "w"):
        c.f32(f)[idx] = 0.0
    c.f64("pvx")[idx] = 0.0; c.f64("pvy")[idx] = 0.0
    c.act()[idx] = 0.0


def _drive(c, idx, speed, throttle):
    """cars `idx` going `speed` m/s the way they face, on `throttle`"""
    qs, qc = c.f32("qs").astype(np.float64), c.f32("qc").astype(np.float64)
    vx, vy = (qc * speed).astype(np.float32), (qs * speed).astype(np.float32)
    c.set_velocity(vx[idx], vy[idx], idx)
    c.f64("pvx")[idx] = vx[idx]; c.f64("pvy")[idx] = vy[idx]
    c.act()[idx, 0] = np.float32(throttle)


def _post(A):
    """the body positions of arena sections A, as float64"""
    return A["f32"][f32i["xpx"]].astype(np.float64), A["f32"][f32i["xpy"]].astype(np.float64)


def _aim(c, tx, ty, moving):
    """place the cars so that the step ends at (tx, ty): the cars at rest there, the `moving` ones short of it by what
    the step moves them (probe).  Returns the oracle's positions after the step."""
    _place(c, tx, ty)
    if moving.any():
        x0, y0 = c.f32("xpx").astype(np.float64), c.f32("xpy").astype(np.float64)
        x1, y1 = _post(c.probe())
        _place(c, np.where(moving, tx - (x1 - x0), tx), np.where(moving, ty - (y1 - y0), ty))
    return _post(c.probe())


def _chord_ties(c):
    """tie_targets() dealt over the cars; one car in three drives (20 m/s the way it faces, on throttle), the others rest
    where they are put, so that float32 neighbours stay neighbours.  want: the nearest chord of either search at the
    oracle's position after the step."""
    P = pool(c.track)
    c.fill(_calm(P))
    n = np.arange(c.N)
    moving = n % 3 == 0
    _rest(c, ~moving)
    _drive(c, moving, 20.0, 0.6)
    c.i32("first_step")[:] = 0
    T = _deal(tie_targets(c.track), c.N)
    px, py = _aim(c, T[:, 0], T[:, 1], moving)
    s = chord_search(track_tables(c.track)[0], px, py)
    c.want = dict(pbi=s["pbi"], bbi=s["bbi"])
    c.meta = dict(px=px, py=py)


def capsule_dist(sl, x, y):
    """LapTimer._is_position_on_startline's distance from (x, y) to the chord of segment row `sl`, in its arithmetic"""
    sx, sy, dx, dy = sl[2], sl[3], sl[4] - sl[2], sl[5] - sl[3]
    ll = dx * dx + dy * dy
    assert ll >= 1e-6
    tt = _clamp01(((x - sx) * dx + (y - sy) * dy) / ll)
    return np.sqrt(P2(x - (sx + tt * dx)) + P2(y - (sy + tt * dy)))


def band_offsets(eps):
    """the 11 distances from the capsule's edge that startline_band aims at, for a screen bound of `eps`"""
    return np.array([0.0, 1e-6, -1e-6, eps / 2, -eps / 2, eps, -eps, 2 * eps, -2 * eps, 1.0, -1.0])


BAND_PLACES = 4      # left side, right side, round end at the chord's start, at its end
BAND_TOL = 2.5e-7    # how far a car's distance from the edge may lie from the offset it stands for


def _lattice_search(dist, target, x, y, M=200):
    """float32 positions next to (x, y) [N] whose dist() is closest to `target` [N]: for each of 2 M + 1 float32
    neighbours of x, the three neighbours of y around where the distance's slope puts the target"""
    ux, uy = np.spacing(x.astype(np.float32)).astype(np.float64), np.spacing(y.astype(np.float32)).astype(np.float64)
    h = 1e-3
    d0 = dist(x, y)
    gx, gy = (dist(x + h, y) - dist(x - h, y)) / (2 * h), (dist(x, y + h) - dist(x, y - h)) / (2 * h)
    # candidates [N, 2 M + 1, 3]: x moved by i float32 neighbours, i = -M .. M; for each i the y that the distance's
    # slope (gx, gy) puts on the target, as a count j of float32 neighbours, and the two next to it (the slope is only
    # a first guess around the round ends; every candidate's distance is then evaluated itself)
    i = np.arange(-M, M + 1)[None, :, None]
    col = lambda v: v[:, None, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        est = np.where(col(np.abs(gy * uy) > 1e-12),
                       (col(target - d0) - i * col(gx * ux)) / col(gy * uy), 0.0)
    j = np.clip(np.rint(est), -4 * M, 4 * M) + np.array([-1.0, 0.0, 1.0])[None, None, :]
    cx = (col(x) + i * col(ux)).astype(np.float32).astype(np.float64) + 0.0 * j
    cy = (col(y) + j * col(uy)).astype(np.float32).astype(np.float64)
    res = np.abs(dist(cx, cy) - col(target)) + 1e-13 * (np.abs(i) + np.abs(j))     # ties: the smallest move
    k = np.argmin(res.reshape(len(x), -1), 1)
    n = np.arange(len(x))
    return cx.reshape(len(x), -1)[n, k], cy.reshape(len(x), -1)[n, k]


def _startline_band(c):
    """Cars at rest whose position after the step lies at band_offsets() from the edge of the start line's capsule
    (distance width / 2 from its chord, in LapTimer's float64 arithmetic): along both sides and around both round
    ends, five places each.  A resting car stays where it is put, also on the sides, which are the walls' centre lines
    (a body that did not move enters no new contact), so each car takes the float32 position next to its place whose
    distance comes closest to the offset (_lattice_search).  The previous position is absent, off the line
    (10 m further out) or on it (the chord's midpoint); lt_crossed 1 / 0; the rest as lap_gate's passing case."""
    P = pool(c.track)
    c.fill(_calm(P))
    seg, _, L = track_tables(c.track)
    sl = seg[seg[:, 0] == 1.0][0]
    s, e, h = sl[2:4], sl[4:6], sl[6] / 2.0
    u = (e - s) / np.hypot(*(e - s))
    nl = np.array([-u[1], u[0]])
    n = np.arange(c.N)
    joff, place, sub, prev, cr = n % 11, (n // 11) % 4, (n // 44) % 5, (n // 220) % 3, (n // 660) % 2
    t = np.array([0.1, 0.3, 0.5, 0.7, 0.9])[sub]
    phi = np.radians(np.array([-60.0, -30.0, 0.0, 30.0, 60.0]))[sub]
    rot = lambda v, a: np.stack([v[0] * np.cos(a) - v[1] * np.sin(a), v[0] * np.sin(a) + v[1] * np.cos(a)], 1)
    nrm = np.where((place == 0)[:, None], nl[None], np.where((place == 1)[:, None], -nl[None],
                   np.where((place == 2)[:, None], rot(-u, phi), rot(u, phi))))
    foot = np.where((place < 2)[:, None], s[None] + t[:, None] * (e - s)[None], np.where((place == 2)[:, None], s[None], e[None]))
    B = foot + h * nrm
    off = band_offsets(1.0)[joff] * np.where((joff >= 3) & (joff <= 8), screen_eps(B[:, 0], B[:, 1]), 1.0)
    _rest(c, slice(None))
    c.i32("first_step")[:] = 0
    c.A["time"][:] = 20.0
    c.f64("lt_start")[:] = -10.0
    c.f64("lt_cur")[:] = 30.0
    c.f64("lt_dist")[:] = L
    c.i32("lt_timing")[:] = 1
    c.i32("lt_crossed")[:] = cr
    c.i32("lt_laps")[:] = (n // 1320) % 2
    x, y = (B[:, k] + off * nrm[:, k] for k in (0, 1))
    x, y = x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)
    sx, sy, dx, dy = sl[2], sl[3], sl[4] - sl[2], sl[5] - sl[3]

    def fast(px, py):      # capsule_dist with x * x for pow(x, 2.0): the same to an ulp, for the search alone
        tt = _clamp01(((px - sx) * dx + (py - sy) * dy) / (dx * dx + dy * dy))
        return np.hypot(px - (sx + tt * dx), py - (sy + tt * dy))
    x, y = _lattice_search(fast, h + off, x, y)
    _place(c, x, y)
    out = B + 10.0 * nrm
    mid = 0.5 * (s + e)
    c.f64("lt_px")[:] = np.where(prev == 2, mid[0], out[:, 0])
    c.f64("lt_py")[:] = np.where(prev == 2, mid[1], out[:, 1])
    c.i32("lt_has_pos")[:] = np.array([0, 1, 3])[prev]
    c.f64("prev_px")[:] = c.f64("lt_px"); c.f64("prev_py")[:] = c.f64("lt_py")
    px, py = _post(c.probe())
    dist = capsule_dist(sl, px, py)
    now, before, has = dist <= h, prev == 2, prev != 0
    c.want = dict(now=now, before=before, lap=has & now & ~before & (cr == 1), first=has & now & ~before & (cr == 0))
    c.meta = dict(px=px, py=py, edge=dist - h, off=off, joff=joff, place=place, h=h)


def _no_startline(c):
    """driving cars on the track without a STARTLINE, a previous position recorded 0.4 m behind them (every third: none),
    timing and crossed flags in all combinations: the lap timer adds the move to lt_dist and nothing else happens"""
    c.fill(_moving(pool(c.track)))
    n = np.arange(c.N)
    has = n % 3 != 2
    c.i32("lt_has_pos")[:] = has
    c.f64("lt_px")[:] = c.f32("xpx").astype(np.float64) - 0.4
    c.f64("lt_py")[:] = c.f32("xpy").astype(np.float64)
    c.i32("lt_crossed")[:] = (n // 3) % 2
    c.i32("lt_timing")[:] = (n // 6) % 2
    c.f64("lt_dist")[:] = np.where((n // 12) % 2 == 0, 0.0, track_tables(c.track)[2])
    c.A["time"][:] = 20.0
    c.f64("lt_start")[:] = -10.0
    c.act()[:, 0] = np.float32(0.5)
    c.want = dict(has=has, timing=c.i32("lt_timing") != 0)


def wall_query(walls, px, py, radius=0.5):
    """CarPhysics._check_wall_collision's decision for points (px, py) in float64 geometry (the engines work in
    float32): (on a wall, decided by the vertex distance -- inside no box, within `radius` of a box's corner --, the
    margin in metres by which the nearest box face / corner circle is missed or hit)"""
    on = np.zeros(len(px), bool)
    vert = np.zeros(len(px), bool)
    margin = np.full(len(px), np.inf)
    for lo in range(0, len(px), 256):
        x, y = px[lo:lo + 256, None] - walls[None, :, 0], py[lo:lo + 256, None] - walls[None, :, 1]
        cs, sn = np.cos(walls[None, :, 2]), np.sin(walls[None, :, 2])
        lx, ly = cs * x + sn * y, -sn * x + cs * y
        ax, ay = np.abs(lx) - walls[None, :, 3], np.abs(ly) - 0.5
        box = np.maximum(ax, ay)                          # <= 0: inside
        vd = np.hypot(ax, ay)                             # the nearest corner's distance
        inside = (box <= 0).any(1)
        near = (vd < radius).any(1)
        on[lo:lo + 256] = inside | near
        vert[lo:lo + 256] = ~inside & near
        margin[lo:lo + 256] = np.minimum(np.abs(box).min(1), np.abs(vd - radius).min(1))
    return on, vert, margin


GPU_MAX_ISLAND = 8    # csrc/nascar_layout.h MAX_ISLAND: touching contacts the device solves per island


def _on_track_query(c, keep_crowded=False):
    """Cars put next to the walls' faces (0.6 m inside to 0.6 m outside), around their corners (0.1 .. 1.1 m: the
    0.5 m radius tests the vertex distance), inside the boxes and far outside the broadphase grid; two in three rest,
    the others go 12 m/s.  The walls push back, so `want` is taken at the oracle's position after the step.
    keep_crowded: the island_overflow set, see _island_overflow."""
    P = pool(c.track)
    c.fill(_calm(P))
    walls = track_tables(c.track)[1]
    n = np.arange(c.N)
    kind = n % 8                       # 0-2 a face, 3-5 a corner, 6 inside, 7 far away
    w = walls[(n // 8 * 13) % len(walls)]
    cs, sn = np.cos(w[:, 2]), np.sin(w[:, 2])
    k = n // 8
    face = np.array([-0.6, -0.3, -0.01, 0.01, 0.2, 0.49, 0.51, 0.6])[k % 8]
    sgn = np.where((k // 8) % 2 == 0, 1.0, -1.0)
    along = np.array([-0.8, 0.0, 0.5, 0.97])[(k // 16) % 4]
    r = np.array([0.1, 0.45, 0.499, 0.5, 0.501, 0.55, 0.8, 1.1])[k % 8]
    th = (k // 8) % 12 * (np.pi / 6) + 0.05
    cx = np.where((k // 96) % 2 == 0, 1.0, -1.0) * w[:, 3]
    cy = np.where((k // 192) % 2 == 0, 0.5, -0.5)
    lx = np.select([kind < 3, kind < 6, kind == 6], [along * w[:, 3], cx + r * np.cos(th), along * w[:, 3]], 0.0)
    ly = np.select([kind < 3, kind < 6, kind == 6], [sgn * (0.5 + face), cy + r * np.sin(th), 0.4 * sgn * (k % 3 - 1)], 0.0)
    tx, ty = w[:, 0] + cs * lx - sn * ly, w[:, 1] + sn * lx + cs * ly
    far = kind == 7
    ang = k * 0.7
    rad = np.array([400.0, 2e3, 1e4, 5e4])[k % 4]
    tx, ty = np.where(far, w[:, 0] + rad * np.cos(ang), tx), np.where(far, w[:, 1] + rad * np.sin(ang), ty)
    moving = n % 3 == 0
    _rest(c, ~moving)
    _drive(c, moving, 12.0, 0.4)
    c.i32("first_step")[:] = 0
    for _ in range(3):
        px, py = _aim(c, tx, ty, moving)
        # The device solves islands of up to GPU_MAX_ISLAND touching contacts; more raise its error flag (overflow =
        # 2), as more than MAXC pairs do, and the oracle has no such limit.  A car that the oracle leaves with more
        # contact records than that, touching or not (so this asks more than the capacity does) -- inside the 1 m
        # chords of a tight curve -- goes to its wall's far-away place instead; _island_overflow keeps those cars.
        many = c.probe()["i32"][i32i["nct"]] > GPU_MAX_ISLAND
        if keep_crowded or not many.any():
            break
        tx, ty = np.where(many, w[:, 0] + rad * np.cos(ang), tx), np.where(many, w[:, 1] + rad * np.sin(ang), ty)
    assert keep_crowded or not many.any()
    on, vert, margin = wall_query(walls, px, py)
    c.want = dict(on_wall=on, vertex=vert)
    c.meta = dict(px=px, py=py, margin=margin, crowded=many)


def _island_overflow(c):
    """on_track_query's placement on `degenerate` as it first comes out, with the cars that on_track_query sends away:
    inside the 1 m wall chords of the tight curves the oracle leaves 21 of the 2400 cars with more than GPU_MAX_ISLAND
    contact records (c.meta["crowded"]), and the device raises its island-capacity error for one of them.  Not in SETS:
    these cars' states need not equal the oracle's; tests/test_gpu_generated_tracks.py::test_island_overflow_flag
    asserts the flag."""
    _on_track_query(c, keep_crowded=True)
    assert c.meta["crowded"].sum() >= 3


LOOKUP_INFO = ("on_track", "lap_distance", "speed")     # the or_car_info fields kept for the on_track_query sets

# name -> (builder, track, the layouts' C, reset_on_lap)
CLASSES = {
    "speed_gates": (_speed_gates, "daytona", (1, 10), False),
    "input_gates": (_input_gates, "martinsville", (1, 10), False),
    "rpm": (_rpm, "daytona", (1,), False),
    "tyres": (_tyres, "daytona", (1, 10), False),
    "weight_transfer": (_weight_transfer, "martinsville", (1,), False),
    "ring": (_ring, "daytona", (1, 10), False),
    "bank": (_bank, "daytona", (1,), False),
    "bank_martinsville": (_bank, "martinsville", (10,), False),
    "stuck": (_stuck, "daytona", (1, 10), False),
    "backward": (_backward, "daytona", (1, 10), False),
    "impact": (_impact, "daytona", (1,), False),
    "impact_crowded": (_impact, "pocket", (10,), False),
    "lap_gate": (_lap_gate, "daytona", (1, 10), False),
    "lap_gate_reset_on_lap": (_lap_gate, "martinsville", (1, 10), True),
    "termination": (_termination, "daytona", (3,), False),
    "termination_reset_on_lap": (_termination, "martinsville", (3,), True),
    "reset_dirty": (_reset_dirty, "martinsville", (10,), False),
    "reset_dirty_crowded": (_reset_dirty, "pocket", (1, 10), False),
    "chord_ties_seg64": (_chord_ties, "seg64", (1, 10), False),
    "chord_ties_seg17": (_chord_ties, "seg17", (1,), False),
    "chord_ties_ring4": (_chord_ties, "ring4", (10,), False),
    "chord_ties_degenerate": (_chord_ties, "degenerate", (1,), False),
    "startline_band_seg64": (_startline_band, "seg64", (1, 10), False),
    "startline_band_degenerate": (_startline_band, "degenerate", (10,), False),
    "no_startline": (_no_startline, "nostart", (10,), False),
    "on_track_query_seg64": (_on_track_query, "seg64", (10,), False),
    "on_track_query_degenerate": (_on_track_query, "degenerate", (1,), False),
}
SETS = [(name, C) for name, (_, _, Cs, _) in CLASSES.items() for C in Cs]
# sets that run outside the one-step comparison (build() takes them too)
EXTRA = {"island_overflow": (_island_overflow, "degenerate", (1,), False)}


def build(name, C):
    """the case set of class `name` in the E x C layout, built once per process; read-only"""
    if (name, C) not in _built:
        fn, track, Cs, rol = CLASSES[name] if name in CLASSES else EXTRA[name]
        assert C in Cs
        c = Cases(name, track, C, rol)
        fn(c)
        _built[name, C] = c.done()
    return _built[name, C]


def predicate(c):
    """The gate sides of every case recomputed from the blob and the actions alone, in each gate's own arithmetic;
    keys as c.want.  (The sides that depend on what the step adds -- backward, lap_gate -- take the probed addend from
    c.meta, which the CPU test checks against the oracle's step.)"""
    A = gpu_arena(c.blob, c.E, c.C)
    f64 = lambda f: A["f64"][f64i[f]]
    i32 = lambda f: A["i32"][i32i[f]]
    sp = speed32(A["f32"])
    act = c.actions.reshape(c.N, 2).astype(np.float64)
    base = c.name.split("_reset_on_lap")[0].replace("_martinsville", "").replace("_crowded", "")
    for t in track_gen.FAMILY:
        if base.endswith("_" + t):
            base = base[:-len(t) - 1]
            break
    if base == "speed_gates":
        thr = np.array(SPEED_GATES)[c.want["gate"]]
        return dict(gate=c.want["gate"], above=sp > thr, below=sp < thr)
    if base == "input_gates":
        dis = i32("disabled") != 0
        a = np.where(dis[:, None], 0.0, act)
        thr, brk = np.where(a[:, 0] >= 0, a[:, 0], 0.0), np.where(a[:, 0] >= 0, 0.0, -a[:, 0])
        return dict(thr_on=np.minimum(thr, 1.0) > 0.01, brk_on=np.minimum(brk, 1.0) > 0.01,
                    steer_on=np.abs(np.clip(a[:, 1], -1, 1) * STEER_K) > 0.01, disabled=dis)
    if base == "rpm":
        thr = np.clip(act[:, 0], 0, 1)
        _, unit, lo, hi = rpm_next(f64("rpm"), thr)
        den = ((1000.0 + 800.0 * thr) - f64("rpm")) + 0.1
        return dict(unit=unit, lo=lo, hi=hi, tiny_den=np.sign(den) * (np.abs(den) < 1e-12))
    if base == "tyres":
        t0 = f64("temp0")
        full = i32("acc_len") == 10
        lat = A["acc"][1::2]
        lo_mean, hi_mean = (lat.sum(0) - lat.max(0) - 12.0) / 10.0, (lat.sum(0) - lat.min(0) + 12.0) / 10.0
        latg = np.where(full & (lo_mean / 9.81 > 2.0), 1, np.where(full & (lat.min(0) > 12.0) & (hi_mean / 9.81 < 2.0), -1, 0))
        return dict(band0=np.where(t0 < 85.0, -1, np.where(t0 > 105.0, 1, 0)), slip_gt5=f64("slip") > 5.0,
                    worn0=f64("wear0") >= 100.0, latg=latg)
    if base == "weight_transfer":
        return dict(aero=sp > 50.0, lon=A["acc"][0], lat=A["acc"][1])
    if base == "ring":
        return dict(acc_len=i32("acc_len"), acc_head=i32("acc_head"))
    if base == "bank":
        return dict(banked=~(np.abs(f64("bank")) < 0.1), ge1=~(sp < 1.0), gt5=sp > 5.0)
    if base == "stuck":
        dx = A["f32"][f32i["xpx"]].astype(np.float64) - f64("stuck_sx")
        dy = A["f32"][f32i["xpy"]].astype(np.float64) - f64("stuck_sy")
        rest = (A["f32"][f32i["vx"]] == 0) & (A["f32"][f32i["vy"]] == 0) & (act == 0).all(1)
        return dict(rest=rest, dur10=(f64("stuck_dur") + DT) > 10.0, dur15=(f64("stuck_dur") + DT) > 15.0,
                    moved_lt1=np.sqrt(dx * dx + dy * dy) < 1.0, slow=sp < 0.5)
    if base == "backward":
        L, pd = c.meta["L"], c.meta["prog"] - f64("prog_hist")
        wrap = (pd > L / 2) | (pd < -L / 2)
        pd = np.where(pd > L / 2, pd - L, np.where(pd < -L / 2, pd + L, pd))
        nb = np.where(pd < 0, f64("back") + np.abs(pd), 0.0)
        return dict(kind=c.want["kind"], backwards=pd < 0, gt25=nb > 25.0, gt200=nb > 200.0, wrap=wrap)
    if base == "impact":
        eff = np.where(i32("imp_present") != 0, f64("imp"), 0.0)
        cum2 = np.where(eff > 100.0, f64("cum_impact") + eff, f64("cum_impact"))
        live = c.meta["live"]
        return dict(gt50000=(eff > 50000.0) & ~live, gt100=(eff > 100.0) & ~live, cum_gt=(cum2 > 250000.0) & ~live)
    if base == "lap_gate":
        orc = OracleEnv(c.path, 1, 1)
        L = orc.total_length()
        orc.close()
        tm, cr = i32("lt_timing") != 0, i32("lt_crossed") != 0
        cur = np.where(tm, np.repeat(A["time"], c.C) - f64("lt_start"), f64("lt_cur"))
        short = (f64("lt_dist") + c.meta["moved"]) < 0.95 * L
        return dict(lap=cr & tm & ~(cur < 10.0) & ~short, first=~cr, cur_lt10=cur < 10.0, short=short)
    if base == "termination":
        term, trunc, reason = termination_expect(c)
        return dict(term=term, trunc=trunc, reason=reason)
    if base == "reset_dirty":
        return dict(reset=c.mask != 0)
    # The lookups read the position the step ends at: c.meta holds it (the CPU test checks it against the oracle's
    # step).  For chord_ties and on_track_query this calls the builder's own function on the builder's own positions,
    # so agreement with `want` says nothing by itself: what checks these sets independently is the oracle's step, in
    # test_chord_ties_reach (its bank and prog_hist against the chord `want` names) and test_on_track_query_outcomes
    # (its on_track against wall_query).
    if base == "chord_ties":
        s = chord_search(track_tables(c.track)[0], c.meta["px"], c.meta["py"])
        return dict(pbi=s["pbi"], bbi=s["bbi"])
    if base == "startline_band":
        seg = track_tables(c.track)[0]
        sl = seg[seg[:, 0] == 1.0][0]
        has = (i32("lt_has_pos") & 1) != 0
        now = capsule_dist(sl, c.meta["px"], c.meta["py"]) <= sl[6] / 2.0
        before = has & (capsule_dist(sl, f64("lt_px"), f64("lt_py")) <= sl[6] / 2.0)
        assert np.array_equal(before, (i32("lt_has_pos") & 2) != 0)      # the device's cached bit is consistent
        cr = i32("lt_crossed") != 0
        return dict(now=now, before=before, lap=has & now & ~before & cr, first=has & now & ~before & ~cr)
    if base == "no_startline":
        return dict(has=i32("lt_has_pos") != 0, timing=i32("lt_timing") != 0)
    if base == "on_track_query":
        on, vert, _ = wall_query(track_tables(c.track)[1], c.meta["px"], c.meta["py"])
        return dict(on_wall=on, vertex=vert)
    raise KeyError(c.name)


_stepped = {}
_info = {}


def oracle_step(name, C):
    """The oracle's side of a case set, computed once per process and shared: (state sections after the step -- after
    reset(mask) for reset_dirty --, obs, reward, car flags, env flags)."""
    if (name, C) not in _stepped:
        c = build(name, C)
        orc = c.oracle()
        if c.mask is not None:
            for e in np.flatnonzero(c.mask):
                orc.reset(int(e))
            out = orc.outputs()
        else:
            out = orc.step(c.actions)
        A = oracle_arena(orc)
        if name.startswith("on_track_query"):
            rows = np.array([[orc.car_info(n)[f] for f in LOOKUP_INFO] for n in range(c.N)], np.float64)
            rows.setflags(write=False)
            _info[name, C] = rows
        orc.close()
        for a in list(A.values()) + list(out):
            a.setflags(write=False)
        _stepped[name, C] = (A,) + tuple(out)
    return _stepped[name, C]


def oracle_info(name, C):
    """or_car_info's LOOKUP_INFO columns [N, 3] after oracle_step(name, C), for the on_track_query sets"""
    oracle_step(name, C)
    return _info[name, C]

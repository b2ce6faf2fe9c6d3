"""Case classes for the car-car contact solver (nascar_set_car_contact).  TEST INFRASTRUCTURE, CPU only.

A case is one env of C car bodies, 7 float32 each: x y qs qc vx vy w -- what the solver loads.  A class (CaseSet) is a
batch of such envs [E, C, 7]: tests/test_gpu_car_contact.py runs it through the device (nascar_debug_car_contact) and
through the oracle (oracle_lib.car_contact, Box2D's algorithm for two dynamic bodies) and compares them bit for bit;
tests/test_car_contact_cpu.py pins on the oracle alone that every class reaches what it was built for.

Every class records per env what it was built to reach (`want`); its `reach` recomputes that label from the oracle's
outputs alone (contact counts, pairs, impulses, velocities), where a gate is involved in the gate's own float32
arithmetic (vrel32: b2ContactSolver's vB + wB x rB - vA - wA x rA, left to right), and the two must agree for every env.
`need` lists the labels a class must contain.

Geometry used throughout: the car box is 5.042 x 1.996 m (half extents HX, HY as float32), its polygon radius 0.01 m,
so two boxes touch while the largest face separation is <= 0.02 m.  `face2` puts two cars nose to tail 0.01 m apart (a
two-point manifold, normal exactly (1, 0)); `corner1` turns the second car by 45 degrees so that one corner meets the
first car's nose face (a one-point manifold, the same normal).  With that normal and no spin the relative normal speed
is the difference of two float32 x-velocities, exactly.

The write-back class comes from a seeded search (WB_SEED, WB_SEARCH random three-car piles): a contact whose last normal
pass brought its normal impulse to 0 while its friction impulse, clamped by the iteration before, stayed non-zero
(`zero_normal`), and among those a car that no contact gave a normal impulse but whose velocity changed (`unstored`:
the car the step's former `jmax > 0` write-back rule lost).  The search finds 350 piles with such a contact (1.8 %), 34 of them with such a car (0.2 %).
"""
import numpy as np

import oracle_lib

f32 = np.float32
HX, HY = f32(5.042 / 2.0), f32(1.996 / 2.0)
R_TOTAL = 0.02                       # 2 * b2_polygonRadius
GAP = float(2.0 * HX) + 0.01         # nose to tail, faces 0.01 m apart: touching
FRICTION = f32(0.7)
ONE = f32(1.0)
ONE_UP, ONE_DOWN = np.nextafter(ONE, f32(2.0)), np.nextafter(ONE, f32(0.0))
CULL = f32(5.7)
WB_SEED, WB_SEARCH, WB_KEEP = 20261, 20000, 16
NAMES = ["gate", "friction", "angular", "cull", "chain3", "chain4", "chain10", "star", "writeback", "pile4", "pile10",
         "layout1", "layout2", "layout3", "layout10", "layout64"]          # every class all_sets() builds
LAYOUT_E = {1: 2 * 128 + 5, 2: 2 * 64 + 5, 3: 2 * 42 + 7, 10: 2 * 12 + 5, 64: 5}   # the last workgroup is partial


def body(x, y, ang=0.0, vx=0.0, vy=0.0, w=0.0):
    """one body row; angle 0 gives the rotation (0, 1) exactly"""
    return np.array([x, y, np.sin(ang), np.cos(ang), vx, vy, w], np.float64).astype(f32)


def vrel32(a, b, normal, point):
    """the solver's relative normal speed of bodies a, b (rows) at a world point, in float32, in Box2D's association"""
    a, b = a.astype(f32), b.astype(f32)
    n, p = np.asarray(normal, f32), np.asarray(point, f32)
    rA, rB = (p[0] - a[0], p[1] - a[1]), (p[0] - b[0], p[1] - b[1])
    dvx = ((b[4] + (-b[6] * rB[1])) - a[4]) - (-a[6] * rA[1])
    dvy = ((b[5] + b[6] * rB[0]) - a[5]) - (a[6] * rA[0])
    return f32(f32(n[0] * dvx) + f32(n[1] * dvy))


class CaseSet:
    def __init__(self, name, C, envs, want, reach, need):
        self.name, self.C = name, C
        self.bodies = np.ascontiguousarray(np.stack(envs).astype(f32).reshape(len(envs), C, 7))
        self.want, self.reach, self.need = list(want), reach, set(need)
        self._res = {}
        assert len(self.want) == len(self.bodies)

    @property
    def E(self):
        return len(self.bodies)

    def solve(self, cap=None, cull=True):
        key = (cap, cull)
        if key not in self._res:
            self._res[key] = oracle_lib.car_contact(self.bodies, self.C, cap, cull)
        return self._res[key]

    def reached(self):
        """the labels recomputed from the oracle's outputs, one per env"""
        r = self.solve()
        return [self.reach(self, r, e) for e in range(self.E)]


def _points(r, e, k=0):
    """contact k of env e: (i, j, point count, normal, points [2, 2], ni [2], ti [2], clamp ni [2])"""
    i, j, n = r["pairs"][e, k]
    c = r["con"][e, k]
    return int(i), int(j), int(n), c[0:2], c[2:6].reshape(2, 2), c[6:10:2], c[7:10:2], c[10:12]


# ---------------------------------------------------------------- two-car geometries
def _corner_x():
    """x of the 45-degree car's centre whose lowest-x corner sits 0.005 m off the first car's nose face; that corner
    lies (HX - HY) * sqrt(0.5) = 1.077 m below the centre, so centre offsets y in (0.1, 2.05) keep it on the face"""
    return float(HX) + 0.005 + (float(HX) + float(HY)) * np.sqrt(0.5)


def _pair(geo, va=(0.0, 0.0), vb=(0.0, 0.0), wa=0.0, wb=0.0, yoff=None):
    if geo == "face2":
        return [body(0.0, 0.0, 0.0, va[0], va[1], wa), body(GAP, 0.3 if yoff is None else yoff, 0.0, vb[0], vb[1], wb)]
    return [body(0.0, 0.0, 0.0, va[0], va[1], wa),
            body(_corner_x(), 0.2 if yoff is None else yoff, np.pi / 4.0, vb[0], vb[1], wb)]


def _geo_of(n):
    return "face2" if n == 2 else "corner1"


# ---------------------------------------------------------------- restitution gate
GATE_SPEEDS = {"open": ONE_UP, "at": ONE, "below": ONE_DOWN, "rest": f32(0.0), "sep": f32(-1.5)}


def _gate_reach(cs, r, e):
    if r["solved"][e] != 1:
        return ("none",)
    i, j, n, nrm, pts, ni, ti, _ = _points(r, e)
    vr = {float(vrel32(cs.bodies[e, i], cs.bodies[e, j], nrm, pts[q])) for q in range(n)}
    if len(vr) != 1:
        return ("mixed",)
    vr = f32(vr.pop())
    side = ("open" if vr == -ONE_UP else "at" if vr == -ONE else "below" if vr == -ONE_DOWN else
            "rest" if vr == 0 else "sep" if vr > 0 else "other")
    if side == "sep" and (ni[:n].any() or not np.array_equal(r["out"][e, :, :3], cs.bodies[e, :, 4:7])):
        side = "sep_with_impulse"
    if side in ("open", "at", "below") and not (ni[:n] > 0).all():
        side += "_no_impulse"
    return (_geo_of(n), side)


def gate():
    envs, want = [], []
    for geo in ("face2", "corner1"):
        for side, s in GATE_SPEEDS.items():
            for mover in ("a", "b"):      # the first car runs into the second, or the second backs into the first
                envs.append(np.stack(_pair(geo, va=(s, 0.0)) if mover == "a" else _pair(geo, vb=(-s, 0.0))))
                want.append((geo, side))
    return CaseSet("gate", 2, envs, want, _gate_reach, set(want))


# ---------------------------------------------------------------- friction
def _friction_reach(cs, r, e):
    if r["solved"][e] != 1:
        return "none"
    _, _, n, _, _, ni, ti, clamp = _points(r, e)
    if n != 1 or not ni[0] > 0:
        return "none"
    bound = f32(FRICTION * clamp[0])      # the clamp of the last friction pass, as the solver forms it
    if ti[0] == bound and ti[0] > 0:
        return "clamp+"
    if ti[0] == -bound and ti[0] < 0:
        return "clamp-"
    return "inside" if ti[0] != 0 and abs(ti[0]) < bound else "none"


def friction():
    envs, want = [], []
    for yoff in (0.2, 1.6):
        for vt, lab in ((30.0, "clamp-"), (-30.0, "clamp+"), (20.0, "clamp-"), (-25.0, "clamp+"), (0.3, "inside"),
                        (-0.25, "inside"), (4.0, "inside")):
            envs.append(np.stack(_pair("corner1", va=(3.0, vt), yoff=yoff)))
            want.append(lab)
    return CaseSet("friction", 2, envs, want, _friction_reach, {"clamp+", "clamp-", "inside"})


# ---------------------------------------------------------------- angular response
def _angular_reach(cs, r, e):
    if r["solved"][e] != 1:
        return "none"
    spun = int((cs.bodies[e, :, 6] != 0).sum())
    dw = r["out"][e, :, 2] - cs.bodies[e, :, 6]
    if not (dw != 0).all():
        return "no_response"
    return {1: "one", 2: "both"}.get(spun, "none")


def angular():
    envs, want = [], []
    for wa, wb in ((1.5, 0.0), (0.0, -2.0), (1.2, -0.8), (-1.0, 1.0)):
        for geo, yoff in (("corner1", 0.6), ("corner1", 1.7), ("face2", 0.9)):
            envs.append(np.stack(_pair(geo, va=(4.0, 0.5), vb=(-1.0, 0.0), wa=wa, wb=wb, yoff=yoff)))
            want.append("one" if wa == 0.0 or wb == 0.0 else "both")
    return CaseSet("angular", 2, envs, want, _angular_reach, {"one", "both"})


# ---------------------------------------------------------------- cull reach
def cull_reach_limit():
    """centre distance up to which two cars touch corner to corner along their common diagonal: the gap g between the
    corners is seen by the nose face at g * HX / R (its normal lies at atan2(HY, HX) from the diagonal)"""
    R = float(np.hypot(float(HX), float(HY)))
    return 2.0 * R + R_TOTAL * R / float(HX)


def _cull_reach(cs, r, e):
    return "touch" if r["solved"][e] == 1 else "apart"


def cull():
    envs, want = [], []
    lim = cull_reach_limit()
    diag = float(np.arctan2(float(HY), float(HX)))
    for axis in (0, 1):
        ang = -diag if axis == 0 else np.pi / 2.0 - diag       # the (HX, HY) corner on the +x / +y axis
        ds = [5.40 + 0.001 * k for k in range(51)] + [float(np.nextafter(CULL, f32(0.0))), float(CULL),
                                                     float(np.nextafter(CULL, f32(9.0)))]
        for d in ds:
            assert abs(d - lim) > 1e-4, d                      # no case within rounding of the limit
            p = (d, 0.0) if axis == 0 else (0.0, d)
            v = (-2.0, 0.0) if axis == 0 else (0.0, -2.0)
            envs.append(np.stack([body(0.0, 0.0, ang), body(p[0], p[1], ang, v[0], v[1])]))
            want.append("touch" if d < lim else "apart")
    return CaseSet("cull", 2, envs, want, _cull_reach, {"touch", "apart"})


# ---------------------------------------------------------------- chains and stars
def _chain_reach(cs, r, e):
    C = cs.C
    n = int(r["solved"][e])
    if n != C - 1 or r["dropped"][e] or [tuple(p[:2]) for p in r["pairs"][e, :n]] != [(k, k + 1) for k in range(C - 1)]:
        return "none"
    return ("fwd" if r["out"][e, :, 0].astype(np.float64).sum() > 0 else "bwd", int((r["out"][e, :, 3] > 0).sum()))


def chain(C):
    envs, want = [], []
    # the impulse travels with the pair order (through the whole row in the first iteration) or against it (one pair
    # further per iteration: 6 iterations reach 7 cars)
    for d in ("fwd", "bwd"):
        for v in (5.0, 0.9):
            env = [body(k * GAP, 0.1 * (-1) ** k) for k in range(C)]
            env[0 if d == "fwd" else C - 1][4] = f32(v if d == "fwd" else -v)
            envs.append(np.stack(env))
            want.append((d, C if d == "fwd" else min(C, 7)))
    return CaseSet(f"chain{C}", C, envs, want, _chain_reach, set(want))


def _star_reach(cs, r, e):
    n = int(r["solved"][e])
    if n != 3 or r["dropped"][e]:
        return "none"
    common = set(r["pairs"][e, 0, :2]) & set(r["pairs"][e, 1, :2]) & set(r["pairs"][e, 2, :2])
    return ("star", int(common.pop())) if len(common) == 1 else "none"


def star():
    hub = body(0.0, 0.0)
    arms = [body(GAP, 0.2, 0.0, -4.0, 0.0), body(-GAP, -0.2, 0.0, 3.0, 0.3), body(-0.5, float(2.0 * HY) + 0.01, 0.0, 0.4, -2.0)]
    envs, want = [], []
    for at in range(4):            # the hub as car 0 .. 3: the pair order around it changes
        env = list(arms)
        env.insert(at, hub)
        envs.append(np.stack(env))
        want.append(("star", at))
    return CaseSet("star", 4, envs, want, _star_reach, set(want))


# ---------------------------------------------------------------- random piles: write-back gate, capacity
def _pile(rng, n, C, sx, sy, v=8.0, w=3.0):
    b = np.zeros((n, C, 7), np.float64)
    b[:, :, 0] = rng.uniform(-sx, sx, (n, C))
    b[:, :, 1] = rng.uniform(-sy, sy, (n, C))
    a = rng.uniform(-np.pi, np.pi, (n, C))
    b[:, :, 2], b[:, :, 3] = np.sin(a), np.cos(a)
    b[:, :, 4:6] = rng.uniform(-v, v, (n, C, 2))
    b[:, :, 6] = rng.uniform(-w, w, (n, C))
    return b.astype(f32)


def _wb_reach(cs, r, e):
    n = int(r["solved"][e])
    zero = False
    for k in range(n):
        _, _, m, _, _, ni, ti, _ = _points(r, e, k)
        zero |= bool(((ni[:m] == 0) & (ti[:m] != 0)).any())
    if not zero:
        return "none"
    touched = np.zeros(cs.C, bool)
    touched[r["pairs"][e, :n, :2].ravel()] = True
    moved = (r["out"][e, :, :3] != cs.bodies[e, :, 4:7]).any(1)
    return "unstored" if (touched & moved & (r["out"][e, :, 3] == 0)).any() else "zero_normal"


def writeback():
    """the seeded search of the module docstring; its first WB_KEEP hits of either kind"""
    cand = CaseSet("wb_search", 3, list(_pile(np.random.default_rng(WB_SEED), WB_SEARCH, 3, 2.8, 1.5)),
                   ["none"] * WB_SEARCH, _wb_reach, ())
    lab = np.array(cand.reached())
    envs, want = [], []
    for kind in ("zero_normal", "unstored"):
        for e in np.nonzero(lab == kind)[0][:WB_KEEP]:
            envs.append(cand.bodies[e])
            want.append(kind)
    return CaseSet("writeback", 3, envs, want, _wb_reach, {"zero_normal", "unstored"}) if envs else None


def _pile_reach(cs, r, e):
    return "pile" if r["solved"][e] == cs.C and r["dropped"][e] > 0 else "none"


def pile(C):
    """C cars heaped on one spot: every pair touches, C (C - 1) / 2 > C of them"""
    b = _pile(np.random.default_rng(400 + C), 8, C, 1.0, 0.5)
    return CaseSet(f"pile{C}", C, list(b), ["pile"] * len(b), _pile_reach, {"pile"})


# ---------------------------------------------------------------- layout
def _row_env(rng, C, touching):
    """C cars in a row along x, slightly turned, moving at random: neighbours nose to tail (touching) or 8 m apart"""
    gaps = np.where(rng.random(max(C - 1, 0)) < 0.5, GAP, 8.0) if touching else np.full(max(C - 1, 0), 8.0)
    if touching and C > 1 and not (gaps == GAP).any():
        gaps[rng.integers(C - 1)] = GAP
    x = np.concatenate([[0.0], np.cumsum(gaps)]) + rng.uniform(-50.0, 50.0)
    return np.stack([body(x[k], rng.uniform(-0.2, 0.2), rng.uniform(-0.03, 0.03), rng.uniform(-5, 5), rng.uniform(-5, 5),
                          rng.uniform(-1, 1)) for k in range(C)])


def _layout_reach(cs, r, e):
    return "contact" if r["solved"][e] > 0 else "free"


def layout(C):
    """whole and partial workgroups of C-car envs; contact envs interleaved with contact-free ones; env 1 and the last
    env repeat env 0's coordinates with other velocities (nothing may leak from one env into another)"""
    rng = np.random.default_rng(900 + C)
    E = LAYOUT_E[C]
    envs, want = [], []
    for e in range(E):
        touching = C > 1 and e % 3 != 2
        env = _row_env(rng, C, touching)
        if e in (1, E - 1):
            env = envs[0].copy()
            env[:, 4:7] = rng.uniform(-4.0, 4.0, (C, 3)).astype(f32)
            touching = C > 1
        envs.append(env)
        want.append("contact" if touching else "free")
    return CaseSet(f"layout{C}", C, envs, want, _layout_reach, {"free"} if C == 1 else {"contact", "free"})


_all = None


def all_sets():
    """every class, built once per process"""
    global _all
    if _all is None:
        sets = [gate(), friction(), angular(), cull(), chain(3), chain(4), chain(10), star(), writeback(), pile(4),
                pile(10)] + [layout(C) for C in sorted(LAYOUT_E)]
        _all = [s for s in sets if s is not None]
    return _all

"""The car-car contact case classes (tests/car_contact_cases.py) on the oracle alone (or_car_contact): every class
reaches what it was built for, and the solve has the properties of Box2D's sequential impulses, checked in float64
arithmetic on the oracle's float32 outputs.  No GPU."""
import numpy as np
import pytest

import car_contact_cases as cc

NAMES = cc.NAMES
M = 1500.0
I = 1500.0 * (5.042 ** 2 + 1.996 ** 2) * 0.5 / 12.0


def sets():
    return {s.name: s for s in cc.all_sets()}


def test_the_list_of_classes_is_the_module_s():
    assert sorted(sets()) == sorted(NAMES)
    assert sum(s.E for s in cc.all_sets()) < 4000


@pytest.mark.parametrize("name", NAMES)
def test_class_reaches_what_it_was_built_for(name):
    s = sets()[name]       # (a class the module left out fails here: it is not skipped)
    got = s.reached()
    bad = [(e, s.want[e], got[e]) for e in range(s.E) if got[e] != s.want[e]]
    assert not bad, bad[:10]
    assert s.need <= set(got), s.need - set(got)


def test_layout_classes_cover_the_lane_layouts():
    for C, per_wg in ((1, 128), (2, 64), (3, 42), (10, 12), (64, 2)):
        s = sets()[f"layout{C}"]
        assert s.E > per_wg and s.E % per_wg != 0                          # more than one workgroup, the last partial
        assert np.array_equal(s.bodies[0, :, :4], s.bodies[1, :, :4])      # identical coordinates, other velocities
        assert not np.array_equal(s.bodies[0, :, 4:], s.bodies[1, :, 4:])
        if C > 1:
            w = np.array(s.want)
            assert ((w[:-1] == "contact") & (w[1:] == "free")).any() and ((w[:-1] == "free") & (w[1:] == "contact")).any()
            assert not np.array_equal(s.solve()["out"][0], s.solve()["out"][1])
    r = sets()["layout1"].solve()
    assert not r["solved"].any() and np.array_equal(r["out"][:, :, :3], sets()["layout1"].bodies[:, :, 4:7])


def test_piles_hold_more_touching_pairs_than_the_cap():
    for C in (4, 10):
        s = sets()[f"pile{C}"]
        r, full = s.solve(), s.solve(cap=C * (C - 1) // 2)
        assert (full["dropped"] == 0).all() and (full["solved"] > C).all()
        assert np.array_equal(r["solved"] + r["dropped"], full["solved"])
        assert np.array_equal(r["pairs"], full["pairs"][:, :C])            # the first C pairs in (i, j) order


@pytest.mark.parametrize("name", NAMES)
def test_cull_changes_nothing(name):
    """centres more than 5.7 m apart on an axis cannot touch (two circumradii and two polygon radii: 5.443 m)"""
    s = sets()[name]
    a, b = s.solve(cull=True), s.solve(cull=False)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _contacts(r):
    """every contact point of a result: (ni, ti, clamp ni) float64 arrays"""
    live = np.arange(r["pairs"].shape[1])[None, :] < r["solved"][:, None]
    out = []
    for q in range(2):
        m = live & (r["pairs"][:, :, 2] > q)
        out.append(np.stack([r["con"][:, :, 6 + 2 * q][m], r["con"][:, :, 7 + 2 * q][m], r["con"][:, :, 10 + q][m]], 1))
    return np.concatenate(out).astype(np.float64).T


def test_impulses_stay_in_the_friction_cone():
    """normalImpulse >= 0, and the tangent impulse inside the cone.  The cone a friction pass clamps against is that of
    the normal impulse as the iteration before left it (b2ContactSolver solves friction first); the last normal pass
    may then lower the normal impulse, down to 0 -- the write-back class is built on exactly that -- so |ti| <= 0.7 ni
    against the FINAL ni holds only where the last pass did not lower it.  Asserted: |ti| <= float32(0.7f * clamp ni)
    exactly, for every contact; and |ti| <= 0.7 ni (1 + 2^-23: the float32 product's rounding) for every contact whose
    final ni is not below the clamp ni."""
    n_lowered = n_all = 0
    for s in cc.all_sets():
        ni, ti, cl = _contacts(s.solve())
        assert (ni >= 0).all() and (cl >= 0).all(), s.name
        bound = (np.float32(0.7) * cl.astype(np.float32)).astype(np.float64)
        assert (np.abs(ti) <= bound).all(), s.name
        kept = ni >= cl
        assert (np.abs(ti[kept]) <= 0.7 * ni[kept] * (1.0 + 2.0 ** -23)).all(), s.name
        n_lowered += int((~kept).sum())
        n_all += len(ni)
    print(f"{n_all} contact points, {n_lowered} with the normal impulse lowered by the last pass")
    assert n_all > 1000


def test_momentum_is_conserved():
    """per env: linear momentum and angular momentum about the origin, to the relative bound of
    test_gpu_extra.test_car_contact_impulses_conserve_momentum (1e-3 of the largest momentum change)"""
    worst = 0.0
    for s in cc.all_sets():
        r = s.solve()
        b = s.bodies.astype(np.float64)
        o = r["out"].astype(np.float64)
        dvx, dvy, dw = o[:, :, 0] - b[:, :, 4], o[:, :, 1] - b[:, :, 5], o[:, :, 2] - b[:, :, 6]
        cx, cy = b[:, :, 0], b[:, :, 1]
        p = M * np.hypot(dvx, dvy).max(1)
        hit = p > 0
        assert hit[r["out"][:, :, 3].max(1) > 0].all(), s.name
        assert not dw[~hit].any(), s.name
        lx, ly = np.abs(M * dvx.sum(1)), np.abs(M * dvy.sum(1))
        L = np.abs((I * dw + M * (cx * dvy - cy * dvx)).sum(1))
        arm = 1.0 + np.hypot(cx, cy).max(1)
        assert (lx[hit] < 1e-3 * p[hit]).all() and (ly[hit] < 1e-3 * p[hit]).all(), s.name
        assert (L[hit] < 1e-3 * p[hit] * arm[hit]).all(), s.name
        if hit.any():
            worst = max(worst, (lx[hit] / p[hit]).max(), (ly[hit] / p[hit]).max(), (L[hit] / (p[hit] * arm[hit])).max())
    print(f"largest relative momentum defect {worst:.3e}")


# ---------------------------------------------------------------- restitution against a float64 run
def _solve64(a, b, n, p):
    """the oracle's algorithm for ONE one-point contact between bodies a, b (float64 rows) with world normal n and point
    p, in float64: set-up, 6 iterations of friction then normal.  The constants are the float32 ones widened, so that
    the float32 run differs by its arithmetic alone.  Returns (vA, wA, vB, wB)."""
    f = np.float32
    m = float(f(1.0) / f(1500.0))
    i = float(f(1.0) / f(1500.0 * (5.042 * 5.042 + 1.996 * 1.996) * 0.5 / 12.0))
    mu, rest = float(f(0.7)), float(f(0.1))
    cr = lambda u, v: u[0] * v[1] - u[1] * v[0]
    crs = lambda s, v: np.array([-s * v[1], s * v[0]])
    vA, wA, vB, wB = a[4:6].copy(), a[6], b[4:6].copy(), b[6]
    rA, rB = p - a[0:2], p - b[0:2]
    t = np.array([n[1], -n[0]])
    nm = 1.0 / (m + m + i * cr(rA, n) ** 2 + i * cr(rB, n) ** 2)
    tm = 1.0 / (m + m + i * cr(rA, t) ** 2 + i * cr(rB, t) ** 2)
    rel = lambda: vB + crs(wB, rB) - vA - crs(wA, rA)
    vrel = float(n @ rel())
    bias = -rest * vrel if vrel < -1.0 else 0.0
    ni = ti = 0.0
    for _ in range(6):
        lam = tm * -(rel() @ t)
        new = max(-mu * ni, min(ti + lam, mu * ni))
        lam, ti = new - ti, new
        P = lam * t
        vA, wA, vB, wB = vA - m * P, wA - i * cr(rA, P), vB + m * P, wB + i * cr(rB, P)
        lam = -nm * (rel() @ n - bias)
        new = max(ni + lam, 0.0)
        lam, ni = new - ni, new
        P = lam * n
        vA, wA, vB, wB = vA - m * P, wA - i * cr(rA, P), vB + m * P, wB + i * cr(rB, P)
    return vA, wA, vB, wB


def _vn(a, va, wa, b, vb, wb, n, p):
    rA, rB = p - a[0:2], p - b[0:2]
    return float(n @ (vb + np.array([-wb * rB[1], wb * rB[0]]) - va - np.array([-wa * rA[1], wa * rA[0]])))


def test_restitution_against_a_float64_run():
    """One-contact, one-point envs of the two-car classes: the normal speed at the contact point after the solve is
    -0.1 x the speed before where the gate is open (before < -1 m/s in the gate's float32 arithmetic), 0 where it is
    closed and the cars approach or rest, and unchanged (no impulse at all) where they separate.  The tolerance is 8 x
    the largest deviation of the float32 oracle's post-solve normal speed from a float64 run of the same algorithm on
    the same manifold (_solve64), 8 being test_gpu_field.py's factor.  Measured: 91 cases, 52 of them open; largest
    deviation 4.9e-07 m/s, so the tolerance is 4.0e-06 m/s; the largest distance from the law is 4.9e-07 m/s."""
    rows = []
    for name in ("gate", "friction", "angular", "cull", "layout2"):
        s = sets()[name]
        r = s.solve()
        for e in range(s.E):
            if r["solved"][e] != 1 or r["pairs"][e, 0, 2] != 1:
                continue
            a, b = s.bodies[e, 0].astype(np.float64), s.bodies[e, 1].astype(np.float64)
            n, p = r["con"][e, 0, 0:2].astype(np.float64), r["con"][e, 0, 2:4].astype(np.float64)
            o = r["out"][e].astype(np.float64)
            pre32 = cc.vrel32(s.bodies[e, 0], s.bodies[e, 1], r["con"][e, 0, 0:2], r["con"][e, 0, 2:4])
            pre = _vn(a, a[4:6], a[6], b, b[4:6], b[6], n, p)
            post = _vn(a, o[0, 0:2], o[0, 2], b, o[1, 0:2], o[1, 2], n, p)
            vA, wA, vB, wB = _solve64(a, b, n, p)
            post64 = _vn(a, vA, wA, b, vB, wB, n, p)
            rows.append((name, e, float(pre32), pre, post, post64, float(r["con"][e, 0, 6])))
    assert len(rows) >= 40
    dev = max(abs(x[4] - x[5]) for x in rows)
    tol = 8.0 * dev
    n_open, worst = 0, 0.0
    for name, e, pre32, pre, post, post64, ni in rows:
        if pre32 < -1.0:
            n_open += 1
            law = -float(np.float32(0.1)) * pre
        elif pre32 <= 0.0:
            law = 0.0
        else:
            assert ni == 0.0 and post == pre, (name, e)
            continue
        worst = max(worst, abs(post - law))
    print(f"{len(rows)} cases, {n_open} open; float32 vs float64 deviation {dev:.3e}, tolerance {tol:.3e}, "
          f"largest distance from the law {worst:.3e}")
    assert dev > 0.0 and n_open >= 10
    for name, e, pre32, pre, post, post64, ni in rows:
        if pre32 <= 0.0:
            law = -float(np.float32(0.1)) * pre if pre32 < -1.0 else 0.0
            assert abs(post - law) <= tol, (name, e, pre, post, law, tol)

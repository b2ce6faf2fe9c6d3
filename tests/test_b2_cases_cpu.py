"""What tests/b2_cases.py's classes exercise, counted on the CPU oracle (or_toi, or_collide) and on the float64
restatement of the TOI cull's bounds.  tests/test_gpu_b2_prims.py compares the device with the oracle on exactly these
cases (b2_cases.N_GPU = 100 003 per class); the floors here keep that comparison from going vacuous when the generator
changes.  Every floor is at most half of the count measured with the committed generator:

b2TimeOfImpact (or_toi), per class: FAILED / OVERLAPPED / TOUCHING / SEPARATED, TOUCHING with 0 < beta < 1, cases the
float64 cull decision skips, share of cases within the float32 budget of a cull threshold ("near")
    approach   1 /  1785 / 48657 / 49560    48332    48699     1.2 %
    scrape     3 / 10358 /  5462 / 84180      103    76981    18.5 %
    far        0 /  9219 /   337 / 90447      247    77787     0.2 %
    overlap0   1 / 63013 /  9119 / 27870     8216    25943     0.9 %
    corner     0 /  9940 /  2329 / 87734     2183    74710     0.4 %
    alpha0     0 /  1618 / 43454 / 54931    42635    53890     2.5 %
    gate       0 / 21152 /  2960 / 75891        0    61149    16.2 %
    captured   4 /     0 /  1492 /  2222      658   (the product's own computed jobs: TOI comparison only)
  FAILED: 9 in all.  No case the float64 decision skips is TOUCHING; the largest float64 bound among the TOUCHING cases
  is 6.31 mm (scrape) against the 9.25 mm threshold.  About 12 000 cases per class carry whole turns on the car's
  angles and about 5 000 a wall angle beyond +-2 pi.  In the gate class 4 092 cases have their second-order bound 0.1 to
  0.6 mm off the threshold at |da| of 0.05 .. 0.1: what a start-pose rotation of too low an order would move across it.

b2CollidePolygons (or_collide), per class: results with 0 / 1 / 2 points, e_faceA / e_faceB among those that reached
the clipping (stage 2), early exits after the type was written (stage 1)
    approach   48521 / 26749 / 24733    17183 / 34299    0
    scrape     72372 / 24529 /  3102     2919 / 24770    0
    far       100003 /     0 /     0        0 /     0    0
    overlap0   29044 / 43263 / 27696    20564 / 50397    0
    corner     97807 /   169 /  2027     1579 /   618    0
    alpha0     52064 / 35594 / 12345     9869 / 38074    0
    ties       24369 /  8609 / 67025    70612 /  8011    3
  The far class's end poses lie 0.05 m or more off the wall, beyond the two polygon radii, so every one of them leaves
  b2CollidePolygons at its first test: that class pins the early exit (only the point count written) and cannot have
  points or a type.
"""
import numpy as np
import pytest

import b2_cases as B

# floors: (OVERLAPPED, TOUCHING, SEPARATED, TOUCHING with 0 < beta < 1, skipped by the float64 decision)
TOI_FLOORS = {
    "approach": (800, 24000, 24000, 24000, 24000),
    "scrape": (5000, 2700, 42000, 50, 38000),
    "far": (4500, 160, 45000, 120, 38000),
    "overlap0": (31000, 4500, 13000, 4000, 12000),
    "corner": (4900, 1100, 43000, 1000, 37000),
    "alpha0": (800, 21000, 27000, 21000, 26000),
    "gate": (10000, 1400, 37000, 0, 30000),
}
# floors: (0 points, 1 point, 2 points, e_faceA, e_faceB)
MANI_FLOORS = {
    "approach": (24000, 13000, 12000, 8500, 17000),
    "scrape": (36000, 12000, 1500, 1400, 12000),
    "far": (100003, 0, 0, 0, 0),
    "overlap0": (14000, 21000, 13000, 10000, 25000),
    "corner": (48000, 80, 1000, 780, 300),
    "ties": (12000, 4300, 33000, 35000, 4000),
    "alpha0": (26000, 17000, 6000, 4900, 19000),
}


@pytest.mark.parametrize("name", B.TOI_CLASSES)
def test_toi_class_reaches_its_outcomes(name):
    k, beta, state, far64, near = B.gpu_toi(name)
    assert k.shape == (B.N_GPU, 12) and B.N_GPU % 64 != 0
    touching = state == B.TOI_TOUCHING
    got = ((state == B.TOI_OVERLAPPED).sum(), touching.sum(), (state == B.TOI_SEPARATED).sum(),
           (touching & (beta > 0) & (beta < 1)).sum(), far64.sum())
    assert all(g >= f for g, f in zip(got, TOI_FLOORS[name])), (name, got)
    # the float64 bounds never skip a call the oracle finds TOUCHING, and leave the threshold's own margin unused
    assert not (far64 & touching).any()
    b1, b2, da = B.case_bounds(k)
    bound = np.maximum(b1, np.where(da <= 0.1, b2, -np.inf))
    assert bound[touching].max() < B.CULL_T - 0.002
    # the cases the device's float32 evaluation may decide either way: at most a fifth of the class
    assert near.mean() <= 0.20, near.mean()
    # whole turns on the car's angles, wall angles beyond +-2 pi, the tracks' far corners
    assert (np.abs(k[:, 5]) > 4 * np.pi).sum() >= 5000
    assert (np.abs(k[:, 9]) > 2 * np.pi).sum() >= 2000
    assert ((np.abs(k[:, 7:9]).max(1) > 1000) & touching).sum() >= TOI_FLOORS[name][1] // 20
    if name == "alpha0":
        assert k[:, 6].min() > 0.05 and k[:, 6].max() < 0.95
    if name == "gate":
        off = np.abs(b2 - B.CULL_T)
        assert ((off > 1e-4) & (off < 6e-4) & (da > 0.05) & (b1 < B.CULL_T - 1e-3)).sum() >= 1000
    if name == "far":   # rotations either side of the second-order bound's |da| <= 0.1 gate
        da32 = np.abs(k[:, 5].astype(np.float64) - k[:, 4])
        assert ((da32 > 0.09) & (da32 <= 0.1)).sum() >= 3000 and ((da32 > 0.1) & (da32 < 0.11)).sum() >= 3000
        assert (da32 > 0.5).sum() >= 2000


def test_toi_failed_and_captured():
    failed = sum(int((B.gpu_toi(name)[2] == B.TOI_FAILED).sum()) for name in B.TOI_CLASSES + ("captured",))
    assert failed >= 4
    k, beta, state, _, _ = B.gpu_toi("captured")
    assert k.shape == (3718, 12)
    touching = state == B.TOI_TOUCHING
    assert touching.sum() >= 700 and (touching & (beta > 0) & (beta < 1)).sum() >= 300
    assert (state == B.TOI_SEPARATED).sum() >= 1100


@pytest.mark.parametrize("name", B.MANI_CLASSES)
def test_manifold_class_reaches_its_results(name):
    k, o = B.gpu_mani(name)
    assert k.shape == (B.N_GPU, 8)
    stage, pc, typ = B.mani_decode_oracle(o)
    got = ((pc == 0).sum(), (pc == 1).sum(), (pc == 2).sum(), ((stage == 2) & (typ == 1)).sum(),
           ((stage == 2) & (typ == 2)).sum())
    assert all(g >= f for g, f in zip(got, MANI_FLOORS[name])), (name, got)
    assert np.all((stage == 2) | (pc == 0))
    if name == "ties":
        assert (stage == 1).sum() >= 1
        # the point test's tie itself: 2-point results beside 0-point ones at a gap of the two radii +- 1 ulp
        assert ((stage == 2) & (pc == 0)).sum() >= 1000


def test_shuffle_is_a_permutation():
    parts = [B.toi_cases(name, 1001) for name in B.TOI_CLASSES]
    allc, perm = B.shuffled(parts)
    assert np.array_equal(np.sort(perm), np.arange(1001 * len(B.TOI_CLASSES)))
    assert np.array_equal(allc, np.concatenate(parts)[perm])

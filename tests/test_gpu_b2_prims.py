"""The Box2D step's primitives on the device against the oracle's own functions, case by case and bit for bit:
b2TimeOfImpact (time_of_impact / gjk_distance as solve_toi calls them, through nascar_debug_toi), the exact TOI cull's
decision (toi_far) and b2CollidePolygons with its packed result (contact_manifold, through nascar_debug_collide).

The cases are tests/b2_cases.py's: 100 003 per class, one lane each, so the last wave is partial; the classes are
also shuffled into one buffer, so that the lanes of a wave diverge, and one launch has a single case.  What the classes
reach (outcome counts, manifold kinds, the share of cases too close to a cull threshold to call) is pinned on the
oracle by tests/test_b2_cases_cpu.py.  Last, the cull is checked where it runs: a counting build re-runs every skipped
call on the crowded POCKET(40) scene.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import b2_cases as B
import crowded

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOI_ALL = B.TOI_CLASSES + ("captured",)
_dev = {}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def device_toi(cases):
    """nascar_debug_toi on cases [n, 12]: (beta float32, state int32, far int32) as numpy arrays"""
    from nascargymnasium_amd import _lib
    n = len(cases)
    k = torch.from_numpy(np.array(cases, np.float32, order="C")).cuda()   # (a copy: the shared cases are read-only)
    beta = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    state = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    far = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().nascar_debug_toi(_ptr(k), n, _ptr(beta), _ptr(state), _ptr(far), _stream()))
    torch.cuda.synchronize()
    return beta.cpu().numpy(), state.cpu().numpy(), far.cpu().numpy()


def device_collide(cases):
    """nascar_debug_collide on cases [n, 8]: raw ManiRes rows [n, 12] float32"""
    from nascargymnasium_amd import _lib
    n = len(cases)
    k = torch.from_numpy(np.array(cases, np.float32, order="C")).cuda()   # (a copy: the shared cases are read-only)
    out = torch.full((n, 12), -7.0, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().nascar_debug_collide(_ptr(k), n, _ptr(out), _stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _toi(name):
    if ("toi", name) not in _dev:
        _dev["toi", name] = device_toi(B.gpu_toi(name)[0])
    return _dev["toi", name]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_toi_equal(what, k, beta, state, obeta, ostate):
    bad = np.flatnonzero((state != ostate) | (_bits(beta) != _bits(obeta)))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(k)} b2TimeOfImpact results differ from the oracle's, first case "
                           f"{bad[0]} = {[float(v).hex() for v in k[bad[0]]]} {k[bad[0]].tolist()}: device state "
                           f"{state[bad[0]]} beta {float(beta[bad[0]]).hex()}, oracle state {ostate[bad[0]]} beta "
                           f"{float(obeta[bad[0]]).hex()}")


@pytest.mark.parametrize("name", TOI_ALL)
def test_toi_matches_oracle(name):
    """state and the bits of beta equal or_toi's for every case (the captured jobs' own qs / qc are not used: both
    sides set the wall's rotation from its angle)"""
    k, obeta, ostate, _, _ = B.gpu_toi(name)
    beta, state, _ = _toi(name)
    _assert_toi_equal(name, k, beta, state, obeta, ostate)


def test_toi_shuffled_and_single_case():
    """all classes shuffled into one buffer (divergent waves), and a launch of one case"""
    parts = [B.gpu_toi(name) for name in TOI_ALL]
    k, perm = B.shuffled([p[0] for p in parts])
    obeta = np.concatenate([p[1] for p in parts])[perm]
    ostate = np.concatenate([p[2] for p in parts])[perm]
    beta, state, far = device_toi(k)
    _assert_toi_equal("shuffled", k, beta, state, obeta, ostate)
    assert not ((far == 1) & (ostate == B.TOI_TOUCHING)).any()
    # the cull's decision does not depend on a case's neighbours in the wave
    far_sorted = np.concatenate([_toi(name)[2] for name in TOI_ALL])[perm]
    assert np.array_equal(far, far_sorted)
    i = int(np.flatnonzero((ostate == B.TOI_TOUCHING) & (obeta > 0) & (obeta < 1))[0])
    b1, s1, f1 = device_toi(k[i:i + 1])
    _assert_toi_equal("single case", k[i:i + 1], b1, s1, obeta[i:i + 1], ostate[i:i + 1])
    assert f1[0] == 0


@pytest.mark.parametrize("name", TOI_ALL)
def test_cull_never_skips_a_touching_call(name):
    """safety: no case with far == 1 whose b2TimeOfImpact is TOUCHING (the one outcome with alpha != 1)"""
    k, _, ostate, _, _ = B.gpu_toi(name)
    _, _, far = _toi(name)
    assert set(np.unique(far).tolist()) <= {0, 1}
    bad = np.flatnonzero((far == 1) & (ostate == B.TOI_TOUCHING))
    assert len(bad) == 0, f"{name}: {len(bad)} TOUCHING calls culled, first case {bad[0]} = {k[bad[0]].tolist()}"


@pytest.mark.parametrize("name", B.TOI_CLASSES)
def test_cull_rounding_margin(name):
    """The float32 evaluation of the two bounds stays within the 3 mm it budgets for itself: away from the thresholds
    (|bound - 9.25 mm| > 3 mm for both bounds, |da| not within 1e-6 of the 0.1 gate) the device decides as the float64
    bounds on the same float32 inputs do.  And it does cull: at least half as often as the float64 decision."""
    k, _, _, far64, near = B.gpu_toi(name)
    _, _, far = _toi(name)
    b1, b2, da = B.case_bounds(k)
    bad = np.flatnonzero(~near & ((far == 1) != far64))
    print(f"{name}: device culls {int(far.sum())}, float64 {int(far64.sum())}, near {near.mean() * 100:.1f} %, "
          f"disagreements among the near cases {int((near & ((far == 1) != far64)).sum())}")
    assert len(bad) == 0, (f"{name}: {len(bad)} decisions differ from the float64 bounds' outside the 3 mm band, first "
                           f"case {bad[0]} = {k[bad[0]].tolist()}: far {far[bad[0]]}, b1 {b1[bad[0]]:.6f} b2 "
                           f"{b2[bad[0]]:.6f} |da| {da[bad[0]]:.6f}")
    assert 2 * int(far.sum()) >= int(far64.sum())


@pytest.mark.parametrize("name", B.TOI_CLASSES)
def test_cull_float32_error(name):
    """A tighter band than the 3 mm budget, from the arithmetic itself.  Each bound is a sum of about 25 float32
    operations on terms below 16 m (|c - wall| and the boxes' extents; the 1500 m coordinates cancel in c - wall,
    whose rounding is half an ulp of the difference), each rounding at most 2^-24 x 16 m = 1e-6 m: below 2.5e-5 m in
    all.  The rotations add 1 ulp of sin / cos on at most 25 m of lever (1.5e-6 m) and toi_far_rot2's 5th-order Taylor
    rotation 1e-7 x 3.5 m.  So the float32 bounds lie within 4e-5 m of the float64 ones, and outside a band of 0.1 mm
    around the threshold the two decide alike.  (A Taylor rotation cut to 2nd order is off by |da|^3 / 6 x 3.5 m, up
    to 0.6 mm at the 0.1 gate: inside the 3 mm budget, outside this band.)"""
    k, _, _, far64, _ = B.gpu_toi(name)
    _, _, far = _toi(name)
    b1, b2, da = B.case_bounds(k)
    gate = da <= 0.1
    tight = (np.abs(b1 - B.CULL_T) <= 1e-4) | (gate & (np.abs(b2 - B.CULL_T) <= 1e-4)) | (np.abs(da - 0.1) <= 1e-6)
    bad = np.flatnonzero(~tight & ((far == 1) != far64))
    assert len(bad) == 0, (f"{name}: {len(bad)} decisions differ from the float64 bounds' outside a 0.1 mm band, first "
                           f"case {bad[0]} = {k[bad[0]].tolist()}: far {far[bad[0]]}, b1 {b1[bad[0]]:.6f} b2 "
                           f"{b2[bad[0]]:.6f} |da| {da[bad[0]]:.6f}")


@pytest.mark.parametrize("name", B.MANI_CLASSES)
def test_manifold_matches_oracle(name):
    """contact_manifold's packed result decoded as contact_apply decodes it, against or_collide on a manifold seeded
    with the same sentinels: stage and point count always; the type from stage 1; local normal, local point and the
    first pointCount points' coordinates and ids at stage 2, bit for bit"""
    k, o = B.gpu_mani(name)
    _assert_mani_equal(name, k, device_collide(k), o)


def _assert_mani_equal(what, k, r, o):
    stage, pc, typ = B.mani_decode_device(r)
    ostage, opc, otyp = B.mani_decode_oracle(o)
    rb, ob = _bits(r), _bits(o)
    bad = (stage != ostage) | (pc != opc) | ((ostage >= 1) & (typ != otyp))
    s2 = ostage == 2
    # device words: 1-2 local normal, 3-4 local point, 5-7 point 0 (x y id), 8-10 point 1; oracle: 2-3, 4-5, 6-7 + 10, 8-9 + 11
    for d, q in ((1, 2), (2, 3), (3, 4), (4, 5)):
        bad |= s2 & (rb[:, d] != ob[:, q])
    for d, q in ((5, 6), (6, 7), (7, 10)):
        bad |= s2 & (opc > 0) & (rb[:, d] != ob[:, q])
    for d, q in ((8, 8), (9, 9), (10, 11)):
        bad |= s2 & (opc > 1) & (rb[:, d] != ob[:, q])
    bad = np.flatnonzero(bad)
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(k)} manifolds differ from the oracle's, first case {bad[0]} = "
                           f"{k[bad[0]].tolist()}: device (stage, points, type) "
                           f"{(stage[bad[0]], pc[bad[0]], typ[bad[0]])} words {rb[bad[0]].tolist()}, oracle "
                           f"{(ostage[bad[0]], opc[bad[0]], otyp[bad[0]])} words {ob[bad[0]].tolist()}")
    # the words past the written ones keep contact_manifold's own initial values
    assert np.all(rb[stage < 2, 1] == 0x7FC0DEAD) and np.all(rb[:, 11] == 0)


def test_manifold_shuffled_and_single_case():
    parts = [B.gpu_mani(name) for name in B.MANI_CLASSES]
    k, perm = B.shuffled([p[0] for p in parts], seed=98)
    o = np.concatenate([p[1] for p in parts])[perm]
    _assert_mani_equal("shuffled", k, device_collide(k), o)
    i = int(np.flatnonzero(B.mani_decode_oracle(o)[1] == 2)[0])
    _assert_mani_equal("single case", k[i:i + 1], device_collide(k[i:i + 1]), o[i:i + 1])


def test_cull_check_in_situ(tmp_path):
    """The cull where it runs: the 12 x 10 POCKET(40) scene (400 steps, full of scraping and TOI events:
    tests/test_crowded_cpu.py) through the counting check build in a fresh child process (tests/cullcheck_child.py).
    Every call the cull skips is run anyway: none may be TOUCHING (counter 11), while calls are both computed
    (counter 12) and skipped (counter 13); the build computes what the oracle does."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    variant = os.path.join(root, "tools", "build", "libnascar_cullcheck.so")
    assert os.path.exists(variant), "run __graft_entry__.build() first"
    sc = crowded.SCENES["12x10"]
    run = crowded.scene_run(tmp_path, sc)
    af, of = str(tmp_path / "actions.npy"), str(tmp_path / "out.npz")
    np.save(af, run.actions)
    child = os.path.join(root, "tests", "cullcheck_child.py")
    r = subprocess.run([sys.executable, child, run.path, str(sc["E"]), str(sc["C"]), str(sc["epb"]), af, of],
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, NASCAR_LIB=variant))
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.load(of)
    counts = out["counts"]
    print(f"in-situ cull check: culled and TOUCHING {int(counts[11])}, computed {int(counts[12])}, culled {int(counts[13])}")
    assert counts[11] == 0, counts[11:14].tolist()
    assert counts[12] > 0 and counts[13] > 0, counts[11:14].tolist()
    assert np.array_equal(_bits(out["obs"]), _bits(run.obs))

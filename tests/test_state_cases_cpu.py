"""tests/state_cases.py on the oracle alone: every case sits on the side of its gate that its builder aimed at, the
oracle's step takes both outcomes of every gate the sets are built for, and the state read-back the device is compared
through (or_get_car_full / or_get_env_full, oracle_lib.pack_arena) is the inverse of the injection."""
import numpy as np
import pytest

import state_cases as S
from oracle_lib import car_state, gpu_arena, oracle_arena, pack_arena
from state_cases import f32i, f64i, i32i


# with reset_on_lap the time limit (60 s) takes every env that the truncation (180 s) would
ONE_SIDED = {("termination_reset_on_lap", "trunc")}


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("name,C", S.SETS)
def test_every_case_sits_where_it_was_aimed(name, C):
    """predicate() == want for ALL cases of the set, and no boolean side is empty"""
    c = S.build(name, C)
    got = S.predicate(c)
    assert set(got) == set(c.want)
    for k, w in c.want.items():
        w, g = np.asarray(w), np.asarray(got[k])
        bad = np.flatnonzero(w != g)
        assert len(bad) == 0, f"{name} C={C}: {k} differs for {len(bad)} cases, first {bad[0]}: want {w[bad[0]]} got {g[bad[0]]}"
        if w.dtype == bool and (name, k) not in ONE_SIDED:
            assert w.any() and not w.all(), f"{name}: {k} has one side only"


def test_speed_gates_three_sides_per_gate():
    c = S.build("speed_gates", 1)
    for g, t in enumerate(S.SPEED_GATES):
        m = c.want["gate"] == g
        above, below = c.want["above"][m], c.want["below"][m]
        assert above.any() and below.any(), t
        if float(np.float32(t)) == t:     # a threshold float32 holds: the speed sits exactly on it too
            assert (~above & ~below).any(), t
        for a in range(3):                # throttle, brake, coast on every side
            ma = m & ((np.arange(c.N) // 108) % 3 == a)
            assert c.want["above"][ma].any() and c.want["below"][ma].any()


def _after(name, C):
    c = S.build(name, C)
    A, obs, rew, cf, ef = S.oracle_step(name, C)
    return c, gpu_arena(c.blob, c.E, c.C), A, rew.reshape(-1), cf.reshape(-1), ef


def test_rpm_outcomes():
    c, A0, A, *_ = _after("rpm", 1)
    new, unit, lo, hi = S.rpm_next(A0["f64"][f64i["rpm"]], np.clip(c.actions.reshape(-1, 2)[:, 0].astype(np.float64), 0, 1))
    assert _same(A["f64"][f64i["rpm"]], new)
    assert (new == 600.0).any() and (new == 9500.0).any()
    assert ((new > 600.0) & (new < 600.0 + 1e-9)).any() and ((new < 9500.0) & (new > 9500.0 - 1e-9)).any()
    assert set(np.unique(c.want["tiny_den"])) == {-1.0, 0.0, 1.0}


def test_ring_outcomes():
    c, A0, A, *_ = _after("ring", 1)
    ln, hd = c.want["acc_len"], c.want["acc_head"]
    assert len(set(zip(ln.tolist(), hd.tolist()))) == 110
    assert np.array_equal(A["i32"][i32i["acc_len"]], np.minimum(ln + 1, 10))
    assert np.array_equal(A["i32"][i32i["acc_head"]], np.where(ln == 10, (hd + 1) % 10, hd))
    slot = np.where(ln == 10, hd, (hd + ln) % 10)
    changed = (A["acc"].view(np.uint64) != A0["acc"].view(np.uint64)).reshape(10, 2, c.N).any(1)
    assert np.array_equal(changed, np.arange(10)[:, None] == slot[None, :])     # only the appended slot is written


def test_weight_transfer_saturates():
    c, A0, A, *_ = _after("weight_transfer", 1)
    n = np.arange(c.N)
    slot = A0["i32"][i32i["acc_head"]]      # a full ring: the new sample replaces the oldest
    lon, lat = A["acc"][2 * slot, n], A["acc"][2 * slot + 1, n]
    assert np.array_equal(lon, 12.0 * np.sign(c.want["lon"])) and np.array_equal(lat, 12.0 * np.sign(c.want["lat"]))
    loads = np.stack([A["f64"][f64i["load%d" % i]] for i in range(4)])
    assert (loads >= 50.0).all()
    front = loads[:2].sum(0)
    assert (front[c.want["lon"] == 40.0] < 450.0).all() and (front[c.want["lon"] == -12.0] > 7000.0).all()


def test_tyres_outcomes():
    c, A0, A, *_ = _after("tyres", 1)
    T = np.stack([A["f64"][f64i["temp%d" % i]] for i in range(4)])
    W = np.stack([A["f64"][f64i["wear%d" % i]] for i in range(4)])
    assert (T >= 25.0).all() and (T <= 120.0).all() and (T == 25.0).any() and (T == 120.0).any()
    assert (W <= 100.0).all() and (W == 100.0).any() and ((W > 99.0) & (W < 100.0)).any()
    assert set(np.unique(c.want["band0"])) == {-1, 0, 1} and set(np.unique(c.want["latg"])) == {-1, 0, 1}


@pytest.mark.parametrize("C", [1, 10])
def test_stuck_outcomes(C):
    c, A0, A, rew, cf, ef = _after("stuck", C)
    w = c.want
    dis = A["i32"][i32i["disabled"]] != 0
    had = A0["i32"][i32i["has_stuck_start"]] != 0
    rest = w["rest"]
    expect = w["dur10"] & (w["moved_lt1"] | w["dur15"] | ~had)      # no stuck start: it is taken now, moved = 0
    assert np.array_equal(dis[rest], expect[rest])
    for a, b in ((w["dur10"], w["moved_lt1"]), (w["dur10"], ~w["moved_lt1"] & w["dur15"]), (w["dur10"], ~w["moved_lt1"] & ~w["dur15"])):
        assert (rest & had & a & b).any()
    assert dis[rest].any() and (~dis[rest]).any()
    sd = A["f64"][f64i["stuck_dur"]]
    mv = ~rest
    assert (sd[mv] == 0.0).any() and (sd[mv] > 0.0).any()          # either side of 0.5 m/s


@pytest.mark.parametrize("C", [1, 10])
def test_backward_outcomes(C):
    c, A0, A, rew, cf, ef = _after("backward", C)
    w = c.want
    assert _same(A["f64"][f64i["prog_hist"]], c.meta["prog"])          # the probe saw this step's progress
    dis = A["i32"][i32i["disabled"]] != 0
    assert np.array_equal(dis, w["gt200"])
    back = A["f64"][f64i["back"]]
    assert np.array_equal(back > 25.0, w["gt25"]) and np.array_equal(back > 200.0, w["gt200"])
    assert (back == 25.0).any() and (back == 200.0).any()
    for k in range(12):
        assert (w["kind"] == k).sum() == c.N // 12
    wr = w["wrap"]
    # the wrap that turns -L / 2 into +L / 2 needs a car in the lap's first half, the other one a car in its second
    assert (wr & ~w["backwards"]).any() and (wr & w["backwards"]).any()
    k9, k11 = w["kind"] == 9, w["kind"] == 11
    second = c.meta["prog"] > c.meta["L"] / 2         # a hair short of / past +-L / 2, and exactly on it
    assert np.array_equal(wr[k9], second[k9]) and np.array_equal(wr[k11], ~second[k11]) and not wr[w["kind"] == 10].any()


@pytest.mark.parametrize("name,C", [("impact", 1), ("impact_crowded", 10)])
def test_impact_outcomes(name, C):
    c, A0, A, rew, cf, ef = _after(name, C)
    w, live = c.want, c.meta["live"]
    dis = A["i32"][i32i["disabled"]] != 0
    expect = w["gt50000"] | w["cum_gt"]
    calm = ~live & (A["i32"][i32i["nact"]] == 0)          # (on the crowded scene a free car may touch a wall this step)
    assert np.array_equal(dis[calm], expect[calm]) and (dis[~live] >= expect[~live]).all() and calm.sum() > c.N // 2
    assert dis[~live].any() and (~dis[~live]).any()
    ci = A["f64"][f64i["cum_impact"]]
    assert (ci == 250000.0).any()
    if name == "impact_crowded":
        grew = ci[live] > A0["f64"][f64i["cum_impact"]][live]
        assert grew.sum() > 50 and dis[live].any() and (~dis[live]).any()
        assert (A["i32"][i32i["nact"]][live] > 0).sum() > 100


@pytest.mark.parametrize("name", ["lap_gate", "lap_gate_reset_on_lap"])
@pytest.mark.parametrize("C", [1, 10])
def test_lap_gate_outcomes(name, C):
    c, A0, A, rew, cf, ef = _after(name, C)
    w = c.want
    laps = A["i32"][i32i["lt_laps"]] - A0["i32"][i32i["lt_laps"]]
    assert np.array_equal(laps == 1, w["lap"]) and ((laps == 0) | (laps == 1)).all()
    assert (A["i32"][i32i["lt_has_pos"]] == 3).all()                    # every car drove onto the line
    assert (A["i32"][i32i["lt_crossed"]][w["first"]] == 1).all()
    held = ~w["lap"] & ~w["first"] & (A0["i32"][i32i["lt_timing"]] != 0)
    assert (held & w["cur_lt10"]).any() and (held & ~w["cur_lt10"] & w["short"]).any()
    assert (w["lap"] & (A["f64"][f64i["lt_last"]] == 10.0)).any()       # lt_cur exactly 10.0 is a lap
    term = ef[:, 0] != 0
    if c.reset_on_lap:
        assert term.any() and not term.all()
        if C == 1:
            assert np.array_equal(term, w["lap"])
    else:
        assert not term.any()


@pytest.mark.parametrize("name", ["termination", "termination_reset_on_lap"])
def test_termination_outcomes(name):
    c, A0, A, rew, cf, ef = _after(name, 3)
    w = c.want
    assert np.array_equal(A["i32"][i32i["disabled"]], A0["i32"][i32i["disabled"]])    # the step disables nobody
    assert np.array_equal(ef[:, 0] != 0, w["term"]) and np.array_equal(ef[:, 1] != 0, w["trunc"])
    fired = w["reason"] != 0
    assert np.array_equal(ef[fired, 2], w["reason"][fired])
    assert set(np.unique(w["reason"])) == ({0, 1, 2, 3} if c.reset_on_lap else {0, 1, 2, 4})
    pend = A0["ei32"][1] != 0
    assert (pend & (w["reason"] == 0) & w["term"]).any() and (pend & w["trunc"]).any() == (not c.reset_on_lap)
    assert (A["ei32"][1] == 0).all()
    # priority: envs over the time limit whose cars are all disabled / all under -250 keep reason 1 / 2
    late = (A0["time"] + S.DT) > 60.0
    assert (late & (w["reason"] == 1)).any() and (late & (w["reason"] == 2)).any()


@pytest.mark.parametrize("name,C", [("reset_dirty", 10), ("reset_dirty_crowded", 1), ("reset_dirty_crowded", 10)])
def test_reset_dirty_outcomes(name, C):
    c, A0, A, *_ = _after(name, C)
    m = np.repeat(c.mask != 0, C)
    for k in ("f32", "f64", "i32", "acc"):
        assert _same(A[k][:, ~m], A0[k][:, ~m]), k
    assert (A["f64"][f64i["rpm"]][m] == 1000.0).all() and (A["i32"][i32i["first_step"]][m] == 1).all()
    assert _same(A["f64"][f64i["bank"]], A0["f64"][f64i["bank"]])       # Car.reset keeps current_banking_angle
    assert (A["i32"][i32i["nact"]][m] == 0).all()
    if name == "reset_dirty_crowded":
        assert (A0["i32"][i32i["nact"]][m] > 0).sum() > 50 and (A0["i32"][i32i["disabled"]][m] != 0).any()
    else:
        assert (A0["f64"][f64i["bank"]][m] != 0.0).any()


def test_bank_and_input_sides():
    c = S.build("bank", 1)
    w = c.want
    assert (w["banked"] & w["ge1"] & w["gt5"]).any() and (w["banked"] & w["ge1"] & ~w["gt5"]).any()
    assert (w["banked"] & ~w["ge1"]).any()
    c = S.build("input_gates", 1)
    _, _, A, rew, cf, ef = _after("input_gates", 1)
    assert (rew[c.want["disabled"]] == 0.0).all() and (rew[~c.want["disabled"]] != 0.0).all()


# ---------------------------------------------------------------- the track lookups on the generated tracks
LOOKUP_SETS = [(n, C) for n, C in S.SETS
               if S.CLASSES[n][0] in (S._chord_ties, S._startline_band, S._no_startline, S._on_track_query)]


def _ends_where_probed(c, A):
    """the builder's probe saw the position this step ends at"""
    assert _same(A["f32"][f32i["xpx"]].astype(np.float64), c.meta["px"])
    assert _same(A["f32"][f32i["xpy"]].astype(np.float64), c.meta["py"])


@pytest.mark.parametrize("name,C", [s for s in LOOKUP_SETS if s[0].startswith("chord_ties")])
def test_chord_ties_reach(name, C):
    """What the chord_ties sets reach, counted on the oracle's positions after the step (of 2400 cars each; seg64 /
    seg17 / ring4 / degenerate): nearest chord at index >= 16: 1722 / 155 / - / -; chord 16 nearest on seg17: 155;
    a second chord within 2 screen_eps: 1598 / 1573 / 1909 / 1582; the two smallest distances equal or 1 ulp apart:
    725 / 867 / 1017 / 877; runner-up with another banking: 2400 / 2317 / 2400 / 1937; projection clamped at 0: 9 /
    25 / 218 / 79, at 1: 722 / 858 / 920 / 818; the two searches disagree on the chord: 0 / 5 / 35 / 80.  The
    oracle's step leaves the banking of the chord `want` names, and the progress along it."""
    c, A0, A, *_ = _after(name, C)
    _ends_where_probed(c, A)
    seg = S.track_tables(c.track)[0]
    st = S.lookup_stats(seg, c.meta["px"], c.meta["py"])
    assert np.array_equal(st["pbi"], c.want["pbi"]) and np.array_equal(st["bbi"], c.want["bbi"])
    print(name, C, {k: (int((v >= 16).sum()) if k in ("pbi", "bbi") else [int((v == s).sum()) for s in (-1, 1)] if k == "clamp"
                        else int(v.sum())) for k, v in st.items()}, "chord 16:", int((st["pbi"] == 16).sum()),
          "searches disagree:", int((st["pbi"] != st["bbi"]).sum()))
    if c.track == "seg64":
        assert (st["pbi"] >= 16).sum() >= c.N // 4 and (st["bbi"] >= 16).sum() >= c.N // 4
        assert len(np.unique(st["pbi"])) == 64
    if c.track == "seg17":
        assert (st["pbi"] == 16).sum() >= 50 and (st["bbi"] == 16).sum() >= 50
    assert st["close"].sum() >= 200 and st["tie"].sum() >= 100 and st["bank_differs"].sum() >= 100
    assert (st["clamp"] == -1).any() and (st["clamp"] == 1).any()
    far = np.abs(c.meta["px"]) + np.abs(c.meta["py"])
    assert (far > 5e4).sum() >= 20 and ((far > 1e3) & (far < 1e4)).sum() >= 20
    # the oracle's own searches found these chords
    assert _same(A["f64"][f64i["bank"]], seg[c.want["bbi"], 12])
    k = c.want["pbi"]
    sx, sy, dx, dy = seg[k, 2], seg[k, 3], seg[k, 4] - seg[k, 2], seg[k, 5] - seg[k, 3]
    ll = dx * dx + dy * dy
    with np.errstate(divide="ignore", invalid="ignore"):
        tt = S._clamp01(((c.meta["px"] - sx) * dx + (c.meta["py"] - sy) * dy) / ll)
    qx, qy = np.where(ll < 1e-6, sx, sx + tt * dx), np.where(ll < 1e-6, sy, sy + tt * dy)
    prefix = np.concatenate([[0.0], np.cumsum(np.sqrt(S.P2(seg[:, 4] - seg[:, 2]) + S.P2(seg[:, 5] - seg[:, 3])))])[k]
    assert _same(A["f64"][f64i["prog_hist"]], prefix + np.sqrt(S.P2(qx - sx) + S.P2(qy - sy)))


@pytest.mark.parametrize("name,C", [s for s in LOOKUP_SETS if s[0].startswith("startline_band")])
def test_startline_band_outcomes(name, C):
    """every offset of band_offsets() (0, +-1e-6, +-screen_eps / 2, +-screen_eps, +-2 screen_eps, +-1 m from the
    capsule's edge) is met to BAND_TOL on both sides and around both ends (measured: to 5.3e-8 on seg64, whose start
    line is rotated and 350 m out, and to 4.6e-8 on degenerate); (now, before) takes all four values; of 2400 cars,
    206 / 233 (seg64 / degenerate) complete a lap and 216 / 244 cross for the first time; the cars end where they
    were put"""
    c, A0, A, *_ = _after(name, C)
    _ends_where_probed(c, A)
    assert _same(A["f32"][f32i["xpx"]], A0["f32"][f32i["xpx"]]) and _same(A["f32"][f32i["xpy"]], A0["f32"][f32i["xpy"]])
    m, w = c.meta, c.want
    err = np.abs(m["edge"] - m["off"])
    worst = 0.0
    for p in range(S.BAND_PLACES):
        for j in range(len(S.band_offsets(1.0))):
            sel = (m["place"] == p) & (m["joff"] == j)
            assert sel.sum() >= 5 and err[sel].min() <= S.BAND_TOL, (p, j, err[sel].min())
            worst = max(worst, err[sel].min())
            nominal = S.band_offsets(1.0)[j]
            if nominal != 0.0:          # and on the side of the edge it was aimed at
                assert (np.sign(m["edge"][sel][err[sel] <= S.BAND_TOL]) == np.sign(nominal)).all()
    if c.track == "degenerate":       # its start line runs along +x at the origin: float32 holds the edge itself
        assert (m["edge"] == 0.0).any()
    for now in (False, True):
        for before in (False, True):
            assert ((w["now"] == now) & (w["before"] == before)).sum() >= 100
    laps = A["i32"][i32i["lt_laps"]] - A0["i32"][i32i["lt_laps"]]
    assert np.array_equal(laps == 1, w["lap"]) and ((laps == 0) | (laps == 1)).all() and w["lap"].any()
    first = (A["i32"][i32i["lt_crossed"]] == 1) & (A0["i32"][i32i["lt_crossed"]] == 0)
    assert np.array_equal(first, w["first"]) and w["first"].any()
    assert np.array_equal(A["i32"][i32i["lt_has_pos"]], np.where(w["now"], 3, 1))
    print(name, C, "worst best offset error", worst, "laps", int(w["lap"].sum()), "first crossings", int(w["first"].sum()))


def test_no_startline_outcomes():
    """without a STARTLINE no lap field changes but the position, and lt_dist takes the move of the cars that had one"""
    (name, C), = [s for s in LOOKUP_SETS if s[0] == "no_startline"]
    c, A0, A, *_ = _after(name, C)
    for f in ("lt_timing", "lt_has_last", "lt_has_best", "lt_crossed", "lt_laps"):
        assert np.array_equal(A["i32"][i32i[f]], A0["i32"][i32i[f]]), f
    for f in ("lt_start", "lt_last", "lt_best"):
        assert _same(A["f64"][f64i[f]], A0["f64"][f64i[f]]), f
    assert (A["i32"][i32i["lt_has_pos"]] == 1).all()
    dx = A["f32"][f32i["xpx"]].astype(np.float64) - A0["f64"][f64i["lt_px"]]
    dy = A["f32"][f32i["xpy"]].astype(np.float64) - A0["f64"][f64i["lt_py"]]
    d = np.sqrt(dx * dx + dy * dy)
    assert (d[c.want["has"]] > 0.3).any() and (d < 50.0).all()
    assert _same(A["f64"][f64i["lt_dist"]], np.where(c.want["has"], A0["f64"][f64i["lt_dist"]] + d, A0["f64"][f64i["lt_dist"]]))
    tm = c.want["timing"]
    assert (A["f64"][f64i["lt_cur"]][tm] > 29.9).all() and _same(A["f64"][f64i["lt_cur"]][~tm], A0["f64"][f64i["lt_cur"]][~tm])


@pytest.mark.parametrize("name,C", [s for s in LOOKUP_SETS if s[0].startswith("on_track_query")])
def test_on_track_query_outcomes(name, C):
    """on a wall / off every wall, of 2400 cars: 1460 / 940 on seg64, 1568 / 832 on degenerate; decided by the vertex
    distance (inside no box, within 0.5 m of a corner): 321 / 459.  The float64 geometry of wall_query agrees with the
    oracle's float32 query for every car it decides by more than 0.1 mm (114 / 93 cars lie closer)."""
    c, A0, A, *_ = _after(name, C)
    _ends_where_probed(c, A)
    w = c.want
    on = S.oracle_info(name, C)[:, 0] == 0.0
    sure = c.meta["margin"] > 1e-4
    assert sure.sum() > 0.9 * c.N and np.array_equal(on[sure], w["on_wall"][sure])
    assert on.sum() >= c.N // 5 and (~on).sum() >= c.N // 5
    assert (w["vertex"] & sure & on).sum() >= 50
    print(name, C, "on a wall", int(on.sum()), "by the vertex distance", int((w["vertex"] & sure).sum()), "unsure", int((~sure).sum()))


# ---------------------------------------------------------------- the read-back
@pytest.mark.parametrize("name,C", [("impact_crowded", 10), ("lap_gate", 1), ("termination_reset_on_lap", 3)])
def test_set_get_car_full_is_identity(name, C):
    """inject_gpu_state (or_set_car_full / or_set_env_full) then oracle_arena (or_get_car_full / or_get_env_full)
    returns every section of the blob bit for bit; lt_has_pos comes back in the device's encoding (bit 1: the recorded
    position lies on the start line), which the sets' states carry consistently"""
    c = S.build(name, C)
    A0 = gpu_arena(c.blob, c.E, c.C)
    orc = c.oracle()
    A = oracle_arena(orc)
    for k in A:
        assert _same(A[k], A0[k]), k
    # and the 71 fields or_car_state shares with it agree (lt_has_pos there is the oracle's own 0 / 1)
    hp = 18 + 36 + i32i["lt_has_pos"]
    for n in range(0, c.N, 37):
        full = np.concatenate([A["f32"][:, n].astype(np.float64), A["f64"][:, n], A["i32"][:, n].astype(np.float64)])
        st = car_state(orc, n)
        full[hp] = float(int(full[hp]) & 1)
        assert _same(full, st), n
    orc.close()


def test_lt_has_pos_reports_the_start_line_bit():
    c = S.build("lap_gate", 1)
    A = S.oracle_step("lap_gate", 1)[0]
    assert (gpu_arena(c.blob, c.E, 1)["i32"][i32i["lt_has_pos"]] == 1).all() and (A["i32"][i32i["lt_has_pos"]] == 3).all()


def test_pack_arena_inverts_gpu_arena():
    """pack_arena(gpu_arena(blob)) == blob for a blob with every byte set (the padding between sections is zero in
    both); gpu_arena returns views, so writing a section of a writable blob's arena writes the blob"""
    E, C = 7, 3
    rng = np.random.default_rng(1)
    blob = np.zeros(len(pack_arena({}, E, C)), np.uint8)
    V = gpu_arena(blob, E, C)
    for k in V:
        V[k].view(np.uint8)[...] = rng.integers(0, 256, V[k].view(np.uint8).shape, dtype=np.uint8)
    assert blob.any()
    again = pack_arena(gpu_arena(blob, E, C), E, C)
    assert np.array_equal(again, blob)
    V["time"][3] = 12.5
    assert gpu_arena(blob, E, C)["time"][3] == 12.5 and not np.array_equal(again, blob)
    part = pack_arena({k: V[k] for k in V if k != "ctl"}, E, C)
    assert (gpu_arena(part, E, C)["ctl"] == 0).all()

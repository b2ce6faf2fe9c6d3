"""The track lookups, the sensors and the segment staging on generated tracks of up to 64 segments (tests/track_gen.py).

The bundled tracks have 7-9 segments, so the chord screen's loops over chords 16 .. 63 (screen_candidates), mask bits
at or above 16, a start line that is rotated and away from the origin, a track without a start line, zero-length
chords and workgroups whose tracks differ widely in nseg ran nowhere.  Here: the 64 / 65 segment limit; the sensors
against the oracle's brute-force cast; closed loops against the oracle (noisy driver, staggered masked resets, so that
car_reset's unscreened track_progress runs on every track) through the fused model + logic kernel and the two-launch
path, with the sharded and the fused rollout equal to the per-step path; a mixed batch with nseg 1, 4, 17 and 64 in
neighbouring workgroups, fixed and in random-track mode (rt_switch_kernel's reset on a many-segment track), each at 1
and at 12 envs per workgroup; the info columns of the on_track_query case sets; the device's island-capacity flag.  The single-step case sets on these tracks (chord ties, the start line's
band, no start line, the wall query) run in tests/test_gpu_state_parity.py::test_one_step; what they reach is pinned
on the oracle in tests/test_state_cases_cpu.py.

Scratch-build check.  With one change in csrc/nascar_kernels.hip each, the new tests (test_one_step's chord_ties and
startline_band sets, test_closed_loop_vs_oracle, test_mixed_batch_vs_oracle, test_rollouts_equal_the_per_step_path;
for the last change also test_mixed_batch_random_tracks and test_one_step_two_launch)
ran as follows on an MI355X, and passed again without the change:
  * screen_candidates, the first `k >= SCREEN_R` loop (the minimum over chords 16 ..) removed: NO test fails, and none
    can.  The minimum is then taken over chords 0 .. 15 alone, so it can only be larger; the cut grows with it and the
    mask becomes a superset of the right one, which the exact float64 search over it turns into the same chord.  The
    loop buys a smaller mask, not a result;
  * the second `k >= SCREEN_R` loop (the mask bits 16 ..) removed: test_one_step[chord_ties_seg64-*] (all 4),
    [chord_ties_seg17-*] (2) and [startline_band_seg64-*] (4) fail -- `bank`, `prog_hist` and what follows from them;
  * `2.0f * screen_eps(x, y)` -> `0.0f`: test_one_step[chord_ties_*] on all four tracks (10 cases) fail;
  * `d2 < pbest` -> `<=` in bank_and_progress_screened: test_one_step[chord_ties_seg17-*], [chord_ties_ring4-*] and
    [chord_ties_degenerate-*] (6 cases) fail.  Not seg64's: at a joint's wedge both chords give the same progress
    (prefix[k] + |chord k| == prefix[k + 1]), and seg64's only joint where they would not, the lap's wrap, closes to
    1e-13 m, not bit for bit, so there is no exact tie there;
  * `h - e` -> `h + e` in on_startline_screened: all 6 test_one_step[startline_band_*] fail;
  * `tid < T.nseg` -> `tid < min(T.nseg, 16)` in stage_track_lds: test_closed_loop_vs_oracle[seg64-12-10],
    [seg64-16-1], [seg17-16-3], test_mixed_batch_vs_oracle[1] and test_mixed_batch_random_tracks[1] fail, each in its
    two-launch engine at one env per workgroup (the fused kernel stages through g_step_segs), and
    test_one_step_two_launch fails on chord_ties_seg64, chord_ties_seg17 and startline_band_seg64.  At 12 envs per
    workgroup the closed loops' two-launch engines passed: the LDS rows left unwritten still held what an earlier
    kernel had put there.  The rollouts pass under it: all three paths stage alike.
"""
import numpy as np
import pytest

import state_cases as S
import track_gen
from closed_loop import closed_loop_vs_oracle, make_envs

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    d = tmp_path_factory.mktemp("generated")
    paths = {n: track_gen.write(d, n) for n in track_gen.FAMILY}
    paths["seg64flat"] = track_gen.write(d, "seg64flat", track_gen.flat("seg64"))
    paths["seg65"] = track_gen.write(d, "seg65", track_gen.too_many_segments())
    return paths


# ---------------------------------------------------------------- the segment-count limit
def test_segment_count_limit(family):
    """64 segments load; 65 raise from BatchedCarEnv, and a fresh engine on the same device works afterwards; the
    one-segment track loads and steps, equal to the oracle"""
    from nascargymnasium_amd.batched import BatchedCarEnv
    from oracle_lib import OracleEnv
    env = BatchedCarEnv(2, 3, family["seg64"], device="cuda:0", beam_cell=4.0)
    env.close()
    with pytest.raises(RuntimeError, match="segment count 65 out of range"):
        BatchedCarEnv(2, 3, family["seg65"], device="cuda:0", beam_cell=4.0)
    env = BatchedCarEnv(4, 3, family["seg1"], device="cuda:0", beam_cell=4.0)
    orc = OracleEnv(family["seg1"], 4, 3)
    assert np.array_equal(env.reset().cpu().numpy(), orc.reset()[0])
    rng = np.random.default_rng(2)
    for k in range(60):
        a = rng.uniform(-1, 1, (4, 3, 2)).astype(np.float32)
        a[..., 0] = np.abs(a[..., 0])
        go, gr, _, _ = env.step(torch.from_numpy(a).cuda())
        oo, orw, _, _ = orc.step(a)
        assert np.array_equal(go.cpu().numpy(), oo) and np.array_equal(gr.cpu().numpy(), orw), k
    assert float(np.abs(oo[..., 0]).max()) > 0
    orc.close()
    env.close()


# ---------------------------------------------------------------- sensors
@pytest.mark.parametrize("name,seed", [("seg64", 64), ("degenerate", 16), ("ring4", 4)])
def test_sensors_on_generated_tracks(family, name, seed):
    """beam lists at 4 and 16 lanes, wall groups and the oracle's brute-force cast, bit for bit, at the default 1 m cells"""
    from test_gpu_sensors import _check_sensors
    _check_sensors(family[name], 256, 4, seed)


# ---------------------------------------------------------------- closed loops
def _closed_loop(path, E, C, layouts, fused, steps=300, seed=17):
    from oracle_lib import OracleGroups
    envs = make_envs(E, C, path, layouts, fused=fused, beam_cell=4.0)
    orc = OracleGroups([path] * E if isinstance(path, str) else path, C, shards=4 if isinstance(path, str) else 1)
    stagger = {20 + (260 // E) * e: e for e in range(E)}          # every env is reset once, at its own step
    try:
        return closed_loop_vs_oracle(envs, orc, steps, seed=seed, stagger=stagger)
    finally:
        for env in envs:
            env.close()
        orc.close()


@pytest.mark.parametrize("name,E,C,layouts,fused", [
    ("seg64", 12, 10, [12, 1, 12], (2,)), ("seg64", 16, 1, [16, 1], (0,)), ("seg64flat", 12, 10, [12, 12], (1,)),
    ("seg17", 16, 3, [16, 1, 16], (2,)), ("nostart", 8, 3, [8, 8], (1,)), ("degenerate", 8, 3, [8, 8, 1], (1,))])
def test_closed_loop_vs_oracle(family, name, E, C, layouts, fused):
    """300 noisy-driver steps, every env reset once through the mask (car_reset -> track_progress), == the oracle every
    step, through the fused model_logic_kernel (`fused`) and through model_kernel + logic_kernel.  seg64flat is seg64
    without banking: the progress-only lookup (track_progress_screened) over 64 chords."""
    t = _closed_loop(family[name], E, C, layouts, fused)
    assert t["max_age"] > 0


@pytest.mark.parametrize("name,E,C", [("seg64", 12, 10), ("degenerate", 8, 3), ("nostart", 8, 3)])
def test_rollouts_equal_the_per_step_path(family, name, E, C):
    """the sharded rollout and the fused rollout_kernel end on the per-step path's observations and state: on seg64
    (64 chords staged), on degenerate (zero-length chords) and on nostart (startline = -1)"""
    from nascargymnasium_amd.batched import BatchedCarEnv
    K = 300
    outs = []
    for streams in (4, 0, None):
        b = BatchedCarEnv(E, C, family[name], device="cuda:0", beam_cell=4.0)
        b.reset()
        if streams is None:
            for k in range(K):
                b.step_driven(3, seed=5, step=k, auto_reset=True)
        else:
            b.set_rollout_streams(streams)
            b.rollout(3, seed=5, step0=0, steps=K)
        outs.append((b.obs.cpu().numpy().copy(), b.get_state().cpu().numpy().copy()))
        b.close()
    for o, s in outs[:2]:
        assert np.array_equal(o.view(np.uint32), outs[2][0].view(np.uint32)) and np.array_equal(s, outs[2][1])
    assert float(np.abs(outs[2][0][..., 0]).max()) > 0.005      # the cars left the start (50 m)


# ---------------------------------------------------------------- mixed batches
@pytest.mark.parametrize("epb", [1, 12])
def test_mixed_batch_vs_oracle(family, epb):
    """48 envs x 10 cars, env e on track e mod 6 of the family (nseg 1, 4, 17, 64, 4, 16 in neighbouring workgroups),
    300 noisy-driver steps with masked resets and in-launch auto-reset: each env == the oracle on its own track"""
    E, C = 48, 10
    files = [family[track_gen.FAMILY[e % 6]] for e in range(E)]
    t = _closed_loop(files, E, C, [epb, epb], (1,))
    assert t["max_age"] > 0


@pytest.mark.parametrize("epb", [1, 12])
def test_mixed_batch_random_tracks(family, epb):
    """The mixed batch in random-track mode: 48 envs x 10 cars over the family, at 1 env per workgroup through
    model_kernel + logic_kernel (stage_track_lds) and at 12 through the fused kernel, 300 noisy-driver steps with
    in-launch auto-reset; every env is also reset through the mask three times (a reset draws the env's next track), so
    rt_switch_kernel resets cars on the 64-segment track and regroups workgroups of very different nseg.  Every env
    == a fresh oracle env on each track it is sent to, every step; the tracks are the host replay of the draws
    (test_gpu_random_tracks._replay_tracks), and under these seeds envs go from the 64-segment track to seg1 and from
    seg1 to the 64-segment track in mid-run (env 1 does both: draws 1 and 2)."""
    from concurrent.futures import ThreadPoolExecutor
    from nascargymnasium_amd.batched import BatchedCarEnv
    from drivers import NoisyRuleDriver
    from oracle_lib import OracleEnv
    from test_gpu_random_tracks import _replay_tracks
    E, C, K = 48, 10, 300
    tracks = [family[n] for n in track_gen.FAMILY]
    eng = BatchedCarEnv(E, C, [tracks[e % 6] for e in range(E)], device="cuda:0", envs_per_block=epb, beam_cell=4.0)
    assert eng.envs_per_block == epb
    eng.set_fused_logic(epb == 12)
    seeds = np.arange(E, dtype=np.uint64) * 104729 + 3
    eng.set_random_tracks(tracks, seeds)
    ids = eng.random_track_ids
    t_start = np.array([eng._track_id[tracks[e % 6]] for e in range(E)], np.int32)
    i64, i1 = eng._track_id[family["seg64"]], eng._track_id[family["seg1"]]
    pool = ThreadPoolExecutor(8)          # the oracle envs step in host threads (the C step releases the GIL)
    obs = eng.reset().cpu().numpy().copy()              # every env draws (draw 0) and gets fresh worlds there
    ndraw = np.ones(E, np.int64)
    replay = lambda: _replay_tracks(seeds, np.zeros(E, np.int64), t_start, ndraw, ids)
    hist = [eng.env_track_ids()[0].copy()]
    assert np.array_equal(hist[0], replay())
    files = eng.env_track_files()
    orcs = [OracleEnv(files[e], 1, C) for e in range(E)]
    for e in range(E):
        assert np.array_equal(obs[e], orcs[e].reset()[0][0]), e
    drv = NoisyRuleDriver(E * C, seed=29)

    def moved(envs, k):
        nonlocal files
        ndraw[envs] += 1
        now = eng.env_track_ids()[0].copy()
        assert np.array_equal(now, replay()), k
        hist.append(now)
        files = eng.env_track_files()
        for e in envs:
            orcs[e].close()
            orcs[e] = OracleEnv(files[e], 1, C)
            assert np.array_equal(obs[e], orcs[e].reset()[0][0]), (k, e, files[e])
    for k in range(K):
        sel = [e for e in range(E) if k in (30 + e, 120 + e, 210 + e)]
        if sel:
            m = torch.zeros(E, dtype=torch.uint8, device=eng.device)
            m[sel] = 1
            obs = eng.reset(m).cpu().numpy().copy()
            moved(sel, k)
        a = drv.actions(obs, k).reshape(E, C, 2)
        go, gr, term, trunc = eng.step(torch.from_numpy(a).cuda(), auto_reset=True, terminal_obs=True)
        obs, gr = go.cpu().numpy().copy(), gr.cpu().numpy()
        ef, tobs = eng.env_flags.cpu().numpy(), eng.terminal_obs.cpu().numpy()
        ended = []
        outs = list(pool.map(lambda e: orcs[e].step(a[e][None]), range(E)))
        for e in range(E):
            oo, orw, ocf, oef = outs[e]
            odone = bool(oef[0, 0] or oef[0, 1])
            assert np.array_equal(gr[e], orw[0]) and odone == bool(ef[e] & 8), (k, e, files[e])
            assert np.array_equal(tobs[e] if odone else obs[e], oo[0]), (k, e, files[e])
            if odone:
                ended.append(e)
        if ended:
            moved(ended, k)
    got, draws = eng.env_track_ids()
    assert np.array_equal(draws, ndraw) and (draws >= 4).all()
    hist = np.array(hist)      # the tracks after the first draw and after every reset
    moves = {(int(a), int(b)) for e in range(E) for a, b in zip(hist[:-1, e], hist[1:, e]) if a != b}
    assert (i64, i1) in moves and (i1, i64) in moves, moves
    pool.shutdown()
    for o in orcs:
        o.close()
    eng.close()


# ---------------------------------------------------------------- the info columns of the wall query
@pytest.mark.parametrize("name,C,epb", [(n, C, epb) for n, C in S.SETS if n.startswith("on_track_query") for epb in S.LAYOUTS[C]])
def test_on_track_info(name, C, epb):
    """nascar_get_info's on_track, lap distance and speed after the step of the on_track_query sets == or_car_info's,
    for every car (query_on_wall through the broadphase grid list, next to faces and corners and far outside the grid)"""
    from nascargymnasium_amd import _lib
    from test_gpu_state_parity import _engine, _load
    c = S.build(name, C)
    ref = S.oracle_info(name, C)
    env = _engine(c, epb)
    try:
        _load(env, c.blob, c.E, C)
        env.step(torch.from_numpy(c.actions.copy()).to(env.device))
        info = env.info_tensor().cpu().numpy().reshape(c.N, -1)
    finally:
        env.close()
    for j, f in enumerate(("on_track", "total_distance_traveled", "speed")):
        g = info[:, _lib.INFO_INDEX[f]]
        bad = np.flatnonzero(g.view(np.uint64) != ref[:, j].view(np.uint64))
        assert len(bad) == 0, f"{name}: info `{f}` differs for {len(bad)} cars, first {bad[0]}: device {g[bad[0]]!r} oracle {ref[bad[0], j]!r}"
    assert (info[:, _lib.INFO_INDEX["on_track"]] == 0.0).sum() >= c.N // 5


# ---------------------------------------------------------------- the case sets through the two-launch path
@pytest.mark.parametrize("name,C,epb", [("chord_ties_seg64", 10, 12), ("chord_ties_seg17", 1, 128), ("startline_band_seg64", 10, 12),
                                        ("chord_ties_degenerate", 1, 128)])
def test_one_step_two_launch(name, C, epb):
    """test_gpu_state_parity.test_one_step steps through the fused model + logic kernel (the engine's default, which
    stages the segments in g_step_segs); here the same sets take model_kernel + logic_kernel (stage_track_lds)"""
    from oracle_lib import gpu_arena
    from test_gpu_state_parity import _engine, _load, compare_outputs, compare_state
    c = S.build(name, C)
    O, obs, rew, cf, ef = S.oracle_step(name, C)
    env = _engine(c, epb)
    try:
        env.set_fused_logic(False)
        _load(env, c.blob, c.E, C)
        env.step(torch.from_numpy(c.actions.copy()).to(env.device))
        what = f"{name} {c.E} x {C} at {epb} envs per workgroup, model_kernel + logic_kernel"
        compare_state(what, gpu_arena(env.get_state().cpu().numpy(), c.E, C), O, C)
        compare_outputs(what, env, obs, rew, cf, ef)
    finally:
        env.close()


def test_island_overflow_flag():
    """More than MAX_ISLAND = 8 touching walls in one island is beyond what the device solves: it must say so.  The
    island_overflow set (state_cases._island_overflow) holds 21 cars that the oracle leaves with more than 8 contact
    records; after the step the device's `overflow` field is 2 for at least one of them and for no other car, the
    flagged cars carry CF_ERROR and info's `error`, and no other car does."""
    from nascargymnasium_amd import _lib
    from oracle_lib import gpu_arena
    from state_cases import i32i
    from test_gpu_state_parity import _engine, _load
    c = S.build("island_overflow", 1)
    env = _engine(c, 128)
    try:
        _load(env, c.blob, c.E, 1)
        env.step(torch.from_numpy(c.actions.copy()).to(env.device))
        over = gpu_arena(env.get_state().cpu().numpy(), c.E, 1)["i32"][i32i["overflow"]]
        cf = env.car_flags.cpu().numpy().reshape(-1)
        err = env.info_tensor().cpu().numpy().reshape(c.N, -1)[:, _lib.INFO_INDEX["error"]]
    finally:
        env.close()
    flagged = over != 0
    assert flagged.any() and (over[flagged] == 2).all(), np.unique(over)
    assert not (flagged & ~c.meta["crowded"]).any(), np.flatnonzero(flagged & ~c.meta["crowded"])
    assert np.array_equal((cf & _lib.CF_ERROR) != 0, flagged) and np.array_equal(err, over.astype(np.float64))

"""Random-track mode on the device (CarEnv(track_file=None), src/car_env.py:243-303, 331-398; learn/ppo.py:65-78):
each env's track draws, the fresh worlds on the new track and the regrouping of the workgroups by track all happen on
the device (BatchedCarEnv.set_random_tracks).  Every env is compared with an oracle env run fresh on each track the env
is sent to, every step; the device's draws are replayed on the host (_lib.track_draw); the rollout equals the per-step
path with the mode on.  A whole batch switching in one step (many switching envs per rt_switch_kernel workgroup) against
the oracle; leaving the mode (clear_random_tracks), entering it with given draw counters and re-seeding in mid-run."""
import numpy as np
import pytest

from block_map_check import assert_block_map, assert_every_env_once

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _actions(rng, E, C):
    """a third of the envs drive (throttle >= 0, random steering: wall crashes, impact disables), the rest idle (stuck
    disables after ~10 s): episodes of ~600-1000 steps, so every env switches track a few times"""
    a = rng.uniform(-1, 1, (E, C, 2)).astype(np.float32)
    drive = (np.arange(E) % 3 == 0)[:, None]
    a[..., 0] = np.where(drive, np.abs(a[..., 0]), 0.0)
    return a


def _replay_tracks(seeds, k0, t0, draws, ids):
    """the track sequence the device must have drawn: draw k of env e from its seed and current track"""
    from nascargymnasium_amd import _lib
    cur = np.array(t0, np.int32)
    for k in range(int(np.min(k0)), int(np.max(draws))):
        live = (k0 <= k) & (k < draws)
        cur = np.where(live, _lib.track_draw(seeds, k, cur, ids), cur)
    return cur


@pytest.mark.parametrize("E,C,epb", [(40, 2, 3), (24, 1, 8)])
def test_random_tracks_vs_oracle_every_step(E, C, epb):
    from nascargymnasium_amd import _lib
    from nascargymnasium_amd.batched import BatchedCarEnv
    from nascargymnasium_amd.track import available_tracks
    from oracle_lib import OracleEnv
    tracks = available_tracks()
    eng = BatchedCarEnv(E, C, [tracks[e % len(tracks)] for e in range(E)], device="cuda:0", envs_per_block=epb)
    seeds = np.arange(E, dtype=np.uint64) * 7919 + 11
    eng.set_random_tracks(tracks, seeds)
    ids = eng.random_track_ids
    t_start = np.array([eng._track_id[tracks[e % len(tracks)]] for e in range(E)], np.int32)
    obs = eng.reset().cpu().numpy()                   # every env draws (draw 0) and gets fresh worlds there
    files = eng.env_track_files()
    orcs = [OracleEnv(files[e], 1, C) for e in range(E)]
    for e in range(E):
        assert np.array_equal(obs[e], orcs[e].reset()[0][0]), e
    rng = np.random.default_rng(21)
    switches, seen = 0, set(files)
    for k in range(1500):
        a = _actions(rng, E, C)
        go, gr, term, trunc = eng.step(torch.from_numpy(a).cuda(), auto_reset=True, terminal_obs=True)
        go, gr = go.cpu().numpy(), gr.cpu().numpy()
        ef = eng.env_flags.cpu().numpy()
        tobs = eng.terminal_obs.cpu().numpy()
        done = np.nonzero(ef & 8)[0]
        files_now = eng.env_track_files() if done.size else files
        for e in range(E):
            oo, orw, _, oef = orcs[e].step(a[e][None])
            assert np.array_equal(gr[e], orw[0]), (k, e)
            odone = bool(oef[0, 0] or oef[0, 1])
            assert odone == bool(ef[e] & 8), (k, e)
            if odone:
                assert np.array_equal(tobs[e], oo[0]), (k, e)          # the old track's final observation
                assert files_now[e] != files[e], (k, e)                # never the track it just drove
                switches += 1
                seen.add(files_now[e])
                orcs[e].close()
                orcs[e] = OracleEnv(files_now[e], 1, C)                 # fresh worlds on the new track
                oo = orcs[e].reset()[0]
            assert np.array_equal(go[e], oo[0]), (k, e)
        files = files_now
    assert switches >= E, switches
    assert len(seen) >= 6, seen
    got, draws = eng.env_track_ids()
    assert np.array_equal(got, _replay_tracks(seeds, np.zeros(E, np.int64), t_start, draws, ids))
    for o in orcs:
        o.close()
    eng.close()


def test_random_tracks_rollout_equals_per_step():
    """nascar_rollout with random tracks on (one shard, the switch and the block map after every step) == per-step
    nascar_step_driven with it on, from the same state: per-step records, final obs, state and track assignment"""
    from nascargymnasium_amd.batched import BatchedCarEnv
    from nascargymnasium_amd.track import available_tracks
    tracks = available_tracks()
    E, C, W, K = 96, 4, 3550, 200
    # reset_on_lap: every env terminates at t > 60 s (step 3601) -- all 96 switch track in one step -- and auto-resets
    engs = [BatchedCarEnv(E, C, [tracks[e % 8] for e in range(E)], reset_on_lap=True, device="cuda:0") for _ in range(2)]
    seeds = np.arange(E, dtype=np.uint64) + 5
    for g in engs:
        g.set_random_tracks(tracks, seeds)
        g.reset()
    a, b = engs
    for k in range(W):
        for g in engs:
            g.step_driven(0, seed=9, step=k, auto_reset=True)
    assert torch.equal(a.get_state(), b.get_state())
    R, EF = [], []
    for k in range(K):
        a.step_driven(0, seed=9, step=W + k, auto_reset=True)
        R.append(a.reward.clone()); EF.append(a.env_flags.clone())
    obs_b, Rb, CFb, EFb = b.rollout(0, K, seed=9, step0=W, auto_reset=True, trajectory=True)
    torch.cuda.synchronize()
    n_reset = 0
    for k in range(K):
        assert torch.equal(R[k], Rb[k]) and torch.equal(EF[k], EFb[k]), k
        n_reset += int(((EF[k] & 8) != 0).sum())
    assert n_reset >= E
    assert torch.equal(a.obs, obs_b)
    assert torch.equal(a.get_state(), b.get_state())
    assert np.array_equal(a.env_track_ids()[0], b.env_track_ids()[0])
    for g in engs:
        g.close()


@pytest.mark.parametrize("extra_tracks", [0, 2])     # 8 tracks: the packed-count fast path; 10: the generic path
def test_device_block_map_matches_host_layout(tmp_path, extra_tracks):
    """block_map_kernel (random-track mode's workgroup layout, rebuilt on the device) against the layout computed here
    from the device's env -> track map, after the initial build, after masked resets (draws) and after steps whose
    auto-resets switch tracks: the used workgroups exactly as expected, the rest empty (track -1)."""
    from nascargymnasium_amd.batched import BatchedCarEnv
    from nascargymnasium_amd.track import available_tracks
    tracks = available_tracks()
    for k in range(extra_tracks):     # copies of bundled tracks under other names: more tracks than the fast path takes
        p = tmp_path / f"extra{k}.track"
        p.write_text(open(tracks[k]).read())
        tracks.append(str(p))
    E, C, epb = 301, 1, 5
    eng = BatchedCarEnv(E, C, [tracks[e % len(tracks)] for e in range(E)], device="cuda:0", envs_per_block=epb)
    eng.set_random_tracks(tracks, np.arange(E, dtype=np.uint64) * 31 + 7)
    rng = np.random.default_rng(3)
    checks = 0

    def check():
        ids, _ = eng.env_track_ids()
        bt, be = eng.block_map()
        assert_block_map(bt, be, ids, len(tracks), epb)
        assert_every_env_once(bt, be, E)
        return 1
    checks += check()
    eng.reset()
    checks += check()
    for k in range(6):
        mask = torch.from_numpy((rng.random(E) < 0.3).astype(np.uint8)).cuda()
        eng.reset(mask)
        checks += check()
    a = torch.zeros(E, C, 2, device="cuda")          # idle: every env stuck-disabled at ~600 steps, auto-resets, switches
    for k in range(700):
        eng.step(a, auto_reset=True)
    checks += check()
    assert checks == 9
    eng.close()


# ------------------------------------------------------------------ many envs switching in one step
_IDLE = {}


def _idle_oracle(C):
    """an idle env's whole first episode on every bundled track (its history depends on nothing else), from the oracle,
    computed once per car count: (rewards [8, K, C], obs [8, K, C, 38], K) -- idle envs end at the same step K - 1 on all
    8 tracks (stuck-disabled, all_cars_disabled), which is asserted here, so a batch of idle envs switches in one step"""
    if C not in _IDLE:
        from nascargymnasium_amd.track import available_tracks
        from oracle_lib import OracleEnv
        rews, obss = [], []
        for t in available_tracks():
            orc = OracleEnv(t, 1, C)
            orc.reset()
            a = np.zeros((1, C, 2), np.float32)
            R, O = [], []
            for k in range(1000):
                oo, orw, _, oef = orc.step(a)
                R.append(orw[0].copy()); O.append(oo[0].copy())
                if oef[0, 0] or oef[0, 1]:
                    assert oef[0, 0] and oef[0, 2] == 1, oef      # terminated: all cars disabled
                    break
            orc.close()
            rews.append(np.array(R)); obss.append(np.array(O))
        assert len({len(r) for r in rews}) == 1, [len(r) for r in rews]
        _IDLE[C] = (np.array(rews), np.array(obss), len(rews[0]))
    return _IDLE[C]


@pytest.mark.parametrize("E,C,epb,sample", [(130, 5, 3, 0), (2100, 1, 8, 32)])
def test_mass_switch_vs_oracle(E, C, epb, sample):
    """Every env of the batch switches track in one step (idle envs on all 8 tracks end at the same step): rt_switch_kernel
    lists up to 64 switching envs per workgroup by ballot prefix (E = 130: workgroups of 64, 64 and 2 envs), resets
    ns * C = 320 > 256 cars in two passes of its car loop and walks their rays in 20 passes; E = 2100: the layout after
    2100 switches in one step, at 3 envs per fast-path thread.  Up to the switch every env equals the idle oracle of its
    track every step; at the switch the terminal observation is the old track's, the new track is the host replay of the
    env's draw, the observation that of a fresh oracle env on the new track; then 40 driven steps against those fresh
    oracles (E = 2100: a fixed sample of 32 envs)."""
    from nascargymnasium_amd import _lib
    from nascargymnasium_amd.batched import BatchedCarEnv
    from nascargymnasium_amd.track import available_tracks
    from oracle_lib import OracleEnv, OracleGroups
    tracks = available_tracks()
    old = (np.arange(E) % 8).astype(np.int32)
    eng = BatchedCarEnv(E, C, [tracks[t] for t in old], device="cuda:0", envs_per_block=epb)
    assert [eng._track_id[t] for t in tracks] == list(range(8))
    idle_rew, idle_obs, K = _idle_oracle(C)
    eng.reset()
    seeds = np.arange(E, dtype=np.uint64) * 7919 + 11
    eng.set_random_tracks(tracks, seeds)         # on from here: the envs stay where they are until their episodes end
    ids = eng.random_track_ids
    zero = torch.zeros(E, C, 2, device="cuda")
    for k in range(K):
        go, gr, term, trunc = eng.step(zero, auto_reset=True, terminal_obs=True)
        assert np.array_equal(gr.cpu().numpy(), idle_rew[old, k]), k
        done = ((eng.env_flags & 8) != 0).cpu().numpy()
        if k < K - 1:
            assert not done.any(), (k, np.nonzero(done)[0][:8])
            assert np.array_equal(go.cpu().numpy(), idle_obs[old, k]), k
    # the end step: every env at once (>= 90 % of them in one and the same step is the least this case is about)
    assert done.sum() >= 0.9 * E and done.all(), (int(done.sum()), np.nonzero(~done)[0][:8])
    assert term.all() and not trunc.any()
    assert np.array_equal(eng.terminal_obs.cpu().numpy(), idle_obs[old, K - 1])
    new, draws = eng.env_track_ids()
    assert np.array_equal(new, _lib.track_draw(seeds, 0, old, ids)) and (draws == 1).all()
    assert (new != old).all() and len(set(new.tolist())) == 8
    bt, be = eng.block_map()
    assert_block_map(bt, be, new, 8, epb)
    assert_every_env_once(bt, be, E)
    fresh = []
    for t in tracks:
        orc = OracleEnv(t, 1, C)
        fresh.append(orc.reset()[0][0].copy())
        orc.close()
    go = go.cpu().numpy()
    for e in range(E):
        assert np.array_equal(go[e], fresh[new[e]]), e
    # 40 driven steps on the new tracks
    if sample:
        sel = [0, 2, 3, 1023, 1024, 2099]
        rng = np.random.default_rng(1)
        for t in range(8):      # some envs of every new track
            on_t = [e for e in np.nonzero(new == t)[0].tolist() if e not in sel]
            sel += rng.choice(on_t, 3, replace=False).tolist()
        sel += [e for e in range(500, E) if e not in sel][:sample - len(sel)]
        sel = np.array(sorted(sel))
        assert len(sel) == sample and len(set(sel.tolist())) == sample
    else:
        sel = np.arange(E)
    orc = OracleGroups([tracks[new[e]] for e in sel], C)
    assert np.array_equal(go[sel], orc.reset()[0])
    rng = np.random.default_rng(33)
    live = np.ones(len(sel), bool)    # an env whose cars are all disabled within these steps ends (the oracle's too): its
    for j in range(40):               # last step is compared, terminal observation included, then it is left out
        a = rng.uniform(-1, 1, (E, C, 2)).astype(np.float32)
        a[..., 0] = np.abs(a[..., 0])
        go, gr, term, trunc = eng.step(torch.from_numpy(a).cuda(), auto_reset=True, terminal_obs=True)
        oo, orw, ocf, oef = orc.step(a[sel])
        odone = (oef[:, 0] != 0) | (oef[:, 1] != 0)
        got = np.where(odone[:, None, None], eng.terminal_obs.cpu().numpy()[sel], go.cpu().numpy()[sel])
        bad = np.argwhere((got != oo) & live[:, None, None])
        assert len(bad) == 0, (f"driven step {j}: obs differ at (env, car, field) {sel[bad[:, 0]][:6].tolist()} "
                               f"{bad[:6, 1:].tolist()}, {len(set(bad[:, 0].tolist()))} envs, new tracks "
                               f"{sorted(set(new[sel[bad[:, 0]]].tolist()))}")
        assert np.array_equal(gr.cpu().numpy()[sel][live], orw[live]), j
        assert np.array_equal(term.cpu().numpy()[sel][live], oef[live, 0] != 0), j
        assert np.array_equal(trunc.cpu().numpy()[sel][live], oef[live, 1] != 0), j
        assert np.array_equal(((eng.env_flags & 8) != 0).cpu().numpy()[sel][live], odone[live]), j
        keep = live & ~odone          # (car flags: of the envs that go on)
        assert np.array_equal(eng.car_flags.cpu().numpy()[sel][keep] & 5, ocf[keep] & 5), j
        live = keep
    # (on the oracle only talladega's envs end this early -- its wall is close to the start pose -- an eighth of them all)
    assert live.sum() >= 0.75 * len(sel), int(live.sum())
    assert float(np.abs(oo[..., 0:5]).max()) > 0      # the cars moved
    orc.close()
    eng.close()


# ------------------------------------------------------------------ mode switches
def _rt_engine(E, C, seeds, epb=None):
    from nascargymnasium_amd.batched import BatchedCarEnv
    from nascargymnasium_amd.track import available_tracks
    tracks = available_tracks()
    eng = BatchedCarEnv(E, C, [tracks[e % 8] for e in range(E)], device="cuda:0", envs_per_block=epb)
    eng.set_random_tracks(tracks, seeds)
    return eng, tracks


def _same_step(a, b, act, auto_reset):
    ta = torch.from_numpy(act).cuda()
    for g in (a, b):
        g.step(ta, auto_reset=auto_reset, terminal_obs=auto_reset)
    for name in ("obs", "reward", "env_flags", "car_flags"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    if auto_reset:
        assert torch.equal(a.terminal_obs, b.terminal_obs)


def test_clear_random_tracks_keeps_the_envs_where_they_are():
    """clear_random_tracks: the envs keep the tracks the device drew for them, the host builds the workgroup layout
    again (its interleaved order), stepping goes on bit-identically to a twin that stays in the mode, and
    set_env_tracks manages the tracks again (refused while the mode is on)."""
    from oracle_lib import OracleEnv
    E, C = 96, 2
    seeds = np.arange(E, dtype=np.uint64) * 13 + 3
    (A, tracks), (B, _) = _rt_engine(E, C, seeds), _rt_engine(E, C, seeds)
    for g in (A, B):
        g.reset()
    rng = np.random.default_rng(21)
    for k in range(300):
        _same_step(A, B, _actions(rng, E, C), True)
    assert torch.equal(A.get_state(), B.get_state())
    ids, _ = A.env_track_ids()
    B.clear_random_tracks()
    assert B.random_track_ids is None
    got, draws = B.env_track_ids()
    assert np.array_equal(got, ids) and (draws == 0).all() and np.array_equal(B.env_track, ids)
    bt, be = B.block_map()
    assert_block_map(bt, be, ids, 8, B.envs_per_block, fixed_grid=False, host_order=True)
    assert_every_env_once(bt, be, E)
    for k in range(60):
        _same_step(A, B, _actions(rng, E, C), False)
        assert torch.equal(A.get_state(), B.get_state()), k
    assert np.array_equal(B.env_track_ids()[0], ids) and np.array_equal(A.env_track_ids()[0], ids)
    with pytest.raises(RuntimeError, match="random-track mode is on"):
        A.set_env_tracks([tracks[0]] * E)
    want = [tracks[(e // 3) % 8] for e in range(E)]
    B.set_env_tracks(want)
    assert np.array_equal(B.env_track_ids()[0], ids)              # not before the reset
    obs = B.reset().cpu().numpy()
    now = B.env_track_ids()[0]
    assert np.array_equal(now, (np.arange(E) // 3) % 8)
    bt, be = B.block_map()
    assert_block_map(bt, be, now, 8, B.envs_per_block, fixed_grid=False, host_order=True)
    for t in range(8):
        orc = OracleEnv(tracks[t], 1, C)
        fo = orc.reset()[0][0]
        orc.close()
        assert (obs[now == t] == fo).all(), t
    A.close(); B.close()


def test_set_random_tracks_continues_from_given_draws():
    """set_random_tracks(draws=d) on an engine brought to another's state (its arena, observation, env -> track map and
    draw counters, as bench.py's drop_in pass starts its variants): it makes the other's next draws and stays equal to
    it over a mass reset and the steps after it."""
    from nascargymnasium_amd import _lib
    from nascargymnasium_amd.batched import BatchedCarEnv
    E, C = 96, 2
    seeds = np.arange(E, dtype=np.uint64) * 101 + 9
    A, tracks = _rt_engine(E, C, seeds)
    A.reset()
    rng = np.random.default_rng(5)
    A.reset(torch.from_numpy((rng.random(E) < 0.5).astype(np.uint8)).cuda())     # draw counters 1 and 2
    for k in range(100):
        A.step(torch.from_numpy(_actions(rng, E, C)).cuda(), auto_reset=True)
    ids, draws = A.env_track_ids()
    assert set(draws.tolist()) >= {1, 2}
    B = BatchedCarEnv(E, C, [tracks[e % 8] for e in range(E)], device="cuda:0")
    B.set_env_tracks([tracks[t] for t in ids])       # (applies at once: B has not been reset or stepped)
    B.set_state(A.get_state())
    B.obs.copy_(A.obs)
    B.set_random_tracks(tracks, seeds, draws=draws)
    got, gd = B.env_track_ids()
    assert np.array_equal(got, ids) and np.array_equal(gd, draws)
    for k in range(20):
        _same_step(A, B, _actions(rng, E, C), True)
    ids, draws = A.env_track_ids()
    for g in (A, B):
        g.reset()                                    # the mass reset: every env draws
    want = _lib.track_draw(seeds, draws, ids, A.random_track_ids)
    for g in (A, B):
        got, gd = g.env_track_ids()
        assert np.array_equal(got, want) and np.array_equal(gd, draws + 1)
    assert torch.equal(A.obs, B.obs)
    bt, be = B.block_map()
    assert_block_map(bt, be, want, 8, B.envs_per_block)
    for k in range(40):
        _same_step(A, B, _actions(rng, E, C), True)
    assert torch.equal(A.get_state(), B.get_state())
    assert np.array_equal(A.env_track_ids()[0], B.env_track_ids()[0])
    A.close(); B.close()


def test_vec_env_reseed_mid_run():
    """VecCarEnv.seed(s) and env_method("seed", v, indices=[i]) in the middle of a run: a re-seeded env's next reset takes
    draw 0 of its new seed from the track it is on, the others go on with their counters; episode_tracks replays the
    device's draws from the seeds (it asserts the replay against the device's map itself)."""
    from nascargymnasium_amd import VecCarEnv, _lib
    E = 12
    venv = VecCarEnv(E, None, num_cars=1, seed=5)
    eng = venv.engine
    tid = venv._ids
    venv.reset()
    for k in range(5):
        venv.step(np.zeros((E, 2), np.float32))
    ids0, d0 = eng.env_track_ids()
    assert (d0 == 2).all()                           # draw 0 at construction, draw 1 at the reset
    assert venv.seed(77) == [77 + e for e in range(E)]
    ids, d = eng.env_track_ids()
    assert np.array_equal(ids, ids0) and (d == 0).all()      # the envs stay where they are; counters restart
    venv.reset()
    s77 = np.arange(E, dtype=np.uint64) + 77
    ids1, d1 = eng.env_track_ids()
    assert np.array_equal(ids1, _lib.track_draw(s77, 0, ids0, tid)) and (d1 == 1).all()
    assert [t[-1] for t in venv.episode_tracks] == venv.env_tracks
    for k in range(5):
        venv.step(np.zeros((E, 2), np.float32))
    assert venv.env_method("seed", 1234, indices=[3]) == [[1234]]
    ids, d = eng.env_track_ids()
    assert np.array_equal(ids, ids1) and d[3] == 0 and (np.delete(d, 3) == 1).all()
    venv.reset()
    seeds = s77.copy(); seeds[3] = 1234
    k = np.ones(E, np.int32); k[3] = 0
    ids2, d2 = eng.env_track_ids()
    assert np.array_equal(ids2, _lib.track_draw(seeds, k, ids1, tid)) and np.array_equal(d2, k + 1)
    venv.reset()
    ids3, d3 = eng.env_track_ids()
    assert np.array_equal(ids3, _lib.track_draw(seeds, k + 1, ids2, tid)) and np.array_equal(d3, k + 2)
    et = venv.episode_tracks
    assert [t[-1] for t in et] == venv.env_tracks
    by_id = eng._track_files_by_id
    assert list(et[3]) == [by_id[int(ids2[3])], by_id[int(ids3[3])]]
    assert list(et[0]) == [by_id[int(i[0])] for i in (ids1, ids2, ids3)]
    venv.close()

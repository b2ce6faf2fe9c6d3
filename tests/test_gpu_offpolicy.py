"""On-device off-policy collection (BatchedCarEnv.set_explorer / collect_transitions, policy 7, and
offpolicy.ReplayBuffer.sample) against the host oracle tests/offpolicy_ref.py; the conditions on the inputs are checked on
the host by tests/test_offpolicy_cpu.py.

Tolerances, the rule of tests/test_gpu_onpolicy.py: sampled and noisy actions against float64 within max(8 x max |numpy
f32 - f64| of the same formula on the same rows, 1e-6); everything that is the same arithmetic on both sides (scale /
unscale, the clip, placement, collect_transitions against per-step, the sampler's gather) bit for bit.
"""
import numpy as np
import pytest

import golden_replay as GR
import offpolicy_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from nascargymnasium_amd import _lib                                       # noqa: E402
from nascargymnasium_amd import policy as P                                # noqa: E402
from nascargymnasium_amd.offpolicy import ReplayBuffer, ReplaySamples      # noqa: E402
from test_gpu_field import _engine                                         # noqa: E402
from test_offpolicy_cpu import CLAMP_ROW, golden_obs, raw_head, sac_1235, scaled_head_actor   # noqa: E402

SEED = R.TEST_SEED
NETS = {"sac_1235": sac_1235, "scaled_head": scaled_head_actor}
RING = ("obs", "next_obs", "actions", "rewards", "dones", "timeouts", "live")
f32 = np.float32


def _np(t):
    return t.cpu().numpy()


def _tol(a32, a64):
    return max(8 * float(np.abs(np.asarray(a32, np.float64) - a64).max()), 1e-6)


def _load_obs(env, rows):
    env.reset()
    env.obs.copy_(torch.from_numpy(rows).cuda().reshape(env.E, env.C, 38))


def _close(name, got, h32, h64):
    tol = _tol(h32, h64)
    d = float(np.abs(got.astype(np.float64) - h64).max())
    print(f"{name}: max |kernel - f64| {d:.3g} tol {tol:.3g}")
    assert np.all(np.isfinite(got)) and d <= tol, (name, d, tol)


def _ring_np(rb):
    return {f: _np(getattr(rb, f)).reshape(rb.capacity, rb.N, *getattr(rb, f).shape[3:]) for f in RING}


# ------------------------------------------------------------------ the sampled SAC epilogue at the edge shapes
@pytest.mark.parametrize("E,C", [(1, 1), (31, 1), (32, 1), (33, 1), (37, 5), (129, 1)])
@pytest.mark.parametrize("net", ["sac_1235", "scaled_head"])
def test_epilogue_values_at_the_edge_shapes(net, E, C):
    actor, step, n = NETS[net](), 3, E * C
    rows = golden_obs()[CLAMP_ROW:CLAMP_ROW + n]
    _, ls = raw_head(actor, rows)
    assert ((ls > P.LOG_STD_MAX) | (ls < P.LOG_STD_MIN)).any(), "no clamped row in the slice"
    env = _engine(["martinsville.track"], E, C)
    env.set_explorer(actor)
    _load_obs(env, rows)
    u = _np(env.policy_actions(7, seed=SEED, step=step)).reshape(-1, 2).copy()
    rb = ReplayBuffer(env, 2)
    env.collect_transitions(rb, 1, seed=SEED, step0=step)
    torch.cuda.synchronize()
    assert (rb.pos, rb.size, rb.full) == (1, 1, False)
    ring = _ring_np(rb)
    s = ring["actions"][0]
    assert np.array_equal(ring["obs"][0], rows) and np.array_equal(ring["next_obs"][0], _np(env.obs).reshape(-1, 38))
    u64, s64 = R.squashed_sample(actor, rows, SEED, step, dtype=np.float64)
    u32, s32 = R.squashed_sample(actor, rows, SEED, step, dtype=np.float32)
    _close(f"{net} {E}x{C} u", u, u32, u64)
    _close(f"{net} {E}x{C} s", s, s32, s64)
    assert np.array_equal(s, f32(2) * ((u + f32(1)) / f32(2)) - f32(1))     # scale_action of the kernel's own u
    assert np.abs(u).max() <= 1 and np.abs(s).max() <= 1
    assert not ring["dones"][0].any() and ring["live"][0].all()
    env.close()


# ------------------------------------------------------------------ exploration noise on a deterministic actor
@pytest.mark.parametrize("which", ["sac_1235", "tanh64"])
def test_noise_on_a_deterministic_actor(which):
    ctrl = sac_1235().deterministic() if which == "sac_1235" else P.random_mlp(64, 64, P.TANH, P.OUT_SQUASH, seed=8)
    E, C, step = 37, 5, 6
    rows = golden_obs()[200:200 + E * C]
    env = _engine(["martinsville.track"], E, C)
    env.set_explorer(ctrl)                                                  # sigma None: zeros
    _load_obs(env, rows)
    det = env.controller_forward(env._explorer[0], env.obs).clone()
    assert torch.equal(env.policy_actions(7, seed=SEED, step=step), det)    # sigma = 0: the controller's action, bit for bit
    env.update_explorer(sigma=(0.0, 0.0))
    assert torch.equal(env.policy_actions(7, seed=SEED, step=step), det)
    sigma = (0.15, 0.75)                                                    # learn/ddpg.py:93 and learn/td3_n.py:94
    env.update_explorer(sigma=sigma)
    u = _np(env.policy_actions(7, seed=SEED, step=step)).reshape(-1, 2).copy()
    rb = ReplayBuffer(env, 1)
    env.collect_transitions(rb, 1, seed=SEED, step0=step)
    s = _np(rb.actions[0]).reshape(-1, 2)
    u64, s64 = R.noisy_action(ctrl, sigma, rows, SEED, step, dtype=np.float64)
    u32, s32 = R.noisy_action(ctrl, sigma, rows, SEED, step, dtype=np.float32)
    _close(f"{which} noisy u", u, u32, u64)
    _close(f"{which} noisy s", s, s32, s64)
    assert np.array_equal(u, R.unscale(s))                                  # the env is stepped with unscale_action(s)
    # the clip: wherever the unclipped float64 value is outside the Box by more than the tolerance, s is the bound itself
    det64 = P.mlp_forward_numpy(ctrl, rows, np.float64)
    raw = R.scale(det64, np.float64) + np.asarray(sigma) * R.eps(len(rows), SEED, step, dtype=np.float64)
    out = np.abs(raw) > 1 + 1e-3
    assert out.any() and np.array_equal(s[out], np.sign(raw[out]).astype(f32)) and np.abs(s).max() <= 1
    assert not np.array_equal(u, _np(det).reshape(-1, 2))
    env.close()


def test_a_sampled_actor_takes_no_sigma():
    env = _engine(["martinsville.track"], 4, 1)
    with pytest.raises(ValueError, match="takes no noise sigma"):
        env.set_explorer(scaled_head_actor(), sigma=(0.1, 0.1))
    env.set_explorer(scaled_head_actor())
    with pytest.raises(RuntimeError, match="takes no noise sigma"):
        env.update_explorer(sigma=(0.1, 0.1))
    env.close()


# ------------------------------------------------------------------ placement independence
def _twins(n, tracks, E, C, actor, rows, streams=None):
    envs = [_engine(tracks, E, C) for _ in range(n)]
    for i, e in enumerate(envs):
        e.set_explorer(actor)
        if streams:
            e.set_rollout_streams(streams[i])
    envs[0].reset()
    if rows is not None:
        envs[0].obs.copy_(torch.from_numpy(rows).cuda().reshape(E, C, 38))
    for e in envs[1:]:
        e.reset()
        e.set_state(envs[0].get_state())
        e.obs.copy_(envs[0].obs)
    return envs


def test_one_shard_and_four_shards_agree():
    a, b = _twins(2, ["martinsville.track"], 96, 1, sac_1235(), golden_obs()[:96], streams=(1, 4))
    ra, rb = ReplayBuffer(a, 3), ReplayBuffer(b, 3)
    a.collect_transitions(ra, 4, seed=SEED, step0=7)
    b.collect_transitions(rb, 4, seed=SEED, step0=7)
    torch.cuda.synchronize()
    for f in RING:
        assert torch.equal(getattr(ra, f), getattr(rb, f)), f
    assert torch.equal(a.obs, b.obs) and (ra.pos, ra.full) == (1, True)
    a.close(); b.close()


def test_a_car_in_another_env_slot_and_tile():
    """the same cars as 37 envs x 5 slots and as 185 envs x 1: the draw is the car index's, the net sees the row alone"""
    actor, rows = scaled_head_actor(), golden_obs()[CLAMP_ROW:CLAMP_ROW + 185]
    a, b = _engine(["martinsville.track"], 37, 5), _engine(["martinsville.track"], 185, 1)
    got = []
    for e in (a, b):
        e.set_explorer(actor)
        _load_obs(e, rows)
        u = e.policy_actions(7, seed=SEED, step=2).reshape(-1).clone()
        r = ReplayBuffer(e, 1)
        e.collect_transitions(r, 1, seed=SEED, step0=2)
        got.append((u, r.actions.reshape(-1).clone()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    a.close(); b.close()


def test_random_tracks_do_not_move_the_draws():
    actor, rows = sac_1235(), golden_obs()[:96]
    a, b = _engine(["martinsville.track"], 96, 1), _engine(["martinsville.track"], 96, 1)
    b.set_random_tracks(["martinsville", "daytona"], np.arange(96, dtype=np.uint64) * 13 + 5)
    rings = []
    for e in (a, b):
        e.set_explorer(actor)
        _load_obs(e, rows)
        r = ReplayBuffer(e, 2)
        e.collect_transitions(r, 2, seed=SEED, step0=5)
        rings.append(r)
    torch.cuda.synchronize()
    assert torch.equal(rings[0].actions[0], rings[1].actions[0]) and torch.equal(rings[0].obs[0], rings[1].obs[0])
    # the second record is sampled on another track's observation: against the oracle on the recorded observation
    o1 = _np(rings[1].obs[1]).reshape(-1, 38)
    assert np.array_equal(o1, _np(rings[1].next_obs[0]).reshape(-1, 38))
    _, s64 = R.squashed_sample(actor, o1, SEED, 6, dtype=np.float64)
    _, s32 = R.squashed_sample(actor, o1, SEED, 6, dtype=np.float32)
    _close("random tracks, record 1", _np(rings[1].actions[1]).reshape(-1, 2), s32, s64)
    a.close(); b.close()


# ------------------------------------------------------------------ collect_transitions equals the per-step path
def _host_step(b, ring, source, seed, step):
    """one step of the per-step path on env b into the NumPy ring: policy_actions + step(terminal_obs)"""
    obs = _np(b.obs).reshape(-1, 38).copy()
    u = b.policy_actions(source, seed=seed, step=step).clone()
    b.launch_step(u, auto_reset=True, terminal_obs=True)
    ef, cf = _np(b.env_flags), _np(b.car_flags).reshape(-1)
    done = np.repeat((ef & 3) != 0, b.C)
    timeout = np.repeat(((ef & 2) != 0) & ((ef & 1) == 0), b.C)
    nxt = np.where(done[:, None], _np(b.terminal_obs).reshape(-1, 38), _np(b.obs).reshape(-1, 38))
    live = ((cf & 1) == 0) | ((cf & 2) != 0)
    ring.add(obs, nxt, R.scale(_np(u).reshape(-1, 2)), _np(b.reward).reshape(-1), done, timeout, live)


@pytest.mark.parametrize("source", [7, 0])
@pytest.mark.parametrize("tracks,E,C", [(["martinsville.track"], 33, 1), (["martinsville.track", "daytona.track"], 37, 5)])
def test_collect_transitions_equals_per_step(tracks, E, C, source):
    a, b = _twins(2, tracks, E, C, scaled_head_actor(), None)
    rb, ring, step = ReplayBuffer(a, 5), R.Ring(5, E * C), 40
    for K in (3, 3, 3, 11):                                                 # wraps once, then twice in one call
        a.collect_transitions(rb, K, seed=SEED, step0=step, source=source)
        for k in range(K):
            _host_step(b, ring, source, SEED, step + k)
        step += K
        assert (rb.pos, rb.size, rb.full) == (ring.pos, ring.size, ring.full)
        got = _ring_np(rb)
        for f in RING:
            assert np.array_equal(got[f], getattr(ring, f)), (f, step)
        assert torch.equal(a.obs, b.obs)
    assert torch.equal(a.get_state(), b.get_state())
    a.close(); b.close()


# ------------------------------------------------------------------ episode ends
def _check_sample_dones(rb):
    sm = rb.sample(512, seed=5, draw=1)
    slot, car = R.sample_indices(512, rb.size, rb.N, 5, 1)
    ring = _ring_np(rb)
    want = ring["dones"][slot, car].astype(f32) * (1 - ring["timeouts"][slot, car].astype(f32))
    assert np.array_equal(_np(sm.dones), want)
    return want


def test_a_time_limit_stores_the_terminal_observation_and_a_timeout():
    d = GR.load("daytona_long")
    E, K, warm = 2, 16, 10790
    a, b = _engine(["daytona.track"], E, 1), _engine(["daytona.track"], E, 1)
    a.set_explorer(sac_1235())
    a.reset()
    acts = torch.from_numpy(np.ascontiguousarray(d["actions"][:warm])).cuda()
    for k in range(warm):
        a.launch_step(acts[k].expand(E, 1, 2).contiguous())
    assert not bool(a.env_flags.any())
    b.reset()
    b.set_state(a.get_state())
    b.obs.copy_(a.obs)
    rb = ReplayBuffer(a, K)
    a.collect_transitions(rb, K, seed=SEED, step0=0)
    ring = _ring_np(rb)
    cut = ring["timeouts"] != 0
    assert cut.any() and np.array_equal(ring["dones"], ring["timeouts"]), "no env of the window was cut by the time limit"
    for k in range(K):
        b.launch_step(torch.from_numpy(R.unscale(ring["actions"][k])).cuda().reshape(E, 1, 2), auto_reset=True, terminal_obs=True)
        ef = _np(b.env_flags)
        assert np.array_equal(cut[k], ((ef & 2) != 0) & ((ef & 1) == 0)), k
        nxt = np.where(cut[k][:, None], _np(b.terminal_obs)[:, 0], _np(b.obs)[:, 0])
        assert np.array_equal(ring["next_obs"][k], nxt), k
        if k + 1 < K:
            assert np.array_equal(ring["obs"][k + 1], _np(b.obs)[:, 0])
            for e in np.flatnonzero(cut[k]):                                # the env was reset under the terminal observation
                assert not np.array_equal(ring["next_obs"][k, e], ring["obs"][k + 1, e])
    assert torch.equal(a.obs, b.obs)
    want = _check_sample_dones(rb)
    assert not want.any()                                                   # SB3 does not treat a time limit as terminal
    a.close(); b.close()


def test_a_termination_is_done_without_a_timeout():
    """the fixture's cars brake at a standstill (-1, 0) until the low-reward rule ends the episode at step 835
    (test_gpu_onpolicy.test_terminated_envs_get_no_timeout_value); the explorer here does the same: a squashed actor
    with mean (-10, 0) whatever the observation, no noise"""
    d = GR.load("daytona_low_reward")
    E, C, K, warm = 2, int(d["C"]), 16, 830
    assert np.all(d["actions"][828:836] == f32([-1, 0])) and np.flatnonzero(d["terminated"])[0] == 835
    c = P.random_mlp(64, 64, P.TANH, P.OUT_SQUASH, seed=2)
    c = c._replace(w3=np.zeros_like(c.w3), b3=f32([-10, 0]))
    a = _engine(["daytona.track"], E, C)
    a.set_explorer(c)
    a.reset()
    acts = torch.from_numpy(np.ascontiguousarray(d["actions"][:warm])).cuda()
    for k in range(warm):
        a.launch_step(acts[k].expand(E, C, 2).contiguous())
    assert not bool((a.env_flags & 3).any())
    rb = ReplayBuffer(a, K)
    a.collect_transitions(rb, K, seed=SEED, step0=0)
    ring = _ring_np(rb)
    assert np.all(ring["actions"] == f32([-1, 0]))
    assert ring["dones"].any() and not ring["timeouts"].any(), "no env of the window terminated"
    k, n = [int(x[0]) for x in np.nonzero(ring["dones"])]
    assert k + 1 < K and not np.array_equal(ring["next_obs"][k, n], ring["obs"][k + 1, n])
    idle = ring["dones"][k] == 0
    assert np.array_equal(ring["next_obs"][k][idle], ring["obs"][k + 1][idle])
    want = _check_sample_dones(rb)
    assert want.any() and not want.all()
    a.close()


def test_live_is_zero_exactly_for_cars_disabled_before_the_step():
    """talladega_10car: car 8 is disabled at step 2, cars 1 and 2 at steps 5 and 6 of the fixture's actions"""
    d = GR.load("talladega_10car")
    E, C, warm, K = 2, int(d["C"]), 4, 8
    a = _engine(["talladega.track"], E, C)
    a.set_explorer(sac_1235())
    a.reset()
    acts = torch.from_numpy(np.ascontiguousarray(d["actions"][:warm + K])).cuda()
    for k in range(warm):
        a.launch_step(acts[k].expand(E, C, 2).contiguous())
    rb = ReplayBuffer(a, K)
    before = []
    for k in range(K):
        before.append(_np(a.info_tensor()[..., _lib.INFO_INDEX["disabled"]]).reshape(-1) != 0)
        a.collect_transitions(rb, 1, seed=SEED, step0=k, source=0)
    after = _np(a.info_tensor()[..., _lib.INFO_INDEX["disabled"]]).reshape(-1) != 0
    live, before = _ring_np(rb)["live"], np.array(before)
    print("disabled before each step:", before.sum(1), "after the last:", after.sum())
    assert before.any() and not before.all()
    assert np.array_equal(live == 0, before)
    a.close()


# ------------------------------------------------------------------ the sampler
@pytest.fixture(scope="module")
def filled():
    """37 x 5, capacity 5: the ring after 3 steps (partly filled) and after 8 (full, wrapped), as host copies"""
    env = _engine(["martinsville.track"], 37, 5)
    env.reset()
    rb = ReplayBuffer(env, 5)
    env.collect_transitions(rb, 3, seed=1, step0=0, source=0)
    yield env, rb
    env.close()


def _guarded(B, pad=8):
    dev = "cuda:0"
    mk = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device=dev)
    return ReplaySamples(mk(B + pad, 38), mk(B + pad, 2), mk(B + pad, 38), mk(B + pad), mk(B + pad),
                         torch.full((B + pad,), 201, dtype=torch.uint8, device=dev))


@pytest.mark.parametrize("full", [False, True])
def test_sampler_gathers_the_oracles_rows(filled, full):
    env, rb = filled
    if full and not rb.full:
        env.collect_transitions(rb, 5, seed=1, step0=3, source=0)
    assert rb.size == (5 if full else 3) and rb.full == full
    ring, N = _ring_np(rb), rb.N
    base = None
    for B in (0, 1, 63, 64, 65, 1000):
        out = _guarded(B)
        sm = rb.sample(B, seed=9, draw=4, out=out)
        torch.cuda.synchronize()
        slot, car = R.sample_indices(B, rb.size, N, 9, 4)
        assert slot.size == 0 or (slot.max() < rb.size and car.max() < N)
        want = (ring["obs"][slot, car], ring["actions"][slot, car], ring["next_obs"][slot, car],
                ring["dones"][slot, car].astype(f32) * (1 - ring["timeouts"][slot, car].astype(f32)),
                ring["rewards"][slot, car], ring["live"][slot, car])
        for name, t, w in zip(ReplaySamples._fields, sm, want):
            g = _np(t)
            assert np.array_equal(g[:B], w), (name, B)
            assert np.all(g[B:] == (201 if name == "live" else -7.0)), (name, B, "guard rows")
        if B == 1000:
            base = slot * N + car
            assert len(np.unique(slot)) == rb.size
    for kw in ({"seed": 9, "draw": 5}, {"seed": 10, "draw": 4}):
        s2, c2 = R.sample_indices(1000, rb.size, N, kw["seed"], kw["draw"])
        assert not np.array_equal(s2 * N + c2, base)
        sm = rb.sample(1000, **kw)
        assert np.array_equal(_np(sm.rewards), ring["rewards"][s2, c2])
    fresh = rb.sample(65, seed=9, draw=4)                                   # buffers of the call's own
    assert tuple(fresh.obs.shape) == (65, 38) and torch.equal(fresh.actions, rb.sample(65, seed=9, draw=4).actions)


# ------------------------------------------------------------------ updates and errors
def test_updates_take_no_controller_ids_and_take_effect():
    E, C = 33, 2
    a, fresh = _engine(["martinsville.track"], E, C), _engine(["martinsville.track"], E, C)
    acts = [P.random_squashed_actor(64, 64, seed=50 + i, activation=P.TANH) for i in range(20)]
    a.set_explorer(P.random_squashed_actor(64, 64, seed=1, activation=P.TANH))
    a.reset()
    first = a.policy_actions(7, seed=1, step=0).clone()
    for x in acts:
        a.update_explorer(x)
    ids = [a.add_controller(P.random_mlp(64, 64, P.TANH, P.OUT_CLIP, seed=i)) for i in range(15)]
    assert ids == list(range(1, 16))
    fresh.set_explorer(acts[-1])
    fresh.reset()
    assert not torch.equal(first, a.policy_actions(7, seed=1, step=0))
    ra, rf = ReplayBuffer(a, 4), ReplayBuffer(fresh, 4)
    a.collect_transitions(ra, 3, seed=1, step0=0)
    fresh.collect_transitions(rf, 3, seed=1, step0=0)
    for f in RING:
        assert torch.equal(getattr(ra, f), getattr(rf, f)), f
    with pytest.raises(RuntimeError, match="update of controller"):
        a.update_explorer(P.random_squashed_actor(256, 256, seed=1))
    with pytest.raises(RuntimeError, match="update of controller"):
        a.update_explorer(P.random_mlp(64, 64, P.TANH, P.OUT_SQUASH, seed=1))
    a.close(); fresh.close()


def test_error_paths():
    env = _engine(["martinsville.track"], 8, 2)
    env.reset()
    rb = ReplayBuffer(env, 4)
    with pytest.raises(RuntimeError, match="policy 7 needs an explorer"):
        env.policy_actions(7)
    with pytest.raises(RuntimeError, match="policy 7 needs an explorer"):
        env.collect_transitions(rb, 2)
    with pytest.raises(RuntimeError, match="no explorer loaded"):
        env.update_explorer(scaled_head_actor())
    with pytest.raises(ValueError, match="SquashedActor or an OUT_SQUASH"):
        env.set_explorer(P.random_mlp(64, 64, P.TANH, P.OUT_CLIP))
    env.collect_transitions(rb, 1, source=0)                                # the warm-up source needs no explorer
    env.set_explorer(scaled_head_actor())
    cid = env._explorer[0]
    with pytest.raises(RuntimeError, match="nascar_collect_transitions"):
        env.step_driven(7)
    with pytest.raises(RuntimeError, match="nascar_collect_transitions"):
        env.rollout(7, 2)
    with pytest.raises(RuntimeError, match="critic or a sampled actor"):
        env.set_car_controllers([cid, "rule"])
    with pytest.raises(RuntimeError, match="critic or a sampled actor"):
        env.controller_forward(cid, env.obs)
    with pytest.raises(RuntimeError, match="source must be 7"):
        env.collect_transitions(rb, 2, source=4)
    with pytest.raises(RuntimeError, match="steps must be >= 1"):
        env.collect_transitions(rb, 0)
    env.set_rollout_streams(0)
    with pytest.raises(RuntimeError, match="fused rollout kernel fills no replay ring"):
        env.collect_transitions(rb, 2)
    env.set_rollout_streams(4)
    env.set_rollout_pipe(8)
    with pytest.raises(RuntimeError, match="pipelined rollout fills no replay ring"):
        env.collect_transitions(rb, 2)
    env.set_rollout_pipe(0)
    env.set_fitness(True)
    with pytest.raises(RuntimeError, match="fitness accumulation"):
        env.collect_transitions(rb, 2)
    env.set_fitness(False)
    # the C entry points: pos outside the ring, misaligned pointers, sizes
    import ctypes
    L, st = env.L, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    r = rb.struct()
    obs = ctypes.c_void_p(env.obs.data_ptr())
    for pos in (-1, 4):
        assert L.nascar_collect_transitions(env.h, 7, 0, 0, 1, obs, ctypes.byref(r), pos, st) < 0
        assert b"outside [0, capacity" in L.nascar_last_error()
    assert L.nascar_collect_transitions(env.h, 7, 0, 0, 1, ctypes.c_void_p(env.obs.data_ptr() + 4), ctypes.byref(r), 0, st) < 0
    assert b"8-byte aligned" in L.nascar_last_error()
    bad = rb.struct()
    bad.actions = rb.actions.data_ptr() + 4
    assert L.nascar_collect_transitions(env.h, 7, 0, 0, 1, obs, ctypes.byref(bad), 0, st) < 0
    assert b"8-byte aligned" in L.nascar_last_error()
    out = _guarded(4)
    ptrs = [ctypes.c_void_p(t.data_ptr()) for t in (out.obs, out.next_obs, out.actions, out.rewards, out.dones, out.live)]
    for size in (0, 5):
        assert L.nascar_replay_sample(env.h, ctypes.byref(r), size, 0, 0, 4, *ptrs, st) < 0
        assert b"outside [1, capacity" in L.nascar_last_error()
    assert L.nascar_replay_sample(env.h, ctypes.byref(r), 1, 0, 0, -1, *ptrs, st) < 0 and b"batch must be" in L.nascar_last_error()
    assert L.nascar_replay_sample(env.h, ctypes.byref(bad), 1, 0, 0, 4, *ptrs, st) < 0 and b"8-byte aligned" in L.nascar_last_error()
    ptrs[0] = ctypes.c_void_p(out.obs.data_ptr() + 4)
    assert L.nascar_replay_sample(env.h, ctypes.byref(r), 1, 0, 0, 4, *ptrs, st) < 0 and b"8-byte aligned" in L.nascar_last_error()
    torch.cuda.synchronize()
    assert np.all(_np(out.obs) == -7.0)                                     # nothing was launched
    with pytest.raises(ValueError, match="another env shape"):
        env.collect_transitions(ReplayBuffer(_Shape(env, 8, 1), 2), 1)
    with pytest.raises(ValueError, match="empty"):
        ReplayBuffer(env, 2).sample(4)
    env.set_explorer(None)
    with pytest.raises(RuntimeError, match="policy 7 needs an explorer"):
        env.policy_actions(7)
    env.set_explorer(scaled_head_actor())
    env.collect_transitions(rb, 2)                                          # and after all that it still collects
    assert bool(torch.isfinite(rb.actions).all()) and rb.size == 3
    env.close()


class _Shape:
    """an env's stand-in with another shape, for ReplayBuffer's allocation alone"""

    def __init__(self, env, E, C):
        self.E, self.C, self.N, self.device, self.h = E, C, E * C, env.device, env.h

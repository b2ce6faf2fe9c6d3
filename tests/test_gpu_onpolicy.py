"""On-device on-policy collection (BatchedCarEnv.set_actor_critic / collect / gae, policy 6) against the host oracle
tests/onpolicy_ref.py; the conditions on the inputs are checked on the host by tests/test_onpolicy_cpu.py.

Tolerances: values, sampled actions and log-probabilities against float64 within max(8 x max |numpy f32 - f64| of the same
formula on the same rows, 1e-6), the rule of tests/test_gpu_policy_shapes.py; everything that is the same arithmetic on
both sides (the clip, placement, collect against per-step, GAE against its float32 restatement) bit for bit.
"""
import numpy as np
import pytest

import golden_replay as GR
import onpolicy_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from nascargymnasium_amd import policy as P                              # noqa: E402
from test_gpu_field import _engine                                        # noqa: E402
from test_onpolicy_cpu import golden_obs, ppo_849                         # noqa: E402

SEED = R.TEST_SEED
FIELDS = ("obs", "actions", "log_probs", "values", "rewards", "timeout_values", "car_flags", "env_flags", "advantages",
          "returns")


def _pair():
    """pi 64-64 Tanh and vf 256-128 ReLU: two shapes, so two launches"""
    return P.random_actor_critic(64, 64, P.TANH, log_std=(-0.3, 0.2), seed=11, vf_shape=(256, 128), vf_activation=P.RELU)


NETS = {"ppo_849": ppo_849, "pair": _pair}


def _tol(f32, f64):
    return max(8 * float(np.abs(np.asarray(f32, np.float64) - f64).max()), 1e-6)


def _host(ac, obs, seed, step, ids=None):
    """{dtype: (values, actions, clipped, log_probs)} of the oracle on obs rows [n, 38] for the cars `ids`"""
    out = {}
    for dt in (np.float64, np.float32):
        mu, v = P.actor_critic_numpy(ac, obs, dt)
        a, c, lp = R.sample(mu, ac.log_std, R.eps(len(obs), seed, step, ids, dtype=dt), dt)
        out[dt] = (v, a, c, lp)
    return out


def _check_values(name, got, host, sl=slice(None)):
    worst = {}
    for key, i in (("values", 0), ("actions", 1), ("log_probs", 3)):
        if key not in got:
            continue
        f64, f32 = host[np.float64][i][sl], host[np.float32][i][sl]
        tol = _tol(f32, f64)
        d = float(np.abs(got[key].astype(np.float64) - f64).max())
        worst[key] = (d, tol)
        print(f"{name} {key}: max |kernel - f64| {d:.3g} tol {tol:.3g}")
        assert np.all(np.isfinite(got[key])) and d <= tol, (name, key, d, tol)
    return worst


def _load_obs(env, rows):
    env.reset()
    env.obs.copy_(torch.from_numpy(rows).cuda().reshape(env.E, env.C, 38))


def _np(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------ forward and sample at the edge shapes
@pytest.mark.parametrize("E,C", [(1, 1), (31, 1), (32, 1), (33, 1), (37, 5), (129, 1)])
@pytest.mark.parametrize("net", ["ppo_849", "pair"])
def test_forward_and_sample_at_the_edge_shapes(net, E, C):
    ac, step = NETS[net](), 3
    rows = golden_obs()[100:100 + E * C]
    env = _engine(["martinsville.track"], E, C)
    env.set_actor_critic(ac)
    _load_obs(env, rows)
    pa = _np(env.policy_actions(6, seed=SEED, step=step)).copy()
    b = env.collect(1, seed=SEED, step0=step)
    torch.cuda.synchronize()
    assert [tuple(getattr(b, f).shape) for f in FIELDS] == [(2, E, C, 38), (1, E, C, 2), (1, E, C), (2, E, C), (1, E, C),
                                                             (1, E, C), (1, E, C), (1, E), (1, E, C), (1, E, C)]
    assert np.array_equal(_np(b.obs[0]).reshape(-1, 38), rows) and torch.equal(b.obs[1], env.obs)
    host = _host(ac, rows, SEED, step)
    got = {"values": _np(b.values[0]).ravel(), "actions": _np(b.actions[0]).reshape(-1, 2), "log_probs": _np(b.log_probs[0]).ravel()}
    _check_values(f"{net} {E}x{C}", got, host)
    # the action that drove the envs: np.clip of the recorded one, bit for bit, and what policy_actions(6) returns
    one = np.float32(1)
    assert np.array_equal(pa.reshape(-1, 2), np.clip(got["actions"], -one, one))
    assert (np.abs(got["actions"]) > 1).any() or E * C < 8
    # values [1]: V of the observation after the step
    _, v1 = P.actor_critic_numpy(ac, _np(b.obs[1]).reshape(-1, 38), np.float64)
    _, v1f = P.actor_critic_numpy(ac, _np(b.obs[1]).reshape(-1, 38), np.float32)
    assert np.abs(_np(b.values[1]).ravel() - v1).max() <= _tol(v1f, v1)
    assert not np.any(_np(b.timeout_values))
    env.close()


# ------------------------------------------------------------------ placement independence
def _twins(n, tracks, E, C, ac, rows, streams=None):
    envs = [_engine(tracks, E, C) for _ in range(n)]
    for i, e in enumerate(envs):
        e.set_actor_critic(ac)
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
    ac = ppo_849()
    a, b = _twins(2, ["martinsville.track"], 96, 1, ac, golden_obs()[:96], streams=(1, 4))
    ra, rb = a.collect(4, seed=SEED, step0=7), b.collect(4, seed=SEED, step0=7)
    torch.cuda.synchronize()
    for f in FIELDS:
        assert torch.equal(getattr(ra, f), getattr(rb, f)), f
    a.close(); b.close()


def test_a_car_in_another_env_slot_and_tile():
    """the same cars as 37 envs x 5 slots (4 shards) and as 185 envs x 1: the draw is the car index's, the nets see the
    row alone; then one observation repeated over every row: every car's value is the same bits, and with a vanishing std
    so is its action (the mean), in whatever tile, wave or workgroup the row sits"""
    ac = _pair()
    rows = golden_obs()[300:485]
    a, b = _engine(["martinsville.track"], 37, 5), _engine(["martinsville.track"], 185, 1)
    for e in (a, b):
        e.set_actor_critic(ac)
        _load_obs(e, rows)
    ra, rb = a.collect(1, seed=SEED, step0=2), b.collect(1, seed=SEED, step0=2)
    for f in ("actions", "log_probs"):
        assert torch.equal(getattr(ra, f)[0].reshape(-1), getattr(rb, f)[0].reshape(-1)), f
    assert torch.equal(ra.values[0].reshape(-1), rb.values[0].reshape(-1))
    rep = np.repeat(rows[17:18], 185, axis=0)
    b.update_actor_critic(ac._replace(log_std=np.array([-30.0, -30.0], np.float32)))
    _load_obs(b, rep)
    r = b.collect(1, seed=SEED, step0=2)
    v, act = _np(r.values[0]).ravel(), _np(r.actions[0]).reshape(-1, 2)
    assert np.all(v == v[0]) and np.all(act == act[0])
    mu64, v64 = P.actor_critic_numpy(ac, rep[:1], np.float64)
    mu32, v32 = P.actor_critic_numpy(ac, rep[:1], np.float32)
    assert abs(v[0] - v64[0]) <= _tol(v32, v64) and np.abs(act[0] - mu64[0]).max() <= _tol(mu32, mu64)
    a.close(); b.close()


def test_random_tracks_do_not_move_the_draws():
    ac, rows = ppo_849(), golden_obs()[:96]
    a, b = _engine(["martinsville.track"], 96, 1), _engine(["martinsville.track"], 96, 1)
    b.set_random_tracks(["martinsville", "daytona"], np.arange(96, dtype=np.uint64) * 13 + 5)
    for e in (a, b):
        e.set_actor_critic(ac)
        _load_obs(e, rows)
    pa, pb = a.policy_actions(6, seed=SEED, step=5).clone(), b.policy_actions(6, seed=SEED, step=5).clone()
    ra, rb = a.collect(2, seed=SEED, step0=5), b.collect(2, seed=SEED, step0=5)
    torch.cuda.synchronize()
    assert torch.equal(pa, pb)
    for f in ("actions", "log_probs"):
        assert torch.equal(getattr(ra, f)[0], getattr(rb, f)[0]), f
    assert torch.equal(ra.values[0], rb.values[0])
    # the second record is sampled on another track's observation: against the oracle on the recorded observation
    o1 = _np(rb.obs[1]).reshape(-1, 38)
    got = {"values": _np(rb.values[1]).ravel(), "actions": _np(rb.actions[1]).reshape(-1, 2), "log_probs": _np(rb.log_probs[1]).ravel()}
    _check_values("random tracks, record 1", got, _host(ac, o1, SEED, 6))
    a.close(); b.close()


# ------------------------------------------------------------------ collect equals per-step
@pytest.mark.parametrize("tracks,E,C,streams", [(["martinsville.track"], 96, 1, 4), (["martinsville.track"], 96, 1, 1),
                                                (["martinsville.track", "daytona.track"], 37, 2, 4)])
def test_collect_equals_per_step(tracks, E, C, streams):
    K, step0, ac = 8, 40, ppo_849()
    a, b, c = _twins(3, tracks, E, C, ac, None, streams=(streams, streams, streams))
    snap, obs0 = a.get_state().clone(), a.obs.clone()
    r = a.collect(K, seed=SEED, step0=step0)
    one = torch.tensor(1.0, device="cuda:0")
    assert torch.equal(r.obs[0], obs0)
    for k in range(K):
        act = b.policy_actions(6, seed=SEED, step=step0 + k).clone()
        assert torch.equal(act, torch.clamp(r.actions[k], -one, one)), f"action of step {k}"
        b.launch_step(act, auto_reset=True)
        assert torch.equal(b.obs, r.obs[k + 1]), f"obs differs at step {k}"
        assert torch.equal(b.reward, r.rewards[k]), f"reward differs at step {k}"
        assert torch.equal(b.car_flags, r.car_flags[k]) and torch.equal(b.env_flags, r.env_flags[k]), f"flags differ at step {k}"
    assert torch.equal(a.get_state(), b.get_state()) and torch.equal(a.obs, b.obs)
    assert torch.equal(a.reward, r.rewards[K - 1]) and torch.equal(a.env_flags, r.env_flags[K - 1])
    # K x collect(1) fills the same records, values and log-probabilities included
    for k in range(K):
        r1 = c.collect(1, seed=SEED, step0=step0 + k)
        for f in ("actions", "log_probs", "rewards", "timeout_values", "car_flags", "env_flags"):
            assert torch.equal(getattr(r1, f)[0], getattr(r, f)[k]), (f, k)
        assert torch.equal(r1.values[0], r.values[k]) and torch.equal(r1.values[1], r.values[k + 1]), k
        assert torch.equal(r1.obs[1], r.obs[k + 1]), k
    # the recorded actions are the ones that drove the envs: replayed through plain step() from the same snapshot
    c.set_state(snap)
    c.obs.copy_(obs0)
    for k in range(K):
        c.launch_step(torch.clamp(r.actions[k], -one, one), auto_reset=True)
        assert torch.equal(c.obs, r.obs[k + 1]) and torch.equal(c.reward, r.rewards[k]), k
        assert torch.equal(c.car_flags, r.car_flags[k]) and torch.equal(c.env_flags, r.env_flags[k]), k
    for e in (a, b, c):
        e.close()


# ------------------------------------------------------------------ timeout bootstrap, and collect's GAE
def test_timeout_values_bootstrap_the_time_limit():
    d = GR.load("daytona_long")
    E, K, warm, ac, g, lam = 2, 16, 10790, ppo_849(), 0.98, 0.9
    a, b = _engine(["daytona.track"], E, 1), _engine(["daytona.track"], E, 1)
    a.set_actor_critic(ac)
    a.reset()
    acts = torch.from_numpy(np.ascontiguousarray(d["actions"][:warm])).cuda()          # [warm, 1, 2]
    for k in range(warm):
        a.launch_step(acts[k].expand(E, 1, 2).contiguous())
    assert not bool(a.env_flags.any())
    b.reset()
    b.set_state(a.get_state())
    b.obs.copy_(a.obs)
    r = a.collect(K, seed=SEED, step0=0, gamma=g, gae_lambda=lam)
    ef = _np(r.env_flags)
    cut = (ef & 2 != 0) & (ef & 1 == 0)
    assert cut.any(), "no env of the window was cut by the time limit"
    tv = _np(r.timeout_values)[..., 0]
    one = torch.tensor(1.0, device="cuda:0")
    seen = 0
    for k in range(K):
        b.launch_step(torch.clamp(r.actions[k], -one, one), auto_reset=True, terminal_obs=True)
        assert torch.equal(b.env_flags, r.env_flags[k]) and torch.equal(b.obs, r.obs[k + 1]), k
        if cut[k].any():
            t = _np(b.terminal_obs)[:, 0]
            _, v64 = P.actor_critic_numpy(ac, t, np.float64)
            _, v32 = P.actor_critic_numpy(ac, t, np.float32)
            tol = _tol(v32[cut[k]], v64[cut[k]])
            dv = np.abs(tv[k][cut[k]] - v64[cut[k]]).max()
            print(f"step {k}: timeout values {tv[k][cut[k]]}, V(terminal obs) {v64[cut[k]]}, |diff| {dv:.3g} tol {tol:.3g}")
            assert dv <= tol and np.all(tv[k][cut[k]] != 0)
            assert not np.array_equal(t, _np(r.obs[k + 1])[:, 0])                     # the env was reset under it
            seen += int(cut[k].sum())
    assert seen == int(cut.sum()) and np.all(tv[~cut] == 0)
    # collect's advantages and returns are gae() of its own records, and the float32 restatement's
    adv, ret = a.gae(r.rewards, r.values, r.timeout_values, r.env_flags, g, lam)
    assert torch.equal(adv, r.advantages) and torch.equal(ret, r.returns)
    done = np.repeat((ef & 3 != 0)[:, :, None], 1, axis=2).reshape(K, E)
    ha, hr = R.gae(_np(r.rewards).reshape(K, E), _np(r.values).reshape(K + 1, E), tv, done, g, lam)
    assert np.array_equal(_np(adv).reshape(K, E), ha) and np.array_equal(_np(ret).reshape(K, E), hr)
    a.close(); b.close()


def test_terminated_envs_get_no_timeout_value():
    """an env that terminates (low reward, reason 2) inside the window is reset like a truncated one, but SB3 bootstraps
    only time limits: its timeout values stay exactly 0.  The fixture's cars brake at a standstill (-1, 0) from step 828
    until the low-reward rule ends the episode at step 835; the actor here does the same (mean (-3, 0) whatever the
    observation, a vanishing std), under ppo_849's critic."""
    d = GR.load("daytona_low_reward")
    E, C, K, warm = 2, int(d["C"]), 16, 830
    assert np.all(d["actions"][828:836] == np.float32([-1, 0])) and np.flatnonzero(d["terminated"])[0] == 835
    ac = ppo_849()
    ac = ac._replace(pi=ac.pi._replace(w3=np.zeros_like(ac.pi.w3), b3=np.float32([-3, 0])), log_std=np.float32([-30, -30]))
    a = _engine(["daytona.track"], E, C)
    a.set_actor_critic(ac)
    a.reset()
    acts = torch.from_numpy(np.ascontiguousarray(d["actions"][:warm])).cuda()          # [warm, C, 2]
    for k in range(warm):
        a.launch_step(acts[k].expand(E, C, 2).contiguous())
    assert not bool((a.env_flags & 3).any())
    r = a.collect(K, seed=SEED, step0=0)
    ef = _np(r.env_flags)
    assert (ef & 1).any(), "no env of the window terminated"
    assert (ef[ef & 1 != 0] & 8).all()                                                  # and was reset in the same step
    assert not np.any(_np(r.timeout_values))
    a.close()


# ------------------------------------------------------------------ GAE
@pytest.mark.parametrize("K,E,C", [(1, 3, 2), (5, 3, 2), (64, 130, 3)])
def test_gae_equals_the_float32_restatement(K, E, C):
    rng = np.random.default_rng(K * 1000 + E)
    rewards = rng.normal(0, 1, (K, E, C)).astype(np.float32)
    values = rng.normal(0, 3, (K + 1, E, C)).astype(np.float32)
    kind = rng.choice([0, 1, 2, 3], (K, E), p=[0.9, 0.06, 0.03, 0.01]).astype(np.uint8)   # terminated / truncated bits
    flags = (kind | np.where(kind != 0, 8, 0) | (rng.integers(0, 8, (K, E)) << 4)).astype(np.uint8)   # + reset, reason bits
    cut = kind == 2
    if K > 1:
        cut[K // 2, 0], flags[K // 2, 0] = True, 2 | 8
    tv = np.where(cut[:, :, None], rng.normal(0, 3, (K, E, C)), 0).astype(np.float32)
    done = np.repeat((flags & 3 != 0)[:, :, None], C, axis=2)
    g, lam = 0.99, 0.95
    env = _engine(["martinsville.track"], E, C)
    adv, ret = env.gae(*[torch.from_numpy(x).cuda() for x in (rewards, values, tv, flags)], g, lam)
    ha, hr = R.gae(rewards.reshape(K, -1), values.reshape(K + 1, -1), tv.reshape(K, -1), done.reshape(K, -1), g, lam)
    assert np.array_equal(_np(adv).reshape(K, -1), ha)
    assert np.array_equal(_np(ret).reshape(K, -1), hr)
    if K > 1:
        a64, _ = R.gae(rewards.reshape(K, -1), values.reshape(K + 1, -1), tv.reshape(K, -1), done.reshape(K, -1), g, lam, np.float64)
        assert not np.array_equal(ha.astype(np.float64), a64)
    with pytest.raises(ValueError, match="values"):
        env.gae(*[torch.from_numpy(x).cuda() for x in (rewards, values[:K], tv, flags)], g, lam)
    env.close()


# ------------------------------------------------------------------ error paths and updates
def test_error_paths():
    env = _engine(["martinsville.track"], 8, 2)
    env.reset()
    with pytest.raises(RuntimeError, match="policy 6 needs an actor-critic"):
        env.policy_actions(6)
    with pytest.raises(RuntimeError, match="policy 6 needs an actor-critic"):
        env.collect(2)
    with pytest.raises(RuntimeError, match="no actor-critic loaded"):
        env.update_actor_critic(ppo_849())
    env.set_actor_critic(ppo_849())
    with pytest.raises(RuntimeError, match="policy 6"):
        env.step_driven(6)
    with pytest.raises(RuntimeError, match="nascar_collect"):
        env.rollout(6, 2)
    env.set_rollout_streams(0)
    with pytest.raises(RuntimeError, match="fused rollout kernel has no actor-critic"):
        env.collect(2)
    env.set_rollout_streams(4)
    env.set_rollout_pipe(8)
    with pytest.raises(RuntimeError, match="pipelined rollout has no actor-critic"):
        env.collect(2)
    env.set_rollout_pipe(0)
    env.set_fitness(True)
    with pytest.raises(RuntimeError, match="fitness accumulation"):
        env.collect(2)
    env.set_fitness(False)
    with pytest.raises(RuntimeError, match="update of controller"):
        env.update_actor_critic(_pair())
    with pytest.raises(RuntimeError, match="critic or a sampled actor"):
        env.set_car_controllers([0, 1])
    with pytest.raises(RuntimeError, match="critic or a sampled actor"):
        env.controller_forward(1, env.obs)
    small = env.collect(2)
    with pytest.raises(ValueError, match="fewer than steps"):
        env.collect(3, out=small)
    r = env.collect(2)                                                      # and after all that it still collects
    assert bool(torch.isfinite(r.advantages).all())
    env.close()


def test_updates_take_no_controller_ids_and_take_effect():
    E, C, K = 33, 2, 3
    ac0 = P.random_actor_critic(64, 64, P.TANH, log_std=(-0.5, -0.1), seed=1)
    acs = [P.random_actor_critic(64, 64, P.TANH, log_std=(-0.4 + 0.01 * i, 0.1), seed=50 + i) for i in range(40)]
    a, fresh = _engine(["martinsville.track"], E, C), _engine(["martinsville.track"], E, C)
    a.set_actor_critic(ac0)
    a.reset()
    first = a.policy_actions(6, seed=1, step=0).clone()
    for ac in acs:
        a.update_actor_critic(ac)
    ids = [a.add_controller(P.random_mlp(64, 64, P.TANH, P.OUT_CLIP, seed=i)) for i in range(14)]
    assert ids == list(range(2, 16))                                        # the 16th id of the handle
    with pytest.raises(RuntimeError, match="at most 16 controllers"):
        a.add_controller(P.random_mlp(64, 64, P.TANH, P.OUT_CLIP, seed=99))
    fresh.set_actor_critic(acs[-1])
    fresh.reset()
    assert not torch.equal(first, a.policy_actions(6, seed=1, step=0))
    ra, rf = a.collect(K, seed=1, step0=0), fresh.collect(K, seed=1, step0=0)
    torch.cuda.synchronize()
    for f in FIELDS:
        assert torch.equal(getattr(ra, f), getattr(rf, f)), f
    a.close(); fresh.close()

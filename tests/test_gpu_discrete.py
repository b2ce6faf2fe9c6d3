"""The categorical actor-critic (policy 6 with a DiscreteActorCritic, MLP_OUT_CATEGORICAL / MLP_OUT_MODE) and the wide
512-512 ReLU kernel on the device, against the host oracle tests/discrete_ref.py; the conditions on the inputs are checked
on the host by tests/test_discrete_cpu.py.

Tolerances: log-probabilities and values against float64 within max(8 x max |numpy f32 - f64| of the same formula on the
same rows, 1e-6), the rule of tests/test_gpu_policy_shapes.py.  The sampled index is discrete: it must be the float64
oracle's on every car whose u is farther than the margin (the same rule on the normalised prefix sums) from each of its
four boundaries, and inside that band one of the categories the band reaches.  Everything that is the same arithmetic on
both sides (the pair table, collect against per-step, the twin stepped by index) bit for bit.
"""
import numpy as np
import pytest

import discrete_ref as D
import golden_replay as GR
import onpolicy_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from nascargymnasium_amd import policy as P                                           # noqa: E402
from nascargymnasium_amd.onpolicy import (DiscreteRolloutBatch, NormalizedDiscreteRolloutBatch,   # noqa: E402
                                           RolloutBatch)
from test_discrete_cpu import NETS, STEP, net_64, net_512                             # noqa: E402
from test_gpu_field import _engine                                                     # noqa: E402
from test_onpolicy_cpu import golden_obs                                               # noqa: E402

SEED = R.TEST_SEED
MART = ["martinsville.track"]
FIELDS = ("obs", "actions", "log_probs", "values", "rewards", "timeout_values", "car_flags", "env_flags", "advantages",
          "returns")


def _tol(f32, f64):
    return max(8 * float(np.abs(np.asarray(f32, np.float64) - f64).max()), 1e-6)


def _np(t):
    return t.cpu().numpy()


def _load_obs(env, rows):
    env.reset()
    env.obs.copy_(torch.from_numpy(rows).cuda().reshape(env.E, env.C, 38))


def _pairs(idx):
    return torch.from_numpy(D.PAIRS).cuda()[idx.long()]


def _check_draw(name, ac, rows, idx, logp, values, seed, step, ids=None):
    """the device's indices, log-probabilities and values on obs rows [n, 38] against the float64 oracle"""
    n = len(rows)
    l64, v64 = P.discrete_actor_critic_numpy(ac, rows, np.float64)
    l32, v32 = P.discrete_actor_critic_numpy(ac, rows, np.float32)
    u = D.uniform(n, seed, step, ids)
    margin, inb = D.band(l32, l64, u)
    a64, _, p64 = D.sample(l64, u, np.float64)
    lo, hi = (p64 <= (u - margin)[:, None]).sum(axis=1), (p64 <= (u + margin)[:, None]).sum(axis=1)
    print(f"{name}: margin {margin:.3g}, {int(inb.sum())} of {n} cars in the band, counts {np.bincount(idx, minlength=5).tolist()}")
    assert idx.min() >= 0 and idx.max() <= 4
    assert inb.mean() <= 0.01
    assert np.array_equal(idx[~inb], a64[~inb])
    assert np.all((idx[inb] >= lo[inb]) & (idx[inb] <= hi[inb]))
    lp64, lp32 = D.logp_of(l64, idx, np.float64), D.logp_of(l32, idx, np.float32)
    for key, got, f32, f64 in (("log_probs", logp, lp32, lp64), ("values", values, v32, v64)):
        tol, d = _tol(f32, f64), float(np.abs(got.astype(np.float64) - f64).max())
        print(f"{name} {key}: max |kernel - f64| {d:.3g} tol {tol:.3g}")
        assert np.all(np.isfinite(got)) and d <= tol, (name, key, d, tol)


# ------------------------------------------------------------------ forward and sample at the edge shapes
@pytest.mark.parametrize("E,C", [(1, 1), (31, 1), (32, 1), (33, 1), (37, 5), (129, 1)])
@pytest.mark.parametrize("net", ["64", "split", "512"])
def test_forward_and_sample_at_the_edge_shapes(net, E, C):
    ac = NETS[net]()
    rows = golden_obs()[100:100 + E * C]
    env = _engine(MART, E, C)
    env.set_actor_critic(ac)
    _load_obs(env, rows)
    pa = env.policy_actions(6, seed=SEED, step=STEP).clone()
    b = env.collect(1, seed=SEED, step0=STEP)
    torch.cuda.synchronize()
    assert isinstance(b, DiscreteRolloutBatch)
    assert [tuple(getattr(b, f).shape) for f in FIELDS] == [(2, E, C, 38), (1, E, C), (1, E, C), (2, E, C), (1, E, C),
                                                             (1, E, C), (1, E, C), (1, E), (1, E, C), (1, E, C)]
    assert [getattr(b, f).dtype for f in FIELDS] == [torch.float32, torch.int32] + [torch.float32] * 4 + [torch.uint8] * 2 + \
        [torch.float32] * 2
    assert np.array_equal(_np(b.obs[0]).reshape(-1, 38), rows) and torch.equal(b.obs[1], env.obs)
    idx = _np(b.actions[0]).ravel().astype(np.int64)
    _check_draw(f"{net} {E}x{C}", ac, rows, idx, _np(b.log_probs[0]).ravel(), _np(b.values[0]).ravel(), SEED, STEP)
    # the action that drove the envs: the table pair of the recorded index, bit for bit, and what policy_actions(6) returns
    assert torch.equal(pa, _pairs(b.actions[0]))
    # values [1]: V of the observation after the step
    o1 = _np(b.obs[1]).reshape(-1, 38)
    _, v1 = P.discrete_actor_critic_numpy(ac, o1, np.float64)
    _, v1f = P.discrete_actor_critic_numpy(ac, o1, np.float32)
    assert np.abs(_np(b.values[1]).ravel() - v1).max() <= _tol(v1f, v1)
    assert not np.any(_np(b.timeout_values))
    env.close()


# ------------------------------------------------------------------ the recorded index steps the env as step() does
def _twins(n, E, C, ac, rows=None, streams=None, tracks=MART):
    envs = [_engine(tracks, E, C) for _ in range(n)]
    for i, e in enumerate(envs):
        if ac is not None:
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


@pytest.mark.parametrize("E,C", [(96, 1), (37, 5)])
def test_a_twin_stepped_by_the_recorded_index(E, C):
    K = 40
    a, b = _twins(2, E, C, net_64())
    r = a.collect(K, seed=SEED, step0=5)
    assert r.actions.dtype == torch.int32 and len(torch.unique(r.actions)) == 5
    for k in range(K):
        b.launch_step(r.actions[k], auto_reset=True)                        # int32: nascar_step's discrete path
        assert torch.equal(b.obs, r.obs[k + 1]) and torch.equal(b.reward, r.rewards[k]), k
        assert torch.equal(b.car_flags, r.car_flags[k]) and torch.equal(b.env_flags, r.env_flags[k]), k
    assert torch.equal(a.get_state(), b.get_state()) and torch.equal(a.obs, b.obs)
    a.close(); b.close()


# ------------------------------------------------------------------ path equivalence
@pytest.mark.parametrize("net", ["64", "512"])
def test_collect_equals_per_step_and_one_shard_equals_four(net):
    K, step0, ac = 6, 40, NETS[net]()
    a4, a1, b = _twins(3, 96, 1, ac, streams=(4, 1, 4))
    obs0 = a4.obs.clone()
    r4, r1 = a4.collect(K, seed=SEED, step0=step0), a1.collect(K, seed=SEED, step0=step0)
    torch.cuda.synchronize()
    for f in FIELDS:
        assert torch.equal(getattr(r4, f), getattr(r1, f)), f
    assert torch.equal(r4.obs[0], obs0)
    for k in range(K):
        act = b.policy_actions(6, seed=SEED, step=step0 + k).clone()
        assert torch.equal(act, _pairs(r4.actions[k])), f"action of step {k}"
        b.launch_step(act, auto_reset=True)
        assert torch.equal(b.obs, r4.obs[k + 1]) and torch.equal(b.reward, r4.rewards[k]), k
        assert torch.equal(b.car_flags, r4.car_flags[k]) and torch.equal(b.env_flags, r4.env_flags[k]), k
    assert torch.equal(a4.get_state(), b.get_state()) and torch.equal(a1.get_state(), b.get_state())
    adv, ret = a4.gae(r4.rewards, r4.values, r4.timeout_values, r4.env_flags)
    assert torch.equal(adv, r4.advantages) and torch.equal(ret, r4.returns)
    for e in (a4, a1, b):
        e.close()


@pytest.mark.parametrize("net", ["split", "512"])
def test_a_car_in_another_env_slot_and_tile_keeps_its_draw(net):
    ac = NETS[net]()
    rows = golden_obs()[300:485]
    a, b = _engine(MART, 37, 5), _engine(MART, 185, 1)
    for e in (a, b):
        e.set_actor_critic(ac)
        _load_obs(e, rows)
    ra, rb = a.collect(1, seed=SEED, step0=2), b.collect(1, seed=SEED, step0=2)
    for f in ("actions", "log_probs"):
        assert torch.equal(getattr(ra, f)[0].reshape(-1), getattr(rb, f)[0].reshape(-1)), f
    assert torch.equal(ra.values[0].reshape(-1), rb.values[0].reshape(-1))
    a.close(); b.close()


# ------------------------------------------------------------------ under normalisation
def test_collect_equals_per_step_under_normalisation():
    E, C, K, step0, ac = 96, 1, 20, 40, net_64()
    envs = []
    for _ in range(2):
        e = _engine(MART, E, C)
        e.set_actor_critic(ac)
        e.reset()
        e.rollout(0, 30, seed=3)
        e.set_normalize(clip_obs=1.0)
        e.normalize_step()
        envs.append(e)
    a, b = envs
    assert a.norm_stats() == b.norm_stats() and torch.equal(a.norm_obs, b.norm_obs)
    obs0 = a.norm_obs.clone()
    r = a.collect(K, seed=SEED, step0=step0)
    assert isinstance(r, NormalizedDiscreteRolloutBatch) and r.actions.dtype == torch.int32 and torch.equal(r.obs[0], obs0)
    for k in range(K):
        act = b.policy_actions(6, seed=SEED, step=step0 + k, obs=b.norm_obs).clone()
        assert torch.equal(act, _pairs(r.actions[k])), f"action of step {k}"
        b.launch_step(act, auto_reset=True, terminal_obs=True)
        b.normalize_step(terminal_obs=True)
        assert torch.equal(b.norm_obs, r.obs[k + 1]), f"normalised obs differs at step {k}"
        assert torch.equal(b.norm_reward, r.rewards[k]) and torch.equal(b.reward, r.raw_rewards[k]), f"reward differs at step {k}"
        assert torch.equal(b.car_flags, r.car_flags[k]) and torch.equal(b.env_flags, r.env_flags[k]), f"flags differ at step {k}"
    assert a.norm_stats() == b.norm_stats()
    assert torch.equal(a.get_state(), b.get_state()) and torch.equal(a.obs, b.obs) and torch.equal(a.norm_obs, b.norm_obs)
    # the nets saw the normalised record
    _check_draw("normalised, record 2", ac, _np(r.obs[2]).reshape(-1, 38), _np(r.actions[2]).ravel().astype(np.int64),
                _np(r.log_probs[2]).ravel(), _np(r.values[2]).ravel(), SEED, step0 + 2)
    a.close(); b.close()


# ------------------------------------------------------------------ the wide critic's timeout values
def test_the_wide_critic_bootstraps_the_time_limit():
    d = GR.load("daytona_long")
    E, K, warm, ac = 2, 16, 10790, net_512()
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
    r = a.collect(K, seed=SEED, step0=0)
    ef = _np(r.env_flags)
    cut = (ef & 2 != 0) & (ef & 1 == 0)
    assert cut.any(), "no env of the window was cut by the time limit"
    tv = _np(r.timeout_values)[..., 0]
    seen = 0
    for k in range(K):
        b.launch_step(r.actions[k], auto_reset=True, terminal_obs=True)
        assert torch.equal(b.env_flags, r.env_flags[k]) and torch.equal(b.obs, r.obs[k + 1]), k
        if cut[k].any():
            t = _np(b.terminal_obs)[:, 0]
            _, v64 = P.discrete_actor_critic_numpy(ac, t, np.float64)
            _, v32 = P.discrete_actor_critic_numpy(ac, t, np.float32)
            tol = _tol(v32[cut[k]], v64[cut[k]])
            dv = np.abs(tv[k][cut[k]] - v64[cut[k]]).max()
            print(f"step {k}: timeout values {tv[k][cut[k]]}, V(terminal obs) {v64[cut[k]]}, |diff| {dv:.3g} tol {tol:.3g}")
            assert dv <= tol and np.all(tv[k][cut[k]] != 0)
            seen += int(cut[k].sum())
    assert seen == int(cut.sum()) and np.all(tv[~cut] == 0)
    a.close(); b.close()


# ------------------------------------------------------------------ the mode as a driver of the field
@pytest.mark.parametrize("net", ["64", "512"])
def test_the_mode_drives_a_field_slot(net):
    E, C, K, ac = 67, 3, 5, NETS[net]()
    a, b = _twins(2, E, C, None)
    for e in (a, b):
        cid = e.add_controller(ac.deterministic())
        e.set_car_controllers(["rule", cid, "rule"])
    # rollout(4, K) equals K x (policy_actions(4) + step)
    obs, rew, cf, ef = a.rollout(4, K, seed=SEED, step0=9, trajectory=True, obs_trajectory=True)
    for k in range(K):
        b.launch_step(b.policy_actions(4, seed=SEED, step=9 + k).clone(), auto_reset=True)
        assert torch.equal(b.obs, obs[k + 1]) and torch.equal(b.reward, rew[k]), k
        assert torch.equal(b.car_flags, cf[k]) and torch.equal(b.env_flags, ef[k]), k
    assert torch.equal(a.get_state(), b.get_state())
    # the slot's cars take the float64 arg max
    rows = golden_obs()[500:500 + E * C]
    a.obs.copy_(torch.from_numpy(rows).cuda().reshape(E, C, 38))
    act = _np(a.policy_actions(4, seed=SEED, step=1))
    mine = rows.reshape(E, C, 38)[:, 1]
    l64, _ = P.discrete_actor_critic_numpy(ac, mine, np.float64)
    l32, _ = P.discrete_actor_critic_numpy(ac, mine, np.float32)
    tol = _tol(l32, l64)
    top = np.sort(l64, axis=1)
    sure = top[:, 4] - top[:, 3] > tol
    print(f"mode {net}: logit tol {tol:.3g}, {int((~sure).sum())} of {E} cars excluded")
    assert (~sure).mean() <= 0.01
    assert np.array_equal(act[:, 1][sure], D.PAIRS[D.mode(l64)][sure])
    assert all(any(np.array_equal(p, q) for q in D.PAIRS) for p in act[:, 1])
    got = a.controller_forward(cid, torch.from_numpy(mine).cuda())
    assert np.array_equal(_np(got), act[:, 1])
    a.close(); b.close()


# ------------------------------------------------------------------ updates and errors
def test_updates_take_no_controller_ids_and_change_the_distribution():
    E, C = 64, 2
    ac0 = net_64()
    a, fresh = _engine(MART, E, C), _engine(MART, E, C)
    a.set_actor_critic(ac0)
    a.reset()
    first = a.policy_actions(6, seed=1, step=0).clone()
    new = None
    for i in range(20):
        new = P.random_discrete_actor_critic(64, 64, P.TANH, seed=50 + i)
        new = new._replace(pi=new.pi._replace(b3=np.float32([0, 0, 9, 0, 0])))      # nearly always category 2
        a.update_actor_critic(new)
    ids = [a.add_controller(P.random_mlp(64, 64, P.TANH, P.OUT_CLIP, seed=i)) for i in range(14)]
    assert ids == list(range(2, 16))
    fresh.set_actor_critic(new)
    fresh.reset()
    ra, rf = a.collect(2, seed=1, step0=0), fresh.collect(2, seed=1, step0=0)
    torch.cuda.synchronize()
    for f in FIELDS:
        assert torch.equal(getattr(ra, f), getattr(rf, f)), f
    brake = torch.tensor([-1.0, 0.0], device="cuda:0")                              # the pair of category 2
    assert float((first == brake).all(dim=2).float().mean()) < 0.6 and float((ra.actions == 2).float().mean()) > 0.9
    a.close(); fresh.close()


def test_error_paths():
    env = _engine(MART, 8, 2)
    env.reset()
    env.set_actor_critic(P.random_actor_critic(64, 64, P.TANH, seed=1))                  # a Gaussian-loaded handle
    with pytest.raises(RuntimeError, match="update of controller"):
        env.update_actor_critic(net_64())
    assert isinstance(env.collect(1), RolloutBatch)
    env.set_actor_critic(net_64())
    with pytest.raises(RuntimeError, match="update of controller"):
        env.update_actor_critic(P.random_actor_critic(64, 64, P.TANH, seed=1))
    plain = RolloutBatch(*[torch.empty((2 + x, *inner), dtype=dt, device="cuda:0") for _n, dt, inner, x in RolloutBatch.spec(8, 2)])
    with pytest.raises(ValueError, match="DiscreteRolloutBatch"):
        env.collect(2, out=plain)
    mine = DiscreteRolloutBatch(*[torch.empty((2 + x, *inner), dtype=dt, device="cuda:0")
                                  for _n, dt, inner, x in DiscreteRolloutBatch.spec(8, 2)])
    r = env.collect(2, out=mine)
    assert r.actions.data_ptr() == mine.actions.data_ptr() and int(r.actions.max()) <= 4
    wide = P.random_mlp(512, 512, P.RELU, P.OUT_SQUASH, seed=1)
    with pytest.raises(RuntimeError, match="512-512: the wide kernel holds no exploring epilogue"):
        env.set_explorer(wide, sigma=(0.1, 0.1))
    with pytest.raises(RuntimeError, match="no explorer head"):
        env.set_explorer(P.random_squashed_actor(512, 512))
    with pytest.raises(RuntimeError, match="critic or a sampled actor"):
        env.set_car_controllers([2, 3])                                                  # output 6 is no driver of the field
    r = env.collect(2)                                                                   # and after all that it still collects
    assert isinstance(r, DiscreteRolloutBatch) and bool(torch.isfinite(r.advantages).all())
    env.close()

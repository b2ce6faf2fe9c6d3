"""Running normalisation on the device (BatchedCarEnv.set_normalize / normalize_step / norm_stats, and collect under it)
against tests/normalize_ref.py, the NumPy restatement of SB3's RunningMeanStd / VecNormalize with float64 batch moments;
tests/test_normalize_cpu.py checks on the host that the inputs used here exercise the clip, the epsilon and both variance
scales.

Bounds.  Batch moments are sums of N float64 terms taken in another order than NumPy's: with u = 2^-53 a column's mean is
held to 4 N u max|x| and its variance to 8 N u max|x|^2 per update (normalize_ref.moment_bounds); a float32 accumulator
misses that at every N above a handful.  Everything that is the same arithmetic on both sides -- normalize_obs and
normalize_reward given the device's statistics, the counts, collect against the per-step loop -- is bit for bit."""
import ctypes

import numpy as np
import pytest

import golden_replay as GR
import normalize_ref as NR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from nascargymnasium_amd import _lib, policy as P                         # noqa: E402
from nascargymnasium_amd.normalize import NormStats                       # noqa: E402
from nascargymnasium_amd.onpolicy import NormalizedRolloutBatch, RolloutBatch   # noqa: E402
from test_gpu_field import _engine                                        # noqa: E402
from test_gpu_onpolicy import FIELDS, SEED, _np, _tol                     # noqa: E402
from test_onpolicy_cpu import golden_obs, ppo_849                         # noqa: E402

NFIELDS = FIELDS + ("raw_rewards",)
MART = ["martinsville.track"]


def _feed(env, rows, reward=None, flags=None, term=None):
    """one normalize_step on caller-given step outputs"""
    env.obs.copy_(torch.from_numpy(rows).cuda().reshape(env.E, env.C, 38))
    env.reward.copy_(torch.from_numpy(np.zeros(env.N, np.float32) if reward is None else reward).cuda().reshape(env.E, env.C))
    env.env_flags.copy_(torch.from_numpy(np.zeros(env.E, np.uint8) if flags is None else flags).cuda())
    if term is not None:
        env.terminal_obs.copy_(torch.from_numpy(term).cuda().reshape(env.E, env.C, 38))
    env.normalize_step(terminal_obs=term is not None)


def _rewards(rows):
    """a float32 reward column with both signs from the rows themselves"""
    return (rows[:, 2] - rows[:, 5] * np.float32(0.5) + rows[:, 21]).astype(np.float32)


def _check_stats(name, got, ref, obs_rows, ret_rows, updates):
    """device statistics `got` (NormStats) against the restatement `ref` (NR.VecNormalize) within the summation bounds;
    obs_rows / ret_rows: every row of the `updates` batches (max |x| is taken over them, N is one batch's)"""
    n = len(obs_rows) // updates
    mb, vb = NR.moment_bounds(obs_rows, updates, n)
    dm, dv = np.abs(got.obs_mean - ref.obs_rms.mean), np.abs(got.obs_var - ref.obs_rms.var)
    rmb, rvb = NR.moment_bounds(np.asarray(ret_rows, np.float64).reshape(-1, 1), updates, n)
    drm, drv = abs(got.ret_mean - ref.ret_rms.mean), abs(got.ret_var - ref.ret_rms.var)
    print(f"{name}: obs mean worst {np.max(dm / np.maximum(mb, 1e-300)):.3g} of its bound, var {np.max(dv / np.maximum(vb, 1e-300)):.3g}; "
          f"ret mean {drm:.3g} (bound {rmb[0]:.3g}), var {drv:.3g} (bound {rvb[0]:.3g})")
    assert np.all(dm <= mb), (name, "obs_mean", dm.max())
    assert np.all(dv <= vb), (name, "obs_var", dv.max())
    assert drm <= rmb[0] and drv <= rvb[0], (name, "returns", drm, drv)
    assert got.obs_count == ref.obs_rms.count and got.ret_count == ref.ret_rms.count, name   # exact


# ------------------------------------------------------------------ moments at the shapes where the reduction can go wrong
@pytest.mark.parametrize("E,C", [(1, 1), (31, 1), (33, 1), (129, 1), (37, 5), (1100, 1)])
def test_one_update_from_fresh_statistics(E, C):
    """1100 rows: four full workgroups of the moments kernel (256 rows each) and one of 76"""
    N = E * C
    rows = NR.batch_rows(golden_obs(), N)
    rew = _rewards(rows)
    env = _engine(MART, E, C)
    env.reset()
    env.set_normalize()
    fresh = env.norm_stats()
    assert fresh == NormStats.fresh(N)
    _feed(env, rows, rew)
    got = env.norm_stats()
    ref = NR.VecNormalize(N)
    ref.step_wait(rows, rew, np.zeros(N, bool))
    _check_stats(f"{E}x{C}", got, ref, rows, rew, 1)
    # against np.mean / np.var of the float64-cast rows directly: one update from the 1e-4 prior leaves them nearly bare
    x = rows.astype(np.float64)
    mb, vb = NR.moment_bounds(rows)
    tot = N + 1e-4
    assert np.all(np.abs(got.obs_mean * tot / N - x.mean(axis=0)) <= mb + 4 * NR.U * np.abs(x).max(axis=0))
    assert np.array_equal(got.returns, rew.astype(np.float64))
    # the same call again on a second engine: the same bits
    twin = _engine(MART, E, C)
    twin.reset()
    twin.set_normalize()
    _feed(twin, rows, rew)
    assert twin.norm_stats() == got
    env.close(); twin.close()


@pytest.mark.parametrize("E,C", [(37, 5), (1100, 1)])
def test_three_successive_updates(E, C):
    N = E * C
    obs = golden_obs()
    batches = [NR.batch_rows(obs, N, i) for i in range(3)]
    env = _engine(MART, E, C)
    env.reset()
    env.set_normalize(gamma=0.9)
    ref = NR.VecNormalize(N, gamma=0.9)
    rets = []
    for b in batches:
        _feed(env, b, _rewards(b))
        ref.step_wait(b, _rewards(b), np.zeros(N, bool))
        rets.append(ref.returns.copy())
    got = env.norm_stats()
    _check_stats(f"{E}x{C} x3", got, ref, np.concatenate(batches), np.concatenate(rets), 3)
    assert got.obs_count == ((1e-4 + N) + N) + N
    assert np.all(np.abs(got.returns - ref.returns) <= 4 * 3 * NR.U * np.abs(ref.returns).max())
    env.close()


# ------------------------------------------------------------------ normalize_obs / normalize_reward, bit for bit
@pytest.mark.parametrize("clip_obs", [1.0, 10.0])
@pytest.mark.parametrize("E,C", [(37, 5), (33, 1)])
def test_normalised_values_are_the_numpy_expressions_on_the_device_statistics(E, C, clip_obs):
    N = E * C
    obs = golden_obs()
    rows, term = NR.batch_rows(obs, N), NR.batch_rows(obs, N, 2)
    rew = _rewards(rows)                                                    # clip_reward = 1.0 binds on some of them
    flags = np.where(np.arange(E) % 4 == 1, 1 | 8, np.where(np.arange(E) % 7 == 2, 2 | 8, 0)).astype(np.uint8)
    done = np.repeat(flags & 3 != 0, C)
    env = _engine(MART, E, C)
    env.reset()
    env.set_normalize(clip_obs=clip_obs, clip_reward=1.0)
    before = env.norm_stats()
    env.norm_terminal_obs.fill_(7.0)
    _feed(env, rows, rew, flags, term)
    st = env.norm_stats()
    nobs, nrew, nterm = _np(env.norm_obs).reshape(N, 38), _np(env.norm_reward).ravel(), _np(env.norm_terminal_obs).reshape(N, 38)
    want = NR.normalize_obs(rows, st.obs_mean, st.obs_var, clip_obs)
    assert np.array_equal(nobs, want), f"worst {np.abs(nobs - want).max():.3g}"
    assert np.array_equal(nrew, NR.normalize_reward(rew, st.ret_var, 1.0))
    assert np.array_equal(nterm[done], NR.normalize_obs(term[done], st.obs_mean, st.obs_var, clip_obs))
    assert np.all(nterm[~done] == 7.0)                                      # rows of envs that did not end: untouched
    if clip_obs == 1.0:
        assert (np.abs(nobs) == 1.0).any() and (np.abs(nobs) < 1.0).any()
    assert (np.abs(nrew) == 1.0).any() and (np.abs(nrew) < 1.0).any()
    # the statistics were updated BEFORE the rows were normalised, the terminal rows' too
    assert not np.array_equal(nobs, NR.normalize_obs(rows, before.obs_mean, before.obs_var, clip_obs))
    assert not np.array_equal(nterm[done], NR.normalize_obs(term[done], before.obs_mean, before.obs_var, clip_obs))
    assert not np.array_equal(nrew, NR.normalize_reward(rew, before.ret_var, 1.0))
    # returns: zeroed for every car of a done env after the reward was normalised, the step's reward elsewhere
    assert np.all(st.returns[done] == 0) and np.array_equal(st.returns[~done], rew[~done].astype(np.float64))
    # the raw buffers are untouched
    assert np.array_equal(_np(env.obs).reshape(N, 38), rows) and np.array_equal(_np(env.reward).ravel(), rew)
    # a flag that is off copies its input
    env.set_normalize(norm_obs=False, norm_reward=True, clip_reward=1.0)
    _feed(env, rows, rew, flags, term)
    assert np.array_equal(_np(env.norm_obs).reshape(N, 38), rows)
    assert np.array_equal(_np(env.norm_terminal_obs).reshape(N, 38)[done], term[done])
    assert env.norm_stats().obs_count == st.obs_count and env.norm_stats().ret_count == st.ret_count + N
    env.close()


# ------------------------------------------------------------------ returns over a window with a done
def test_returns_accumulate_feed_ret_rms_and_are_zeroed_at_a_done():
    """the low-reward fixture: both cars brake at a standstill until the low-reward rule ends the episode at step 835"""
    d = GR.load(NR.RETURN_FIXTURE)
    E, C, K, warm = 2, int(d["C"]), NR.RETURN_K, NR.RETURN_WARM
    N = E * C
    env = _engine(["daytona.track"], E, C)
    env.reset()
    acts = torch.from_numpy(np.ascontiguousarray(d["actions"][:warm + K])).cuda()
    for k in range(warm):
        env.launch_step(acts[k].expand(E, C, 2).contiguous())
    env.set_normalize(clip_obs=1.0, gamma=0.99)
    ref = NR.VecNormalize(N, clip_obs=1.0, gamma=0.99)
    seen_done, all_ret, all_raw = False, [], []
    for k in range(K):
        env.launch_step(acts[warm + k].expand(E, C, 2).contiguous(), auto_reset=True, terminal_obs=True)
        env.normalize_step(terminal_obs=True)
        raw, rew, ef = _np(env.obs).reshape(N, 38), _np(env.reward).ravel(), _np(env.env_flags)
        done = np.repeat(ef & 3 != 0, C)
        term = _np(env.terminal_obs).reshape(N, 38)
        before = ref.returns.copy()
        _, _, rterm = ref.step_wait(raw, rew, done, term)
        all_ret.append(before * 0.99 + rew)
        all_raw.append(raw)
        st = env.norm_stats()
        bound = 4 * (k + 1) * NR.U * max(np.abs(ref.returns).max(), np.abs(all_ret[-1]).max())
        assert np.all(np.abs(st.returns - ref.returns) <= bound), k
        assert np.array_equal(_np(env.norm_reward).ravel(), NR.normalize_reward(rew, st.ret_var, 10.0)), k
        assert np.array_equal(_np(env.norm_obs).reshape(N, 38), NR.normalize_obs(raw, st.obs_mean, st.obs_var, 1.0)), k
        if done.any():
            seen_done = True
            assert np.all(st.returns[done] == 0) and np.all(all_ret[-1][done] != 0)     # they had accumulated: zeroed after
            assert np.array_equal(_np(env.norm_terminal_obs).reshape(N, 38)[done],
                                  NR.normalize_obs(term[done], st.obs_mean, st.obs_var, 1.0))
        if k == 3:
            assert np.all(np.abs(st.returns) > np.abs(rew))                            # more than one step's reward
    assert seen_done, "no env of the window ended"
    got = env.norm_stats()
    _check_stats("returns window", got, ref, np.concatenate(all_raw), np.concatenate(all_ret), K)
    env.close()


# ------------------------------------------------------------------ collect under running statistics
def _warm(env, ac=None, streams=None, **norm):
    """a field that has spread out (30 uniform-random steps from the reset), then normalisation on and one step_wait"""
    if ac is not None:
        env.set_actor_critic(ac)
    if streams is not None:
        env.set_rollout_streams(streams)
    env.reset()
    env.rollout(0, 30, seed=3)
    if norm is not None:
        env.set_normalize(**norm)
        env.normalize_step()
    return env


@pytest.mark.parametrize("E,C,streams", [(96, 1, 1), (96, 1, 4), (37, 5, 1), (37, 5, 4)])
def test_collect_equals_per_step_under_running_statistics(E, C, streams):
    K, step0, ac = 6, 40, ppo_849()
    norm = dict(clip_obs=1.0, gamma=0.99)
    a, b, c = (_warm(_engine(MART, E, C), ac, s, **norm) for s in (streams, 1, streams))
    assert a.norm_stats() == b.norm_stats() and torch.equal(a.norm_obs, b.norm_obs)
    obs0 = a.norm_obs.clone()
    r = a.collect(K, seed=SEED, step0=step0)
    assert isinstance(r, NormalizedRolloutBatch) and torch.equal(r.obs[0], obs0)
    one = torch.tensor(1.0, device="cuda:0")
    for k in range(K):
        act = b.policy_actions(6, seed=SEED, step=step0 + k, obs=b.norm_obs).clone()
        assert torch.equal(act, torch.clamp(r.actions[k], -one, one)), f"action of step {k}"
        b.launch_step(act, auto_reset=True, terminal_obs=True)
        b.normalize_step(terminal_obs=True)
        assert torch.equal(b.norm_obs, r.obs[k + 1]), f"normalised obs differs at step {k}"
        assert torch.equal(b.norm_reward, r.rewards[k]) and torch.equal(b.reward, r.raw_rewards[k]), f"reward differs at step {k}"
        assert torch.equal(b.car_flags, r.car_flags[k]) and torch.equal(b.env_flags, r.env_flags[k]), f"flags differ at step {k}"
        assert not torch.equal(r.rewards[k], r.raw_rewards[k])
    assert a.norm_stats() == b.norm_stats()                                 # the final statistics and returns
    assert torch.equal(a.get_state(), b.get_state()) and torch.equal(a.obs, b.obs) and torch.equal(a.norm_obs, b.norm_obs)
    assert torch.equal(a.reward, r.raw_rewards[K - 1]) and torch.equal(a.norm_reward, r.rewards[K - 1])
    assert not torch.equal(a.obs, a.norm_obs)
    # K x collect(1): values, log-probabilities and timeout values of the same records
    for k in range(K):
        r1 = c.collect(1, seed=SEED, step0=step0 + k)
        for f in ("actions", "log_probs", "rewards", "raw_rewards", "timeout_values", "car_flags", "env_flags"):
            assert torch.equal(getattr(r1, f)[0], getattr(r, f)[k]), (f, k)
        assert torch.equal(r1.values[0], r.values[k]) and torch.equal(r1.values[1], r.values[k + 1]), k
        assert torch.equal(r1.obs[1], r.obs[k + 1]), k
    assert c.norm_stats() == a.norm_stats()
    # the critic valued the normalised record, GAE took the normalised rewards
    _, v64 = P.actor_critic_numpy(ac, _np(r.obs[2]).reshape(-1, 38), np.float64)
    _, v32 = P.actor_critic_numpy(ac, _np(r.obs[2]).reshape(-1, 38), np.float32)
    assert np.abs(_np(r.values[2]).ravel() - v64).max() <= _tol(v32, v64)
    adv, ret = a.gae(r.rewards, r.values, r.timeout_values, r.env_flags)
    assert torch.equal(adv, r.advantages) and torch.equal(ret, r.returns)
    for e in (a, b, c):
        e.close()


def test_one_stream_and_four_streams_agree_under_running_statistics():
    ac = ppo_849()
    a, b = (_warm(_engine(MART, 96, 1), ac, s, clip_obs=1.0) for s in (1, 4))
    ra, rb = a.collect(5, seed=SEED, step0=7), b.collect(5, seed=SEED, step0=7)
    for f in NFIELDS:
        assert torch.equal(getattr(ra, f), getattr(rb, f)), f
    assert a.norm_stats() == b.norm_stats()
    a.close(); b.close()


def test_the_same_rows_as_37x5_and_as_185x1():
    """the batch is the N car slots, whatever the env shape: the same rows give the same statistics and the same records"""
    ac = ppo_849()
    rows = NR.batch_rows(golden_obs(), 185)
    rew = _rewards(rows)
    a, b = _engine(MART, 37, 5), _engine(MART, 185, 1)
    outs = []
    for e in (a, b):
        e.set_actor_critic(ac)
        e.reset()
        e.set_normalize(clip_obs=1.0)
        _feed(e, rows, rew)
        st = e.norm_stats()
        r = e.collect(1, seed=SEED, step0=2)
        outs.append((st, r))
    assert outs[0][0] == outs[1][0]
    for f in ("obs", "actions", "log_probs", "values"):
        assert torch.equal(getattr(outs[0][1], f)[0].reshape(-1), getattr(outs[1][1], f)[0].reshape(-1)), f
    a.close(); b.close()


# ------------------------------------------------------------------ the time-limit bootstrap
def test_timeout_values_are_v_of_the_normalised_terminal_observation():
    """daytona_long as test_gpu_onpolicy.test_timeout_values_bootstrap_the_time_limit replays it: the time limit cuts the
    episode inside the window; the value is V of the terminal observation normalised under the statistics AFTER that
    step's update, within that test's value tolerance, and 0 elsewhere"""
    d = GR.load("daytona_long")
    E, K, warm, ac = 2, 16, 10790, ppo_849()
    a, b = _engine(["daytona.track"], E, 1), _engine(["daytona.track"], E, 1)
    a.set_actor_critic(ac)
    a.reset()
    acts = torch.from_numpy(np.ascontiguousarray(d["actions"][:warm])).cuda()
    for k in range(warm):
        a.launch_step(acts[k].expand(E, 1, 2).contiguous())
    assert not bool(a.env_flags.any())
    b.reset()
    b.set_state(a.get_state())
    b.obs.copy_(a.obs); b.reward.copy_(a.reward); b.env_flags.copy_(a.env_flags)
    for e in (a, b):
        e.set_normalize(clip_obs=1.0)
        e.normalize_step()
    r = a.collect(K, seed=SEED, step0=0)
    ef = _np(r.env_flags)
    cut = (ef & 2 != 0) & (ef & 1 == 0)
    assert cut.any(), "no env of the window was cut by the time limit"
    tv = _np(r.timeout_values)[..., 0]
    one = torch.tensor(1.0, device="cuda:0")
    for k in range(K):
        before = b.norm_stats()
        b.launch_step(torch.clamp(r.actions[k], -one, one), auto_reset=True, terminal_obs=True)
        b.normalize_step(terminal_obs=True)
        assert torch.equal(b.env_flags, r.env_flags[k]) and torch.equal(b.norm_obs, r.obs[k + 1]), k
        if cut[k].any():
            st = b.norm_stats()
            raw = _np(b.terminal_obs)[:, 0]
            t = NR.normalize_obs(raw, st.obs_mean, st.obs_var, 1.0)
            assert np.array_equal(_np(b.norm_terminal_obs)[:, 0][cut[k]], t[cut[k]])
            _, v64 = P.actor_critic_numpy(ac, t, np.float64)
            _, v32 = P.actor_critic_numpy(ac, t, np.float32)
            tol = _tol(v32[cut[k]], v64[cut[k]])
            dv = np.abs(tv[k][cut[k]] - v64[cut[k]]).max()
            # what the pre-update statistics, or no normalisation, would have given
            _, vpre = P.actor_critic_numpy(ac, NR.normalize_obs(raw, before.obs_mean, before.obs_var, 1.0), np.float64)
            _, vraw = P.actor_critic_numpy(ac, raw, np.float64)
            print(f"step {k}: timeout values {tv[k][cut[k]]}, V(normalised terminal obs) {v64[cut[k]]}, |diff| {dv:.3g} "
                  f"tol {tol:.3g}; pre-update statistics would be off by {np.abs(vpre - v64)[cut[k]].max():.3g}, raw by "
                  f"{np.abs(vraw - v64)[cut[k]].max():.3g}")
            assert dv <= tol and np.all(tv[k][cut[k]] != 0)
            assert np.abs(vpre - v64)[cut[k]].max() > tol and np.abs(vraw - v64)[cut[k]].max() > tol
    assert np.all(tv[~cut] == 0)
    a.close(); b.close()


# ------------------------------------------------------------------ frozen statistics
def test_frozen_statistics(tmp_path):
    ac, K = ppo_849(), 6
    src = _warm(_engine(MART, 96, 1), ac, 4, clip_obs=1.0)
    src.collect(4, seed=1, step0=0)
    saved = src.norm_stats()
    saved.save(str(tmp_path / "vecnormalize.npz"))
    src.close()
    loaded = NormStats.load(str(tmp_path / "vecnormalize.npz"))
    assert loaded == saved and loaded.obs_count > 5 * 96                    # _warm's step_wait and collect's four
    outs = []
    for streams in (1, 4, 4):
        e = _warm(_engine(MART, 96, 1), ac, streams, clip_obs=1.0, training=False, stats=loaded)
        before = e.norm_stats()
        assert before == saved
        r = e.collect(K, seed=SEED, step0=40)
        after = e.norm_stats()
        assert np.array_equal(after.record(), before.record())              # bit-equal: nothing was updated
        assert not (_np(r.env_flags) & 3).any() and np.array_equal(after.returns, before.returns)
        outs.append(r)
        # the records are the NumPy expressions under the saved statistics
        assert np.array_equal(_np(r.rewards), NR.normalize_reward(_np(r.raw_rewards), saved.ret_var, 10.0))
        assert np.array_equal(_np(r.obs[K]), NR.normalize_obs(_np(e.obs), saved.obs_mean, saved.obs_var, 1.0))
        e.close()
    for f in NFIELDS:
        assert torch.equal(getattr(outs[0], f), getattr(outs[1], f)), f     # 1 stream == 4 streams
        assert torch.equal(getattr(outs[1], f), getattr(outs[2], f)), f     # a fresh engine reproduces the batch


# ------------------------------------------------------------------ off
def test_off_is_the_engine_that_never_had_it():
    ac = ppo_849()
    a = _warm(_engine(MART, 96, 1), ac, 4, clip_obs=1.0)
    a.collect(2, seed=1, step0=0)
    a.set_normalize(False)
    assert a.normalize is None
    with pytest.raises(RuntimeError, match="normalisation is off"):
        a.norm_obs
    with pytest.raises(RuntimeError, match="normalisation is off"):
        a.norm_stats()
    b = _engine(MART, 96, 1)
    b.set_actor_critic(ac)
    b.reset()
    b.set_state(a.get_state())
    b.obs.copy_(a.obs)
    ra, rb = a.collect(4, seed=SEED, step0=9), b.collect(4, seed=SEED, step0=9)
    assert type(ra) is RolloutBatch and type(rb) is RolloutBatch
    for f in FIELDS:
        assert torch.equal(getattr(ra, f), getattr(rb, f)), f
    # switched on again: fresh statistics
    a.set_normalize()
    assert a.norm_stats() == NormStats.fresh(96)
    a.close(); b.close()


# ------------------------------------------------------------------ reset
def test_a_full_reset_performs_vecnormalize_reset_and_a_masked_one_does_not():
    E, C = 33, 2
    env = _engine(MART, E, C)
    env.set_normalize(clip_obs=1.0)
    out = env.reset()
    raw = _np(env.obs).reshape(-1, 38)
    st = env.norm_stats()
    ref = NR.VecNormalize(E * C, clip_obs=1.0)
    want = ref.reset(raw)
    assert st.obs_count == 1e-4 + E * C and st.ret_count == 1e-4 and not st.returns.any()
    assert out is env.norm_obs and np.array_equal(_np(out).reshape(-1, 38), NR.normalize_obs(raw, st.obs_mean, st.obs_var, 1.0))
    mb, vb = NR.moment_bounds(raw)
    assert np.all(np.abs(st.obs_mean - ref.obs_rms.mean) <= mb) and np.all(np.abs(st.obs_var - ref.obs_rms.var) <= vb)
    assert np.abs(_np(out).reshape(-1, 38) - want).max() <= 1e-6
    mask = torch.zeros(E, dtype=torch.uint8, device="cuda:0")
    mask[3] = 1
    assert env.reset(mask) is env.obs and env.norm_stats() == st
    env.close()


# ------------------------------------------------------------------ error paths
def test_error_paths():
    from nascargymnasium_amd.offpolicy import ReplayBuffer
    env = _engine(MART, 8, 2)
    env.reset()
    with pytest.raises(RuntimeError, match="normalisation is off"):
        env.normalize_step()
    for kw, name in ((dict(clip_obs=0.0), "clip_obs"), (dict(clip_obs=float("nan")), "clip_obs"),
                     (dict(clip_reward=-1.0), "clip_reward"), (dict(clip_reward=float("inf")), "clip_reward"),
                     (dict(epsilon=0.0), "epsilon"), (dict(epsilon=float("nan")), "epsilon"),
                     (dict(gamma=float("inf")), "gamma")):
        with pytest.raises(RuntimeError, match=name):
            env.set_normalize(**kw)
        assert env.normalize is None
    env.set_actor_critic(ppo_849())
    env.set_normalize()
    with pytest.raises(RuntimeError, match="collect_transitions: normalisation is on"):
        env.collect_transitions(ReplayBuffer(env, 2), 1, source=0)
    env.set_rollout_streams(0)
    with pytest.raises(RuntimeError, match="fused rollout kernel has no actor-critic"):
        env.collect(2)
    env.set_rollout_streams(4)
    env.set_rollout_pipe(8)
    with pytest.raises(RuntimeError, match="pipelined rollout has no actor-critic"):
        env.collect(2)
    env.set_rollout_pipe(0)
    # statistics the library itself refuses (NormStats refuses them first on the Python side)
    L, dp = _lib.lib(), ctypes.POINTER(ctypes.c_double)
    for i, v, msg in ((38 + 5, -1e-9, r"obs_var\[5\]"), (78, -1.0, "ret_var"), (76, 0.0, "obs_count"), (79, -2.0, "ret_count"),
                      (3, float("nan"), "not finite")):
        rec = NormStats.fresh().record()
        rec[i] = v
        assert L.nascar_set_norm_stats(env.h, rec.ctypes.data_as(dp), None, None) < 0
        with pytest.raises(RuntimeError, match=msg):
            _lib.check(-1)
    bad = NormStats.fresh(3)
    with pytest.raises(ValueError, match="car slots"):
        env.load_norm_stats(bad)
    plain = RolloutBatch(*[torch.empty((2 + x, *inner), dtype=dt, device="cuda:0") for _n, dt, inner, x in RolloutBatch.spec(8, 2)])
    with pytest.raises(ValueError, match="NormalizedRolloutBatch"):
        env.collect(2, out=plain)
    with pytest.raises(RuntimeError, match="nascar_collect_normalized"):      # the C entry point of the plain batch
        _lib.check(L.nascar_collect(env.h, 0, 0, 1, *[ctypes.c_void_p(t.data_ptr()) for t in
                                                       (plain.obs, plain.rewards, plain.car_flags, plain.env_flags, plain.actions,
                                                        plain.log_probs, plain.values, plain.timeout_values)], None))
    env.normalize_step()
    r = env.collect(2)                                                      # and after all that it still collects
    assert isinstance(r, NormalizedRolloutBatch) and bool(torch.isfinite(r.advantages).all())
    assert env.norm_stats().obs_count == (1e-4 + 16) + 16 + 16
    env.close()

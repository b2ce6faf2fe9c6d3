"""Host side of the running normalisation (no GPU): the NumPy restatement of SB3's RunningMeanStd / VecNormalize
(tests/normalize_ref.py) checked against first principles, the conditions on the inputs tests/test_gpu_normalize.py feeds
the device -- so that those tests cannot pass vacuously -- and the NormStats record."""
import numpy as np
import pytest

import golden_replay as GR
import normalize_ref as NR
from nascargymnasium_amd.normalize import NormStats
from test_onpolicy_cpu import golden_obs


# ------------------------------------------------------------------ the restatement is its own first subject
@pytest.mark.parametrize("sizes", [(185, 185, 185), (1, 31, 129), (33, 1100, 96)])
def test_three_updates_equal_the_moments_of_the_concatenation_plus_the_prior(sizes):
    """RunningMeanStd starts as a pseudo-batch of count 1e-4, mean 0, variance 1; after any updates its state is the
    pooled mean and (population) variance of that pseudo-batch and every row seen:
        tot = 1e-4 + n,  mean = sum x / tot,  var = (1e-4 * (1 + mean^2) + sum (x - mean)^2) / tot
    (the parallel-axis form: no difference of large squares)."""
    obs = golden_obs()
    rms = NR.RunningMeanStd(shape=(38,))
    batches = [NR.batch_rows(obs, n, i) for i, n in enumerate(sizes)]
    for b in batches:
        rms.update(b)
    x = np.concatenate(batches).astype(np.float64)
    tot = 1e-4 + len(x)
    mean = x.sum(axis=0) / tot
    var = (1e-4 * (1.0 + mean * mean) + ((x - mean) ** 2).sum(axis=0)) / tot
    assert rms.count == pytest.approx(tot, rel=1e-15)
    assert np.all(np.abs(rms.mean - mean) <= 1e-12 * np.abs(mean))
    assert np.all(np.abs(rms.var - var) <= 1e-12 * np.abs(var))
    # and the scalar statistic (the returns') takes the same route
    r = NR.RunningMeanStd(shape=())
    cols = [b[:, 2] for b in batches]
    for c in cols:
        r.update(c)
    assert abs(r.mean - mean[2]) <= 1e-12 * abs(mean[2]) and abs(r.var - var[2]) <= 1e-12 * var[2]


def test_step_wait_follows_sb3s_order():
    """the update comes before the normalisation, the terminal rows see the statistics after it, and the returns are
    zeroed after the reward was normalised"""
    obs = golden_obs()
    a, b, t = (NR.batch_rows(obs, 33, i) for i in range(3))
    rew = a[:, 2].copy()
    dones = np.arange(33) % 5 == 0
    vn = NR.VecNormalize(33, clip_obs=1.0)
    n0 = vn.reset(a)
    first = NR.RunningMeanStd(shape=(38,))
    first.update(a)
    assert np.array_equal(n0, NR.normalize_obs(a, first.mean, first.var, 1.0))
    nobs, nrew, nterm = vn.step_wait(b, rew, dones, t)
    first.update(b)
    assert np.array_equal(vn.obs_rms.mean, first.mean) and np.array_equal(vn.obs_rms.var, first.var)
    assert np.array_equal(nobs, NR.normalize_obs(b, first.mean, first.var, 1.0))
    assert np.array_equal(nterm, NR.normalize_obs(t[dones], first.mean, first.var, 1.0))
    ret = NR.RunningMeanStd(shape=())
    ret.update(rew.astype(np.float64))                   # returns were 0: returns = reward
    assert np.array_equal(nrew, NR.normalize_reward(rew, ret.var, 10.0))
    assert np.all(vn.returns[dones] == 0) and np.array_equal(vn.returns[~dones], rew[~dones].astype(np.float64))
    frozen = NR.VecNormalize(33, training=False)
    frozen.step_wait(b, rew, dones, t)
    assert frozen.obs_rms.count == 1e-4 and not frozen.returns.any()


# ------------------------------------------------------------------ conditions on the inputs of the GPU tests
@pytest.mark.parametrize("n", NR.CONDITION_SIZES)
def test_the_gpu_inputs_exercise_clip_epsilon_and_both_variance_scales(n):
    rows = NR.batch_rows(golden_obs(), n)
    rms = NR.RunningMeanStd(shape=(38,))
    rms.update(rows)
    bv = rows.astype(np.float64).var(axis=0)
    assert (bv < 1e-8).any(), "no column whose batch variance is below epsilon"
    assert (bv > 1e-2).any(), "no column whose batch variance is above 1e-2"
    z = (rows.astype(np.float64) - rms.mean) / np.sqrt(rms.var + 1e-8)
    bound = np.abs(z) > 1.0                                                  # a2c.py's clip_obs = 1.0
    assert bound.any() and not bound.all(), "clip_obs = 1.0 binds on all or on no element"
    assert 0.05 < bound.mean() < 0.95
    wide = NR.normalize_obs(rows, rms.mean, rms.var, 10.0)
    assert not np.array_equal(wide, NR.normalize_obs(rows, rms.mean, rms.var, 1.0))
    # without "+ epsilon" the result differs (the near-constant columns): the term is seen
    with np.errstate(divide="ignore", invalid="ignore"):
        bare = np.clip((rows.astype(np.float64) - rms.mean) / np.sqrt(rms.var), -10.0, 10.0).astype(np.float32)
    assert not np.array_equal(bare, wide)
    # the moment bounds of the GPU tests tell a float32 accumulator (what NumPy, hence SB3, uses) from a float64 one
    mb, vb = NR.moment_bounds(rows)
    m32 = rows.mean(axis=0, dtype=np.float32).astype(np.float64)
    assert (np.abs(m32 - rows.astype(np.float64).mean(axis=0)) > mb).sum() > 19
    # the three successive batches differ
    others = [NR.batch_rows(golden_obs(), n, i) for i in (1, 2)]
    assert not np.array_equal(rows, others[0]) and not np.array_equal(others[0], others[1])


def test_the_return_window_contains_a_done():
    d = GR.load(NR.RETURN_FIXTURE)
    first = int(np.flatnonzero(d["terminated"] | d["truncated"])[0])
    assert NR.RETURN_WARM < first < NR.RETURN_WARM + NR.RETURN_K - 1, first       # steps before and after it in the window
    assert not (d["terminated"] | d["truncated"])[:NR.RETURN_WARM].any()
    assert np.all(d["rewards"][NR.RETURN_WARM:first + 1] != 0)                   # the returns move, and so does ret_var


# ------------------------------------------------------------------ NormStats
def _stats(n=7):
    rng = np.random.default_rng(5)
    return NormStats(rng.normal(0, 1, 38), rng.uniform(0, 2, 38), 1234.0001, -0.25, 3.5, 77.0001, rng.normal(0, 1, n))


def test_normstats_npz_round_trip(tmp_path):
    s = _stats()
    for name, path in (("a.npz", tmp_path / "a.npz"), ("bare", tmp_path / "bare")):
        s.save(str(path))
        assert path.exists(), name                                           # the name as given: no suffix appended
        got = NormStats.load(str(path))
        assert got == s and got.obs_mean.dtype == np.float64 and got.returns.dtype == np.float64
    no_ret = NormStats(s.obs_mean, s.obs_var, s.obs_count, s.ret_mean, s.ret_var, s.ret_count)
    no_ret.save(str(tmp_path / "n.npz"))
    assert NormStats.load(str(tmp_path / "n.npz")).returns is None and no_ret != s
    assert NormStats.from_record(s.record(), s.returns) == s and s.record().shape == (80,)
    f = NormStats.fresh(4)
    assert not f.obs_mean.any() and np.all(f.obs_var == 1) and f.obs_count == f.ret_count == 1e-4 and f.ret_var == 1
    assert f.returns.shape == (4,) and not f.returns.any()
    # float32 inputs are taken up as float64 copies
    src = np.ones(38, np.float32)
    c = NormStats(src, src, 1, 0, 1, 1)
    src[0] = 5
    assert c.obs_mean.dtype == np.float64 and c.obs_mean[0] == 1


def test_normstats_validation_errors(tmp_path):
    s = _stats()
    args = [s.obs_mean, s.obs_var, s.obs_count, s.ret_mean, s.ret_var, s.ret_count]

    def bad(i, v, match):
        a = list(args)
        a[i] = v
        with pytest.raises(ValueError, match=match):
            NormStats(*a)
    bad(0, np.zeros(37), "shape")
    bad(1, np.ones((38, 1)), "shape")
    bad(0, np.where(np.arange(38) == 3, np.nan, 0.0), "not finite")
    bad(1, np.where(np.arange(38) == 3, -1e-30, 1.0), "negative")
    bad(4, -1.0, "negative")
    bad(2, 0.0, "count")
    bad(5, -3.0, "count")
    bad(3, np.inf, "not finite")
    with pytest.raises(ValueError, match="not finite"):
        NormStats(*args, returns=[0.0, np.nan])
    with pytest.raises(ValueError, match="80"):
        NormStats.from_record(np.zeros(79))
    np.savez(str(tmp_path / "short.npz"), obs_mean=s.obs_mean)
    with pytest.raises(ValueError, match="obs_var"):
        NormStats.load(str(tmp_path / "short.npz"))
    s.obs_var[0] = -1                                                       # mutated after construction: caught on upload
    with pytest.raises(ValueError, match="negative"):
        s.validate()

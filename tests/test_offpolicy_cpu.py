"""Host side of the off-policy collection (no GPU): the SAC actor loader with its log_std head, SquashedActorNet, the
restated sampler indices, the conditions the GPU value tests rely on (which rows the log_std clamp binds on) and the
host-only controller check (tests/offpolicy_ref.py is the oracle tests/test_gpu_offpolicy.py holds the device to)."""
import io
import math
import os
import zipfile

import numpy as np
import pytest

import offpolicy_ref as R
from nascargymnasium_amd import policy as P

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLAMP_ROW = 1406      # the first golden observation on which sac_1235's log_std exceeds LOG_STD_MAX (printed below)


def golden_obs():
    return np.load(os.path.join(GOLD, "sac_1235_actor.npz"))["obs"]


def sac_1235():
    """the reference's SAC checkpoint as a SquashedActor: the stored actor plus the log_std head fixture"""
    d, h = np.load(os.path.join(GOLD, "sac_1235_actor.npz")), np.load(os.path.join(GOLD, "sac_1235_log_std.npz"))
    w = [d[k.replace(".", "__")] for k in P.ACTOR_KEYS]
    return P.make_squashed_actor(w[:4] + [np.concatenate([w[4], h["weight"]]), np.concatenate([w[5], h["bias"]])], P.RELU, "sac")


def scaled_head_actor():
    """a random 64-64 Tanh squashed actor whose log_std head is scaled (x 300, biases -9 and 30) so that both clamps bind on the
    golden observations -- sac_1235 itself never reaches LOG_STD_MIN there"""
    a = P.random_squashed_actor(64, 64, seed=21, activation=P.TANH)
    w3, b3 = a.w3.copy(), a.b3.copy()
    w3[2:] *= 300
    b3[2:] = b3[2:] * 300 + np.float32([-9, 30])
    return a._replace(w3=w3, b3=b3)


def raw_head(actor, obs, dtype=np.float64):
    """(mu, log_std before the clamp) [n, 2] each"""
    dt = np.dtype(dtype).type
    f = (lambda v: np.maximum(v, dt(0))) if actor.activation == P.RELU else np.tanh
    w1, b1, w2, b2, w3, b3 = [a.astype(dt) for a in actor.arrays]
    h = f(f(np.asarray(obs, dt) @ w1.T + b1) @ w2.T + b2)
    out = h @ w3.T + b3
    return out[:, :2], out[:, 2:]


# ------------------------------------------------------------------ loader
def _write_zip(path, sd):
    torch = pytest.importorskip("torch")
    buf = io.BytesIO()
    torch.save({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, buf)
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("policy.pth", buf.getvalue())
    return str(path)


def _sac_state(actor):
    sd = dict(zip(P.SAC_KEYS, actor.arrays[:4] + (actor.w3[:2], actor.b3[:2])))
    sd.update(zip(P.LOG_STD_KEYS, (actor.w3[2:], actor.b3[2:])))
    sd["critic.qf0.0.weight"] = np.zeros((256, 40), np.float32)
    return sd


def test_loader_round_trip(tmp_path):
    a = P.random_squashed_actor(256, 256, seed=4)
    got = P.load_sb3_sac_actor(_write_zip(tmp_path / "sac.zip", _sac_state(a)))
    assert (got.h1, got.h2, got.activation, got.output, got.kind) == (256, 256, P.RELU, P.OUT_SQUASH_SAMPLE, "sac")
    assert got.w3.shape == (4, 256) and got.b3.shape == (4,)
    for x, y in zip(got.arrays, a.arrays):
        assert x.dtype == np.float32 and np.array_equal(x, y)
    # the mean branch is what the deterministic loaders read from the same zip
    c = P.load_sb3_policy(str(tmp_path / "sac.zip"))
    assert c.output == P.OUT_SQUASH and all(np.array_equal(x, y) for x, y in zip(c.arrays, got.deterministic().arrays))
    w = P.load_sb3_actor(str(tmp_path / "sac.zip"))
    assert np.array_equal(w["actor.mu.weight"], got.w3[:2])


def test_loader_rejects_a_ppo_zip_and_use_sde(tmp_path):
    ac = P.random_actor_critic(64, 64, P.TANH, seed=1)
    sd = dict(zip(P.AC_KEYS + P.VF_KEYS, ac.pi.arrays + ac.vf.arrays))
    sd["log_std"] = ac.log_std
    with pytest.raises(ValueError, match="actor-critic"):
        P.load_sb3_sac_actor(_write_zip(tmp_path / "ppo.zip", sd))
    a = P.random_squashed_actor(256, 256, seed=5)
    sde = {k: v for k, v in _sac_state(a).items() if k not in P.LOG_STD_KEYS}
    sde["actor.log_std"] = np.zeros((256, 2), np.float32)            # gSDE: a parameter, not a layer
    with pytest.raises(ValueError, match="use_sde"):
        P.load_sb3_sac_actor(_write_zip(tmp_path / "sde.zip", sde))
    with pytest.raises(ValueError, match="missing"):
        P.load_sb3_sac_actor(_write_zip(tmp_path / "nohead.zip", {k: v for k, v in _sac_state(a).items()
                                                                  if k not in P.LOG_STD_KEYS}))
    with pytest.raises(ValueError, match="squashed actor shapes"):
        P.make_squashed_actor(a.arrays[:4] + (a.w3[:2], a.b3[:2]))


def test_fixture_is_the_head_of_the_stored_actor():
    a = sac_1235()
    assert (a.h1, a.h2, a.activation) == (256, 256, P.RELU) and a.w3.shape == (4, 256) and a.w3.dtype == np.float32
    z = np.load(os.path.join(GOLD, "sac_1235_log_std.npz"))
    assert sorted(z.files) == ["bias", "weight"] and z["weight"].shape == (2, 256) and z["bias"].shape == (2,)
    assert os.path.getsize(os.path.join(GOLD, "sac_1235_log_std.npz")) < 4096
    # u of a vanishing noise is the deterministic controller's action
    obs = golden_obs()[:64]
    u, s = P.squashed_actor_numpy(a, obs, np.zeros((64, 2)), np.float64)
    assert np.array_equal(u, P.mlp_forward_numpy(a.deterministic(), obs, np.float64))
    assert np.abs(s - u).max() <= 1e-15


# ------------------------------------------------------------------ SquashedActorNet
def test_squashed_actor_net_against_the_float64_restatement():
    torch = pytest.importorskip("torch")
    from nascargymnasium_amd.offpolicy import SquashedActorNet
    a = scaled_head_actor()
    net = SquashedActorNet(a).double()
    assert set(net.state_dict()) == {k[len("actor."):] for k in P.SAC_KEYS + P.LOG_STD_KEYS}
    obs = golden_obs()[:257]
    e = R.eps(257, 1, 2, dtype=np.float64)
    with torch.no_grad():
        act, logp = net.action_log_prob(torch.from_numpy(obs).double(), torch.from_numpy(e))
        det = net(torch.from_numpy(obs).double(), deterministic=True)
    mu, ls = raw_head(a, obs)
    ls = np.clip(ls, -20, 2)
    g = mu + np.exp(ls) * e
    t = np.tanh(g)
    want = (-(g - mu) ** 2 / (2 * np.exp(ls) ** 2) - ls - 0.5 * math.log(2 * math.pi)).sum(1) - np.log(1 - t ** 2 + 1e-6).sum(1)
    assert np.abs(act.numpy() - t).max() <= 1e-12 and np.abs(det.numpy() - np.tanh(mu)).max() <= 1e-12
    assert np.abs(logp.numpy() - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
    u, _ = P.squashed_actor_numpy(a, obs, e, np.float64)
    assert np.abs(u - t).max() <= 1e-15                                 # unscale_action is the identity on Box(-1, 1)
    back = SquashedActorNet(a).export()
    for x, y in zip(back.arrays, a.arrays):
        assert x.dtype == np.float32 and np.array_equal(x, y)
    # an SB3-named state dict loads
    sd = {k[len("actor."):]: torch.from_numpy(v.copy()) for k, v in _sac_state(sac_1235()).items() if k.startswith("actor.")}
    big = SquashedActorNet(P.random_squashed_actor(256, 256, seed=1))
    big.load_state_dict(sd)
    assert all(np.array_equal(x, y) for x, y in zip(big.export().arrays, sac_1235().arrays))


# ------------------------------------------------------------------ draws and indices
def test_explorer_draws_use_salts_of_their_own():
    import onpolicy_ref as OR
    assert len({R.SALT0, R.SALT1, R.SALT_SLOT, R.SALT_CAR, OR.SALT0, OR.SALT1, 0xABCDEF12345, 0x5DEECE66D, 0}) == 9
    e = R.eps(4096, R.TEST_SEED, 3)
    assert e.dtype == np.float32 and np.all(np.isfinite(e)) and not np.array_equal(e, OR.eps(4096, R.TEST_SEED, 3))
    assert np.array_equal(R.eps(5, 3, 9, ids=[7, 8, 9, 10, 11]), R.eps(12, 3, 9)[7:])
    n = e.size
    assert abs(float(e.mean())) <= 5 / math.sqrt(n) and abs(float(e.astype(np.float64).var()) - 1) <= 5 * math.sqrt(2 / n)


def test_sampler_indices_are_in_range_and_uniform():
    size, N, B = 7, 5, 1 << 18
    slot, car = R.sample_indices(B, size, N, seed=3, draw=11)
    assert slot.min() >= 0 and slot.max() == size - 1 and car.min() >= 0 and car.max() == N - 1
    counts = np.bincount(slot * N + car, minlength=size * N)
    p = 1.0 / (size * N)
    mean, sd = B * p, math.sqrt(B * p * (1 - p))
    worst = float(np.abs(counts - mean).max() / sd)
    print(f"pair counts: mean {mean:.1f}, sd {sd:.1f}, worst deviation {worst:.2f} sd")
    assert worst <= 6
    s2, c2 = R.sample_indices(64, size, N, seed=3, draw=12)
    s3, c3 = R.sample_indices(64, size, N, seed=4, draw=11)
    assert not np.array_equal(slot[:64] * N + car[:64], s2 * N + c2) and not np.array_equal(slot[:64] * N + car[:64], s3 * N + c3)
    for sz, n in ((1, 1), (5, 185), (128, 81920)):
        s, c = R.sample_indices(1000, sz, n, 1, 2)
        assert 0 <= s.min() and s.max() < sz and 0 <= c.min() and c.max() < n


def test_clamp_share_of_the_value_tests_inputs():
    """Which rows the log_std clamp binds on.  sac_1235 + its head on the golden observations exceeds LOG_STD_MAX on a
    few rows (the first is CLAMP_ROW: the GPU value tests start their slices there) and never reaches LOG_STD_MIN; the
    scaled-head actor binds both clamps within the first 32 rows of the same slices."""
    obs = golden_obs()
    _, ls = raw_head(sac_1235(), obs)
    hi, lo = (ls > P.LOG_STD_MAX).any(1), (ls < P.LOG_STD_MIN).any(1)
    print(f"sac_1235: log_std in [{ls.min():.3f}, {ls.max():.3f}], rows over the upper clamp {np.flatnonzero(hi)} "
          f"(share {hi.mean():.4f}), under the lower clamp {lo.sum()}")
    assert hi.any() and np.flatnonzero(hi)[0] == CLAMP_ROW and not lo.any()
    _, ls = raw_head(scaled_head_actor(), obs[CLAMP_ROW:CLAMP_ROW + 32])
    hi, lo, mid = (ls > P.LOG_STD_MAX), (ls < P.LOG_STD_MIN), (ls >= P.LOG_STD_MIN) & (ls <= P.LOG_STD_MAX)
    print(f"scaled head, 32 rows: components over {hi.sum()}, under {lo.sum()}, inside {mid.sum()}; row 0: {ls[0]}")
    assert hi.any() and lo.any() and mid.any()
    assert (ls[0] > P.LOG_STD_MAX).any() or (ls[0] < P.LOG_STD_MIN).any()      # the 1 x 1 case clamps too
    # float32 and float64 agree on which side of the clamp every component is (no row sits on the edge)
    _, ls32 = raw_head(scaled_head_actor(), obs[CLAMP_ROW:CLAMP_ROW + 185], np.float32)
    _, ls64 = raw_head(scaled_head_actor(), obs[CLAMP_ROW:CLAMP_ROW + 185])
    assert np.array_equal(ls32 > 2, ls64 > 2) and np.array_equal(ls32 < -20, ls64 < -20)


def test_ring_restates_sb3_add_and_sample():
    ring = R.Ring(3, 2)
    for k in range(4):
        f = np.float32(k)
        ring.add(np.full((2, 38), f), np.full((2, 38), f + 1), np.full((2, 2), f), [f, -f], [k == 1, 0], [k == 1, 0], [1, k != 2])
        assert ring.size == min(k + 1, 3) and ring.pos == (k + 1) % 3
    assert ring.full and ring.obs[0, 0, 0] == 3 and ring.obs[1, 0, 0] == 1
    o, a, no, d, r, live = ring.sample(np.array([1, 1, 2]), np.array([0, 1, 1]))
    assert d.tolist() == [0.0, 0.0, 0.0] and ring.dones[1, 0] == 1          # a timeout is not a termination
    assert r.tolist() == [1.0, -1.0, -2.0] and live.tolist() == [1, 1, 0] and no[0, 0] == 2


# ------------------------------------------------------------------ the host-only controller check
def test_check_controller_on_the_four_row_head():
    from nascargymnasium_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    for h1, h2 in P.MLP_SHAPES:
        _lib.check_controller(P.random_squashed_actor(h1, h2))
    _lib.check_controller(P.random_squashed_actor(64, 64, activation=P.TANH))
    two = P.random_mlp(64, 64, P.RELU, P.OUT_SQUASH)
    with pytest.raises(RuntimeError, match="output 5 .* needs act_dim 4"):
        _lib.check_controller(two._replace(output=P.OUT_SQUASH_SAMPLE))
    four = P.random_squashed_actor(64, 64)
    as_squash = P.Controller(*four.arrays, 64, 64, P.RELU, P.OUT_SQUASH, "x")  # a four-row head with output 2
    with pytest.raises(RuntimeError, match="38 -> 64 -> 64 -> 4"):
        _lib.check_controller(as_squash)
    with pytest.raises(RuntimeError, match="400 -> 300"):
        _lib.check_controller(P.random_squashed_actor(400, 300))
    with pytest.raises(RuntimeError, match="activation"):
        _lib.check_controller(four._replace(activation=2))
    with pytest.raises(RuntimeError, match="output must be"):
        _lib.check_controller(two._replace(output=6))
    from nascargymnasium_amd.offpolicy import BYTES_PER_TRANSITION
    assert BYTES_PER_TRANSITION == 319

"""Host side of the on-policy collection (no GPU): the SB3 actor-critic loader, the critic fixture, the restated draws,
the conditions the GPU value tests rely on, the GAE restatement and ActorCriticNet (tests/onpolicy_ref.py is the oracle
tests/test_gpu_onpolicy.py holds the device to)."""
import io
import json
import math
import os
import zipfile

import numpy as np
import pytest

import onpolicy_ref as R
from nascargymnasium_amd import policy as P

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def ppo_849():
    """the reference's PPO checkpoint as an ActorCritic, from the two fixtures"""
    pi, vf = np.load(os.path.join(GOLD, "ppo_849_actor.npz")), np.load(os.path.join(GOLD, "ppo_849_critic.npz"))
    keys = ("w1", "b1", "w2", "b2", "w3", "b3")
    return P.make_actor_critic([pi[k] for k in keys], [vf[k] for k in keys], int(vf["activation"]), vf["log_std"])


def golden_obs():
    return np.load(os.path.join(GOLD, "sac_1235_actor.npz"))["obs"]


# ------------------------------------------------------------------ loader
def _write_zip(path, ac=None, sd=None, data=None):
    torch = pytest.importorskip("torch")
    if sd is None:
        names = P.AC_KEYS + P.VF_KEYS
        sd = {k: torch.from_numpy(a.copy()) for k, a in zip(names, ac.pi.arrays + ac.vf.arrays)}
        sd["log_std"] = torch.from_numpy(ac.log_std.copy())
        sd["pi_features_extractor.unused"] = torch.zeros(1)
    buf = io.BytesIO()
    torch.save(sd, buf)
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("policy.pth", buf.getvalue())
        if data is not None:
            z.writestr("data", json.dumps(data))
    return str(path)


@pytest.mark.parametrize("act,name", [(P.TANH, None), (P.RELU, "ReLU")])
def test_loader_round_trip(tmp_path, act, name):
    ac = P.random_actor_critic(256, 128, act, log_std=(-0.25, 0.5), seed=3)
    data = None if name is None else {"policy_kwargs": {"activation_fn": f"<class 'torch.nn.modules.activation.{name}'>",
                                                         ":serialized:": "ignored"}}
    got = P.load_sb3_actor_critic(_write_zip(tmp_path / "ac.zip", ac, data=data))
    assert got.pi.activation == act and got.vf.activation == act and got.pi.output == P.OUT_RAW
    assert (got.pi.h1, got.pi.h2, got.vf.h1, got.vf.h2) == (256, 128, 256, 128)
    assert got.vf.w3.shape == (1, 128) and got.vf.b3.shape == (1,)
    for a, b in zip(got.pi.arrays + got.vf.arrays + (got.log_std,), ac.pi.arrays + ac.vf.arrays + (ac.log_std,)):
        assert a.dtype == np.float32 and np.array_equal(a, b)
    # the policy branch is what load_sb3_policy reads, with the raw output
    c = P.load_sb3_policy(str(tmp_path / "ac.zip"))
    assert c.output == P.OUT_CLIP and all(np.array_equal(a, b) for a, b in zip(c.arrays, got.pi.arrays))


def test_loader_rejects_sac_and_unsupported_value_shapes(tmp_path):
    torch = pytest.importorskip("torch")
    sac = {k: torch.from_numpy(v) for k, v in P.random_actor(1).items()}
    with pytest.raises(ValueError, match="SAC"):
        P.load_sb3_actor_critic(_write_zip(tmp_path / "sac.zip", sd=sac))
    ac = P.random_actor_critic(64, 64, P.TANH, seed=1)
    rng = np.random.default_rng(0)
    bad = [rng.uniform(-1, 1, s).astype(np.float32) for s in ((96, 38), (96,), (64, 96), (64,), (1, 64), (1,))]
    with pytest.raises(ValueError, match="38 -> 96 -> 64 -> 1"):
        P.make_value_net(bad, P.TANH)
    names = P.AC_KEYS + P.VF_KEYS
    sd = {k: torch.from_numpy(a.copy()) for k, a in zip(names, ac.pi.arrays + tuple(bad))}
    sd["log_std"] = torch.zeros(2)
    with pytest.raises(ValueError, match="38 -> 96 -> 64 -> 1"):
        P.load_sb3_actor_critic(_write_zip(tmp_path / "odd.zip", sd=sd))
    with pytest.raises(ValueError, match="log_std"):
        P.make_actor_critic(ac.pi.arrays, ac.vf.arrays, P.TANH, [0.0, float("nan")])


# ------------------------------------------------------------------ fixture
def test_critic_fixture_float32_within_the_rule_of_float64():
    ac, obs = ppo_849(), golden_obs()
    z = np.load(os.path.join(GOLD, "ppo_849_critic.npz"))
    assert z["value_f64"].shape == (2236,) and z["value_f32"].dtype == np.float32
    assert (ac.vf.h1, ac.vf.h2, ac.vf.activation) == (64, 64, P.TANH)
    assert np.allclose(ac.log_std, (-0.18, -0.48), atol=0.01)
    mu64, v64 = P.actor_critic_numpy(ac, obs, np.float64)
    mu32, v32 = P.actor_critic_numpy(ac, obs, np.float32)
    assert np.abs(v64 - z["value_f64"]).max() <= 1e-12 * np.abs(v64).max()      # the fixture is this net's float64 value
    tol = max(8 * np.abs(v32.astype(np.float64) - v64).max(), 1e-6)             # the project's rule (test_gpu_policy_shapes)
    d = np.abs(z["value_f32"].astype(np.float64) - z["value_f64"]).max()
    print(f"fixture max |f32 - f64| {d:.3g}, tol {tol:.3g}")
    assert d <= tol
    pi = np.load(os.path.join(GOLD, "ppo_849_actor.npz"))
    assert np.abs(mu64 - pi["mean_f64"]).max() <= 1e-12 and mu32.dtype == np.float32


# ------------------------------------------------------------------ draws
def test_draws_are_standard_normal_and_u0_is_never_zero():
    cars, steps = 1024, 64                                                      # 65 536 (car, step) keys
    e = np.concatenate([R.eps(cars, R.TEST_SEED, s) for s in range(steps)])
    k0 = np.concatenate([R.uniforms(cars, R.TEST_SEED, s)[0] for s in range(steps)])
    u0 = (k0 + 1).astype(np.float32) * np.float32(2.0 ** -24)
    assert u0.min() > 0 and u0.max() <= 1 and np.all(np.isfinite(e)) and e.dtype == np.float32
    n = e.size
    assert n == 131072
    mean, var = float(e.astype(np.float64).mean()), float(e.astype(np.float64).var())
    print(f"mean {mean:.4g} (bound {5 / math.sqrt(n):.4g}), var {var:.5g} (bound 1 +- {5 * math.sqrt(2 / n):.4g})")
    assert abs(mean) <= 5 / math.sqrt(n)
    assert abs(var - 1) <= 5 * math.sqrt(2 / n)
    # the extreme inputs: u0 = 2^-24 gives the largest radius, finite; u0 = 1 gives 0
    assert np.sqrt(np.float32(-2) * np.log(np.float32(2.0 ** -24))) < 6 and np.log(np.float32(1)) == 0
    # a car's draw depends on (seed, car, step) only
    assert np.array_equal(R.eps(5, 3, 9, ids=[7, 8, 9, 10, 11]), R.eps(12, 3, 9)[7:])
    assert not np.array_equal(R.eps(8, 3, 9), R.eps(8, 3, 10)) and not np.array_equal(R.eps(8, 3, 9), R.eps(8, 4, 9))


def test_clip_share_of_the_value_tests_inputs():
    """ppo_849 on the golden observations at the GPU tests' seed: the clip acts on some components and not on others"""
    ac, obs = ppo_849(), golden_obs()
    mu, _ = P.actor_critic_numpy(ac, obs, np.float64)
    a, clipped, _ = R.sample(mu, ac.log_std, R.eps(len(obs), R.TEST_SEED, 0, dtype=np.float64), np.float64)
    share = float((np.abs(a) > 1).mean())
    print(f"clipped share {share:.3f}")
    assert share >= 0.10 and 1 - share >= 0.10
    assert np.array_equal(clipped, np.clip(a, -1, 1))


# ------------------------------------------------------------------ GAE
def _hand_case():
    """5 steps, 2 cars: a termination at step 1 of car 0, a timeout (done with a bootstrap value) at step 2 of car 1"""
    f = np.float32
    rewards = np.array([[0.1, -0.2], [1.3, 0.4], [-0.7, 0.9], [0.25, -1.1], [0.6, 0.3]], f)
    values = np.array([[0.5, 0.7], [0.9, -0.3], [0.2, 1.1], [-0.4, 0.8], [0.3, 0.6], [1.2, -0.9]], f)
    tv = np.zeros((5, 2), f)
    tv[2, 1] = 1.7
    done = np.zeros((5, 2), bool)
    done[1, 0] = done[2, 1] = True
    return rewards, values, tv, done


def test_gae_restatement_equals_the_scalar_loop_and_float32_is_observable():
    rewards, values, tv, done = _hand_case()
    g, lam = 0.99, 0.95
    a64, r64 = R.gae(rewards, values, tv, done, g, lam, np.float64)
    sa, sr = R.gae_scalar(rewards, values, tv, done, g, lam)
    assert np.array_equal(a64, sa) and np.array_equal(r64, sr)
    # by hand: the last step, and the step of the timeout (no bootstrap from the next value, gamma * V(terminal) added)
    assert a64[4, 0] == float(rewards[4, 0]) + g * float(values[5, 0]) - float(values[4, 0])
    assert a64[2, 1] == (float(rewards[2, 1]) + g * float(tv[2, 1])) - float(values[2, 1])
    assert a64[1, 0] == float(rewards[1, 0]) - float(values[1, 0])
    a32, r32 = R.gae(rewards, values, tv, done, g, lam, np.float32)
    assert a32.dtype == np.float32 and r32.dtype == np.float32
    assert np.abs(a32 - a64).max() <= 1e-5
    assert not np.array_equal(a32.astype(np.float64), a64)                      # the float32 order is observable
    assert np.array_equal(r32, a32 + values[:5])


# ------------------------------------------------------------------ ActorCriticNet
def test_actor_critic_net_evaluates_like_the_restatement():
    torch = pytest.importorskip("torch")
    from nascargymnasium_amd.onpolicy import ActorCriticNet, RolloutBatch
    ac = P.random_actor_critic(64, 64, P.TANH, log_std=(-0.2, 0.3), seed=5, vf_shape=(256, 128), vf_activation=P.RELU)
    net = ActorCriticNet(ac).double()
    assert set(P.AC_KEYS + P.VF_KEYS + ("log_std",)) == set(net.state_dict())
    obs = golden_obs()[:257]
    mu, v = P.actor_critic_numpy(ac, obs, np.float64)
    a, _, lp = R.sample(mu, ac.log_std, R.eps(len(obs), 1, 2, dtype=np.float64), np.float64)
    with torch.no_grad():
        values, logp, ent = net.evaluate_actions(torch.from_numpy(obs).double(), torch.from_numpy(a))
    assert tuple(values.shape) == (257, 1) and tuple(logp.shape) == (257,) and tuple(ent.shape) == (257,)
    assert np.abs(values.numpy()[:, 0] - v).max() <= 1e-12
    assert np.abs(logp.numpy() - lp).max() <= 1e-12
    want_ent = float(np.sum(0.5 + 0.5 * math.log(2 * math.pi) + ac.log_std.astype(np.float64)))
    assert np.abs(ent.numpy() - want_ent).max() <= 1e-12
    back = ActorCriticNet(ac).export()
    for x, y in zip(back.pi.arrays + back.vf.arrays + (back.log_std,), ac.pi.arrays + ac.vf.arrays + (ac.log_std,)):
        assert x.dtype == np.float32 and np.array_equal(x, y)
    # RolloutBatch: flatten views and seeded minibatches
    K, E, C = 3, 4, 2
    rb = RolloutBatch(*[torch.arange((K + extra) * int(np.prod(inner))).reshape(K + extra, *inner).to(dt)
                        for _n, dt, inner, extra in RolloutBatch.spec(E, C)])
    flat = rb.flatten()
    assert tuple(flat.obs.shape) == (24, 38) and tuple(flat.actions.shape) == (24, 2) and tuple(flat.values.shape) == (24,)
    assert flat.values.data_ptr() == rb.values.data_ptr()
    mb = list(rb.minibatches(5, seed=1))
    assert [len(m.returns) for m in mb] == [5, 5, 5, 5, 4]
    assert sorted(torch.cat([m.returns for m in mb]).tolist()) == flat.returns.tolist()
    assert all(torch.equal(x.returns, y.returns) for x, y in zip(mb, rb.minibatches(5, seed=1)))

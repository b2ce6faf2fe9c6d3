"""Host side of the categorical actor-critic and of the wide nets (no GPU): the Discrete(5) loader, the torch module, the
host-only controller check, and the conditions the GPU tests rely on, checked on the oracle alone (tests/discrete_ref.py
is the oracle tests/test_gpu_discrete.py holds the device to)."""
import io
import os
import zipfile

import numpy as np
import pytest

import discrete_ref as D
import onpolicy_ref as R
from nascargymnasium_amd import policy as P
from test_onpolicy_cpu import golden_obs

STEP = 3                                    # the step of the GPU value tests
N_CARS = 645                                # the cars the conditions are stated for: golden_obs()[100:745]


def scaled(ac, k=8.0):
    """the head's w3 scaled so that the distribution is not flat"""
    return ac._replace(pi=ac.pi._replace(w3=(ac.pi.w3 * np.float32(k)).astype(np.float32)))


def net_64():
    return scaled(P.random_discrete_actor_critic(64, 64, P.TANH, seed=11))


def net_split():
    """pi 64-64 Tanh and vf 256-128 ReLU: two shapes, so two launches"""
    return scaled(P.random_discrete_actor_critic(64, 64, P.TANH, seed=11, vf_shape=(256, 128), vf_activation=P.RELU))


def net_512():
    return scaled(P.random_discrete_actor_critic(512, 512, P.RELU, seed=11))


NETS = {"64": net_64, "split": net_split, "512": net_512}


# ------------------------------------------------------------------ loaders
def _write_zip(path, sd):
    torch = pytest.importorskip("torch")
    buf = io.BytesIO()
    torch.save({k: torch.from_numpy(np.ascontiguousarray(v).copy()) for k, v in sd.items()}, buf)
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("policy.pth", buf.getvalue())
    return str(path)


def _state_dict(ac):
    sd = dict(zip(P.AC_KEYS + P.VF_KEYS, ac.pi.arrays + ac.vf.arrays))
    if hasattr(ac, "log_std"):
        sd["log_std"] = ac.log_std
    return sd


def test_discrete_loader_round_trip_and_the_two_loaders_refuse_each_other(tmp_path):
    ac = P.random_discrete_actor_critic(256, 128, P.TANH, seed=3)
    got = P.load_sb3_discrete_actor_critic(_write_zip(tmp_path / "d.zip", _state_dict(ac)))
    assert got.pi.output == P.OUT_CATEGORICAL and got.pi.activation == P.TANH and not hasattr(got, "log_std")
    assert got.pi.w3.shape == (5, 128) and got.pi.b3.shape == (5,) and got.vf.w3.shape == (1, 128)
    for a, b in zip(got.pi.arrays + got.vf.arrays, ac.pi.arrays + ac.vf.arrays):
        assert a.dtype == np.float32 and np.array_equal(a, b)
    assert got.deterministic().output == P.OUT_MODE and got.deterministic().w3 is got.pi.w3
    box = P.random_actor_critic(64, 64, P.TANH, seed=1)
    with pytest.raises(ValueError, match="load_sb3_actor_critic"):
        P.load_sb3_discrete_actor_critic(_write_zip(tmp_path / "box.zip", _state_dict(box)))
    with pytest.raises(ValueError, match="load_sb3_discrete_actor_critic"):
        P.load_sb3_actor_critic(str(tmp_path / "d.zip"))
    with pytest.raises(ValueError, match="5 logits"):
        P.make_controller(box.pi.arrays, P.TANH, P.OUT_MODE)
    with pytest.raises(ValueError, match="2 actions"):
        P.make_controller(ac.pi.arrays, P.TANH, P.OUT_CLIP)
    wide = P.random_discrete_actor_critic(512, 512, P.RELU, seed=2)
    assert (wide.vf.h1, wide.vf.h2) == (512, 512) and (512, 512) in P.WIDE_SHAPES and (512, 512) not in P.MLP_SHAPES
    with pytest.raises(ValueError, match="38 -> 512 -> 512 -> 1 .Tanh"):
        P.random_discrete_actor_critic(512, 512, P.TANH, seed=2)
    assert P.random_actor_critic(512, 512, P.RELU, seed=2).vf.h2 == 512        # the Gaussian record takes the wide shape too


# ------------------------------------------------------------------ CategoricalActorCriticNet
def test_categorical_net_evaluates_like_torch_categorical_and_round_trips():
    torch = pytest.importorskip("torch")
    from nascargymnasium_amd.onpolicy import (CategoricalActorCriticNet, DiscreteRolloutBatch,
                                               NormalizedDiscreteRolloutBatch, RolloutBatch)
    ac = net_split()
    net = CategoricalActorCriticNet(ac).double()
    assert set(P.AC_KEYS + P.VF_KEYS) == set(net.state_dict())
    assert tuple(net.action_net.weight.shape) == (5, 64)
    obs = golden_obs()[:257]
    logits, v = P.discrete_actor_critic_numpy(ac, obs, np.float64)
    a, lp, _ = D.sample(logits, D.uniform(len(obs), 1, 2), np.float64)
    with torch.no_grad():
        values, logp, ent = net.evaluate_actions(torch.from_numpy(obs).double(), torch.from_numpy(a))
        dist = torch.distributions.Categorical(logits=torch.from_numpy(logits))
        want_lp, want_ent = dist.log_prob(torch.from_numpy(a)), dist.entropy()
    assert tuple(values.shape) == (257, 1) and tuple(logp.shape) == (257,) and tuple(ent.shape) == (257,)
    assert np.abs(values.numpy()[:, 0] - v).max() <= 1e-12
    assert (logp - want_lp).abs().max() <= 1e-12 and (ent - want_ent).abs().max() <= 1e-12
    assert np.abs(logp.numpy() - lp).max() <= 1e-12                       # the oracle's logp is Categorical's
    assert np.abs(D.logp_of(logits, a) - lp).max() == 0
    back = CategoricalActorCriticNet(ac).export()
    assert back.pi.output == P.OUT_CATEGORICAL and back.vf.activation == P.RELU
    for x, y in zip(back.pi.arrays + back.vf.arrays, ac.pi.arrays + ac.vf.arrays):
        assert x.dtype == np.float32 and np.array_equal(x, y)
    # the batch kinds: int32 actions [K, E, C], flatten / minibatches as RolloutBatch's
    K, E, C = 3, 4, 2
    spec = DiscreteRolloutBatch.spec(E, C)
    assert [s for s in spec if s[0] != "actions"] == [s for s in RolloutBatch.spec(E, C) if s[0] != "actions"]
    assert spec[1] == ("actions", torch.int32, (E, C), 0)
    assert NormalizedDiscreteRolloutBatch.spec(E, C)[-1][0] == "raw_rewards"
    rb = DiscreteRolloutBatch(*[torch.arange((K + extra) * int(np.prod(inner))).reshape(K + extra, *inner).to(dt)
                                for _n, dt, inner, extra in spec])
    flat = rb.flatten()
    assert tuple(flat.obs.shape) == (24, 38) and tuple(flat.actions.shape) == (24,) and flat.actions.dtype == torch.int32
    assert rb.steps == 3 and [len(m.actions) for m in rb.minibatches(5, seed=1)] == [5, 5, 5, 5, 4]


# ------------------------------------------------------------------ the host-only controller check
def test_check_controller_on_the_five_row_head_and_the_wide_shape():
    from nascargymnasium_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    for h1, h2 in P.MLP_SHAPES:
        for act in (P.RELU, P.TANH):
            ac = P.random_discrete_actor_critic(h1, h2, act, seed=1)
            _lib.check_controller(ac.pi)
            _lib.check_controller(ac.deterministic())
    wide = P.random_discrete_actor_critic(512, 512, P.RELU, seed=1)
    _lib.check_controller(wide.pi)
    _lib.check_controller(wide.deterministic())
    _lib.check_controller(wide.vf)                                           # the 512-512 value net
    gauss = P.random_actor_critic(512, 512, P.RELU, seed=1)
    _lib.check_controller(gauss.pi._replace(output=P.OUT_SAMPLE))           # ... and the Gaussian actor
    for out in (P.OUT_RAW, P.OUT_CLIP, P.OUT_SQUASH):
        _lib.check_controller(gauss.pi._replace(output=out))
    with pytest.raises(RuntimeError, match="38 -> 512 -> 512 -> 5 with Tanh"):
        _lib.check_controller(wide.pi._replace(activation=P.TANH))
    with pytest.raises(RuntimeError, match="38 -> 512 -> 512 -> 2 with Tanh"):
        _lib.check_controller(gauss.pi._replace(activation=P.TANH))
    with pytest.raises(RuntimeError, match="38 -> 512 -> 512 -> 4.*no explorer head"):
        _lib.check_controller(P.random_squashed_actor(512, 512))
    with pytest.raises(RuntimeError, match="38 -> 512 -> 256 -> 5 unsupported"):
        _lib.check_controller(P.random_discrete_actor_critic(64, 64, seed=1).pi._replace(h1=512, h2=256))
    five = P.random_discrete_actor_critic(64, 64, P.TANH, seed=1).pi
    for out in range(6):
        with pytest.raises(RuntimeError, match=f"output {out} takes no five-row head"):
            _lib.check_controller(five._replace(output=out))
    two = P.random_mlp(64, 64, P.TANH, P.OUT_CLIP)
    for out, name in ((P.OUT_CATEGORICAL, "sample"), (P.OUT_MODE, "mode")):
        with pytest.raises(RuntimeError, match=f"output must be .* output {out} .categorical {name}. needs act_dim 5"):
            _lib.check_controller(two._replace(output=out))
    with pytest.raises(RuntimeError, match="output must be .* got 8"):
        _lib.check_controller(five._replace(output=8))


# ------------------------------------------------------------------ the draw
def test_the_uniform_is_the_salted_counter_draw():
    assert D.CAT_SALT not in (R.SALT0, R.SALT1, 0xABCDEF12345, 0x5DEECE66D, 0)
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nascar.h")).read()
    assert "0x%X" % D.CAT_SALT in hdr
    u = np.concatenate([D.uniform(1024, R.TEST_SEED, s) for s in range(64)])
    assert u.min() >= 0 and u.max() < 1 and np.array_equal(u, u.astype(np.float32))
    n = u.size
    assert abs(u.mean() - 0.5) <= 5 * np.sqrt(1 / 12 / n) and abs(u.var() - 1 / 12) <= 5 * np.sqrt(1 / 180 / n)
    assert np.array_equal(D.uniform(5, 3, 9, ids=[7, 8, 9, 10, 11]), D.uniform(12, 3, 9)[7:])
    assert not np.array_equal(D.uniform(8, 3, 9), D.uniform(8, 3, 10)) and not np.array_equal(D.uniform(8, 3, 9), D.uniform(8, 4, 9))
    # by hand: three categories of equal weight, two of none (their thresholds are passed together)
    l = np.array([[0.0, 0.0, -1e9, -1e9, 0.0]] * 3)
    a, lp, pn = D.sample(l, np.array([0.0, 0.5, 0.9]), np.float64)
    assert a.tolist() == [0, 1, 4] and np.allclose(lp, np.log(1 / 3)) and np.allclose(pn[0], [1 / 3, 2 / 3, 2 / 3, 2 / 3])
    assert D.mode(np.array([[1.0, 3.0, 3.0, 2.0, 0.0]])).tolist() == [1]


@pytest.mark.parametrize("net", ["64", "512"])
def test_conditions_on_the_gpu_tests_inputs(net):
    """on golden_obs()[100:745] at the GPU tests' seed and step: almost no car's u lies at a boundary of its distribution,
    float32 NumPy picks the float64 index everywhere else, and every category is drawn"""
    ac = NETS[net]()
    rows = golden_obs()[100:100 + N_CARS]
    l64, _ = P.discrete_actor_critic_numpy(ac, rows, np.float64)
    l32, _ = P.discrete_actor_critic_numpy(ac, rows, np.float32)
    u = D.uniform(N_CARS, R.TEST_SEED, STEP)
    margin, inb = D.band(l32, l64, u)
    a64, _, _ = D.sample(l64, u, np.float64)
    a32, _, _ = D.sample(l32, u.astype(np.float32), np.float32)
    counts = np.bincount(a64, minlength=5)
    print(f"net {net}: margin {margin:.3g}, {int(inb.sum())} of {N_CARS} cars in the band, category counts {counts.tolist()}")
    assert inb.mean() <= 0.01
    assert np.array_equal(a32[~inb], a64[~inb])
    assert counts.min() >= 10

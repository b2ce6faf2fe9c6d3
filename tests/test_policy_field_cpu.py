"""Per-car controllers, host side (no GPU): the SB3 checkpoint loader (nascargymnasium_amd.policy.load_sb3_policy) on
synthetic zips, the host-only shape validator behind add_controller, and the numpy forward against the committed
PPO / A2C fixtures (tools/gen_policy_fixtures.py: the reference's ppo_849 and a2c_best_model3 policy branches with
PyTorch float64 / float32 action means on the 2236 observations of sac_1235_actor.npz)."""
import io
import json
import os
import zipfile

import numpy as np
import pytest

from golden_replay import GOLDEN

torch = pytest.importorskip("torch")

from nascargymnasium_amd import policy as P   # noqa: E402


def _write_zip(path, state_dict, data=None):
    buf = io.BytesIO()
    torch.save({k: torch.from_numpy(v) for k, v in state_dict.items()}, buf)
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("policy.pth", buf.getvalue())
        if data is not None:
            z.writestr("data", json.dumps(data))
    return str(path)


def _ac_state(h1, h2, seed):
    c = P.random_mlp(h1, h2, seed=seed)
    sd = dict(zip(P.AC_KEYS, c.arrays))
    rng = np.random.default_rng(seed)
    sd["log_std"] = np.zeros(2, np.float32)   # what an ActorCriticPolicy state dict holds besides the policy branch
    sd["mlp_extractor.value_net.0.weight"] = rng.normal(size=(h1, 38)).astype(np.float32)
    sd["value_net.weight"] = rng.normal(size=(1, h2)).astype(np.float32)
    return c, sd


def fixture_controller(name):
    d = np.load(os.path.join(GOLDEN, name + "_actor.npz"))
    c = P.make_controller([d[k] for k in ("w1", "b1", "w2", "b2", "w3", "b3")], int(d["activation"]), int(d["output"]),
                          "actor_critic")
    assert (c.h1, c.h2) == (int(d["h1"]), int(d["h2"]))
    return c, d["mean_f64"], d["mean_f32"]


def golden_obs():
    return np.load(os.path.join(GOLDEN, "sac_1235_actor.npz"))["obs"]


def test_loader_sac_zip(tmp_path):
    w = P.random_actor(3)
    w["critic.qf0.0.weight"] = np.zeros((256, 40), np.float32)
    c = P.load_sb3_policy(_write_zip(tmp_path / "sac.zip", w, {"policy_kwargs": {"use_sde": False}}))
    assert (c.kind, c.h1, c.h2, c.activation, c.output) == ("sac", 256, 256, P.RELU, P.OUT_SQUASH)
    for a, k in zip(c.arrays, P.ACTOR_KEYS):
        assert a.dtype == np.float32 and np.array_equal(a, w[k])


def test_loader_actor_critic_default_is_tanh(tmp_path):
    want, sd = _ac_state(64, 64, 1)
    # `data` without policy_kwargs, and one whose policy_kwargs holds nothing but a serialized blob: both SB3's default
    for i, data in enumerate([{}, {"policy_kwargs": {":type:": "<class 'dict'>", ":serialized:": "gASV"}}, None]):
        c = P.load_sb3_policy(_write_zip(tmp_path / f"ppo{i}.zip", sd, data))
        assert (c.kind, c.h1, c.h2, c.activation, c.output) == ("actor_critic", 64, 64, P.TANH, P.OUT_CLIP)
        assert all(np.array_equal(a, b) for a, b in zip(c.arrays, want.arrays))


def test_loader_actor_critic_relu(tmp_path):
    want, sd = _ac_state(256, 128, 2)
    data = {"policy_kwargs": {":type:": "<class 'dict'>", ":serialized:": "not base64, never decoded",
                              "net_arch": [256, 128], "activation_fn": "<class 'torch.nn.modules.activation.ReLU'>"}}
    c = P.load_sb3_policy(_write_zip(tmp_path / "a2c.zip", sd, data))
    assert (c.kind, c.h1, c.h2, c.activation, c.output) == ("actor_critic", 256, 128, P.RELU, P.OUT_CLIP)
    assert all(np.array_equal(a, b) for a, b in zip(c.arrays, want.arrays))
    data["policy_kwargs"]["activation_fn"] = "<class 'torch.nn.modules.activation.ELU'>"
    with pytest.raises(ValueError, match="neither ReLU nor Tanh"):
        P.load_sb3_policy(_write_zip(tmp_path / "elu.zip", sd, data))


def test_loader_unknown_keys(tmp_path):
    sd = {"q_net.0.weight": np.zeros((64, 38), np.float32), "q_net.0.bias": np.zeros(64, np.float32)}
    with pytest.raises(ValueError, match="neither an SB3 SAC actor"):
        P.load_sb3_policy(_write_zip(tmp_path / "dqn.zip", sd, {}))
    _, ac = _ac_state(64, 64, 0)
    del ac["action_net.bias"]
    with pytest.raises(ValueError):
        P.load_sb3_policy(_write_zip(tmp_path / "partial.zip", ac, {}))


def test_td3_shape_loads_but_the_validator_rejects_it(tmp_path):
    """SB3's TD3 default [400, 300] is a well-formed MLP (the loader takes it) that the kernels do not hold: the
    host-only nascar_check_controller, add_controller's shape check, names the shape."""
    from nascargymnasium_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    _, sd = _ac_state(400, 300, 4)
    c = P.load_sb3_policy(_write_zip(tmp_path / "td3ish.zip", sd, {}))
    assert (c.h1, c.h2) == (400, 300)
    with pytest.raises(RuntimeError, match=r"38 -> 400 -> 300 -> 2"):
        _lib.check_controller(c)
    for h1, h2 in [(256, 256), (64, 64), (256, 128), (128, 128), (32, 256), (256, 32)]:
        _lib.check_controller(P.random_mlp(h1, h2, P.TANH, P.OUT_CLIP))
    for h1, h2 in [(64, 32), (288, 256), (256, 96), (48, 48)]:
        with pytest.raises(RuntimeError, match=f"{h1} -> {h2}"):
            _lib.check_controller(P.random_mlp(h1, h2))
    with pytest.raises(RuntimeError, match="activation"):
        _lib.check_controller(P.random_mlp(64, 64)._replace(activation=2))
    with pytest.raises(RuntimeError, match="output"):
        _lib.check_controller(P.random_mlp(64, 64)._replace(output=3))


@pytest.mark.parametrize("name,h,act", [("ppo_849", (64, 64), P.TANH), ("a2c_best_model3", (256, 128), P.RELU)])
def test_numpy_forward_matches_the_fixture(name, h, act):
    c, m64, m32 = fixture_controller(name)
    assert (c.h1, c.h2) == h and c.activation == act and c.output == P.OUT_CLIP
    x = golden_obs()
    assert m64.shape == (len(x), 2) and m64.dtype == np.float64 and m32.dtype == np.float32
    got64 = P.mlp_forward_numpy(c, x, np.float64, output=P.OUT_RAW)
    assert np.abs(got64 - m64).max() <= 1e-12, np.abs(got64 - m64).max()
    tol = 8 * np.abs(m32.astype(np.float64) - m64).max()
    got32 = P.mlp_forward_numpy(c, x, np.float32, output=P.OUT_RAW)
    assert got32.dtype == np.float32
    print(name, "numpy f32 vs mean_f64", np.abs(got32 - m64).max(), "tol", tol)
    assert np.abs(got32 - m64).max() <= tol
    assert np.array_equal(P.mlp_forward_numpy(c, x, np.float64), np.clip(got64, -1, 1))


def test_fixture_files_hold_the_policy_branch_only():
    for name, cap in [("ppo_849", 100 << 10), ("a2c_best_model3", 260 << 10)]:
        path = os.path.join(GOLDEN, name + "_actor.npz")
        d = np.load(path)
        assert sorted(d.files) == sorted(["w1", "b1", "w2", "b2", "w3", "b3", "h1", "h2", "activation", "output",
                                          "mean_f64", "mean_f32"])
        assert os.path.getsize(path) < cap

"""Per-car controllers on the device (policy 4, "the field"; csrc/nascar_actor.h mlp_field_kernel): every SB3
checkpoint kind the reference ships -- SAC 256-256 ReLU squashed, PPO 64-64 Tanh clipped, A2C 256-128 ReLU clipped --
through controller_forward, mixed in one env with the built-in sources through policy_actions(4), and in the sharded
rollout.

Tolerance of the float32 kernel against a float64 forward, per fixture: tol = 8 x max |mean_f32 - mean_f64| of the
fixture's own PyTorch float32 / float64 means (about 1.6e-5 for ppo_849, pre-clip range +-4, and 8.8e-5 for
a2c_best_model3, range -45 .. 38); the factor 8 covers the MFMA's summation order and device tanhf against PyTorch's.
"""
import os

import numpy as np
import pytest

from golden_replay import GOLDEN, TRACKS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from nascargymnasium_amd import policy as P   # noqa: E402


def _fixture(name):
    d = np.load(os.path.join(GOLDEN, name + "_actor.npz"))
    c = P.make_controller([d[k] for k in ("w1", "b1", "w2", "b2", "w3", "b3")], int(d["activation"]), int(d["output"]),
                          "actor_critic")
    return c, d["mean_f64"], d["mean_f32"]


def _sac_1235():
    d = np.load(os.path.join(GOLDEN, "sac_1235_actor.npz"))
    w = {k: d[k.replace(".", "__")] for k in P.ACTOR_KEYS}
    return P.make_controller([w[k] for k in P.ACTOR_KEYS], P.RELU, P.OUT_SQUASH, "sac"), w


@pytest.fixture(scope="module")
def obs():
    return np.load(os.path.join(GOLDEN, "sac_1235_actor.npz"))["obs"]


@pytest.fixture(scope="module")
def env1():
    """one small env whose handle holds the controllers of the forward tests (raw and clip variants of both fixtures)"""
    from nascargymnasium_amd.batched import BatchedCarEnv
    env = BatchedCarEnv(1, 1, "martinsville", device="cuda:0")
    ids = {}
    for name in ("ppo_849", "a2c_best_model3"):
        c = _fixture(name)[0]
        ids[name, "clip"] = env.add_controller(c)
        ids[name, "raw"] = env.add_controller(c._replace(output=P.OUT_RAW))
    env.ids = ids
    yield env
    env.close()


def _engine(tracks, E, C, **kw):
    from nascargymnasium_amd.batched import BatchedCarEnv
    files = [os.path.join(TRACKS, tracks[e * len(tracks) // E]) for e in range(E)]
    return BatchedCarEnv(E, C, files if len(tracks) > 1 else files[0], device="cuda:0", **kw)


@pytest.mark.parametrize("n", [2236, 37, 1])
@pytest.mark.parametrize("name", ["ppo_849", "a2c_best_model3"])
def test_raw_forward_matches_float64(env1, obs, name, n):
    _, m64, m32 = _fixture(name)
    tol = 8 * np.abs(m32.astype(np.float64) - m64).max()
    got = env1.controller_forward(env1.ids[name, "raw"], torch.from_numpy(obs[:n]).cuda()).cpu().numpy()
    assert got.shape == (n, 2) and got.dtype == np.float32 and np.all(np.isfinite(got))
    d = np.abs(got.astype(np.float64) - m64[:n])
    print(name, n, "max |kernel - mean_f64|", d.max(), "tol", tol)
    assert d.max() <= tol, (d.max(), tol)


@pytest.mark.parametrize("name", ["ppo_849", "a2c_best_model3"])
def test_clip_is_the_clipped_raw_mean(env1, obs, name):
    """clip mode == np.clip(raw, -1, 1) exactly.  Only ~2 % of A2C's clipped components (and 16 % of PPO's throttle) lie
    inside (-1, 1) on these observations, so the raw mean of EVERY row is compared too: a clipped-only comparison would
    hide errors."""
    _, m64, m32 = _fixture(name)
    x = torch.from_numpy(obs).cuda()
    raw = env1.controller_forward(env1.ids[name, "raw"], x).cpu().numpy()
    clip = env1.controller_forward(env1.ids[name, "clip"], x).cpu().numpy()
    assert np.array_equal(clip, np.clip(raw, np.float32(-1), np.float32(1)))
    d = np.abs(raw.astype(np.float64) - m64)
    assert d.shape == (len(obs), 2) == m64.shape and len(obs) == 2236      # the raw comparison covers all rows
    assert d.max() <= 8 * np.abs(m32.astype(np.float64) - m64).max()
    inside = (np.abs(m64) < 1).mean(0)
    if name == "ppo_849":
        assert inside[1] > 0.9          # PPO's steering is inside the box for ~95 % of the rows
    else:
        assert inside.max() < 0.05


@pytest.mark.parametrize("h1,h2", [(64, 64), (32, 256), (256, 32)])
def test_tanh_random_weights(obs, h1, h2):
    c = P.random_mlp(h1, h2, P.TANH, P.OUT_RAW, seed=h1 + h2)
    ref = P.mlp_forward_numpy(c, obs, np.float64)
    tol = max(8 * np.abs(P.mlp_forward_numpy(c, obs, np.float32).astype(np.float64) - ref).max(), 1e-6)
    from nascargymnasium_amd.batched import BatchedCarEnv
    env = BatchedCarEnv(1, 1, "martinsville", device="cuda:0")     # its own handle: 16 controllers per handle
    got = env.controller_forward(env.add_controller(c), torch.from_numpy(obs).cuda()).cpu().numpy()
    env.close()
    d = np.abs(got.astype(np.float64) - ref)
    print((h1, h2), "max |kernel - f64|", d.max(), "tol", tol)
    assert got.shape == ref.shape and d.max() <= tol, (d.max(), tol)


def test_field_actions_per_slot():
    """E = 37, C = 5: [sac_1235, ppo_849, rule, a2c, uniform].  Each slot's column of policy_actions(4) is bitwise its
    own source's: controller_forward on that slot's observations, policy 0's column for the uniform slot, and -- cars
    do not interact and nothing resets within 20 steps -- slot 2 of a second env driven by policy 1 throughout."""
    E, C, seed = 37, 5, 11
    a, b = _engine(["martinsville.track"], E, C), _engine(["martinsville.track"], E, C)
    ids = [a.add_controller(_sac_1235()[0]), a.add_controller(_fixture("ppo_849")[0]), "rule",
           a.add_controller(_fixture("a2c_best_model3")[0]), "uniform"]
    a.set_car_controllers(ids)
    a.reset(); b.reset()
    for k in range(21):
        act = a.policy_actions(4, seed=seed, step=k).clone()
        for c in (0, 1, 3):
            assert torch.equal(act[:, c], a.controller_forward(ids[c], a.obs[:, c])), (k, c)
        assert torch.equal(act[:, 4], a.policy_actions(0, seed=seed, step=k).clone()[:, 4]), k
        act_b = b.policy_actions(1, seed=seed, step=k).clone()
        assert torch.equal(act[:, 2], act_b[:, 2]), k
        assert torch.equal(a.obs[:, 2], b.obs[:, 2]), k
        a.step(act); b.step(act_b)
        assert int((a.env_flags & 8).sum()) == 0
    assert float(act[:, 2].abs().max()) > 0 and not torch.equal(act[:, 0], act[:, 1])
    a.close(); b.close()


@pytest.mark.parametrize("tracks,E,streams", [(["martinsville.track"], 96, 4), (["martinsville.track"], 96, 1),
                                              (["martinsville.track", "daytona.track"], 48, 4)])
def test_field_rollout_equals_per_step(tracks, E, streams):
    """rollout(4, 40) == 40 x (policy_actions(4, seed, step0 + k) + step(auto_reset=True)), bit for bit: 96 envs in 4
    shards of 24 (ragged tiles at env0 = 0, 24, 48, 72), one shard, and two tracks (non-identity block map: one shard)."""
    C, K, seed, step0 = 4, 40, 3, 100
    a, b = _engine(tracks, E, C), _engine(tracks, E, C)
    b.set_rollout_streams(streams)
    for e in (a, b):
        e.set_car_controllers([e.add_controller(_sac_1235()[0]), "rule", e.add_controller(_fixture("ppo_849")[0]), "noisy"])
    a.reset()
    b.set_state(a.get_state())
    b.obs.copy_(a.obs)
    O, R, CF, EF = [], [], [], []
    for k in range(K):
        a.launch_step(a.policy_actions(4, seed=seed, step=step0 + k), auto_reset=True)
        O.append(a.obs.clone()); R.append(a.reward.clone()); CF.append(a.car_flags.clone()); EF.append(a.env_flags.clone())
    Ob, Rb, CFb, EFb = b.rollout(4, K, seed=seed, step0=step0, auto_reset=True, trajectory=True, obs_trajectory=True)
    torch.cuda.synchronize()
    for k in range(K):
        assert torch.equal(O[k], Ob[k + 1]), f"obs differs at step {k}"
        assert torch.equal(R[k], Rb[k]), f"reward differs at step {k}"
        assert torch.equal(CF[k], CFb[k]) and torch.equal(EF[k], EFb[k]), f"flags differ at step {k}"
    assert torch.equal(a.obs, b.obs)
    assert torch.equal(a.get_state(), b.get_state())      # the rule driver's control state included
    a.close(); b.close()


def test_field_error_paths():
    env = _engine(["martinsville.track"], 4, 2)
    env.reset()
    with pytest.raises(RuntimeError, match="controller table"):
        env.policy_actions(4)                                   # no table
    with pytest.raises(RuntimeError, match="controller table"):
        env.rollout(4, 3)
    cid = env.add_controller(P.random_mlp(64, 64, P.TANH, P.OUT_CLIP))
    with pytest.raises(RuntimeError, match="unknown controller id 5"):
        env.set_car_controllers([cid, 5])                       # an id nobody returned
    with pytest.raises(RuntimeError, match="unknown controller id -4"):
        env.set_car_controllers([cid, -4])
    with pytest.raises(RuntimeError, match="400 -> 300"):
        env.add_controller(P.random_mlp(400, 300))              # TD3's default: no kernel
    env.set_car_controllers([cid, "rule"])
    with pytest.raises(RuntimeError, match="policy 4"):
        env.step_driven(4)
    env.set_rollout_streams(0)
    with pytest.raises(RuntimeError, match="policy 4"):
        env.rollout(4, 3)                                       # the fused rollout kernel has no controllers
    env.set_rollout_streams(2)
    env.set_rollout_pipe(64)                                    # the pipe setting falls back to the streams schedule
    _, rew, _, _ = env.rollout(4, 3)
    env.set_rollout_pipe(0)
    obs, rew, _, _ = env.step(env.policy_actions(4))            # the env still steps
    torch.cuda.synchronize()
    assert torch.isfinite(obs).all() and torch.isfinite(rew).all()
    env.set_car_controllers(None)
    with pytest.raises(RuntimeError, match="controller table"):
        env.policy_actions(4)
    env.close()


def test_all_sac_field_equals_policy_2():
    """sac_1235 through add_controller in all 4 slots == the same checkpoint through set_actor(precision="fp32") and
    policy 2: <8, 8, ReLU> with the squash output performs actor_mfma32_kernel's operations in its order."""
    E, C = 64, 4
    env = _engine(["martinsville.track"], E, C)
    ctrl, w = _sac_1235()
    env.set_actor(w, precision="fp32")
    cid = env.add_controller(ctrl)
    env.set_car_controllers([cid] * C)
    env.reset()
    for k in range(10):
        a4 = env.policy_actions(4).clone()
        a2 = env.policy_actions(2).clone()
        assert torch.equal(a4, a2), k
        assert torch.equal(a4, env.actor_forward(env.obs)), k
        env.step(a4, auto_reset=True)
    env.close()

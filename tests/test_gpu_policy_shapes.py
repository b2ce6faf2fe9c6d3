"""The policy-inference kernels of csrc/nascar_actor.h at the shapes the other files leave out (cases:
tests/policy_cases.py; what they reach is checked on the host by tests/test_policy_cases_cpu.py).

A  actor_kernel (bf16, persistent) with 1-2 and 2-3 tiles per wave: the steady-state loop, its prefetch of the next
   tile, the uneven workgroup ranges and a ragged last tile inside a multi-tile wave.  A row's arithmetic does not
   depend on its tile, wave or lane (every MFMA column is computed on its own in a fixed k order), so the big batch
   must equal, bit for bit, the rows of one 4096-row forward -- the regime tests/test_gpu_actor.py verifies -- and any
   difference is a scheduling or prefetch bug.  Also against that file's references at that file's tolerances.
B  all 12 mlp_field_kernel instantiations at n around one wave's tile and one workgroup, against float64.
C  the clip and squash epilogues on nets whose raw means straddle and far exceed +-1.
D  launch_field with several different controllers of one shape in one launch, ids that differ from their slots.
E  a second set_actor on one handle, the 16-controller cap, empty batches.

Tolerances: bf16 actor vs the float64 emulation of its operand rounding 2e-4, f32 actor vs the PyTorch f32 forward 1e-5
(tests/test_gpu_actor.py); controllers vs float64 max(8 x max |numpy_f32 - f64|, 1e-6) per net and output, computed from
the references alone (tests/test_gpu_field.py).
"""
import numpy as np
import pytest

import policy_cases as PC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from nascargymnasium_amd import policy as P                              # noqa: E402
from test_gpu_actor import _obs_batch, _ref_bf16, _ref_fp32               # noqa: E402
from test_gpu_field import _engine                                        # noqa: E402

ACTOR_SEED = 5


def _env1():
    from nascargymnasium_amd.batched import BatchedCarEnv
    return BatchedCarEnv(1, 1, "martinsville", device="cuda:0")


def _forward(env, x):
    return env.actor_forward(torch.from_numpy(x).cuda()).cpu().numpy()


# ------------------------------------------------------------------ A: the persistent actor's multi-tile regime
@pytest.fixture(scope="module")
def actor_base():
    """the 4096-row block, its one-tile-per-wave forwards at both precisions and the two references (computed once)"""
    w = P.random_actor(ACTOR_SEED)
    x = _obs_batch(PC.BASE_ROWS, ACTOR_SEED)
    assert x.shape == (PC.BASE_ROWS, 38)
    env = _env1()
    env.set_actor(w, precision="bf16")
    out_bf16 = _forward(env, x)
    env.set_actor(w, precision="fp32")
    out_fp32 = _forward(env, x)
    env.close()
    ref_bf16, ref_fp32 = _ref_bf16(w, x), _ref_fp32(w, x)
    assert np.abs(out_bf16 - ref_bf16).max() <= 2e-4 and np.abs(out_fp32 - ref_fp32).max() <= 1e-5   # the known regime
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return dict(w=w, x=x, bf16=out_bf16, fp32=out_fp32, ref_bf16=ref_bf16, ref_fp32=ref_fp32, cus=cus)


@pytest.mark.parametrize("which", ["n_a", "n_b"])
def test_bf16_actor_multi_tile_waves(actor_base, which):
    b = actor_base
    n = PC.big_batch_sizes(b["cus"])[which == "n_b"]
    G, counts = PC.actor_tile_plan(n, b["cus"])
    assert counts.max() >= (2 if which == "n_a" else 3)                 # the loop runs again on this device
    idx = PC.big_batch_index(n)
    env = _env1()
    env.set_actor(b["w"], precision="bf16")
    got = _forward(env, b["x"][idx])
    env.close()
    assert got.shape == (n, 2) and np.all(np.isfinite(got))
    bad = np.flatnonzero((got != b["bf16"][idx]).any(1))
    assert bad.size == 0, (f"{bad.size} rows differ from the 4096-row forward; first rows {bad[:8]}, tiles "
                           f"{np.unique(bad // 32)[:8]} (grid {G}, tiles per wave {counts.min()}..{counts.max()})")
    d = np.abs(got - b["ref_bf16"][idx]).max()                          # the reference is row-wise: gathered, not redone
    print(f"bf16 actor {which} = {n} rows, grid {G}, {counts.min()}..{counts.max()} tiles per wave: "
          f"max |kernel - bf16 emulation| {d:.3g} (tol 2e-4)")
    assert d <= 2e-4


def test_fp32_actor_at_the_big_batch(actor_base):
    b = actor_base
    n = PC.big_batch_sizes(b["cus"])[0]
    idx = PC.big_batch_index(n)
    env = _env1()
    env.set_actor(b["w"], precision="fp32")
    got = _forward(env, b["x"][idx])
    env.close()
    d = np.abs(got - b["ref_fp32"][idx]).max()
    print(f"fp32 actor n_a = {n} rows: max |kernel - torch f32 forward| {d:.3g} (tol 1e-5)")
    assert got.shape == (n, 2) and d <= 1e-5
    assert np.array_equal(got, b["fp32"][idx])


def test_policy_2_bf16_at_the_big_batch(actor_base):
    """the bf16 kernel through the path a rollout uses, at the README's scale: E = ceil(n_a / 10) envs of 10 cars"""
    from nascargymnasium_amd.batched import BatchedCarEnv
    b = actor_base
    n_a = PC.big_batch_sizes(b["cus"])[0]
    E, C = (n_a + 9) // 10, 10
    idx = PC.big_batch_index(E * C)                                     # its first n_a rows are the n_a batch
    x = torch.from_numpy(b["x"][idx]).cuda()
    env = BatchedCarEnv(E, C, "daytona", device="cuda:0")
    env.set_actor(b["w"], precision="bf16")
    env.obs.copy_(x.reshape(E, C, 38))
    a2 = env.policy_actions(2).clone()
    fwd = env.actor_forward(x)
    env.close()
    assert PC.actor_tile_plan(E * C, b["cus"])[1].max() >= 2
    assert torch.equal(a2.reshape(E * C, 2), fwd)
    assert np.array_equal(fwd.cpu().numpy(), b["bf16"][idx])


# ------------------------------------------------------------------ B: every mlp_field_kernel instantiation
@pytest.fixture(scope="module")
def obs():
    return PC.fixture_obs()


@pytest.fixture(scope="module")
def env12():
    """one handle with the 12 raw nets"""
    env = _env1()
    nets = PC.all_nets()
    env.ids = {key: env.add_controller(c) for key, c in nets.items()}
    env.nets = nets
    yield env
    env.close()


def _tol(ctrl, x, ref, output=None):
    return max(8 * np.abs(P.mlp_forward_numpy(ctrl, x, np.float32, output).astype(np.float64) - ref).max(), 1e-6)


@pytest.mark.parametrize("h1,h2,act", PC.NETS)
def test_every_instantiation_matches_float64(env12, obs, h1, h2, act):
    c = env12.nets[h1, h2, act]
    ref = P.mlp_forward_numpy(c, obs, np.float64)
    tol = _tol(c, obs, ref)
    worst = 0.0
    for n in PC.FORWARD_SIZES:
        got = env12.controller_forward(env12.ids[h1, h2, act], torch.from_numpy(obs[:n]).cuda()).cpu().numpy()
        assert got.shape == (n, 2) and got.dtype == np.float32 and np.all(np.isfinite(got))
        d = np.abs(got.astype(np.float64) - ref[:n]).max()
        worst = max(worst, d)
        assert d <= tol, (n, d, tol)
    print(f"<{h1 // 32}, {h2 // 32}, {'ReLU' if act == P.RELU else 'Tanh'}> max |kernel - f64| {worst:.3g} tol {tol:.3g}")


# ------------------------------------------------------------------ C: output transforms that bite
@pytest.mark.parametrize("h1,h2,act", PC.NETS)
def test_clip_and_squash_bite(obs, h1, h2, act):
    c1 = PC.standardised(PC.all_nets()[h1, h2, act], obs, 1.0)
    c40 = PC.standardised(PC.all_nets()[h1, h2, act], obs, 40.0)
    env = _env1()
    x = torch.from_numpy(obs).cuda()

    def run(c, output):
        return env.controller_forward(env.add_controller(c._replace(output=output)), x).cpu().numpy()
    raw1, clip1, sq1 = run(c1, P.OUT_RAW), run(c1, P.OUT_CLIP), run(c1, P.OUT_SQUASH)
    clip40, sq40 = run(c40, P.OUT_CLIP), run(c40, P.OUT_SQUASH)
    env.close()
    one = np.float32(1)
    # k = 1: half of every component inside (-1, 1)
    mu1 = P.mlp_forward_numpy(c1, obs, np.float64, P.OUT_RAW)
    assert np.abs(raw1.astype(np.float64) - mu1).max() <= _tol(c1, obs, mu1, P.OUT_RAW)
    assert np.array_equal(clip1, np.clip(raw1, -one, one))
    assert (np.abs(clip1) == 1).mean() > 0.3 and (np.abs(clip1) < 1).mean() > 0.3      # the clip acted, and not everywhere
    ref_sq = P.mlp_forward_numpy(c1, obs, np.float64, P.OUT_SQUASH)
    tol_sq = _tol(c1, obs, ref_sq, P.OUT_SQUASH)
    d_sq = np.abs(sq1.astype(np.float64) - ref_sq).max()
    print(f"<{h1 // 32}, {h2 // 32}, {act}> squash max |kernel - f64| {d_sq:.3g} tol {tol_sq:.3g}")
    assert d_sq <= tol_sq, (d_sq, tol_sq)
    assert np.all(np.abs(sq1) <= 1)
    # k = 40: most rows saturate
    mu40 = P.mlp_forward_numpy(c40, obs, np.float64, P.OUT_RAW)
    tol40 = _tol(c40, obs, mu40, P.OUT_RAW)
    assert np.all(np.isfinite(sq40)) and np.all(np.isfinite(clip40))
    assert np.all(np.abs(sq40) <= 1) and np.all(np.abs(clip40) <= 1)
    far = np.abs(mu40) >= 10                                            # f32 tanh is 1 from about 9.01
    assert far.mean() >= 0.5
    assert np.array_equal(sq40[far], np.sign(mu40[far]).astype(np.float32))
    out = np.abs(mu40) >= 1 + tol40
    assert out.mean() >= 0.5
    assert np.array_equal(clip40[out], np.sign(mu40[out]).astype(np.float32))


# ------------------------------------------------------------------ D: grouped launches
def _field_pair(E, C, slots, ctrls, obs_rows):
    """(a, b): a with the field installed, b a twin for the whole-batch built-in policies; both with the same obs"""
    a, b = _engine(["martinsville.track"], E, C), _engine(["martinsville.track"], E, C)
    ids = [a.add_controller(c) for c in ctrls]
    assert ids == list(range(len(ctrls)))
    a.set_car_controllers(slots)
    a.reset(); b.reset()
    x = torch.from_numpy(obs_rows).cuda().reshape(E, C, 38)
    a.obs.copy_(x); b.obs.copy_(x)
    return a, b


@pytest.mark.parametrize("reverse", [False, True])
def test_grouped_launches_tell_their_controllers_apart(obs, reverse):
    E, C, seed, step = 37, 10, 11, 4
    slots, ctrls = PC.grouped_field()
    if reverse:
        slots = slots[::-1]
    a, b = _field_pair(E, C, slots, ctrls, obs[:E * C])
    act = a.policy_actions(4, seed=seed, step=step).clone()
    net = [c for c in range(C) if not isinstance(slots[c], str)]
    assert len(net) == 8 and all(slots[c] != c for c in net)
    for c in net:
        want = a.controller_forward(slots[c], a.obs[:, c])
        assert torch.equal(act[:, c], want), f"slot {c} (controller {slots[c]}) is not its controller's forward"
        ref = P.mlp_forward_numpy(ctrls[slots[c]], obs[:E * C].reshape(E, C, 38)[:, c], np.float64)
        assert np.abs(want.cpu().numpy() - ref).max() <= _tol(ctrls[slots[c]], obs[:E * C].reshape(E, C, 38)[:, c], ref)
    c_rule, c_uni = slots.index("rule"), slots.index("uniform")
    assert torch.equal(act[:, c_rule], b.policy_actions(1, seed=seed, step=step).clone()[:, c_rule])
    assert torch.equal(act[:, c_uni], b.policy_actions(0, seed=seed, step=step).clone()[:, c_uni])
    for i, c in enumerate(net):
        for d in net[i + 1:]:
            assert not torch.equal(act[:, c], act[:, d]), (c, d)
    a.close(); b.close()


def test_grouped_field_rollout_equals_per_step():
    """the bounded grouped field on 96 envs in 4 shards of 24 (ragged tiles at env0 = 0, 24, 48, 72):
    rollout(4, 20) == 20 x (policy_actions(4) + launch_step), bit for bit"""
    E, C, K, seed, step0 = 96, 10, 20, 3, 100
    slots, ctrls = PC.grouped_field(bounded=True)
    a, b = _engine(["martinsville.track"], E, C), _engine(["martinsville.track"], E, C)
    b.set_rollout_streams(4)
    for e in (a, b):
        for c in ctrls:
            e.add_controller(c)
        e.set_car_controllers(slots)
    a.reset()
    b.set_state(a.get_state())
    b.obs.copy_(a.obs)
    O, R, CF, EF = [], [], [], []
    for k in range(K):
        act = a.policy_actions(4, seed=seed, step=step0 + k)
        assert float(act.abs().max()) <= 1.0
        a.launch_step(act, auto_reset=True)
        O.append(a.obs.clone()); R.append(a.reward.clone()); CF.append(a.car_flags.clone()); EF.append(a.env_flags.clone())
    Ob, Rb, CFb, EFb = b.rollout(4, K, seed=seed, step0=step0, auto_reset=True, trajectory=True, obs_trajectory=True)
    torch.cuda.synchronize()
    for k in range(K):
        assert torch.equal(O[k], Ob[k + 1]), f"obs differs at step {k}"
        assert torch.equal(R[k], Rb[k]), f"reward differs at step {k}"
        assert torch.equal(CF[k], CFb[k]) and torch.equal(EF[k], EFb[k]), f"flags differ at step {k}"
    assert torch.equal(a.get_state(), b.get_state())
    a.close(); b.close()


# ------------------------------------------------------------------ E: housekeeping
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_second_set_actor_takes_effect(obs, precision):
    w0, w1 = P.random_actor(21), P.random_actor(22)
    x = torch.from_numpy(obs[:129]).cuda()
    env = _env1()
    env.set_actor(w0, precision=precision)
    first = env.actor_forward(x).clone()
    env.set_actor(w1, precision=precision)
    second = env.actor_forward(x).clone()
    env.close()
    fresh = _env1()
    fresh.set_actor(w1, precision=precision)
    want = fresh.actor_forward(x).clone()
    fresh.close()
    assert torch.equal(second, want)
    assert float((second - first).abs().max()) > 1e-3


def test_seventeenth_controller_is_refused(obs):
    env = _env1()
    x = torch.from_numpy(obs[:33]).cuda()
    nets = [P.random_mlp(64, 64, P.TANH, P.OUT_RAW, seed=500 + i) for i in range(17)]
    ids = [env.add_controller(c) for c in nets[:16]]
    assert ids == list(range(16))
    before = [env.controller_forward(i, x).clone() for i in (0, 15)]
    with pytest.raises(RuntimeError, match="at most 16 controllers"):
        env.add_controller(nets[16])
    for i, want in zip((0, 15), before):
        got = env.controller_forward(i, x)
        assert torch.equal(got, want)
        ref = P.mlp_forward_numpy(nets[i], obs[:33], np.float64)
        assert np.abs(got.cpu().numpy() - ref).max() <= _tol(nets[i], obs[:33], ref)
    env.close()


def test_empty_batches():
    env = _env1()
    cid = env.add_controller(P.random_mlp(64, 64, P.TANH, P.OUT_CLIP))
    empty = torch.empty((0, 38), dtype=torch.float32, device="cuda:0")
    out = env.controller_forward(cid, empty)
    assert tuple(out.shape) == (0, 2) and out.dtype == torch.float32
    for precision in ("bf16", "fp32"):
        env.set_actor(P.random_actor(1), precision=precision)
        out = env.actor_forward(empty)
        assert tuple(out.shape) == (0, 2) and out.dtype == torch.float32
    torch.cuda.synchronize()
    env.close()

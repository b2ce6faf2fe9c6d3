"""Single-step parity of the WHOLE device state against the oracle.

Each case set of tests/state_cases.py (what the sets reach is pinned on the oracle by tests/test_state_cases_cpu.py)
is loaded into a BatchedCarEnv with set_state and into an OracleEnv with inject_gpu_state, both take one step with the
set's actions (or reset the set's mask), and everything the step wrote is compared: all float32 and int32 per-car
fields, the acceleration ring, the env's time and words, the listener's keys and first normals, every contact record
(wall, flags, manifold, both accumulated impulses, toi, toiCount -- all 20 words, slot by slot: both engines keep the
b2Contact list in the same order, so no keyed comparison is needed) and every float64 field bit for bit, except `slip`
(ocml atan2 against glibc's) and `lfm` (sqrt for CPython's ** 0.5).  `lfm` must lie within 1 ulp of the oracle's
value; `slip` is measured at up to 2 ulp, so its 1-ulp bound stands as test_slip_within_one_ulp (expected to fail,
strictly) and every comparison holds it to the 3 ulp a 1-ulp atan2 allows (compare_state).  After ONE step from a
shared state those two are the only fields a last-bit library difference has reached, so everything else is held to
equality, and a difference names the field and the case it came from.  Every test prints the share of cars whose
slip / lfm differ at all and the largest distance (pytest -s); DESIGN 3.3 quotes them.  The step's own
outputs (obs, reward, flags, reason) are compared too.  The engine's driver-state section stays as nascar_create made
it.  Layouts: C = 1, 3 or 10 at one env per workgroup and at the fullest layout (state_cases.LAYOUTS).

The teacher-forced tests do the same along a trajectory: at every step the device's state is injected into the oracle
and both step once, so nothing accumulates (a few thousand realistic transitions, with wall contacts on the crowded
scene).  The float64 library functions themselves are pinned where the model uses them through nascar_debug_f64math.

Scratch-build check: with one token changed in csrc/nascar_kernels.hip these tests failed as follows (and passed
again without it):
  * `c.stuck_dur > 10.0` -> `>=` (logic_run): all four test_one_step[stuck-*] -- `disabled`, `cum_reward` and the
    env words of the 87 cars whose stuck_dur + dt is exactly 10.0;
  * `c.acc_head = h0 + 1 < 10 ? ...` -> `< 9` (the ring's wrap, car_update_physics): all four test_one_step[ring-*]
    and both [weight_transfer-*] -- `acc_head` of the cars with a full ring and the head in slot 8;
  * `c.cum_reward < -250.0f` -> `c.cum_reward + rew < -250.0f` (the termination's test after instead of before the
    update): all four test_one_step[termination*] -- the reason / terminated words of 220 envs.
"""
import ctypes

import numpy as np
import pytest

import crowded
import state_cases as S
from gpu_state import F32, F64, I32
from oracle_lib import GPU_MAXC, OracleEnv, gpu_arena, inject_gpu_state, oracle_arena
from state_cases import f64i, i32i

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ULP_FIELDS = ("slip", "lfm")
CASES = [(name, C, epb) for name, C in S.SETS for epb in S.LAYOUTS[C]]
_shares = {}


def _engine(c, epb):
    from nascargymnasium_amd.batched import BatchedCarEnv
    env = BatchedCarEnv(c.E, c.C, c.path, reset_on_lap=c.reset_on_lap, device="cuda:0", envs_per_block=epb)
    assert env.envs_per_block == epb
    return env


def _load(env, blob, E, C):
    """the sections of `blob` into the engine, its own driver-state section kept"""
    own = env.get_state().cpu().numpy().copy()
    assert own.shape == blob.shape
    dst, src = gpu_arena(own, E, C), gpu_arena(blob, E, C)
    for k in dst:
        if k != "ctl":
            dst[k][...] = src[k]
    env.set_state(torch.from_numpy(own).to(env.device))


def ulps(a, b):
    """distance in units in the last place between float64 arrays (finite, same sign or zero)"""
    ia, ib = (np.ascontiguousarray(x, np.float64).view(np.int64) for x in (a, b))
    ia, ib = (np.where(i < 0, np.int64(-2 ** 63) - i, i) for i in (ia, ib))
    return np.abs(ia - ib)


SLIP_BOUND = 3      # see compare_state


def compare_state(what, G, O, C):
    """Device sections G against oracle sections O: every difference is collected and reported together.  Returns
    {field: (share of cars differing, max ulp)} of ULP_FIELDS.  `lfm` must lie within 1 ulp.  `slip` is held here to
    SLIP_BOUND = 3 ulp, which is what a 1-ulp atan2 allows: slip = |sr| * (180 / pi) is rounded again, so two angles
    one ulp apart (relative distance up to 2^-52, i.e. up to 2 ulp of the product) give products up to 2 + 2 * 1/2
    ulp apart; the 1-ulp bound DESIGN used to state for it is test_slip_within_one_ulp's."""
    errs = []

    def bits(x):
        return np.ascontiguousarray(x).view(np.uint32 if x.dtype.itemsize == 4 else np.uint64)

    def same(label, g, o, axis_car):
        bad = np.argwhere(bits(g) != bits(o))
        if len(bad):
            errs.append(f"{label} differs for {len(np.unique(bad[:, axis_car]))} cars / envs, first at {bad[0].tolist()}: "
                        f"device {g[tuple(bad[0])]!r} oracle {o[tuple(bad[0])]!r}")
    for k, f in enumerate(F32):
        same(f"f32 field `{f}`", G["f32"][k:k + 1], O["f32"][k:k + 1], 1)
    for k, f in enumerate(I32):
        same(f"i32 field `{f}`", G["i32"][k:k + 1], O["i32"][k:k + 1], 1)
    out = {}
    for k, f in enumerate(F64):
        if f in ULP_FIELDS:
            d = ulps(G["f64"][k], O["f64"][k])
            out[f] = (float((d != 0).mean()), int(d.max()))
            bad = np.flatnonzero(d > (SLIP_BOUND if f == "slip" else 1))
            if len(bad):
                errs.append(f"`{f}` is {int(d.max())} ulp from the oracle's (car {bad[0]}: device "
                            f"{float(G['f64'][k, bad[0]]).hex()} oracle {float(O['f64'][k, bad[0]]).hex()})")
        else:
            same(f"f64 field `{f}`", G["f64"][k:k + 1], O["f64"][k:k + 1], 1)
    same("the acceleration ring", G["acc"], O["acc"], 1)
    same("the env time", G["time"][None], O["time"][None], 1)
    same("the env words (created, pending, reason, terminated, truncated)", G["ei32"], O["ei32"], 1)
    nct, nact = O["i32"][i32i["nct"]], O["i32"][i32i["nact"]]
    assert nct.max() <= GPU_MAXC and nact.max() <= GPU_MAXC
    live = (np.arange(GPU_MAXC)[None, :] < nct[:, None]).repeat(20, 1)
    same("the contact records (20 words each)", np.where(live, G["ct"], 0), np.where(live, O["ct"], 0), 0)
    act = np.arange(GPU_MAXC)[None, :] < nact[:, None]
    same("the listener keys", np.where(act, G["key"], 0), np.where(act, O["key"], 0), 0)
    same("the listener normals", np.where(act.repeat(2, 1), G["n"], 0), np.where(act.repeat(2, 1), O["n"], 0), 0)
    assert not errs, f"{what}: " + "; ".join(errs)
    return out


def compare_outputs(what, env, obs, rew, cf, ef):
    go, gr = env.obs.cpu().numpy(), env.reward.cpu().numpy()
    gcf, gef = env.car_flags.cpu().numpy(), env.env_flags.cpu().numpy()
    bad = np.argwhere(go.view(np.uint32) != obs.view(np.uint32))
    assert len(bad) == 0, f"{what}: obs differ at {bad[:5].tolist()}"
    bad = np.argwhere(gr.view(np.uint32) != rew.view(np.uint32))
    assert len(bad) == 0, f"{what}: rewards differ at {bad[:5].tolist()}: {gr[tuple(bad[0])]} vs {rew[tuple(bad[0])]}"
    assert np.array_equal(gcf & 5, cf & 5), f"{what}: disabled / collision flags"
    assert np.array_equal(gef & 1, ef[:, 0]) and np.array_equal((gef >> 1) & 1, ef[:, 1]), f"{what}: done flags"
    assert np.array_equal((gef >> 4) & 7, ef[:, 2]), f"{what}: termination reasons"


@pytest.mark.parametrize("name,C,epb", CASES)
def test_one_step(name, C, epb):
    """one step (for the reset_dirty sets: one reset(mask)) of every case set, in every layout"""
    c = S.build(name, C)
    O, obs, rew, cf, ef = S.oracle_step(name, C)
    env = _engine(c, epb)
    _load(env, c.blob, c.E, C)
    if c.mask is not None:
        env.reset(torch.from_numpy(c.mask.copy()).to(env.device))
    else:
        env.step(torch.from_numpy(c.actions.copy()).to(env.device))
    G = gpu_arena(env.get_state().cpu().numpy(), c.E, C)
    what = f"{name} {c.E} x {C} at {epb} envs per workgroup"
    try:
        sh = compare_state(what, G, O, C)
        if c.mask is None:
            compare_outputs(what, env, obs, rew, cf, ef)
        else:
            m = c.mask != 0
            assert np.array_equal(env.obs.cpu().numpy()[m].view(np.uint32), obs[m].view(np.uint32)), f"{what}: reset obs"
    finally:
        env.close()
    _shares[name, C, epb] = sh
    print(f"{what}: " + ", ".join(f"{f} differs for {100 * s:.3f} % of the cars, at most {m} ulp" for f, (s, m) in sh.items()))


@pytest.mark.xfail(strict=True, reason="measured: slip is up to 2 ulp from the oracle's, for 6 - 26 % of the cars")
def test_slip_within_one_ulp():
    """The bound DESIGN 3.3 used to state for `slip`.  It does not hold, and cannot with a 1-ulp atan2: ocml's atan2
    is within 1 ulp of glibc's (test_f64_atan2_of_the_slip_angle; 10.1 % of the points differ), but slip = |sr| *
    (180 / pi) rounds once more, which turns some 1-ulp angles into 2-ulp products.  Measured on an MI355X, ROCm 7.2
    against glibc 2.35: at most 2 ulp in every case set and in both teacher-forced runs (72 000 transitions); the cars
    differing at all are 6.5 % (stuck) to 26.3 % (ring, rpm, tyres, backward) per set, 21.3 % on daytona 24 x 10 and
    6.0 % on the crowded scene.  First case seen: speed_gates car 62, device 0x1.f6e540cf99748p+0, oracle
    0x1.f6e540cf9974ap+0.  Equality would take glibc's own atan2 on the device."""
    worst = 0
    for name, C, epb in (("speed_gates", 1, 128), ("ring", 10, 12)):
        if (name, C, epb) not in _shares:
            test_one_step(name, C, epb)
        worst = max(worst, _shares[name, C, epb]["slip"][1])
    assert worst <= 1, f"slip is {worst} ulp from the oracle's"


@pytest.mark.parametrize("name", ["termination", "termination_reset_on_lap"])
@pytest.mark.parametrize("epb", S.LAYOUTS[3])
def test_termination_auto_reset(name, epb):
    """step(auto_reset=True): the done envs' cars come out reset (the oracle: step, then reset of every done env), the
    others as after a plain step"""
    c = S.build(name, 3)
    orc = c.oracle()
    _, rew, cf, ef = orc.step(c.actions)
    done = (ef[:, 0] != 0) | (ef[:, 1] != 0)
    assert done.any() and not done.all()
    for e in np.flatnonzero(done):
        orc.reset(int(e))
    obs = orc.outputs()[0]
    O = oracle_arena(orc)
    orc.close()
    env = _engine(c, epb)
    _load(env, c.blob, c.E, 3)
    env.step(torch.from_numpy(c.actions.copy()).to(env.device), auto_reset=True)
    G = gpu_arena(env.get_state().cpu().numpy(), c.E, 3)
    what = f"{name} with auto-reset at {epb} envs per workgroup"
    try:
        compare_state(what, G, O, 3)
        compare_outputs(what, env, obs, rew, cf, ef)
        assert np.array_equal((env.env_flags.cpu().numpy() & 8) != 0, done)
    finally:
        env.close()


def _teacher_forced(what, env, path, E, C, k0, K, act_fn):
    """K steps: inject the device's state into the oracle, step both with the same actions, compare everything"""
    orc = OracleEnv(path, E, C)
    worst = {f: (0.0, 0) for f in ULP_FIELDS}
    diff = {f: 0 for f in ULP_FIELDS}
    contacts = 0
    for k in range(k0, k0 + K):
        blob = env.get_state().cpu().numpy()
        inject_gpu_state(orc, blob, E, C, list(range(E)), wire=k == k0)
        a = act_fn(k, env.obs.cpu().numpy())
        env.step(torch.from_numpy(a).to(env.device))
        out = orc.step(a)
        sh = compare_state(f"{what}, step {k}", gpu_arena(env.get_state().cpu().numpy(), E, C), oracle_arena(orc), C)
        compare_outputs(f"{what}, step {k}", env, *out)
        for f, (s, m) in sh.items():
            diff[f] += round(s * E * C)
            worst[f] = (diff[f] / ((k - k0 + 1) * E * C), max(worst[f][1], m))
        contacts += int((out[2] & 4 != 0).sum())
    orc.close()
    print(f"{what}: {K * E * C} transitions, {contacts} with a wall impulse; " +
          ", ".join(f"{f} differs for {100 * s:.3f} %, at most {m} ulp" for f, (s, m) in worst.items()))
    return contacts


def test_teacher_forced_crowded(tmp_path):
    """200 steps of the crowded POCKET(40) scene (12 x 10, one workgroup) from the step its cars reach the walls"""
    from nascargymnasium_amd.batched import BatchedCarEnv
    sc = crowded.SCENES["12x10"]
    E, C = sc["E"], sc["C"]
    path = crowded.write_pocket(tmp_path, sc["r"])
    rng = np.random.default_rng(crowded.SEED)
    acts = [crowded.actions(rng, E, C) for _ in range(crowded.ROLLOUT_START - 10 + 200)]
    env = BatchedCarEnv(E, C, path, device="cuda:0", envs_per_block=sc["epb"])
    env.reset()
    k0 = crowded.ROLLOUT_START - 10
    for k in range(k0):
        env.launch_step(torch.from_numpy(acts[k]).to(env.device))
    try:
        contacts = _teacher_forced("crowded 12 x 10", env, path, E, C, k0, 200, lambda k, obs: acts[k])
        assert contacts > 1000
    finally:
        env.close()


def test_teacher_forced_daytona():
    """200 steps of daytona 24 x 10 under the noisy rule driver, from the reset"""
    from drivers import NoisyRuleDriver
    from nascargymnasium_amd.batched import BatchedCarEnv
    E, C = 24, 10
    path = S.track_path("daytona")
    env = BatchedCarEnv(E, C, path, device="cuda:0")
    env.reset()
    drv = NoisyRuleDriver(E * C, seed=7)
    try:
        _teacher_forced("daytona 24 x 10", env, path, E, C, 0, 200,
                        lambda k, obs: drv.actions(obs.reshape(E, C, 38), k).reshape(E, C, 2))
    finally:
        env.close()


# ---------------------------------------------------------------- the float64 library functions, where they are used
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def device_f64(fn, x, y=None):
    from nascargymnasium_amd import _lib
    tx = torch.from_numpy(np.ascontiguousarray(x, np.float64)).cuda()
    ty = torch.from_numpy(np.ascontiguousarray(y, np.float64)).cuda() if y is not None else None
    out = torch.full((len(x),), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().nascar_debug_f64math(_ptr(tx), _ptr(ty) if ty is not None else None, _ptr(out), len(x), fn,
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def host_libm(fn, *args):
    """glibc's double function `fn` over arrays, through ctypes (the reference's CPython calls the same libm)"""
    m = ctypes.CDLL("libm.so.6")
    f = getattr(m, fn)
    f.restype = ctypes.c_double
    f.argtypes = [ctypes.c_double] * len(args)
    return np.array([f(*(float(v) for v in row)) for row in zip(*args)], np.float64)


def _report(what, dev, ref):
    d = ulps(dev, ref)
    print(f"{what}: {len(d)} points, {100 * float((d != 0).mean()):.4f} % differ from glibc, at most {int(d.max())} ulp")
    return d


N_MATH = 100_003     # one lane per point, the last wave partial


def test_f64_exp_in_the_engine_blend():
    """exp(-2 t), t in [0, 1] (the power blend between 12 and 25 m/s): at most 1 ulp from glibc's"""
    rng = np.random.default_rng(11)
    t = np.concatenate([[0.0, 1.0, np.nextafter(0.0, 1), np.nextafter(1.0, 0)], rng.uniform(0, 1, N_MATH - 4)])
    t[4:4 + 1300] = (np.linspace(12, 25, 1300).astype(np.float32).astype(np.float64) - 12.0) / (25.0 - 12.0)
    d = _report("exp(-2 t)", device_f64(0, t), host_libm("exp", -2.0 * t))
    assert d.max() <= 1, (t[d.argmax()].hex(), int(d.max()))


def test_f64_atan2_of_the_slip_angle():
    """atan2(|cr|, d) on unit (cr, d), with cr = 0, d = +-1 and d around 0: at most 1 ulp from glibc's"""
    rng = np.random.default_rng(12)
    th = rng.uniform(-np.pi, np.pi, N_MATH)
    th[:2000] = rng.uniform(-1e-6, 1e-6, 2000)                  # a car going straight: cr around 0, d = 1
    th[2000:4000] = np.pi / 2 + rng.uniform(-1e-7, 1e-7, 2000)  # sideways: d around 0
    th[4000:5000] = np.pi + rng.uniform(-1e-6, 1e-6, 1000)      # backwards: d = -1
    cr, dd = np.sin(th), np.cos(th)
    cr[:8], dd[:8] = [0.0, 0.0, -0.0, -0.0, 1.0, -1.0, 1.0, 5e-324], [1.0, -1.0, 1.0, -1.0, 0.0, 0.0, -0.0, -1.0]
    d = _report("atan2(|cr|, d)", device_f64(1, cr, dd), host_libm("atan2", np.abs(cr), dd))
    assert d.max() <= 1, (cr[d.argmax()].hex(), dd[d.argmax()].hex(), int(d.max()))


def test_f64_tan_of_the_steering_angle():
    """tan(s), |s| <= 45 degrees, s = a float32 action times 45 degrees as the model forms it: at most 1 ulp"""
    rng = np.random.default_rng(13)
    a = rng.uniform(-1, 1, N_MATH).astype(np.float32)
    a[:6] = [0.0, 1.0, -1.0, np.float32(0.0128), 1e-30, -1e-30]
    s = a.astype(np.float64) * S.STEER_K
    d = _report("tan(steer)", device_f64(2, s), host_libm("tan", s))
    assert d.max() <= 1, (s[d.argmax()].hex(), int(d.max()))


def _force_components(rng, n):
    """(cx, cy) as _apply_lateral_tire_forces forms them: velocity error times 7500, up to a few hundred kN"""
    mag = 10.0 ** rng.uniform(-6, 5.8, n)
    th = rng.uniform(-np.pi, np.pi, n)
    return mag * np.cos(th), mag * np.sin(th)


def test_f64_sqrt_stands_for_pow_half():
    """sqrt(a^2 + b^2) as the model writes (a ** 2 + b ** 2) ** 0.5: bit-equal to the host's sqrt (both correctly
    rounded) and at most 1 ulp from glibc's pow(., 0.5), which the reference's CPython calls"""
    rng = np.random.default_rng(14)
    a, b = _force_components(rng, N_MATH)
    a[:4], b[:4] = [0.0, 3.0, 0.0, 1e-200], [0.0, 4.0, 7.5, 0.0]
    dev = device_f64(3, a, b)
    s = a * a + b * b
    assert np.array_equal(dev.view(np.uint64), np.sqrt(s).view(np.uint64)), "device sqrt != host sqrt"
    d = _report("sqrt(a^2 + b^2) against pow(., 0.5)", dev, host_libm("pow", s, np.full_like(s, 0.5)))
    assert d.max() <= 1, (s[d.argmax()].hex(), int(d.max()))


def _squares():
    rng = np.random.default_rng(15)
    return np.concatenate([_force_components(rng, 40_000)[0], rng.uniform(-5000, 5000, 20_000),
                           rng.uniform(0, 2.5, 20_000), rng.uniform(0, 90, 20_003),
                           [0.0, -0.0, 1.0, -1.0, 1e-170, 1e150]])


def test_f64_square_is_the_hosts_product():
    """x * x as the model writes Python's x ** 2, over the model's ranges (forces, distances, speed ratios, the slip
    excess): the device's product equals the host's bit for bit, and lies within 1 ulp of glibc's pow(x, 2.0)"""
    x = _squares()
    dev = device_f64(4, x)
    assert np.array_equal(dev.view(np.uint64), (x * x).view(np.uint64))
    d = _report("x * x against pow(x, 2.0)", dev, host_libm("pow", x, np.full_like(x, 2.0)))
    assert d.max() <= 1, (x[d.argmax()].hex(), int(d.max()))


@pytest.mark.xfail(strict=True, reason="measured: glibc 2.35's pow(x, 2.0) is 1 ulp from x * x for 0.078 % of the points")
def test_f64_square_equals_pow_two():
    """x * x == pow(x, 2.0) bit for bit, which DESIGN 3.4 used to rely on.  It does not hold: glibc's pow is not
    correctly rounded (since 2.28 it is a 0.52-ulp log / exp evaluation), so for 78 of these 100 009 points (0.078 %)
    pow(x, 2.0) is the neighbour of the correctly rounded square, e.g. x = 1536.84331...: never more than 1 ulp.  No
    float64 field of the state was seen to differ for it in the single-step tests above (the squares feed sums and
    products that absorb a last bit); equality would take glibc's own pow on the device."""
    x = _squares()
    ref = host_libm("pow", x, np.full_like(x, 2.0))
    assert np.array_equal(device_f64(4, x).view(np.uint64), ref.view(np.uint64))

"""b2_step's capacity paths on crowded tight-curve scenes (tests/crowded.py): device == CPU oracle, bit for bit.

The bundled tracks never give a car more than 7 contacts, so the paths that csrc/nascar_device.h takes past its
capacities (contact records leaving LDS at CT_LDS_CAP, b2TimeOfImpact rounds past TOI_JOBCAP, owner-computed event
manifolds past MANI_JOBCAP, general TOI islands, the MAXC overflow flag) ran unseen.  The POCKET tracks crowd 120 or
128 cars into a curve of 1-degree chords; tests/test_crowded_cpu.py proves from the oracle's statistics which paths
each scene takes in which wave, and here every engine layout must equal the oracle on them.  The tools build with caps
of 3 / 3 / 2 (tools/build/libnascar_smallcaps.so) crosses every cap at almost every step and must equal the product
build.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import crowded

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def tracks(tmp_path_factory):
    return tmp_path_factory.mktemp("crowded")


_device = {}


def _product(tracks, name, epb, fused):
    """the product library's run of a scene's saved actions (once per process and layout)"""
    key = (name, epb, fused)
    if key not in _device:
        sc = crowded.SCENES[name]
        run = crowded.scene_run(tracks, sc)
        _device[key] = crowded.device_run(run.path, sc["E"], sc["C"], epb, fused, run.actions, info_every=10)
    return _device[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_equals_oracle(d, run, lay, steps=None, envs=None):
    """per-step obs, reward, terminated / truncated and car_flags & 5 of device run `d` equal the oracle run's on
    steps [0, steps) of `envs` (default: all), bit for bit"""
    S = run.steps if steps is None else steps
    e = slice(None) if envs is None else envs
    for what, g, o in (("obs", _bits(d["obs"][:S, e]), _bits(run.obs[:S, e])),
                       ("reward", _bits(d["reward"][:S, e]), _bits(run.reward[:S, e])),
                       ("disabled / collision flags", d["car_flags"][:S, e] & 5, run.car_flags[:S, e] & 5),
                       ("terminated", (d["env_flags"][:S, e] & 1) != 0, run.env_flags[:S, e, 0] != 0),
                       ("truncated", (d["env_flags"][:S, e] & 2) != 0, run.env_flags[:S, e, 1] != 0)):
        bad = np.argwhere(g != o)
        assert len(bad) == 0, f"{lay}: {what} differ from the oracle first at step {bad[0, 0]}, at {bad[:5].tolist()}"


def _assert_block_map(d, E, C, epb):
    """the engine's workgroups hold the envs that crowded.wave_of (the coverage counts' wave membership) assumes"""
    want = np.arange(-(-E // epb) * epb).reshape(-1, epb)
    want[want >= E] = -1
    assert np.array_equal(d["blk_env"], want), (d["blk_env"].tolist(), epb)


@pytest.mark.parametrize("name", sorted(crowded.SCENES))
def test_crowded_scene_vs_oracle(tracks, name):
    """Every step of the scene through every engine (12 x 10: 12 envs per workgroup fused and two-launch, and one env
    per workgroup; 128 x 1: 128 envs per workgroup fused and two-launch): obs, reward, terminated / truncated and the
    disabled / collision flags equal the oracle's bit for bit, n_contacts equals the oracle's every 10th step, no
    error flag is raised, and the engines end with equal state arenas.  What the scene covers in these layouts' waves:
    tests/test_crowded_cpu.py."""
    sc = crowded.SCENES[name]
    E, C = sc["E"], sc["C"]
    run = crowded.scene_run(tracks, sc)
    engines = [(sc["epb"], True), (sc["epb"], False)] + ([(1, True)] if name == "12x10" else [])
    runs = []
    for epb, fused in engines:
        lay = f"{name}, envs per block {epb}, " + ("fused model + logic" if fused else "model_kernel + logic_kernel")
        d = _product(tracks, name, epb, fused)
        _assert_block_map(d, E, C, epb)
        assert np.array_equal(_bits(d["obs0"]), _bits(run.obs0)), f"{lay}: reset obs"
        _assert_equals_oracle(d, run, lay)
        ks = d["info_steps"]
        bad = np.argwhere(d["n_contacts"] != run.nct[ks])
        assert len(bad) == 0, f"{lay}: n_contacts differ from the oracle at step {ks[bad[0, 0]]}: {bad[:5].tolist()}"
        assert not (d["error"] != 0).any(), f"{lay}: info error field"
        assert not (d["car_flags"] & 128).any(), f"{lay}: error flag at {np.argwhere(d['car_flags'] & 128)[:5].tolist()}"
        runs.append((lay, d))
    for lay, d in runs[1:]:
        assert np.array_equal(d["state"], runs[0][1]["state"]), f"final state arena: {lay} vs {runs[0][0]}"


def test_crowded_rollout_equals_per_step(tracks):
    """From the 12 x 10 scene's state after crowded.ROLLOUT_START steps (57 of the 120 cars above 4 contacts, their
    records outside LDS; the cars only reach the curve around step 290), 60 steps of the device noisy rule driver
    through the sharded rollout, the fused rollout kernel and nascar_step_driven one step at a time end with equal
    observations and state arenas; at least 20 cars hold more than 4 contacts at the start and at the end."""
    from nascargymnasium_amd import _lib
    from nascargymnasium_amd.batched import BatchedCarEnv
    sc = crowded.SCENES["12x10"]
    E, C, K, seed = sc["E"], sc["C"], 60, 5
    run = crowded.scene_run(tracks, sc)
    nct = _lib.INFO_INDEX["n_contacts"]
    a = BatchedCarEnv(E, C, run.path, device="cuda:0", envs_per_block=sc["epb"])
    a.reset()
    ta = torch.from_numpy(np.array(run.actions[:crowded.ROLLOUT_START])).cuda()
    for k in range(crowded.ROLLOUT_START):
        a.launch_step(ta[k])
    k0 = crowded.ROLLOUT_START - 1
    assert np.array_equal(_bits(a.obs.cpu().numpy()), _bits(run.obs[k0]))
    n0 = a.info_tensor()[..., nct].cpu().numpy()
    assert np.array_equal(n0, run.nct[k0]) and int((n0 > 4).sum()) >= 20, int((n0 > 4).sum())
    state0, obs0 = a.get_state(), a.obs.clone()
    twins = []
    for streams in (4, 0):
        t = BatchedCarEnv(E, C, run.path, device="cuda:0", envs_per_block=sc["epb"])
        t.set_rollout_streams(streams)
        t.set_state(state0)
        t.obs.copy_(obs0)
        t.rollout(3, K, seed=seed, step0=0, auto_reset=True)
        twins.append((f"rollout, set_rollout_streams({streams})", t))
    for k in range(K):
        a.step_driven(3, seed=seed, step=k, auto_reset=True)
    n1 = a.info_tensor()[..., nct].cpu().numpy()
    assert int((n1 > 4).sum()) >= 20, int((n1 > 4).sum())
    sa = a.get_state()
    assert not torch.equal(sa, state0)
    for name, t in twins:
        assert torch.equal(t.obs, a.obs), f"final obs differ: {name} at {torch.nonzero(t.obs != a.obs)[:5].tolist()}"
        assert torch.equal(t.get_state(), sa), f"final state arena differs: {name}"
        assert not (t.car_flags & 128).any()
        t.close()
    assert not (a.car_flags & 128).any()
    a.close()


def test_contact_overflow_is_flagged(tracks):
    """POCKET(16), 12 x 10 at 12 envs per workgroup: a car collects a 17th fat-AABB pair at step k* (the oracle keeps 24
    and goes on; tests/test_crowded_cpu.py).  Up to k* - 1 every env equals the oracle bit for bit and no error flag
    is up; at the step an env's first car passes 16 contacts in the oracle (k* for the first env), bit 7 of car_flags
    and info's error field are up for exactly those cars of the env; envs with no such car so far stay bit-exact and
    unflagged through k* + 50; a masked reset of an overflowed env clears its flag and leaves the other envs'."""
    sc = crowded.OVERFLOW
    E, C = sc["E"], sc["C"]
    run = crowded.scene_run(tracks, sc)
    ks = crowded.first_overflow(run.nct)
    assert ks is not None
    S = ks + 51
    d = crowded.device_run(run.path, E, C, sc["epb"], True, run.actions[:S], info_every=1, keep_env=True)
    env = d["env"]
    lay = "overflow scene"
    _assert_equals_oracle(d, run, lay, steps=ks)
    assert not (d["car_flags"][:ks] & 128).any() and not d["error"][:ks].any()
    assert np.array_equal(d["n_contacts"][:ks], run.nct[:ks])
    over = run.nct[:S] > crowded.GPU_MAXC                      # [S, E, C]
    dirty = np.maximum.accumulate(over.any(2), 0)              # [S, E]: some car of the env has overflowed by step k
    first = np.where(dirty.any(0), dirty.argmax(0), -1)        # each env's first overflow step
    assert (first < 0).any() and (first >= 0).any()
    flagged = (d["car_flags"] & 128) != 0
    for e in np.nonzero(first >= 0)[0]:
        k = int(first[e])
        assert np.array_equal(flagged[k, e], over[k, e]), (int(e), k, flagged[k, e].tolist(), over[k, e].tolist())
        assert np.array_equal(d["error"][k, e] == 1, over[k, e]) and not (d["error"][k, e] > 1).any(), (int(e), k)
        assert not flagged[:k, e].any()
    assert np.array_equal(flagged[ks], over[ks]) and over[ks].any()
    for k in range(ks, S):
        clean = np.nonzero(~dirty[k])[0]
        assert len(clean) > 0
        for what, g, o in (("obs", _bits(d["obs"][k, clean]), _bits(run.obs[k, clean])),
                           ("reward", _bits(d["reward"][k, clean]), _bits(run.reward[k, clean])),
                           ("flags", d["car_flags"][k, clean] & (5 | 128), run.car_flags[k, clean] & 5),
                           ("terminated", (d["env_flags"][k, clean] & 1) != 0, run.env_flags[k, clean, 0] != 0),
                           ("truncated", (d["env_flags"][k, clean] & 2) != 0, run.env_flags[k, clean, 1] != 0)):
            assert np.array_equal(g, o), f"step {k}: {what} of the envs without overflow {clean.tolist()}"
    # the flag is kept until the env is reset, and a masked reset clears it for that env alone
    lost = np.nonzero(dirty[S - 1])[0]
    assert flagged[S - 1, lost].any(1).all()
    e0 = int(np.nonzero(over[ks].any(1))[0][0])
    m = torch.zeros(E, dtype=torch.uint8, device=env.device)
    m[e0] = 1
    env.reset(m)
    from nascargymnasium_amd import _lib
    err = env.info_tensor()[..., _lib.INFO_INDEX["error"]].cpu().numpy()
    assert not err[e0].any()
    env.launch_step(torch.from_numpy(np.array(run.actions[S])).cuda())
    cf = env.car_flags.cpu().numpy()
    assert not (cf[e0] & 128).any()
    for e in lost:
        if e != e0:
            assert (cf[e] & 128).any() and err[e].any(), int(e)
    assert not (cf[~dirty[S - 1]] & 128).any()
    env.close()


def test_small_caps_build_identical(tracks, tmp_path):
    """The tools build with TOI_JOBCAP = MANI_JOBCAP = 3 and CT_LDS_CAP = 2 (__graft_entry__.build) in a fresh child
    process (tests/step_child.py): the 12 x 10 scene's saved actions at 12 envs per workgroup, fused and two-launch.
    With these caps a wave takes a second b2TimeOfImpact round, leaves event manifolds to their owners and moves
    contact records out of LDS many times over (tests/test_crowded_cpu.py counts the steps and waves), and a lane's
    contacts straddle the boundaries; every step's obs, reward, car and env flags and the final state arena equal the
    product build's, which test_crowded_scene_vs_oracle holds to the oracle."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    variant = os.path.join(root, "tools", "build", "libnascar_smallcaps.so")
    assert os.path.exists(variant), "build() builds the small-caps test variant"
    sc = crowded.SCENES["12x10"]
    run = crowded.scene_run(tracks, sc)
    af, of = str(tmp_path / "actions.npy"), str(tmp_path / "out.npz")
    np.save(af, run.actions)
    child = os.path.join(root, "tests", "step_child.py")
    r = subprocess.run([sys.executable, child, run.path, str(sc["E"]), str(sc["C"]), str(sc["epb"]), af, of],
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, NASCAR_LIB=variant))
    assert r.returncode == 0, r.stderr[-2000:]
    small = np.load(of)
    for name, fused in (("fused", True), ("unfused", False)):
        d = _product(tracks, "12x10", sc["epb"], fused)
        for key in ("obs", "reward", "car_flags", "env_flags"):
            g, o = small[f"{name}_{key}"], d[key]
            if g.dtype == np.float32:
                g, o = _bits(g), _bits(o)
            bad = np.argwhere(g != o)
            assert len(bad) == 0, f"{name}: {key} differ from the product build first at step {bad[0, 0]}: {bad[:5].tolist()}"
        assert np.array_equal(small[f"{name}_state"], d["state"]), f"{name}: final state arena"

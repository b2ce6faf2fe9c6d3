"""Opponent-aware distance sensors on the device (nascar_set_car_visibility) against the expected rows of
tests/opponents.py: min(the oracle's walls-only row, b2PolygonShape::RayCast against the env's other cars' boxes).
tests/test_opponents_cpu.py pins that restatement to the oracle and proves what the scenes exercise."""
import ctypes
import os

import numpy as np
import pytest

import opponents as op

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EF_RESET = 8


def _path(track):
    return os.path.join(op.TRACKS, track)


def _debug_sensors(env, poses, impl):
    from nascargymnasium_amd import _lib
    p = torch.from_numpy(np.array(poses, np.float32).reshape(-1, 3)).cuda()
    obs = torch.full((env.N, 38), -7.0, dtype=torch.float32, device="cuda")
    _lib.check(env.L.nascar_debug_sensors(env.h, ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(obs.data_ptr()),
                                          impl, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return obs.cpu().numpy()


def _same(a, b, what):
    bad = np.argwhere(np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} values differ, first at {bad[0].tolist()}: " \
                          f"{np.asarray(a)[tuple(bad[0])]!r} vs {np.asarray(b)[tuple(bad[0])]!r}"


@pytest.mark.parametrize("track,E,C", [("martinsville.track", 64, 10), ("daytona.track", 64, 10), ("daytona.track", 13, 10),
                                       ("daytona.track", 5, 3), ("daytona.track", 1, 2), ("daytona.track", 16, 1)])
def test_debug_sensors_on_cluster_poses(track, E, C):
    """switch on: the beam-list kernel at 16 lanes per car (128-, 64- and 256-thread workgroups) and at 4 lanes, and the
    wall-group kernel, equal each other and the expected rows bit for bit and leave obs[:, :22] alone; switch off: the
    same poses give the walls-only oracle rows; with one car per env the switch changes nothing"""
    from nascargymnasium_amd.batched import BatchedCarEnv
    poses, walls, rows, st = op.cluster_expected(track, E, C)
    if E * C >= 15:
        assert st["near"].any() == (C > 1), "the scene shows no car"
    if (E, C) == (64, 10):
        assert st["near"].sum() >= op.CLUSTER_FLOOR["near"] and st["inside"].sum() >= op.CLUSTER_FLOOR["inside"]
        assert (st["car"] & ~st["near"]).sum() >= op.CLUSTER_FLOOR["behind"]
    env = BatchedCarEnv(E, C, _path(track), device="cuda:0")
    assert env.car_visibility is False
    off = _debug_sensors(env, poses, 1)
    env.set_car_visibility(True)
    assert env.car_visibility is True
    out = {"16x128": _debug_sensors(env, poses, 1)}
    for rb in (64, 256):
        env.set_sensor_block(rb)
        out[f"16x{rb}"] = _debug_sensors(env, poses, 1)
    env.set_sensor_block(0)
    env.set_sensor_lanes(4)
    out["4"] = _debug_sensors(env, poses, 1)
    env.set_sensor_lanes(0)
    out["groups"] = _debug_sensors(env, poses, 0)
    env.set_car_visibility(False)
    off_groups = _debug_sensors(env, poses, 0)
    env.close()
    want = rows.reshape(E * C, 16)
    for k, o in out.items():
        assert (o[:, :22] == -7.0).all(), f"{k}: the sensor launch wrote outside obs[22:38]"
        _same(o[:, 22:], want, f"{k} lanes x threads vs the expected rows")
    _same(off[:, 22:], walls.reshape(E * C, 16), "switch off vs the walls-only rows")
    _same(off_groups[:, 22:], walls.reshape(E * C, 16), "switch off again (wall groups) vs the walls-only rows")
    if C == 1:
        _same(want, walls.reshape(E * C, 16), "one car per env")


def test_closed_loop_against_the_oracle_contact_off():
    """daytona 4 x 10, every car its own throttle, 600 steps through step() at 1 and at 12 envs per workgroup, cars
    seen but not touched: every step obs[..., :22], rewards and flags are the oracle's and obs[..., 22:] are the
    expected rows built from the oracle's poses"""
    from nascargymnasium_amd.batched import BatchedCarEnv
    sc = op.THROTTLE
    R = op.throttle_run()
    assert int(R["near"][::5].sum()) >= op.THROTTLE_FLOOR_NEAR
    E, C, S = sc["E"], sc["C"], sc["steps"]
    envs = []
    for epb in (1, 12):
        env = BatchedCarEnv(E, C, _path(sc["track"]), device="cuda:0", envs_per_block=epb)
        assert env.envs_per_block == epb
        env.set_car_visibility(True)
        envs.append(env)
    act = torch.from_numpy(R["actions"].copy()).cuda()
    want = R["obs"].copy()
    want[..., 22:] = R["rows"]
    done = (R["env_flags"][..., 0] != 0) | (R["env_flags"][..., 1] != 0)
    seen = 0
    for k in range(S + 1):
        for env in envs:
            if k == 0:
                env.reset()
            else:
                env.step(act[k - 1])
            lay = f"record {k}, {env.envs_per_block} envs per workgroup"
            go = env.obs.cpu().numpy()
            _same(go[..., :22], want[k][..., :22], lay + ": obs[:22]")
            _same(go[..., 22:], want[k][..., 22:], lay + ": sensors")
            if k:
                _same(env.reward.cpu().numpy(), R["reward"][k], lay + ": reward")
                assert np.array_equal(env.car_flags.cpu().numpy() & 5, R["car_flags"][k] & 5), lay + ": car flags"
                assert np.array_equal((env.env_flags.cpu().numpy() & 3) != 0, done[k]), lay + ": env flags"
        seen += int((want[k][..., 22:] != R["obs"][k][..., 22:]).sum())
    for env in envs:
        env.close()
    assert seen >= op.THROTTLE_FLOOR_NEAR, "the cars never saw each other"


def _state_poses(env):
    """[E, C, 3] float32 body positions and angles from the state blob"""
    from gpu_state import decode
    d = decode(env.get_state().cpu().numpy(), env.N)
    return np.stack([d["xpx"], d["xpy"], d["a"]], 1).reshape(env.E, env.C, 3).astype(np.float32)


def _expected_from_state(env, track):
    from oracle_lib import OracleEnv
    poses = _state_poses(env)
    orc = OracleEnv(_path(track), 1, 1)
    walls = op.wall_rows(orc, poses).reshape(env.E, env.C, 16)
    orc.close()
    return op.expected_rows(poses, walls)[0], walls


def test_auto_reset_and_terminal_obs_contact_on():
    """talladega 6 x 10 on the staggered grid: after a step that truncates two envs, their obs[22:38] are the
    expected rows of the reset poses (grid neighbours seen), terminal_obs[22:38] are the rows of a twin that took the
    step without auto-reset, and a masked reset() gives the reset rows too"""
    from nascargymnasium_amd.batched import BatchedCarEnv
    from oracle_lib import gpu_arena
    track, E, C = "talladega.track", 6, 10
    mk = lambda: BatchedCarEnv(E, C, _path(track), device="cuda:0")
    env, twin = mk(), mk()
    for x in (env, twin):
        x.set_car_contact(True)
        x.set_car_visibility(True)
    env.reset()
    grid = env.obs.cpu().numpy()
    want, walls = _expected_from_state(env, track)
    _same(grid[..., 22:], want, "reset rows on the grid")
    # car 2 stands 8 m behind car 0 in the same column: its ray 0 ends on car 0's rear face
    assert np.all(np.abs(grid[:, 2, 22].astype(np.float64) * 250.0 - (8.0 - float(op.CAR_HX))) < 1e-3), grid[:, 2, 22] * 250
    assert (walls[:, 2, 0] * 250.0 > 8.0).all()
    for k in range(40):   # leave the grid
        env.step_driven(3, seed=9, step=k, auto_reset=True)
    blob = env.get_state().cpu().numpy().copy()
    ends = [1, 4]
    gpu_arena(blob, E, C)["time"][ends] = 180.0      # the next step passes the 180 s limit: truncated
    st = torch.from_numpy(blob).cuda()
    for x in (env, twin):
        x.set_state(st)
    a = env.policy_actions(3, seed=9, step=40).clone()
    env.step(a, auto_reset=True, terminal_obs=True)
    twin.step(a, auto_reset=False)
    ef = env.env_flags.cpu().numpy()
    assert ((ef & EF_RESET) != 0).tolist() == [e in ends for e in range(E)], ef
    go, term, to = env.obs.cpu().numpy(), env.terminal_obs.cpu().numpy(), twin.obs.cpu().numpy()
    want, _ = _expected_from_state(env, track)       # reset envs: the grid again; the others: the step's poses
    _same(go[..., 22:], want, "obs after the auto-reset step vs the rows of the state's poses")
    _same(go[ends][..., 22:], grid[ends][..., 22:], "the reset envs see their grid neighbours")
    _same(term[ends], to[ends], "terminal_obs vs the twin without auto-reset")
    keep = [e for e in range(E) if e not in ends]
    _same(go[keep], to[keep], "envs that went on")
    m = torch.zeros(E, dtype=torch.uint8, device="cuda")
    m[ends] = 1
    twin.reset(m)
    _same(twin.obs.cpu().numpy()[..., 22:], go[..., 22:], "masked reset vs the auto-reset rows")
    env.close()
    twin.close()


@pytest.mark.parametrize("contact", [True, False])
def test_rollout_equals_per_step(contact):
    """switch on, talladega 24 x 10, 300 steps of the noisy rule driver: the sharded rollout at 1 and 4 streams with an
    obs trajectory equals the per-step path bit for bit -- every step's obs, reward and flags, and the final state"""
    from nascargymnasium_amd.batched import BatchedCarEnv
    track, E, C, S = "talladega.track", 24, 10, 300

    def mk():
        x = BatchedCarEnv(E, C, _path(track), device="cuda:0")
        x.set_car_contact(contact)
        x.set_car_visibility(True)
        x.reset()
        return x
    ref = mk()
    obs = torch.empty(S + 1, E, C, 38, device="cuda")
    rew, cf = torch.empty(S, E, C, device="cuda"), torch.empty(S, E, C, dtype=torch.uint8, device="cuda")
    ef = torch.empty(S, E, dtype=torch.uint8, device="cuda")
    obs[0] = ref.obs
    for k in range(S):
        ref.step_driven(3, seed=4, step=k, auto_reset=True)
        obs[k + 1], rew[k], cf[k], ef[k] = ref.obs, ref.reward, ref.car_flags, ref.env_flags
    want, walls = _expected_from_state(ref, track)     # the last record: the expected rows of the state's poses
    _same(obs[S].cpu().numpy()[..., 22:], want, "the last step's sensors")
    print(f"contact {contact}: {(want < walls).sum()} of {want.size} rays of the last record see a car")
    assert (want < walls).any(), "the scene shows no car"
    for streams in (1, 4):
        x = mk()
        x.set_rollout_streams(streams)
        o, r, c, e = x.rollout(3, S, seed=4, step0=0, auto_reset=True, trajectory=True, obs_trajectory=True)
        assert torch.equal(o, obs), f"{streams} streams: obs trajectory"
        assert torch.equal(r, rew) and torch.equal(c, cf) and torch.equal(e, ef), f"{streams} streams: records"
        assert torch.equal(x.get_state(), ref.get_state()), f"{streams} streams: final state"
        x.close()
    ref.close()


def test_combinations_refused_or_rescheduled():
    """the fused single-launch rollout and random-track mode refuse the switch with an error that names the
    combination; with the pipelined rollout set, rollout() gives the streams schedule's results"""
    from nascargymnasium_amd.batched import BatchedCarEnv
    track, E, C = "talladega.track", 12, 4
    mk = lambda: BatchedCarEnv(E, C, _path(track), device="cuda:0")
    env = mk()
    env.set_car_visibility(True)
    env.reset()
    before = env.obs.clone()
    env.set_rollout_streams(0)
    with pytest.raises(RuntimeError, match="car visibility.*fused single-launch rollout"):
        env.rollout(3, 5, seed=1)
    assert torch.equal(env.obs, before)
    env.set_rollout_streams(2)
    env.set_random_tracks([_path("talladega.track"), _path("daytona.track")], seeds=np.arange(E))
    for call in (lambda: env.reset(), lambda: env.step(torch.zeros(E, C, 2, device="cuda")),
                 lambda: env.step_driven(3), lambda: env.rollout(3, 5, seed=1)):
        with pytest.raises(RuntimeError, match="car visibility.*random-track mode"):
            call()
    env.close()
    a, b = mk(), mk()
    for x in (a, b):
        x.set_car_visibility(True)
        x.reset()
    a.set_rollout_pipe(16)
    ra = a.rollout(3, 60, seed=3, trajectory=True)
    rb = b.rollout(3, 60, seed=3, trajectory=True)
    assert a.rollout_pipe_status() == 0
    for u, v in zip(ra, rb):
        assert torch.equal(u, v)
    assert torch.equal(a.get_state(), b.get_state())
    blind = mk()
    blind.reset()
    blind.rollout(3, 60, seed=3)
    assert not torch.equal(blind.obs[..., 22:], a.obs[..., 22:]), "the scene shows no car"
    for x in (a, b, blind):
        x.close()


def test_off_is_off():
    """the switch toggled on for a step and off again mid-run: the next 100 steps and the state equal those of a twin
    that never had it on (the switch is no part of the state; explicit actions, so no driver reads the sensors)"""
    from nascargymnasium_amd.batched import BatchedCarEnv
    track, E, C, S = "daytona.track", 8, 10, 251
    rng = np.random.default_rng(8)
    u = rng.uniform(-1, 1, (S, E, C, 2)).astype(np.float32)
    u[..., 0] = (0.4 + 0.6 * rng.uniform(0, 1, (1, E, C))) * (0.8 + 0.2 * np.abs(u[..., 0]))   # each car its own pace
    u[..., 1] *= 0.1
    act = torch.from_numpy(u).cuda()
    a = BatchedCarEnv(E, C, _path(track), device="cuda:0")
    b = BatchedCarEnv(E, C, _path(track), device="cuda:0")
    a.reset()
    b.reset()
    for k in range(150):
        a.step(act[k], auto_reset=True)
        b.step(act[k], auto_reset=True)
    a.set_car_visibility(True)
    a.step(act[150], auto_reset=True)
    b.step(act[150], auto_reset=True)
    assert not torch.equal(a.obs[..., 22:], b.obs[..., 22:]), "the scene shows no car"
    assert torch.equal(a.obs[..., :22], b.obs[..., :22]) and torch.equal(a.reward, b.reward)
    assert torch.equal(a.get_state(), b.get_state())
    a.set_car_visibility(False)
    assert a.car_visibility is False
    for k in range(151, S):
        a.step(act[k], auto_reset=True)
        b.step(act[k], auto_reset=True)
        assert torch.equal(a.obs, b.obs) and torch.equal(a.reward, b.reward), k
        assert torch.equal(a.car_flags, b.car_flags) and torch.equal(a.env_flags, b.env_flags), k
    assert torch.equal(a.get_state(), b.get_state())
    a.close()
    b.close()


def test_vec_env_and_car_env_reach_the_switch():
    """VecCarEnv (through .engine and env_method) and CarEnv (the reference's constructor, then set_car_visibility):
    with the cars stacked at the start pose nothing changes; after they spread the sensors differ from a blind twin"""
    from nascargymnasium_amd.car_env import CarEnv
    from nascargymnasium_amd.vec_env import VecCarEnv
    v = VecCarEnv(3, "daytona", num_cars=4)
    assert v.engine.car_visibility is False
    assert v.env_method("set_car_visibility", True) == [True] * 3 and v.engine.car_visibility is True
    assert v.env_method("set_car_visibility", False, indices=[1]) == [False]
    v.close()
    envs = [CarEnv(track_file="daytona", num_cars=3), CarEnv(track_file="daytona", num_cars=3)]
    envs[0].set_car_visibility(True)
    assert envs[0].car_visibility is True and envs[1].car_visibility is False
    o = [e.reset()[0] for e in envs]
    assert np.array_equal(o[0], o[1])                      # stacked: every origin inside every other box
    a = np.array([[1.0, 0.0], [0.6, 0.0], [0.3, 0.0]], np.float32)
    for k in range(200):
        o = [e.step(a)[0] for e in envs]
    assert np.array_equal(o[0][:, :22], o[1][:, :22]) and not np.array_equal(o[0][:, 22:], o[1][:, 22:])
    assert (o[0][:, 22:] <= o[1][:, 22:]).all()
    for e in envs:
        e.close()

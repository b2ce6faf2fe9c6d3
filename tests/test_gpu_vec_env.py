"""VecCarEnv's device bookkeeping at more than one workgroup: SB3 Monitor's episode return and length
(vec_post_kernel) against Monitor restated on the host, the action-space check (action_check_kernel and the host
branch for non-int32 discrete actions) at single bad values, the closed ends and indices past the first block, and
the discrete path against the engine."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

E = 300          # two 256-thread blocks of vec_post_kernel, the second partial; 600 continuous action values: 3 blocks


def _drive_params(C, seed=18):
    """seeded per-car steering of the driving envs (one env in three): full throttle, straight for `after` steps of
    the episode, then a constant left-hand steering angle -- into martinsville's wall at speed (impact-disabled after
    ~280 - 600 steps, so some envs finish two episodes in 700 steps).  Every other driving env steers all its cars
    alike (they crash together: the short episodes), the others car by car.  The rest idle (stuck-disabled at 600)."""
    rng = np.random.default_rng(seed)
    after, steer = rng.integers(60, 221, (E, C)), rng.uniform(-0.45, -0.05, (E, C)).astype(np.float32)
    alike = (np.arange(E) % 6 == 0)[:, None]
    return np.where(alike, after[:, :1], after), np.where(alike, steer[:, :1], steer)


def _drive_actions(n, after, steer):
    """actions [E, C, 2] at episode step n[e] of env e"""
    a = np.zeros(steer.shape + (2,), np.float32)
    drive = (np.arange(E) % 3 == 0)[:, None]
    a[..., 0] = np.where(drive, 1.0, 0.0)
    a[..., 1] = np.where(drive & (n[:, None] >= after), steer, 0.0)
    return a


@pytest.mark.parametrize("tensors", [False, True])
@pytest.mark.parametrize("C", [1, 3])
def test_monitor_episode_return_and_length(C, tensors):
    """info["episode"] is SB3 Monitor's: Monitor.step appends float(reward) to a list and, at done, reports
    r = round(sum(list), 6) and l = len(list) (added left to right in float64), then starts a new list; reset() starts
    one too.  Restated here per env (and car) and compared exactly at every episode end of a 700-step run of 300 envs,
    with a venv.reset() in the middle of the episodes.  C = 3: array-wise, every car's return Python's round(total, 6).

    Python >= 3.12's built-in sum is compensated (Neumaier), and Monitor calls sum; the kernel and this test add
    plainly.  Measured on this test's episodes (printed below, not asserted): of the 290 episode returns at C = 1 and
    the 792 car returns of 264 episodes at C = 3 (lengths 282 - 600), 0 round differently to 6 places under math.fsum."""
    from nascargymnasium_amd import VecCarEnv
    venv = VecCarEnv(E, "martinsville", num_cars=C, return_tensors=tensors)
    venv.reset()
    after, steer = _drive_params(C)
    n = np.zeros(E, np.int64)                    # the step each env is at within its episode
    hist = [[[] for _ in range(C)] for _ in range(E)]
    end_steps, episodes, fsum_differs, returns = set(), np.zeros(E, np.int64), 0, 0
    after_reset = 0
    RESET_AT = 20
    for k in range(700):
        if k == RESET_AT:       # mid-episode: every env's return and length start again from zero
            assert min(len(h[0]) for h in hist) > 0
            venv.reset()
            hist = [[[] for _ in range(C)] for _ in range(E)]
            n[:] = 0
        a = _drive_actions(n, after, steer)
        n += 1
        act = a if C > 1 else a[:, 0]
        obs, rew, done, infos = venv.step(torch.from_numpy(act).cuda() if tensors else act)
        if tensors:
            assert rew.is_cuda and done.is_cuda
            rew, done_any = rew.cpu().numpy(), bool(done.any())
        else:
            done_any = bool(done.any())
        rew = rew.reshape(E, C)
        for e in range(E):
            for c in range(C):
                hist[e][c].append(float(rew[e, c]))
        if not done_any:        # (the lazy infos are read only on steps that end an episode)
            continue
        done = done.cpu().numpy() if tensors else done
        for e in range(E):
            if not done[e]:
                assert infos[e] == {}, (k, e)
                continue
            totals = []
            for c in range(C):
                t = 0.0
                for r in hist[e][c]:
                    t += r
                totals.append(t)
                returns += 1
                fsum_differs += round(math.fsum(hist[e][c]), 6) != round(t, 6)
            ep = infos[e]["episode"]
            if C == 1:
                assert isinstance(ep["r"], float) and ep["r"] == round(totals[0], 6), (k, e, ep["r"], totals)
            else:
                want = np.array([round(t, 6) for t in totals], np.float64)
                assert ep["r"].shape == (C,) and ep["r"].dtype == np.float64
                assert np.array_equal(ep["r"], want), (k, e, ep["r"], want)
            assert ep["l"] == len(hist[e][0]), (k, e, ep["l"], len(hist[e][0]))
            hist[e] = [[] for _ in range(C)]
            n[e] = 0
            end_steps.add(k)
            episodes[e] += 1
            after_reset += k >= RESET_AT
    print(f"monitor C={C} tensors={tensors}: {int(episodes.sum())} episodes, {returns} returns, "
          f"{fsum_differs} round differently under math.fsum, {len(end_steps)} distinct end steps")
    assert len(end_steps) >= 20, sorted(end_steps)
    assert episodes.max() >= 2, episodes.max()
    assert after_reset >= E // 3 and (episodes[np.arange(E) % 3 != 0] >= 1).all()    # idle envs (~600 steps) included
    venv.close()


def _valid_continuous():
    a = np.zeros((E, 2), np.float32)
    one = np.float32(1)
    edge = [1.0, -1.0, -0.0, 1e-45, np.nextafter(one, np.float32(0)), np.nextafter(-one, np.float32(0))]
    a.reshape(-1)[[0, 255, 256, 257, 598, 599]] = np.array(edge, np.float32)
    assert a.reshape(-1)[257] != 0 and abs(a.reshape(-1)[257]) < np.finfo(np.float32).tiny     # a denormal
    return a


def _expect_invalid(venv, actions):
    """the action check alone (step_async), read through check_actions(): raises, and the flag is cleared by the raise.
    The step itself is not taken: the env state after an invalid action is undefined."""
    venv.step_async(actions)
    with pytest.raises(AssertionError, match="Invalid action"):
        venv.check_actions()
    assert int(venv._bad.item()) == 0
    venv.check_actions()


def test_continuous_action_check_single_values():
    from nascargymnasium_amd import VecCarEnv
    venv = VecCarEnv(E, "martinsville", num_cars=1, return_tensors=True)
    venv.reset()
    good = _valid_continuous()
    venv.step(torch.from_numpy(good).cuda())     # the closed ends, -0.0, a denormal and the values next inside the ends
    venv.check_actions()
    one = np.float32(1)
    bad = [np.nextafter(one, np.float32(2)), np.nextafter(-one, np.float32(-2)), np.float32("nan"), np.float32("inf"),
           -np.float32("inf")]
    assert bad[0] > 1 and bad[1] < -1
    for i in (0, 255, 256, 599):                 # the first and last thread of block 0, the first of block 1, the last
        for v in bad:
            a = good.copy()
            a.reshape(-1)[i] = v
            _expect_invalid(venv, torch.from_numpy(a).cuda())
    venv.step(torch.from_numpy(good).cuda())
    venv.check_actions()
    venv.close()


@pytest.mark.parametrize("C", [1, 2])
def test_discrete_action_check_single_values(C):
    from nascargymnasium_amd import VecCarEnv
    venv = VecCarEnv(E, "martinsville", num_cars=C, discrete_action_space=True, return_tensors=True)
    venv.reset()
    n = E * C
    rng = np.random.default_rng(5)
    good = rng.integers(0, 5, n).astype(np.int32)
    good[[0, 255, 256, n - 1]] = [0, 4, 4, 0]
    shape = (E,) if C == 1 else (E, C)
    venv.step(torch.from_numpy(good.reshape(shape)).cuda())
    venv.check_actions()
    for i in (0, 255, 256, n - 1):               # int32: checked on the device (action_check_kernel)
        for v in (-1, 5, np.iinfo(np.int32).min):
            a = good.copy()
            a[i] = v
            _expect_invalid(venv, torch.from_numpy(a.reshape(shape)).cuda())
    # any other dtype: checked before the conversion to int32 would hide the value
    for i in (0, 256, n - 1):
        a = good.astype(np.float32)
        a[i] = 2.5
        _expect_invalid(venv, torch.from_numpy(a.reshape(shape)).cuda())
        a = good.astype(np.int64)
        a[i] = 2 ** 32 + 1                       # (int32 conversion: 1, a valid action)
        _expect_invalid(venv, torch.from_numpy(a.reshape(shape)).cuda())
        _expect_invalid(venv, a.reshape(shape))  # and as a NumPy array, as SB3 hands actions over
    for whole in (good.astype(np.int64), good.astype(np.float64)):
        venv.step(torch.from_numpy(whole.reshape(shape)).cuda())
        venv.check_actions()
        venv.step(whole.reshape(shape))
        venv.check_actions()
    venv.close()


@pytest.mark.parametrize("C,tensors", [(1, False), (2, True)])
def test_discrete_vec_env_equals_engine(C, tensors):
    """200 steps of VecCarEnv(discrete_action_space=True) on random valid actions == BatchedCarEnv's discrete step
    with auto-reset on the same actions: obs, rewards, dones"""
    from nascargymnasium_amd import VecCarEnv
    from nascargymnasium_amd.batched import BatchedCarEnv
    venv = VecCarEnv(E, "martinsville", num_cars=C, discrete_action_space=True, return_tensors=tensors)
    ref = BatchedCarEnv(E, C, "martinsville", device="cuda:0")
    o = venv.reset()
    ro = ref.reset()
    o = o.cpu().numpy() if tensors else o
    assert np.array_equal(o.reshape(E, C, 38), ro.cpu().numpy())
    rng = np.random.default_rng(11)
    moved = 0
    for k in range(200):
        a = rng.integers(0, 5, (E, C))
        a[:, 0] = np.where(np.arange(E) % 2 == 0, 1, a[:, 0])          # half the envs keep the throttle open
        act = a if C > 1 else a[:, 0]                                   # int64, as MultiDiscrete.sample() gives
        obs, rew, done, infos = venv.step(torch.from_numpy(act).cuda() if tensors else act)
        robs, rrew, rterm, rtrunc = ref.step(torch.from_numpy(a.astype(np.int32)).cuda(), auto_reset=True)
        if tensors:
            obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
        assert np.array_equal(obs.reshape(E, C, 38), robs.cpu().numpy()), k
        assert np.array_equal(rew.reshape(E, C), rrew.cpu().numpy()), k
        assert np.array_equal(done, (rterm | rtrunc).cpu().numpy()), k
        moved = max(moved, float(np.abs(rrew.cpu().numpy()).max()))
    venv.check_actions()
    assert moved > 0
    venv.close(); ref.close()

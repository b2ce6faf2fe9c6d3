"""The inputs of tests/test_gpu_race_mlp.py, proved on the CPU oracle (tests/oracle_lib.py, car contact off): the trained
SAC / PPO controllers time a nascar_banked lap well inside the GPU tests' step caps, also when every action is perturbed
by twice the device actor's bound, and the constant drivers are disabled where the GPU tests expect their cars parked.
The GPU tests import their step caps from race_mlp_cases, as this file does, so the two cannot drift apart."""
import numpy as np
import pytest

import race_mlp_cases as rc
from race_mlp_cases import (ALL_TRACKS, FULL_THROTTLE_DISABLED_AT, LAP_HEADROOM, LAP_WINDOW, P2_STEPS, PARK_STEPS,
                            STUCK_DISABLED_AT, TT_STEPS)
from nascargymnasium_amd import policy as P

CAPS = {"time trial, policy 4": TT_STEPS, "time trial, policy 2": P2_STEPS}


@pytest.fixture(scope="module")
def banked_laps():
    """first-lap and disabled steps [run][slot] of [SAC, PPO, A2C] x 2 on nascar_banked: unperturbed, then two noise seeds"""
    field = [rc.sac_fixture(), rc.ac_fixture("ppo_849"), rc.ac_fixture("a2c_best_model3")] * 2
    return [rc.closed_loop("nascar_banked", field, min(CAPS.values()), seed) for seed in (None, 1, 2)]


def test_sac_and_ppo_lap_inside_the_step_caps(banked_laps):
    """Oracle: SAC's first lap at step 2595, PPO's at 2610 - 2611 in all three runs (A2C's, which no GPU precondition
    names, at 2588 - 2626).  The slots of tests 2 and 3 (SAC in slots 0 - 2, PPO in slot 2) start from the same grid
    point as these, car contact being off, so the slot does not enter."""
    laps = np.array([lap for lap, _ in banked_laps])            # [3 runs][6 slots]
    print("first laps", laps.tolist(), "disabled", [d.tolist() for _, d in banked_laps])
    sac_ppo = laps[:, [0, 1, 3, 4]]
    assert (sac_ppo > 0).all()
    assert sac_ppo.max() - sac_ppo.min() <= LAP_WINDOW
    for what, cap in CAPS.items():
        assert sac_ppo.max() + LAP_HEADROOM <= cap, what
    # slots 0 / 3 and 1 / 4 of the unperturbed run are the same car twice: a best-lap and fastest-lap tie by index
    assert laps[0, 0] == laps[0, 3] and laps[0, 1] == laps[0, 4]


@pytest.mark.parametrize("name", ALL_TRACKS)
def test_constant_drivers_are_disabled_where_expected(name):
    """(1, 0) is disabled at step 404 on martinsville and nowhere else within 900 steps; (0, 0) at step 600 everywhere
    (the stuck rule).  No lap is timed on the way."""
    lap, dis = rc.closed_loop(name, [(1.0, 0.0), (0.0, 0.0)], 900)
    assert dis[1] == STUCK_DISABLED_AT and not lap.any()
    assert dis[0] == (FULL_THROTTLE_DISABLED_AT if name == "martinsville" else 0)
    assert FULL_THROTTLE_DISABLED_AT + 40 <= PARK_STEPS < STUCK_DISABLED_AT


def test_full_throttle_controller_is_exact():
    """zero weights, b3 = (1, 0), clipped: (1, 0) by bits in float32 and float64, on every golden observation"""
    F = rc.full_throttle()
    obs = rc.golden_obs()
    for dt in (np.float32, np.float64):
        out = P.mlp_forward_numpy(F, obs, dt)
        assert out.shape == (len(obs), 2) and out.dtype == dt
        assert np.array_equal(out, np.tile(np.array([1, 0], dt), (len(obs), 1))) and not np.signbit(out).any()
    assert (F.h1, F.h2, F.activation) == (lambda c: (c.h1, c.h2, c.activation))(rc.ac_fixture("ppo_849"))   # one launch group
    assert rc.wide().output == P.OUT_MODE and rc.wide().w3.shape == (5, 512)

"""Coverage of the crowded scenes (tests/crowded.py), from the CPU oracle alone.

tests/test_gpu_crowded.py compares the device with the oracle on these scenes to pin b2_step's capacity paths; that
only means something while the scenes reach those paths.  Each condition below is one path's precondition, counted from
the oracle's contact counts and SolveTOI statistics with the cars grouped into waves as the step kernels group them;
a scene that stops covering a path fails here, without a GPU.  Floors are at most half of what the oracle shows.
"""
import numpy as np
import pytest

import crowded


@pytest.fixture(scope="module")
def tracks(tmp_path_factory):
    return tmp_path_factory.mktemp("crowded")


def _cov(tracks, sc):
    run = crowded.scene_run(tracks, sc)
    return run, crowded.coverage(run.stats, run.nct, run.active, crowded.wave_of(sc["E"], sc["C"], sc["epb"]))


def test_wave_of():
    """thread el * C + car of workgroup e // epb, 64 threads per wave"""
    w = crowded.wave_of(12, 10, 12)
    assert (w[..., 0] == 0).all() and w[6, 3, 1] == 0 and w[6, 4, 1] == 1 and w[..., 1].sum() == 120 - 64
    w = crowded.wave_of(128, 1, 128)
    assert (w[..., 0] == 0).all() and (w[:64, 0, 1] == 0).all() and (w[64:, 0, 1] == 1).all()
    w = crowded.wave_of(12, 10, 1)
    assert np.array_equal(w[..., 0], np.repeat(np.arange(12), 10).reshape(12, 10)) and (w[..., 1] == 0).all()
    w = crowded.wave_of(30, 4, 16)   # a partial last workgroup
    assert w[29, 3].tolist() == [1, (13 * 4 + 3) >> 6] and w[15, 3].tolist() == [0, 0] and w[16, 0].tolist() == [1, 0]


def test_actions_are_throttle_heavy():
    a = crowded.actions(np.random.default_rng(crowded.SEED), 12, 10)
    assert a.dtype == np.float32 and a.shape == (12, 10, 2)
    assert (a[..., 0] >= 0.4).all() and (a[..., 0] <= 1.0).all() and (np.abs(a[..., 1]) <= 0.6).all()


def test_coverage_counts_on_a_hand_made_run():
    """coverage() on 2 steps x 2 envs x 40 cars at 2 envs per workgroup (wave 0: env 0 + 24 cars of env 1)"""
    S, E, C = 2, 2, 40
    stats = np.zeros((S, E, C, 4), np.int32)
    nct = np.zeros((S, E, C), np.int32)
    stats[0, 0, :, 1] = 1          # step 0: 40 event contacts in env 0 ...
    stats[0, 1, :23, 1] = 0
    stats[0, 1, 30:, 1] = 3        # ... and 30 in wave 1: wave 0 above 32, wave 1 not
    stats[1, 1, 23, 0] = 4         # step 1: 4 TOUCHING calls in the last car of wave 0
    stats[1, 1, 24, 0] = 3         # and 3 in the first car of wave 1
    stats[1, 0, 5, 2:] = (3, 4)
    nct[1, 0, :7] = (5, 4, 3, 2, 17, 16, 0)
    cov = crowded.coverage(stats, nct, nct, crowded.wave_of(E, C, 2))
    assert (cov["mani_gt32"], cov["mani_gt3"], cov["touch_gt3"], cov["touch_gt64"]) == (1, 2, 1, 0)
    assert (cov["ct_gt4"], cov["ct_gt2"], cov["island3"], cov["events3"]) == (3, 5, 1, 1)
    assert (cov["max_nct"], cov["max_island"], cov["max_events"], cov["overflow"]) == (17, 4, 3, 1)
    assert crowded.first_overflow(nct) == 1 and crowded.first_overflow(nct[:1]) is None


def test_pocket40_12x10_covers_the_capacity_paths(tracks):
    """POCKET(40), 12 x 10 at 12 envs per workgroup (waves of 64 and 56 cars), 400 steps.  Measured:
      car-steps with n_contacts > 4 (CT_LDS_CAP)                  10 247   floor 5 000
      car-steps with toi_max_island >= 3                              79   floor 20
      (step, wave) with event contacts above 32 (MANI_JOBCAP)         46   floor 10
      car-steps with toi_events >= 3                                  76   exists
    and for the small-caps build (TOI_JOBCAP = MANI_JOBCAP = 3, CT_LDS_CAP = 2):
      (step, wave) with TOUCHING first-pass TOIs above 3              71   floor 15
      (step, wave) with event contacts above 3                       154   floor 40
      car-steps with n_contacts > 2                               11 718   floor 5 000
    Maxima: 12 contacts, 5 active collisions, islands of 5, 5 events per car and step, 128 event contacts and 33
    TOUCHING TOIs per wave (so the product build's TOI_JOBCAP of 64 is not provably exceeded: small-caps build only).
    At one env per workgroup (the third engine of the GPU test) a wave is one env's 10 cars: 7 pairs above 32."""
    run, cov = _cov(tracks, crowded.SCENES["12x10"])
    print(cov)
    assert cov["ct_gt4"] >= 5000 and cov["island3"] >= 20 and cov["mani_gt32"] >= 10 and cov["events3"] >= 1
    assert cov["touch_gt3"] >= 15 and cov["mani_gt3"] >= 40 and cov["ct_gt2"] >= 5000
    assert cov["overflow"] == 0 and cov["max_nct"] <= crowded.GPU_MAXC      # the scene must not overflow MAXC
    assert cov["max_island"] <= 8 and cov["max_events"] <= 8              # MAX_ISLAND / MAX_SUBSTEPS stay unreached
    # the rollout test starts crowded: at least 20 cars above 4 contacts in the state after ROLLOUT_START steps
    # (57 measured; none before step 290)
    assert int((run.nct[crowded.ROLLOUT_START - 1] > 4).sum()) >= 20


def test_pocket25_128x1_covers_the_capacity_paths(tracks):
    """POCKET(25), 128 x 1 at 128 envs per workgroup (two full waves of 64 one-car envs), 400 steps; every car
    starts from the same grid slot and reaches the curve around step 300 (at 300 steps no island of 3 and no wave
    above 32 event contacts occurs, so the scene runs 400).  Measured, floors at half:
      car-steps with n_contacts > 4                  6 596   floor 3 298
      car-steps with toi_max_island >= 3                63   floor 31
      (step, wave) with event contacts above 32         33   floor 16
      car-steps with toi_events >= 3                    26   floor 13
      (step, wave) with TOUCHING TOIs above 3           73   floor 36
      (step, wave) with event contacts above 3         127   floor 63
      car-steps with n_contacts > 2                  8 224   floor 4 112
    Maxima: 15 contacts (no overflow), islands of 6."""
    run, cov = _cov(tracks, crowded.SCENES["128x1"])
    print(cov)
    assert cov["ct_gt4"] >= 3298 and cov["island3"] >= 31 and cov["mani_gt32"] >= 16 and cov["events3"] >= 13
    assert cov["touch_gt3"] >= 36 and cov["mani_gt3"] >= 63 and cov["ct_gt2"] >= 4112
    assert cov["overflow"] == 0 and cov["max_nct"] <= crowded.GPU_MAXC
    assert cov["max_island"] <= 8 and cov["max_events"] <= 8


def test_pocket16_overflows_the_device_contact_buffer(tracks):
    """POCKET(16), 12 x 10, 500 steps: some car holds more than MAXC = 16 contacts (13 car-steps, up to 18, first at
    step k* = 318), none more than 23 (the oracle keeps OB_MAXC = 24, so the oracle itself never overflows), and some
    env (8 of 12) has no car above 16 through step k* + 50."""
    run, cov = _cov(tracks, crowded.OVERFLOW)
    print(cov)
    k = crowded.first_overflow(run.nct)
    assert k is not None and cov["overflow"] >= 1
    assert cov["max_nct"] <= 23
    assert k + 50 < run.steps
    clean = ~(run.nct[:k + 51] > crowded.GPU_MAXC).any((0, 2))
    assert clean.any() and not clean.all()

"""What tests/policy_cases.py's cases reach, checked on the host restatements alone (the actor's tile plan, the float64
forward), so that tests/test_gpu_policy_shapes.py cannot pass vacuously when a generator or the kernel's schedule
changes.

Measured with the committed generators (fixture observations, 2236 rows): the 12 default-init nets' raw means stay
within +-0.22; after standardised(k = 1) 50.0 % of every raw-mean component lies inside (-1, 1) for each net (max |mu|
7 .. 26); after k = 40 the share of rows with |mu| >= 10 is 80 .. 93 % per component.
"""
import numpy as np
import pytest

import policy_cases as PC
from nascargymnasium_amd import policy as P


def test_plan_constants_are_the_kernels():
    assert PC.header_define("ACT_WAVES") == PC.ACT_WAVES == 8
    assert PC.header_define("AM_WAVES") == PC.AM_WAVES == 4
    with open(PC.ACTOR_H) as f:
        shapes = f.read().split("#define MLP_SHAPES(X)")[1].split("\n")[0]
    assert tuple((32 * int(a), 32 * int(b)) for a, b in
                 (s.strip("() ").split(",") for s in shapes.split("X")[1:])) == PC.MLP_SHAPES
    assert len(PC.NETS) == len(set(PC.NETS)) == 12


def test_tile_plan_small_batches():
    """the regimes the older tests reach: 4096 rows are one tile per wave on 16 workgroups; 37 rows two tiles"""
    G, counts = PC.actor_tile_plan(4096, 256)
    assert G == 16 and counts.shape == (16, 8) and (counts == 1).all()
    G, counts = PC.actor_tile_plan(37, 256)
    assert G == 1 and counts[0].tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
    G, counts = PC.actor_tile_plan(1, 256)
    assert G == 1 and counts.sum() == 1
    G, counts = PC.actor_tile_plan(8192 * 10, 256)          # the README's workload: 2560 tiles, 10 per workgroup
    assert G == 256 and set(counts.ravel().tolist()) == {1, 2}


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_big_batches_reach_the_steady_state_loop(cus):
    n_a, n_b = PC.big_batch_sizes(cus)
    assert n_a > 32 * 8 * cus and n_b > 32 * 8 * cus
    G, ca = PC.actor_tile_plan(n_a, cus)
    assert G == cus
    assert (ca == 1).any() and (ca == 2).any() and ca.min() >= 1
    per_wg = ca.sum(1)
    assert set(per_wg.tolist()) == {8, 9}                   # uneven ntile * b / G split
    assert n_a % 32 == 27                                   # ragged last tile
    # the last tile belongs to a wave that has taken a tile before it: the clamped fetch is a prefetch
    last = (n_a + 31) // 32 - 1
    start = (last + 1) * (G - 1) // G
    assert last - start >= PC.ACT_WAVES
    G, cb = PC.actor_tile_plan(n_b, cus)
    assert G == cus and cb.min() >= 2 and cb.max() >= 3
    assert n_b % 32 == 1                                    # the last tile holds one row
    last = (n_b + 31) // 32 - 1
    assert last - (last + 1) * (G - 1) // G >= PC.ACT_WAVES
    if cus == 256:
        assert (n_a, n_b) == (69723, 164033)
    # every row of the base block is in both batches
    for n in (n_a, n_b):
        idx = PC.big_batch_index(n)
        assert idx.min() == 0 and idx.max() == PC.BASE_ROWS - 1 and len(np.unique(idx)) == PC.BASE_ROWS
        assert idx[PC.BASE_ROWS:2 * PC.BASE_ROWS].tolist() == idx[:PC.BASE_ROWS].tolist() and idx[1] == PC.STRIDE % PC.BASE_ROWS


@pytest.mark.parametrize("h1,h2,act", PC.NETS)
def test_standardised_nets_make_the_transforms_bite(h1, h2, act):
    obs = PC.fixture_obs()
    assert obs.shape == (2236, 38)
    c = PC.all_nets()[h1, h2, act]
    assert np.abs(P.mlp_forward_numpy(c, obs, np.float64)).max() < 1.0       # default init: clip would be the identity
    mu1 = P.mlp_forward_numpy(PC.standardised(c, obs, 1.0), obs, np.float64)
    inside = (np.abs(mu1) < 1).mean(0)
    assert ((inside >= 0.4) & (inside <= 0.6)).all(), inside
    mu40 = P.mlp_forward_numpy(PC.standardised(c, obs, 40.0), obs, np.float64)
    sat = (np.abs(mu40) >= 10).mean(0)
    assert (sat >= 0.5).all(), sat
    assert (mu40 >= 10).any() and (mu40 <= -10).any()                         # both signs saturate


def test_forward_sizes_straddle_the_tile_edges():
    t, w = 32, 32 * PC.AM_WAVES
    assert {t - 1, t, t + 1, w - 1, w, w + 1, 1} <= set(PC.FORWARD_SIZES) and max(PC.FORWARD_SIZES) == len(PC.fixture_obs())


@pytest.mark.parametrize("bounded", [False, True])
def test_grouped_field_groups(bounded):
    slots, ctrls = PC.grouped_field(bounded)
    assert len(slots) == 10 and slots[3] == "rule" and slots[8] == "uniform"
    net_slots = [(c, s) for c, s in enumerate(slots) if not isinstance(s, str)]
    assert sorted(s for _, s in net_slots) == list(range(len(ctrls))) and len(ctrls) <= 16
    assert all(s != c for c, s in net_slots)                          # id != position in the field
    assert all(s != 9 - c for c, s in net_slots)                      # ... nor in the reversed field
    assert any(c >= 5 for c, _ in net_slots)
    groups = PC.launch_groups(slots, ctrls)
    assert sorted(len(m) for _, m in groups) == [1, 3, 4]
    assert sum(len(m) >= 3 for _, m in groups) >= 2
    for _, members in groups:
        ids = [s for _, s in members]
        if len(ids) > 1:
            assert ids != sorted(ids)                                     # blockIdx.y order is not id order
        for i in range(len(ids)):
            for j in range(i + 1, len(ids)):
                a, b = ctrls[ids[i]], ctrls[ids[j]]
                assert not np.array_equal(a.w1, b.w1) and not np.array_equal(a.w3, b.w3)
    outs = [ctrls[s].output for _, s in net_slots]
    if bounded:
        assert set(outs) == {P.OUT_CLIP, P.OUT_SQUASH}
    else:
        assert set(outs) == {P.OUT_RAW, P.OUT_CLIP, P.OUT_SQUASH}
    # the columns of different nets differ on the observations the GPU test uses (float64 forward)
    obs = PC.fixture_obs()[:370].reshape(37, 10, 38)
    cols = [P.mlp_forward_numpy(ctrls[s], obs[:, c], np.float64) for c, s in net_slots]
    for i in range(len(cols)):
        for j in range(i + 1, len(cols)):
            assert np.abs(cols[i] - cols[j]).max() > 1e-2

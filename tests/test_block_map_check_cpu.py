"""tests/block_map_check.py must notice a wrong workgroup layout: the assertions the GPU tests hold block_map_kernel
to are fed maps with the defects that kernel could have (wrong maps are never run on the device: an env listed twice
or not at all sends the step kernels wrong)."""
import numpy as np
import pytest

from block_map_check import (assert_block_map, assert_every_env_once, distribution, expected_host_map, expected_map)

NT = 10
CASES = [(2500, 8, "round_robin"), (2500, 8, "skewed"), (1025, 5, "runs"), (1100, 12, "exact"), (301, 1, "single")]


def _device_map(ids, ntracks, epb, stale=-7):
    """a correct device map: the used prefix, then the fixed grid's empty workgroups (their env slots hold stale values)"""
    bt, be = expected_map(ids, ntracks, epb)
    nb = (len(ids) + epb - 1) // epb + ntracks
    pad = nb - len(bt)
    return (np.concatenate([bt, np.full(pad, -1, np.int32)]),
            np.concatenate([be, np.full((pad, epb), stale, np.int32)]))


@pytest.mark.parametrize("E,epb,dist", CASES)
def test_correct_maps_pass(E, epb, dist):
    ids = distribution(dist, E, NT, epb, seed=4)
    bt, be = _device_map(ids, NT, epb)
    assert_block_map(bt, be, ids, NT, epb)
    assert_every_env_once(bt, be, E)
    ht, he = expected_host_map(ids, NT, epb)
    assert_block_map(ht, he, ids, NT, epb, fixed_grid=False, host_order=True)
    assert sorted(map(tuple, np.c_[ht, he])) == sorted(map(tuple, np.c_[expected_map(ids, NT, epb)]))


def test_distributions_are_what_the_gpu_tests_need():
    ids = distribution("exact", 1100, 8, 12, seed=1)
    n = np.bincount(ids, minlength=8)
    assert n[1] == 24 and n[2] == 25                        # k epb and k epb + 1
    ids = distribution("single", 2048, 8, 5)
    assert (np.bincount(ids, minlength=8) == [0, 0, 0, 2048, 0, 0, 0, 0]).all()
    ids = distribution("runs", 8192, 8, 5)                  # a fast-path thread's 8 envs share a track
    assert (ids.reshape(1024, 8) == ids.reshape(1024, 8)[:, :1]).all()
    ids = distribution("skewed", 5000, 8, 5, seed=2)
    n = np.bincount(ids, minlength=8)
    assert n.max() > 4 * max(1, n.min()) and n.sum() == 5000


def _fails(bt, be, ids, epb, once=None):
    with pytest.raises(AssertionError):
        assert_block_map(bt, be, ids, NT, epb)
    if once is not None:
        if once:
            with pytest.raises(AssertionError, match="exactly once"):
                assert_every_env_once(bt, be, len(ids))
        else:
            assert_every_env_once(bt, be, len(ids))         # (the layout assertion alone sees this defect)


@pytest.mark.parametrize("E,epb,dist", [c for c in CASES if c[1] > 1])
def test_two_envs_swapped_inside_a_workgroup(E, epb, dist):
    ids = distribution(dist, E, NT, epb, seed=4)
    bt, be = _device_map(ids, NT, epb)
    w = int(np.nonzero((be >= 0).sum(axis=1) >= 2)[0][-1])
    be[w, [0, 1]] = be[w, [1, 0]]
    _fails(bt, be, ids, epb, once=False)


@pytest.mark.parametrize("E,epb,dist", CASES)
def test_one_env_duplicated_over_another(E, epb, dist):
    ids = distribution(dist, E, NT, epb, seed=4)
    bt, be = _device_map(ids, NT, epb)
    used = np.nonzero(bt >= 0)[0]
    be[used[-1], 0] = be[used[0], 0]
    _fails(bt, be, ids, epb, once=True)
    bt, be = _device_map(ids, NT, epb)                      # the same env of the same track, one slot on
    be[used[0], 0] = be[used[1], 0] if epb == 1 else be[used[0], 1]
    _fails(bt, be, ids, epb, once=True)


def _ranked_by_chunks(ids, ntracks, epb, carry, tails=True, stale=None):
    """the generic path's construction: 1024-env chunks, an env's slot = its track's first slot + the count of the
    track's envs in earlier chunks (carry; False: restarted from 0 in every chunk) + its rank within the chunk"""
    E = len(ids)
    cnt = np.bincount(ids, minlength=ntracks)
    nbt = (cnt + epb - 1) // epb
    boff = np.concatenate([[0], np.cumsum(nbt)])
    nb = (E + epb - 1) // epb + ntracks
    be = (np.full(nb * epb, -7, np.int32) if stale is None else stale.ravel().copy())
    bt = np.full(nb, -1, np.int32)
    for t in range(ntracks):
        bt[boff[t]:boff[t + 1]] = t
        if tails:
            be[boff[t] * epb + cnt[t]:boff[t + 1] * epb] = -1
    run = np.zeros(ntracks, np.int64)
    for c0 in range(0, E, 1024):
        seen = np.zeros(ntracks, np.int64)
        for e in range(c0, min(E, c0 + 1024)):
            t = ids[e]
            be[boff[t] * epb + (run[t] if carry else 0) + seen[t]] = e
            seen[t] += 1
        run += seen
    return bt, be.reshape(nb, epb)


@pytest.mark.parametrize("E,epb,dist", [(2500, 8, "round_robin"), (2500, 8, "skewed"), (1025, 5, "runs"),
                                        (1025, 1, "single")])
def test_second_chunk_ranks_restarted(E, epb, dist):
    ids = distribution(dist, E, NT, epb, seed=4)
    bt, be = _ranked_by_chunks(ids, NT, epb, carry=True)
    assert_block_map(bt, be, ids, NT, epb)                  # the construction itself is right with the carry ...
    bt, be = _ranked_by_chunks(ids, NT, epb, carry=False)   # ... and wrong without: chunk 2 lands on chunk 1's slots
    _fails(bt, be, ids, epb, once=True)


@pytest.mark.parametrize("E,epb,dist", [(2500, 8, "round_robin"), (1100, 12, "exact"), (1025, 5, "skewed")])
def test_tail_slot_left_unfilled(E, epb, dist):
    ids = distribution(dist, E, NT, epb, seed=4)
    prev = distribution("skewed", E, NT, epb, seed=9)       # the map before: its env ids are what an unfilled slot keeps
    _, stale = _ranked_by_chunks(prev, NT, epb, carry=True)
    bt, be = _ranked_by_chunks(ids, NT, epb, carry=True, tails=True, stale=stale)
    assert_block_map(bt, be, ids, NT, epb)
    bt, be = _ranked_by_chunks(ids, NT, epb, carry=True, tails=False, stale=stale)
    _fails(bt, be, ids, epb)
    bt, be = _device_map(ids, NT, epb)                      # one tail slot holding an env of the same workgroup
    w = int(np.nonzero((be == -1).any(axis=1) & (bt >= 0))[0][0])
    be[w, -1] = be[w, 0]
    _fails(bt, be, ids, epb, once=True)


def test_grid_length_and_empty_workgroups():
    E, epb = 301, 5
    ids = distribution("round_robin", E, NT, epb)
    bt, be = _device_map(ids, NT, epb)
    with pytest.raises(AssertionError):
        assert_block_map(bt[:-1], be[:-1], ids, NT, epb)    # a grid one workgroup short
    bt[-1] = 0                                              # a workgroup past the used prefix that is not empty
    with pytest.raises(AssertionError, match="past the used prefix"):
        assert_block_map(bt, be, ids, NT, epb)
    ht, he = expected_host_map(ids, NT, epb)
    with pytest.raises(AssertionError):                     # the track-major order is not the host's interleaved one
        assert_block_map(*expected_map(ids, NT, epb), ids, NT, epb, fixed_grid=False, host_order=True)
    assert_block_map(ht, he, ids, NT, epb, fixed_grid=False, host_order=True)

"""The workgroup layout of random-track mode restated in NumPy, and the assertions the GPU tests hold
block_map_kernel's output to (tests/test_gpu_block_map.py, tests/test_gpu_random_tracks.py).  No device code here:
tests/test_block_map_check_cpu.py feeds these assertions wrong maps and sees each one fail."""
import numpy as np


def expected_map(ids, ntracks, epb):
    """the layout block_map_kernel must build: tracks in id order, each track's envs in ascending order in whole
    workgroups of epb envs (the last one padded with -1)"""
    bt, be = [], []
    for t in range(ntracks):
        envs = np.nonzero(ids == t)[0].tolist()
        for i in range(0, len(envs), epb):
            bt.append(t)
            chunk = envs[i:i + epb]
            be.append(chunk + [-1] * (epb - len(chunk)))
    return np.array(bt, np.int32), np.array(be, np.int32).reshape(-1, epb)


def expected_host_map(ids, ntracks, epb):
    """the layout the host builds outside random-track mode (prepare()): the same workgroups, workgroup i of a track
    with n of them sorted at (i + 1/2) / n over all tracks (stable: ties keep the track-major order)"""
    bt, be = expected_map(ids, ntracks, epb)
    key = np.zeros(len(bt))
    for t in range(ntracks):
        w = np.nonzero(bt == t)[0]
        key[w] = (np.arange(len(w)) + 0.5) / max(1, len(w))
    order = np.argsort(key, kind="stable")
    return bt[order], be[order]


def assert_block_map(bt, be, ids, ntracks, epb, fixed_grid=True, host_order=False):
    """(bt [nb], be [nb, epb]) is the layout of the env -> track map `ids`:
    the grid length (random-track mode's fixed grid: ceil(E / epb) + ntracks), the used prefix exactly the expected
    workgroups, every workgroup past it empty (track -1), and every env id 0..E-1 listed exactly once"""
    ids = np.asarray(ids)
    bt, be = np.asarray(bt), np.asarray(be)
    E = len(ids)
    want_t, want_e = (expected_host_map if host_order else expected_map)(ids, ntracks, epb)
    n = len(want_t)
    assert be.shape == (len(bt), epb), (be.shape, len(bt), epb)
    if fixed_grid:
        assert len(bt) == (E + epb - 1) // epb + ntracks, (len(bt), E, epb, ntracks)
    else:
        assert len(bt) == n, (len(bt), n)
    assert np.array_equal(bt[:n], want_t), f"workgroup tracks differ first at workgroup {_first_diff(bt[:n], want_t)}"
    assert (bt[n:] == -1).all(), f"workgroups past the used prefix ({n}) are not all empty: {bt[n:]}"
    assert np.array_equal(be[:n], want_e), f"env slots differ first at workgroup {_first_diff(be[:n], want_e)}"
    assert_every_env_once(bt, be, E)


def _first_diff(a, b):
    if a.shape != b.shape:
        return f"(shapes {a.shape} / {b.shape})"
    d = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
    return int(d[0]) if d.size else None


def assert_every_env_once(bt, be, E):
    """the separate statement of "no env missing (it would never step), none twice (two workgroups would step it)":
    over the workgroups the kernels run (track >= 0), every env id 0..E-1 occurs exactly once in blk_env"""
    bt, be = np.asarray(bt), np.asarray(be)
    listed = be[bt >= 0].ravel()
    listed = listed[listed >= 0]
    assert listed.size == 0 or listed.max() < E, f"env id {listed.max()} out of range"
    times = np.bincount(listed, minlength=E)
    assert (times == 1).all(), (f"envs not listed exactly once: missing {np.nonzero(times == 0)[0][:8].tolist()}, "
                                f"repeated {np.nonzero(times > 1)[0][:8].tolist()}")


# ------------------------------------------------------------------ env -> track distributions of the tests
def distribution(name, E, ntracks, epb, seed=0):
    """per-env track index (0..ntracks-1) of the named distribution"""
    e = np.arange(E)
    if name == "round_robin":
        return (e % ntracks).astype(np.int32)
    if name == "single":        # all envs on track 3: the tracks in front of it and behind it have zero envs
        return np.full(E, 3, np.int32)
    if name == "runs":          # contiguous runs: a fast-path thread's R consecutive envs share a track
        return (e * ntracks // E).astype(np.int32)
    if name == "skewed":        # seeded, most envs on few tracks, possibly none on some
        rng = np.random.default_rng(seed)
        p = rng.dirichlet(np.full(ntracks, 0.4))
        return rng.choice(ntracks, size=E, p=p).astype(np.int32)
    if name == "exact":         # track 1 fills its last workgroup exactly (2 epb envs), track 2 has one env more
        ids = np.empty(E, np.int32)
        n1, n2 = 2 * epb, 2 * epb + 1
        assert E >= n1 + n2 + 1
        rest = np.array([t for t in range(ntracks) if t not in (1, 2)], np.int32)
        ids[:] = rest[e % len(rest)]
        rng = np.random.default_rng(seed)
        pick = rng.permutation(E)[:n1 + n2]
        ids[pick[:n1]] = 1
        ids[pick[n1:]] = 2
        return ids
    raise ValueError(name)

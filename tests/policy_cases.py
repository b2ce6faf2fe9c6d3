"""Cases for the policy-inference kernels of csrc/nascar_actor.h (actor_kernel, actor_mfma32_kernel, mlp_field_kernel)
at the shapes where they take another path.  TEST INFRASTRUCTURE: plain numpy, importable without a GPU.

  actor_tile_plan   the persistent bf16 actor's schedule restated: which (workgroup, wave) takes how many 32-row tiles
  big_batch_sizes   two batch sizes that put actor_kernel into its steady-state loop (waves with 2 and 3 tiles, the
                    prefetch of the next tile taken, uneven workgroup ranges, a ragged last tile)
  all_nets          one random controller per mlp_field_kernel instantiation (MLP_SHAPES x {ReLU, Tanh})
  standardised      a controller whose output layer is rescaled so that the clip and squash transforms bite
  grouped_field     a 10-slot field whose launches hold several different controllers of one shape each

What the cases reach is checked on the host alone by tests/test_policy_cases_cpu.py; tests/test_gpu_policy_shapes.py
runs the device on them.
"""
import os
import re

import numpy as np

from nascargymnasium_amd import policy as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTOR_H = os.path.join(ROOT, "nascargymnasium_amd", "csrc", "nascar_actor.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "sac_1235_actor.npz")

ACT_WAVES = 8        # waves per actor_kernel workgroup
AM_WAVES = 4         # waves per actor_mfma32_kernel / mlp_field_kernel workgroup
MLP_SHAPES = ((256, 256), (256, 128), (256, 32), (128, 128), (64, 64), (32, 256))
NETS = tuple((h1, h2, act) for h1, h2 in MLP_SHAPES for act in (P.RELU, P.TANH))
BASE_ROWS = 4096     # the block the big batches are drawn from: the largest batch of tests/test_gpu_actor.py
STRIDE = 7919        # prime, coprime with BASE_ROWS: row i of a big batch is row (i * STRIDE) % BASE_ROWS of the block
FORWARD_SIZES = (1, 31, 32, 33, 127, 128, 129, 2236)   # around one wave's tile (32) and one workgroup (AM_WAVES * 32)


def header_define(name):
    """the value of `#define name <int>` in csrc/nascar_actor.h"""
    with open(ACTOR_H) as f:
        m = re.search(r"^#define\s+%s\s+(\d+)\b" % re.escape(name), f.read(), re.M)
    if not m:
        raise LookupError(f"no #define {name} in {ACTOR_H}")
    return int(m.group(1))


def actor_tile_plan(n, cus, waves=ACT_WAVES):
    """actor_kernel's schedule for n rows on a device of `cus` CUs (nascar_kernels.hip actor_grid and the kernel's tile
    loop): the grid G = min(ceil(n / (32 * waves)), cus), at least 1; workgroup b owns the tiles [ntile * b // G,
    ntile * (b + 1) // G) and its wave w takes start + w, start + w + waves, ...  Returns (G, counts[G, waves])."""
    ntile = (n + 31) // 32
    G = max(1, min((n + 32 * waves - 1) // (32 * waves), cus))
    counts = np.zeros((G, waves), np.int64)
    for b in range(G):
        start, end = ntile * b // G, ntile * (b + 1) // G
        for w in range(waves):
            counts[b, w] = len(range(start + w, end, waves))
    assert counts.sum() == ntile
    return G, counts


def big_batch_sizes(cus):
    """(n_a, n_b).  n_a: 8 cus + cus // 2 + 3 tiles, so workgroups of 8 and of 9 tiles -- waves with one tile beside
    waves with two -- and a last tile of 27 rows.  n_b: 20 cus + 7 tiles, workgroups of 20 and 21 -- every wave takes 2
    or 3 -- and a last tile of one row."""
    return 32 * (8 * cus + cus // 2 + 3) - 5, 32 * (20 * cus + 7) - 31


def big_batch_index(n):
    """rows of the BASE_ROWS block that make up a big batch of n rows"""
    return (np.arange(n, dtype=np.int64) * STRIDE) % BASE_ROWS


def fixture_obs():
    """the 2236 golden-trace observations of the sac_1235 fixture"""
    return np.load(FIXTURE)["obs"]


def all_nets(output=P.OUT_RAW):
    """{(h1, h2, activation): random controller} for the 12 mlp_field_kernel instantiations"""
    return {(h1, h2, act): P.random_mlp(h1, h2, act, output, seed=h1 + h2 + act) for h1, h2, act in NETS}


def standardised(ctrl, obs, k=1.0):
    """`ctrl` with w3' = w3 * k / MAD and b3' = (b3 - median) * k / MAD per output component, the median and the median
    absolute deviation taken from the float64 raw means on `obs`: the new raw mean is k * (mu - median) / MAD, so at
    k = 1 half of each component lies inside (-1, 1) -- where clip and squash are not the identity for the other half
    -- and at k = 40 most rows saturate.  (Default-init nets give raw means within +-0.25: clip does nothing there.)"""
    mu = P.mlp_forward_numpy(ctrl, obs, np.float64, output=P.OUT_RAW)
    med = np.median(mu, axis=0)
    mad = np.median(np.abs(mu - med), axis=0)
    w3 = (ctrl.w3.astype(np.float64) * (k / mad)[:, None]).astype(np.float32)
    b3 = ((ctrl.b3.astype(np.float64) - med) * (k / mad)).astype(np.float32)
    return ctrl._replace(w3=w3, b3=b3)


def grouped_field(bounded=False):
    """(slots, controllers) of the grouped-launch field: slots = [A0, B0, A1, "rule", A2, B1, C0, A3, "uniform", B2] with
    every network given as its index into `controllers`, the order in which they are to be added (so the index is the
    id add_controller returns).  A0-A3: four 64-64 Tanh nets (raw / clip / squash / clip), B0-B2: three 256-128 ReLU
    nets (squash / clip / raw), C0: one 128-128 ReLU net (clip); all standardised (k = 1) on the fixture observations so
    that their transforms differ.  launch_field packs the A nets into one launch (4 slots), the B nets into another
    (3) and C0 into a third.  The add order makes every id differ from its slot, also in the reversed field, and no
    group's ids ascend with its slots.  bounded=True: raw outputs become clip, for a field that drives an env."""
    obs = fixture_obs()
    raw = P.OUT_CLIP if bounded else P.OUT_RAW

    def net(h1, h2, act, out, seed):
        return standardised(P.random_mlp(h1, h2, act, out, seed=seed), obs)
    A = [net(64, 64, P.TANH, out, 100 + i) for i, out in enumerate((raw, P.OUT_CLIP, P.OUT_SQUASH, P.OUT_CLIP))]
    B = [net(256, 128, P.RELU, out, 200 + i) for i, out in enumerate((P.OUT_SQUASH, P.OUT_CLIP, raw))]
    C0 = net(128, 128, P.RELU, P.OUT_CLIP, 300)
    controllers = [A[1], B[1], B[2], A[0], A[3], B[0], A[2], C0]
    slots = [3, 5, 0, "rule", 6, 1, 7, 4, "uniform", 2]
    return slots, controllers


def launch_groups(slots, controllers):
    """the launches launch_field makes for a field: [(h1, h2, activation), [(slot, id), ...]] in launch order"""
    groups = {}
    for c, s in enumerate(slots):
        if isinstance(s, str):
            continue
        k = controllers[s]
        groups.setdefault((k.h1, k.h2, k.activation), []).append((c, s))
    return list(groups.items())

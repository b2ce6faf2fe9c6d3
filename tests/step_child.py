"""Child process of tests/test_gpu_crowded.py::test_small_caps_build_identical: the given actions stepped through the
library named by NASCAR_LIB (a tools variant build) at `epb` envs per workgroup, through the fused model + logic kernel
and the two-launch path; per-step obs, reward and flags and the final state of both written to an .npz file.
    NASCAR_LIB=<variant.so> python tests/step_child.py <track> <E> <C> <epb> <actions.npy> <out.npz>"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from nascargymnasium_amd import _lib
    import crowded
    path, E, C, epb, af, of = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], sys.argv[6]
    assert os.path.samefile(_lib.LIB_PATH, os.environ["NASCAR_LIB"])
    acts = np.load(af)
    out = {}
    for name, fused in (("fused", True), ("unfused", False)):
        r = crowded.device_run(path, E, C, epb, fused, acts)
        for key in ("obs", "reward", "car_flags", "env_flags", "state"):
            out[f"{name}_{key}"] = r[key]
    np.savez(of, **out)


if __name__ == "__main__":
    main()

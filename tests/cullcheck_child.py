"""Child process of tests/test_gpu_b2_prims.py::test_cull_check_in_situ: the given actions stepped through the counting
check build named by NASCAR_LIB (tools/build/libnascar_cullcheck.so: -DNASCAR_PROFILE -DNASCAR_PROFILE_COUNT
-DNASCAR_TOI_CULL_CHECK), which runs every b2TimeOfImpact call the exact cull skips and counts the TOUCHING ones; the
three counters and the per-step obs written to an .npz file.
    NASCAR_LIB=<cullcheck.so> python tests/cullcheck_child.py <track> <E> <C> <epb> <actions.npy> <out.npz>"""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# the profile buffer's layout (csrc/nascar_device.h; tools/phase_profile.py allocates the same words)
NW = 65536
COUNTERS = 2 * NW * 16
APROF_BASE = COUNTERS + 64
LPROF_BASE = APROF_BASE + 4096 * 16
CPROF_BASE = LPROF_BASE + NW * 16
RPROF_BASE = CPROF_BASE + (1 << 19) * 48
TCAP_BASE, TCAP_MAX = RPROF_BASE + 65536 * 5, 16384


def main():
    import torch
    from nascargymnasium_amd import _lib
    import crowded
    path, E, C, epb, af, of = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], sys.argv[6]
    assert os.path.samefile(_lib.LIB_PATH, os.environ["NASCAR_LIB"])
    L = _lib.lib()
    L.nascar_debug_profile.argtypes = [ctypes.c_void_p]
    L.nascar_debug_profile.restype = ctypes.c_int
    buf = torch.zeros(TCAP_BASE + 8 + TCAP_MAX * 8, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    _lib.check(L.nascar_debug_profile(ctypes.c_void_p(buf.data_ptr())))
    r = crowded.device_run(path, E, C, epb, True, np.load(af))
    torch.cuda.synchronize()
    counts = buf[COUNTERS:COUNTERS + 16].cpu().numpy()
    _lib.check(L.nascar_debug_profile(ctypes.c_void_p(0)))
    np.savez(of, counts=counts, obs=r["obs"])


if __name__ == "__main__":
    main()

"""Record the workspace sizes a built libcgps.so reports, as the table tests/test_plan.py holds the library to.

    python tests/golden/make_workspace_sizes.py <path to the libcgps.so of the commit to record> [out.npz]

The table is taken from the commit BEFORE a change to the sizing code, never from the code under test.  The calls
need no GPU.  Stored: the grids (N, d, dtype code, op, nrhs) and two uint64 arrays,
  sizes[op, dtype, d - 1, N]              cgps_workspace_bytes, ops 0..8
  sweep_sizes[op - 2, nrhs, dtype, d - 1, N]   cgps_solve_workspace_bytes, ops HALFSOLVE / BACKSOLVE / SOLVE
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def n_grid():
    """The thresholds the plans branch on, each with its neighbours."""
    ns = [1, 2, 3, 4, 5, 7, 8, 31, 32, 33, 127, 128, 129, 255, 256, 257, 502, 1000, 1023, 1024, 1025]
    for c in (32768, 65408, 131072, 262144):
        ns += [c - 1, c, c + 1]
    ns += [2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 2 ** 21 + 3, 2 ** 24 + 5]
    return ns


OPS = list(range(9))
SWEEP_OPS = [2, 3, 4]
NRHS = [2, 3, 4, 5, 8, 9, 17]
DS = list(range(1, 9))
DTYPES = [0, 1]          # CGPS_F32, CGPS_F64


def record(lib_path):
    lib = ctypes.CDLL(lib_path)
    i64, sz = ctypes.c_int64, ctypes.c_size_t
    lib.cgps_workspace_bytes.argtypes = [i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(sz)]
    lib.cgps_solve_workspace_bytes.argtypes = [i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.POINTER(sz)]
    ns = n_grid()
    sizes = np.zeros((len(OPS), len(DTYPES), len(DS), len(ns)), dtype=np.uint64)
    sweeps = np.zeros((len(SWEEP_OPS), len(NRHS), len(DTYPES), len(DS), len(ns)), dtype=np.uint64)
    b = sz(0)
    for it, dt in enumerate(DTYPES):
        for idd, d in enumerate(DS):
            for i, n in enumerate(ns):
                for io, op in enumerate(OPS):
                    assert lib.cgps_workspace_bytes(n, d, dt, op, ctypes.byref(b)) == 0
                    sizes[io, it, idd, i] = b.value
                for io, op in enumerate(SWEEP_OPS):
                    for ir, m in enumerate(NRHS):
                        assert lib.cgps_solve_workspace_bytes(n, d, dt, op, m, ctypes.byref(b)) == 0
                        sweeps[io, ir, it, idd, i] = b.value
    return dict(version=np.int64(lib.cgps_version()), N=np.array(ns, dtype=np.int64), d=np.array(DS), dtype=np.array(DTYPES),
                op=np.array(OPS), sweep_op=np.array(SWEEP_OPS), nrhs=np.array(NRHS), sizes=sizes, sweep_sizes=sweeps)


if __name__ == "__main__":
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "workspace_sizes.npz")
    np.savez_compressed(out, **record(sys.argv[1]))
    print("wrote", out, os.path.getsize(out), "bytes")

"""The host-side plans (csrc/cgps_plan.h): the workspace sizes are those of the commit before the plan header,
to the byte, and everything a pass writes fits the region the plan hands it.  CPU only."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

from cyclic_gps import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "cyclic-gps_amd", "csrc")


def test_workspace_sizes_are_those_of_the_recorded_table():
    """tests/golden/workspace_sizes.npz was written by golden/make_workspace_sizes.py from the library of the commit
    before cgps_plan.h: every op, d = 1..8, both dtypes, the thresholds the plans branch on and their neighbours."""
    g = np.load(os.path.join(HERE, "golden", "workspace_sizes.npz"))
    lib = _hip.lib()
    assert int(g["version"]) == lib.cgps_version() == 320
    assert len(g["N"]) >= 38 and list(g["d"]) == list(range(1, 9)) and list(g["op"]) == list(range(9))
    b = ctypes.c_size_t(0)
    bad = []
    for it, dt in enumerate(g["dtype"]):
        for idd, d in enumerate(g["d"]):
            for i, n in enumerate(g["N"]):
                for io, op in enumerate(g["op"]):
                    assert lib.cgps_workspace_bytes(int(n), int(d), int(dt), int(op), ctypes.byref(b)) == 0
                    if b.value != int(g["sizes"][io, it, idd, i]):
                        bad.append(("op", int(op), int(dt), int(d), int(n), b.value, int(g["sizes"][io, it, idd, i])))
                for io, op in enumerate(g["sweep_op"]):
                    for ir, m in enumerate(g["nrhs"]):
                        assert lib.cgps_solve_workspace_bytes(int(n), int(d), int(dt), int(op), int(m), ctypes.byref(b)) == 0
                        if b.value != int(g["sweep_sizes"][io, ir, it, idd, i]):
                            bad.append(("sweep", int(op), int(m), int(dt), int(d), int(n), b.value,
                                        int(g["sweep_sizes"][io, ir, it, idd, i])))
    assert not bad, bad[:10]


def _host_compiler():
    for cxx in ("c++", "g++", "clang++"):
        if shutil.which(cxx):
            return [shutil.which(cxx)]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return [hipcc, "-x", "c++"]          # as a plain host compiler: no HIP language, no device pass


def test_every_pass_writes_inside_its_region(tmp_path):
    """tests/plan_check.cpp includes cgps_plan.h alone and is built by a plain C++17 host compiler (the header is
    host-pure); it walks every plan over N = 1..3000 and the thresholds, d = 1..8, both scalar sizes, every panel
    width and CU counts 1 / 64 / 256 / 304."""
    exe = str(tmp_path / "plan_check")
    subprocess.run(_host_compiler() + ["-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(HERE, "plan_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " 0 failed" in r.stdout

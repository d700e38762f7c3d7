"""The generator specification without a GPU: csrc/cgps_rng.h, built alone by a host compiler, against the numpy
restatement of the specification (tests/_rngref.py) and the recorded anchors; the sampling entry points are declared,
bound and exported; their host-side arithmetic (workspace size, argument checks) runs before any HIP call.

Tolerances: Philox words bit-exact.  fp64 normals 1e-13, fp32 normals 1e-5 against the float64 evaluation of the same
u1, u2: accurate libm calls differ by a few ulp at |z| <= 8.6 (fp64: 8.6 * 2^-52 ~ 2e-15) and 5.8 (fp32: 5.8 * 2^-23 ~
7e-7), so both bounds leave more than a factor of ten; approximate intrinsics (1e-6 relative and worse) do not pass."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _rngref
from cyclic_gps import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "cyclic-gps_amd", "csrc")
NEW = ("cgps_normal_fill", "cgps_sample_workspace_bytes", "cgps_sample")


def test_reference_reproduces_the_recorded_anchors():
    for counter, key, words in _rngref.KNOWN_ANSWERS:
        assert tuple(int(w) for w in _rngref.philox4x32_10(counter, key)) == words
    z = _rngref.standard_normal(2, 3, 2024)
    np.testing.assert_allclose(z, [[0.99998332, -0.09707062, -1.47733487], [1.16680506, -0.87152559, -0.58234695]], atol=5e-9)
    z = _rngref.standard_normal(2, 5, 2024, dtype=np.float32)
    np.testing.assert_allclose(z, [[-0.11691724, 0.99785749, 0.15243754, 0.08834561, -1.05520091],
                                   [-1.33981186, 0.57087217, -0.45224312, 0.10429369, 1.55538017]], atol=5e-9)
    # a column never depends on how many are asked for; rows are addressed by their index
    for dt in (np.float64, np.float32):
        wide = _rngref.standard_normal(7, 9, 5, stream=3, dtype=dt)
        for c in (1, 2, 3, 4, 5, 8):
            np.testing.assert_array_equal(_rngref.standard_normal(7, c, 5, stream=3, dtype=dt), wide[:, :c])
        np.testing.assert_array_equal(_rngref.standard_normal(3, 9, 5, stream=3, dtype=dt, row0=4), wide[4:])


def _host_compiler():
    for cxx in ("c++", "g++", "clang++"):
        if shutil.which(cxx):
            return [shutil.which(cxx)]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return [hipcc, "-x", "c++"]          # as a plain host compiler: no HIP language, no device pass


def test_header_built_by_a_host_compiler_matches_the_reference(tmp_path):
    exe = str(tmp_path / "rng_check")
    subprocess.run(_host_compiler() + ["-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(HERE, "rng_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")
    kat = [tuple(int(w, 16) for w in ln.split()[1:]) for ln in lines if ln.startswith("kat")]
    assert kat == [k[2] for k in _rngref.KNOWN_ANSWERS]
    for tag, dt, tol in (("f64", np.float64, 1e-13), ("f32", np.float32, 1e-5)):
        got = np.full((64, 9), np.nan)
        for ln in lines:
            if ln.startswith(tag):
                _, i, j, v = ln.split()
                got[int(i), int(j)] = float(v)
        ref = _rngref.standard_normal(64, 9, 2024, dtype=dt)
        err = float(np.abs(got - ref).max())
        print(tag, "max |header - reference| = %.3g (bound %.0e)" % (err, tol))
        assert err <= tol, (tag, err)                      # (NaN: a value the program did not print)


def test_new_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cgps.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _hip.exported_symbols(), name
        assert hasattr(lib, name), name
    assert _hip.lib().cgps_version() == 320


def test_sample_workspace_sizes():
    lib = _hip.lib()
    b = ctypes.c_size_t(0)
    sizes = {}
    for dt, s in ((_hip.F32, 4), (_hip.F64, 8)):
        for d in range(1, 9):
            for n in (1, 2, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1000, 4097, 70001, 2 ** 20, 2 ** 20 + 1):
                for m in (1, 2, 3, 8, 9, 1000):
                    assert lib.cgps_sample_workspace_bytes(n, d, dt, m, ctypes.byref(b)) == 0, (dt, d, n, m)
                    assert b.value >= 256 and b.value % 256 == 0
                    # never more than a fifth of the samples themselves (plus rounding of the slices)
                    chunks = min((m + 7) // 8, 128)
                    assert b.value <= n * d * 8 * chunks * s // 5 + 512 * chunks + 256, (dt, d, n, m, b.value)
                    sizes[dt, d, n, m] = b.value
    # a system one tile takes to the end needs no coarse-solution buffers
    assert sizes[_hip.F64, 4, 128, 8] == 256 and sizes[_hip.F64, 4, 512, 2] == 256
    # all chunks of a pass in one launch: a slice per chunk, up to the fixed group of 128 chunks
    assert sizes[_hip.F64, 4, 70001, 1000] == 125 * sizes[_hip.F64, 4, 70001, 8]
    assert lib.cgps_sample_workspace_bytes(70001, 4, _hip.F64, 8 * 128, ctypes.byref(b)) == 0
    full = b.value
    assert lib.cgps_sample_workspace_bytes(70001, 4, _hip.F64, 8 * 500, ctypes.byref(b)) == 0 and b.value == full


def test_argument_errors_before_any_hip_call():
    lib = _hip.lib()
    b = ctypes.c_size_t(0)
    assert lib.cgps_sample_workspace_bytes(0, 4, _hip.F64, 8, ctypes.byref(b)) == 1
    assert lib.cgps_sample_workspace_bytes(8, 4, _hip.F64, 0, ctypes.byref(b)) == 1
    assert lib.cgps_sample_workspace_bytes(8, 4, _hip.F64, 8, None) == 1
    assert lib.cgps_sample_workspace_bytes(8, 9, _hip.F64, 8, ctypes.byref(b)) == 3
    assert lib.cgps_sample_workspace_bytes(8, 4, 7, 8, ctypes.byref(b)) == 3
    host = (ctypes.c_double * 64)()                        # a non-null address; nothing gets as far as reading it
    p = ctypes.cast(host, ctypes.c_void_p)
    assert lib.cgps_sample(None, None, None, 8, 4, _hip.F64, 8, None, 1, 0, None, None, 0, None) == 1
    assert lib.cgps_sample(p, p, p, 8, 4, _hip.F64, 8, None, 1, 0, None, p, 256, None) == 1
    assert lib.cgps_sample(p, p, p, 0, 4, _hip.F64, 8, None, 1, 0, p, p, 256, None) == 1
    assert lib.cgps_sample(p, p, p, 8, 4, _hip.F64, 0, None, 1, 0, p, p, 256, None) == 1
    assert lib.cgps_sample(p, p, p, 8, 9, _hip.F64, 8, None, 1, 0, p, p, 256, None) == 3
    assert lib.cgps_sample(p, p, p, 8, 4, 7, 8, None, 1, 0, p, p, 256, None) == 3
    assert b"" != lib.cgps_last_error()
    assert lib.cgps_normal_fill(None, 8, 4, _hip.F64, 1, 0, None) == 1
    assert lib.cgps_normal_fill(p, 0, 4, _hip.F64, 1, 0, None) == 1
    assert lib.cgps_normal_fill(p, 8, 0, _hip.F64, 1, 0, None) == 1
    assert lib.cgps_normal_fill(p, 8, 4, 7, 1, 0, None) == 3


@pytest.mark.skipif(__import__("torch").cuda.is_available(), reason="only meaningful without a GPU")
def test_no_cpu_fallback_for_sampling():
    import torch
    import _util
    import cyclic_gps.cyclic_reduction as cr
    with pytest.raises(_hip.CgpsError):
        cr.standard_normal(4, 2, 1)
    with pytest.raises(_hip.CgpsError):
        cr.standard_normal(4, 2, 1, device="cpu")
    Rs, Os, _, _, _ = _util.conditioned_system(8, 2)
    dec = (torch.tensor([8]), [Rs], [], [])                # never looked at: there is no device to stage it to
    with pytest.raises(_hip.CgpsError):
        cr.sample(dec, 3, 1)

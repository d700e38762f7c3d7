"""The record stages of the one-launch solve + log-det in one wave's registers (csrc/cgps_tile_rec.h: 4 x 4 fp64
blocks, grids of at most 256 tiles): values against the oracle at the smallest grids that reach each case, against the
LDS form of the same stages (CGPS_FOLD_REG=0, read once per process: two child processes), repeatability through one
workspace, failure reporting, the shard form, and the host check of the layout helpers.

d = 4 fp64 below 65 536 rows runs one row per lane (256-row tiles), so N = 2049, 4096, 4097, 8191, 8449, 65 535 and
65 536 rows give 9, 16, 17, 32, 34, 256 and 256 tiles: a ragged last tile, one full group, a full group plus a group of
one, a 2-record top stage, a ragged top stage and the full 16 x 16 tree.  2^19 + 1 and 2^20 rows are the sizes that run
the 512-thread kernel whose hand-off uses coherent loads only."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import _util
import _fold_reg_child as child
from oracle import cr_oracle as O
from cyclic_gps import leg
import cyclic_gps.cyclic_reduction as cr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "cyclic-gps_amd", "csrc")
SMALL = [2049, 4096, 4097, 8191, 8449, 65535, 65536]
TOL = dict(rtol=1e-9, atol=1e-10)      # tests/test_hip_parity.py, fp64 mahal_and_det against the oracle


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL)
def test_values_against_oracle(n):
    Rs, Os, b, _, logdet = _util.conditioned_system(n, 4, seed=100 + n)
    ref_m, ref_ld = O.mahal_and_det(Rs, Os, b)
    m, ld = cr.mahal_and_det(Rs.cuda(), Os.cuda(), b.cuda())
    print("n=%d mahal %.17g (oracle %.17g) logdet %.17g (oracle %.17g)" % (n, float(m), float(ref_m), float(ld), float(ref_ld)))
    np.testing.assert_allclose([float(m), float(ld)], [float(ref_m), float(ref_ld)], **TOL)
    np.testing.assert_allclose(float(ld), logdet, **TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL)
def test_leg_rows_assembled_in_registers(n):
    """The same grids with the rows of a rank-4 LEG model assembled by the streaming lanes (the SRC = 1 kernels), against
    the blocks-in-memory path; tolerances of tests/test_leg_fused.py for this comparison."""
    gen = torch.Generator().manual_seed(500 + n)
    Nm = torch.tril(0.4 * torch.randn(4, 4, generator=gen, dtype=torch.float64)) + 0.8 * torch.eye(4, dtype=torch.float64)
    Rm = torch.tril(0.3 * torch.randn(4, 4, generator=gen, dtype=torch.float64), -1)
    G = (Nm @ Nm.T + Rm - Rm.T + 1e-5 * torch.eye(4, dtype=torch.float64)).cuda()
    A = torch.randn(4, 2, generator=gen, dtype=torch.float64)
    A = (A @ A.T * 0.5).cuda()
    ts = torch.cumsum(0.05 + 0.5 * torch.rand(n, generator=gen, dtype=torch.float64), 0).cuda()
    v = torch.randn(n, 4, generator=gen, dtype=torch.float64).cuda()
    Rs, Os = leg.peg_precision(ts, G)
    m0, l0 = cr._mahal_and_det(Rs + A, Os, v, levelwise=True)          # one launch per level: no record stages at all
    m1, l1 = leg.leg_mahal_and_det(ts, G, A, v)
    print("n=%d mahal %.17g (%.17g) logdet %.17g (%.17g)" % (n, float(m1), float(m0), float(l1), float(l0)))
    assert abs(float(l1) - float(l0)) <= 1e-9 * max(1.0, abs(float(l0)))
    assert abs(float(m1) - float(m0)) <= 1e-8 * max(1.0, abs(float(m0)))


@pytest.fixture(scope="module")
def both_paths(tmp_path_factory):
    """{"reg": results, "lds": results} of tests/_fold_reg_child.py, one fresh process each"""
    out = {}
    for name, flag in (("reg", None), ("lds", "0")):
        path = str(tmp_path_factory.mktemp("fold_reg") / (name + ".npz"))
        env = dict(os.environ)
        env.pop("CGPS_FOLD_REG", None)
        if flag is not None:
            env["CGPS_FOLD_REG"] = flag
        r = subprocess.run([sys.executable, os.path.join(HERE, "_fold_reg_child.py"), path], env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out[name] = dict(np.load(path))
    return out


@pytest.mark.gpu
def test_register_stages_against_lds_stages(both_paths):
    reg, lds = both_paths["reg"], both_paths["lds"]
    worst = 0.0
    for n in child.ROWS:
        a, b = reg["out_%d" % n], lds["out_%d" % n]
        rel = float(np.max(np.abs(a - b) / np.abs(b)))
        worst = max(worst, rel)
        print("n=%d registers %s  LDS %s  relative difference %.3g" % (n, a.tolist(), b.tolist(), rel))
        assert int(reg["info_%d" % n]) == 0 and int(lds["info_%d" % n]) == 0
        np.testing.assert_allclose(a, b, err_msg="n=%d" % n, **TOL)
    print("largest relative difference %.3g" % worst)


@pytest.mark.gpu
def test_repeatable_through_one_workspace():
    """Three different 4097-row systems (17 tiles: a full group and a group of one, a 2-record top stage) alternate
    through one workspace; every result equals, bit for bit, what that system gave on its first call."""
    systems = [_util.conditioned_system(4097, 4, seed=seed, device="cuda")[:3] for seed in (11, 12, 13)]
    refs = [O.mahal_and_det(*(t.cpu() for t in s)) for s in systems]
    first = [None] * 3
    cr.CHECK_POSITIVE_DEFINITE = False
    try:
        outs = []
        for it in range(50):
            k = (it * 7 + it // 5) % 3
            outs.append((k, cr.mahal_and_det(*systems[k])))
        torch.cuda.synchronize()
    finally:
        cr.CHECK_POSITIVE_DEFINITE = True
    for k, (m, ld) in outs:
        m, ld = float(m), float(ld)
        if first[k] is None:
            first[k] = (m, ld)
            np.testing.assert_allclose([m, ld], [float(refs[k][0]), float(refs[k][1])], **TOL)
        assert (m, ld) == first[k], (k, m, ld, first[k])


@pytest.mark.gpu
@pytest.mark.parametrize("name,row,tile", [("first", 100, 0), ("last", 4096, 16)])
def test_failure_names_a_row_of_the_tile(name, row, tile, both_paths):
    out, info = child.mahal_logdet(*child.indefinite_system(4097, row))
    print("indefinite block in row %d: info %d out2 %s; child processes: registers %d, LDS %d"
          % (row, info, out.tolist(), int(both_paths["reg"]["fail_info_" + name]), int(both_paths["lds"]["fail_info_" + name])))
    assert np.isnan(out).all()
    assert info != 0 and 256 * tile <= info - 1 <= min(256 * tile + 255, 4096)       # info = 1 + a row
    for path in ("reg", "lds"):
        assert np.isnan(both_paths[path]["fail_out_" + name]).all() and int(both_paths[path]["fail_info_" + name]) != 0
    assert int(both_paths["reg"]["fail_info_" + name]) == info
    Rs, Os, b = child.indefinite_system(4097, row)
    with pytest.raises(cr.NotPSDError):
        cr.mahal_and_det(Rs, Os, b)


@pytest.mark.gpu
def test_shard_record_against_lds_stages(both_paths):
    """cgps_shard_reduce on an 8449-row shard (34 tiles) with a left coupling: record and partial result"""
    a, b = both_paths["reg"]["shard"], both_paths["lds"]["shard"]
    assert a.shape == b.shape == (60,) and np.isfinite(a).all()
    print("largest relative difference %.3g" % float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))))
    np.testing.assert_allclose(a, b, **TOL)
    assert a[58] == 0.0 and b[58] == 0.0          # no fail code


def _host_compiler():
    for cxx in ("c++", "g++", "clang++"):
        if shutil.which(cxx):
            return [shutil.which(cxx)]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return [hipcc, "-x", "c++"]          # as a plain host compiler: no HIP language, no device pass


def test_layout_helpers_on_the_host(tmp_path):
    """tests/fold_reg_layout_check.cpp includes cgps_tile_rec.h alone (its layout helpers are host-pure) and walks every
    n = 1..16 next to the LDS path's elimination rule."""
    exe = str(tmp_path / "fold_reg_layout_check")
    subprocess.run(_host_compiler() + ["-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(HERE, "fold_reg_layout_check.cpp"),
                                       "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " 0 failed" in r.stdout

"""The first levels of a full tile's cyclic reduction in the registers of the lanes that streamed its rows
(csrc/cgps_tile_wave.h: 4 x 4 fp64 blocks read from memory): values against the oracle and the generator's closed-form
log-det, against the staged path of the same binary (CGPS_WAVE_LEVELS=0, read once per process: two child processes),
repeatability through one workspace, failure reporting, the shard form, and the host check of the lane map.

d = 4 fp64 runs 256-row tiles.  Up to 2048 rows it is one workgroup: 1024 and 2048 rows are one full tile at 4 and 8
rows per lane.  Up to 65 536 rows it runs one row per lane: 2304 rows are nine full tiles, 4096 + r rows are sixteen
full tiles (in-register levels) followed by a ragged tile of r rows (staged path) whose end falls on every lane-group and
wave boundary.  2^19 + 1 (ragged last tile) and 2^20 rows run the 512-thread kernel at 16 rows per lane, 2^21 rows the 256-thread
kernel with two workgroups per CU."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import _util
import _wave_levels_child as child
from oracle import cr_oracle as O
from cyclic_gps import _hip
import cyclic_gps.cyclic_reduction as cr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "cyclic-gps_amd", "csrc")
TOL = dict(rtol=1e-9, atol=1e-10)      # tests/test_hip_parity.py::test_ragged_sizes_against_oracle


@pytest.mark.gpu
@pytest.mark.parametrize("n", child.ROWS)
def test_values_against_oracle(n):
    Rs, Os, b, _, logdet = _util.conditioned_system(n, 4, seed=100 + n)
    ref_m, ref_ld = O.mahal_and_det(Rs, Os, b)
    m, ld = cr.mahal_and_det(Rs.cuda(), Os.cuda(), b.cuda())
    print("n=%d mahal %.17g (oracle %.17g) logdet %.17g (oracle %.17g, closed form %.17g)"
          % (n, float(m), float(ref_m), float(ld), float(ref_ld), logdet))
    np.testing.assert_allclose([float(m), float(ld)], [float(ref_m), float(ref_ld)], **TOL)
    np.testing.assert_allclose(float(ld), logdet, **TOL)


@pytest.fixture(scope="module")
def both_paths(tmp_path_factory):
    """{"wave": results, "staged": results} of tests/_wave_levels_child.py, one fresh process each"""
    out = {}
    for name, flag in (("wave", None), ("staged", "0")):
        path = str(tmp_path_factory.mktemp("wave_levels") / (name + ".npz"))
        env = dict(os.environ)
        env.pop("CGPS_WAVE_LEVELS", None)
        if flag is not None:
            env["CGPS_WAVE_LEVELS"] = flag
        r = subprocess.run([sys.executable, os.path.join(HERE, "_wave_levels_child.py"), path], env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out[name] = dict(np.load(path))
    return out


@pytest.mark.gpu
def test_wave_levels_against_staged_path(both_paths):
    """The two paths order the arithmetic differently: agreement within TOL, not bit identity."""
    wave, staged = both_paths["wave"], both_paths["staged"]
    worst = 0.0
    for n in child.ROWS:
        a, b = wave["out_%d" % n], staged["out_%d" % n]
        rel = float(np.max(np.abs(a - b) / np.abs(b)))
        worst = max(worst, rel)
        print("n=%d registers %s  staged %s  relative difference %.3g" % (n, a.tolist(), b.tolist(), rel))
        assert int(wave["info_%d" % n]) == 0 and int(staged["info_%d" % n]) == 0
        np.testing.assert_allclose(a, b, err_msg="n=%d" % n, **TOL)
    print("largest relative difference %.3g" % worst)


@pytest.mark.gpu
def test_repeatable_through_one_workspace():
    """Three 4097-row systems (sixteen full tiles and a tile of one row) and three 2^20-row systems alternate through ONE
    workspace; every result equals, bit for bit, what that system gave on its first call."""
    systems = [_util.conditioned_system(n, 4, seed=seed, device="cuda")[:3] for n, seed in
               ((4097, 11), (2 ** 20, 12), (4097, 13), (2 ** 20, 14), (4097, 15), (2 ** 20, 16))]
    ws = _hip.workspace(2 ** 20, 4, torch.float64, _hip.OP_MAHAL_LOGDET, "cuda")
    assert ws[1] >= _hip.workspace(4097, 4, torch.float64, _hip.OP_MAHAL_LOGDET, "cuda")[1]
    first = [None] * len(systems)
    for it in range(42):
        k = (it * 5 + it // 6) % len(systems)
        out, info = child.mahal_logdet(*systems[k], ws=ws)
        assert info == 0 and np.isfinite(out).all()
        if first[k] is None:
            first[k] = out
        assert (out == first[k]).all(), (it, k, out.tolist(), first[k].tolist())
    assert all(f is not None for f in first)
    assert len({tuple(f.tolist()) for f in first}) == len(systems)      # six different systems, six different results


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,row", child.FAILS)
def test_indefinite_block_is_reported(name, n, row, both_paths):
    out, info = child.mahal_logdet(*child.indefinite_system(n, row))
    print("indefinite block in row %d of %d: info %d out2 %s; child processes: registers %d, staged %d"
          % (row, n, info, out.tolist(), int(both_paths["wave"]["fail_info_" + name]), int(both_paths["staged"]["fail_info_" + name])))
    assert np.isnan(out).all()
    assert 1 <= info <= n                                            # info = 1 + a row
    for path in ("wave", "staged"):
        r = both_paths[path]
        assert np.isnan(r["fail_out_" + name]).all() and 1 <= int(r["fail_info_" + name]) <= n
        assert int(r["fail_raised_" + name]) == 1
    assert int(both_paths["wave"]["fail_info_" + name]) == info
    with pytest.raises(cr.NotPSDError):
        cr.mahal_and_det(*child.indefinite_system(n, row))


@pytest.mark.gpu
@pytest.mark.parametrize("n", child.SHARDS)
def test_shard_form_against_whole_system(n, both_paths):
    """cgps_shard_reduce on an n-row shard with a left neighbour + cgps_finish_records, against the whole system"""
    for path in ("wave", "staged"):
        a, b = both_paths[path]["shard_%d" % n], both_paths[path]["whole_%d" % n]
        print("%s: shards %s  whole %s  relative difference %.3g" % (path, a.tolist(), b.tolist(), float(np.max(np.abs(a - b) / np.abs(b)))))
        assert np.isfinite(a).all()
        np.testing.assert_allclose(a, b, err_msg=path, **TOL)
    np.testing.assert_allclose(both_paths["wave"]["whole_%d" % n], both_paths["staged"]["whole_%d" % n], **TOL)


def _host_compiler():
    for cxx in ("c++", "g++", "clang++"):
        if shutil.which(cxx):
            return [shutil.which(cxx)]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return [hipcc, "-x", "c++"]          # as a plain host compiler: no HIP language, no device pass


def test_lane_map_on_the_host(tmp_path):
    """tests/wave_levels_layout_check.cpp includes cgps_tile_wave.h alone (its lane map is host-pure) and walks full tiles
    of 64, 128 and 256 rows for every L <= 4 next to the LDS path's elimination and parking rules."""
    exe = str(tmp_path / "wave_levels_layout_check")
    subprocess.run(_host_compiler() + ["-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(HERE, "wave_levels_layout_check.cpp"),
                                       "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " 0 failed" in r.stdout

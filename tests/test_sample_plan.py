"""The plan of cgps_sample (sample_ws in csrc/cgps_plan.h) without a GPU: every backward pass writes inside its chunk's
slice of the workspace, for N = 1..3000 and the thresholds, d = 1..8, both scalar sizes, one sample to five thousand."""
import os
import subprocess

from test_rng_spec import CSRC, HERE, _host_compiler


def test_every_sample_pass_writes_inside_its_slice(tmp_path):
    exe = str(tmp_path / "sample_plan_check")
    subprocess.run(_host_compiler() + ["-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(HERE, "sample_plan_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " 0 failed" in r.stdout

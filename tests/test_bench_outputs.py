"""bench.py's plain run: exactly --steps timed steps, the headline fields, nothing of --full, and --dump-outputs
writing what the last timed step computed (the same inputs, hence the same outputs, from run to run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_and_full_options():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


@pytest.mark.gpu
def test_plain_run_dumps_the_outputs_of_its_last_step(tmp_path):
    outs = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rows", str(1 << 16), "--steps", "3",
               "--warmup", "1", "--prewarm-seconds", "0.2", "--dump-outputs", str(d)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, p.stdout
        line = json.loads(lines[0])
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert line["value"] > 0 and line["unit"] == "GB/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
        assert line["cpu_baseline"] is None and line["roofline"] is None and "headline_cold" not in line.get("extras", {})
        assert line["check"]["logdet_rel_err"] < 1e-10 and line["check"]["mahal_rel_err"] < 1e-9
        got = {}
        for name in ("mahal", "logdet"):
            a = np.load(d / (name + ".npy"))
            assert a.dtype == np.float64 and a.shape == () and np.isfinite(a)
            got[name] = float(a)
        outs.append(got)
    for name in ("mahal", "logdet"):
        assert abs(outs[0][name] - outs[1][name]) <= 1e-12 * abs(outs[0][name]), (name, outs)

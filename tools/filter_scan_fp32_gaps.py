"""fp32 error of the time-parallel filter (chunk_rows= of leg.filter_predictive_batch) and of the serial
kernel against the dense fp64 truths of tests/test_leg_filter.py, in units of the error the same recursion has when
torch evaluates it in fp32 (tests/_filterref.py; floor 16 eps32), at gap scales 1, 1e-3 and 1e-6 on the masked ragged
batch with variances.  The suite asserts the unit-gap figure (bound 4); this prints all three.

    python tools/filter_scan_fp32_gaps.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cyclic-gps_amd"), os.path.join(ROOT, "tests")]
import _filterref  # noqa: E402
from cyclic_gps import leg  # noqa: E402
from test_leg_filter import LENGTHS, ROWS, _cuda_model, _ragged, _truth  # noqa: E402
from test_leg_posterior_batch import _model, _series  # noqa: E402

F32, F64 = torch.float32, torch.float64
eps = float(torch.finfo(F32).eps)
for scale in (1.0, 1e-3, 1e-6):
    for d, obs in ((1, 1), (5, 1), (5, 3), (8, 8)):
        _, mats = _model(d, obs, 300 + 10 * d + obs)
        series = [(t[0] + (t - t[0]) * scale, x, mk, s) for t, x, mk, s in _series(obs, list(LENGTHS), 301 + 10 * d + obs)]
        truth = [_truth(mats, t, x, s, mk) for t, x, mk, s in series]
        refs = [_filterref.filter_ref(mats, t, x, s, mk, dtype=F32) for t, x, mk, s in series]
        m = _cuda_model(mats, F32)
        ts, xs, ob, nv = _ragged(series, F32)
        kw = dict(lengths=list(LENGTHS), observed=ob, noise_var=nv)
        outs = {"serial": leg.filter_predictive_batch(m, ts, xs, **kw), "(4,3)": leg.filter_predictive_batch(m, ts, xs, chunk_rows=(4, 3), **kw),
                "64": leg.filter_predictive_batch(m, ts, xs, chunk_rows=64, **kw)}
        for name, out in outs.items():
            worst_ratio, worst_abs = 0.0, 0.0
            for j, key in enumerate(ROWS):
                want = torch.cat([t[key] for t in truth])
                ref = torch.cat([r[key] for r in refs]).to(F64)
                scl = 1 + want.abs()
                e_lib = float(((out[j].cpu().to(F64).reshape(want.shape) - want).abs() / scl).max())
                e_ref = float(((ref.reshape(want.shape) - want).abs() / scl).max())
                worst_ratio = max(worst_ratio, e_lib / max(e_ref, 16 * eps))
                worst_abs = max(worst_abs, e_lib)
            print("scale %g d %d obs %d %s: worst error %.3e, in units of max(torch fp32 recursion's, 16 eps32): %.2f" % (scale, d, obs, name, worst_abs, worst_ratio), flush=True)

"""Time leg.log_likelihood_batch against a Python loop of leg.log_likelihood (device events after warm-up).

Workload: fp64, rank 5, obs_dim 1, the model of tests/golden/leg_co2like.npz, B series of 502 rows from
leg.co2_like_series with different seeds (standardised as co2_workload does).  Cases: forward only, and forward +
backward of out.sum() with all four matrices trainable, for B in --batches.

    python tools/time_leg_batch.py [--batches 1,64,1024] [--reps 20] [--loop-reps 3] [--json out.json]
    python tools/time_leg_batch.py --profile-only --batches 1024     (forward calls only, for rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cyclic-gps_amd")]
from cyclic_gps import leg  # noqa: E402


def workload(B, rows=502, dtype=torch.float64):
    g = np.load(os.path.join(ROOT, "tests", "golden", "leg_co2like.npz"))
    m = leg.LEGMatrices(*(torch.from_numpy(g[k]).to(dtype).cuda() for k in ("N", "R", "B", "Lambda")))
    ts, xs = [], []
    for b in range(B):
        t, x = leg.co2_like_series(rows=rows, seed=b, dtype=dtype)
        ts.append(12 * (t - t.min()))
        xs.append((x - x.mean()) / x.std())
    return m, torch.stack(ts).cuda(), torch.stack(xs).cuda()


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times)), float(min(times))


def trainable(m):
    return leg.LEGMatrices(*(t.clone().requires_grad_(True) for t in (m.N, m.R, m.B, m.Lambda)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile-only", action="store_true")
    a = ap.parse_args()
    res = []
    for B in [int(x) for x in a.batches.split(",")]:
        m, ts, xs = workload(B)
        if a.profile_only:
            with torch.no_grad():
                for _ in range(a.reps):
                    leg.log_likelihood_batch(m, ts, xs)
            torch.cuda.synchronize()
            continue
        # the batch agrees with the loop before anything is timed
        with torch.no_grad():
            ref = torch.stack([leg.log_likelihood(m, ts[b], xs[b]) for b in range(B)])
            out = leg.log_likelihood_batch(m, ts, xs)
        err = float(((out - ref).abs() / ref.abs().clamp_min(1.0)).max())
        assert err < 1e-9, err

        def fwd_batch():
            with torch.no_grad():
                leg.log_likelihood_batch(m, ts, xs)

        def fwd_loop():
            with torch.no_grad():
                for b in range(B):
                    leg.log_likelihood(m, ts[b], xs[b])

        mg = trainable(m)

        def fb_batch():
            for p in (mg.N, mg.R, mg.B, mg.Lambda):
                p.grad = None
            leg.log_likelihood_batch(mg, ts, xs).sum().backward()

        def fb_loop():
            for p in (mg.N, mg.R, mg.B, mg.Lambda):
                p.grad = None
            for b in range(B):
                leg.log_likelihood(mg, ts[b], xs[b]).backward()

        loop_reps = a.loop_reps if B > 64 else a.reps
        row = {"B": B, "rows": 502, "d": 5, "dtype": "float64", "max_rel_err_vs_loop": err}
        row["fwd_batch_us"], row["fwd_batch_min_us"] = timed(fwd_batch, a.reps, 3)
        row["fwd_loop_us"], _ = timed(fwd_loop, loop_reps, 1)
        row["fwdbwd_batch_us"], row["fwdbwd_batch_min_us"] = timed(fb_batch, a.reps, 3)
        row["fwdbwd_loop_us"], _ = timed(fb_loop, loop_reps, 1)
        row["fwd_speedup"] = row["fwd_loop_us"] / row["fwd_batch_us"]
        row["fwdbwd_speedup"] = row["fwdbwd_loop_us"] / row["fwdbwd_batch_us"]
        print(json.dumps(row), flush=True)
        res.append(row)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

"""Time the time-parallel form of the filter (``chunk_rows=`` of leg.filter_predictive*, cgps_leg_filter_scan: DESIGN.md
4.23) against the serial kernel -- device events, median of --reps calls after 3 warm-ups, fp64, rank 5, 70 % of the
entries observed, per-point noise variances (the workload of tools/time_filter.py, whose model and data it takes).

    python tools/time_filter_scan.py [--obs 1,3] [--rows 16384,131072,1048576] [--chunk-rows 16,32,64,128]
                                     [--fanout 16,32,64] [--batches 64,1024] [--serial-max-rows 131072] [--reps 20]
                                     [--json out.json]
        one long series, per (obs_dim, rows):
          serial_us          leg.filter_predictive without chunk_rows (rows > --serial-max-rows: ONE call, no warm-up);
          scan_us[L][F]      the call with chunk_rows=(L, F), for every pair; best = the fastest pair; speedup = serial / best;
        the batched workload of DESIGN 4.22, per (obs_dim, B) with B series of 502 rows:
          serial_us, auto_us (chunk_rows="auto"), auto_over_serial.
    Every timed configuration is first held to the serial result (rtol 1e-7, atol 1e-9).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cyclic-gps_amd"), os.path.join(ROOT, "tools")]
from cyclic_gps import leg  # noqa: E402
from time_loo import data, model, timed_alternating  # noqa: E402


def long_series(rows, obs, seed=0, dtype=torch.float64):
    """One series of ``rows`` rows: irregular gaps of 0.2 .. 1.2, standard normal observations, 70 % observed, noise
    variances uniform in [0, 1]."""
    gen = torch.Generator().manual_seed(seed + rows + obs)
    ts = torch.cumsum(0.2 + torch.rand(rows, generator=gen, dtype=dtype), 0)
    xs = torch.randn(rows, obs, generator=gen, dtype=dtype)
    observed = torch.rand(rows, obs, generator=gen) < 0.7
    noise = torch.rand(rows, obs, generator=gen, dtype=dtype)
    return ts.cuda(), xs.cuda(), observed.cuda(), noise.cuda()


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b) * 1e3


def agree(out, ref):
    for a, b in zip(out[:5], ref[:5]):
        assert bool(((a - b).abs() - 1e-7 * b.abs() <= 1e-9).all()), float((a - b).abs().max())


def measure_long(m, rows, obs, pairs, reps, serial_max_rows):
    ts, xs, observed, noise = long_series(rows, obs)
    kw = dict(observed=observed, noise_var=noise)
    row = {"obs": obs, "rows": rows, "d": m.N.shape[0], "dtype": "float64"}
    with torch.no_grad():
        if rows > serial_max_rows:
            ref, row["serial_us"] = once(lambda: leg.filter_predictive(m, ts, xs, **kw))
            row["serial_calls"] = 1
        else:
            ref = leg.filter_predictive(m, ts, xs, **kw)
            row["serial_us"] = timed_alternating({"serial": lambda: leg.filter_predictive(m, ts, xs, **kw)}, reps)["serial"][0]
        fns = {}
        for L, F in pairs:
            agree(leg.filter_predictive(m, ts, xs, chunk_rows=(L, F), **kw), ref)
            fns["%d,%d" % (L, F)] = (lambda L=L, F=F: leg.filter_predictive(m, ts, xs, chunk_rows=(L, F), **kw))
        t = timed_alternating(fns, reps)
    row["scan_us"] = {k: v[0] for k, v in t.items()}
    best = min(t, key=lambda k: t[k][0])
    row["best"], row["best_us"], row["speedup"] = best, t[best][0], row["serial_us"] / t[best][0]
    return row


def measure_batch(m, B, obs, reps):
    ts, xs, observed, noise = data(B, obs)
    kw = dict(observed=observed, noise_var=noise)
    with torch.no_grad():
        agree(leg.filter_predictive_batch(m, ts, xs, chunk_rows="auto", **kw), leg.filter_predictive_batch(m, ts, xs, **kw))
        t = timed_alternating({"serial": lambda: leg.filter_predictive_batch(m, ts, xs, **kw),
                               "auto": lambda: leg.filter_predictive_batch(m, ts, xs, chunk_rows="auto", **kw)}, reps)
    return {"obs": obs, "B": B, "rows": ts.shape[1], "serial_us": t["serial"][0], "auto_us": t["auto"][0],
            "auto": [leg.FILTER_CHUNK_ROWS, leg.FILTER_SCAN_FANOUT], "auto_over_serial": t["auto"][0] / t["serial"][0]}


def main():
    ints = lambda s: [int(x) for x in s.split(",") if x]      # noqa: E731
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", default="1,3")
    ap.add_argument("--rows", default="16384,131072,1048576")
    ap.add_argument("--chunk-rows", default="16,32,64,128")
    ap.add_argument("--fanout", default="16,32,64")
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--serial-max-rows", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = []

    def keep(row):
        print(json.dumps(row), flush=True)
        res.append(row)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as fh:
                json.dump(res, fh, indent=1)

    pairs = [(L, F) for L in ints(a.chunk_rows) for F in ints(a.fanout)]
    for obs in ints(a.obs):
        m = model(obs)
        for rows in ints(a.rows):
            keep(measure_long(m, rows, obs, pairs, a.reps, a.serial_max_rows))
        for B in ints(a.batches):
            keep(measure_batch(m, B, obs, a.reps))


if __name__ == "__main__":
    main()

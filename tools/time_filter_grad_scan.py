"""Time the time-parallel backward of the LEG filter (``backward_chunk_rows=`` of leg.filter_predictive*)
against the serial reverse walk -- device events, median of --reps calls after 3 warm-ups, the variants alternated inside
every repetition.  No threshold: the numbers go into README.md and DESIGN.md 4.25, and ``"auto"``
(leg.FILTER_BACKWARD_CHUNK_ROWS) and leg.FILTER_LINK_REPLICATE are chosen from them.

Workload: fp64, rank 5, 70 % of the entries observed, per-point noise variances, obs_dim 1 and 3 (the model and data of
tools/time_filter_scan.py and tools/time_filter_grad.py).  What is timed is forward plus backward of ``loglik.sum()``
with gradients in the model's four matrices; the forward is ``chunk_rows="auto"`` throughout.

    python tools/time_filter_grad_scan.py [--obs 1,3] [--rows 16384,131072,1048576] [--chunk-rows 32,64,128,256,512]
                                          [--batches 64,1024] [--serial-max-rows 16384] [--reps 20] [--json out.json]
        one long series, per (obs_dim, rows):
          fwd_us                the forward alone (no graph)
          serial_fwd_bwd_us     backward_chunk_rows=None (rows > --serial-max-rows: ONE call, after the other variants have
                                loaded its kernels; serial_calls says how many were timed)
          probes_us[L]          backward_chunk_rows=L with d sequential probe calls (d + 2 calls of the entry)
          replicated_us[L]      the same with ONE call over d + 1 copies of the models in the probes' place (two calls,
                                d + 1 times the memory)
          best / best_us / speedup = serial over the fastest variant
        the batched workload of DESIGN 4.24, per (obs_dim, B) with B series of 502 rows: the same columns, the serial
        backward timed like the others.
    Every variant's gradient in N is first held to the serial one (1e-7 of its largest entry).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cyclic-gps_amd"), os.path.join(ROOT, "tools")]
from cyclic_gps import leg  # noqa: E402
from time_filter_grad import trainable  # noqa: E402
from time_filter_scan import long_series, once  # noqa: E402
from time_loo import data, model, timed_alternating  # noqa: E402


def fwd_bwd(call, m, L, replicate):
    """One forward + backward; returns the gradient in N"""
    mt = trainable(m)
    keep = leg.FILTER_LINK_REPLICATE
    leg.FILTER_LINK_REPLICATE = replicate
    try:
        call(mt, chunk_rows="auto", differentiable=True, backward_chunk_rows=L).loglik.sum().backward()
    finally:
        leg.FILTER_LINK_REPLICATE = keep
    return mt.N.grad


def measure(call, m, Ls, reps, serial_once):
    row = {}
    variants = {"probes_us": False, "replicated_us": True}
    fns = {"fwd": lambda: call(m, chunk_rows="auto")}
    for name, replicate in variants.items():
        for L in Ls:
            fns["%s %d" % (name, L)] = (lambda L=L, replicate=replicate: fwd_bwd(call, m, L, replicate))
    if not serial_once:
        fns["serial"] = lambda: fwd_bwd(call, m, None, False)
    first = {k: fn() for k, fn in fns.items() if k != "fwd"}
    t = timed_alternating(fns, reps)
    if serial_once:
        first["serial"], row["serial_fwd_bwd_us"] = once(lambda: fwd_bwd(call, m, None, False))
        row["serial_calls"] = 1
    else:
        row["serial_fwd_bwd_us"], row["serial_calls"] = t["serial"][0], reps
    ref = first.pop("serial")
    scale = float(ref.abs().max())
    row["worst_grad_N_error"] = max(float((g - ref).abs().max()) / scale for g in first.values())
    assert row["worst_grad_N_error"] <= 1e-7, row["worst_grad_N_error"]
    row["fwd_us"] = t["fwd"][0]
    for name in variants:
        row[name] = {str(L): round(t["%s %d" % (name, L)][0], 1) for L in Ls}
    best = min((k for k in t if k not in ("fwd", "serial")), key=lambda k: t[k][0])
    row["best"], row["best_us"], row["speedup"] = best, t[best][0], row["serial_fwd_bwd_us"] / t[best][0]
    return row


def main():
    ints = lambda s: [int(x) for x in s.split(",") if x]      # noqa: E731
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", default="1,3")
    ap.add_argument("--rows", default="16384,131072,1048576")
    ap.add_argument("--chunk-rows", default="32,64,128,256,512")
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--serial-max-rows", type=int, default=16384)
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

    Ls = ints(a.chunk_rows)
    for obs in ints(a.obs):
        m = model(obs)
        for rows in ints(a.rows):
            ts, xs, observed, noise = long_series(rows, obs)
            call = lambda mt, **kw: leg.filter_predictive(mt, ts, xs, observed=observed, noise_var=noise, **kw)      # noqa: E731
            row = {"obs": obs, "rows": rows, "d": m.N.shape[0], "dtype": "float64"}
            row.update(measure(call, m, Ls, a.reps, rows > a.serial_max_rows))
            keep(row)
        for B in ints(a.batches):
            ts, xs, observed, noise = data(B, obs)
            call = lambda mt, **kw: leg.filter_predictive_batch(mt, ts, xs, observed=observed, noise_var=noise, **kw)      # noqa: E731
            row = {"obs": obs, "B": B, "rows": ts.shape[1], "d": m.N.shape[0], "dtype": "float64"}
            row.update(measure(call, m, Ls, a.reps, False))
            keep(row)


if __name__ == "__main__":
    main()

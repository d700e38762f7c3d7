"""Time cr.mahal_and_det_batch against the two things a caller has without it (device events after warm-up, the
versions alternated inside every repetition of one process).

Workload: fp64, B systems of 502 rows from tests/_util.conditioned_system with different seeds, d = 5 and d = 4, dense
layout.  Cases: forward only, and forward + backward of sum(mahal) + sum(logdet) with Rs, Os and x trainable.
  batch : one cr.mahal_and_det_batch call
  loop  : (a) a Python loop of cr.mahal_and_det, one call per system -- what a caller has today
  concat: (b) ONE cr.mahal_and_det on the concatenated system with zero coupling blocks between the systems; it gives
          only the sums over the systems and is the cost floor of the existing kernels

    python tools/time_mahal_batch.py [--batches 1,64,1024] [--dims 5,4] [--reps 20] [--loop-reps 3] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cyclic-gps_amd"), os.path.join(ROOT, "tests")]
import cyclic_gps.cyclic_reduction as cr  # noqa: E402
import _util  # noqa: E402


def workload(B, d, rows=502, dtype=torch.float64):
    """Dense operands Rs [B, n, d, d], Os [B, n-1, d, d], x [B, n, d] and the concatenated ones with zero cuts."""
    systems = [_util.conditioned_system(rows, d, seed=b)[:3] for b in range(min(B, 16))]
    systems = [systems[b % len(systems)] for b in range(B)]       # (the values do not matter for the time)
    Rs = torch.stack([s[0] for s in systems]).to(dtype).cuda()
    Os = torch.stack([s[1] for s in systems]).to(dtype).cuda()
    x = torch.stack([s[2] for s in systems]).to(dtype).cuda()
    Oc = torch.zeros(B, rows, d, d, dtype=dtype, device="cuda")
    Oc[:, :rows - 1] = Os
    return Rs, Os, x, Rs.reshape(B * rows, d, d), Oc.reshape(B * rows, d, d)[:B * rows - 1].contiguous(), x.reshape(B * rows, d)


def timed_alternating(fns, reps, warmup):
    """name -> (median, min) in microseconds, the variants alternated inside every repetition (other work shares the
    machine: a drift then hits all of them alike)."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3)
    return {k: (float(np.median(v)), float(min(v))) for k, v in times.items()}


def row_for(B, d, reps, loop_reps):
    Rs, Os, x, Rc, Oc, xc = workload(B, d)
    with torch.no_grad():
        m, ld = cr.mahal_and_det_batch(Rs, Os, x)
        ref = [cr.mahal_and_det(Rs[b], Os[b], x[b]) for b in range(B)]
        rm, rl = torch.stack([r[0] for r in ref]), torch.stack([r[1] for r in ref])
        sm, sl = cr.mahal_and_det(Rc, Oc, xc)
    err = max(float(((m - rm).abs() / rm.abs().clamp_min(1.0)).max()), float(((ld - rl).abs() / rl.abs().clamp_min(1.0)).max()))
    assert err < 1e-9, err
    assert abs(float(m.sum() - sm)) <= 1e-9 * abs(float(sm)) and abs(float(ld.sum() - sl)) <= 1e-9 * abs(float(sl))
    leaves = [t.clone().requires_grad_(True) for t in (Rs, Os, x)]
    cleaves = [t.clone().requires_grad_(True) for t in (Rc, Oc, xc)]

    def zero(ts):
        for t in ts:
            t.grad = None

    def fwd_batch():
        with torch.no_grad():
            cr.mahal_and_det_batch(Rs, Os, x)

    def fwd_concat():
        with torch.no_grad():
            cr.mahal_and_det(Rc, Oc, xc)

    def fwd_loop():
        with torch.no_grad():
            for b in range(B):
                cr.mahal_and_det(Rs[b], Os[b], x[b])

    def fb_batch():
        zero(leaves)
        m, ld = cr.mahal_and_det_batch(*leaves)
        (m.sum() + ld.sum()).backward()

    def fb_concat():
        zero(cleaves)
        m, ld = cr.mahal_and_det(*cleaves)
        (m + ld).backward()

    def fb_loop():
        zero(leaves)
        for b in range(B):
            m, ld = cr.mahal_and_det(leaves[0][b], leaves[1][b], leaves[2][b])
            (m + ld).backward()

    row = {"B": B, "rows": Rs.shape[1], "d": d, "dtype": "float64", "max_rel_err_vs_loop": err}
    got = timed_alternating({"fwd_batch": fwd_batch, "fwd_concat": fwd_concat}, reps, 3)
    got.update(timed_alternating({"fwdbwd_batch": fb_batch, "fwdbwd_concat": fb_concat}, reps, 3))
    if B > 64:        # the loop is far too slow to alternate at full repetitions
        got.update(timed_alternating({"fwd_loop": fwd_loop}, loop_reps, 1))
        got.update(timed_alternating({"fwdbwd_loop": fb_loop}, loop_reps, 1))
    else:
        got.update(timed_alternating({"fwd_loop": fwd_loop, "fwd_batch_again": fwd_batch}, reps, 2))
        got.update(timed_alternating({"fwdbwd_loop": fb_loop, "fwdbwd_batch_again": fb_batch}, reps, 2))
    for name, (med, low) in got.items():
        row[name + "_us"], row[name + "_min_us"] = med, low
    for k in ("fwd", "fwdbwd"):
        row[k + "_speedup_vs_loop"] = row[k + "_loop_us"] / row[k + "_batch_us"]
        row[k + "_ratio_to_concat"] = row[k + "_batch_us"] / row[k + "_concat_us"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--dims", default="5,4")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = []
    for d in [int(v) for v in a.dims.split(",")]:
        for B in [int(v) for v in a.batches.split(",")]:
            row = row_for(B, d, a.reps, a.loop_reps)
            print(json.dumps(row), flush=True)
            res.append(row)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

"""Time predict.make_predictions_batch against a Python loop of predict.make_predictions, and
leg.insample_posterior_batch(observed=) against a loop of leg.insample_posterior(observed=) (device events: median of
--reps after 3 warm-ups).

Workload: fp64, rank 5, obs_dim 1, the model and the 784 target times of tests/golden/leg_co2like.npz, B series of 502
rows from leg.co2_like_series with different seeds (standardised as co2_workload does), the targets shared by all series.

    python tools/time_leg_posterior_batch.py [--batches 1,64,1024] [--reps 20] [--loop-reps 3] [--json out.json]
        per B: predict_batch_us / predict_loop_us (make_predictions_batch, check_sorted=False, against the loop, which is
        what a user ran before the batched call existed), posterior_obs_batch_us / posterior_obs_loop_us (70 % of the
        entries kept, another mask per series), and assembly_{plain,obs,noise}_{kernel,composed}_us: the concatenated
        posterior system alone (leg._posterior_operands_batch + leg._posterior_system_rows) with K's blocks written once by
        cgps_leg_posterior_blocks_seg against the composition it replaces (CGPS_LEG_BLOCKS_COMPOSED=1:
        cgps_peg_precision_seg, then the gather or einsum and the add as torch passes), alternated inside every
        repetition; plain, with the mask, and with noise variances uniform in [0, 1].  The batch agrees with the loop
        before anything is timed.
    python tools/time_leg_posterior_batch.py --profile-only --batches 1024
        the batched calls only, the program to put after  rocprofv3 --kernel-trace --stats --
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cyclic-gps_amd")]
from cyclic_gps import leg, predict  # noqa: E402


def workload(B, rows=502, dtype=torch.float64):
    g = np.load(os.path.join(ROOT, "tests", "golden", "leg_co2like.npz"))
    m = leg.LEGMatrices(*(torch.from_numpy(g[k]).to(dtype).cuda() for k in ("N", "R", "B", "Lambda")))
    ts, xs = [], []
    for b in range(B):
        t, x = leg.co2_like_series(rows=rows, seed=b, dtype=dtype)
        ts.append(12 * (t - t.min()))
        xs.append((x - x.mean()) / x.std())
    return m, torch.stack(ts).cuda(), torch.stack(xs).cuda(), torch.from_numpy(g["target_ts"]).to(dtype).cuda()


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


def timed_alternating(fns, reps, warmup):
    """The same for several variants, alternated inside every repetition (other work shares the machine: a drift then
    hits all of them alike): name -> (median, min) in microseconds."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--observed", type=float, default=0.7, metavar="FRACTION")
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile-only", action="store_true")
    a = ap.parse_args()
    res = []
    for B in [int(x) for x in a.batches.split(",")]:
        m, ts, xs, tt = workload(B)
        n = ts.shape[1]
        obs = (torch.rand(xs.shape, generator=torch.Generator().manual_seed(B)) < a.observed).cuda()

        def predict_batch():
            predict.make_predictions_batch(m, ts, xs, tt, check_sorted=False)

        def posterior_obs_batch():
            leg.insample_posterior_batch(m, ts, xs, observed=obs)

        if a.profile_only:
            for _ in range(a.reps):
                predict_batch()
                posterior_obs_batch()
            torch.cuda.synchronize()
            continue

        def predict_loop():
            with torch.no_grad():
                for b in range(B):
                    predict.make_predictions(m, ts[b], xs[b], tt, check_sorted=False)

        def posterior_obs_loop():
            with torch.no_grad():
                for b in range(B):
                    leg.insample_posterior(m, ts[b], xs[b], observed=obs[b])

        # the batch agrees with the loop before anything is timed
        pm, pv = predict.make_predictions_batch(m, ts, xs, tt)
        mean, (Sd, So) = leg.insample_posterior_batch(m, ts, xs, observed=obs)
        err = 0.0
        with torch.no_grad():
            for b in range(0, B, max(1, B // 16)):
                rm, rv = predict.make_predictions(m, ts[b], xs[b], tt)
                lm, (lSd, lSo) = leg.insample_posterior(m, ts[b], xs[b], observed=obs[b])
                for got, ref in ((pm[b], rm), (pv[b], rv), (mean[b], lm), (Sd[b], lSd), (So[b], lSo)):
                    err = max(err, float(((got - ref).abs() / ref.abs().clamp_min(1.0)).max()))
        assert err < 1e-8, err

        plan = leg._cached_batch_plan([n] * B, ts.device)
        tsf, xsf, obsf = ts.reshape(-1), xs.reshape(B * n, -1), obs.reshape(B * n, -1)

        noisef = torch.rand(xsf.shape, generator=torch.Generator().manual_seed(B + 1), dtype=xsf.dtype).cuda()

        def assembly(observed, noise, composed):
            def run():
                if composed:
                    os.environ["CGPS_LEG_BLOCKS_COMPOSED"] = "1"
                try:
                    with torch.no_grad():
                        source, term, rows, _ = leg._posterior_operands_batch(m, tsf, xsf, observed, noise)
                        leg._posterior_system_rows(plan, tsf, m.G.contiguous(), source, term, rows, None)
                finally:
                    os.environ.pop("CGPS_LEG_BLOCKS_COMPOSED", None)
            return run

        variants = {}
        for name, ob, nv in (("plain", None, None), ("obs", obsf, None), ("noise", None, noisef)):
            variants["assembly_%s_kernel" % name] = assembly(ob, nv, False)
            variants["assembly_%s_composed" % name] = assembly(ob, nv, True)

        loop_reps = a.loop_reps if B > 64 else a.reps
        row = {"B": B, "rows": n, "targets": int(tt.shape[0]), "d": 5, "dtype": "float64", "observed": a.observed,
               "max_rel_err_vs_loop": err}
        for name, fn, reps, warm in (("predict_batch", predict_batch, a.reps, 3), ("predict_loop", predict_loop, loop_reps, 1),
                                     ("posterior_obs_batch", posterior_obs_batch, a.reps, 3),
                                     ("posterior_obs_loop", posterior_obs_loop, loop_reps, 1)):
            row[name + "_us"], row[name + "_min_us"] = timed(fn, reps, warm)
        for name, (med, low) in timed_alternating(variants, a.reps, 3).items():
            row[name + "_us"], row[name + "_min_us"] = med, low
        row["predict_speedup_vs_loop"] = row["predict_loop_us"] / row["predict_batch_us"]
        row["posterior_obs_speedup_vs_loop"] = row["posterior_obs_loop_us"] / row["posterior_obs_batch_us"]
        print(json.dumps(row), flush=True)
        res.append(row)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

"""Time leg.log_likelihood_batch against a Python loop of leg.log_likelihood (device events after warm-up).

Workload: fp64, rank 5, obs_dim 1, the model of tests/golden/leg_co2like.npz, B series of 502 rows from
leg.co2_like_series with different seeds (standardised as co2_workload does).  Cases: forward only, and forward +
backward of out.sum() with all four matrices trainable, for B in --batches.

    python tools/time_leg_batch.py [--batches 1,64,1024] [--reps 20] [--loop-reps 3] [--json out.json]
    python tools/time_leg_batch.py --profile-only --batches 1024     (forward calls only, for rocprofv3 --kernel-trace --stats)
    python tools/time_leg_batch.py --observed 0.7 [--batches 1,64,1024]
        every entry observed with probability 0.7 (another mask per series): log_likelihood_batch(observed=mask) against
        a Python loop of log_likelihood(observed=) and against the fully observed log_likelihood_batch on the same shapes
        (the batched calls alternate inside every repetition).  The masked call keeps its plan (device offsets, the
        series-cut mask: about R bytes from the host) between calls, the fully observed call builds it every time;
        *_obs_us is the call as users get it, *_obs_cold_us the call with the plan cache emptied first, so that both
        sides build a plan, and *_ratio_to_full is taken from the latter
    python tools/time_leg_batch.py --noise [--batches 1,64,1024]
        every entry with a noise variance of its own, uniform in [0, 1], at obs_dim 1 (the golden model) and obs_dim 3
        (its B and Lambda extended, see noise_model): log_likelihood_batch(noise_var=s) against (a) a Python loop of
        log_likelihood(noise_var=) and (b) the fully observed log_likelihood_batch on the same shapes, forward and
        forward + backward, the batched calls alternated inside every repetition.  kernel_* are the launches alone
        (leg_loglik_batch_reductions_w against leg_loglik_batch_reductions on operands built beforehand); the other
        figures are whole calls, the torch work that builds weights, v, q and c included; *_cold empties the plan cache
        first, as under --observed
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


def trainable(m):
    return leg.LEGMatrices(*(t.clone().requires_grad_(True) for t in (m.N, m.R, m.B, m.Lambda)))


def observed_row(m, ts, xs, fraction, reps, loop_reps):
    """The masked batch against its two baselines, forward only and forward + backward."""
    B = ts.shape[0]
    obs = torch.rand(xs.shape, generator=torch.Generator().manual_seed(B)) < fraction
    obs = obs.cuda()
    with torch.no_grad():
        ref = torch.stack([leg.log_likelihood(m, ts[b], xs[b], observed=obs[b]) for b in range(B)])
        out = leg.log_likelihood_batch(m, ts, xs, observed=obs)
    err = float(((out - ref).abs() / ref.abs().clamp_min(1.0)).max())
    assert err < 1e-9, err
    mg = trainable(m)

    def zero():
        for p in (mg.N, mg.R, mg.B, mg.Lambda):
            p.grad = None

    def fwd_obs():
        with torch.no_grad():
            leg.log_likelihood_batch(m, ts, xs, observed=obs)

    def fwd_obs_cold():
        leg._plans.clear()
        fwd_obs()

    def fwd_full():
        with torch.no_grad():
            leg.log_likelihood_batch(m, ts, xs)

    def fwd_loop():
        with torch.no_grad():
            for b in range(B):
                leg.log_likelihood(m, ts[b], xs[b], observed=obs[b])

    def fb_obs():
        zero()
        leg.log_likelihood_batch(mg, ts, xs, observed=obs).sum().backward()

    def fb_obs_cold():
        leg._plans.clear()
        fb_obs()

    def fb_full():
        zero()
        leg.log_likelihood_batch(mg, ts, xs).sum().backward()

    def fb_loop():
        zero()
        for b in range(B):
            leg.log_likelihood(mg, ts[b], xs[b], observed=obs[b]).backward()

    row = {"B": B, "rows": ts.shape[1], "d": 5, "dtype": "float64", "observed": fraction, "max_rel_err_vs_loop": err}
    got = timed_alternating({"fwd_obs": fwd_obs, "fwd_obs_cold": fwd_obs_cold, "fwd_full": fwd_full}, reps, 3)
    got.update(timed_alternating({"fwdbwd_obs": fb_obs, "fwdbwd_obs_cold": fb_obs_cold, "fwdbwd_full": fb_full}, reps, 3))
    got["fwd_loop"] = timed(fwd_loop, loop_reps, 1)
    got["fwdbwd_loop"] = timed(fb_loop, loop_reps, 1)
    for name, (med, low) in got.items():
        row[name + "_us"], row[name + "_min_us"] = med, low
    for k in ("fwd", "fwdbwd"):
        row[k + "_speedup_vs_loop"] = row[k + "_loop_us"] / row[k + "_obs_us"]
        row[k + "_ratio_to_full"] = row[k + "_obs_cold_us"] / row[k + "_full_us"]      # a plan built on both sides
        row[k + "_cached_ratio_to_full"] = row[k + "_obs_us"] / row[k + "_full_us"]
    return row


def noise_model(m, xs, obs_dim):
    """obs_dim 1: the golden model and data.  obs_dim 3: channel c observes the golden loading rotated by c places and
    scaled by 1 - c / 4, its own noise 1 + c / 2 times the golden one, correlated with its neighbour (Lambda lower
    bidiagonal); the data of channel c are the series of c places further on in the batch."""
    if obs_dim == 1:
        return m, xs
    Bm = torch.cat([(1 - c / 4) * torch.roll(m.B, c, 1) for c in range(obs_dim)])
    lam = float(m.Lambda[0, 0])
    Lm = torch.diag(torch.tensor([lam * (1 + c / 2) for c in range(obs_dim)], dtype=m.B.dtype))
    Lm = Lm + 0.3 * lam * torch.diag(torch.ones(obs_dim - 1, dtype=m.B.dtype), -1)
    return leg.LEGMatrices(m.N, m.R, Bm, Lm.to(m.B.device)), torch.cat([torch.roll(xs, c, 0) for c in range(obs_dim)], -1)


def noise_row(m, ts, xs, obs_dim, reps, loop_reps):
    """The batch with per-observation noise against its two baselines: kernels alone, forward, forward + backward."""
    B, n = ts.shape
    m, xs = noise_model(m, xs, obs_dim)
    s = torch.rand(xs.shape, generator=torch.Generator().manual_seed(B), dtype=xs.dtype).cuda()
    with torch.no_grad():
        ref = torch.stack([leg.log_likelihood(m, ts[b], xs[b], noise_var=s[b]) for b in range(B)])
        out = leg.log_likelihood_batch(m, ts, xs, noise_var=s)
    err = float(((out - ref).abs() / ref.abs().clamp_min(1.0)).max())
    assert err < 1e-9, err
    mg = trainable(m)

    def zero():
        for p in (mg.N, mg.R, mg.B, mg.Lambda):
            p.grad = None

    # the launches alone, on operands built once
    plan = leg._BatchPlan([n] * B, ts.device)
    with torch.no_grad():
        tsf, xsf = ts.reshape(-1).contiguous(), xs.reshape(B * n, obs_dim)
        G = m.G.contiguous()
        basis, weights, c_rows, xl, xz = leg._noise_operands(m, tsf, xsf, None, s.reshape(B * n, obs_dim))
        basis, weights = basis.contiguous(), weights.contiguous()
        v = (xl @ m.B).contiguous()
        q = ((xl * xz).sum(-1) + c_rows).contiguous()
        A = (m.B.T @ m.LLT_inv @ m.B).contiguous()

    def kernel_w():
        leg.leg_loglik_batch_reductions_w(tsf, G, basis, weights, v, q, plan)

    def kernel_full():
        leg.leg_loglik_batch_reductions(tsf, G, A, v, q, plan)

    def fwd_w():
        with torch.no_grad():
            leg.log_likelihood_batch(m, ts, xs, noise_var=s)

    def fwd_w_cold():
        leg._plans.clear()
        fwd_w()

    def fwd_full():
        with torch.no_grad():
            leg.log_likelihood_batch(m, ts, xs)

    def fwd_loop():
        with torch.no_grad():
            for b in range(B):
                leg.log_likelihood(m, ts[b], xs[b], noise_var=s[b])

    def fb_w():
        zero()
        leg.log_likelihood_batch(mg, ts, xs, noise_var=s).sum().backward()

    def fb_w_cold():
        leg._plans.clear()
        fb_w()

    def fb_full():
        zero()
        leg.log_likelihood_batch(mg, ts, xs).sum().backward()

    def fb_loop():
        zero()
        for b in range(B):
            leg.log_likelihood(mg, ts[b], xs[b], noise_var=s[b]).backward()

    row = {"B": B, "rows": n, "d": 5, "dtype": "float64", "noise": True, "obs_dim": obs_dim, "Kb": int(basis.shape[0]),
           "max_rel_err_vs_loop": err}
    got = timed_alternating({"kernel_w": kernel_w, "kernel_full": kernel_full}, reps, 3)
    got.update(timed_alternating({"fwd_w": fwd_w, "fwd_w_cold": fwd_w_cold, "fwd_full": fwd_full}, reps, 3))
    got.update(timed_alternating({"fwdbwd_w": fb_w, "fwdbwd_w_cold": fb_w_cold, "fwdbwd_full": fb_full}, reps, 3))
    got["fwd_loop"] = timed(fwd_loop, loop_reps, 1)
    got["fwdbwd_loop"] = timed(fb_loop, loop_reps, 1)
    for name, (med, low) in got.items():
        row[name + "_us"], row[name + "_min_us"] = med, low
    row["kernel_ratio_to_full"] = row["kernel_w_us"] / row["kernel_full_us"]
    for k in ("fwd", "fwdbwd"):
        row[k + "_speedup_vs_loop"] = row[k + "_loop_us"] / row[k + "_w_us"]
        row[k + "_ratio_to_full"] = row[k + "_w_cold_us"] / row[k + "_full_us"]        # a plan built on both sides
        row[k + "_cached_ratio_to_full"] = row[k + "_w_us"] / row[k + "_full_us"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--observed", type=float, default=None, metavar="FRACTION")
    ap.add_argument("--noise", action="store_true")
    a = ap.parse_args()
    res = []
    for B in [int(x) for x in a.batches.split(",")]:
        m, ts, xs = workload(B)
        if a.noise:
            for obs_dim in (1, 3):
                row = noise_row(m, ts, xs, obs_dim, a.reps, a.loop_reps if B > 64 else a.reps)
                print(json.dumps(row), flush=True)
                res.append(row)
            continue
        if a.observed is not None:
            row = observed_row(m, ts, xs, a.observed, a.reps, a.loop_reps if B > 64 else a.reps)
            print(json.dumps(row), flush=True)
            res.append(row)
            continue
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

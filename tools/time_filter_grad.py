"""Time the gradients through the LEG filter (``differentiable=True``, cgps_leg_filter_adjoint: DESIGN.md 4.24) -- device
events, median of --reps calls after 3 warm-ups, the variants of a comparison alternated inside every repetition.  No
threshold: the numbers go into README.md and DESIGN.md 4.24.

Workload: that of tools/time_loo.py -- fp64, rank 5, series of 502 rows, 70 % of the entries observed, per-point noise
variances, obs_dim 1 and 3.

    python tools/time_filter_grad.py [--obs 1,3] [--batches 64,1024] [--models 16x64] [--reps 20] [--json out.json]
        per (obs_dim, B):
          filter_fwd_us            leg.filter_predictive_batch, the default (no graph)
          filter_fwd_bwd_us        filter_predictive_batch(differentiable=True).loglik.sum().backward(), gradients in the
                                   model's four matrices
          adjoint_us               the C entry alone (gaps, reverse walk, Frechet pass) on the saved states, cotangent 1 on
                                   every logpdf
          loglik_fwd_bwd_us        leg.log_likelihood_batch(...).sum().backward() on the same data, the smoother's path
          loglik_full_fwd_bwd_us   the same fully observed without variances (the README's 71 ms at 1 024 series)
        per models MxB: filter_predictive_models forward, forward + backward, and
        log_likelihood_models_observed(...).sum().backward().
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cyclic-gps_amd"), os.path.join(ROOT, "tools")]
from cyclic_gps import leg  # noqa: E402
from time_loo import data, model, timed_alternating  # noqa: E402


def trainable(m):
    return leg.LEGMatrices(*(t.detach().clone().requires_grad_(True) for t in (m.N, m.R, m.B, m.Lambda)))


def adjoint_alone(m, ts, xs, observed, noise):
    """A closure that runs cgps_leg_filter_adjoint on the states of one forward call"""
    B, n, obs = xs.shape
    dt, dev = xs.dtype, xs.device
    mats = leg._stack1(m)
    d = mats[0].shape[1]
    G = (leg._contract(mats[0], mats[0].transpose(1, 2)) + (mats[1] - mats[1].transpose(1, 2)) + leg._scaled_eye(d, 1e-5, dt, dev)).contiguous()
    LLT = (leg._contract(mats[3], mats[3].transpose(1, 2)) + leg._scaled_eye(obs, 1e-9, dt, dev)).contiguous()
    plan = leg._cached_batch_plan([n] * B, dev)
    xs_c, pattern, nv = leg._loo_data(xs.reshape(B * n, obs), observed.reshape(B * n, obs), noise.reshape(B * n, obs), dt)
    ts_c = ts.reshape(-1).contiguous()
    out = leg._filter_rows(ts_c, xs_c, pattern, nv, plan.offsets, G, mats[2].contiguous(), LLT, None)
    gap = ts_c - torch.roll(ts_c, 1)
    gap[plan.offsets[:-1]] = 0
    ones = torch.ones(1, B * n, dtype=dt, device=dev)
    return lambda: leg._filter_adjoint_rows(xs_c, pattern, nv, plan.offsets, G, mats[2].contiguous(), LLT, gap, out[3], out[4],
                                            None, None, [None, None, ones, None, None])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", default="1,3")
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--models", default="16x64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    results = []
    for obs in (int(v) for v in a.obs.split(",")):
        for B in (int(v) for v in a.batches.split(",")):
            m = model(obs)
            ts, xs, observed, noise = data(B, obs)
            kw = dict(observed=observed, noise_var=noise)

            def fwd_bwd(call, **k):
                mt = trainable(m)
                call(mt, ts, xs, **k).sum().backward()

            fns = {
                "filter_fwd_us": lambda: leg.filter_predictive_batch(m, ts, xs, **kw),
                "filter_fwd_bwd_us": lambda: fwd_bwd(lambda *p, **k: leg.filter_predictive_batch(*p, differentiable=True, **k).loglik, **kw),
                "adjoint_us": adjoint_alone(m, ts, xs, observed, noise),
                "loglik_fwd_bwd_us": lambda: fwd_bwd(leg.log_likelihood_batch, **kw),
                "loglik_full_fwd_bwd_us": lambda: fwd_bwd(leg.log_likelihood_batch),
            }
            t = timed_alternating(fns, a.reps)
            row = {"obs": obs, "B": B, "rows": xs.shape[1]}
            row.update({k: round(v[0], 1) for k, v in t.items()})
            results.append(row)
            print(json.dumps(row), flush=True)
    for spec in (s for s in a.models.split(",") if s):
        M, B = (int(v) for v in spec.split("x"))
        for obs in (int(v) for v in a.obs.split(",")):
            ms = [model(obs, seed=k) for k in range(M)]
            ts, xs, observed, noise = data(B, obs)
            kw = dict(observed=observed, noise_var=noise)

            def fwd_bwd_models(call, **k):
                mt = [trainable(m) for m in ms]
                call(mt, ts, xs, **k).sum().backward()

            fns = {
                "filter_fwd_us": lambda: leg.filter_predictive_models(ms, ts, xs, **kw),
                "filter_fwd_bwd_us": lambda: fwd_bwd_models(
                    lambda *p, **k: leg.filter_predictive_models(*p, differentiable=True, **k).loglik, **kw),
                "loglik_fwd_bwd_us": lambda: fwd_bwd_models(leg.log_likelihood_models_observed, **kw),
            }
            t = timed_alternating(fns, a.reps)
            row = {"obs": obs, "models": M, "B": B, "rows": xs.shape[1]}
            row.update({k: round(v[0], 1) for k, v in t.items()})
            results.append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()

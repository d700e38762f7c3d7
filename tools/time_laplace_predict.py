"""Time the predictions from the Laplace posterior (predict.laplace_predictions_batch, leg.glm_predictive,
cgps_leg_glm_predict: DESIGN.md 4.28) -- device events, median of --reps calls after 3 warm-ups, the variants of a
comparison alternated inside every repetition.  No threshold: the numbers go into README.md and DESIGN.md 4.28.

Workload: that of tools/time_laplace.py -- fp64, rank 5, series of 502 rows, 70 % of the entries observed, obs_dim 1 and
3, Poisson counts with an offset of 1 -- and the 784 target times of tests/golden/leg_co2like.npz, shared by all series,
with held-out counts at every target.

    python tools/time_laplace_predict.py [--obs 1,3] [--batches 64,1024] [--reps 10] [--loop-series 16] [--json out.json]
        per (obs_dim, B):
          predict_kernel_us, predict_composed_us   cgps_leg_glm_predict alone on the latent Gaussians at the B x 784 targets,
                                 with held-out counts, and the same arithmetic as torch passes (CGPS_LEG_GLM_COMPOSED=1 takes it)
          predict_kernel_nodata_us                 the kernel without target_ys (Poisson: closed forms, no quadrature)
          bernoulli_kernel_us, bernoulli_composed_us   the same entries read as binary outcomes (two quadratures per entry)
          call_us                the whole call: Newton loop, intercast, predictions
          call_posterior_us      the whole call with posterior= (no Newton step)
          loop_us                a Python loop of predict.laplace_predictions over the first --loop-series series, scaled to B
                                 (timed once: it is long)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cyclic-gps_amd"), os.path.join(ROOT, "tools")]
from cyclic_gps import _hip, leg, predict  # noqa: E402
from time_loo import data, model, timed_alternating  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", default="1,3")
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--loop-series", type=int, default=16)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    tt = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "leg_co2like.npz"))["target_ts"]).to(torch.float64).cuda()
    p = tt.shape[0]
    results = []
    for obs in (int(v) for v in a.obs.split(",")):
        for B in (int(v) for v in a.batches.split(",")):
            m = model(obs)
            ts, xs, observed, _ = data(B, obs)
            gen = torch.Generator().manual_seed(7 * B + obs)
            ys = torch.poisson(torch.exp(1 + 0.5 * xs.cpu()), generator=gen).cuda()
            tys = torch.poisson(torch.full((B, p, obs), 3.0, dtype=torch.float64), generator=gen).cuda()
            offset = torch.ones(obs, dtype=xs.dtype, device="cuda")
            kw = dict(family="poisson", observed=observed, offset=offset, target_ys=tys, check_sorted=False)
            post = leg.laplace_posterior_batch(m, ts, ys, family="poisson", observed=observed, offset=offset)
            r = predict.laplace_predictions_batch(m, ts, ys, tt, posterior=post, **kw)
            d = m.N.shape[0]
            zm, zc = r.z_mean.reshape(B * p, d).contiguous(), r.z_cov.reshape(B * p, d, d).contiguous()
            yf, yb, Bm = tys.reshape(B * p, obs).contiguous(), (tys.reshape(B * p, obs) > 2).to(tys.dtype), m.B.contiguous()
            P, Bn = _hip.GLM_POISSON, _hip.GLM_BERNOULLI
            fns = {
                "predict_kernel_us": lambda: leg._glm_predict_hip(P, zm, zc, yf, None, offset, None, Bm),
                "predict_composed_us": lambda: leg._glm_predict_composed(P, zm, zc, yf, None, offset, None, Bm),
                "predict_kernel_nodata_us": lambda: leg._glm_predict_hip(P, zm, zc, None, None, offset, None, Bm),
                "bernoulli_kernel_us": lambda: leg._glm_predict_hip(Bn, zm, zc, yb, None, offset, None, Bm),
                "bernoulli_composed_us": lambda: leg._glm_predict_composed(Bn, zm, zc, yb, None, offset, None, Bm),
                "call_us": lambda: predict.laplace_predictions_batch(m, ts, ys, tt, **kw),
                "call_posterior_us": lambda: predict.laplace_predictions_batch(m, ts, ys, tt, posterior=post, **kw),
            }
            t = timed_alternating(fns, a.reps)
            k = min(a.loop_series, B)
            loop = lambda: [predict.laplace_predictions(m, ts[b], ys[b], tt, "poisson", observed=observed[b], offset=offset,      # noqa: E731
                                                        target_ys=tys[b], check_sorted=False) for b in range(k)]
            tl = timed_alternating({"loop": loop}, 1, warmup=1)["loop"][0] * B / k
            row = {"obs": obs, "B": B, "rows": xs.shape[1], "targets": p, "entries": B * p * obs, "eta_var_max": float(r.eta_var.max()),
                   "converged": bool(r.converged.all()), "loop_us": round(tl, 1), "loop_series_timed": k}
            row.update({k_: round(v[0], 1) for k_, v in t.items()})
            results.append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()

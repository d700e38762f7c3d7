"""Time leg.log_likelihood_models against a Python loop of leg.log_likelihood_batch over the models (device events
after warm-up, as tools/time_leg_batch.py).

Workload: fp64, rank 5, obs_dim 1, B series of 502 rows from leg.co2_like_series with different seeds (standardised as
co2_workload does); M models: the model of tests/golden/leg_co2like.npz with every matrix perturbed by 5 % noise of its
own.  Cases: forward only, and forward + backward of out.sum() with all four matrices of every model trainable, for
(M, B) in --shapes.  Values and gradients are compared with the loop's before anything is timed.

    python tools/time_leg_models.py [--shapes 256x1,64x16,16x1024] [--reps 20] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cyclic-gps_amd"), os.path.join(ROOT, "tools")]
from cyclic_gps import leg  # noqa: E402
from time_leg_batch import timed, workload  # noqa: E402


def models(m, M):
    gen = torch.Generator().manual_seed(M)
    out = []
    for _ in range(M):
        mats = []
        for t, tril in ((m.N, 0), (m.R, -1), (m.B, None), (m.Lambda, 0)):
            p = t.cpu() * (1 + 0.05 * torch.randn(t.shape, generator=gen, dtype=t.dtype))
            mats.append((p if tril is None else torch.tril(p, tril)).cuda())
        out.append(leg.LEGMatrices(*mats))
    return out


def trainable(ms):
    return [leg.LEGMatrices(*(t.clone().requires_grad_(True) for t in (m.N, m.R, m.B, m.Lambda))) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x1,64x16,16x1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = []
    for shape in a.shapes.split(","):
        M, B = (int(x) for x in shape.split("x"))
        m, ts, xs = workload(B)
        ms = models(m, M)
        # the one call agrees with the loop before anything is timed
        with torch.no_grad():
            ref = torch.stack([leg.log_likelihood_batch(mk, ts, xs) for mk in ms])
            out = leg.log_likelihood_models(ms, ts, xs)
        err = float(((out - ref).abs() / ref.abs().clamp_min(1.0)).max())
        assert err < 1e-9, err

        def fwd_models():
            with torch.no_grad():
                leg.log_likelihood_models(ms, ts, xs)

        def fwd_loop():
            with torch.no_grad():
                for mk in ms:
                    leg.log_likelihood_batch(mk, ts, xs)

        mg = trainable(ms)

        def zero():
            for mk in mg:
                for p in (mk.N, mk.R, mk.B, mk.Lambda):
                    p.grad = None

        def fb_models():
            zero()
            leg.log_likelihood_models(mg, ts, xs).sum().backward()

        def fb_loop():
            zero()
            for mk in mg:
                leg.log_likelihood_batch(mk, ts, xs).sum().backward()

        # ... and so do the gradients, every tensor relative to its own largest entry
        def grads(step):
            step()
            return [p.grad.clone() for mk in mg for p in (mk.N, mk.R, mk.B, mk.Lambda)]

        gerr = max(float((g1 - g0).abs().max() / g0.abs().max()) for g1, g0 in zip(grads(fb_models), grads(fb_loop)))
        assert gerr < 1e-7, gerr

        row = {"M": M, "B": B, "rows": 502, "d": 5, "dtype": "float64", "max_rel_err_vs_loop": err,
               "max_rel_grad_err_vs_loop": gerr}
        row["fwd_models_us"], row["fwd_models_min_us"] = timed(fwd_models, a.reps, 3)
        row["fwd_loop_us"], row["fwd_loop_min_us"] = timed(fwd_loop, a.reps, 3)
        row["fwdbwd_models_us"], row["fwdbwd_models_min_us"] = timed(fb_models, a.reps, 3)
        row["fwdbwd_loop_us"], row["fwdbwd_loop_min_us"] = timed(fb_loop, a.reps, 3)
        row["fwd_speedup"] = row["fwd_loop_us"] / row["fwd_models_us"]
        row["fwdbwd_speedup"] = row["fwdbwd_loop_us"] / row["fwdbwd_models_us"]
        print(json.dumps(row), flush=True)
        res.append(row)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

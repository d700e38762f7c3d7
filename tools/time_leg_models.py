"""Time leg.log_likelihood_models against a Python loop of leg.log_likelihood_batch over the models (device events
after warm-up, as tools/time_leg_batch.py).

Workload: fp64, rank 5, obs_dim 1, B series of 502 rows from leg.co2_like_series with different seeds (standardised as
co2_workload does); M models: the model of tests/golden/leg_co2like.npz with every matrix perturbed by 5 % noise of its
own.  Cases: forward only, and forward + backward of out.sum() with all four matrices of every model trainable, for
(M, B) in --shapes.  Values and gradients are compared with the loop's before anything is timed.

    python tools/time_leg_models.py [--shapes 256x1,64x16,16x1024] [--reps 20] [--json out.json]

    python tools/time_leg_models.py --observed 0.7 [--obs-dims 1,3] [--loop-reps 3]
        every entry observed with probability 0.7 (another mask per series, shared by the models):
        log_likelihood_models_observed(observed=mask) against (i) the loop of log_likelihood_batch(observed=mask) over the models
        and (ii) the fully observed log_likelihood_models on the same shapes.  obs_dim 3 is time_leg_batch.noise_model's
        extension of the golden model and data.

    python tools/time_leg_models.py --noise [--obs-dims 1,3] [--loop-reps 3]
        every entry with a noise variance of its own, uniform in [0, 1]: log_likelihood_models_observed(noise_var=s) against the
        same two baselines, the gradient in noise_var included in the comparison.

--loop-reps: repetitions of the loop at shapes with more than 64 series (after one warm-up instead of three), as
tools/time_leg_batch.py has it; everything else takes --reps after three warm-ups.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cyclic-gps_amd"), os.path.join(ROOT, "tools")]
from cyclic_gps import leg  # noqa: E402
from time_leg_batch import noise_model, timed, workload  # noqa: E402


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


def row_for(M, B, obs_dim, keep, noise, reps, loop_reps):
    """One shape: the one call against the loop over the models (and, with a mask or noise, against the fully observed
    one call), values and gradients compared first."""
    m, ts, xs = workload(B)
    if obs_dim != 1:
        m, xs = noise_model(m, xs, obs_dim)
    ms = models(m, M)
    kw = {}
    if keep is not None:
        kw["observed"] = (torch.rand(xs.shape, generator=torch.Generator().manual_seed(B)) < keep).cuda()
    if noise:
        kw["noise_var"] = torch.rand(xs.shape, generator=torch.Generator().manual_seed(B + 1), dtype=xs.dtype).cuda()
    # the one call agrees with the loop before anything is timed
    with torch.no_grad():
        ref = torch.stack([leg.log_likelihood_batch(mk, ts, xs, **kw) for mk in ms])
        out = leg.log_likelihood_models_observed(ms, ts, xs, **kw)
    err = float(((out - ref).abs() / ref.abs().clamp_min(1.0)).max())
    assert err < 1e-9, err

    def fwd_models():
        with torch.no_grad():
            leg.log_likelihood_models_observed(ms, ts, xs, **kw)

    def fwd_full():
        with torch.no_grad():
            leg.log_likelihood_models(ms, ts, xs)

    def fwd_loop():
        with torch.no_grad():
            for mk in ms:
                leg.log_likelihood_batch(mk, ts, xs, **kw)

    mg = trainable(ms)
    kwg = dict(kw)
    if noise:
        kwg["noise_var"] = kw["noise_var"].clone().requires_grad_(True)
    leaves = [p for mk in mg for p in (mk.N, mk.R, mk.B, mk.Lambda)] + ([kwg["noise_var"]] if noise else [])

    def zero():
        for p in leaves:
            p.grad = None

    def fb_models():
        zero()
        leg.log_likelihood_models_observed(mg, ts, xs, **kwg).sum().backward()

    def fb_full():
        zero()
        leg.log_likelihood_models(mg, ts, xs).sum().backward()

    def fb_loop():
        zero()
        for mk in mg:
            leg.log_likelihood_batch(mk, ts, xs, **kwg).sum().backward()

    # ... and so do the gradients, every tensor relative to its own largest entry
    def grads(step):
        step()
        return [p.grad.clone() for p in leaves]

    gerr = max(float((g1 - g0).abs().max() / g0.abs().max()) for g1, g0 in zip(grads(fb_models), grads(fb_loop)))
    assert gerr < 1e-7, gerr

    row = {"M": M, "B": B, "rows": 502, "d": 5, "dtype": "float64", "max_rel_err_vs_loop": err,
           "max_rel_grad_err_vs_loop": gerr}
    if kw:
        row.update({"obs_dim": obs_dim, "observed": keep, "noise": noise})
    lr, lw = (reps, 3) if B <= 64 or loop_reps is None else (loop_reps, 1)
    row["loop_reps"] = lr
    row["fwd_models_us"], row["fwd_models_min_us"] = timed(fwd_models, reps, 3)
    row["fwd_loop_us"], row["fwd_loop_min_us"] = timed(fwd_loop, lr, lw)
    row["fwdbwd_models_us"], row["fwdbwd_models_min_us"] = timed(fb_models, reps, 3)
    row["fwdbwd_loop_us"], row["fwdbwd_loop_min_us"] = timed(fb_loop, lr, lw)
    row["fwd_speedup"] = row["fwd_loop_us"] / row["fwd_models_us"]
    row["fwdbwd_speedup"] = row["fwdbwd_loop_us"] / row["fwdbwd_models_us"]
    if kw:                                                  # (ii) the fully observed one call on the same shapes
        row["fwd_full_us"], row["fwd_full_min_us"] = timed(fwd_full, reps, 3)
        row["fwdbwd_full_us"], row["fwdbwd_full_min_us"] = timed(fb_full, reps, 3)
        row["fwd_ratio_to_full"] = row["fwd_models_us"] / row["fwd_full_us"]
        row["fwdbwd_ratio_to_full"] = row["fwdbwd_models_us"] / row["fwdbwd_full_us"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x1,64x16,16x1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--observed", type=float, default=None, metavar="KEEP")
    ap.add_argument("--noise", action="store_true")
    ap.add_argument("--obs-dims", default=None)
    a = ap.parse_args()
    masked = a.observed is not None or a.noise
    obs_dims = [int(x) for x in (a.obs_dims or ("1,3" if masked else "1")).split(",")]
    res = []
    for shape in a.shapes.split(","):
        M, B = (int(x) for x in shape.split("x"))
        for obs_dim in obs_dims:
            row = row_for(M, B, obs_dim, a.observed, a.noise, a.reps, a.loop_reps)
            print(json.dumps(row), flush=True)
            res.append(row)
            if a.json:                                      # (after every row: a long run leaves what it has)
                os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
                with open(a.json, "w") as f:
                    json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

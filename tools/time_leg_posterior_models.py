"""Time the posterior and the predictions of many LEG models over one batch in one call (leg.insample_posterior_models,
predict.make_predictions_models: DESIGN.md 4.18) against a Python loop of the batched calls over the models (device
events after warm-up, as tools/time_leg_models.py).

Workload: fp64, rank 5, obs_dim 1, B series of 502 rows from leg.co2_like_series with different seeds (standardised as
co2_workload does), the 784 targets of tests/golden/leg_co2like.npz for every series; M models: the model of that file
with every matrix perturbed by 5 % noise of its own (tools/time_leg_models.models).  Cases, for (M, B) in --shapes:
  predictions         make_predictions_models against the loop of make_predictions_batch over the models;
  latent              predictive_posterior_models against the loop of predictive_posterior_batch (the same without the
                      image under every model's B);
  posterior_observed  insample_posterior_models(observed=mask), every entry kept with probability --observed, against the
                      loop of insample_posterior_batch(observed=mask);
  assembly            cgps_leg_posterior_blocks_models alone (plain and table source) against cgps_peg_precision_models
                      plus the torch add of the rows' terms that it replaces, alternated inside every repetition.
The one call is compared with the loop before anything is timed.  Median (and minimum) of --reps calls after three
warm-ups; at shapes with more than 64 series --big-reps calls.

    python tools/time_leg_posterior_models.py [--shapes 256x1,64x16,16x1024] [--reps 20] [--big-reps 5] [--json out.json]
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
from time_leg_batch import timed, timed_alternating, workload  # noqa: E402
from time_leg_models import models  # noqa: E402


def rel_err(got, want):
    return float(((got - want).abs() / want.abs().clamp_min(1.0)).max())


def row_for(M, B, keep, reps):
    m, ts, xs = workload(B)
    ms = models(m, M)
    g = np.load(os.path.join(ROOT, "tests", "golden", "leg_co2like.npz"))
    tt = torch.from_numpy(g["target_ts"]).to(ts.dtype).cuda()
    observed = (torch.rand(xs.shape, generator=torch.Generator().manual_seed(B)) < keep).cuda()
    row = {"M": M, "B": B, "rows": int(ts.shape[1]), "targets": int(tt.shape[0]), "d": 5, "dtype": "float64", "observed": keep,
           "reps": reps}

    def pred_models():
        return predict.make_predictions_models(ms, ts, xs, tt)

    def pred_loop():
        return [predict.make_predictions_batch(mk, ts, xs, tt) for mk in ms]

    def latent_models():
        return predict.predictive_posterior_models(ms, ts, xs, tt)

    def latent_loop():
        return [predict.predictive_posterior_batch(mk, ts, xs, tt) for mk in ms]

    def post_models():
        return leg.insample_posterior_models(ms, ts, xs, observed=observed)

    def post_loop():
        return [leg.insample_posterior_batch(mk, ts, xs, observed=observed) for mk in ms]

    # the one call agrees with the loop before anything is timed (model by model: the loop's results are not kept)
    pm, pv = pred_models()
    mean, (Sd, So) = post_models()
    err = 0.0
    for k, mk in enumerate(ms):
        rm, rv = predict.make_predictions_batch(mk, ts, xs, tt)
        qm, (qd, qo) = leg.insample_posterior_batch(mk, ts, xs, observed=observed)
        err = max(err, rel_err(pm[k], rm), rel_err(pv[k], rv), rel_err(mean[k], qm), rel_err(Sd[k], qd), rel_err(So[k], qo))
    assert err < 1e-8, err
    row["max_rel_err_vs_loop"] = err
    del pm, pv, mean, Sd, So, rm, rv, qm, qd, qo

    row["predictions_models_us"], row["predictions_models_min_us"] = timed(pred_models, reps, 3)
    row["predictions_loop_us"], row["predictions_loop_min_us"] = timed(pred_loop, reps, 3)
    row["predictions_speedup"] = row["predictions_loop_us"] / row["predictions_models_us"]
    row["latent_models_us"], row["latent_models_min_us"] = timed(latent_models, reps, 3)
    row["latent_loop_us"], row["latent_loop_min_us"] = timed(latent_loop, reps, 3)
    row["latent_speedup"] = row["latent_loop_us"] / row["latent_models_us"]
    row["posterior_observed_models_us"], row["posterior_observed_models_min_us"] = timed(post_models, reps, 3)
    row["posterior_observed_loop_us"], row["posterior_observed_loop_min_us"] = timed(post_loop, reps, 3)
    row["posterior_observed_speedup"] = row["posterior_observed_loop_us"] / row["posterior_observed_models_us"]

    # the assembly alone, on operands built once, one chunk's worth of models
    with torch.no_grad():
        _, mats, tsf, xsf, lens, obs2, _, _, _ = leg._models_posterior_args(ms, ts, xs, None, observed, None)
        plan = leg._cached_batch_plan(lens, tsf.device)
        per = min(M, max(1, leg.MODELS_POSTERIOR_MAX_ROWS // plan.R))
        mats = tuple(t[:per] for t in mats)
        R, d = plan.R, 5
        for name, ob in (("plain", None), ("table", obs2)):
            G, source, term, rows, _ = leg._models_posterior_operands(mats, xsf, ob, None)
            idx = None if rows is None else rows.long().clamp(max=term.shape[1] - 1)

            def fused():
                return leg._posterior_blocks_models(tsf, G, plan.cut, source, term, rows)

            def composed():
                Rs, Os = leg._peg_precision_models(tsf, G, plan.cut)
                add = term.unsqueeze(1) if source == _hip.ROWS_PLAIN else term[:, idx]
                return (Rs.view(per, R, d, d) + add).view(per * R, d, d), Os

            K, Ko, _ = fused()
            Kc, Koc = composed()
            assert torch.equal(K, Kc) and torch.equal(Ko, Koc)
            del K, Ko, Kc, Koc
            t = timed_alternating({"fused": fused, "composed": composed}, reps, 3)
            row["assembly_%s_models" % name] = per
            row["assembly_%s_fused_us" % name], row["assembly_%s_fused_min_us" % name] = t["fused"]
            row["assembly_%s_composed_us" % name], row["assembly_%s_composed_min_us" % name] = t["composed"]
            row["assembly_%s_speedup" % name] = t["composed"][0] / t["fused"][0]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x1,64x16,16x1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--big-reps", type=int, default=5)
    ap.add_argument("--observed", type=float, default=0.7, metavar="KEEP")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = []
    for shape in a.shapes.split(","):
        M, B = (int(x) for x in shape.split("x"))
        row = row_for(M, B, a.observed, a.reps if B <= 64 else a.big_reps)
        print(json.dumps(row), flush=True)
        res.append(row)
        if a.json:                                          # (after every row: a long run leaves what it has)
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

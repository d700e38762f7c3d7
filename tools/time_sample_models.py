"""Time posterior paths under many LEG models in one call (leg.sample_from_posterior_models) and replicated
observations (leg.sample_observations_batch / cgps_leg_observations): DESIGN.md 4.21.  Device events, median (and
minimum) of --reps calls after three warm-ups, --big-reps calls at shapes with more than 64 series, as
tools/time_leg_posterior_models.py.

Workload: fp64, rank 5, obs_dim 1, B series of 502 rows (tools/time_leg_batch.workload), S = 8 samples; M models: the
model of tests/golden/leg_co2like.npz with every matrix perturbed by 5 % noise of its own (tools/time_leg_models.models).
For (M, B) in --shapes:
  sample            sample_from_posterior_models against the Python loop of sample_from_posterior_batch over the models
                    (the loop is the code as it stood before the models call existed);
  operands          the part of the models call that is still a loop over the models: ``_models_sampling_operands``;
  perturbation      cgps_leg_perturbation_models alone, one chunk's worth of models, against the loop of
                    cgps_leg_perturbation_seg launches it replaces;
  observations      cgps_leg_observations alone (all models, plain and with mask + variances);
  replicate_batch   sample_observations_batch (model 0) against the torch composition of leg.sample_observations:
                    cr.standard_normal + baddbmm, with a per-row factor from torch.linalg.cholesky when noise_var is given.
The one call is compared with the loop before anything is timed.

    python tools/time_sample_models.py [--shapes 256x1,64x16,16x1024] [--reps 20] [--big-reps 5] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cyclic-gps_amd"), os.path.join(ROOT, "tools")]
from cyclic_gps import leg  # noqa: E402
import cyclic_gps.cyclic_reduction as cr  # noqa: E402
from time_leg_batch import timed, timed_alternating, workload  # noqa: E402
from time_leg_models import models  # noqa: E402

S, SEED = 8, 7


def row_for(M, B, reps):
    m, ts, xs = workload(B)
    ms = models(m, M)
    n, d, obs = int(ts.shape[1]), 5, 1
    row = {"M": M, "B": B, "rows": n, "d": d, "dtype": "float64", "S": S, "reps": reps}

    def sample_models():
        return leg.sample_from_posterior_models(ms, ts, xs, S, SEED)

    def sample_loop():
        return [leg.sample_from_posterior_batch(mk, ts, xs, S, SEED, stream=4 * k) for k, mk in enumerate(ms)]

    z = sample_models()
    err = 0.0
    for k, mk in enumerate(ms):
        zk = leg.sample_from_posterior_batch(mk, ts, xs, S, SEED, stream=4 * k)
        err = max(err, float(((z[k] - zk).abs() / zk.abs().clamp_min(1.0)).max()))
        assert torch.equal(leg.posterior_perturbation_models([mk], ts, xs, S, SEED, stream=4 * k)[0],
                           leg.posterior_perturbation_batch(mk, ts, xs, S, SEED, stream=4 * k))
    assert err < 1e-7, err
    row["max_rel_err_vs_loop"] = err
    del zk
    row["sample_models_us"], row["sample_models_min_us"] = timed(sample_models, reps, 3)
    row["sample_loop_us"], row["sample_loop_min_us"] = timed(sample_loop, reps, 3)
    row["sample_speedup"] = row["sample_loop_us"] / row["sample_models_us"]

    with torch.no_grad():
        tsf, xsf = ts.reshape(-1), xs.reshape(-1, obs)
        lens = [n] * B
        plan = leg._cached_batch_plan(lens, tsf.device)
        ids = leg._series_ids_arg(None, lens, d, obs, tsf.device)
        row["operands_us"], row["operands_min_us"] = timed(lambda: leg._models_sampling_operands(ms, tsf, xsf, None, None), reps, 3)
        per = min(M, max(1, leg.MODELS_POSTERIOR_MAX_ROWS // plan.R))
        G, _, _, _, v, hsource, hterm, _ = leg._models_sampling_operands(ms[:per], tsf, xsf, None, None)
        words = torch.arange(per, dtype=torch.int64, device=tsf.device) * 4

        def pert_models():
            return leg._perturbation_models(tsf, G, plan, ids, hsource, hterm, None, v, S, SEED, words)

        def pert_loop():
            return [leg._perturbation_models(tsf, G[k], plan, ids, hsource, hterm[k], None, v[k], S, SEED, 4 * k) for k in range(per)]

        one = pert_models().view(per, plan.R, d, S)
        assert all(torch.equal(one[k], r) for k, r in enumerate(pert_loop()))
        del one
        t = timed_alternating({"models": pert_models, "loop": pert_loop}, reps, 3)
        row["perturbation_models"] = per
        row["perturbation_models_us"], row["perturbation_models_min_us"] = t["models"]
        row["perturbation_loop_us"], row["perturbation_loop_min_us"] = t["loop"]
        row["perturbation_speedup"] = t["loop"][0] / t["models"][0]

        # replicated observations: the launch alone for all models, then one model against the torch composition
        gen = torch.Generator().manual_seed(B)
        observed = (torch.rand(plan.R, obs, generator=gen) < 0.7).cuda()
        nv = (0.5 * torch.rand(plan.R, obs, generator=gen, dtype=torch.float64)).cuda()
        Bm = torch.stack([mk.B for mk in ms]).contiguous()
        LLT = torch.stack([mk.LLT for mk in ms]).contiguous()
        wd = torch.arange(M, dtype=torch.int64, device=tsf.device) * 4
        zf = z.reshape(M * plan.R, d, S)
        _, pattern, nvc = leg._loo_data(xsf[:0], observed, nv, torch.float64)
        t = timed_alternating({"plain": lambda: leg._observations_rows(zf, None, None, plan, ids, Bm, LLT, SEED, wd),
                               "masked_noise": lambda: leg._observations_rows(zf, pattern, nvc, plan, ids, Bm, LLT, SEED, wd)}, reps, 3)
        row["observations_plain_us"], row["observations_plain_min_us"] = t["plain"]
        row["observations_masked_noise_us"], row["observations_masked_noise_min_us"] = t["masked_noise"]
        moved = 8 * M * plan.R * S * (d + obs)                       # z read once, x written once
        row["observations_plain_gbps"] = moved / t["plain"][0] / 1e3

        m0, z0 = ms[0], z[0].reshape(plan.R, d, S).contiguous()

        def composed_plain():
            return leg.sample_observations(m0, z0, SEED, stream=2)

        def composed_noise():
            eps = cr.standard_normal(plan.R * obs, S, SEED, stream=2, dtype=z0.dtype, device=z0.device).reshape(plan.R, obs, S)
            sv = torch.where(observed, nv, torch.zeros((), dtype=nv.dtype, device=nv.device))
            T = torch.linalg.cholesky(m0.LLT + torch.diag_embed(sv))
            return torch.baddbmm(torch.matmul(T, eps), m0.B.expand(plan.R, -1, -1), z0)

        t = timed_alternating({"kernel_plain": lambda: leg.sample_observations_batch(m0, z0, SEED, lengths=lens),
                               "composed_plain": composed_plain,
                               "kernel_noise": lambda: leg.sample_observations_batch(m0, z0, SEED, lengths=lens, observed=observed, noise_var=nv),
                               "composed_noise": composed_noise}, reps, 3)
        for k_, v_ in t.items():
            row["replicate_batch_%s_us" % k_], row["replicate_batch_%s_min_us" % k_] = v_
        row["replicate_batch_plain_speedup"] = t["composed_plain"][0] / t["kernel_plain"][0]
        row["replicate_batch_noise_speedup"] = t["composed_noise"][0] / t["kernel_noise"][0]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x1,64x16,16x1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--big-reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = []
    for shape in a.shapes.split(","):
        M, B = (int(x) for x in shape.split("x"))
        row = row_for(M, B, a.reps if B <= 64 else a.big_reps)
        print(json.dumps(row), flush=True)
        res.append(row)
        if a.json:                                          # (after every row: a long run leaves what it has)
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

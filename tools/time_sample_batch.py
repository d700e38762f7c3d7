"""Time leg.sample_from_posterior_batch (perturb and solve) against a Python loop of
leg.sample_from_posterior, and against cr.sample off the factor of the concatenated system (the sampler whose draws
would depend on a series' position in the batch), device events: median of --reps after 3 warm-ups.

Workload: fp64, rank 5, obs_dim 1, the model of tests/golden/leg_co2like.npz, B series of 502 rows from
leg.co2_like_series with different seeds (standardised as co2_workload does), S = 8 samples.

    python tools/time_sample_batch.py [--batches 64,1024] [--samples 8] [--reps 20] [--loop-reps 3] [--json out.json]
        per B: batch_us (the whole call), its parts perturbation_us (operands of H and v, the assembly, the
        cgps_leg_perturbation_seg launch), kernel_us (that launch alone), decompose_us and solve_us; loop_us (one
        leg.sample_from_posterior per series); concat_us (the posterior system, cr.decompose_solve and cr.sample on the
        concatenated system).
    python tools/time_sample_batch.py --profile-only --batches 1024
        the batched call only, the program to put after  rocprofv3 --kernel-trace --stats --
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cyclic-gps_amd"), os.path.join(ROOT, "tools")]
from cyclic_gps import _hip, leg  # noqa: E402
import cyclic_gps.cyclic_reduction as cr  # noqa: E402
from time_leg_posterior_batch import timed, workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile-only", action="store_true")
    a = ap.parse_args()
    S, seed, res = a.samples, 2024, []
    for B in [int(x) for x in a.batches.split(",")]:
        m, ts, xs, _ = workload(B)
        n = ts.shape[1]

        def batch():
            return leg.sample_from_posterior_batch(m, ts, xs, S, seed)

        if a.profile_only:
            for _ in range(a.reps):
                batch()
            torch.cuda.synchronize()
            continue

        def loop():
            for b in range(B):
                leg.sample_from_posterior(m, ts[b], xs[b], S, seed)

        plan = leg._cached_batch_plan([n] * B, ts.device)
        tsf, xsf = ts.reshape(-1), xs.reshape(B * n, -1)
        ids = torch.arange(B, dtype=torch.int64, device=ts.device)

        def concat():
            with torch.no_grad():
                source, term, rows, v = leg._posterior_operands_batch(m, tsf, xsf, None, None)
                K_Rs, K_Os = leg._posterior_system_rows(plan, tsf, m.G.contiguous(), source, term, rows, None)
                dec, mean = cr.decompose_solve(K_Rs, K_Os, v)
                return cr.sample(dec, S, seed, mean=mean)

        def perturbation():
            with torch.no_grad():
                return leg._posterior_perturbation_flat(m, tsf, xsf, None, None, plan, ids, S, seed, 0)

        K_Rs, K_Os, rhs = perturbation()
        G, H = m.G.contiguous(), leg.observation_noise_factors(m).contiguous()
        v = leg._posterior_operands_batch(m, tsf, xsf, None, None)[3]
        dec = cr.decompose(K_Rs, K_Os)

        def kernel():
            return leg._perturbation_models(tsf, G, plan, ids, _hip.H_PLAIN, H, None, v, S, seed, 0)

        # the batched draws have the posterior's mean and spread before anything is timed (64 draws of one series
        # against leg.insample_posterior: a coarse check, the tests hold the exact ones)
        x = leg.sample_from_posterior_batch(m, ts[:1], xs[:1], 64, seed)[0]
        mean, (Sd, _) = leg.insample_posterior(m, ts[0], xs[0])
        z = (x.mean(-1) - mean) / torch.sqrt(torch.diagonal(Sd, dim1=1, dim2=2) / 64)
        assert float(z.abs().max()) < 6.0, float(z.abs().max())

        loop_reps = a.loop_reps if B > 64 else a.reps
        row = {"B": B, "rows": n, "d": 5, "dtype": "float64", "samples": S}
        for name, fn, reps, warm in (("batch", batch, a.reps, 3), ("perturbation", perturbation, a.reps, 3),
                                     ("kernel", kernel, a.reps, 3), ("decompose", lambda: cr.decompose(K_Rs, K_Os), a.reps, 3),
                                     ("solve", lambda: cr.solve(dec, rhs), a.reps, 3), ("concat", concat, a.reps, 3),
                                     ("loop", loop, loop_reps, 1)):
            row[name + "_us"], row[name + "_min_us"] = timed(fn, reps, warm)
        row["speedup_vs_loop"] = row["loop_us"] / row["batch_us"]
        row["ratio_to_concat"] = row["batch_us"] / row["concat_us"]
        print(json.dumps(row), flush=True)
        res.append(row)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

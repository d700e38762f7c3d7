"""Time the LEG reductions of a series with per-observation noise variances (device events after warm-up, the variants
alternated inside every repetition of one process).

Workload: fp64, rank 5, N and R of tests/golden/leg_co2like.npz; n = 502 (leg.co2_like_series) and n = 2^20 (regular
grid, random data); noise variances uniform in [0, 1].  Two observation models: obs_dim 1 (the golden B and Lambda, one
basis block, Kb = 1) and obs_dim 3 (B and Lambda drawn once from a fixed seed, Kb = 6; the data of the three channels
are the one series plus noise).  Variants:
  w_fused      (a) leg.leg_loglik_reductions_w: one launch, row i adds sum_k weights[i, k] basis[k] in registers
               (cgps_leg_mahal_logdet_pair_w)
  w_unfused    (b) the same system through memory: peg_precision, Rs + einsum(weights, basis), two cr.mahal_and_det
  const_fused  (c) leg.leg_loglik_reductions of the same series with the one constant noise Lambda Lambda^T
               (cgps_leg_mahal_logdet_pair): what the per-row term costs is w_fused - const_fused
  ll_noise     leg.log_likelihood(m, ts, xs, noise_var=s) end to end (weights, the fused call, the scalars)
The positive-definiteness check (a device -> host read per call) is off while timing.

    python tools/time_leg_noise.py [--sizes 502,1048576] [--obs 1,3] [--reps 30] [--json out.json]
    python tools/time_leg_noise.py --profile-only --sizes 1048576    (fused calls only, for rocprofv3 --kernel-trace --stats)
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
import cyclic_gps.cyclic_reduction as cr  # noqa: E402


def workload(n, obs, dtype=torch.float64):
    g = np.load(os.path.join(ROOT, "tests", "golden", "leg_co2like.npz"))
    mats = {k: torch.from_numpy(g[k]).to(dtype) for k in ("N", "R", "B", "Lambda")}
    gen = torch.Generator().manual_seed(n + obs)
    if obs > 1:
        d = mats["N"].shape[0]
        mats["B"] = mats["B"].abs().mean() * torch.randn(obs, d, generator=gen, dtype=dtype)
        mats["Lambda"] = torch.tril(0.2 * torch.randn(obs, obs, generator=gen, dtype=dtype)) + 0.6 * torch.eye(obs, dtype=dtype)
    m = leg.LEGMatrices(*(mats[k].cuda() for k in ("N", "R", "B", "Lambda")))
    if n <= 4096:
        t, x = leg.co2_like_series(rows=n, seed=0, dtype=dtype)
        ts, xs = 12 * (t - t.min()), (x - x.mean()) / x.std()
    else:
        ts, xs = 0.25 * torch.arange(n, dtype=dtype), torch.randn(n, 1, generator=gen, dtype=dtype)
    if obs > 1:
        xs = xs + 0.1 * torch.randn(n, obs, generator=gen, dtype=dtype)
    s = torch.rand(n, obs, generator=gen, dtype=dtype)
    return m, ts.cuda(), xs.cuda(), s.cuda()


def timed_alternating(fns, reps, warmup):
    """{name: (median us, min us)}: every repetition runs each variant once, in turn."""
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
    ap.add_argument("--sizes", default="502,1048576")
    ap.add_argument("--obs", default="1,3")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile-only", action="store_true")
    a = ap.parse_args()
    res = []
    cr.CHECK_POSITIVE_DEFINITE = False
    with torch.no_grad():
        for n in [int(x) for x in a.sizes.split(",")]:
            for obs in [int(x) for x in a.obs.split(",")]:
                m, ts, xs, s = workload(n, obs)
                G = m.G.contiguous()
                basis, weights, Li_rows, _ = leg.observation_weights(m, None, s)
                basis, weights = basis.contiguous(), weights.contiguous()
                v = ((xs.unsqueeze(1) @ Li_rows).squeeze(1) @ m.B).contiguous()
                A_const, v_const = (m.B.T @ m.LLT_inv @ m.B).contiguous(), leg.compute_v(m, xs)
                if a.profile_only:
                    for _ in range(a.reps):
                        leg.leg_loglik_reductions_w(ts, G, basis, weights, v)
                        leg.leg_loglik_reductions(ts, G, A_const, v_const)
                    torch.cuda.synchronize()
                    continue

                def w_unfused():
                    Rs, Os = leg.peg_precision(ts, G)
                    _, sg = cr.mahal_and_det(Rs, Os, torch.zeros_like(v))
                    km, kd = cr.mahal_and_det(Rs + torch.einsum("nk,kij->nij", weights, basis), Os, v)
                    return km, kd, sg

                fns = {"w_fused": lambda: leg.leg_loglik_reductions_w(ts, G, basis, weights, v),
                       "w_unfused": w_unfused,
                       "const_fused": lambda: leg.leg_loglik_reductions(ts, G, A_const, v_const),
                       "ll_noise": lambda: leg.log_likelihood(m, ts, xs, noise_var=s)}
                # the fused call agrees with the unfused composition before anything is timed
                got, want = fns["w_fused"](), w_unfused()
                err = max(abs(float(x) - float(y)) / max(1.0, abs(float(y))) for x, y in zip(got, want))
                assert err < 1e-8, err
                row = {"n": n, "d": 5, "dtype": "float64", "obs": obs, "Kb": int(basis.shape[0]), "max_rel_err_vs_unfused": err}
                for k, (med, mn) in timed_alternating(fns, a.reps, 3).items():
                    row[k + "_us"], row[k + "_min_us"] = med, mn
                row["fused_speedup_vs_unfused"] = row["w_unfused_us"] / row["w_fused_us"]
                row["per_row_term_cost_us"] = row["w_fused_us"] - row["const_fused_us"]
                print(json.dumps(row), flush=True)
                res.append(row)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

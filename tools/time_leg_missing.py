"""Time the LEG reductions of a series with missing rows (device events after warm-up, the variants alternated
inside every repetition of one process).

Workload: fp64, rank 5, obs_dim 1, the model of tests/golden/leg_co2like.npz; n = 502 (leg.co2_like_series) and
n = 2^20 (regular grid, random data); 30 % of the rows missing at random.  Variants:
  obs_fused    leg.leg_loglik_reductions_obs: one launch, row i adds A_table[pattern[i]]  (cgps_leg_mahal_logdet_pair_obs)
  obs_unfused  the same system through memory: peg_precision, Rs + A_table[pattern], two cr.mahal_and_det
  full_fused   leg.leg_loglik_reductions of the same series fully observed (cgps_leg_mahal_logdet_pair): what the
               per-row indirection costs is obs_fused - full_fused
  ll_observed  leg.log_likelihood(m, ts, xs, observed=mask) end to end (tables, gathers, the fused call, the scalars)
The positive-definiteness check (a device -> host read per call) is off while timing.

    python tools/time_leg_missing.py [--sizes 502,1048576] [--reps 30] [--json out.json]
    python tools/time_leg_missing.py --profile-only --sizes 1048576    (fused calls only, for rocprofv3 --kernel-trace --stats)
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


def workload(n, dtype=torch.float64):
    g = np.load(os.path.join(ROOT, "tests", "golden", "leg_co2like.npz"))
    m = leg.LEGMatrices(*(torch.from_numpy(g[k]).to(dtype).cuda() for k in ("N", "R", "B", "Lambda")))
    gen = torch.Generator().manual_seed(n)
    if n <= 4096:
        t, x = leg.co2_like_series(rows=n, seed=0, dtype=dtype)
        ts, xs = 12 * (t - t.min()), (x - x.mean()) / x.std()
    else:
        ts, xs = 0.25 * torch.arange(n, dtype=dtype), torch.randn(n, 1, generator=gen, dtype=dtype)
    mask = torch.rand(n, generator=gen) > 0.3
    return m, ts.cuda(), xs.cuda(), mask.cuda()


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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile-only", action="store_true")
    a = ap.parse_args()
    res = []
    cr.CHECK_POSITIVE_DEFINITE = False
    with torch.no_grad():
        for n in [int(x) for x in a.sizes.split(",")]:
            m, ts, xs, mask = workload(n)
            G = m.G.contiguous()
            pattern, A_table, Li_table, _ = leg.observation_tables(m, mask)
            idx = pattern.long()
            A_table = A_table.contiguous()
            xz = torch.where(mask.unsqueeze(-1), xs, torch.zeros_like(xs))
            v = ((xz.unsqueeze(1) @ Li_table[idx]).squeeze(1) @ m.B).contiguous()
            A_full, v_full = A_table[-1].contiguous(), leg.compute_v(m, xs)
            if a.profile_only:
                for _ in range(a.reps):
                    leg.leg_loglik_reductions_obs(ts, G, A_table, pattern, v)
                    leg.leg_loglik_reductions(ts, G, A_full, v_full)
                torch.cuda.synchronize()
                continue

            def obs_unfused():
                Rs, Os = leg.peg_precision(ts, G)
                _, s = cr.mahal_and_det(Rs, Os, torch.zeros_like(v))
                km, kd = cr.mahal_and_det(Rs + A_table[idx], Os, v)
                return km, kd, s

            fns = {"obs_fused": lambda: leg.leg_loglik_reductions_obs(ts, G, A_table, pattern, v),
                   "obs_unfused": obs_unfused,
                   "full_fused": lambda: leg.leg_loglik_reductions(ts, G, A_full, v_full),
                   "ll_observed": lambda: leg.log_likelihood(m, ts, xs, observed=mask)}
            # the fused call agrees with the unfused composition before anything is timed
            got, want = fns["obs_fused"](), obs_unfused()
            err = max(abs(float(x) - float(y)) / max(1.0, abs(float(y))) for x, y in zip(got, want))
            assert err < 1e-8, err
            row = {"n": n, "d": 5, "dtype": "float64", "missing_rows": int((~mask).sum()), "max_rel_err_vs_unfused": err}
            for k, (med, mn) in timed_alternating(fns, a.reps, 3).items():
                row[k + "_us"], row[k + "_min_us"] = med, mn
            row["fused_speedup_vs_unfused"] = row["obs_unfused_us"] / row["obs_fused_us"]
            row["indirection_cost_us"] = row["obs_fused_us"] - row["full_fused_us"]
            print(json.dumps(row), flush=True)
            res.append(row)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

"""Time the gradient of the Laplace evidence (leg.laplace_posterior_batch(differentiable=True), cgps_leg_glm_evidence_rhs,
cgps_leg_glm_evidence_adjoint: DESIGN.md 4.27) -- device events, median of --reps calls after 3 warm-ups, the variants of
a comparison alternated inside every repetition.  No threshold: the numbers go into README.md and DESIGN.md 4.27.

Workload: that of tools/time_laplace.py -- fp64, rank 5, series of 502 rows, 70 % of the entries observed, obs_dim 1 and
3, Poisson counts with an offset of 1.

    python tools/time_laplace_grad.py [--obs 1,3] [--batches 64,1024] [--reps 10] [--json out.json]
        per (obs_dim, B):
          laplace_us            leg.laplace_posterior_batch, the plain inference call
          value_and_grad_us     the differentiable call and the backward of log_evidence.sum() in N, R, B, offset and ts
          value_and_grad_composed_us   the same with CGPS_LEG_GLM_COMPOSED=1 (step and both gradient entries from torch passes)
          rhs_kernel_us, rhs_composed_us          cgps_leg_glm_evidence_rhs alone and its torch composition
          adjoint_kernel_us, adjoint_composed_us  cgps_leg_glm_evidence_adjoint alone and its torch composition
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cyclic-gps_amd"), os.path.join(ROOT, "tools")]
from cyclic_gps import leg  # noqa: E402
from time_laplace import composed  # noqa: E402
from time_loo import data, model, timed_alternating  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", default="1,3")
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    results = []
    for obs in (int(v) for v in a.obs.split(",")):
        for B in (int(v) for v in a.batches.split(",")):
            m0 = model(obs)
            m = leg.LEGMatrices(*(t.detach().clone().requires_grad_(True) for t in (m0.N, m0.R, m0.B)), m0.Lambda.detach())
            ts, xs, observed, _ = data(B, obs)
            ts = ts.detach().clone().requires_grad_(True)
            gen = torch.Generator().manual_seed(7 * B + obs)
            ys = torch.poisson(torch.exp(1 + 0.5 * xs.cpu()), generator=gen).cuda()
            offset = torch.ones(obs, dtype=xs.dtype, device="cuda", requires_grad=True)
            kw = dict(family="poisson", observed=observed, offset=offset)
            leaves = [m.N, m.R, m.B, offset, ts]

            def value_and_grad():
                r = leg.laplace_posterior_batch(m, ts, ys, differentiable=True, allow_unconverged=True, **kw)
                return torch.autograd.grad(r.log_evidence.sum(), leaves)

            r = leg.laplace_posterior_batch(m, ts, ys, differentiable=True, allow_unconverged=True, **kw)
            sv = leg._laplace_saved(r.log_evidence)
            op, blocks = sv["op"], [sv[k] for k in ("z", "u", "Sd", "So", "Pd", "Po")]
            gE = torch.ones(B, dtype=torch.float64, device="cuda")
            fns = {
                "laplace_us": lambda: leg.laplace_posterior_batch(m, ts, ys, **kw),
                "value_and_grad_us": value_and_grad,
                "value_and_grad_composed_us": composed(value_and_grad),
                "rhs_kernel_us": lambda: leg._glm_evidence_rhs_hip(op, sv["z"], sv["Sd"]),
                "rhs_composed_us": lambda: leg._glm_evidence_rhs_composed(op, sv["z"], sv["Sd"]),
                "adjoint_kernel_us": lambda: leg._glm_evidence_adjoint_hip(op, *blocks, gE),
                "adjoint_composed_us": lambda: leg._glm_evidence_adjoint_composed(op, *blocks, gE),
            }
            t = timed_alternating(fns, a.reps)
            row = {"obs": obs, "B": B, "rows": xs.shape[1], "iterations": int(r.iterations.max()), "converged": bool(r.converged.all())}
            row.update({k_: round(v[0], 1) for k_, v in t.items()})
            results.append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()

"""Time the Laplace posterior for Poisson counts (leg.laplace_posterior_batch, cgps_leg_glm_step: DESIGN.md 4.26) -- device
events, median of --reps calls after 3 warm-ups, the variants of a comparison alternated inside every repetition.  No
threshold: the numbers go into README.md and DESIGN.md 4.26.

Workload: the shapes of tools/time_loo.py -- fp64, rank 5, series of 502 rows, 70 % of the entries observed, obs_dim 1
and 3 -- with counts drawn as Poisson(exp(1 + x / 2)) from the standardised series x and an offset of 1.

    python tools/time_laplace.py [--obs 1,3] [--batches 64,1024] [--reps 10] [--loop-series 64] [--json out.json]
        per (obs_dim, B):
          step_kernel_us      one launch of cgps_leg_glm_step on the second Newton step's operands
          step_composed_us    the same step as torch passes (CGPS_LEG_GLM_COMPOSED=1 takes it)
          laplace_us          leg.laplace_posterior_batch, the whole call; `iterations` the most any series took
          laplace_composed_us the whole call with the composed step
          loop_us             a Python loop of leg.laplace_posterior over the first --loop-series series, scaled to B
                              (timed once: it is long)
          gaussian_us         leg.insample_posterior_batch on the same shapes and mask: the cost of ONE Gaussian posterior
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
from time_loo import data, model, timed_alternating  # noqa: E402


def step_operands(m, ts, ys, observed, offset):
    """(op, z, prop, state) of the second Newton step of the batch"""
    B, n, obs = ys.shape
    dt, dev = ys.dtype, ys.device
    plan = leg._cached_batch_plan([n] * B, dev)
    Rs, Os = leg._peg_precision_seg(ts.reshape(-1).contiguous(), m.G.contiguous(), plan.cut)
    op = leg._GlmOperands(plan, Rs, Os, ys.reshape(B * n, obs).contiguous(), observed.reshape(B * n, obs).contiguous(), offset,
                          None, m.B.contiguous(), _hip.GLM_POISSON, leg.LAPLACE_TOL[dt])
    z = torch.zeros(B * n, m.N.shape[0], dtype=dt, device=dev)
    z, J, rhs, state = leg._glm_step_hip(op, z, None, None)
    z, J, rhs, state = leg._glm_step_hip(op, z, cr.decompose_solve(J, Os, rhs)[1], state)
    return op, z, cr.decompose_solve(J, Os, rhs)[1], state


def composed(fn):
    def run():
        os.environ["CGPS_LEG_GLM_COMPOSED"] = "1"
        try:
            return fn()
        finally:
            del os.environ["CGPS_LEG_GLM_COMPOSED"]
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", default="1,3")
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--loop-series", type=int, default=64)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    results = []
    for obs in (int(v) for v in a.obs.split(",")):
        for B in (int(v) for v in a.batches.split(",")):
            m = model(obs)
            ts, xs, observed, _ = data(B, obs)
            gen = torch.Generator().manual_seed(7 * B + obs)
            ys = torch.poisson(torch.exp(1 + 0.5 * xs.cpu()), generator=gen).cuda()
            offset = torch.ones(obs, dtype=xs.dtype, device="cuda")
            kw = dict(family="poisson", observed=observed, offset=offset)
            op, z, prop, state = step_operands(m, ts, ys, observed, offset)
            whole = lambda: leg.laplace_posterior_batch(m, ts, ys, **kw)      # noqa: E731
            fns = {
                "step_kernel_us": lambda: leg._glm_step_hip(op, z, prop, state),
                "step_composed_us": lambda: leg._glm_step_composed(op, z, prop, state),
                "laplace_us": whole,
                "laplace_composed_us": composed(whole),
                "gaussian_us": lambda: leg.insample_posterior_batch(m, ts, xs, observed=observed),
            }
            t = timed_alternating(fns, a.reps)
            r = whole()
            k = min(a.loop_series, B)
            loop = lambda: [leg.laplace_posterior(m, ts[b], ys[b], "poisson", observed=observed[b], offset=offset) for b in range(k)]      # noqa: E731
            tl = timed_alternating({"loop": loop}, 1, warmup=1)["loop"][0] * B / k
            row = {"obs": obs, "B": B, "rows": xs.shape[1], "iterations": int(r.iterations.max()), "converged": bool(r.converged.all()),
                   "loop_us": round(tl, 1), "loop_series_timed": k}
            row.update({k_: round(v[0], 1) for k_, v in t.items()})
            results.append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()

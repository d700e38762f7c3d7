"""Time the leave-one-out predictives (leg.loo_predictive*, cgps_leg_loo: DESIGN.md 4.20) -- device events, median of
--reps calls after 3 warm-ups, the variants of a comparison alternated inside every repetition.

Workload: fp64, rank 5, series of 502 rows from leg.co2_like_series (standardised as co2_workload does), the model of
tests/golden/leg_co2like.npz for obs_dim 1; for obs_dim 3 that model's B and Lambda stacked and perturbed, the three
channels of a series three series of different seeds.  70 % of the entries observed (another mask per series) and
noise variances uniform in [0, 1].

    python tools/time_loo.py [--obs 1,3] [--batches 1,64,1024] [--models 16x64] [--reps 20] [--json out.json]
        per (obs_dim, B):
          loo_call_us / posterior_call_us   leg.loo_predictive_batch against the leg.insample_posterior_batch underneath
                                            it: the difference is what the predictives cost on top of the posterior;
          entry_us / torch_us               the C entry alone (leg._loo_rows, leave="entry"; row_us: leave="row") against
                                            the same formulas as batched torch passes on the same (mean, Sd);
          entry_gbps                        the entry's achieved bytes per second: R M (d^2 + d) sizeof read plus the
                                            outputs written;
          refit_loop_us (B = 1 only)        what a user did before: n obs_dim calls of leg.insample_posterior(observed=
                                            the mask without one entry).  32 of them are timed and the time is SCALED
                                            to n obs_dim calls.
        per models MxB: the same for leg.loo_predictive_models against leg.insample_posterior_models.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cyclic-gps_amd")]
from cyclic_gps import leg  # noqa: E402

REFIT_TIMED = 32


def model(obs, seed=0, dtype=torch.float64):
    g = np.load(os.path.join(ROOT, "tests", "golden", "leg_co2like.npz"))
    N, R, B, L = (torch.from_numpy(g[k]).to(dtype) for k in ("N", "R", "B", "Lambda"))
    gen = torch.Generator().manual_seed(seed)
    if seed:
        N = N + 0.02 * torch.tril(torch.randn(N.shape, generator=gen, dtype=dtype))
    if obs > 1 or seed:
        B = B.expand(obs, -1) * (1 + 0.3 * torch.randn(obs, B.shape[1], generator=gen, dtype=dtype))
        L = torch.tril(0.1 * torch.randn(obs, obs, generator=gen, dtype=dtype)) + float(L[0, 0]) * torch.eye(obs, dtype=dtype)
    return leg.LEGMatrices(*(t.contiguous().cuda() for t in (N, R, B, L)))


def data(B, obs, rows=502, dtype=torch.float64):
    ts, xs = [], []
    for b in range(B):
        chans = []
        for c in range(obs):
            t, x = leg.co2_like_series(rows=rows, seed=b * obs + c, dtype=dtype)
            chans.append((x[:, 0] - x.mean()) / x.std())
        ts.append(12 * (t - t.min()))
        xs.append(torch.stack(chans, 1))
    ts, xs = torch.stack(ts).cuda(), torch.stack(xs).cuda()
    gen = torch.Generator().manual_seed(B + obs)
    observed = (torch.rand(xs.shape, generator=gen) < 0.7).cuda()
    noise = torch.rand(xs.shape, generator=gen, dtype=dtype).cuda()
    return ts, xs, observed, noise


def timed_alternating(fns, reps, warmup=3):
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


def torch_loo(Bm, LLT, xs, mask, s, mu, Sd):
    """leave="entry" as batched torch passes: Bm [M, obs, d], LLT [M, obs, obs], data [R, ...], mu [M, R, d], Sd [M, R, d, d]."""
    dt = mu.dtype
    zero = torch.zeros((), dtype=dt, device=mu.device)
    Mt = mask.to(dt)
    unobs = torch.diag_embed(1 - Mt)
    W = Mt.unsqueeze(2) * (LLT.unsqueeze(1) + torch.diag_embed(torch.where(mask, s, zero))) * Mt.unsqueeze(1) + unobs
    Li = torch.linalg.inv_ex(W)[0] - unobs
    xz = torch.where(mask, xs, zero)
    Bk = Bm.unsqueeze(1)
    e = Mt * (xz - (Bk @ mu.unsqueeze(-1)).squeeze(-1))
    g = (Li @ e.unsqueeze(-1)).squeeze(-1)
    P = Li - Li @ (Bk @ Sd @ Bk.transpose(-1, -2)) @ Li
    pcc = torch.where(mask, torch.diagonal(P, dim1=-2, dim2=-1), 1 + zero)
    nan = torch.full((), float("nan"), dtype=dt, device=mu.device)
    mean = torch.where(mask, xz - g / pcc, nan)
    var = torch.where(mask, 1 / pcc, nan)
    lp = torch.where(mask, -0.5 * g * g / pcc + 0.5 * torch.log(pcc) - 0.5 * math.log(2 * math.pi), zero)
    return mean, var, lp


def entry_rows(ms, xs, observed, noise, mean, Sd, offsets, reps):
    """The C entry alone on a given posterior against the torch passes; agreement first."""
    M, (obs, d) = len(ms), ms[0].B.shape
    R, dt = xs.shape[0], xs.dtype
    Bm = torch.stack([m.B for m in ms]).contiguous()
    LLT = torch.stack([m.LLT for m in ms]).contiguous()
    xs_c, pattern, nv = leg._loo_data(xs, observed, noise, dt)
    mean, Sd = mean.reshape(M * R, d).contiguous(), Sd.reshape(M * R, d, d).contiguous()
    out = leg._loo_rows(xs_c, pattern, nv, offsets, Bm, LLT, mean, Sd, 0)
    ref = torch_loo(Bm, LLT, xs_c, observed, nv, mean.view(M, R, d), Sd.view(M, R, d, d))
    err = max(float((torch.nan_to_num(a) - torch.nan_to_num(b)).abs().max()) for a, b in zip(out[:3], ref))
    assert err < 1e-8 and int(out[4].item()) == 0, err
    t = timed_alternating({
        "entry": lambda: leg._loo_rows(xs_c, pattern, nv, offsets, Bm, LLT, mean, Sd, 0),
        "row": lambda: leg._loo_rows(xs_c, pattern, nv, offsets, Bm, LLT, mean, Sd, 1),
        "torch": lambda: torch_loo(Bm, LLT, xs_c, observed, nv, mean.view(M, R, d), Sd.view(M, R, d, d))}, reps)
    sz = xs.element_size()
    nbytes = R * M * (d * d + d) * sz + 3 * M * R * obs * sz
    return {"entry_us": t["entry"][0], "entry_min_us": t["entry"][1], "row_us": t["row"][0], "torch_us": t["torch"][0],
            "entry_bytes": nbytes, "entry_gbps": nbytes / t["entry"][0] * 1e-3, "entry_vs_torch_max_abs_err": err}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", default="1,3")
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--models", default="16x64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = []
    for obs in [int(x) for x in a.obs.split(",")]:
        m = model(obs)
        for B in [int(x) for x in a.batches.split(",")]:
            ts, xs, observed, noise = data(B, obs)
            n = ts.shape[1]
            kw = dict(observed=observed, noise_var=noise)
            row = {"obs": obs, "B": B, "rows": n, "d": 5, "dtype": "float64", "models": 1}
            t = timed_alternating({"loo": lambda: leg.loo_predictive_batch(m, ts, xs, **kw),
                                   "posterior": lambda: leg.insample_posterior_batch(m, ts, xs, **kw)}, a.reps)
            row["loo_call_us"], row["posterior_call_us"] = t["loo"][0], t["posterior"][0]
            mean, (Sd, _) = leg.insample_posterior_batch(m, ts, xs, **kw)
            plan = leg._cached_batch_plan([n] * B, ts.device)
            f = lambda t_: t_.reshape((B * n,) + tuple(t_.shape[2:]))      # noqa: E731
            row.update(entry_rows([m], f(xs), f(observed), f(noise), mean, Sd, plan.offsets, a.reps))
            if B == 1:
                entries = observed[0].nonzero()[:REFIT_TIMED]

                def refit():
                    with torch.no_grad():
                        for i, c in entries.tolist():
                            left = observed[0].clone()
                            left[i, c] = False
                            leg.insample_posterior(m, ts[0], xs[0], observed=left, noise_var=noise[0])

                t = timed_alternating({"refit": refit}, max(3, a.reps // 4), 1)
                row["refit_timed_calls"] = int(entries.shape[0])
                row["refit_loop_us"] = t["refit"][0] * n * obs / entries.shape[0]     # scaled to n obs calls
                row["refit_loop_over_loo_call"] = row["refit_loop_us"] / row["loo_call_us"]
            print(json.dumps(row), flush=True)
            res.append(row)
        for spec in [s for s in a.models.split(",") if s]:
            M, B = (int(x) for x in spec.split("x"))
            ms = [model(obs, seed=k) for k in range(M)]
            ts, xs, observed, noise = data(B, obs)
            n = ts.shape[1]
            kw = dict(observed=observed, noise_var=noise)
            row = {"obs": obs, "B": B, "rows": n, "d": 5, "dtype": "float64", "models": M}
            t = timed_alternating({"loo": lambda: leg.loo_predictive_models(ms, ts, xs, **kw),
                                   "posterior": lambda: leg.insample_posterior_models(ms, ts, xs, **kw)}, a.reps)
            row["loo_call_us"], row["posterior_call_us"] = t["loo"][0], t["posterior"][0]
            mean, (Sd, _) = leg.insample_posterior_models(ms, ts, xs, **kw)
            plan = leg._cached_batch_plan([n] * B, ts.device)
            f = lambda t_: t_.reshape((B * n,) + tuple(t_.shape[2:]))      # noqa: E731
            row.update(entry_rows(ms, f(xs), f(observed), f(noise), mean, Sd, plan.offsets, a.reps))
            print(json.dumps(row), flush=True)
            res.append(row)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

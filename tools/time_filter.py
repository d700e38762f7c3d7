"""Time the one-step-ahead predictives and filtered states (leg.filter_predictive*, cgps_leg_filter: DESIGN.md 4.22) --
device events, median of --reps calls after 3 warm-ups, the variants of a comparison alternated inside every repetition.

Workload: that of tools/time_loo.py -- fp64, rank 5, series of 502 rows from leg.co2_like_series, the model of
tests/golden/leg_co2like.npz (obs_dim 3: its B and Lambda stacked and perturbed), 70 % of the entries observed and noise
variances uniform in [0, 1].

    python tools/time_filter.py [--obs 1,3] [--batches 64,1024] [--models 16x64] [--reps 20] [--json out.json]
        per (obs_dim, B) and per models MxB:
          filter_call_us     leg.filter_predictive_batch (leg.filter_predictive_models): the whole call;
          filter_entry_us    the C entry alone (leg._filter_rows): the kernel's own time, plus one 4-byte memset;
          torch_loop_us      (a) the same recursion as torch passes vectorised over the series (and models), one step per
                             row, the matrix exponentials of ALL gaps taken in one batched call before the loop: what a
                             user has without the kernel.  Agreement with the kernel is asserted first;
          loglik_us          (b) leg.log_likelihood_batch (leg.log_likelihood_models_observed) on the same data;
          posterior_us       (c) leg.insample_posterior_batch (leg.insample_posterior_models) on the same data;
          *_over_filter      each of the three divided by filter_call_us.
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cyclic-gps_amd"), os.path.join(ROOT, "tools")]
from cyclic_gps import leg  # noqa: E402
from time_loo import data, model, timed_alternating  # noqa: E402


def torch_filter(G, Bm, LLT, ts, xs, mask, s):
    """The recursion of DESIGN 4.22 as torch passes: G [M, d, d], Bm [M, obs, d], LLT [M, obs, obs]; ts [B, n], xs, mask
    and s [B, n, obs].  Returns (mean [M, B, n, obs], cov, logpdf [M, B, n], z_mean, z_cov, loglik [M, B])."""
    dt, dev = G.dtype, G.device
    M, d = G.shape[:2]
    B, n, obs = xs.shape
    zero = torch.zeros((), dtype=dt, device=dev)
    eye = torch.eye(d, dtype=dt, device=dev)
    E_all = torch.matrix_exp(-0.5 * (ts[:, 1:] - ts[:, :-1])[None, :, :, None, None] * G[:, None, None])   # [M, B, n-1, d, d]
    Bk, Ck = Bm[:, None], LLT[:, None]
    m, Dm = torch.zeros(M, B, d, dtype=dt, device=dev), torch.zeros(M, B, d, d, dtype=dt, device=dev)
    outs = [[] for _ in range(5)]
    for i in range(n):
        if i:
            E = E_all[:, :, i - 1]
            m, Dm = (E @ m.unsqueeze(-1)).squeeze(-1), E @ Dm @ E.transpose(-1, -2)
        mk = mask[:, i]
        Mt = mk.to(dt)
        pm = (Bk @ m.unsqueeze(-1)).squeeze(-1)
        BP = Bk @ (eye + Dm)
        pc = BP @ Bk.transpose(-1, -2) + Ck + torch.diag_embed(torch.where(mk, s[:, i], zero))
        W = Mt.unsqueeze(-1) * pc * Mt.unsqueeze(-2) + torch.diag_embed(1 - Mt)
        Si = torch.linalg.inv_ex(W)[0]                    # (inv_ex and logdet: the batched calls leg.py itself makes)
        e = (Mt * (torch.where(mk, xs[:, i], zero) - pm)).unsqueeze(-1)
        Se = Si @ e
        BPo = Mt.unsqueeze(-1) * BP
        lp = -0.5 * (e * Se).sum((-1, -2)) - 0.5 * torch.logdet(W) - 0.5 * math.log(2 * math.pi) * Mt.sum(-1)
        m = m + (BPo.transpose(-1, -2) @ Se).squeeze(-1)
        Dm = Dm - BPo.transpose(-1, -2) @ Si @ BPo
        for o, t in zip(outs, (pm, pc, lp, m, eye + Dm)):
            o.append(t)
    outs = [torch.stack(o, 2) for o in outs]
    return outs + [outs[2].to(torch.float64).sum(-1)]


def measure(ms, ts, xs, observed, noise, reps):
    M, (obs, d) = len(ms), ms[0].B.shape
    B, n = ts.shape
    dt = xs.dtype
    kw = dict(observed=observed, noise_var=noise)
    G = torch.stack([m.G for m in ms]).contiguous()
    Bm = torch.stack([m.B for m in ms]).contiguous()
    LLT = torch.stack([m.LLT for m in ms]).contiguous()
    f = lambda t_: t_.reshape((B * n,) + tuple(t_.shape[2:]))      # noqa: E731
    plan = leg._cached_batch_plan([n] * B, ts.device)
    xs_c, pattern, nv = leg._loo_data(f(xs), f(observed), f(noise), dt)
    ts_c = f(ts).contiguous()
    entry = lambda: leg._filter_rows(ts_c, xs_c, pattern, nv, plan.offsets, G, Bm, LLT, None)      # noqa: E731
    if M == 1:
        fns = {"filter_call": lambda: leg.filter_predictive_batch(ms[0], ts, xs, **kw),
               "loglik": lambda: leg.log_likelihood_batch(ms[0], ts, xs, **kw),
               "posterior": lambda: leg.insample_posterior_batch(ms[0], ts, xs, **kw)}
    else:
        fns = {"filter_call": lambda: leg.filter_predictive_models(ms, ts, xs, **kw),
               "loglik": lambda: leg.log_likelihood_models_observed(ms, ts, xs, **kw),
               "posterior": lambda: leg.insample_posterior_models(ms, ts, xs, **kw)}
    fns["filter_entry"] = entry
    fns["torch_loop"] = lambda: torch_filter(G, Bm, LLT, ts, xs, observed, noise)
    with torch.no_grad():
        out, ref = entry(), torch_filter(G, Bm, LLT, ts, xs, observed, noise)
        assert int(out[8].item()) == 0
        err = max(float((a.reshape(b.shape) - b).abs().max()) for a, b in zip(out[:6], ref))
        assert err < 1e-8, err
        t = timed_alternating(fns, reps)
    row = {"obs": obs, "B": B, "rows": n, "d": d, "dtype": "float64", "models": M, "filter_vs_torch_max_abs_err": err}
    for k, v in t.items():
        row[k + "_us"], row[k + "_min_us"] = v
    for k in ("torch_loop", "loglik", "posterior"):
        row[k + "_over_filter"] = row[k + "_us"] / row["filter_call_us"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", default="1,3")
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--models", default="16x64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = []
    for obs in [int(x) for x in a.obs.split(",")]:
        specs = [(1, int(x)) for x in a.batches.split(",") if x]
        specs += [tuple(int(x) for x in s.split("x")) for s in a.models.split(",") if s]
        for M, B in specs:
            ms = [model(obs, seed=k) for k in range(M)]
            row = measure(ms, *data(B, obs), a.reps)
            print(json.dumps(row), flush=True)
            res.append(row)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

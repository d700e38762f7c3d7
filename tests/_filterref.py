"""The forward (filtering) recursion of a LEG series in torch, for any dtype: what cgps_leg_filter
evaluates, as one torch pass per row.  tests/test_filterref.py holds it in fp64 to the dense truths of ``_noiseref``;
tests/test_leg_filter.py runs it in fp32 for the error an fp32 evaluation of the recursion has.

The prior of the first row is N(0, I); across a gap, E = exp(-1/2 gap G), m^- = E m, P^- = I + E (P - I) E^T; row i
observes the channels o of its mask with noise Cn = Lambda Lambda^T + 1e-9 I + diag(s_i):
    predictive of all channels: N(B m^-, B P^- B^T + Lambda Lambda^T + 1e-9 I + diag(s_i on o))
    e = x_o - B_o m^-,  S = (B P^- B^T + Cn)[o, o] = T T^T,  logpdf = -1/2 |T^-1 e|^2 - sum log T_cc - k/2 log 2 pi
    K = P^- B_o^T S^-1,  m = m^- + K e,  P = P^- - (T^-1 B_o P^-)^T (T^-1 B_o P^-)
Entries of xs and s outside the mask are never touched (they may hold NaN)."""
import math

import torch

F64 = torch.float64


def filter_ref(mats, ts, xs, s=None, mask=None, init=None, dtype=F64):
    """mats = (N, R, B, Lambda); ts [n], xs [n, obs]; s [n, obs] noise variances or None (zero); mask bool [n, obs] or
    None (everything observed); init = (t, mean [d], cov [d, d]) or None (the prior at the first row).  Everything is
    cast to ``dtype`` and evaluated in it on the CPU.  Returns a dict: mean [n, obs], cov [n, obs, obs], logpdf [n],
    z_mean [n, d], z_cov [n, d, d], pre_mean [n, d] (m^-), loglik (0-d fp64, the row terms added in row order) and
    state = (t, mean, cov) after the last row."""
    Nm, Rm, Bm, Lm = (t.detach().to("cpu", dtype) for t in mats)
    ts, xs = ts.detach().to("cpu", dtype), xs.detach().to("cpu", dtype)
    n, obs = xs.shape
    d = Nm.shape[0]
    mask = torch.ones(n, obs, dtype=torch.bool) if mask is None else mask.cpu()
    s = torch.zeros(n, obs, dtype=dtype) if s is None else s.detach().to("cpu", dtype)
    eye = torch.eye(d, dtype=dtype)
    G = Nm @ Nm.T + Rm - Rm.T + 1e-5 * eye
    LLT = Lm @ Lm.T + 1e-9 * torch.eye(obs, dtype=dtype)
    if init is None:
        t_prev, m, Dm = None, torch.zeros(d, dtype=dtype), torch.zeros(d, d, dtype=dtype)
    else:
        t_prev, m, Dm = init[0].detach().to("cpu", dtype), init[1].detach().to("cpu", dtype), init[2].detach().to("cpu", dtype) - eye
    out = {"mean": torch.zeros(n, obs, dtype=dtype), "cov": torch.zeros(n, obs, obs, dtype=dtype),
           "logpdf": torch.zeros(n, dtype=dtype), "z_mean": torch.zeros(n, d, dtype=dtype),
           "z_cov": torch.zeros(n, d, d, dtype=dtype), "pre_mean": torch.zeros(n, d, dtype=dtype)}
    ll = 0.0
    for i in range(n):
        if t_prev is not None:
            E = torch.matrix_exp(-0.5 * (ts[i] - t_prev) * G)
            m, Dm = E @ m, E @ Dm @ E.T
        t_prev = ts[i]
        P = eye + Dm
        o = mask[i].nonzero().flatten()
        so = torch.zeros(obs, dtype=dtype)
        so[o] = s[i, o]
        out["pre_mean"][i] = m
        out["mean"][i] = Bm @ m
        out["cov"][i] = Bm @ P @ Bm.T + LLT + torch.diag(so)
        if o.numel():
            Bo = Bm[o]
            T = torch.linalg.cholesky(out["cov"][i][o][:, o])
            e = torch.linalg.solve_triangular(T, (xs[i, o] - Bo @ m)[:, None], upper=False)[:, 0]
            V = torch.linalg.solve_triangular(T, Bo @ P, upper=False)
            out["logpdf"][i] = -0.5 * (e * e).sum() - torch.log(torch.diagonal(T)).sum() - 0.5 * o.numel() * math.log(2 * math.pi)
            m = m + V.T @ e
            Dm = Dm - V.T @ V
            Dm = 0.5 * (Dm + Dm.T)
        ll += float(out["logpdf"][i])
        out["z_mean"][i], out["z_cov"][i] = m, eye + Dm
    out["loglik"] = torch.tensor(ll, dtype=F64)
    out["state"] = (t_prev, m, eye + Dm)
    return out

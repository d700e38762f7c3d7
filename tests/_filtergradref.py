"""References for the gradients through the LEG filter, in torch on the CPU, for any dtype.

(a) ``filter_diff`` / ``filter_diff_operands``: the recursion of tests/_filterref.py written so that autograd passes
    through it -- no input is detached, G carries its + 1e-5 I and LLT its + 1e-9 I.  Every covariance that the recursion
    carries is symmetrised where it is formed, so the gradient in a symmetric input (init.cov) is symmetric and the
    cotangents of ``cov`` and ``z_cov`` act through their symmetric parts, as the kernel's do.  Entries of xs and s
    outside the mask are never touched (they may hold NaN) and get exactly zero gradient.
(b) ``filter_adjoint_ref``: the reverse walk of cgps_leg_filter_adjoint as explicit torch ops from the saved filtered
    states, row by row from the last to the first; only the Frechet step of a gap goes through autograd of
    ``torch.matrix_exp`` on that one gap.
tests/test_filtergradref.py holds (a) to the dense density of tests/_gradref.py and (b) to autograd of (a)."""
import math

import torch

F64 = torch.float64
KEYS = ("mean", "cov", "logpdf", "z_mean", "z_cov")


def sym(X):
    return 0.5 * (X + X.transpose(-1, -2))


def operands(mats, dtype=F64):
    """(G, B, LLT) of the four model matrices, differentiable."""
    Nm, Rm, Bm, Lm = (t.to(dtype) for t in mats)
    d, obs = Nm.shape[0], Bm.shape[0]
    G = Nm @ Nm.T + Rm - Rm.T + 1e-5 * torch.eye(d, dtype=dtype)
    LLT = Lm @ Lm.T + 1e-9 * torch.eye(obs, dtype=dtype)
    return G, Bm, LLT


def filter_diff_operands(G, Bm, LLT, ts, xs, s=None, mask=None, init=None):
    """The recursion from (G, B, LLT); everything in the dtype of G.  ts [n], xs [n, obs], s [n, obs] or None, mask bool
    [n, obs] or None, init = (t, mean [d], cov [d, d]) or None.  Returns a dict: mean, cov, logpdf, z_mean, z_cov (stacked
    over the rows), loglik (0-d, the sum of logpdf) and state = (t, mean, cov)."""
    dtype = G.dtype
    n, obs = xs.shape
    d = G.shape[0]
    mask = torch.ones(n, obs, dtype=torch.bool) if mask is None else mask.cpu()
    eye = torch.eye(d, dtype=dtype)
    if init is None:
        t_prev, m, Dm = None, torch.zeros(d, dtype=dtype), torch.zeros(d, d, dtype=dtype)
    else:
        t_prev, m, Dm = init[0].to(dtype), init[1].to(dtype), sym(init[2].to(dtype) - eye)
    rows = {k: [] for k in KEYS}
    for i in range(n):
        if t_prev is not None:
            E = torch.matrix_exp(-0.5 * (ts[i] - t_prev) * G)
            m, Dm = E @ m, sym(E @ Dm @ E.T)
        t_prev = ts[i]
        P = eye + Dm
        o = mask[i].nonzero().flatten()
        cov = sym(Bm @ P @ Bm.T) + sym(LLT)
        if s is not None and o.numel():
            so = torch.zeros(obs, dtype=dtype).index_put((o,), s[i, o])
            cov = cov + torch.diag(so)
        rows["mean"].append(Bm @ m)
        rows["cov"].append(cov)
        if o.numel():
            Bo = Bm[o]
            T = torch.linalg.cholesky(cov[o][:, o])
            e = torch.linalg.solve_triangular(T, (xs[i, o] - Bo @ m)[:, None], upper=False)[:, 0]
            V = torch.linalg.solve_triangular(T, Bo @ P, upper=False)
            rows["logpdf"].append(-0.5 * (e * e).sum() - torch.log(torch.diagonal(T)).sum() - 0.5 * o.numel() * math.log(2 * math.pi))
            m = m + V.T @ e
            Dm = sym(Dm - V.T @ V)
        else:
            rows["logpdf"].append(torch.zeros((), dtype=dtype))
        rows["z_mean"].append(m)
        rows["z_cov"].append(eye + Dm)
    shapes = {"mean": (0, obs), "cov": (0, obs, obs), "logpdf": (0,), "z_mean": (0, d), "z_cov": (0, d, d)}
    out = {k: (torch.stack(v) if v else torch.zeros(shapes[k], dtype=dtype)) for k, v in rows.items()}
    out["loglik"] = out["logpdf"].sum()
    out["state"] = (t_prev, m, eye + Dm)
    return out


def filter_diff(mats, ts, xs, s=None, mask=None, init=None, dtype=F64):
    """(a) from the four model matrices (N, R, B, Lambda): inputs are cast to ``dtype``, never detached."""
    G, Bm, LLT = operands(mats, dtype)
    c = lambda t: None if t is None else t.to(dtype)      # noqa: E731
    init = None if init is None else tuple(c(t) for t in init)
    return filter_diff_operands(G, Bm, LLT, c(ts), c(xs), c(s), mask, init)


def _frechet_adjoint(G, gap, Ebar):
    """(G_bar, gap_bar) of E = exp(-1/2 gap G) under the cotangent Ebar, by autograd on this one gap."""
    Gl = G.detach().clone().requires_grad_(True)
    gl = gap.detach().clone().requires_grad_(True)
    E = torch.matrix_exp(-0.5 * gl * Gl)
    gG, gg = torch.autograd.grad(E, (Gl, gl), Ebar)
    return gG, gg


def filter_adjoint_ref(G, Bm, LLT, ts, xs, s, mask, init, z_mean, z_cov, cot):
    """(b): the reverse walk.  Operands and data as ``filter_diff_operands`` (detached here), z_mean [n, d] and z_cov
    [n, d, d] the saved filtered states, ``cot`` a dict of cotangents with any of the keys mean, cov, logpdf, z_mean, z_cov
    (per row), loglik (0-d), state_mean [d], state_cov [d, d].  Returns a dict: G, B, LLT, xs [n, obs], s [n, obs], gap
    [n] (the gradient in the gap BEFORE every row; entry 0 is the gap from init.t, 0 without init), m0 [d], P0 [d, d]."""
    with torch.no_grad():
        G, Bm, LLT, ts, xs, z_mean, z_cov = (t.detach() for t in (G, Bm, LLT, ts, xs, z_mean, z_cov))
        dtype = G.dtype
        n, obs = xs.shape
        d = G.shape[0]
        mask = torch.ones(n, obs, dtype=torch.bool) if mask is None else mask.cpu()
        eye = torch.eye(d, dtype=dtype)
        g = {k: (cot[k].detach().to(dtype).clone() if cot.get(k) is not None else None) for k in KEYS}
        if cot.get("loglik") is not None:
            g["logpdf"] = (g["logpdf"] if g["logpdf"] is not None else torch.zeros(n, dtype=dtype)) + cot["loglik"].detach().to(dtype)
        mb = torch.zeros(d, dtype=dtype) if cot.get("state_mean") is None else cot["state_mean"].detach().to(dtype).clone()
        Db = torch.zeros(d, d, dtype=dtype) if cot.get("state_cov") is None else sym(cot["state_cov"].detach().to(dtype))
        out = {"G": torch.zeros(d, d, dtype=dtype), "B": torch.zeros(obs, d, dtype=dtype), "LLT": torch.zeros(obs, obs, dtype=dtype),
               "xs": torch.zeros(n, obs, dtype=dtype), "s": torch.zeros(n, obs, dtype=dtype), "gap": torch.zeros(n, dtype=dtype)}
        for i in range(n - 1, -1, -1):
            if g["z_mean"] is not None:
                mb = mb + g["z_mean"][i]
            if g["z_cov"] is not None:
                Db = Db + sym(g["z_cov"][i])
            lb = g["logpdf"][i] if g["logpdf"] is not None else torch.zeros((), dtype=dtype)
            if i > 0:
                mp, Dp, gap = z_mean[i - 1], z_cov[i - 1] - eye, ts[i] - ts[i - 1]
            elif init is not None:
                mp, Dp, gap = init[1].detach().to(dtype), sym(init[2].detach().to(dtype)) - eye, ts[0] - init[0].detach().to(dtype)
            else:
                mp, Dp, gap = torch.zeros(d, dtype=dtype), torch.zeros(d, d, dtype=dtype), torch.zeros((), dtype=dtype)
            E = torch.matrix_exp(-0.5 * gap * G)
            m, ED = E @ mp, E @ Dp
            P = eye + sym(ED @ E.T)
            on = mask[i].to(dtype)
            o = mask[i].nonzero().flatten()
            al, Kt, Wi = torch.zeros(obs, dtype=dtype), torch.zeros(obs, d, dtype=dtype), torch.zeros(obs, obs, dtype=dtype)
            if o.numel():
                A = Bm[o]
                S = A @ P @ A.T + LLT[o][:, o]
                if s is not None:
                    S = S + torch.diag(s[i, o].detach().to(dtype))
                W = torch.linalg.inv(sym(S))
                al[o] = W @ (xs[i, o] - A @ m)
                Kt[o] = W @ A @ P
                Wi[o[:, None], o[None, :]] = W
            h = Kt @ mb
            DK = Db @ Kt.T
            eb = h - lb * al
            Sf = (Kt @ DK - sym(torch.outer(h, al)) + 0.5 * lb * (torch.outer(al, al) - Wi)) * torch.outer(on, on)
            if g["cov"] is not None:
                Sf = Sf + sym(g["cov"][i])
            ef = eb - (g["mean"][i] if g["mean"] is not None else 0.0)
            out["xs"][i] = eb * on
            out["s"][i] = torch.diagonal(Sf) * on
            out["LLT"] += Sf
            out["B"] += -torch.outer(ef, m) + torch.outer(al, P @ mb) + 2 * Sf @ Bm @ P - 2 * DK.T @ P
            Db = Db + sym(torch.outer(mb, Bm.T @ al)) - 2 * sym(DK @ Bm) + Bm.T @ Sf @ Bm
            mb = mb - Bm.T @ ef
            Ebar = torch.outer(mb, mp) + 2 * Db @ ED
            with torch.enable_grad():
                gG, gg = _frechet_adjoint(G, gap, Ebar)
            out["G"] += gG
            out["gap"][i] = gg
            mb, Db = E.T @ mb, sym(E.T @ Db @ E)
        out["m0"], out["P0"] = mb, Db
        return out


def gap_to_times(gap_bar, with_init):
    """(the gradient in ts [n], the gradient in init.t or None) from the gradient in the gaps before the rows"""
    n = gap_bar.shape[0]
    gt = torch.zeros_like(gap_bar)
    if n > 1:
        gt[1:] += gap_bar[1:]
        gt[:-1] -= gap_bar[1:]
    if with_init and n:
        gt[0] += gap_bar[0]
        return gt, -gap_bar[0]
    return gt, None


def matrix_grads(mats, G_bar, B_bar, LLT_bar):
    """(N_bar, R_bar, B_bar, Lambda_bar) from the adjoints of G = N N^T + R - R^T + 1e-5 I and LLT = Lambda Lambda^T + 1e-9 I"""
    Nm, _, _, Lm = (t.detach().to(G_bar.dtype) for t in mats)
    return (G_bar + G_bar.T) @ Nm, G_bar - G_bar.T, B_bar, (LLT_bar + LLT_bar.T) @ Lm

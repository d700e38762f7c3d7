"""fp64 CPU truth of the leave-one-out predictives of a LEG series (tests/test_leg_loo.py), independent of the HIP
kernels, of the posterior and of the precision identity the library evaluates: the observed entries of the series are
ONE dense Gaussian N(0, C) (``_noiseref._dense_parts``), and the predictive of an entry (or of a row's entries) is what
deleting it from C and conditioning on everything that is left gives.

Also the two numbers the tests' tolerances are made of.  kappa: an evaluation from the posterior (mu_i, S_ii) forms
the LOO precision as a difference of two numbers of the size of the noise precision Li, so it loses
kappa = Li[c, c] var_loo(i, c) >= 1 per entry; for a whole row the same loss is the largest eigenvalue of
Li[o, o] cov_loo(i) (the two coincide for one observed channel).  cond(W_i): the condition number of the row's noise
block W = M Cn M + (I - M), which every product with Li carries."""
import math

import torch

import _noiseref as nr

F64 = torch.float64


def _noise_blocks(Lm, s, mask):
    """Per row: Li = M W^-1 M [n, obs, obs] and cond(W) [n], W = M (LLT + diag(s)) M + (I - M)."""
    obs = mask.shape[1]
    LLT = Lm @ Lm.T + 1e-9 * torch.eye(obs, dtype=F64)
    Mt = mask.to(F64)
    W = Mt.unsqueeze(2) * (LLT + torch.diag_embed(torch.where(mask, s, torch.zeros_like(s)))) * Mt.unsqueeze(1) \
        + torch.diag_embed(1 - Mt)
    Li = torch.linalg.inv(W) - torch.diag_embed(1 - Mt)
    return Li, torch.linalg.cond(W)


def _condition(C, x, out, rest):
    """N(mean, cov) of x[out] given x[rest] under N(0, C), and the log density of x[out] under it."""
    Coo = C[out][:, out]
    if rest.numel():
        Cor = C[out][:, rest]
        sol = torch.linalg.solve(C[rest][:, rest], torch.cat([x[rest, None], Cor.T], 1))
        mean, cov = Cor @ sol[:, 0], Coo - Cor @ sol[:, 1:]
    else:
        mean, cov = torch.zeros(out.numel(), dtype=F64), Coo
    cov = 0.5 * (cov + cov.T)
    r = x[out] - mean
    lp = -0.5 * (r @ torch.linalg.solve(cov, r)) - 0.5 * torch.logdet(cov) - 0.5 * out.numel() * math.log(2 * math.pi)
    return mean, cov, lp


def loo_truth(mats, ts, xs, s=None, mask=None, leave="entry"):
    """The leave-one-out predictives of one series by deletion.  mats = (N, R, B, Lambda) fp64; ts [n], xs [n, obs];
    s [n, obs] noise variances or None (zero); mask bool [n, obs] or None (everything observed).  Entries of xs and s
    outside the mask are never touched.  Returns a dict of fp64 tensors:
      leave="entry": mean, var, logpdf, kappa [n, obs] (NaN, NaN, 0, 0 where nothing is observed);
      leave="row":   mean [n, obs], var [n, obs, obs] (NaN in the rows and columns of unobserved channels), logpdf [n]
                     (0 for a row that observes nothing), kappa [n] (0 there);
      both: cond_w [n], score (0-d, the sum of the log densities)."""
    Nm, Rm, Bm, Lm = (t.detach().to("cpu", F64) for t in mats)
    ts, xs = ts.detach().to("cpu", F64), xs.detach().to("cpu", F64)
    n, obs = xs.shape
    mask = torch.ones(n, obs, dtype=torch.bool) if mask is None else mask.cpu()
    s = torch.zeros(n, obs, dtype=F64) if s is None else s.detach().to("cpu", F64)
    _, _, C, x = nr._dense_parts(Nm, Rm, Bm, Lm, ts, xs, s, mask)
    Li, cond_w = _noise_blocks(Lm, s, mask)
    m = x.numel()
    pos = torch.full((n * obs,), -1, dtype=torch.long)           # entry (i, c) -> its index among the observed ones
    pos[mask.reshape(-1)] = torch.arange(m)
    pos = pos.reshape(n, obs)
    every = torch.arange(m)
    nan = float("nan")
    mean = torch.full((n, obs), nan, dtype=F64)
    if leave == "entry":
        var, lp, kappa = torch.full((n, obs), nan, dtype=F64), torch.zeros(n, obs, dtype=F64), torch.zeros(n, obs, dtype=F64)
        for i in range(n):
            for c in range(obs):
                j = int(pos[i, c])
                if j < 0:
                    continue
                mu, cov, l = _condition(C, x, every[j:j + 1], torch.cat([every[:j], every[j + 1:]]))
                mean[i, c], var[i, c], lp[i, c] = mu[0], cov[0, 0], l
                kappa[i, c] = Li[i, c, c] * cov[0, 0]
    elif leave == "row":
        var, lp, kappa = torch.full((n, obs, obs), nan, dtype=F64), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
        for i in range(n):
            o = mask[i].nonzero().flatten()
            if o.numel() == 0:
                continue
            out = pos[i, o]
            keep = torch.ones(m, dtype=torch.bool)
            keep[out] = False
            mu, cov, l = _condition(C, x, out, every[keep])
            mean[i, o], lp[i] = mu, l
            var[i, o.unsqueeze(1), o.unsqueeze(0)] = cov
            kappa[i] = torch.linalg.eigvals(Li[i][o][:, o] @ cov).real.max()
    else:
        raise ValueError(leave)
    return {"mean": mean, "var": var, "logpdf": lp, "kappa": kappa, "cond_w": cond_w, "score": lp.sum()}

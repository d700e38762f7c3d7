"""fp64 CPU references for LEG series with per-observation noise variances (tests/test_leg_noise*.py), independent of
the HIP kernels and of ``leg.observation_weights``: ``_missref.py`` with diag(s) added to the noise of the observed
entries, the observed entries alone as ONE dense Gaussian.

Latent z ~ N(0, Sigma), Sigma the stationary covariance (_gapref.prior_covariance) of G = N N^T + R - R^T + 1e-5 I;
x_t = B z_t + e_t + f_t, e_t ~ N(0, Lambda Lambda^T + 1e-9 I), f_t ~ N(0, diag(s_t)); only the entries (t, c) with
mask[t, c] are data.  Entries of xs and s outside the mask are never touched (they may hold NaN)."""
import math

import torch

import _gapref
import _missref as mr

F64 = torch.float64


def leg_case(d, obs, n, seed, keep=0.6):
    """``_missref.leg_case`` plus noise variances s [n, obs] drawn from [0, 2]: ([N, R, B, Lambda, xs, ts, s], mask)."""
    case, mask = mr.leg_case(d, obs, n, seed, keep)
    s = 2.0 * torch.rand(n, obs, generator=torch.Generator().manual_seed(seed + 1000), dtype=F64)
    return case + [s], mask


def _dense_parts(Nm, Rm, Bm, Lm, ts, xs, s, mask):
    """(Sigma [n d, n d], H = rows of kron(I, B) of the observed entries, C = H Sigma H^T + noise, the observed x)"""
    d = Nm.shape[0]
    n, obs = xs.shape
    G = Nm @ Nm.T + Rm - Rm.T + 1e-5 * torch.eye(d, dtype=F64)
    Sigma = _gapref.prior_covariance(ts, G)             # the covariance form: no block formula, no 1 / gap
    idx = mask.reshape(-1).nonzero().flatten()
    H = torch.kron(torch.eye(n, dtype=F64), Bm)[idx]
    LLT = Lm @ Lm.T + 1e-9 * torch.eye(obs, dtype=F64)
    noise = torch.kron(torch.eye(n, dtype=F64), LLT)[idx][:, idx] + torch.diag(s.reshape(-1)[idx])
    return Sigma, H, H @ Sigma @ H.T + noise, xs.reshape(-1)[idx]


def leg_dense_loglik(Nm, Rm, Bm, Lm, ts, xs, s, mask):
    """log density of the observed entries (differentiable in the seven tensors; d / d xs and d / d s are zero outside
    the mask)."""
    _, _, C, x = _dense_parts(Nm, Rm, Bm, Lm, ts, xs, s, mask)
    if x.numel() == 0:
        return xs.new_zeros(())
    Lc = torch.linalg.cholesky(C)
    z = torch.linalg.solve_triangular(Lc, x[:, None], upper=False)
    return -0.5 * (z * z).sum() - torch.log(torch.diagonal(Lc)).sum() - 0.5 * x.numel() * math.log(2 * math.pi)


def leg_dense_value_and_grads(Nm, Rm, Bm, Lm, ts, xs, s, mask):
    """(ll, [dN, dR, dB, dLambda, dxs, dts, ds]) of leg_dense_loglik, every argument trainable."""
    args = [t.detach().to("cpu", F64).clone().requires_grad_(True) for t in (Nm, Rm, Bm, Lm, ts, xs, s)]
    ll = leg_dense_loglik(*args, mask.cpu())
    g = torch.autograd.grad(ll, args)
    return ll.detach(), [g[0], g[1], g[2], g[3], g[5], g[4], g[6]]


def leg_dense_posterior(Nm, Rm, Bm, Lm, ts, xs, s, mask):
    """Posterior of the latent at ALL rows given the observed entries: (mean [n, d], covariance [n, d, n, d])."""
    args = [t.detach().to("cpu", F64) for t in (Nm, Rm, Bm, Lm, ts, xs, s)]
    Sigma, H, C, x = _dense_parts(*args, mask.cpu())
    n, d = xs.shape[0], Nm.shape[0]
    Szx = Sigma @ H.T
    mean = Szx @ torch.linalg.solve(C, x)
    cov = Sigma - Szx @ torch.linalg.solve(C, Szx.T)
    return mean.reshape(n, d), cov.reshape(n, d, n, d)

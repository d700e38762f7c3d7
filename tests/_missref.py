"""fp64 CPU references for LEG series with missing observations (tests/test_leg_missing*.py), independent of the HIP
kernels and of ``leg.observation_tables``: the observed entries alone as ONE dense Gaussian, built like
``_gradref.leg_dense_loglik``.

Latent z ~ N(0, Sigma), Sigma the stationary covariance (_gapref.prior_covariance) of G = N N^T + R - R^T + 1e-5 I;
x_t = B z_t + e_t, e_t ~ N(0, Lambda Lambda^T + 1e-9 I); only the entries (t, c) with mask[t, c] are data.  Entries of
xs outside the mask are never touched (they may hold NaN)."""
import math

import torch

import _gapref

F64 = torch.float64


def leg_case(d, obs, n, seed, keep=0.6):
    """[N, R, B, Lambda, xs, ts] (the conditioning of test_gradients._leg_case) and a mask [n, obs] that keeps ~60 % of
    the entries, with the first row, the last row and a run of four rows wholly missing."""
    gen = torch.Generator().manual_seed(seed)
    Nm = torch.tril(0.2 / d ** 0.5 * torch.randn(d, d, generator=gen, dtype=F64), -1) + \
        torch.diag(0.9 + 0.3 * torch.rand(d, generator=gen, dtype=F64))
    Rm = torch.tril(0.3 * torch.randn(d, d, generator=gen, dtype=F64), -1)
    Bm = 0.7 * torch.randn(obs, d, generator=gen, dtype=F64)
    Lm = torch.tril(0.2 * torch.randn(obs, obs, generator=gen, dtype=F64)) + 0.6 * torch.eye(obs, dtype=F64)
    ts = 3.0 + torch.cumsum(0.2 + torch.rand(n, generator=gen, dtype=F64), 0)
    xs = torch.randn(n, obs, generator=gen, dtype=F64)
    mask = torch.rand(n, obs, generator=gen) < keep
    mask[0] = False
    mask[n - 1] = False
    if n > 14:
        mask[10:14] = False
    return [Nm, Rm, Bm, Lm, xs, ts], mask


def _dense_parts(Nm, Rm, Bm, Lm, ts, xs, mask):
    """(Sigma [n d, n d], H = rows of kron(I, B) of the observed entries, C = H Sigma H^T + noise, the observed x)"""
    d = Nm.shape[0]
    n, obs = xs.shape
    G = Nm @ Nm.T + Rm - Rm.T + 1e-5 * torch.eye(d, dtype=F64)
    Sigma = _gapref.prior_covariance(ts, G)             # the covariance form: no block formula, no 1 / gap
    idx = mask.reshape(-1).nonzero().flatten()
    H = torch.kron(torch.eye(n, dtype=F64), Bm)[idx]
    LLT = Lm @ Lm.T + 1e-9 * torch.eye(obs, dtype=F64)
    C = H @ Sigma @ H.T + torch.kron(torch.eye(n, dtype=F64), LLT)[idx][:, idx]
    return Sigma, H, C, xs.reshape(-1)[idx]


def leg_dense_loglik(Nm, Rm, Bm, Lm, ts, xs, mask):
    """log density of the observed entries (differentiable in the six tensors; d / d xs is zero outside the mask)."""
    _, _, C, x = _dense_parts(Nm, Rm, Bm, Lm, ts, xs, mask)
    if x.numel() == 0:
        return xs.new_zeros(())
    Lc = torch.linalg.cholesky(C)
    z = torch.linalg.solve_triangular(Lc, x[:, None], upper=False)
    return -0.5 * (z * z).sum() - torch.log(torch.diagonal(Lc)).sum() - 0.5 * x.numel() * math.log(2 * math.pi)


def leg_dense_value_and_grads(Nm, Rm, Bm, Lm, ts, xs, mask):
    """(ll, [dN, dR, dB, dLambda, dxs, dts]) of leg_dense_loglik, every argument trainable."""
    args = [t.detach().to("cpu", F64).clone().requires_grad_(True) for t in (Nm, Rm, Bm, Lm, ts, xs)]
    ll = leg_dense_loglik(*args, mask.cpu())
    g = torch.autograd.grad(ll, args)
    return ll.detach(), [g[0], g[1], g[2], g[3], g[5], g[4]]


def leg_dense_posterior(Nm, Rm, Bm, Lm, ts, xs, mask):
    """Posterior of the latent at ALL rows given the observed entries: (mean [n, d], covariance [n, d, n, d])."""
    args = [t.detach().to("cpu", F64) for t in (Nm, Rm, Bm, Lm, ts, xs)]
    Sigma, H, C, x = _dense_parts(*args, mask.cpu())
    n, d = xs.shape[0], Nm.shape[0]
    Szx = Sigma @ H.T
    mean = Szx @ torch.linalg.solve(C, x)
    cov = Sigma - Szx @ torch.linalg.solve(C, Szx.T)
    return mean.reshape(n, d), cov.reshape(n, d, n, d)

"""fp64 CPU references for gradients, independent of the HIP kernels (tests/test_gradients.py).

* Dense: J assembled densely from (sym(Rs), Os); m = y^T J^-1 y and log|J| through torch.linalg.cholesky, gradients
  by autograd.  Building J from sym(R) = (R + R^T)/2 makes every dR reference symmetric; compare it with the
  symmetric part of the kernel's dR.
* Oracle closed form (large N): the adjoint formulas of cyclic_reduction.py, evaluated with the CPU oracle's
  solve / inverse_blocks (oracle/cr_oracle.py).
* LEG: the log-likelihood as a dense multivariate-normal log-density of the observations, x ~ N(0, B~ Sigma B~^T +
  Lambda~), with Sigma the stationary covariance of the latent, Cov(z_i, z_j) = exp(-(t_i - t_j) G / 2)
  (_gapref.py): it does not go through the PEG block formula that the kernels evaluate.
"""
import functools
import math

import torch

import _gapref
import _util
from oracle import cr_oracle as O

F64 = torch.float64


def sym(R):
    return 0.5 * (R + R.transpose(-1, -2))


def dense_J(Rs, Os):
    """[N d, N d] matrix with diagonal blocks sym(Rs), lower off-diagonal blocks J[i+1, i] = Os[i]; differentiable."""
    N, d = Rs.shape[0], Rs.shape[1]
    J = Rs.new_zeros(N, d, N, d)
    i = torch.arange(N)
    J[i, :, i, :] = sym(Rs)
    if N > 1:
        J[i[1:], :, i[:-1], :] = Os
        J[i[:-1], :, i[1:], :] = Os.transpose(-1, -2)
    return J.reshape(N * d, N * d)


def _flat(y, N, d):
    return y.reshape(N * d, -1)


def dense_value_and_grads(kind, Rs, Os, y, u=None):
    """(value, dR, dO, dy) of one scalar of the system, in fp64 on the CPU by autograd through a dense Cholesky.
    kind: "mahal" (sum over columns of y_c^T J^-1 y_c), "logdet" (log|J|), "solvedot" (<u, J^-1 y>)."""
    R, Os_, Y = (t.detach().to("cpu", F64).clone().requires_grad_(True) for t in (Rs, Os, y))
    N, d = R.shape[0], R.shape[1]
    L = torch.linalg.cholesky(dense_J(R, Os_))
    if kind == "mahal":
        z = torch.linalg.solve_triangular(L, _flat(Y, N, d), upper=False)
        val = (z * z).sum()
    elif kind == "logdet":
        val = 2 * torch.log(torch.diagonal(L)).sum()
    elif kind == "solvedot":
        x = torch.cholesky_solve(_flat(Y, N, d), L)
        val = (_flat(u.detach().to("cpu", F64), N, d) * x).sum()
    else:
        raise ValueError(kind)
    gR, gO, gy = torch.autograd.grad(val, (R, Os_, Y), allow_unused=True)
    z = lambda g, t: torch.zeros_like(t) if g is None else g   # noqa: E731
    return val.detach(), z(gR, R), z(gO, Os_), z(gy, Y)


@functools.lru_cache(maxsize=None)
def cr_case(N, d, seed=0):
    """Operands of a well-conditioned system (tests/_util.conditioned_system) in fp64 on the CPU: Rs, Os, y [N, d],
    Y[m] [N, d, m] for m in (2, 3, 8) and cotangents U[m] of the same shapes (U[1] is [N, d])."""
    Rs, Os, b, _, _ = _util.conditioned_system(N, d, seed=1000 + 17 * N + d + seed)
    g = torch.Generator().manual_seed(7 * N + d + seed)
    Y = {1: b}
    U = {1: torch.randn(N, d, generator=g, dtype=F64)}
    for m in (2, 3, 8):
        Y[m] = torch.randn(N, d, m, generator=g, dtype=F64)
        U[m] = torch.randn(N, d, m, generator=g, dtype=F64)
    return Rs, Os, Y, U


@functools.lru_cache(maxsize=None)
def cr_dense_ref(N, d, kind, m=1, seed=0):
    """dense_value_and_grads on cr_case(N, d, seed), cached (the fp32 and fp64 tests share it)."""
    Rs, Os, Y, U = cr_case(N, d, seed)
    return dense_value_and_grads(kind, Rs, Os, Y[m], U[m] if kind == "solvedot" else None)


def _pair(a, b):
    """sum_c a[:, :, c] b[:, :, c]^T per block row ([N, d] or [N, d, m] -> [N, d, d])"""
    a2, b2 = a.reshape(a.shape[0], a.shape[1], -1), b.reshape(b.shape[0], b.shape[1], -1)
    return a2 @ b2.transpose(-1, -2)


def _osolve(dec, y):
    """the oracle's solve takes [N, d]; one column at a time for [N, d, m]"""
    if y.dim() == 2:
        return O.solve(dec, y)
    return torch.stack([O.solve(dec, y[:, :, c]) for c in range(y.shape[2])], dim=2)


def oracle_value_and_grads(kind, Rs, Os, y, u=None):
    """(value, dR, dO, dy) from the closed-form adjoints with the oracle's solve / inverse_blocks (fp64, CPU):
      m = y^T J^-1 y, w = J^-1 y:  dm/dy = 2w, dm/dR_i = -w_i w_i^T, dm/dO_i = -2 w_{i+1} w_i^T
      l = log|J|, S = J^-1:         dl/dR_i = S_ii, dl/dO_i = 2 S_{i+1,i}
      s = <u, J^-1 y>, a = J^-1 u:  ds/dy = a, ds/dR_i = -sym(a_i w_i^T), ds/dO_i = -(a_{i+1} w_i^T + w_{i+1} a_i^T)
    dR is returned symmetrised, as the dense reference gives it."""
    Rs, Os, y = (t.detach().to("cpu", F64) for t in (Rs, Os, y))
    Rs = sym(Rs)
    dec = O.decompose(Rs, Os)
    if kind == "logdet":
        Sd, So = O.inverse_blocks(dec)
        return O.det(dec), Sd, 2 * So, torch.zeros_like(y)
    w = _osolve(dec, y)
    if kind == "mahal":
        return (y * w).sum(), -sym(_pair(w, w)), -2 * _pair(w[1:], w[:-1]), 2 * w
    if kind == "solvedot":
        u = u.detach().to("cpu", F64)
        a = _osolve(dec, u)
        return (u * w).sum(), -sym(_pair(a, w)), -(_pair(a[1:], w[:-1]) + _pair(w[1:], a[:-1])), a
    raise ValueError(kind)


# ---- LEG -----------------------------------------------------------------------------------------------------------
def leg_dense_loglik(Nm, Rm, Bm, Lm, ts, xs):
    """log p(xs | ts) of the LEG model as one dense Gaussian density over all n * obs observations (fp64 CPU, torch ops,
    differentiable in all six arguments).  Latent z ~ N(0, Sigma), Sigma = _gapref.prior_covariance(ts, G) with
    G = N N^T + R - R^T + 1e-5 I; x_t = B z_t + e_t, e_t ~ N(0, Lambda Lambda^T + 1e-9 I)."""
    d = Nm.shape[0]
    n, obs = xs.shape
    G = Nm @ Nm.T + Rm - Rm.T + 1e-5 * torch.eye(d, dtype=F64)
    Sigma = _gapref.prior_covariance(ts, G)             # the covariance form: no block formula, no 1 / gap
    Bt = torch.kron(torch.eye(n, dtype=F64), Bm)
    LLT = Lm @ Lm.T + 1e-9 * torch.eye(obs, dtype=F64)
    C = Bt @ Sigma @ Bt.T + torch.kron(torch.eye(n, dtype=F64), LLT)
    Lc = torch.linalg.cholesky(C)
    z = torch.linalg.solve_triangular(Lc, xs.reshape(-1, 1), upper=False)
    return -0.5 * (z * z).sum() - torch.log(torch.diagonal(Lc)).sum() - 0.5 * n * obs * math.log(2 * math.pi)


def leg_dense_value_and_grads(Nm, Rm, Bm, Lm, ts, xs):
    """(ll, [dN, dR, dB, dLambda, dxs, dts]) of leg_dense_loglik, every argument trainable."""
    args = [t.detach().to("cpu", F64).clone().requires_grad_(True) for t in (Nm, Rm, Bm, Lm, ts, xs)]
    ll = leg_dense_loglik(*args)
    g = torch.autograd.grad(ll, args)
    return ll.detach(), [g[0], g[1], g[2], g[3], g[5], g[4]]

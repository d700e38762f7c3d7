"""float64 restatement of the perturb-and-solve draw of one LEG series, written from its definition:

    x[:, :, s] = K^-1 (v + w[:, :, s]),   w_r = (r == 0 ? eps_0 : u_{r-1}) - (r + 1 < n ? E_r^T u_r : 0) + H_r eps'_r
    E_r = exp(-1/2 (t_{r+1} - t_r) G),  I - E_r E_r^T = L_r L_r^T,  u_r = L_r^-T eps_{r+1}
    H_r = B^T M_r T_r^-T,  W_r = M_r (LLT + diag(s_r)) M_r + (I - M_r) = T_r T_r^T,  M_r = diag(observed_r)

eps_r[i] is element (id 2^40 + r d + i, column s) of the generator (tests/_rngref.py) under `stream`, eps'_r[c] element
(id 2^40 + r obs + c, s) under `stream + 1`.  Everything dense, per series, numpy float64 (the matrix exponential is
torch.matrix_exp in float64); I - E E^T is formed as written, which is good to eps / (gap |G|)."""
import numpy as np
import torch

import _rngref


def model(Nm, Rm, Bm, Lm):
    """(G, B, LLT) as float64 numpy arrays from the four model matrices (leg.LEGMatrices)."""
    Nm, Rm, Bm, Lm = (np.asarray(t, dtype=np.float64) for t in (Nm, Rm, Bm, Lm))
    G = Nm @ Nm.T + Rm - Rm.T + 1e-5 * np.eye(Nm.shape[0])
    return G, Bm, Lm @ Lm.T + 1e-9 * np.eye(Lm.shape[0])


def _expm(A):
    return torch.matrix_exp(torch.from_numpy(A)).numpy()


def h_block(Bm, LLT, observed, s):
    """(H [d, obs], Li [obs, obs]) of one row: observed bool [obs], s variances [obs]."""
    M = np.diag(observed.astype(np.float64))
    s = np.where(observed, s, 0.0)
    W = M @ (LLT + np.diag(s)) @ M + (np.eye(len(s)) - M)
    T = np.linalg.cholesky(W)
    return Bm.T @ M @ np.linalg.inv(T).T, np.linalg.inv(W) - (np.eye(len(s)) - M)


def series_terms(G, Bm, LLT, ts, observed=None, s=None, prior=False):
    """The local pieces of one series: E [n-1, d, d], L [n-1, d, d], H [n, d, obs], Li [n, obs, obs]."""
    ts = np.asarray(ts, dtype=np.float64)
    n, d, obs = len(ts), G.shape[0], Bm.shape[0]
    observed = np.ones((n, obs), dtype=bool) if observed is None else np.asarray(observed, dtype=bool).reshape(n, -1)
    observed = np.broadcast_to(observed, (n, obs))
    s = np.zeros((n, obs)) if s is None else np.broadcast_to(np.asarray(s, dtype=np.float64).reshape(n, -1), (n, obs))
    E = np.stack([_expm(-0.5 * (ts[r + 1] - ts[r]) * G) for r in range(n - 1)]) if n > 1 else np.zeros((0, d, d))
    L = np.stack([np.linalg.cholesky(np.eye(d) - e @ e.T) for e in E]) if n > 1 else np.zeros((0, d, d))
    H, Li = np.zeros((n, d, obs)), np.zeros((n, obs, obs))
    if not prior:
        for r in range(n):
            H[r], Li[r] = h_block(Bm, LLT, observed[r], s[r])
    return dict(E=E, L=L, H=H, Li=Li, observed=observed)


def w_from_noise(terms, eps, epsp):
    """w [n, d, S] from eps [n, d, S] and eps' [n, obs, S]."""
    E, L, H = terms["E"], terms["L"], terms["H"]
    n = H.shape[0]
    u = [np.linalg.solve(L[r].T, eps[r + 1]) for r in range(n - 1)]
    w = np.empty_like(eps)
    for r in range(n):
        w[r] = (eps[0] if r == 0 else u[r - 1]) + H[r] @ epsp[r]
        if r + 1 < n:
            w[r] -= E[r].T @ u[r]
    return w


def dense_K(terms):
    """K [n d, n d] from the same pieces: R_0 = I + ..., R_r = Q_{r-1}^-1 + E_r^T Q_r^-1 E_r + B^T Li_r B, O_r = -Q_r^-1 E_r."""
    E, L, H = terms["E"], terms["L"], terms["H"]
    n, d = H.shape[0], H.shape[1]
    K = np.zeros((n * d, n * d))
    Qi = [np.linalg.inv(l @ l.T) for l in L]
    for r in range(n):
        blk = (np.eye(d) if r == 0 else Qi[r - 1]) + H[r] @ H[r].T
        if r + 1 < n:
            blk = blk + E[r].T @ Qi[r] @ E[r]
            off = -Qi[r] @ E[r]
            K[(r + 1) * d:(r + 2) * d, r * d:(r + 1) * d] = off
            K[r * d:(r + 1) * d, (r + 1) * d:(r + 2) * d] = off.T
        K[r * d:(r + 1) * d, r * d:(r + 1) * d] = blk
    return K


def dense_K_truth(G, Bm, ts, Li):
    """The same K another way: the inverse of the stationary covariance Cov(z_i, z_j) = exp(-1/2 (t_i - t_j) G), i >= j,
    plus the rows' B^T Li_r B."""
    ts = np.asarray(ts, dtype=np.float64)
    n, d = len(ts), G.shape[0]
    C = np.zeros((n * d, n * d))
    for i in range(n):
        for j in range(i + 1):
            c = _expm(-0.5 * (ts[i] - ts[j]) * G)
            C[i * d:(i + 1) * d, j * d:(j + 1) * d] = c
            C[j * d:(j + 1) * d, i * d:(i + 1) * d] = c.T
    K = np.linalg.inv(C)
    for r in range(n):
        K[r * d:(r + 1) * d, r * d:(r + 1) * d] += Bm.T @ Li[r] @ Bm
    return K


def rhs_v(terms, Bm, xs):
    """v [n, d] = B^T Li_r x~_r, x~ = xs where observed and 0 elsewhere (whatever xs holds there)."""
    xz = np.where(terms["observed"], np.asarray(xs, dtype=np.float64), 0.0)
    return np.einsum("od,nop,np->nd", Bm, terms["Li"], xz)


def noise(n, d, obs, sid, S, seed, stream=0, dtype=np.float64):
    base = int(sid) << 40
    eps = _rngref.standard_normal(n * d, S, seed, stream, dtype, row0=base).reshape(n, d, S)
    epsp = _rngref.standard_normal(n * obs, S, seed, stream + 1, dtype, row0=base).reshape(n, obs, S)
    return eps, epsp


def draws(G, Bm, LLT, ts, xs, sid, S, seed, stream=0, observed=None, s=None, prior=False, dtype=np.float64):
    """(rhs [n, d, S], x [n, d, S], K, v) of one series with id `sid`; `dtype` names the generator (fp64 or fp32
    uniforms), the arithmetic is float64 either way."""
    terms = series_terms(G, Bm, LLT, ts, observed, s, prior)
    n, d, obs = terms["H"].shape
    eps, epsp = noise(n, d, obs, sid, S, seed, stream, dtype)
    v = np.zeros((n, d)) if prior else rhs_v(terms, Bm, xs)
    rhs = v[:, :, None] + w_from_noise(terms, eps, epsp)
    K = dense_K(terms)
    x = np.linalg.solve(K, rhs.reshape(n * d, S)).reshape(n, d, S)
    return rhs, x, K, v

"""A truth for the LEG prior that does not go through the PEG block formula, and a cancellation-free restatement of that
formula (tests/test_leg_gaps.py; the dense references of _gradref.py, _missref.py and _noiseref.py).

* ``prior_covariance``: the latent process is stationary with Cov(z_i, z_j) = exp(-(t_i - t_j) G / 2) for t_i >= t_j
  (and the transpose above the diagonal).  Nothing in it is of size 1 / gap, so it stays accurate however close two time
  stamps are: it is what the precision blocks must invert, whatever formula builds them.
* ``blocks_cancel_free``: the blocks of the PEG precision from F = E - I instead of E.  The reference's
  I - E E^T subtracts two matrices of size 1 to get one of size gap * |G|; with E = I + F it is
  M = -(F + F^T + F F^T), three terms of the size of the result.  F comes from
  matrix_exp([[A, I], [0, 0]]) = [[e^A, phi_1(A)], [0, I]]  as  F = A phi_1(A).
Neither calls ``leg.peg_precision``.  torch ops on CPU tensors only."""
import torch

F64 = torch.float64


def prior_covariance(ts, G):
    """[n d, n d] covariance of the latent at the time stamps ts [n] (ascending) for the generator G [d, d]; fp64,
    differentiable in both."""
    ts, G = ts.to(F64), G.to(F64)
    n, d = ts.shape[0], G.shape[0]
    lag = (ts[:, None] - ts[None, :]).abs()
    E = torch.matrix_exp(-0.5 * lag[:, :, None, None] * G)                 # [n, n, d, d], right where t_i >= t_j
    low = (torch.arange(n)[:, None] >= torch.arange(n)[None, :])[:, :, None, None]
    return torch.where(low, E, E.transpose(-1, -2)).permute(0, 2, 1, 3).reshape(n * d, n * d)


def gap_exp(dt, G):
    """(E, F) = (exp(A), exp(A) - I) of A = -dt G / 2 for every gap in dt [m]; F without cancellation."""
    d = G.shape[0]
    A = -0.5 * dt.reshape(-1, 1, 1) * G
    aug = A.new_zeros(A.shape[0], 2 * d, 2 * d)
    aug[:, :d, :d] = A
    aug[:, :d, d:] = torch.eye(d, dtype=A.dtype)
    X = torch.matrix_exp(aug)
    return X[:, :d, :d], A @ X[:, :d, d:]


def blocks_cancel_free(ts, G, dtype=F64):
    """(Rs [n, d, d], Os [n - 1, d, d]) of the PEG prior precision in ``dtype``, differentiable in ts and G."""
    ts, G = ts.to(dtype), G.to(dtype)
    n, d = ts.shape[0], G.shape[0]
    eye = torch.eye(d, dtype=dtype)
    E, F = gap_exp(ts[1:] - ts[:-1], G)
    Et, Ft = E.transpose(-1, -2), F.transpose(-1, -2)
    a = torch.linalg.solve(-(F + Ft + Ft @ F), Et)                         # (I - E^T E)^-1 E^T
    b = torch.linalg.solve(-(F + Ft + F @ Ft), E)                          # (I - E E^T)^-1 E
    Rs = eye.repeat(n, 1, 1)
    Rs[:-1] = Rs[:-1] + Et @ b
    Rs[1:] = Rs[1:] + E @ a
    return Rs, -b


def block_error(got, true):
    """max over blocks of |got - true|_max / max(1, |true|_max): the error of a block against its own size, or against
    1 where the block is small (the identity is added to it)."""
    got, true = got.to(F64), true.to(F64)
    if true.shape[0] == 0:
        return 0.0
    err = (got - true).abs().flatten(1).max(1).values
    return float((err / true.abs().flatten(1).max(1).values.clamp_min(1.0)).max())

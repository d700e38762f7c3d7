"""Writes tests/golden/leg_gap_blocks.npz: the blocks of the PEG prior precision at 60 digits (mpmath), for gaps from
far below to far above the length scale of the generator.  Run by hand (python tests/golden/make_golden_gaps.py), never
by a test; needs mpmath.

For every d in 1..8 and both dtypes (keys "<f32|f64>_d<d>_<name>"):
  G  [d, d]      the generator of tests/test_leg_fused._model(d, dtype, seed), rounded to the dtype; the seed is the
                 first of 100 + d, 200 + d, ... whose sym(G) has a condition number of at most MAX_COND (see below)
  ts [14]        time stamps from 0, rounded to the dtype; the 13 gaps ascend, gap * |G|_1 log-spaced from 1e-7 (fp64)
                 or 1e-5 (fp32) to 2e3, so that the small gaps survive the rounding of the time stamps
  Rs [14, d, d], Os [13, d, d]   fp64, the blocks evaluated at 60 digits FROM THE ROUNDED G and ts:
      E = exp(-gap G / 2),  b = (I - E E^T)^-1 E,  a = (I - E^T E)^-1 E^T,
      Rs_i = I + E_i^T b_i + E_{i-1} a_{i-1},  Os_i = -b_i

Why the condition number is bounded.  a = M^-1 E^T with M = I - E^T E ~ gap * sym(G): whatever forms M in the working
precision and solves with it leaves a relative error of about cond(sym(G)) * eps in the blocks, at EVERY gap.  The
fixture is there to pin the error that grows like eps / gap, so it keeps the other one small: with cond <= 64 a
careful evaluation in the working precision stays within a few tens of eps over the whole range of gaps.
"""
import os

import mpmath as mp
import numpy as np
import torch

ROWS = 14
MAX_COND = 64.0
HERE = os.path.dirname(os.path.abspath(__file__))


def model_G(d, seed):
    """G of test_leg_fused._model, fp64 on the CPU"""
    gen = torch.Generator().manual_seed(seed)
    Nm = torch.tril(0.4 * torch.randn(d, d, generator=gen, dtype=torch.float64)) + 0.8 * torch.eye(d, dtype=torch.float64)
    Rm = torch.tril(0.3 * torch.randn(d, d, generator=gen, dtype=torch.float64), -1)
    return Nm @ Nm.T + Rm - Rm.T + 1e-5 * torch.eye(d, dtype=torch.float64)


def pick_seed(d):
    seed = 100 + d
    while True:
        G = model_G(d, seed)
        ev = torch.linalg.eigvalsh(0.5 * (G + G.T))
        if float(ev[-1] / ev[0]) <= MAX_COND:
            return seed
        seed += 100


def true_blocks(G, ts):
    mp.mp.dps = 60
    d, n = G.shape[0], ts.shape[0]
    Gm = mp.matrix([[mp.mpf(float(G[i, j])) for j in range(d)] for i in range(d)])
    eye = mp.eye(d)
    Rs = [eye.copy() for _ in range(n)]
    Os = []
    for i in range(n - 1):
        tau = mp.mpf(float(ts[i + 1])) - mp.mpf(float(ts[i]))
        E = mp.expm(-tau / 2 * Gm)
        b = mp.inverse(eye - E * E.T) * E
        a = mp.inverse(eye - E.T * E) * E.T
        Rs[i] += E.T * b
        Rs[i + 1] += E * a
        Os.append(-b)
    def f(Ms):
        return np.array([[[float(M[i, j]) for j in range(d)] for i in range(d)] for M in Ms], dtype=np.float64)
    return f(Rs), f(Os)


def main():
    out = {}
    for name, dtype, lo in (("f32", np.float32, 1e-5), ("f64", np.float64, 1e-7)):
        for d in range(1, 9):
            G = model_G(d, pick_seed(d)).numpy().astype(dtype)
            norm1 = float(np.abs(G.astype(np.float64)).sum(0).max())
            gaps = np.logspace(np.log10(lo), np.log10(2e3), ROWS - 1) / norm1
            ts = np.concatenate([[0.0], np.cumsum(gaps)]).astype(dtype)
            assert np.all(np.diff(ts.astype(np.float64)) > 0)
            Rs, Os = true_blocks(G, ts)
            for k, v in (("G", G), ("ts", ts), ("Rs", Rs), ("Os", Os)):
                out["%s_d%d_%s" % (name, d, k)] = v
    np.savez_compressed(os.path.join(HERE, "leg_gap_blocks.npz"), **out)


if __name__ == "__main__":
    main()

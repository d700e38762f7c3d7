"""``leg.observation_tables`` and ``leg.merge_targets`` on the CPU (no kernels): every pattern of obs = 1 ... 4 against
explicit sub-matrix inverses and log-determinants, the code of a mask row, the all-observed entry against what the
fully observed code computes, the ValueErrors, and the masked log-likelihood / posterior formulas against the dense
Gaussian of the observed entries (tests/_missref.py) with the blocks assembled densely."""
import math

import numpy as np
import pytest
import torch

import _gradref as gr
import _missref as mr
from cyclic_gps import leg

F64 = torch.float64


def _model(d, obs, seed):
    (Nm, Rm, Bm, Lm, _, _), _ = mr.leg_case(d, obs, 3, seed)
    return leg.LEGMatrices(Nm, Rm, Bm, Lm)


@pytest.mark.parametrize("obs", [1, 2, 3, 4])
def test_every_pattern_against_explicit_submatrices(obs):
    d = 3
    m = _model(d, obs, 10 + obs)
    P = 1 << obs
    masks = torch.tensor([[(p >> c) & 1 for c in range(obs)] for p in range(P)], dtype=torch.bool)
    pattern, A_table, Li_table, c_table = leg.observation_tables(m, masks)
    assert pattern.dtype == torch.uint8 and pattern.tolist() == list(range(P))       # row p of `masks` has code p
    assert A_table.shape == (P, d, d) and Li_table.shape == (P, obs, obs) and c_table.shape == (P,)
    LLT = m.LLT
    for p in range(P):
        S = [c for c in range(obs) if (p >> c) & 1]
        Li = torch.zeros(obs, obs, dtype=F64)
        logdet = 0.0
        if S:
            sub = LLT[S][:, S]
            Li[np.ix_(S, S)] = torch.linalg.inv(sub)
            logdet = float(torch.logdet(sub))
        np.testing.assert_allclose(Li_table[p].numpy(), Li.numpy(), rtol=1e-12, atol=1e-12 * float(Li.abs().max()))
        want_A = m.B.T @ Li @ m.B
        np.testing.assert_allclose(A_table[p].numpy(), want_A.numpy(), rtol=1e-11, atol=1e-12 * max(1.0, float(want_A.abs().max())))
        want_c = len(S) * math.log(2 * math.pi) + logdet
        assert abs(float(c_table[p]) - want_c) <= 1e-12 * max(1.0, abs(want_c))
    assert float(Li_table[0].abs().max()) == 0.0 and float(A_table[0].abs().max()) == 0.0 and float(c_table[0]) == 0.0


@pytest.mark.parametrize("obs", [1, 2, 3])
def test_all_observed_entry_is_what_the_fully_observed_code_computes(obs):
    m = _model(4, obs, 20 + obs)
    n = 5
    for observed in (torch.ones(n, obs, dtype=torch.bool), torch.ones(n, dtype=torch.bool)):      # per channel, per row
        pattern, A_table, Li_table, c_table = leg.observation_tables(m, observed)
        assert pattern.tolist() == [(1 << obs) - 1] * n
        Li = m.LLT_inv
        np.testing.assert_allclose(Li_table[-1].numpy(), Li.numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(A_table[-1].numpy(), (m.B.T @ Li @ m.B).numpy(), rtol=1e-11, atol=1e-13)
        want = torch.log(2 * math.pi * m.LLT[0, 0]) if obs == 1 else torch.logdet(2 * math.pi * m.LLT)
        assert abs(float(c_table[-1]) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    pattern, _, _, _ = leg.observation_tables(m, torch.tensor([True, False, True]))
    assert pattern.tolist() == [(1 << obs) - 1, 0, (1 << obs) - 1]


def test_code_of_a_mask_row():
    m = _model(2, 3, 5)
    observed = torch.tensor([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [0, 0, 0], [1, 1, 1]], dtype=torch.bool)
    assert leg.observation_tables(m, observed)[0].tolist() == [1, 2, 4, 5, 0, 7]
    m8 = leg.LEGMatrices(torch.eye(2, dtype=F64), torch.zeros(2, 2, dtype=F64), torch.ones(8, 2, dtype=F64), torch.eye(8, dtype=F64))
    pattern, A_table, _, _ = leg.observation_tables(m8, torch.ones(2, 8, dtype=torch.bool))
    assert pattern.tolist() == [255, 255] and A_table.shape == (256, 2, 2)


def test_value_errors():
    m = _model(2, 2, 6)
    ts, xs = torch.arange(4, dtype=F64), torch.zeros(4, 2, dtype=F64)
    with pytest.raises(ValueError):
        leg.observation_tables(m, torch.ones(4, 3, dtype=torch.bool))          # not obs_dim columns
    with pytest.raises(ValueError):
        leg.observation_tables(m, torch.ones(4, 2, dtype=F64))                  # not bool
    with pytest.raises(ValueError):
        leg.log_likelihood(m, ts, xs, observed=torch.ones(5, 2, dtype=torch.bool))      # not the rows of xs
    with pytest.raises(ValueError):
        leg.insample_posterior(m, ts, xs, observed=torch.ones(3, dtype=torch.bool))
    m9 = leg.LEGMatrices(torch.eye(2, dtype=F64), torch.zeros(2, 2, dtype=F64), torch.ones(9, 2, dtype=F64), torch.eye(9, dtype=F64))
    with pytest.raises(ValueError):
        leg.observation_tables(m9, torch.ones(4, 9, dtype=torch.bool))          # obs_dim > 8


def test_tables_are_differentiable_in_B_and_Lambda():
    (Nm, Rm, Bm, Lm, _, _), mask = mr.leg_case(3, 2, 6, 31)
    Bm, Lm = Bm.requires_grad_(True), Lm.requires_grad_(True)
    _, A_table, Li_table, c_table = leg.observation_tables(leg.LEGMatrices(Nm, Rm, Bm, Lm), mask)
    (A_table.sum() + Li_table.sum() + c_table.sum()).backward()
    assert Bm.grad is not None and Lm.grad is not None and torch.isfinite(Bm.grad).all() and torch.isfinite(Lm.grad).all()


@pytest.mark.parametrize("d,obs,n", [(3, 3, 37), (2, 1, 12)])
def test_masked_formulas_against_the_dense_gaussian_of_the_observed_entries(d, obs, n):
    """ll and the posterior at all rows from the tables, with K assembled densely on the CPU (no kernels): NaN in the
    unobserved entries of xs is ignored."""
    (Nm, Rm, Bm, Lm, xs, ts), mask = mr.leg_case(d, obs, n, 50 + d)
    m = leg.LEGMatrices(Nm, Rm, Bm, Lm)
    want_ll = mr.leg_dense_loglik(Nm, Rm, Bm, Lm, ts, xs, mask)
    want_mean, want_cov = mr.leg_dense_posterior(Nm, Rm, Bm, Lm, ts, xs, mask)
    xs = torch.where(mask, xs, torch.full_like(xs, float("nan")))
    pattern, A_table, Li_table, c_table = leg.observation_tables(m, mask)
    idx = pattern.long()
    xz = torch.where(mask, xs, torch.zeros_like(xs))
    xl = torch.einsum("no,nop->np", xz, Li_table[idx])
    v = xl @ Bm
    Rs, Os = leg.peg_precision(ts, m.G)
    K = gr.dense_J(Rs + A_table[idx], Os)
    w = torch.linalg.solve(K, v.reshape(-1))
    ll = -0.5 * (((xl * xz).sum() - v.reshape(-1) @ w) + (c_table[idx].sum() + torch.logdet(K) - torch.logdet(gr.dense_J(Rs, Os))))
    assert abs(float(ll) - float(want_ll)) <= 1e-10 * max(1.0, abs(float(want_ll)))
    np.testing.assert_allclose(w.reshape(n, d).numpy(), want_mean.numpy(), rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(torch.linalg.inv(K).numpy(), want_cov.reshape(n * d, n * d).numpy(), rtol=1e-8, atol=1e-10)


def test_merge_targets_on_the_cpu():
    ts = torch.tensor([0.0, 1.0, 2.5, 4.0], dtype=F64)
    xs = torch.arange(8, dtype=F64).reshape(4, 2)
    tt = torch.tensor([3.0, -1.0, 0.5, 9.0], dtype=F64)
    ts_all, xs_all, observed, where = leg.merge_targets(ts, xs, tt)
    assert ts_all.tolist() == [-1.0, 0.0, 0.5, 1.0, 2.5, 3.0, 4.0, 9.0]
    assert observed.tolist() == [False, True, False, True, True, False, True, False]
    assert where.tolist() == [5, 0, 2, 7] and torch.equal(ts_all[where], tt)
    assert torch.equal(xs_all[observed], xs) and float(xs_all[~observed].abs().max()) == 0.0
    with pytest.raises(ValueError):
        leg.merge_targets(ts, xs, torch.tensor([2.5], dtype=F64))
    ts_all, _, observed, where = leg.merge_targets(ts, xs, torch.tensor([2.5], dtype=F64), check=False)
    assert ts_all.tolist() == [0.0, 1.0, 2.5, 2.5, 4.0] and where.tolist() == [3] and observed.tolist() == [True, True, True, False, True]

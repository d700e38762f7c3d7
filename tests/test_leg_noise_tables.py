"""``leg.observation_weights`` on the CPU (no kernels): every row against explicit sub-matrix inverses and
log-determinants for obs = 1 ... 4 with random masks and variances, the weighted basis against B^T Li B, zero variances
against ``leg.observation_tables``, the [n] broadcast, NaN at unobserved entries, the log-likelihood / posterior formulas
against the dense Gaussian of the observed entries (tests/_noiseref.py) with the blocks assembled densely, the
ValueErrors, and the argument checks of the C entry."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _gradref as gr
import _noiseref as nr
from cyclic_gps import _hip, leg

F64 = torch.float64


def _model(d, obs, seed):
    (Nm, Rm, Bm, Lm, _, _, _), _ = nr.leg_case(d, obs, 3, seed)
    return leg.LEGMatrices(Nm, Rm, Bm, Lm)


def _rows(n, obs, seed):
    """random mask (rows observing everything, nothing and something in between all occur) and s in [0, 2]"""
    gen = torch.Generator().manual_seed(seed)
    mask = torch.rand(n, obs, generator=gen) < 0.6
    mask[0] = True
    mask[1] = False
    return mask, 2.0 * torch.rand(n, obs, generator=gen, dtype=F64)


@pytest.mark.parametrize("obs", [1, 2, 3, 4])
def test_every_row_against_explicit_submatrices(obs):
    d, n = 3, 40
    m = _model(d, obs, 10 + obs)
    mask, s = _rows(n, obs, 100 + obs)
    basis, weights, Li_rows, c_rows = leg.observation_weights(m, mask, s)
    Kb = obs * (obs + 1) // 2
    assert basis.shape == (Kb, d, d) and weights.shape == (n, Kb) and Li_rows.shape == (n, obs, obs) and c_rows.shape == (n,)
    pairs = [(c, e) for c in range(obs) for e in range(c + 1)]           # row-major over the lower triangle
    for k, (c, e) in enumerate(pairs):
        bc, be = m.B[c], m.B[e]
        want = torch.outer(bc, bc) if c == e else torch.outer(bc, be) + torch.outer(be, bc)
        np.testing.assert_allclose(basis[k].numpy(), want.numpy(), rtol=1e-14, atol=0)
    LLT = m.LLT
    for i in range(n):
        S = [c for c in range(obs) if mask[i, c]]
        Li = torch.zeros(obs, obs, dtype=F64)
        logdet = 0.0
        if S:
            sub = (LLT + torch.diag(s[i]))[S][:, S]
            Li[np.ix_(S, S)] = torch.linalg.inv(sub)
            logdet = float(torch.logdet(sub))
        np.testing.assert_allclose(Li_rows[i].numpy(), Li.numpy(), rtol=1e-12, atol=1e-12 * max(1.0, float(Li.abs().max())))
        for k, (c, e) in enumerate(pairs):
            assert float(weights[i, k]) == float(Li_rows[i, c, e])
        want_A = m.B.T @ Li @ m.B
        got_A = torch.einsum("k,kij->ij", weights[i], basis)
        np.testing.assert_allclose(got_A.numpy(), want_A.numpy(), rtol=0, atol=1e-12 * max(1.0, float(want_A.abs().max())))
        want_c = len(S) * math.log(2 * math.pi) + logdet
        assert abs(float(c_rows[i]) - want_c) <= 1e-12 * max(1.0, abs(want_c))
        if not S:
            assert float(weights[i].abs().max()) == 0.0 and float(c_rows[i]) == 0.0


@pytest.mark.parametrize("obs", [1, 2, 3])
def test_zero_variance_reproduces_the_tables_row_by_row(obs):
    m = _model(4, obs, 20 + obs)
    mask, _ = _rows(30, obs, 200 + obs)
    pattern, A_table, Li_table, c_table = leg.observation_tables(m, mask)
    idx = pattern.long()
    basis, weights, Li_rows, c_rows = leg.observation_weights(m, mask, torch.zeros(30, obs, dtype=F64))
    np.testing.assert_allclose(Li_rows.numpy(), Li_table[idx].numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(c_rows.numpy(), c_table[idx].numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(torch.einsum("nk,kij->nij", weights, basis).numpy(), A_table[idx].numpy(), rtol=0, atol=1e-12)
    # observed=None is everything observed: the fully observed system
    basis, weights, Li_rows, c_rows = leg.observation_weights(m, None, torch.zeros(30, dtype=F64))
    np.testing.assert_allclose(Li_rows.numpy(), m.LLT_inv.expand(30, -1, -1).numpy(), rtol=1e-12, atol=1e-14)
    want = torch.log(2 * math.pi * m.LLT[0, 0]) if obs == 1 else torch.logdet(2 * math.pi * m.LLT)
    np.testing.assert_allclose(c_rows.numpy(), np.full(30, float(want)), rtol=1e-12)
    np.testing.assert_allclose(torch.einsum("nk,kij->nij", weights, basis).numpy(),
                               (m.B.T @ m.LLT_inv @ m.B).expand(30, -1, -1).numpy(), rtol=0, atol=1e-12)


def test_one_variance_per_row_is_broadcast_over_the_channels():
    m = _model(3, 3, 7)
    mask, s = _rows(12, 3, 8)
    a = leg.observation_weights(m, mask, s[:, 0])
    b = leg.observation_weights(m, mask, s[:, :1].expand(-1, 3).contiguous())
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    c = leg.observation_weights(m, mask[:, 0], s[:, 0])                    # whole rows, one variance each
    d = leg.observation_weights(m, mask[:, :1].expand(-1, 3), s[:, 0])
    for x, y in zip(c, d):
        assert torch.equal(x, y)


@pytest.mark.parametrize("obs", [1, 3])
def test_nan_at_unobserved_entries_is_ignored(obs):
    d, n = 3, 25
    (Nm, Rm, Bm, Lm, xs, ts, _), _ = nr.leg_case(d, obs, n, 40 + obs)
    m = leg.LEGMatrices(Nm, Rm, Bm, Lm)
    mask, s = _rows(n, obs, 41 + obs)
    nan = torch.full_like(s, float("nan"))
    clean = leg.observation_weights(m, mask, s)
    dirty = leg.observation_weights(m, mask, torch.where(mask, s, nan))
    for x, y in zip(clean, dirty):
        assert torch.isfinite(y).all() and torch.equal(x, y)
    a = leg._posterior_system(m, ts, xs, mask, s)
    b = leg._posterior_system(m, ts, torch.where(mask, xs, nan), mask, torch.where(mask, s, nan))
    for x, y in zip(a, b):
        assert torch.isfinite(y).all() and torch.equal(x, y)
    # ... and the gradient of noise_var is finite, and zero where nothing is observed
    sg = torch.where(mask, s, nan).requires_grad_(True)
    out = leg.observation_weights(m, mask, sg)
    (out[1].sum() + out[3].sum()).backward()
    assert torch.isfinite(sg.grad).all() and float(sg.grad[~mask].abs().max()) == 0.0


def test_weights_are_differentiable_in_B_Lambda_and_the_variances():
    (Nm, Rm, Bm, Lm, _, _, s), mask = nr.leg_case(3, 2, 6, 31)
    Bm, Lm, s = Bm.requires_grad_(True), Lm.requires_grad_(True), s.requires_grad_(True)
    basis, weights, Li_rows, c_rows = leg.observation_weights(leg.LEGMatrices(Nm, Rm, Bm, Lm), mask, s)
    (basis.sum() + weights.sum() + Li_rows.sum() + c_rows.sum()).backward()
    for g in (Bm.grad, Lm.grad, s.grad):
        assert g is not None and torch.isfinite(g).all()


@pytest.mark.parametrize("d,obs,n", [(3, 3, 37), (2, 1, 12), (5, 2, 20)])
def test_formulas_against_the_dense_gaussian_of_the_observed_entries(d, obs, n):
    """ll and the posterior at all rows from the weights, with K assembled densely on the CPU (no kernels)."""
    (Nm, Rm, Bm, Lm, xs, ts, s), mask = nr.leg_case(d, obs, n, 50 + d)
    m = leg.LEGMatrices(Nm, Rm, Bm, Lm)
    want_ll = nr.leg_dense_loglik(Nm, Rm, Bm, Lm, ts, xs, s, mask)
    want_mean, want_cov = nr.leg_dense_posterior(Nm, Rm, Bm, Lm, ts, xs, s, mask)
    nan = torch.full_like(xs, float("nan"))
    xs, s = torch.where(mask, xs, nan), torch.where(mask, s, nan)
    basis, weights, Li_rows, c_rows = leg.observation_weights(m, mask, s)
    xz = torch.where(mask, xs, torch.zeros_like(xs))
    xl = torch.einsum("no,nop->np", xz, Li_rows)
    v = xl @ Bm
    Rs, Os = leg.peg_precision(ts, m.G)
    K = gr.dense_J(Rs + torch.einsum("nk,kij->nij", weights, basis), Os)
    w = torch.linalg.solve(K, v.reshape(-1))
    ll = -0.5 * (((xl * xz).sum() - v.reshape(-1) @ w) + (c_rows.sum() + torch.logdet(K) - torch.logdet(gr.dense_J(Rs, Os))))
    assert abs(float(ll) - float(want_ll)) <= 1e-10 * max(1.0, abs(float(want_ll)))
    np.testing.assert_allclose(w.reshape(n, d).numpy(), want_mean.numpy(), rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(torch.linalg.inv(K).numpy(), want_cov.reshape(n * d, n * d).numpy(), rtol=1e-8, atol=1e-10)
    K_Rs, K_Os, v2 = leg._posterior_system(m, ts, xs, mask, s)             # what the public functions factor
    np.testing.assert_allclose(gr.dense_J(K_Rs, K_Os).numpy(), K.numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(v2.numpy(), v.numpy(), rtol=1e-13, atol=1e-13)


def test_value_errors():
    m = _model(2, 2, 6)
    ts, xs = torch.arange(4, dtype=F64), torch.zeros(4, 2, dtype=F64)
    ok = torch.ones(4, 2, dtype=torch.bool)
    with pytest.raises(ValueError):
        leg.observation_weights(m, ok, torch.zeros(4, 3, dtype=F64))            # not obs_dim columns
    with pytest.raises(ValueError):
        leg.observation_weights(m, ok, torch.zeros(4, 2, 1, dtype=F64))
    with pytest.raises(ValueError):
        leg.observation_weights(m, ok, torch.zeros(4, 2, dtype=torch.int64))    # not floating point
    with pytest.raises(ValueError):
        leg.observation_weights(m, ok, [[0.0, 0.0]] * 4)                        # not a tensor
    with pytest.raises(ValueError):
        leg.observation_weights(m, ok, torch.zeros(5, 2, dtype=F64))            # not the rows of observed
    with pytest.raises(ValueError):
        leg.observation_weights(m, torch.ones(4, 2, dtype=F64), torch.zeros(4, 2, dtype=F64))      # observed not bool
    with pytest.raises(ValueError):
        leg.log_likelihood(m, ts, xs, noise_var=torch.zeros(5, 2, dtype=F64))   # not the rows of xs
    with pytest.raises(ValueError):
        leg.log_likelihood(m, ts, xs, observed=torch.ones(3, dtype=torch.bool), noise_var=torch.zeros(4, dtype=F64))
    with pytest.raises(ValueError):
        leg.insample_posterior(m, ts, xs, noise_var=torch.zeros(3, dtype=F64))
    with pytest.raises(ValueError):
        leg.sample_from_posterior(m, ts, xs, 2, 0, noise_var=torch.zeros(4, 3, dtype=F64))
    m9 = leg.LEGMatrices(torch.eye(2, dtype=F64), torch.zeros(2, 2, dtype=F64), torch.ones(9, 2, dtype=F64), torch.eye(9, dtype=F64))
    with pytest.raises(ValueError):
        leg.observation_weights(m9, None, torch.zeros(4, 9, dtype=F64))         # obs_dim > 8


def test_wrapper_checks_shapes_and_dtypes_before_anything_is_launched():
    """CPU tensors throughout: every call below must raise before it reaches the library."""
    n, d, Kb = 6, 3, 3
    ts, G, v = torch.arange(n, dtype=F64), torch.eye(d, dtype=F64), torch.zeros(n, d, dtype=F64)
    basis, weights = torch.zeros(Kb, d, d, dtype=F64), torch.zeros(n, Kb, dtype=F64)
    for bad_basis in (basis[0], torch.zeros(Kb, d, d + 1, dtype=F64), torch.zeros(0, d, d, dtype=F64),
                      torch.zeros(65, d, d, dtype=F64)):
        with pytest.raises(ValueError, match="basis"):
            leg.leg_loglik_reductions_w(ts, G, bad_basis, weights, v)
    for bad_w in (weights[:-1], weights[:, :-1], weights.reshape(-1), weights.T):
        with pytest.raises(ValueError, match="weights"):
            leg.leg_loglik_reductions_w(ts, G, basis, bad_w, v)
    with pytest.raises(ValueError, match="v must"):
        leg.leg_loglik_reductions_w(ts, G, basis, weights, v[:-1])
    with pytest.raises(ValueError, match="dtype"):
        leg.leg_loglik_reductions_w(ts, G, basis, weights.float(), v)
    with pytest.raises(ValueError, match="dtype"):
        leg.leg_loglik_reductions_w(ts, G, basis.float(), weights, v)
    with pytest.raises(ValueError, match="device"):
        leg.leg_loglik_reductions_w(ts, G, basis, weights, v)


def test_c_entry_is_exported_and_checks_its_arguments_before_any_launch():
    assert "cgps_leg_mahal_logdet_pair_w" in _hip.exported_symbols()
    lib = _hip.lib()
    fn = lib.cgps_leg_mahal_logdet_pair_w
    assert lib.cgps_version() == 320
    fake = ctypes.c_void_p(256)
    call = lambda basis, Kb, w, N=10, d=5, dt=_hip.F64, ts=fake, ws=fake: fn(       # noqa: E731
        ts, fake, basis, Kb, w, None, N, d, dt, ws, 1 << 20, fake, fake, None)
    assert call(fake, 0, fake) == 1 and b"cgps_leg_mahal_logdet_pair_w" in lib.cgps_last_error()
    assert call(fake, 65, fake) == 1 and call(fake, -1, fake) == 1
    assert call(None, 6, fake) == 1 and call(fake, 6, None) == 1
    assert call(fake, 6, fake, N=0) == 1 and call(fake, 6, fake, N=-3) == 1
    assert call(fake, 6, fake, ts=None) == 1 and call(fake, 6, fake, ws=None) == 1
    assert fn(fake, None, fake, 6, fake, None, 10, 5, _hip.F64, fake, 1 << 20, fake, fake, None) == 1
    assert fn(fake, fake, fake, 6, fake, None, 10, 5, _hip.F64, fake, 1 << 20, None, fake, None) == 1
    assert fn(fake, fake, fake, 6, fake, None, 10, 5, _hip.F64, fake, 1 << 20, fake, None, None) == 1
    # d = 8 and fp64 d = 6 are refused before any launch (the pointers are never touched)
    for d, dt in ((8, _hip.F64), (8, _hip.F32), (6, _hip.F64)):
        assert call(fake, 6, fake, d=d, dt=dt) == 3

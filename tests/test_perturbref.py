"""The definition of the perturb-and-solve draw (tests/_perturbref.py) checked on the CPU in float64:
with the generator replaced by unit vectors the map noise -> w satisfies W W^T = K exactly (up to rounding), the
observation factor satisfies (M T^-T)(M T^-T)^T = Li, and the torch builder of H (leg.observation_noise_factors) agrees
with the restatement.  No GPU."""
import os
import re

import numpy as np
import torch

import _perturbref as pr
import _util
from cyclic_gps import _hip, leg

LENGTHS = [1, 4, 7]


def _case():
    g = np.load(os.path.join(_util.GOLDEN, "leg_small_irregular.npz"))
    G, Bm, LLT = pr.model(g["N"], g["R"], g["B"], g["Lambda"])
    torch.manual_seed(1)
    masks = [(torch.rand(n, Bm.shape[0]) > 0.3).numpy() for n in LENGTHS]           # drawn per series, in order
    series, s0 = [], 0
    for n, mask in zip(LENGTHS, masks):
        var = (2.0 * torch.rand(n, Bm.shape[0], dtype=torch.float64)).numpy()
        series.append((g["ts"][s0:s0 + n], g["xs"][s0:s0 + n], mask, var))
        s0 += n
    m = leg.LEGMatrices(*(torch.from_numpy(g[k]) for k in ("N", "R", "B", "Lambda")))
    return G, Bm, LLT, series, m


def _w_matrix(terms):
    """The dense map (eps, eps') -> w: the generator replaced by the unit vectors."""
    n, d, obs = terms["H"].shape
    eye = np.eye(n * d + n * obs)
    return pr.w_from_noise(terms, eye[:n * d].reshape(n, d, -1), eye[n * d:].reshape(n, obs, -1)).reshape(n * d, -1)


def test_w_w_transpose_is_k():
    G, Bm, LLT, series, _ = _case()
    for ts, _, mask, var in series:
        for observed, s, prior in ((None, None, False), (mask, None, False), (None, var, False), (mask, var, False),
                                   (None, None, True)):
            terms = pr.series_terms(G, Bm, LLT, ts, observed, s, prior)
            W = _w_matrix(terms)
            K = pr.dense_K(terms)
            truth = pr.dense_K_truth(G, Bm, ts, terms["Li"])
            scale = np.abs(truth).max()
            err, err_truth = np.abs(W @ W.T - K).max() / scale, np.abs(K - truth).max() / scale
            print("n=%d prior=%s: |W W^T - K| / max|K| = %.2g, |K - K_truth| / max|K| = %.2g" % (len(ts), prior, err, err_truth))
            assert err <= 1e-12 and err_truth <= 1e-10, (err, err_truth)
            Ki = np.linalg.inv(truth)
            assert np.abs(Ki @ W @ W.T @ Ki - Ki).max() <= 1e-10 * np.abs(Ki).max()


def test_observation_factor_is_a_root_of_li():
    _, Bm, LLT, series, _ = _case()
    obs = Bm.shape[0]
    rows = [(np.array([(p >> c) & 1 for c in range(obs)], dtype=bool), np.zeros(obs)) for p in range(1 << obs)]
    rows += [(mask[r], var[r]) for _, _, mask, var in series for r in range(len(mask))]
    for observed, s in rows:
        H, Li = pr.h_block(Bm, LLT, observed, s)
        assert np.abs(H @ H.T - Bm.T @ Li @ Bm).max() <= 1e-13 * max(1.0, np.abs(Bm.T @ Li @ Bm).max())
        assert not H[:, ~observed].any()                        # noise at an unobserved channel multiplies zero
        C = (LLT + np.diag(s))[np.ix_(observed, observed)]
        if observed.any():
            assert np.abs(Li[np.ix_(observed, observed)] - np.linalg.inv(C)).max() <= 1e-12 * np.abs(np.linalg.inv(C)).max()


def test_torch_factors_agree_with_the_restatement():
    _, Bm, LLT, series, m = _case()
    obs = Bm.shape[0]
    H0 = leg.observation_noise_factors(m).numpy()
    np.testing.assert_allclose(H0, pr.h_block(Bm, LLT, np.ones(obs, dtype=bool), np.zeros(obs))[0], rtol=1e-12, atol=1e-14)
    mask = torch.from_numpy(np.concatenate([sr[2] for sr in series]))
    var = torch.from_numpy(np.concatenate([sr[3] for sr in series]))
    var_nan = torch.where(mask, var, torch.full_like(var, float("nan")))          # ignored where unobserved
    table = leg.observation_noise_factors(m, observed=mask).numpy()
    pattern = leg.observation_tables(m, mask)[0].numpy()
    rows_m = leg.observation_noise_factors(m, observed=mask, noise_var=var_nan).numpy()
    rows_v = leg.observation_noise_factors(m, noise_var=var).numpy()
    assert table.shape == (1 << obs, Bm.shape[1], obs) and rows_m.shape == (mask.shape[0], Bm.shape[1], obs)
    for r in range(mask.shape[0]):
        o, s = mask[r].numpy(), var[r].numpy()
        np.testing.assert_allclose(table[pattern[r]], pr.h_block(Bm, LLT, o, np.zeros(obs))[0], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(rows_m[r], pr.h_block(Bm, LLT, o, s)[0], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(rows_v[r], pr.h_block(Bm, LLT, np.ones(obs, dtype=bool), s)[0], rtol=1e-12, atol=1e-14)
        assert not table[pattern[r]][:, ~o].any() and not rows_m[r][:, ~o].any()


def test_symbol_is_declared_and_exported():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "cgps.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+cgps_leg_perturbation_seg\s*\(", text)
    assert "cgps_leg_perturbation_seg" in _hip.exported_symbols() and hasattr(_hip.lib(), "cgps_leg_perturbation_seg")
    for name in ("posterior_perturbation_batch", "sample_from_posterior_batch", "sample_from_prior_batch"):
        assert callable(getattr(leg, name))


def test_arguments_outside_the_contract_launch_nothing():
    """CGPS_ERR_ARG (1) / CGPS_ERR_UNSUPPORTED (3) come back before the runtime is touched: no GPU needed.  The
    pointers are never dereferenced on the host."""
    import ctypes
    fn, p = _hip.lib().cgps_leg_perturbation_seg, ctypes.c_void_p(64)

    def call(R=4, d=3, dtype=_hip.F64, B=1, hsource=_hip.H_PLAIN, hterm=p, entries=0, obs=2, rows=None, nrhs=2, ts=p, out=p):
        return fn(ts, R, p, d, dtype, p, p, B, hsource, hterm, entries, obs, rows, None, nrhs, 1, 0, out, p, None)

    assert call(B=0) == 0 and call(R=0) == 0                       # nothing to do: CGPS_OK
    for kw in (dict(B=-1), dict(R=-1), dict(nrhs=0), dict(ts=None), dict(out=None), dict(hsource=4), dict(hsource=-1),
               dict(hterm=None), dict(obs=0), dict(obs=9), dict(hsource=_hip.H_TABLE, entries=4),
               dict(hsource=_hip.H_TABLE, rows=p, entries=0), dict(hsource=_hip.H_TABLE, rows=p, entries=257), dict(d=0)):
        assert call(**kw) == 1, kw
    assert call(d=9) == 3 and call(dtype=7) == 3

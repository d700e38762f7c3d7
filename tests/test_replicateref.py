"""The definition of the replicated observations (tests/_replicateref.py) checked on the CPU in
float64: with the generator replaced by unit vectors the map noise -> x - B z is a lower-triangular root of
LLT + diag(s mask) for every mask; the stream words of a draw and its replicate are distinct, and distinct from every
word of another model under the default stream + 4 k.  The new C entries are declared, exported and refuse arguments
outside their contract before the runtime is touched.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import _missref as mr
import _replicateref as rr
from cyclic_gps import _hip, leg


def test_noise_factor_is_a_root_of_the_rows_noise_covariance():
    obs, d = 3, 4
    (Nm, Rm, Bm, Lm, _, _), _ = mr.leg_case(d, obs, 4, 17)
    _, Bn, LLT = rr.model(Nm.numpy(), Rm.numpy(), Bm.numpy(), Lm.numpy())
    s = np.array([0.7, 0.05, 1.9])
    masks = np.array([[(p >> c) & 1 for c in range(obs)] for p in range(1 << obs)], dtype=bool)
    n = len(masks)
    s_nan = np.where(masks, s, np.nan)                              # ignored where unobserved
    # z = 0 and eps''_r = I: x[r] is T_r itself
    T = rr.replicate_from_noise(Bn, LLT, np.zeros((n, d, obs)), np.broadcast_to(np.eye(obs), (n, obs, obs)), masks, s_nan)
    for r in range(n):
        C = LLT + np.diag(np.where(masks[r], s, 0.0))
        err = np.abs(T[r] @ T[r].T - C).max() / np.abs(C).max()
        print("mask %s: |T T^T - (LLT + diag(s mask))| / max = %.2g" % (masks[r].astype(int), err))
        assert err <= 1e-12, (r, err)
        assert not np.triu(T[r], 1).any() and (np.diag(T[r]) > 0).all()
    # no mask, no variances: the factor of LLT alone; the latent part is B z
    z = np.random.default_rng(0).standard_normal((2, d, 5))
    x0 = rr.replicate_from_noise(Bn, LLT, z, np.zeros((2, obs, 5)))
    np.testing.assert_allclose(x0, np.einsum("cj,rjs->rcs", Bn, z), rtol=1e-14, atol=1e-15)
    T0 = rr.replicate_from_noise(Bn, LLT, np.zeros((1, d, obs)), np.eye(obs)[None])[0]
    assert np.abs(T0 @ T0.T - LLT).max() <= 1e-12 * np.abs(LLT).max()


def test_stream_words_of_draws_and_replicates_do_not_collide():
    for stream in (0, 7, leg.MAX_STREAM_WORD - 4 * 2):
        M = 3
        words = [rr.draw_words(w) for w in rr.default_model_streams(M, stream)]
        assert rr.default_model_streams(M, stream) == leg._model_stream_words(M, stream, None)
        for k, wk in enumerate(words):
            assert len(set(wk)) == 3                                # latent, observation noise, replicate
            for j, wj in enumerate(words):
                assert j == k or not set(wk) & set(wj), (stream, k, j)
        assert max(max(w) for w in words) < 1 << 32                 # the generator's word is 32 bits
    # the replicate of a series reads other numbers than the draw's observation noise of the same rows
    a = rr.noise(5, 2, 9, 4, seed=3, stream=0)
    b = rr._rngref.standard_normal(10, 4, 3, 1, np.float64, row0=9 << 40).reshape(5, 2, 4)
    assert not np.isclose(a, b).any()


def test_stream_word_arguments():
    assert leg._model_stream_words(3, 5, None) == [5, 9, 13]
    assert leg._model_stream_words(3, 0, [7, 7, 2]) == [7, 7, 2]
    import torch
    assert leg._model_stream_words(2, 0, torch.tensor([4, leg.MAX_STREAM_WORD])) == [4, (1 << 32) - 4]
    for bad in (lambda: leg._model_stream_words(3, 0, [1, 2]), lambda: leg._model_stream_words(2, 0, [0, (1 << 32) - 3]),
                lambda: leg._model_stream_words(2, 0, [-1, 0]), lambda: leg._model_stream_words(2, (1 << 32) - 6, None),
                lambda: leg._model_stream_words(2, 0, torch.tensor([0.0, 1.0]))):
        with pytest.raises(ValueError):
            bad()


def test_symbols_are_declared_and_exported():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "cgps.h")).read(), flags=re.S)
    for name in ("cgps_leg_perturbation_models", "cgps_leg_observations"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text)
        assert name in _hip.exported_symbols() and hasattr(_hip.lib(), name)
    for name in ("posterior_perturbation_models", "sample_from_posterior_models", "sample_from_prior_models",
                 "sample_observations_batch", "sample_observations_models"):
        assert callable(getattr(leg, name))


def test_arguments_outside_the_contract_launch_nothing():
    """CGPS_ERR_ARG (1) / CGPS_ERR_UNSUPPORTED (3) come back before the runtime is touched: no GPU needed.  The
    pointers are never dereferenced on the host."""
    lib, p = _hip.lib(), ctypes.c_void_p(64)

    def pert(R=4, M=2, d=3, dtype=_hip.F64, B=1, hsource=_hip.H_PLAIN, hterm=p, entries=0, obs=2, rows=None, nrhs=2, ts=p,
             out=p, words=p):
        return lib.cgps_leg_perturbation_models(ts, R, M, p, d, dtype, p, p, B, hsource, hterm, entries, obs, rows, None, nrhs,
                                                1, words, out, p, None)

    assert pert(B=0) == 0 and pert(R=0) == 0                       # nothing to do: CGPS_OK
    for kw in (dict(B=-1), dict(R=-1), dict(M=0), dict(M=65536), dict(nrhs=0), dict(ts=None), dict(out=None),
               dict(words=None), dict(hsource=4), dict(hsource=-1), dict(hterm=None), dict(obs=0), dict(obs=9),
               dict(hsource=_hip.H_TABLE, entries=4), dict(hsource=_hip.H_TABLE, rows=p, entries=0),
               dict(hsource=_hip.H_TABLE, rows=p, entries=257)):
        assert pert(**kw) == 1, kw
        assert b"cgps_leg_perturbation_models" in lib.cgps_last_error()
    assert pert(d=0) == 3 and pert(d=9) == 3 and pert(dtype=7) == 3

    def repl(z=p, B=1, R=4, M=2, d=3, obs=2, dtype=_hip.F64, nrhs=2, x=p, words=p, Bmat=p):
        return lib.cgps_leg_observations(z, None, None, p, p, B, R, M, Bmat, p, d, obs, dtype, nrhs, 1, words, x, p, None)

    assert repl(B=0) == 0 and repl(R=0) == 0
    for kw in (dict(B=-1), dict(R=-1), dict(M=0), dict(M=65536), dict(nrhs=0), dict(z=None), dict(x=None), dict(words=None),
               dict(Bmat=None)):
        assert repl(**kw) == 1, kw
        assert b"cgps_leg_observations" in lib.cgps_last_error()
    assert repl(d=0) == 3 and repl(d=9) == 3 and repl(obs=0) == 3 and repl(obs=9) == 3 and repl(dtype=7) == 3

"""Sample paths and replicated observations under many LEG models (leg.posterior_perturbation_models,
leg.sample_from_posterior_models, leg.sample_from_prior_models, leg.sample_observations_batch / _models: DESIGN.md
4.21): slot k against the one-model batched call (bitwise on the right-hand sides) and against the float64
restatements (tests/_perturbref.py, tests/_replicateref.py); chunks of whole models; position independence of the
replicates; fp32; the joint distribution of draws and replicates; errors and edges.

The shapes are those of tests/test_sample_batch.py (its builders are imported, not copied): ragged [1, 2, 7, 33, 64, 65]
and dense [3, 33], ids [5, 0, 2^24 - 1, 7, 123456, 3], the four modes with NaN at unobserved entries; three models from
_missref.leg_case.  fp64 bound: LEG_TOL (rtol 1e-7, atol 1e-9), the project's bound for a sweep through a LEG factor."""
import functools
import os

import numpy as np
import pytest
import torch

import _perturbref as pr
import _replicateref as rr
import _rngref
import _util
import test_sample_batch as sb
from cyclic_gps import leg
import cyclic_gps.cyclic_reduction as cr

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
LEG_TOL, LENGTHS, IDS, MODES, SMAX = sb.LEG_TOL, sb.LENGTHS, sb.IDS, sb.MODES, sb.SMAX
M = 3
GIVEN_WORDS = [7, 7, 2]
R = sum(LENGTHS)
_np = sb._np


def _models(d, obs, dtype=F64):
    """Three models of _missref.leg_case (the first is test_sample_batch's): ([LEGMatrices on the GPU], [their fp64 CPU
    matrices])."""
    both = [sb._model(d, obs, seed, dtype) for seed in (70 + d, 170 + d, 270 + d)]
    return [m for m, _ in both], [mats for _, mats in both]


@functools.lru_cache(maxsize=None)
def _case(d):
    obs, _, _, series, dense = sb._case(d)
    ms, mats = _models(d, obs)
    return obs, ms, mats, series, dense


@functools.lru_cache(maxsize=None)
def _refs(d, mode, words, ids, S=SMAX, prior=False):
    """Per model the restated definition's (rhs, x) of the ragged batch, computed once and shared: [M] of ([R, d, S],
    [R, d, S])."""
    _, _, mats, series, _ = _case(d)
    out = []
    for k in range(M):
        ref = sb._ref(mats[k], series, mode, ids, S, 100 + d, stream=words[k], prior=prior)
        out.append((sb._cat(ref, 0), sb._cat(ref, 1)))
    return out


def _words(given):
    return tuple(GIVEN_WORDS) if given else (0, 4, 8)


# ---- 1. slot equality --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 5, 8])
def test_slot_k_is_the_batch_call_fp64(d):
    """Default words 0, 4, 8 with the default ids and model_streams=[7, 7, 2] with the given ids; S in {1, 3, 9}; the four
    modes: the right-hand sides of slot k are the one-model call's bit for bit, the draws within LEG_TOL of it and of
    the definition.  Then the dense layout."""
    obs, ms, mats, series, dense = _case(d)
    seed = 100 + d
    for mode in MODES:
        ts, xs, kw = sb._ragged(series, F64, mode)
        for given in (False, True):
            w, ids = _words(given), (IDS if given else None)
            refs = _refs(d, mode, w, tuple(ids or range(len(series))))
            args = dict(kw, series_ids=ids, model_streams=GIVEN_WORDS if given else None)
            for S in (1, 3, 9):
                rhs = leg.posterior_perturbation_models(ms, ts, xs, S, seed, **args)
                x = leg.sample_from_posterior_models(ms, ts, xs, S, seed, **args)
                assert rhs.shape == x.shape == (M, R, d, S) and x.dtype == F64 and x.is_cuda and not x.requires_grad
                for k in range(M):
                    what = "d=%d %s words=%s S=%d model %d" % (d, mode, w, S, k)
                    one = dict(kw, series_ids=ids, stream=w[k])
                    assert torch.equal(rhs[k], leg.posterior_perturbation_batch(ms[k], ts, xs, S, seed, **one)), what
                    xb = leg.sample_from_posterior_batch(ms[k], ts, xs, S, seed, **one)
                    np.testing.assert_allclose(_np(x[k]), _np(xb), err_msg=what + " against the batch call", **LEG_TOL)
                    np.testing.assert_allclose(_np(rhs[k]), refs[k][0][:, :, :S], err_msg=what + " rhs", **LEG_TOL)
                    np.testing.assert_allclose(_np(x[k]), refs[k][1][:, :, :S], err_msg=what + " draws", **LEG_TOL)
        # the dense layout, another first word
        st = lambda j, dt: torch.stack([sr[j] for sr in dense]).to(dt).cuda()          # noqa: E731
        ob, nv = sb._mode(mode, st(2, torch.bool), st(3, F64))
        x = leg.sample_from_posterior_models(ms, st(0, F64), st(1, F64), SMAX, seed, observed=ob, noise_var=nv, stream=3)
        rhs = leg.posterior_perturbation_models(ms, st(0, F64), st(1, F64), SMAX, seed, observed=ob, noise_var=nv, stream=3)
        assert x.shape == rhs.shape == (M, 3, 33, d, SMAX)
        for k in range(M):
            ref = sb._ref(mats[k], dense, mode, range(3), SMAX, seed, stream=3 + 4 * k)
            np.testing.assert_allclose(_np(x[k]), np.stack([r[1] for r in ref]), err_msg="dense %s model %d" % (mode, k), **LEG_TOL)
            one = leg.posterior_perturbation_batch(ms[k], st(0, F64), st(1, F64), SMAX, seed, observed=ob, noise_var=nv, stream=3 + 4 * k)
            assert torch.equal(rhs[k], one)


def test_slot_k_across_the_column_chunk_fp64():
    """S = 33 crosses the perturbation kernel's 32-column chunk and a solve panel."""
    d, S, seed, mode = 3, 33, 103, "both"
    obs, ms, mats, series, _ = _case(d)
    ts, xs, kw = sb._ragged(series, F64, mode)
    rhs = leg.posterior_perturbation_models(ms, ts, xs, S, seed, series_ids=IDS, **kw)
    x = leg.sample_from_posterior_models(ms, ts, xs, S, seed, series_ids=IDS, **kw)
    refs = _refs(d, mode, _words(False), tuple(IDS), S)
    for k in range(M):
        one = dict(kw, series_ids=IDS, stream=4 * k)
        assert torch.equal(rhs[k], leg.posterior_perturbation_batch(ms[k], ts, xs, S, seed, **one))
        np.testing.assert_allclose(_np(x[k]), _np(leg.sample_from_posterior_batch(ms[k], ts, xs, S, seed, **one)), **LEG_TOL)
        np.testing.assert_allclose(_np(x[k]), refs[k][1], **LEG_TOL)
    assert torch.equal(rhs[:, :, :, :9], leg.posterior_perturbation_models(ms, ts, xs, 9, seed, series_ids=IDS, **kw))


@pytest.mark.parametrize("d,dtype", [(1, F64), (5, F64), (4, F32)], ids=["d1-f64", "d5-f64", "d4-f32"])
def test_perturbation_wrapper_without_a_model_axis_is_its_one_model_form(d, dtype):
    """``leg._perturbation_models`` with G [d, d] and an int stream word (cgps_leg_perturbation_seg) against G [1, d, d]
    and a device word (cgps_leg_perturbation_models), the three noise sources."""
    lengths, obs, S, seed, word = [1, 2, 5, 64, 65], 2, 3, 11, 6
    m = sb._model(d, obs, 370 + d, dtype)[0]
    gen = torch.Generator().manual_seed(d)
    n = sum(lengths)
    ts = torch.cat([torch.cumsum(0.5 + torch.rand(k, generator=gen, dtype=F64), 0) for k in lengths]).to(dtype).cuda()
    xs = torch.randn(n, obs, generator=gen, dtype=F64).to(dtype).cuda()
    ob = (torch.rand(n, obs, generator=gen) < 0.7).cuda()
    nv = torch.rand(n, obs, generator=gen, dtype=F64).to(dtype).cuda()
    plan = leg._cached_batch_plan(lengths, ts.device)
    ids = torch.arange(len(lengths), dtype=torch.int64, device=ts.device)
    words = torch.tensor([word], dtype=torch.int64).cuda()
    for observed, noise_var in ((None, None), (ob, None), (ob, nv)):
        G, _, _, _, v, hsource, hterm, pattern = leg._models_sampling_operands([m], ts, xs, observed, noise_var)
        one = leg._perturbation_models(ts, G[0], plan, ids, hsource, hterm[0], pattern, v[0], S, seed, word)
        assert one.shape == (n, d, S) and not bool(torch.isnan(one).any())
        assert torch.equal(one, leg._perturbation_models(ts, G, plan, ids, hsource, hterm, pattern, v, S, seed, words, 0))


@pytest.mark.parametrize("d", [1, 3, 5, 6, 8])
def test_prior_slot_k_is_the_batch_call_fp64(d):
    """d = 6 and d = 8 have no cgps_peg_precision_models in fp64: the assembly with a zero term takes its place."""
    obs, ms, mats, series, _ = _case(d) if d != 6 else (1,) + _models(6, 1) + (sb._series(1, LENGTHS, 506), None)
    ts, _, _ = sb._ragged(series, F64, "plain")
    seed = 100 + d
    for given in (False, True):
        w = _words(given)
        for S in (1, 3, 9):
            z = leg.sample_from_prior_models(ms, ts, S, seed, lengths=LENGTHS, series_ids=IDS, model_streams=GIVEN_WORDS if given else None)
            assert z.shape == (M, R, d, S) and not z.requires_grad
            for k in range(M):
                zb = leg.sample_from_prior_batch(ms[k], ts, S, seed, lengths=LENGTHS, series_ids=IDS, stream=w[k])
                np.testing.assert_allclose(_np(z[k]), _np(zb), err_msg="d=%d S=%d model %d" % (d, S, k), **LEG_TOL)
                if S == 9:
                    ref = sb._ref(mats[k], series, "plain", IDS, S, seed, stream=w[k], prior=True)
                    np.testing.assert_allclose(_np(z[k]), sb._cat(ref, 1), err_msg="d=%d model %d" % (d, k), **LEG_TOL)
    t6 = torch.sort(ts[:6])[0]
    zd = leg.sample_from_prior_models(ms, t6.reshape(2, 3), 3, seed)                # dense: ids 0 and 1
    assert zd.shape == (M, 2, 3, d, 3)
    np.testing.assert_allclose(_np(zd.reshape(M, 6, d, 3)), _np(leg.sample_from_prior_models(ms, t6, 3, seed, lengths=[3, 3])), **LEG_TOL)


def test_equal_words_are_common_random_numbers():
    d = 3
    obs, ms, _, series, _ = _case(d)
    ts, xs, kw = sb._ragged(series, F64, "both")
    twins = [ms[1], ms[1]]
    same = leg.posterior_perturbation_models(twins, ts, xs, 5, 9, model_streams=[6, 6], **kw)
    assert torch.equal(same[0], same[1])
    apart = leg.posterior_perturbation_models(twins, ts, xs, 5, 9, **kw)                 # words 0 and 4
    assert bool((apart[0] != apart[1]).reshape(R, -1).any(dim=1).all())
    pz = leg.sample_from_prior_models(twins, ts, 5, 9, lengths=LENGTHS, model_streams=torch.tensor([6, 6]))
    np.testing.assert_allclose(_np(pz[0]), _np(pz[1]), **LEG_TOL)       # (draws: the two slots sit at other rows of the factor)
    pa = leg.sample_from_prior_models(twins, ts, 5, 9, lengths=LENGTHS)
    assert bool((pa[0] != pa[1]).reshape(R, -1).any(dim=1).all())


# ---- 2. chunks of whole models -----------------------------------------------------------------------------------
def test_chunks_of_whole_models(monkeypatch):
    d = 3
    obs, ms, _, series, _ = _case(d)
    ts, xs, kw = sb._ragged(series, F64, "both")
    whole = (leg.posterior_perturbation_models(ms, ts, xs, 9, 5, series_ids=IDS, **kw),
             leg.sample_from_posterior_models(ms, ts, xs, 9, 5, series_ids=IDS, **kw),
             leg.sample_from_prior_models(ms, ts, 9, 5, lengths=LENGTHS, series_ids=IDS))
    seen, real = [], leg._perturbation_models
    monkeypatch.setattr(leg, "_perturbation_models", lambda ts_, G_, *a, **k: (seen.append(G_.shape[0]), real(ts_, G_, *a, **k))[1])
    monkeypatch.setattr(leg, "MODELS_POSTERIOR_MAX_ROWS", R)                         # one model's rows
    parts = (leg.posterior_perturbation_models(ms, ts, xs, 9, 5, series_ids=IDS, **kw),
             leg.sample_from_posterior_models(ms, ts, xs, 9, 5, series_ids=IDS, **kw),
             leg.sample_from_prior_models(ms, ts, 9, 5, lengths=LENGTHS, series_ids=IDS))
    assert seen == [1] * (3 * M)
    assert torch.equal(parts[0], whole[0])
    np.testing.assert_allclose(_np(parts[1]), _np(whole[1]), **LEG_TOL)
    np.testing.assert_allclose(_np(parts[2]), _np(whole[2]), **LEG_TOL)
    monkeypatch.setattr(leg, "MODELS_POSTERIOR_MAX_ROWS", 2 * R + 1)                 # two models, then one
    del seen[:]
    assert torch.equal(leg.posterior_perturbation_models(ms, ts, xs, 9, 5, series_ids=IDS, **kw), whole[0]) and seen == [2, 1]


# ---- 3. replicated observations ----------------------------------------------------------------------------------
def _replicate_ref(mats, series, mode, ids, z, seed, words, dtype=np.float64):
    """[M, R, obs, S] of the restated definition: z [M, R, d, S] numpy float64, mats the matrices the kernel was given."""
    out = []
    for k, mk in enumerate(mats):
        _, Bm, LLT = rr.model(*(_np(t) for t in mk))
        parts, s0 = [], 0
        for (ts, _, mask, s), sid in zip(series, ids):
            n = ts.shape[0]
            ob, nv = sb._mode(mode, _np(mask), _np(s))
            parts.append(rr.replicates(Bm, LLT, z[k, s0:s0 + n], sid, seed, words[k], ob, nv, dtype))
            s0 += n
        out.append(np.concatenate(parts))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def _replicate_case(d, obs):
    if obs == 1 + d % 3:
        _, ms, mats, series, _ = _case(d)
    else:
        ms, mats = _models(d, obs)
        series = sb._series(obs, LENGTHS, 700 + obs)
    z = torch.randn(M, R, d, 33, dtype=F64, generator=torch.Generator().manual_seed(40 + d)).cuda()
    return ms, mats, series, z


@pytest.mark.parametrize("d,obs", [(1, 2), (3, 1), (5, 3), (8, 3), (3, 8), (3, 4), (3, 5), (8, 6), (3, 7), (8, 4)])
def test_replicates_against_the_definition_fp64(d, obs):
    """M = 3 (default words and [7, 7, 2]) and M = 1; the four modes; S in {1, 3, 9} and 33 (the column-chunk edge)."""
    ms, mats, series, z = _replicate_case(d, obs)
    seed = 300 + d
    for mode in MODES:
        _, _, kw = sb._ragged(series, F64, mode)
        for given in (False, True):
            w, ids = _words(given), (IDS if given else None)
            ref = _replicate_ref(mats, series, mode, ids or range(len(series)), _np(z), seed, w)
            for S in (1, 3, 9, 33):
                x = leg.sample_observations_models(ms, z[..., :S].contiguous(), seed, series_ids=ids,
                                                   model_streams=GIVEN_WORDS if given else None, **kw)
                assert x.shape == (M, R, obs, S) and x.dtype == F64 and x.is_cuda
                np.testing.assert_allclose(_np(x), ref[..., :S], err_msg="d=%d obs=%d %s S=%d" % (d, obs, mode, S), **LEG_TOL)
                for k in range(M):                                             # M = 1: the batch call, and slot k of the models call
                    one = leg.sample_observations_batch(ms[k], z[k, :, :, :S], seed, series_ids=ids, stream=w[k], **kw)
                    assert one.shape == (R, obs, S) and torch.equal(one, x[k]), (mode, S, k)
    # dense layout
    zd = z[:, :99, :, :3].reshape(M, 3, 33, d, 3)
    xd = leg.sample_observations_models(ms, zd, seed)
    xr = leg.sample_observations_models(ms, zd.reshape(M, 99, d, 3), seed, lengths=[33, 33, 33])
    assert xd.shape == (M, 3, 33, obs, 3) and torch.equal(xd.reshape(M, 99, obs, 3), xr)
    assert leg.sample_observations_batch(ms[0], zd[0], seed).shape == (3, 33, obs, 3)


@pytest.mark.parametrize("mode", MODES)
def test_a_series_replicate_does_not_depend_on_its_batch(mode):
    d, obs = 5, 3
    ms, _, series, z = _replicate_case(d, obs)
    seed, S = 11, 9
    z = z[..., :S].contiguous()
    _, _, kw = sb._ragged(series, F64, mode)
    x = leg.sample_observations_models(ms, z, seed, series_ids=IDS, **kw)
    starts = np.concatenate([[0], np.cumsum(LENGTHS)])
    for j, sid in enumerate(IDS):                                           # alone, under its own id
        _, _, kw1 = sb._ragged([series[j]], F64, mode)
        alone = leg.sample_observations_models(ms, z[:, starts[j]:starts[j + 1]].contiguous(), seed, series_ids=[sid], **kw1)
        assert torch.equal(alone, x[:, starts[j]:starts[j + 1]]), (mode, j)
    order = [4, 0, 5, 2, 1, 3]                                              # the batch reordered
    _, _, kwp = sb._ragged(series, F64, mode, order)
    zp = torch.cat([z[:, starts[b]:starts[b + 1]] for b in order], dim=1)
    perm = leg.sample_observations_models(ms, zp, seed, series_ids=[IDS[b] for b in order], **kwp)
    s0 = 0
    for b in order:
        assert torch.equal(perm[:, s0:s0 + LENGTHS[b]], x[:, starts[b]:starts[b + 1]]), (mode, b)
        s0 += LENGTHS[b]
    assert torch.equal(leg.sample_observations_models(ms, z[..., :3].contiguous(), seed, series_ids=IDS, **kw), x[..., :3])
    # the words: another seed, another stream or another id moves every row
    for other in (leg.sample_observations_models(ms, z, seed + 1, series_ids=IDS, **kw),
                  leg.sample_observations_models(ms, z, seed, series_ids=IDS, stream=1, **kw),
                  leg.sample_observations_models(ms, z, seed, series_ids=[(k + 1) % (1 << 24) for k in IDS], **kw)):
        assert bool((other != x).reshape(M * R, -1).any(dim=1).all())


def test_observations_of_the_models_call_are_the_replicates_on_the_same_words():
    d = 3
    obs, ms, _, series, _ = _case(d)
    ts, xs, kw = sb._ragged(series, F64, "both")
    z, x = leg.sample_from_posterior_models(ms, ts, xs, 5, 21, series_ids=IDS, model_streams=GIVEN_WORDS, observations=True, **kw)
    assert torch.equal(z, leg.sample_from_posterior_models(ms, ts, xs, 5, 21, series_ids=IDS, model_streams=GIVEN_WORDS, **kw))
    assert x.shape == (M, R, obs, 5)
    assert torch.equal(x, leg.sample_observations_models(ms, z, 21, series_ids=IDS, model_streams=GIVEN_WORDS, **kw))


# ---- 4. fp32 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 5, 8])
def test_draws_fp32_are_as_accurate_as_the_one_series_sampler(d):
    """The rule of test_sample_batch's test of the same name with the models call in place of the batch call: slot k's
    largest error against the definition (relative to max |x|) is at most four times that of the one-series fp32
    sampler under model k against its own fp64 reference on the same series.
    Measured on an MI355X, largest relative error over the four modes and three models, one-series sampler / models
    call: d = 1: 1.78e-6 / 1.28e-6;  d = 3: 2.14e-6 / 2.82e-6;  d = 5: 2.01e-6 / 2.84e-6;  d = 8: 5.41e-6 / 1.29e-5;
    the largest ratio within one mode and model is 2.38 (d = 8, plain, model 1: 5.41e-6 / 1.29e-5) of the 4 allowed."""
    obs, _, mats, series, _ = _case(d)
    ms32, _ = _models(d, obs, F32)
    S, seed = 8, 200 + d
    for mode in MODES:
        ts, xs, kw = sb._ragged(series, F32, mode)
        x = leg.sample_from_posterior_models(ms32, ts, xs, S, seed, model_streams=[0, 0, 0], **kw)
        assert x.dtype == F32 and x.shape == (M, R, d, S)
        for k in range(M):
            e_loop, s_loop = sb._loop_error_fp32(ms32[k], mats[k], series, mode, S, seed)
            ref = sb._cat(sb._ref(mats[k], series, mode, range(len(series)), S, seed, dtype=np.float32), 1)
            e_models, s_models = float(np.abs(_np(x[k]).astype(np.float64) - ref).max()), float(np.abs(ref).max())
            print("d=%d %s model %d: loop %.3e (relative %.3e), models %.3e (relative %.3e)"
                  % (d, mode, k, e_loop, e_loop / s_loop, e_models, e_models / s_models))
            assert e_models / s_models <= 4 * e_loop / s_loop, (mode, k, e_models / s_models, e_loop / s_loop)


@pytest.mark.parametrize("d,obs", [(1, 2), (3, 1), (5, 3), (8, 3), (3, 8), (3, 4), (3, 5), (8, 6), (3, 7), (8, 4)])
def test_replicates_fp32_are_as_accurate_as_the_torch_composition(d, obs):
    """fp32, S in {1, 3, 9, 65} (65 crosses the 64-column chunk): the kernel's largest error against the float64
    reference on the same fp32 inputs, relative to max |x|, is at most four times the error of the same formula as fp32
    torch ops (B z + cholesky(LLT + diag(s mask)) eps'', LLT formed in fp32 as the library forms it).
    Measured on an MI355X, largest relative error over the four modes and the column counts, kernel / torch ops:
    (d, obs) = (1, 2): 1.06e-7 / 1.02e-7;  (3, 1): 9.93e-8 / 1.01e-7;  (5, 3): 1.27e-7 / 1.10e-7;
    (8, 3): 1.36e-7 / 1.03e-7;  (3, 8): 1.71e-7 / 1.01e-7; the largest ratio within one mode is 2.19 ((3, 8), noise:
    1.71e-7 / 7.80e-8) of the 4 allowed."""
    _, mats, series, z64 = _replicate_case(d, obs)
    ms32, _ = _models(d, obs, F32)
    mats32 = [tuple(t.float().double() for t in mk) for mk in mats]              # what the kernel is given, exactly
    S, seed = 65, 400 + d
    z = torch.randn(M, R, d, S, dtype=F32, generator=torch.Generator().manual_seed(60 + d))
    w = _words(False)
    for mode in MODES:
        _, _, kw = sb._ragged(series, F32, mode)
        ref = _replicate_ref(mats32, series, mode, range(len(series)), z.double().numpy(), seed, w, np.float32)
        scale = float(np.abs(ref).max())
        # the same formula in fp32 torch ops on the CPU
        comp = []
        for k, mk in enumerate(mats):
            Bm, Lm = mk[2].float(), mk[3].float()
            LLT = Lm @ Lm.T + 1e-9 * torch.eye(obs)
            parts, s0 = [], 0
            for b, (t1, _, mask, s) in enumerate(series):
                n = t1.shape[0]
                ob, nv = sb._mode(mode, mask, s)
                sv = torch.from_numpy(rr.row_variances(n, obs, None if ob is None else _np(ob), None if nv is None else _np(nv))).float()
                T = torch.linalg.cholesky(LLT + torch.diag_embed(sv))
                eps = torch.from_numpy(rr.noise(n, obs, b, S, seed, w[k], np.float32)).float()
                parts.append(Bm @ z[k, s0:s0 + n] + T @ eps)
                s0 += n
            comp.append(torch.cat(parts))
        e_torch = float(np.abs(torch.stack(comp).double().numpy() - ref).max()) / scale
        for Sc in (1, 3, 9, 65):
            x = leg.sample_observations_models(ms32, z[..., :Sc].contiguous().cuda(), seed, **kw)
            assert x.dtype == F32 and x.shape == (M, R, obs, Sc)
            e_kernel = float(np.abs(_np(x).astype(np.float64) - ref[..., :Sc]).max()) / scale
            print("d=%d obs=%d %s S=%d: kernel %.3e, torch fp32 composition %.3e (relative to max |x|)"
                  % (d, obs, mode, Sc, e_kernel, e_torch))
            assert e_kernel <= 4 * e_torch, (mode, Sc, e_kernel, e_torch)


# ---- 5. distribution ---------------------------------------------------------------------------------------------
def _golden_models():
    g = np.load(os.path.join(_util.GOLDEN, "leg_small_irregular.npz"))
    first = [g[k] for k in ("N", "R", "B", "Lambda")]
    rng = np.random.default_rng(3)
    second = [a + 0.3 * rng.standard_normal(a.shape) for a in first]             # N, R, B, Lambda in that order
    mats = [tuple(torch.from_numpy(a) for a in mk) for mk in (first, second)]
    lengths = [1, 4, 7]
    torch.manual_seed(1)
    series, s0 = [], 0
    for n in lengths:
        mask = torch.rand(n, 2) > 0.3
        var = 0.5 * torch.rand(n, 2, dtype=F64)
        series.append((torch.from_numpy(g["ts"][s0:s0 + n]), torch.from_numpy(g["xs"][s0:s0 + n]), mask, var))
        s0 += n
    return [leg.LEGMatrices(*(t.cuda() for t in mk)) for mk in mats], mats, lengths, series


def test_distribution_of_draws_and_replicates():
    """4096 joint draws (z, x_rep) under two models, seed 2024, default ids and words 0 and 4, mask and variances on.
    Every statistic within six standard errors (Var of a product of two jointly normal variables: C_ii C_jj + C_ij^2):
    the latent covariance and mean against dense K^-1 and K^-1 v; the replicate covariance against
    B~ C B~^T + blockdiag(LLT + diag(s mask)) and its mean against B~ K^-1 v; the cross-covariance of x_rep - B z with
    the latent draw against zero; the cross-covariance of model 0's and model 1's draws of each series against zero.
    The reference alone stays within 1.48-2.81, 0.42-2.71, 1.96-2.89, 0.40-2.59, 1.98-3.46 and 2.37-2.84 of the 6."""
    ms, mats, lengths, series = _golden_models()
    S = 4096
    ts, xs, kw = sb._ragged(series, F64, "both")
    z, x = leg.sample_from_posterior_models(ms, ts, xs, S, 2024, observations=True, **kw)
    z, x = z.cpu(), x.cpu()
    dev = [[], []]
    for k in range(2):
        G, Bm, LLT = pr.model(*(_np(t) for t in mats[k]))
        s0 = 0
        for b, (n, (t1, x1, mask, var)) in enumerate(zip(lengths, series)):
            terms = pr.series_terms(G, Bm, LLT, _np(t1), _np(mask), _np(var))
            C = torch.from_numpy(np.linalg.inv(pr.dense_K(terms)))
            mu = C @ torch.from_numpy(pr.rhs_v(terms, Bm, _np(x1))).reshape(-1)
            Z = z[k, s0:s0 + n].reshape(n * 3, S)
            D = Z - mu[:, None]
            dg = torch.diagonal(C)
            cov = float(((D @ D.T / S - C).abs() / torch.sqrt((dg[:, None] * dg[None, :] + C * C) / S)).max())
            mean = float(((Z.mean(1) - mu).abs() / torch.sqrt(dg / S)).max())
            # the replicate
            Bt = torch.kron(torch.eye(n, dtype=F64), torch.from_numpy(Bm))
            sv = rr.row_variances(n, 2, _np(mask), _np(var))
            Nn = torch.block_diag(*[torch.from_numpy(LLT + np.diag(sv[r])) for r in range(n)])
            Cx, mux = Bt @ C @ Bt.T + Nn, Bt @ mu
            X = x[k, s0:s0 + n].reshape(n * 2, S)
            Dx = X - mux[:, None]
            dx = torch.diagonal(Cx)
            rcov = float(((Dx @ Dx.T / S - Cx).abs() / torch.sqrt((dx[:, None] * dx[None, :] + Cx * Cx) / S)).max())
            rmean = float(((X.mean(1) - mux).abs() / torch.sqrt(dx / S)).max())
            E = X - Bt @ Z                                           # the replicate's noise: independent of the path
            cross = float(((E @ D.T / S).abs() / torch.sqrt(torch.diagonal(Nn)[:, None] * dg[None, :] / S)).max())
            print("model %d series %d: latent covariance %.2f, mean %.2f; replicate covariance %.2f, mean %.2f; noise x latent "
                  "%.2f standard errors (bound 6)" % (k, b, cov, mean, rcov, rmean, cross))
            assert max(cov, mean, rcov, rmean, cross) <= 6.0, (k, b, cov, mean, rcov, rmean, cross)
            dev[k].append((D, dg))
            s0 += n
    for b in range(len(lengths)):
        (D0, g0), (D1, g1) = dev[0][b], dev[1][b]
        between = float(((D0 @ D1.T / S).abs() / torch.sqrt(g0[:, None] * g1[None, :] / S)).max())
        print("series %d: model 0 x model 1 %.2f standard errors (bound 6)" % (b, between))
        assert between <= 6.0, (b, between)


# ---- 6. errors and edges -----------------------------------------------------------------------------------------
def test_errors_come_before_anything_runs_and_edges(monkeypatch):
    d = 3
    obs, ms, mats, series, _ = _case(d)
    ts, xs, kw = sb._ragged(series, F64, "both")
    post, prior, repl = leg.sample_from_posterior_models, leg.sample_from_prior_models, leg.sample_observations_models
    # B = 0 in both layouts: empty tensors with leading M
    assert post(ms, ts[:0], xs[:0], 4, 1, lengths=[]).shape == (M, 0, d, 4)
    assert post(ms, ts[:0].reshape(0, 5), xs[:0].reshape(0, 5, obs), 4, 1).shape == (M, 0, 5, d, 4)
    assert leg.posterior_perturbation_models(ms, ts[:0], xs[:0], 4, 1, lengths=[]).shape == (M, 0, d, 4)
    assert prior(ms, ts[:0], 4, 1, lengths=[]).shape == (M, 0, d, 4)
    assert prior(ms, ts[:0].reshape(0, 5), 4, 1).shape == (M, 0, 5, d, 4)
    z0 = torch.zeros(M, 0, d, 4, dtype=F64, device="cuda")
    assert repl(ms, z0, 1, lengths=[]).shape == (M, 0, obs, 4) and repl(ms, z0.reshape(M, 0, 5, d, 4), 1).shape == (M, 0, 5, obs, 4)
    assert leg.sample_observations_batch(ms[0], z0[0], 1, lengths=[]).shape == (0, obs, 4)
    zero = post(ms, ts[:0], xs[:0], 4, 1, lengths=[], observations=True)
    assert zero[0].shape == (M, 0, d, 4) and zero[1].shape == (M, 0, obs, 4)
    # ValueErrors, before any launch: with the kernels' bindings taken away nothing could have been launched
    other_rank, _ = sb._model(d + 1, obs, 1)
    z = torch.zeros(M, R, d, 4, dtype=F64, device="cuda")
    bad = [lambda: post([], ts, xs, 4, 1, **kw),
           lambda: post([ms[0], other_rank], ts, xs, 4, 1, **kw),
           lambda: post(ms, ts, xs, 4, 1, model_streams=[0, 4], **kw),
           lambda: post(ms, ts, xs, 4, 1, model_streams=[0, 4, (1 << 32) - 3], **kw),
           lambda: post(ms, ts, xs, 4, 1, model_streams=[0, -1, 4], **kw),
           lambda: post(ms, ts, xs, 4, 1, stream=(1 << 32) - 11, **kw),         # the default words leave the range at model 2
           lambda: post(ms, ts, xs, 0, 1, **kw),
           lambda: post(ms, ts, xs, 4, 1, series_ids=IDS[:-1], **kw),
           lambda: post(ms, ts, xs, 4, 1, series_ids=IDS[:-1] + [1 << 24], **kw),
           lambda: leg.posterior_perturbation_models(ms, ts, xs, 4, 1, series_ids=IDS[:-1] + [-1], **kw),
           lambda: post(ms, ts, xs, 4, 1, lengths=LENGTHS, observed=kw["observed"][:-1]),
           lambda: prior([], ts, 4, 1, lengths=LENGTHS),
           lambda: prior(ms, ts, 4, 1, lengths=LENGTHS, model_streams=[1]),
           lambda: prior(ms, ts, 0, 1, lengths=LENGTHS),
           lambda: prior(ms, ts, 4, 1, lengths=LENGTHS, series_ids=[0]),
           lambda: repl([], z, 1, lengths=LENGTHS),
           lambda: repl(ms, z[:2], 1, lengths=LENGTHS),
           lambda: repl(ms, z[:, :, :2], 1, lengths=LENGTHS),
           lambda: repl(ms, z, 1, lengths=LENGTHS[:-1]),
           lambda: repl(ms, z, 1, lengths=LENGTHS, model_streams=[0, 1 << 32, 4]),
           lambda: repl(ms, z, 1, lengths=LENGTHS, series_ids=[1 << 24] * 6),
           lambda: repl(ms, z, 1, lengths=LENGTHS, observed=kw["observed"][:-1]),
           lambda: repl(ms, z, 1, lengths=LENGTHS, noise_var=torch.ones(R, obs + 1, dtype=F64, device="cuda")),
           lambda: leg.sample_observations_batch(ms[0], z, 1, lengths=LENGTHS),
           lambda: leg.sample_observations_batch(ms[0], z[0], 1, lengths=LENGTHS, stream=(1 << 32) - 3)]
    with monkeypatch.context() as mp:
        launched = []
        for name in ("_perturbation_models", "_posterior_blocks_models", "_peg_precision_models", "_observations_rows"):
            mp.setattr(leg, name, lambda *a, **k: launched.append(1))
        for k, call in enumerate(bad):
            with pytest.raises(ValueError):
                call()
                pytest.fail("case %d did not raise" % k)
        assert not launched
    # a zero-length gap inside series 2 belongs to the data: every model meets it and the first of the call is named,
    # also when the chunks hold one model each
    assert cr.CHECK_POSITIVE_DEFINITE
    start = sum(LENGTHS[:2])
    tz = ts.clone()
    tz[start + 4] = tz[start + 3]
    for rows in (leg.MODELS_POSTERIOR_MAX_ROWS, R):
        monkeypatch.setattr(leg, "MODELS_POSTERIOR_MAX_ROWS", rows)
        for call in (lambda: post(ms, tz, xs, 2, 1, **kw), lambda: prior(ms, tz, 2, 1, lengths=LENGTHS),
                     lambda: leg.posterior_perturbation_models(ms, tz, xs, 2, 1, **kw)):
            with pytest.raises(cr.NotPSDError, match=r"model 0.*series 2.*row 3"):
                call()
    # a failure of model 1 alone, one chunk boundary away (chunks of one model): a noise variance just below -LLT at one
    # row of series 2 makes that row's block of K negative definite for the middle model only
    lam = (1.0, 0.5, 1.5)
    m1, _ = _models(d, 1)
    m1 = [leg.LEGMatrices(m.N, m.R, m.B, torch.full((1, 1), v, dtype=F64, device="cuda")) for m, v in zip(m1, lam)]
    s1 = sb._series(1, LENGTHS, 83)
    t1, x1, kw1 = sb._ragged(s1, F64, "noise")
    nv = kw1["noise_var"].clone()
    llt = float(m1[1].LLT[0, 0])
    nv[start + 3] = -llt - float((m1[1].B ** 2).sum()) / 1e6
    with pytest.raises(cr.NotPSDError, match=r"model 1.*series 2.*row"):
        post(m1, t1, x1, 2, 1, lengths=LENGTHS, noise_var=nv)
    monkeypatch.setattr(leg, "MODELS_POSTERIOR_MAX_ROWS", 1 << 22)
    # NaN at unobserved entries of xs and noise_var (what _ragged puts there) reaches neither the draws nor the replicates
    assert bool(torch.isnan(xs).any()) and bool(torch.isnan(kw["noise_var"]).any())
    zz, xx = post(ms, ts, xs, 3, 1, observations=True, **kw)
    assert bool(torch.isfinite(zz).all()) and bool(torch.isfinite(xx).all())
    clean = dict(kw, noise_var=torch.nan_to_num(kw["noise_var"], nan=0.3))
    assert torch.equal(leg.posterior_perturbation_models(ms, ts, xs, 3, 1, **kw),
                       leg.posterior_perturbation_models(ms, ts, torch.nan_to_num(xs, nan=-2.0), 3, 1, **clean))
    assert torch.equal(xx, repl(ms, zz, 1, **clean))
    # a negative variance that makes a row's noise covariance indefinite is named by the replicates
    with pytest.raises(cr.NotPSDError, match=r"model 1.*series 2.*row 3"):
        repl(m1, torch.zeros(M, R, d, 2, dtype=F64, device="cuda"), 1, lengths=LENGTHS, noise_var=nv)


def test_cpu_tensors_run_on_the_gpu_and_come_back():
    d = 3
    obs, ms, _, series, _ = _case(d)
    ts, xs, kw = sb._ragged(series, F64, "observed")
    cpu_ms = [m.to("cpu") for m in ms]
    z, x = leg.sample_from_posterior_models(ms, ts, xs, 3, 4, observations=True, **kw)
    zc, xc = leg.sample_from_posterior_models(cpu_ms, ts.cpu(), xs.cpu(), 3, 4, lengths=LENGTHS, observed=kw["observed"].cpu(),
                                              observations=True)
    assert zc.device.type == xc.device.type == "cpu" and torch.equal(zc, z.cpu()) and torch.equal(xc, x.cpu())
    pc = leg.sample_from_prior_models(cpu_ms, ts.cpu(), 3, 4, lengths=LENGTHS)
    assert pc.device.type == "cpu" and torch.equal(pc, leg.sample_from_prior_models(ms, ts, 3, 4, lengths=LENGTHS).cpu())
    rc = leg.posterior_perturbation_models(cpu_ms, ts.cpu(), xs.cpu(), 3, 4, lengths=LENGTHS, observed=kw["observed"].cpu())
    assert rc.device.type == "cpu" and torch.equal(rc, leg.posterior_perturbation_models(ms, ts, xs, 3, 4, **kw).cpu())
    bc = leg.sample_observations_batch(cpu_ms[0], z[0].cpu(), 4, lengths=LENGTHS, observed=kw["observed"].cpu())
    assert bc.device.type == "cpu" and torch.equal(bc, x[0].cpu())

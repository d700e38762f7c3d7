"""The posterior and the predictions of many LEG models over one batch in one call (leg.insample_posterior_models,
predict.predictive_posterior_models, predict.make_predictions_models, predict.combine_predictions: DESIGN.md 4.18) and
their two kernels, cgps_leg_posterior_blocks_models and cgps_leg_intercast_models: the kernels bit for bit against their
one-model siblings, the calls against a loop of the ``*_batch`` calls over the models, against dense fp64 truths
(_missref, _noiseref) and against results recorded from the reference (tests/golden/leg_models_predictions.npz).
Symbols, argument checks, validation, empty batches and the mixture run without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _util
from cyclic_gps import _hip, leg, predict
from test_leg_intercast_seg import LENGTHS, _random_posterior, standard_batch, standard_targets
from test_leg_posterior_batch import MODES, SMALL, _dense_truth, _mode_args, _model, _ragged, _series, _split

F64, F32 = torch.float64, torch.float32
EPS32 = float(torch.finfo(F32).eps)
TOL = dict(rtol=1e-9, atol=1e-11)              # what test_leg_posterior_batch.py gives the batch against its loop
M = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _models(d, obs, seed, dtype=F64, device="cpu", count=M):
    """``count`` models of one rank and obs_dim (test_leg_posterior_batch._model with consecutive seeds) and their fp64 CPU
    matrices."""
    pairs = [_model(d, obs, seed + 11 * k, dtype, device) for k in range(count)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _poisoned(series, dtype, mode):
    """The ragged batch of ``_series`` on the GPU for a mode: (ts, xs, observed, noise_var); unobserved entries of xs and
    noise_var hold NaN."""
    ts, xs, mask, s = _ragged(series, dtype)
    ob, nv = _mode_args(mode, mask, s)
    if ob is not None:
        xs = torch.where(ob, xs, torch.full_like(xs, float("nan")))
        if nv is not None:
            nv = torch.where(ob, nv, torch.full_like(nv, float("nan")))
    return ts, xs, ob, nv


def _close(got, want, what):
    assert bool(torch.isfinite(got).all()), what
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), err_msg=what, **TOL)


# ---- without a GPU -------------------------------------------------------------------------------------------------
def test_both_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cgps.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in ("cgps_leg_posterior_blocks_models", "cgps_leg_intercast_models"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _hip.exported_symbols() and hasattr(raw, name), name
    assert _hip.lib().cgps_version() == 320


def test_blocks_models_entry_checks_its_arguments_before_any_launch():
    lib = _hip.lib()
    fn = lib.cgps_leg_posterior_blocks_models
    f = ctypes.c_void_p(4096)                                    # never dereferenced: every call below returns first

    def call(R=8, M=2, d=3, dtype=_hip.F64, source=_hip.ROWS_TABLE, entries=4, ts=f, G=f, cut=f, term=f, rows=f, K=f, Os=f, info=f):
        return fn(ts, G, cut, R, M, d, dtype, source, term, entries, rows, K, Os, info, None)

    assert call(ts=None) == 1 and b"cgps_leg_posterior_blocks_models" in lib.cgps_last_error()
    for hole in ("G", "term", "K", "Os", "info", "rows"):
        assert call(**{hole: None}) == 1, hole
    assert call(R=0) == 1
    assert call(M=0) == 1 and call(M=-1) == 1 and call(M=65536) == 1
    assert call(source=3) == 1 and call(source=-1) == 1
    assert call(entries=0) == 1 and call(entries=257) == 1
    assert call(source=_hip.ROWS_WEIGHTED, entries=0) == 1 and call(source=_hip.ROWS_WEIGHTED, entries=65) == 1
    assert call(source=_hip.ROWS_WEIGHTED, rows=None) == 1
    assert call(d=9) == 3 and call(d=0) in (1, 3) and call(dtype=7) == 3
    assert call(M=65535, d=9) == 3                               # (the largest M passes the check of M)
    assert call(source=_hip.ROWS_PLAIN, rows=None, entries=0, d=9) == 3    # (plain reads neither; a null cut is one series)
    assert call(source=_hip.ROWS_PLAIN, rows=None, entries=0, cut=None, d=9) == 3


def test_intercast_models_entry_checks_its_arguments_before_any_launch():
    lib = _hip.lib()
    fn = lib.cgps_leg_intercast_models
    fake = ctypes.c_void_p(4096)                                 # never dereferenced: every call below returns first

    def call(B, P, M=2, d=3, dtype=_hip.F64, ptrs=None):
        p = ptrs if ptrs is not None else [fake] * 10
        return fn(p[0], p[1], p[2], p[3], B, P, M, p[4], d, dtype, p[5], p[6], p[7], p[8], p[9], None)

    assert call(-1, 4) == 1 and b"cgps_leg_intercast_models" in lib.cgps_last_error()
    assert call(2, -1) == 1
    assert call(2, 4, M=0) == 1 and call(2, 4, M=65536) == 1 and call(0, 0, M=0) == 1
    assert call(2, 4, ptrs=[None] * 10) == 1
    for hole in (0, 1, 2, 3, 4, 5, 6, 8, 9):                    # (7, the off-diagonal blocks, may be null)
        ptrs = [fake] * 10
        ptrs[hole] = None
        assert call(2, 4, ptrs=ptrs) == 1, hole
    assert call(0, 4, ptrs=[None] * 10) == 0                     # nothing to do: OK without touching the runtime
    assert call(2, 0, ptrs=[None] * 10) == 0
    assert call(0, 0, ptrs=[None] * 10) == 0
    assert call(2, 4, d=0) == 3 and call(2, 4, d=9) == 3
    assert call(2, 4, dtype=7) == 3
    assert call(2, 4, M=65535, d=9) == 3


def _cpu_case(B=3, n=4, obs=2, d=3):
    ms, _ = _models(d, obs, 5)
    ts = torch.cumsum(torch.ones(B, n, dtype=F64), 1)
    return ms, ts, torch.zeros(B, n, obs, dtype=F64)


def test_validation_errors_come_before_anything_runs():
    ms, ts, xs = _cpu_case()
    B, n, obs = xs.shape
    tsr, xsr, lens = ts.reshape(-1), xs.reshape(B * n, obs), [n] * B
    tt = torch.tensor([0.5, 1.5], dtype=F64)
    other_rank, _ = _models(2, obs, 5, count=1)
    other_dtype, _ = _models(3, obs, 5, dtype=F32, count=1)
    post, pp, mp = leg.insample_posterior_models, predict.predictive_posterior_models, predict.make_predictions_models
    bad = [
        # the models
        lambda: post([], ts, xs),
        lambda: post(ms[:2] + other_rank, ts, xs),
        lambda: post(ms[:2] + other_dtype, ts, xs),
        lambda: post(ms[:2] + [None], ts, xs),
        lambda: pp([], ts, xs, tt),
        lambda: mp(ms[:1] + other_rank, ts, xs, tt),
        # layouts
        lambda: post(ms, ts, xsr),
        lambda: post(ms, ts[:, :3], xs),
        lambda: post(ms, ts, xs[..., :1]),                                  # the models have two channels
        lambda: post(ms, tsr, xsr, lengths=[n] * (B - 1)),                  # lengths do not sum to the rows
        lambda: post(ms, tsr, xsr, lengths=[n, n, n - 1, 1, 0]),            # an empty series
        lambda: post(ms, tsr, xsr, lengths=torch.tensor([4.0, 4.0, 4.0])),
        lambda: post(ms, ts, xsr, lengths=lens),
        # masks and variances of the wrong kind or shape
        lambda: post(ms, ts, xs, observed=torch.ones(B, n, obs)),
        lambda: post(ms, ts, xs, observed=torch.ones(B, n + 1, dtype=torch.bool)),
        lambda: post(ms, tsr, xsr, lengths=lens, observed=torch.ones(B, n, obs, dtype=torch.bool)),
        lambda: post(ms, ts, xs, noise_var=torch.ones(B, n, obs, dtype=torch.int64)),
        lambda: post(ms, ts, xs, noise_var=torch.ones(B, n, obs + 1, dtype=F64)),
        lambda: post(ms, tsr, xsr, lengths=lens, noise_var=torch.ones(B * n + 1, dtype=F64)),
        # targets
        lambda: pp(ms, ts, xs, torch.ones(B + 1, 2, dtype=F64)),
        lambda: pp(ms, ts, xs, torch.ones(B, 2, 2, dtype=F64)),
        lambda: pp(ms, ts, xs, tt, target_lengths=[2] * B),                 # target_lengths is the ragged layout's
        lambda: mp(ms, ts, xs, tt, target_lengths=[2] * B),
        lambda: pp(ms, ts, xs, torch.ones(2, dtype=torch.int64)),
        lambda: pp(ms, tsr, xsr, tt, lengths=lens),                         # ragged without target_lengths
        lambda: pp(ms, tsr, xsr, tt, lengths=lens, target_lengths=[1, 1]),
        lambda: pp(ms, tsr, xsr, tt, lengths=lens, target_lengths=[1, 1, 1]),
        lambda: pp(ms, tsr, xsr, tt, lengths=lens, target_lengths=[3, -1, 0]),
        lambda: mp(ms, tsr, xsr, tt, lengths=[n] * (B - 1), target_lengths=[2, 0]),
        lambda: mp(ms, ts, xs, tt, observed=torch.ones(B, n + 1, dtype=torch.bool)),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d raised nothing" % k)


def test_empty_batches_have_the_leading_model_dimension():
    ms, ts, xs = _cpu_case()
    d, obs, n = 3, 2, 4
    mean, (Sd, So) = leg.insample_posterior_models(ms, ts[:0], xs[:0])
    assert mean.shape == (M, 0, n, d) and Sd.shape == (M, 0, n, d, d) and So.shape == (M, 0, n - 1, d, d)
    mean, (Sd, So) = leg.insample_posterior_models(ms, ts.reshape(-1)[:0], xs.reshape(-1, obs)[:0], lengths=[])
    assert mean.shape == (M, 0, d) and Sd.shape == (M, 0, d, d) and So.shape == (M, 0, d, d) and mean.dtype == F64
    tt = torch.tensor([0.5, 1.5, 2.5], dtype=F64)
    for fn, w in ((predict.predictive_posterior_models, d), (predict.make_predictions_models, obs)):
        pm, pv = fn(ms, ts[:0], xs[:0], tt)
        assert pm.shape == (M, 0, 3, w) and pv.shape == (M, 0, 3, w, w)
        pm, pv = fn(ms, ts.reshape(-1)[:0], xs.reshape(-1, obs)[:0], tt[:0], lengths=[], target_lengths=[])
        assert pm.shape == (M, 0, w) and pv.shape == (M, 0, w, w)
        # series, but no target anywhere: nothing to launch either
        pm, pv = fn(ms, ts.reshape(-1), xs.reshape(-1, obs), tt[:0], lengths=[n] * 3, target_lengths=[0, 0, 0])
        assert pm.shape == (M, 0, w) and pv.shape == (M, 0, w, w) and pm.dtype == F64
        pm, pv = fn(ms, ts, xs, tt[:0])
        assert pm.shape == (M, 3, 0, w) and pv.shape == (M, 3, 0, w, w)


def test_combine_predictions_is_the_moment_matched_mixture():
    # two components in one dimension, by hand: w = (0.25, 0.75), means (1, 3), variances (0.5, 2)
    #   mean = 0.25 + 2.25 = 2.5;  second moment = 0.25 (0.5 + 1) + 0.75 (2 + 9) = 8.625;  variance = 8.625 - 6.25 = 2.375
    means = torch.tensor([[[1.0]], [[3.0]]], dtype=F64)
    covs = torch.tensor([[[[0.5]]], [[[2.0]]]], dtype=F64)
    mu, cov = predict.combine_predictions(means, covs, torch.tensor([0.25, 0.75], dtype=F64))
    assert mu.shape == (1, 1) and cov.shape == (1, 1, 1)
    assert float(mu) == 2.5 and float(cov) == 2.375              # (every figure is a dyadic fraction: exact)
    # two components in two dimensions with a weight per (model, series): series 0 as above on both axes with a
    # correlation, series 1 all weight on component 1
    means = torch.tensor([[[[1.0, 0.0]], [[5.0, 5.0]]], [[[3.0, 2.0]], [[-1.0, 4.0]]]], dtype=F64)          # [2, 2, 1, 2]
    covs = torch.zeros(2, 2, 1, 2, 2, dtype=F64)
    covs[0, :, 0] = torch.tensor([[0.5, 0.25], [0.25, 1.0]], dtype=F64)
    covs[1, :, 0] = torch.tensor([[2.0, -0.5], [-0.5, 1.0]], dtype=F64)
    w = torch.tensor([[0.25, 0.0], [0.75, 1.0]], dtype=F64)
    mu, cov = predict.combine_predictions(means, covs, w)
    assert mu.shape == (2, 1, 2) and cov.shape == (2, 1, 2, 2)
    assert mu[0, 0].tolist() == [2.5, 1.5]
    # E[x y] = 0.25 (0.25 + 0) + 0.75 (-0.5 + 6) = 4.1875, minus 2.5 * 1.5;  E[y^2] = 0.25 * 1 + 0.75 * 5 = 4, minus 2.25
    assert cov[0, 0].tolist() == [[2.375, 4.1875 - 3.75], [4.1875 - 3.75, 1.75]]
    assert mu[1, 0].tolist() == [-1.0, 4.0] and cov[1, 0].tolist() == [[2.0, -0.5], [-0.5, 1.0]]
    # a slot does not depend on the other series
    mu0, cov0 = predict.combine_predictions(means[:, :1], covs[:, :1], w[:, :1])
    assert torch.equal(mu0, mu[:1]) and torch.equal(cov0, cov[:1])
    # one model with weight one returns its input: the mean exactly, the covariance up to the rounding of
    # (C + m m^T) - m m^T, two roundings of a figure of size |C| + |m|^2
    gen = torch.Generator().manual_seed(3)
    m1 = torch.randn(1, 7, 3, generator=gen, dtype=F64)
    a = torch.randn(1, 7, 3, 3, generator=gen, dtype=F64)
    c1 = a @ a.transpose(-1, -2)
    mu, cov = predict.combine_predictions(m1, c1, torch.ones(1, dtype=F64))
    assert torch.equal(mu, m1[0])
    bound = 2 * float(torch.finfo(F64).eps) * (c1[0].abs() + (m1[0].unsqueeze(-1) * m1[0].unsqueeze(-2)).abs())
    assert bool(((cov - c1[0]).abs() <= bound).all())
    # the weights are not normalised for the caller
    mu2, _ = predict.combine_predictions(m1, c1, torch.full((1,), 2.0, dtype=F64))
    assert torch.equal(mu2, 2 * m1[0])
    for bad in (lambda: predict.combine_predictions(m1, c1[..., :2], torch.ones(1, dtype=F64)),
                lambda: predict.combine_predictions(m1, c1, torch.ones(2, dtype=F64)),
                lambda: predict.combine_predictions(m1, c1, torch.ones(1, 6, dtype=F64)),
                lambda: predict.combine_predictions(m1, c1, torch.ones(1, 7, 3, dtype=F64)),
                lambda: predict.combine_predictions(m1[0, 0, 0], c1, torch.ones(1, dtype=F64))):
        with pytest.raises(ValueError):
            bad()


# ---- on the GPU: the two kernels ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("d", range(1, 9))
def test_models_assembly_equals_the_one_model_kernel_bit_for_bit(d, dtype):
    """cgps_leg_posterior_blocks_models, every rank, both precisions, the three sources (the table with pattern bytes above
    entries - 1): every model's slice of K_Rs and Os is what cgps_leg_posterior_blocks_seg writes for that model, the block
    between two models is exactly zero, info is 0, and one model is the one-model kernel."""
    obs = 1 + d % 3
    ms, _ = _models(d, obs, 40 + d, dtype, "cuda")
    series = _series(obs, LENGTHS, 300 + d)
    ts, xs, mask, s = _ragged(series, dtype)
    plan = leg._cached_batch_plan(LENGTHS, ts.device)
    R = plan.R
    G = torch.stack([m.G for m in ms]).contiguous()
    A = torch.stack([m.B.T @ m.LLT_inv @ m.B for m in ms]).contiguous()
    tabs = [leg.observation_tables(m, mask) for m in ms]
    A_table = torch.stack([t[1] for t in tabs]).contiguous()
    pattern = tabs[0][0].clone()
    pattern[::7] = 255
    pattern[3] = A_table.shape[1]
    bw = [leg.observation_weights(m, mask, s) for m in ms]
    basis = torch.stack([b[0] for b in bw]).to(dtype).contiguous()
    weights = torch.stack([b[1] for b in bw]).to(dtype).contiguous()
    assert A_table.shape == (M, 1 << obs, d, d) and weights.shape == (M, R, obs * (obs + 1) // 2)
    cases = ((_hip.ROWS_PLAIN, A, None), (_hip.ROWS_TABLE, A_table, pattern), (_hip.ROWS_WEIGHTED, basis, weights))
    zero = torch.zeros(d, d, dtype=dtype, device="cuda")
    for source, term, rows in cases:
        for sel in ([0, 1, 2], [1]):                              # three models, and one
            per_model = source == _hip.ROWS_WEIGHTED
            K, Ko, info = leg._posterior_blocks_models(ts, G[sel].contiguous(), plan.cut, source, term[sel].contiguous(),
                                                       rows[sel].contiguous() if per_model else rows)
            m = len(sel)
            assert K.shape == (m * R, d, d) and Ko.shape == (m * R - 1, d, d) and int(info) == 0
            for j, k in enumerate(sel):
                K1, O1, i1 = leg._posterior_blocks_seg(ts, G[k].contiguous(), plan.cut, source, term[k].contiguous(),
                                                       rows[k].contiguous() if per_model else rows)
                assert int(i1) == 0
                assert torch.equal(K[j * R:(j + 1) * R], K1), (source, m, k)
                assert torch.equal(Ko[j * R:(j + 1) * R - 1], O1), (source, m, k)
                if j:
                    assert torch.equal(Ko[j * R - 1], zero) and not torch.signbit(Ko[j * R - 1]).any()
            assert bool(torch.isfinite(K).all())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("d", [1, 3, 5, 7, 8])                # (7: the instantiation DESIGN.md 4.14 warns about)
def test_models_intercast_equals_the_batch_kernel_bit_for_bit(d, dtype):
    """cgps_leg_intercast_models on a posterior of M R rows (the standard batch and its standard targets): every model's
    slice is what cgps_leg_intercast_seg gives on that model's slices, with NaN in every off-diagonal entry between two
    series or two models, and -- for the middle model -- NaN in everything that belongs to its neighbours."""
    gen = torch.Generator().manual_seed(700 + d)
    Gs = []
    for _ in range(M):
        Nm = torch.tril(torch.randn(d, d, generator=gen, dtype=F64)) * 0.4 + torch.eye(d, dtype=F64)
        Rm = torch.tril(torch.randn(d, d, generator=gen, dtype=F64), -1) * 0.3
        Gs.append(Nm @ Nm.T + Rm - Rm.T + 1e-5 * torch.eye(d, dtype=F64))
    dev = lambda t: t.to(dtype).cuda().contiguous()              # noqa: E731
    G = dev(torch.stack(Gs))
    ts, tts = standard_batch(LENGTHS, 40 + d)
    tlens = [int(t.shape[0]) for t in tts]
    plan = leg._cached_batch_plan(LENGTHS, G.device)
    tplan = leg._cached_batch_plan(tlens, G.device, make=predict._TargetPlan)
    R, P = plan.R, tplan.P
    assert P > 64
    mu, Rs, Os = (dev(t) for t in _random_posterior(M * R, d, gen))
    ends = torch.tensor([k * R + e - 1 for k in range(M) for e in plan.starts[1:]][:-1]).cuda()
    Os[ends] = float("nan")                                      # never read: cut gaps and model boundaries
    tcat, ttcat = dev(torch.cat(ts)), dev(torch.cat(tts))

    def run(G_, mu_, Rs_, Os_):
        means = torch.full((G_.shape[0], P, d), float("nan"), dtype=dtype, device="cuda")
        covs = torch.full((G_.shape[0], P, d, d), float("nan"), dtype=dtype, device="cuda")
        predict._intercast_models_hip(G_, mu_, Rs_, Os_, tcat, plan, ttcat, tplan, means, covs)
        return means, covs

    got_m, got_c = run(G, mu, Rs, Os)
    assert bool(torch.isfinite(got_m).all()) and bool(torch.isfinite(got_c).all())
    want = []
    for k in range(M):
        lo, hi = k * R, (k + 1) * R
        wm, wc = predict._intercast_seg_hip(G[k], mu[lo:hi], Rs[lo:hi], Os[lo:hi - 1], tcat, plan, ttcat, tplan)
        want.append((wm, wc))
        assert torch.equal(got_m[k], wm) and torch.equal(got_c[k], wc), k
    # one model is the batch kernel
    one_m, one_c = run(G[1:2].contiguous(), mu[R:2 * R].contiguous(), Rs[R:2 * R].contiguous(), Os[R:2 * R - 1].contiguous())
    assert torch.equal(one_m[0], want[1][0]) and torch.equal(one_c[0], want[1][1])
    # the middle model reads nothing of its neighbours
    mu_n, Rs_n, Os_n, G_n = mu.clone(), Rs.clone(), Os.clone(), G.clone()
    for lo, hi in ((0, R), (2 * R, 3 * R)):
        mu_n[lo:hi], Rs_n[lo:hi] = float("nan"), float("nan")
    Os_n[:R], Os_n[2 * R - 1:] = float("nan"), float("nan")
    G_n[0], G_n[2] = float("nan"), float("nan")
    nan_m, nan_c = run(G_n, mu_n, Rs_n, Os_n)
    assert torch.equal(nan_m[1], want[1][0]) and torch.equal(nan_c[1], want[1][1])


# ---- on the GPU: the calls ---------------------------------------------------------------------------------------------
def _loop(fn, ms, *args, **kw):
    return [fn(m, *args, **kw) for m in ms]


def _standard_targets_of(series, dtype):
    tts = [standard_targets(sr[0], b) for b, sr in enumerate(series)]
    return torch.cat(tts).to(dtype).cuda(), [int(t.shape[0]) for t in tts]


def _dense_inputs(series, dtype, mode):
    """(ts [B, n], xs [B, n, obs], observed, noise_var, targets [B, 6]) of equally long series; NaN where unobserved."""
    st = lambda k, dt: torch.stack([sr[k] for sr in series]).to(dt).cuda()           # noqa: E731
    ts, xs = st(0, dtype), st(1, dtype)
    ob, nv = _mode_args(mode, st(2, torch.bool), st(3, dtype))
    if ob is not None:
        xs = torch.where(ob, xs, torch.full_like(xs, float("nan")))
        if nv is not None:
            nv = torch.where(ob, nv, torch.full_like(nv, float("nan")))
    tq = torch.stack([torch.unique(torch.cat([sr[0][:1] - 0.4, 0.5 * (sr[0][4:8] + sr[0][5:9]), sr[0][-1:] + 0.3])) for sr in series])
    return ts, xs, ob, nv, tq.to(dtype).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("d", range(1, 9))
def test_the_one_call_equals_the_loop_over_the_models_fp64(d):
    """Every rank, plain / observed / noise / both, ragged (the standard lengths and targets) and dense (three series of
    33 rows): the posterior and both prediction calls against a loop of the ``*_batch`` calls over the models.  The
    concatenated reduction pairs rows differently and the stacked operands round differently, so not bit for bit:
    rtol 1e-9, atol 1e-11, as the batch against its own loop."""
    obs = 1 + d % 3
    ms, _ = _models(d, obs, 70 + d, F64, "cuda")
    series = _series(obs, LENGTHS, 500 + d)
    tt, tlens = _standard_targets_of(series, F64)
    R, P = sum(LENGTHS), sum(tlens)
    for mode in MODES:
        ts, xs, ob, nv = _poisoned(series, F64, mode)
        kw = dict(lengths=LENGTHS, observed=ob, noise_var=nv)
        mean, (Sd, So) = leg.insample_posterior_models(ms, ts, xs, **kw)
        assert mean.shape == (M, R, d) and Sd.shape == (M, R, d, d) and So.shape == (M, R - 1, d, d)
        assert not mean.requires_grad
        for k, (rm, (rSd, rSo)) in enumerate(_loop(leg.insample_posterior_batch, ms, ts, xs, **kw)):
            for g_, r_, what in ((mean[k], rm, "mean"), (Sd[k], rSd, "cov_diag"), (So[k], rSo, "cov_off")):
                _close(g_, r_, "%s model %d %s" % (mode, k, what))
        for one, loop, w in ((predict.predictive_posterior_models, predict.predictive_posterior_batch, d),
                             (predict.make_predictions_models, predict.make_predictions_batch, obs)):
            pm, pv = one(ms, ts, xs, tt, target_lengths=tlens, **kw)
            assert pm.shape == (M, P, w) and pv.shape == (M, P, w, w)
            for k, (rm, rv) in enumerate(_loop(loop, ms, ts, xs, tt, target_lengths=tlens, **kw)):
                _close(pm[k], rm, "%s model %d %s mean" % (mode, k, one.__name__))
                _close(pv[k], rv, "%s model %d %s cov" % (mode, k, one.__name__))
    dense = _series(obs, [33, 33, 33], 900 + d)
    for mode in MODES:
        ts, xs, ob, nv, tq = _dense_inputs(dense, F64, mode)
        kw = dict(observed=ob, noise_var=nv)
        mean, (Sd, So) = leg.insample_posterior_models(ms, ts, xs, **kw)
        assert mean.shape == (M, 3, 33, d) and Sd.shape == (M, 3, 33, d, d) and So.shape == (M, 3, 32, d, d)
        for k, (rm, (rSd, rSo)) in enumerate(_loop(leg.insample_posterior_batch, ms, ts, xs, **kw)):
            for g_, r_, what in ((mean[k], rm, "mean"), (Sd[k], rSd, "cov_diag"), (So[k], rSo, "cov_off")):
                _close(g_, r_, "dense %s model %d %s" % (mode, k, what))
        for one, loop, w in ((predict.predictive_posterior_models, predict.predictive_posterior_batch, d),
                             (predict.make_predictions_models, predict.make_predictions_batch, obs)):
            pm, pv = one(ms, ts, xs, tq, **kw)
            assert pm.shape == (M, 3, 6, w) and pv.shape == (M, 3, 6, w, w)
            for k, (rm, rv) in enumerate(_loop(loop, ms, ts, xs, tq, **kw)):
                _close(pm[k], rm, "dense %s model %d %s mean" % (mode, k, one.__name__))
                _close(pv[k], rv, "dense %s model %d %s cov" % (mode, k, one.__name__))


@pytest.mark.gpu
@pytest.mark.parametrize("d", range(1, 9))
def test_the_one_call_in_fp32_is_as_accurate_as_the_loop(d):
    """The rule of test_batched_posterior_fp32_is_as_accurate_as_the_loop: fp32 against the dense fp64 truth of every
    (model, series) (_missref / _noiseref, series of at most 33 rows); per quantity the one call's largest error is at
    most 4 times the largest error of the loop of insample_posterior_batch over the models plus 16 eps32 max|truth|."""
    obs = 1 + d % 3
    ms, mats = _models(d, obs, 70 + d, F32, "cuda")

    def check(label, series, one, loop, mode):
        truth = [[_dense_truth(mats[k], sr, mode) for sr in series] for k in range(M)]
        for q, what in enumerate(("mean", "cov_diag", "cov_off")):
            err = lambda res: max(float((res[k][b][q].double().cpu() - truth[k][b][q]).abs().max())      # noqa: E731
                                  for k in range(M) for b in range(len(series)) if truth[k][b][q].numel())
            scale = max(float(t[q].abs().max()) for tk in truth for t in tk if t[q].numel())
            e_one, e_loop = err(one), err(loop)
            print("%s d=%d %s %s: one call %.3e loop %.3e scale %.3e" % (label, d, mode, what, e_one, e_loop, scale))
            assert e_one <= 4 * e_loop + 16 * EPS32 * scale, (label, mode, what, e_one, e_loop, scale)

    series = _series(obs, SMALL, 600 + d)
    for mode in MODES:
        ts, xs, ob, nv = _poisoned(series, F32, mode)
        kw = dict(lengths=SMALL, observed=ob, noise_var=nv)
        mean, (Sd, So) = leg.insample_posterior_models(ms, ts, xs, **kw)
        assert mean.dtype == F32
        one = [_split(mean[k], Sd[k], So[k], SMALL) for k in range(M)]
        loop = [_split(rm, rSd, rSo, SMALL) for rm, (rSd, rSo) in _loop(leg.insample_posterior_batch, ms, ts, xs, **kw)]
        check("ragged", series, one, loop, mode)
    dense = _series(obs, [33, 33, 33], 650 + d)
    for mode in MODES:
        ts, xs, ob, nv, _ = _dense_inputs(dense, F32, mode)
        kw = dict(observed=ob, noise_var=nv)
        mean, (Sd, So) = leg.insample_posterior_models(ms, ts, xs, **kw)
        assert mean.shape == (M, 3, 33, d) and So.shape == (M, 3, 32, d, d)
        one = [[(mean[k, b], Sd[k, b], So[k, b]) for b in range(3)] for k in range(M)]
        loop = [[(rm[b], rSd[b], rSo[b]) for b in range(3)] for rm, (rSd, rSo) in _loop(leg.insample_posterior_batch, ms, ts, xs, **kw)]
        check("dense", dense, one, loop, mode)


@pytest.mark.gpu
def test_chunks_of_whole_models_give_the_unchunked_results(monkeypatch):
    """MODELS_POSTERIOR_MAX_ROWS at R (1 + 1 + 1 models), just below 2 R (still 1 + 1 + 1: a chunk holds whole models),
    at 2 R (2 + 1) and below R (a chunk always holds one model) against the one chunk of the default."""
    d, obs = 5, 2
    ms, _ = _models(d, obs, 31, F64, "cuda")
    series = _series(obs, LENGTHS, 41)
    tt, tlens = _standard_targets_of(series, F64)
    ts, xs, ob, nv = _poisoned(series, F64, "both")
    kw = dict(lengths=LENGTHS, observed=ob, noise_var=nv)
    R = sum(LENGTHS)
    assert leg.MODELS_POSTERIOR_MAX_ROWS == leg.MODELS_BACKWARD_MAX_ROWS >= M * R

    def results():
        seen = []
        real = leg._posterior_blocks_models
        monkeypatch.setattr(leg, "_posterior_blocks_models", lambda ts_, G_, *a, **k: (seen.append(G_.shape[0]), real(ts_, G_, *a, **k))[1])
        mean, (Sd, So) = leg.insample_posterior_models(ms, ts, xs, **kw)
        chunks = list(seen)
        pm, pv = predict.predictive_posterior_models(ms, ts, xs, tt, target_lengths=tlens, **kw)
        om, ov = predict.make_predictions_models(ms, ts, xs, tt, target_lengths=tlens, **kw)
        monkeypatch.setattr(leg, "_posterior_blocks_models", real)
        assert seen == chunks * 3
        return chunks, (mean, Sd, So, pm, pv, om, ov)

    chunks, whole = results()
    assert chunks == [3]
    for limit, want in ((R, [1, 1, 1]), (2 * R - 1, [1, 1, 1]), (2 * R, [2, 1]), (R // 2, [1, 1, 1])):
        monkeypatch.setattr(leg, "MODELS_POSTERIOR_MAX_ROWS", limit)
        chunks, got = results()
        assert chunks == want, (limit, chunks)
        for g_, w_, what in zip(got, whole, ("mean", "cov_diag", "cov_off", "pp mean", "pp cov", "pred mean", "pred cov")):
            assert g_.shape == w_.shape
            _close(g_, w_, "limit %d %s" % (limit, what))


@pytest.mark.gpu
def test_models_are_independent_and_the_result_is_reproducible():
    d, obs = 4, 2
    ms, _ = _models(d, obs, 12, F64, "cuda")
    series = _series(obs, LENGTHS, 78)
    tt, tlens = _standard_targets_of(series, F64)
    ts, xs, ob, nv = _poisoned(series, F64, "both")
    kw = dict(lengths=LENGTHS, observed=ob, noise_var=nv)

    def everything(models):
        mean, (Sd, So) = leg.insample_posterior_models(models, ts, xs, **kw)
        pm, pv = predict.predictive_posterior_models(models, ts, xs, tt, target_lengths=tlens, **kw)
        om, ov = predict.make_predictions_models(models, ts, xs, tt, target_lengths=tlens, **kw)
        return mean, Sd, So, pm, pv, om, ov

    first = everything(ms)
    # the entries of cov_off at a series boundary are exactly zero, for every model
    plan = leg._cached_batch_plan(LENGTHS, ts.device)
    cuts = (torch.tensor(plan.starts[1:-1]) - 1).cuda()
    So = first[2]
    assert torch.equal(So[:, cuts], torch.zeros(M, len(cuts), d, d, dtype=F64, device="cuda"))
    assert not torch.signbit(So[:, cuts]).any()
    # two identical calls
    assert all(torch.equal(a, b) for a, b in zip(first, everything(ms)))
    # other (finite) matrices for models 0 and 2: model 1's slot does not move by a bit -- its blocks meet theirs only
    # through the zero coupling, and zero times a finite number is zero
    others, _ = _models(d, obs, 400, F64, "cuda")
    changed = everything([others[0], ms[1], others[2]])
    for a, b in zip(first, changed):
        assert torch.equal(a[1], b[1])
        assert not torch.equal(a[0], b[0]) and not torch.equal(a[2], b[2])      # the change matters
    # the mixture of the three predictions, from the log-likelihoods of the same models
    ll = leg.log_likelihood_models_observed(ms, ts, xs, **kw)
    assert ll.shape == (M, len(LENGTHS))
    w = torch.softmax(ll.sum(1), 0)
    mu, cov = predict.combine_predictions(first[5], first[6], w)
    assert mu.shape == first[5].shape[1:] and cov.shape == first[6].shape[1:] and bool(torch.isfinite(cov).all())


@pytest.mark.gpu
def test_predictions_match_the_reference_recordings():
    """tests/golden/leg_models_predictions.npz (make_golden_models_predictions.py): the three models and three series of
    leg_models.npz, the reference's predictive_posterior and make_predictions per (model, series).  Every slot of the
    one call at rtol 1e-6, atol 1e-7, the tolerance of test_batched_predictions_match_the_reference_recordings."""
    g = np.load(os.path.join(_util.GOLDEN, "leg_models_predictions.npz"))
    t = lambda k: torch.from_numpy(g[k]).to(F64).cuda()                              # noqa: E731
    ms = [leg.LEGMatrices(t("N")[k], t("R")[k], t("B")[k], t("Lambda")[k]) for k in range(g["N"].shape[0])]
    lens, tlens = [int(n) for n in g["lengths"]], [int(n) for n in g["target_lengths"]]
    assert len(ms) == 3 and len(lens) == 3 and all(20 <= p for p in tlens[1:])
    tol = dict(rtol=1e-6, atol=1e-7)
    lm, lv = predict.predictive_posterior_models(ms, t("ts"), t("xs"), t("target_ts"), lengths=lens, target_lengths=tlens)
    pm, pv = predict.make_predictions_models(ms, t("ts"), t("xs"), t("target_ts"), lengths=lens, target_lengths=tlens)
    for got, key in ((pm, "pred_mean"), (pv, "pred_cov"), (lm, "pp_mean"), (lv, "pp_cov")):
        assert tuple(got.shape) == g[key].shape, key
        for k in range(3):
            s = 0
            for b, p in enumerate(tlens):
                np.testing.assert_allclose(got[k, s:s + p].cpu().numpy(), g[key][k, s:s + p],
                                           err_msg="%s model %d series %d" % (key, k, b), **tol)
                s += p


@pytest.mark.gpu
def test_a_zero_length_gap_is_named_with_its_series():
    d, obs = 3, 1
    ms, _ = _models(d, obs, 8, F64, "cuda")
    lengths = [9, 17, 12, 6]
    series = _series(obs, lengths, 80)
    ts, xs, _, _ = _ragged(series, F64)
    start = sum(lengths[:2])
    ts[start + 5] = ts[start + 4]                                # a repeated time stamp in series 2
    assert leg.cr.CHECK_POSITIVE_DEFINITE
    for call in (lambda: leg.insample_posterior_models(ms, ts, xs, lengths=lengths),
                 lambda: predict.make_predictions_models(ms, ts, xs, ts[:3] + 0.01, lengths=lengths, target_lengths=[3, 0, 0, 0])):
        with pytest.raises(leg.cr.NotPSDError) as e:
            call()
        hit = re.search(r"model (\d+).*series (\d+).*row (\d+)", str(e.value))
        assert hit and int(hit.group(2)) == 2 and int(hit.group(3)) in (4, 5), str(e.value)
        assert 0 <= int(hit.group(1)) < M


@pytest.mark.gpu
def test_the_model_whose_factor_fails_is_named_and_is_nan_without_the_check():
    """obs_dim 1 and three models with LLT[0, 0] = 1, 0.25 and 2.25.  The time stamps are fine, so the assembly reports
    nothing; a noise variance just below -0.25 at one row of series 2 makes that row's block of K negative definite for
    the middle model alone (the others see a positive variance there): the error names model 1, series 2 and a row inside
    it.  With the check off that model's slots are NaN and nothing raises."""
    d, obs = 3, 1
    ms, _ = _models(d, obs, 8, F64, "cuda")
    lam = (1.0, 0.5, 1.5)
    ms = [leg.LEGMatrices(m.N, m.R, m.B, torch.full((1, 1), v, dtype=F64, device="cuda")) for m, v in zip(ms, lam)]
    lengths = [9, 17, 12, 6]
    series = _series(obs, lengths, 83)
    ts, xs, _, s = _ragged(series, F64)
    fail, b, r = 1, 2, 7
    llt = float(ms[fail].LLT[0, 0])
    assert all(float(m.LLT[0, 0]) > 2 * llt for k, m in enumerate(ms) if k != fail)
    row = sum(lengths[:b]) + r
    bnorm = float((ms[fail].B ** 2).sum())
    s[row] = -llt - bnorm / 1e6                                  # Li = -1e6 / |B|^2: the block gets -1e6 in the direction of B
    tt, tlens = ts[row:row + 2] + 0.01, [0, 0, 2, 0]
    assert leg.cr.CHECK_POSITIVE_DEFINITE
    for call in (lambda: leg.insample_posterior_models(ms, ts, xs, lengths=lengths, noise_var=s),
                 lambda: predict.predictive_posterior_models(ms, ts, xs, tt, lengths=lengths, target_lengths=tlens, noise_var=s)):
        with pytest.raises(leg.cr.NotPSDError) as e:
            call()
        hit = re.search(r"model (\d+).*series (\d+).*row (\d+)", str(e.value))
        # (the factor's info word names a row NEAR the failing block: the model and the series must be the right ones and
        # the row one of the series' own)
        assert hit and int(hit.group(1)) == fail and int(hit.group(2)) == b and 0 <= int(hit.group(3)) < lengths[b], str(e.value)
    leg.cr.CHECK_POSITIVE_DEFINITE = False
    try:
        mean, (Sd, So) = leg.insample_posterior_models(ms, ts, xs, lengths=lengths, noise_var=s)
        pm, pv = predict.predictive_posterior_models(ms, ts, xs, tt, lengths=lengths, target_lengths=tlens, noise_var=s)
    finally:
        leg.cr.CHECK_POSITIVE_DEFINITE = True
    lo, hi = sum(lengths[:b]), sum(lengths[:b + 1])
    assert bool(torch.isnan(mean[fail, lo:hi]).all()) and bool(torch.isnan(Sd[fail, lo:hi]).all())
    assert bool(torch.isnan(So[fail, lo:hi - 1]).all())
    assert bool(torch.isnan(pm[fail]).all()) and bool(torch.isnan(pv[fail]).all())

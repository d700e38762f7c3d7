"""One-step-ahead predictives and filtered states (leg.filter_predictive, leg.filter_predictive_batch,
leg.filter_predictive_models; cgps_leg_filter: DESIGN.md 4.22) against dense fp64 truths that need no filtering algebra,
against the library's own smoother and likelihood, and for the properties a forward recursion has bit for bit:
causality, independence of a series from its place in the batch, of a model from its place among the models.

The truths (``_truth``): the filtered state of row i is the dense Gaussian posterior (``_noiseref``) with the mask's
rows > i switched off; the predictive of row i is that posterior with rows >= i switched off, pushed through B plus the
row's noise; the row's log density is the Gaussian log density of its observed entries under that predictive; the
log-likelihood is ``_noiseref.leg_dense_loglik`` of the whole series.  Bounds: rtol 1e-7, atol 1e-9 for the per-row
outputs and 1e-9 max(1, |ll|) for the log-likelihood, those tests/test_leg_noise.py holds the posterior and the
log-likelihood to against the same truths."""
import functools
import math
import re

import pytest
import torch

import _filterref
import _gapref
import _noiseref as nr
from cyclic_gps import _hip, leg
from test_leg_posterior_batch import MODES, _mode_args, _model, _ragged, _series

cr = leg.cr
F64, F32 = torch.float64, torch.float32
EPS = {F64: float(torch.finfo(F64).eps), F32: float(torch.finfo(F32).eps)}
LENGTHS = (1, 2, 3, 65, 7)
ROWS = ("mean", "cov", "logpdf", "z_mean", "z_cov")
GRID = [(d, obs) for d in (1, 5, 8) for obs in (1, 2, 3, 8)]
RTOL, ATOL, LL_TOL = 1e-7, 1e-9, 1e-9


# ---- truths ------------------------------------------------------------------------------------------------------------
def _truth(mats, ts, xs, s, mask):
    """The dense truth of one series (fp64, CPU): mean [n, obs], cov [n, obs, obs], logpdf [n], z_mean [n, d], z_cov
    [n, d, d], loglik.  s and mask may be None.  Row i's two posteriors are ``_noiseref.leg_dense_posterior`` with the
    rows > i (>= i) of the mask switched off, evaluated here from one prior covariance of the series (rows that are
    switched off and lie after i drop out of a Gaussian's marginal); the first, a middle and the last row are held to
    ``_noiseref.leg_dense_posterior`` itself."""
    Nm, Rm, Bm, Lm = mats
    n, obs = xs.shape
    d = Nm.shape[0]
    mask = torch.ones(n, obs, dtype=torch.bool) if mask is None else mask
    s = torch.zeros(n, obs, dtype=F64) if s is None else torch.where(mask, s, torch.zeros_like(s))
    xz = torch.where(mask, xs, torch.zeros_like(xs))
    G = Nm @ Nm.T + Rm - Rm.T + 1e-5 * torch.eye(d, dtype=F64)
    Sigma = _gapref.prior_covariance(ts, G)
    LLT = Lm @ Lm.T + 1e-9 * torch.eye(obs, dtype=F64)
    HB = torch.kron(torch.eye(n, dtype=F64), Bm)
    noise = torch.kron(torch.eye(n, dtype=F64), LLT) + torch.diag(s.reshape(-1))
    x = xz.reshape(-1)

    def posterior_of_row(i, rows_seen):
        """(mean [d], cov [d, d]) of z_i given the observed entries of the rows < rows_seen (<= i + 1)"""
        k = (i + 1) * d
        Sg = Sigma[:k, :k]
        idx = mask[:rows_seen].reshape(-1).nonzero().flatten()
        if idx.numel() == 0:
            return torch.zeros(d, dtype=F64), Sg[i * d:, i * d:]
        H = HB[idx][:, :k]
        C = H @ Sg @ H.T + noise[idx][:, idx]
        Szx = Sg[i * d:] @ H.T
        sol = torch.linalg.solve(C, torch.cat([x[idx, None], Szx.T], 1))
        return Szx @ sol[:, 0], Sg[i * d:, i * d:] - Szx @ sol[:, 1:]

    out = {"mean": torch.zeros(n, obs, dtype=F64), "cov": torch.zeros(n, obs, obs, dtype=F64),
           "logpdf": torch.zeros(n, dtype=F64), "z_mean": torch.zeros(n, d, dtype=F64), "z_cov": torch.zeros(n, d, d, dtype=F64)}
    for i in range(n):
        out["z_mean"][i], out["z_cov"][i] = posterior_of_row(i, i + 1)
        mu, cov = posterior_of_row(i, i)
        out["mean"][i] = Bm @ mu
        out["cov"][i] = Bm @ cov @ Bm.T + LLT + torch.diag(s[i])
        o = mask[i].nonzero().flatten()
        if o.numel():
            T = torch.linalg.cholesky(out["cov"][i][o][:, o])
            e = torch.linalg.solve_triangular(T, (xz[i, o] - out["mean"][i, o])[:, None], upper=False)
            out["logpdf"][i] = -0.5 * (e * e).sum() - torch.log(torch.diagonal(T)).sum() - 0.5 * o.numel() * math.log(2 * math.pi)
    rows = torch.arange(n).unsqueeze(1)
    for i in sorted({0, n // 2, n - 1}):
        mean, cov = nr.leg_dense_posterior(Nm, Rm, Bm, Lm, ts, xz, s, mask & (rows <= i))
        assert float((mean[i] - out["z_mean"][i]).abs().max()) <= 1e-12 and float((cov[i, :, i, :] - out["z_cov"][i]).abs().max()) <= 1e-12
        mean, cov = nr.leg_dense_posterior(Nm, Rm, Bm, Lm, ts, xz, s, mask & (rows < i))
        assert float((Bm @ mean[i] - out["mean"][i]).abs().max()) <= 1e-12
        assert float((Bm @ cov[i, :, i, :] @ Bm.T + LLT + torch.diag(s[i]) - out["cov"][i]).abs().max()) <= 1e-12
    out["loglik"] = nr.leg_dense_loglik(Nm, Rm, Bm, Lm, ts, xz, s, mask)
    return out


def _truth_args(sr, mode):
    ts, xs, mask, s = sr
    return ts, xs, (s if mode in ("noise", "both") else None), (mask if mode in ("observed", "both") else None)


def _assert_mask_covers(series, obs):
    """What every masked case must contain: a series whose first row observes nothing, a wholly unobserved interior row,
    and (obs > 1) a partly observed row."""
    assert any(not bool(sr[2][0].any()) for sr in series), "no series starts with an unobserved row (pick another seed)"
    assert any(sr[2].shape[0] > 2 and bool((~sr[2][1:-1].any(1)).any()) for sr in series), "no unobserved interior row"
    if obs > 1:
        assert any(bool((sr[2].any(1) & ~sr[2].all(1)).any()) for sr in series), "no partly observed row"


@functools.lru_cache(maxsize=None)
def _case(d, obs, lengths, seed, mode):
    """(model matrices, series, [truth of every series]), computed once and shared by the tests."""
    _, mats = _model(d, obs, seed)
    series = _series(obs, list(lengths), seed + 1)
    if mode in ("observed", "both"):
        _assert_mask_covers(series, obs)
    return mats, series, [_truth(mats, *_truth_args(sr, mode)) for sr in series]


def _seed(d, obs):
    return 300 + 10 * d + obs


def _cat(truths, key):
    return torch.cat([t[key] for t in truths])


def _cuda_model(mats, dtype=F64):
    return leg.LEGMatrices(*(t.to(dtype).cuda() for t in mats))


def _inputs(series, mode, dtype, fill=float("nan")):
    """(ts, xs, observed, noise_var) of the ragged batch on the GPU; xs and noise_var hold ``fill`` where nothing is observed."""
    ts, xs, mask, s = _ragged(series, dtype)
    ob, nv = _mode_args(mode, mask, s)
    if ob is not None:
        xs = torch.where(ob, xs, torch.full_like(xs, fill))
        if nv is not None:
            nv = torch.where(ob, nv, torch.full_like(nv, fill))
    return ts, xs, ob, nv


def _assert_rows_close(out, truths, what, rtol=RTOL, atol=ATOL):
    for key, got in zip(ROWS, out[:5]):
        want = _cat(truths, key)
        got = got.cpu().to(F64).reshape(want.shape)
        err = (got - want).abs()
        print("%s %s: max |err| %.3e (rtol %.1e atol %.1e)" % (what, key, float(err.max()), rtol, atol))
        assert bool((err - rtol * want.abs() <= atol).all()), (what, key, float(err.max()))


def _assert_loglik_close(ll, truths, what, tol=LL_TOL):
    want = torch.stack([t["loglik"] for t in truths])
    got = ll.cpu().reshape(want.shape)
    assert got.dtype == F64
    err = (got - want).abs() / want.abs().clamp_min(1.0)
    print("%s loglik: max err %.3e of max(1, |ll|) (bound %.1e)" % (what, float(err.max()), tol))
    assert bool((err <= tol).all()), (what, float(err.max()))


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def _seq_sum(v):
    acc = 0.0
    for t in v.tolist():
        acc += t
    return acc


def _split(t, lengths):
    return list(torch.split(t, list(lengths)))


# ---- 1. fp64 against the dense truths --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d,obs", GRID)
def test_ragged_batch_against_the_dense_truths(d, obs, mode):
    mats, series, truth = _case(d, obs, LENGTHS, _seed(d, obs), mode)
    ts, xs, ob, nv = _inputs(series, mode, F64)
    out = leg.filter_predictive_batch(_cuda_model(mats), ts, xs, lengths=list(LENGTHS), observed=ob, noise_var=nv)
    R = sum(LENGTHS)
    assert [tuple(t.shape) for t in out[:6]] == [(R, obs), (R, obs, obs), (R,), (R, d), (R, d, d), (len(LENGTHS),)]
    _assert_rows_close(out, truth, "ragged d %d obs %d %s" % (d, obs, mode))
    _assert_loglik_close(out.loglik, truth, "ragged d %d obs %d %s" % (d, obs, mode))
    # the state is that of every series' last row
    ends = torch.tensor(LENGTHS).cumsum(0) - 1
    assert torch.equal(out.state.t, ts[ends.cuda()])
    assert torch.equal(out.state.mean, out.z_mean[ends.cuda()]) and torch.equal(out.state.cov, out.z_cov[ends.cuda()])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "both"])
@pytest.mark.parametrize("d,obs", [(1, 1), (5, 3), (8, 8)])
def test_one_series_against_the_dense_truths(d, obs, mode):
    mats, series, truth = _case(d, obs, (1, 2, 7), _seed(d, obs) + 1, mode)
    m = _cuda_model(mats)
    for sr, tr in zip(series, truth):
        ts, xs, ob, nv = _inputs([sr], mode, F64)
        out = leg.filter_predictive(m, ts, xs, observed=ob, noise_var=nv)
        n = ts.shape[0]
        assert [tuple(t.shape) for t in out[:6]] == [(n, obs), (n, obs, obs), (n,), (n, d), (n, d, d), ()]
        assert tuple(out.state.t.shape) == () and tuple(out.state.mean.shape) == (d,) and tuple(out.state.cov.shape) == (d, d)
        _assert_rows_close(out, [tr], "one series n %d d %d obs %d %s" % (n, d, obs, mode))
        _assert_loglik_close(out.loglik, [tr], "one series n %d" % n)
        # a series alone equals its slot in a batch, bit for bit
        bat = leg.filter_predictive_batch(m, ts, xs, lengths=[n], observed=ob, noise_var=nv)
        assert all(_same_bits(a, b) for a, b in zip(out[:5], bat[:5])) and _same_bits(out.loglik, bat.loglik[0])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_dense_layout_against_the_truths_and_the_ragged_call(mode):
    d, obs, B, n = 5, 2, 3, 7
    mats, series, truth = _case(d, obs, (n,) * B, 41, mode)
    m = _cuda_model(mats)
    ts, xs, ob, nv = _inputs(series, mode, F64)
    rag = leg.filter_predictive_batch(m, ts, xs, lengths=[n] * B, observed=ob, noise_var=nv)
    v = lambda t: None if t is None else t.reshape((B, n) + tuple(t.shape[1:]))      # noqa: E731
    out = leg.filter_predictive_batch(m, v(ts), v(xs), observed=v(ob), noise_var=v(nv))
    assert [tuple(t.shape) for t in out[:6]] == [(B, n, obs), (B, n, obs, obs), (B, n), (B, n, d), (B, n, d, d), (B,)]
    _assert_rows_close(out, truth, "dense %s" % mode)
    _assert_loglik_close(out.loglik, truth, "dense %s" % mode)
    for a, b in zip(out[:5], rag[:5]):
        assert _same_bits(a.reshape(b.shape), b)
    assert _same_bits(out.loglik, rag.loglik) and all(_same_bits(a, b) for a, b in zip(out.state, rag.state))


def _many_short_series(obs, B, seed):
    """B series of 1..4 rows; every fifth of three rows or more has an unobserved interior row, every seventh an
    unobserved first row."""
    lengths = [1 + (b * 7 + b // 4) % 4 for b in range(B)]
    series = _series(obs, lengths, seed)
    for b, (_, _, mask, _) in enumerate(series):
        if b % 7 == 0:
            mask[0] = False
        if b % 5 == 0 and mask.shape[0] >= 3:
            mask[1] = False
    return lengths, series


@functools.lru_cache(maxsize=None)
def _many_case(d, obs, B, seed):
    _, mats = _model(d, obs, seed)
    lengths, series = _many_short_series(obs, B, seed + 1)
    _assert_mask_covers(series, obs)
    return mats, lengths, series, [_truth(mats, *_truth_args(sr, "both")) for sr in series]


@pytest.mark.gpu
@pytest.mark.parametrize("d,obs", [(5, 3), (8, 1), (8, 8)])
def test_many_series_cross_the_workgroup_and_the_grid(d, obs):
    """B = 300 series of 1..4 rows: five 64-lane workgroups whose lanes leave the walk at different rows; with three
    models a second grid row as well.  Against the truths, and bit for bit: the state is the last row's, a permutation
    of the series permutes the results, a series alone equals its slot."""
    B = 300
    mats, lengths, series, truth = _many_case(d, obs, B, 50 + d)
    assert set(lengths) == {1, 2, 3, 4}
    m = _cuda_model(mats)
    ts, xs, ob, nv = _inputs(series, "both", F64)
    out = leg.filter_predictive_batch(m, ts, xs, lengths=lengths, observed=ob, noise_var=nv)
    _assert_rows_close(out, truth, "300 series d %d obs %d" % (d, obs))
    _assert_loglik_close(out.loglik, truth, "300 series")
    ends = (torch.tensor(lengths).cumsum(0) - 1).cuda()
    assert _same_bits(out.state.mean, out.z_mean[ends]) and _same_bits(out.state.cov, out.z_cov[ends])
    for b, lp in enumerate(_split(out.logpdf.cpu(), lengths)):
        assert _seq_sum(lp) == float(out.loglik[b]), b
    perm =torch.randperm(B, generator=torch.Generator().manual_seed(5)).tolist()
    pts, pxs, pob, pnv = _inputs([series[b] for b in perm], "both", F64)
    pout = leg.filter_predictive_batch(m, pts, pxs, lengths=[lengths[b] for b in perm], observed=pob, noise_var=pnv)
    for a, b in zip(out[:5], pout[:5]):
        parts = _split(a, lengths)
        assert _same_bits(torch.cat([parts[j] for j in perm]), b)
    idx = torch.tensor(perm).cuda()
    assert _same_bits(out.loglik[idx], pout.loglik) and all(_same_bits(a[idx], b) for a, b in zip(out.state, pout.state))
    for b in (0, 63, 64, 299):
        t1, x1, o1, n1 = _inputs([series[b]], "both", F64)
        alone = leg.filter_predictive(m, t1, x1, observed=o1, noise_var=n1)
        assert all(_same_bits(_split(a, lengths)[b], c) for a, c in zip(out[:5], alone[:5]))
        assert _same_bits(out.loglik[b], alone.loglik) and _same_bits(out.state.mean[b], alone.state.mean)
    # three models: the second grid row; slice k is the call on model k
    others = [_model(d, obs, 70 + k)[1] for k in range(2)]
    ms = [m] + [_cuda_model(o) for o in others]
    three = leg.filter_predictive_models(ms, ts, xs, lengths=lengths, observed=ob, noise_var=nv)
    assert all(_same_bits(a[0], b) for a, b in zip(three[:6], out[:6]))
    for k in (1, 2):
        each = leg.filter_predictive_batch(ms[k], ts, xs, lengths=lengths, observed=ob, noise_var=nv)
        assert all(_same_bits(a[k], b) for a, b in zip(three[:6], each[:6]))
        assert all(_same_bits(a[k], b) for a, b in zip(three.state[1:], each.state[1:])) and _same_bits(three.state.t, each.state.t)
        assert not _same_bits(three.mean[k], three.mean[0])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dense", [False, True])
def test_models_against_the_truths_and_one_call_per_model(mode, dense):
    d, obs, M = 5, 3, 3
    lengths = (7, 7, 7) if dense else LENGTHS
    cases = [_case(d, obs, lengths, 80, mode)] + [None] * (M - 1)
    series = cases[0][1]
    models = [cases[0][0]] + [_model(d, obs, 81 + k)[1] for k in range(M - 1)]
    truths = [cases[0][2]] + [[_truth(mats, *_truth_args(sr, mode)) for sr in series] for mats in models[1:]]
    ms = [_cuda_model(mats) for mats in models]
    ts, xs, ob, nv = _inputs(series, mode, F64)
    if dense:
        v = lambda t: None if t is None else t.reshape((3, 7) + tuple(t.shape[1:]))      # noqa: E731
        args, kw = (v(ts), v(xs)), dict(observed=v(ob), noise_var=v(nv))
    else:
        args, kw = (ts, xs), dict(lengths=list(lengths), observed=ob, noise_var=nv)
    out = leg.filter_predictive_models(ms, *args, **kw)
    assert out.loglik.shape == (M, len(lengths)) and out.loglik.dtype == F64
    assert tuple(out.state.t.shape) == (len(lengths),) and tuple(out.state.cov.shape) == (M, len(lengths), d, d)
    for k in range(M):
        each = leg.filter_predictive_batch(ms[k], *args, **kw)
        assert all(_same_bits(a[k], b) for a, b in zip(out[:6], each[:6]))
        assert _same_bits(out.state.mean[k], each.state.mean) and _same_bits(out.state.cov[k], each.state.cov)
        _assert_rows_close([t[k] for t in out[:5]], truths[k], "models %s model %d" % (mode, k))
        _assert_loglik_close(out.loglik[k], truths[k], "models %s model %d" % (mode, k))


# ---- 2. identities inside the library --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d,obs", [(1, 1), (5, 2), (5, 3), (8, 8)])
def test_loglik_and_last_state_agree_with_the_likelihood_and_the_smoother(d, obs, mode):
    mats, series, truth = _case(d, obs, LENGTHS, _seed(d, obs), mode)
    m = _cuda_model(mats)
    ts, xs, ob, nv = _inputs(series, mode, F64)
    kw = dict(lengths=list(LENGTHS), observed=ob, noise_var=nv)
    out = leg.filter_predictive_batch(m, ts, xs, **kw)
    ll = leg.log_likelihood_batch(m, ts, xs, **kw).to(F64)
    err = (out.loglik - ll).abs() / ll.abs().clamp_min(1.0)
    print("loglik against log_likelihood_batch: %.3e" % float(err.max()))
    assert bool((err <= 2e-9).all())
    # the sum of the row terms in row order, bit for bit
    for b, lp in enumerate(_split(out.logpdf.cpu(), LENGTHS)):
        assert _seq_sum(lp) == float(out.loglik[b]), b
    # the last row has seen the whole series: the smoother's last row
    mean, (Sd, _) = leg.insample_posterior_batch(m, ts, xs, **kw)
    ends = (torch.tensor(LENGTHS).cumsum(0) - 1).cuda()
    for got, want in ((out.z_mean[ends], mean[ends]), (out.z_cov[ends], Sd[ends])):
        assert bool(((got - want).abs() - RTOL * want.abs() <= ATOL).all())


# ---- 3. causality ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("d,obs", [(5, 3), (8, 8), (1, 1)])
def test_nothing_depends_on_later_rows_bit_for_bit(d, obs):
    n = 7
    _, mats = _model(d, obs, 90 + d)
    (ts, xs, mask, s), = _series(obs, [n], 91 + d)
    m = _cuda_model(mats)
    call = lambda t, x, o, v: leg.filter_predictive(m, t.cuda(), x.cuda(), observed=o.cuda(), noise_var=v.cuda())   # noqa: E731
    base = call(ts, xs, mask, s)
    gen = torch.Generator().manual_seed(7)
    cr.CHECK_POSITIVE_DEFINITE = False              # (a NaN observation fails its row: NaN results, not an exception)
    try:
        for i in range(n):
            xs2, mask2, s2 = xs.clone(), mask.clone(), s.clone()
            xs2[i + 1:] = torch.randn(n - i - 1, obs, generator=gen, dtype=F64)
            if i + 2 < n:
                xs2[i + 2:] = float("nan")
            mask2[i + 1:] = ~mask[i + 1:]
            s2[i + 1:] = 3.0 * torch.rand(n - i - 1, obs, generator=gen, dtype=F64)
            other = call(ts, xs2, mask2, s2)
            assert all(_same_bits(a[:i + 1], b[:i + 1]) for a, b in zip(base[:5], other[:5])), i
            head = call(ts[:i + 1], xs[:i + 1], mask[:i + 1], s[:i + 1])
            assert all(_same_bits(a[:i + 1], b) for a, b in zip(base[:5], head[:5])), i
            assert _same_bits(head.state.mean, base.z_mean[i]) and _same_bits(head.state.cov, base.z_cov[i])
            assert float(head.loglik) == _seq_sum(base.logpdf[:i + 1].cpu())
    finally:
        cr.CHECK_POSITIVE_DEFINITE = True
    assert bool(torch.isfinite(base.logpdf).all())


# ---- 5. unobserved data --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("d,obs", [(5, 1), (5, 3), (8, 8)])
def test_unobserved_entries_are_never_read_and_unobserved_rows_change_nothing(d, obs):
    mats, series, _ = _case(d, obs, LENGTHS, _seed(d, obs), "both")
    Nm, Rm, Bm, Lm = mats
    m = _cuda_model(mats)
    ts, xs, ob, nv = _inputs(series, "both", F64)
    out = leg.filter_predictive_batch(m, ts, xs, lengths=list(LENGTHS), observed=ob, noise_var=nv)
    assert bool(torch.isnan(xs[~ob]).all()) and bool(torch.isnan(nv[~ob]).all())
    _, xs0, _, nv0 = _inputs(series, "both", F64, fill=0.25)
    out0 = leg.filter_predictive_batch(m, ts, xs0, lengths=list(LENGTHS), observed=ob, noise_var=nv0)
    assert all(_same_bits(a, b) for a, b in zip(out[:6], out0[:6])) and all(bool(torch.isfinite(t).all()) for t in out[:6])
    G = Nm @ Nm.T + Rm - Rm.T + 1e-5 * torch.eye(d, dtype=F64)
    LLT = Lm @ Lm.T + 1e-9 * torch.eye(obs, dtype=F64)
    parts = [_split(t.cpu(), LENGTHS) for t in out[:5]]
    seen = 0
    for b, (t1, _, mask, _) in enumerate(series):
        pm, pc, lp, zm, zc = (p[b] for p in parts)
        for i in (~mask.any(1)).nonzero().flatten().tolist():
            seen += 1
            assert float(lp[i]) == 0.0 and bool(torch.isfinite(pc[i]).all())
            if i == 0:                                   # the prior, exactly
                assert torch.equal(zm[0], torch.zeros(d, dtype=F64)) and torch.equal(zc[0], torch.eye(d, dtype=F64))
                assert torch.equal(pm[0], torch.zeros(obs, dtype=F64))
                continue
            E = torch.matrix_exp(-0.5 * (t1[i] - t1[i - 1]) * G)       # z_mean = m^-, z_cov = P^-
            assert float((zm[i] - E @ zm[i - 1]).abs().max()) <= 1e-12
            assert float((zc[i] - (torch.eye(d, dtype=F64) + E @ (zc[i - 1] - torch.eye(d, dtype=F64)) @ E.T)).abs().max()) <= 1e-12
            assert float((pm[i] - Bm @ zm[i]).abs().max()) <= 1e-12 * (1 + float(pm[i].abs().max()))
            assert float((pc[i] - (Bm @ zc[i] @ Bm.T + LLT)).abs().max()) <= 1e-12 * (1 + float(pc[i].abs().max()))
    assert seen >= 4


# ---- 6. continuing -------------------------------------------------------------------------------------------------------
def _assert_continues(tail, whole_rows, whole_state, whole_ll_tail, dtype, what):
    tol = 64 * EPS[dtype]
    for key, a, b in zip(ROWS + ("state mean", "state cov"), list(tail[:5]) + [tail.state.mean, tail.state.cov],
                         list(whole_rows) + [whole_state.mean, whole_state.cov]):
        a, b = a.cpu().to(F64), b.cpu().to(F64)
        err = float(((a - b).abs() / (1 + b.abs())).max())
        print("%s %s: %.2f eps" % (what, key, err / EPS[dtype]))
        assert err <= tol, (what, key, err)
    assert torch.equal(tail.state.t, whole_state.t)
    if whole_ll_tail is not None:
        a, b = tail.loglik.cpu(), whole_ll_tail
        assert bool(((a - b).abs() <= tol * b.abs().clamp_min(1.0) * 8).all())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("d,obs", [(5, 3), (8, 8), (1, 1)])
def test_a_series_continues_from_its_state(d, obs, dtype):
    n = 7
    _, mats = _model(d, obs, 100 + d)
    (ts, xs, mask, s), = _series(obs, [n], 101 + d)
    m = _cuda_model(mats, dtype)
    g = lambda t: t.to(dtype).cuda() if t.dtype != torch.bool else t.cuda()      # noqa: E731
    call = lambda lo, hi, init=None: leg.filter_predictive(m, g(ts[lo:hi]), g(xs[lo:hi]), observed=g(mask[lo:hi]),   # noqa: E731
                                                           noise_var=g(s[lo:hi]), init=init)
    whole = call(0, n)
    for h in (1, n - 1):
        head = call(0, h)
        assert isinstance(head.state, leg.FilterState)
        tail = call(h, n, head.state)
        _assert_continues(tail, [t[h:] for t in whole[:5]], whole.state, None, dtype, "h %d" % h)
        assert abs(float(head.loglik) + float(tail.loglik) - float(whole.loglik)) <= 64 * EPS[dtype] * n * max(1.0, abs(float(whole.loglik)))
    # a zero gap: the state at t_{h-1}, then a row at that same time that observes nothing, then the rows that follow --
    # against the whole series with that row in it (a zero gap inside a series), and against the series without it
    h = 3
    dup = lambda t, fill: torch.cat([t[:h], torch.full_like(t[h - 1:h], fill) if fill is not None else t[h - 1:h], t[h:]])   # noqa: E731
    ts2, xs2, mask2, s2 = dup(ts, None), dup(xs, float("nan")), dup(mask, False), dup(s, float("nan"))
    whole2 = leg.filter_predictive(m, g(ts2), g(xs2), observed=g(mask2), noise_var=g(s2))
    head = call(0, h)
    tail2 = leg.filter_predictive(m, g(ts2[h:]), g(xs2[h:]), observed=g(mask2[h:]), noise_var=g(s2[h:]), init=head.state)
    assert float(head.state.t) == float(g(ts2)[h])
    _assert_continues(tail2, [t[h:] for t in whole2[:5]], whole2.state, None, dtype, "zero gap")
    assert float(tail2.logpdf[0]) == 0.0 and _same_bits(tail2.z_mean[0], head.state.mean)
    _assert_continues(leg.FilterPredictive(*[t[1:] for t in tail2[:5]], tail2.loglik, tail2.state),
                      [t[h:] for t in whole[:5]], whole.state, None, dtype, "zero gap against the series without the row")


@pytest.mark.gpu
@pytest.mark.parametrize("models", [False, True])
def test_a_ragged_batch_continues_from_its_states(models):
    d, obs, lengths = 5, 2, [2, 3, 65, 7]
    heads = [1, 1, 32, 3]
    _, mats = _model(d, obs, 110)
    series = _series(obs, lengths, 111)
    cut = lambda lo_hi: [tuple(t[lo:hi] for t in sr) for sr, (lo, hi) in zip(series, lo_hi)]      # noqa: E731
    first, second = cut([(0, h) for h in heads]), cut([(h, n) for h, n in zip(heads, lengths)])
    if models:
        ms = [_cuda_model(mats), _cuda_model(_model(d, obs, 112)[1])]
        run = lambda sers, init=None: leg.filter_predictive_models(                               # noqa: E731
            ms, *_inputs(sers, "both", F64)[:2], lengths=[sr[0].shape[0] for sr in sers],
            observed=_inputs(sers, "both", F64)[2], noise_var=_inputs(sers, "both", F64)[3], init=init)
    else:
        m = _cuda_model(mats)
        run = lambda sers, init=None: leg.filter_predictive_batch(                                # noqa: E731
            m, *_inputs(sers, "both", F64)[:2], lengths=[sr[0].shape[0] for sr in sers],
            observed=_inputs(sers, "both", F64)[2], noise_var=_inputs(sers, "both", F64)[3], init=init)
    whole, head = run(series), run(first)
    tail = run(second, head.state)
    keep = torch.cat([torch.arange(n) >= h for h, n in zip(heads, lengths)]).cuda()
    rows = [t[:, keep] if models else t[keep] for t in whole[:5]]
    _assert_continues(tail, rows, whole.state, None, F64, "ragged batch")
    err = (head.loglik + tail.loglik - whole.loglik).abs() / whole.loglik.abs().clamp_min(1.0)
    assert bool((err <= 64 * EPS[F64] * max(lengths)).all())


# ---- 7. fp32 -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "both"])
@pytest.mark.parametrize("d,obs", [(1, 1), (5, 1), (5, 3), (8, 8)])
def test_fp32_is_as_accurate_as_the_recursion_in_torch(d, obs, mode):
    """The fp32 error of every output against the fp64 truth is at most 4x that of the same recursion evaluated by torch
    in fp32 on the same inputs (tests/_filterref.py), floor 64 eps32, relative to 1 + |value|, per output, max norm."""
    mats, series, truth = _case(d, obs, LENGTHS, _seed(d, obs), mode)
    m = _cuda_model(mats, F32)
    ts, xs, ob, nv = _inputs(series, mode, F32)
    out = leg.filter_predictive_batch(m, ts, xs, lengths=list(LENGTHS), observed=ob, noise_var=nv)
    assert all(t.dtype == F32 for t in out[:5]) and out.loglik.dtype == F64
    refs = [_filterref.filter_ref(mats, *_truth_args(sr, mode), dtype=F32) for sr in series]
    worst = 0.0
    for j, key in enumerate(ROWS + ("loglik",)):
        want = _cat(truth, key) if key != "loglik" else torch.stack([t["loglik"] for t in truth])
        ref = torch.cat([r[key] for r in refs]) if key != "loglik" else torch.stack([r["loglik"] for r in refs])
        scale = 1 + want.abs()
        e_lib = float(((out[j].cpu().to(F64).reshape(want.shape) - want).abs() / scale).max())
        e_ref = float(((ref.to(F64).reshape(want.shape) - want).abs() / scale).max())
        worst = max(worst, e_lib / max(e_ref, 64 * EPS[F32] / 4))
        print("fp32 d %d obs %d %s %s: library %.3e torch %.3e ratio %.2f" % (d, obs, mode, key, e_lib, e_ref,
                                                                             e_lib / max(e_ref, 1e-300)))
        assert e_lib <= max(4 * e_ref, 64 * EPS[F32]), (key, e_lib, e_ref)
    # the log-likelihood is the fp64 sum of the kernel's own fp32 terms
    for b, lp in enumerate(_split(out.logpdf.cpu().to(F64), LENGTHS)):
        assert abs(_seq_sum(lp) - float(out.loglik[b])) <= 1e-6 * max(1.0, abs(float(out.loglik[b])))
    print("fp32 d %d obs %d %s: worst error in units of max(torch's, 16 eps32): %.2f" % (d, obs, mode, worst))


# ---- 8. failures ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_failing_row_is_named_and_poisons_only_its_series_and_model():
    """A negative noise variance that makes S of one row of series 2 indefinite under model 1 (LLT = 0.36) and not under
    models 0 and 2 (LLT = 3600): an arithmetic failure, reported through the info word."""
    d, obs, lengths = 3, 1, [4, 6, 5]
    ms = []
    for k, lam in enumerate((60.0, 0.6, 60.0)):
        m, _ = _model(d, obs, 120 + k, F64, "cuda")
        ms.append(leg.LEGMatrices(m.N, m.R, m.B, torch.full((1, 1), lam, dtype=F64, device="cuda")))
    series = _series(obs, lengths, 121)
    ts, xs, _, s = _ragged(series, F64)
    clean = leg.filter_predictive_models(ms, ts, xs, lengths=lengths, noise_var=s)
    assert all(bool(torch.isfinite(t).all()) for t in clean[:6])
    start, local = sum(lengths[:2]), 2
    row = start + local
    s = s.clone()
    s[row] = -1000.0                                 # S = B P^- B^T + 0.36 - 1000 < 0 < B P^- B^T + 3600 - 1000
    assert cr.CHECK_POSITIVE_DEFINITE
    with pytest.raises(cr.NotPSDError) as e:
        leg.filter_predictive_batch(ms[1], ts, xs, lengths=lengths, noise_var=s)
    hit = re.search(r"series (\d+).*row (\d+)", str(e.value))
    assert hit and int(hit.group(1)) == 2 and int(hit.group(2)) == local, str(e.value)
    with pytest.raises(cr.NotPSDError) as e:
        leg.filter_predictive(ms[1], ts[start:], xs[start:], noise_var=s[start:])
    assert re.search(r"row %d" % local, str(e.value)), str(e.value)
    with pytest.raises(cr.NotPSDError) as e:
        leg.filter_predictive_models(ms, ts, xs, lengths=lengths, noise_var=s)
    hit = re.search(r"model (\d+).*series (\d+).*row (\d+)", str(e.value))
    assert hit and (int(hit.group(1)), int(hit.group(2)), int(hit.group(3))) == (1, 2, local), str(e.value)
    cr.CHECK_POSITIVE_DEFINITE = False
    try:
        out = leg.filter_predictive_models(ms, ts, xs, lengths=lengths, noise_var=s)
    finally:
        cr.CHECK_POSITIVE_DEFINITE = True
    for a, b in zip(out[:5], clean[:5]):
        assert bool(torch.isnan(a[1, row:]).all()), "the failed row and the rows after it"
        assert _same_bits(a[1, :row], b[1, :row])
        for k in (0, 2):                             # the other models see another S at that row, earlier rows are the same
            assert _same_bits(a[k, :row], b[k, :row]) and bool(torch.isfinite(a[k]).all())
    assert bool(torch.isnan(out.loglik[1, 2])) and bool(torch.isnan(out.state.mean[1, 2]).all()) and bool(torch.isnan(out.state.cov[1, 2]).all())
    assert _same_bits(out.loglik[1, :2], clean.loglik[1, :2]) and _same_bits(out.loglik[[0, 2], :2], clean.loglik[[0, 2], :2])
    assert bool(torch.isfinite(out.loglik[[0, 2]]).all())
    # every other series of every model is bit-identical to the clean call
    for a, b in zip(out[:5], clean[:5]):
        assert _same_bits(a[:, :start], b[:, :start])
    assert _same_bits(out.state.mean[:, :2], clean.state.mean[:, :2]) and _same_bits(out.state.cov[:, :2], clean.state.cov[:, :2])


# ---- 9. the boundary -------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_bound_and_exported():
    import ctypes
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "cgps.h")).read()
    assert re.search(r"\bint cgps_leg_filter\s*\(", header)
    assert "cgps_leg_filter" in _hip.exported_symbols()
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), "cgps_leg_filter")
    assert _hip.lib().cgps_version() == 320
    # argument errors come back as codes, before anything is launched
    lib = _hip.lib()
    none = [None] * 5
    assert lib.cgps_leg_filter(*none, 1, 1, 0, None, None, None, 2, 1, _hip.F64, None, None, None, *([None] * 10)) == 1
    assert lib.cgps_leg_filter(*none, 1, 1, 1, None, None, None, 2, 9, _hip.F64, None, None, None, *([None] * 10)) == 3
    assert lib.cgps_leg_filter(*none, 1, 1, 1, None, None, None, 2, 1, _hip.F64, None, None, None, *([None] * 10)) == 1
    assert b"cgps_leg_filter" in lib.cgps_last_error()
    assert lib.cgps_leg_filter(*none, 0, 0, 1, None, None, None, 2, 1, _hip.F64, None, None, None, *([None] * 10)) == 0

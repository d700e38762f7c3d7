"""Posterior and prior paths of many LEG series in one call (leg.posterior_perturbation_batch,
leg.sample_from_posterior_batch, leg.sample_from_prior_batch: DESIGN.md 4.19) against the float64 restatement of the
draw's definition (tests/_perturbref.py), series by series; position independence, bitwise on the right-hand side;
the distribution of the draws; errors and edges; replay from a HIP graph.

fp64 bound: LEG_TOL of tests/test_sample.py (rtol 1e-7, atol 1e-9), the project's bound for a sweep through a LEG factor
on operands assembled by two codes.  fp32 bound: four times the largest error of the one-series fp32
leg.sample_from_posterior against ITS fp64 reference on the same series (relative to max |x|): S right-hand sides of
norm ~ 1 / sqrt(gap) go through the same factor."""
import functools
import os

import numpy as np
import pytest
import torch

import _missref as mr
import _perturbref as pr
import _rngref
import _util
from oracle import cr_oracle as O
from cyclic_gps import _hip, leg
import cyclic_gps.cyclic_reduction as cr

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
LEG_TOL = dict(rtol=1e-7, atol=1e-9)
LENGTHS = [1, 2, 7, 33, 64, 65]                   # the last two put a row and a series boundary on the 64-lane edge
IDS = [5, 0, (1 << 24) - 1, 7, 123456, 3]
MODES = ["plain", "observed", "noise", "both"]
SMAX = 9


def _np(t):
    return t.detach().cpu().numpy()


def _model(d, obs, seed, dtype=F64):
    (Nm, Rm, Bm, Lm, _, _), _ = mr.leg_case(d, obs, 4, seed)
    return leg.LEGMatrices(*(t.to(dtype).cuda() for t in (Nm, Rm, Bm, Lm))), (Nm, Rm, Bm, Lm)


def _series(obs, lengths, seed):
    """Per series (fp64, CPU): ts, xs, mask [n, obs], variances [n, obs]; a series of five rows or more has its first,
    its last and an interior row wholly missing.  The series' times overlap and are not ordered across series."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for b, n in enumerate(lengths):
        ts = 3.0 - 1.1 * (b % 3) + torch.cumsum(0.2 + torch.rand(n, generator=gen, dtype=F64), 0)
        xs = torch.randn(n, obs, generator=gen, dtype=F64)
        mask = torch.rand(n, obs, generator=gen) < 0.7
        if n >= 5:
            mask[0] = mask[n - 1] = mask[n // 2] = False
        out.append((ts, xs, mask, 2.0 * torch.rand(n, obs, generator=gen, dtype=F64)))
    return out


def _mode(mode, mask, s):
    return (mask if mode in ("observed", "both") else None), (s if mode in ("noise", "both") else None)


def _ragged(series, dtype, mode, order=None):
    """(ts, xs, kwargs) of the concatenated batch on the GPU; xs and the variances hold NaN where nothing is observed."""
    order = range(len(series)) if order is None else order
    c = lambda k, dt: torch.cat([series[b][k] for b in order]).to(dt).cuda()       # noqa: E731
    ob, nv = _mode(mode, c(2, torch.bool), c(3, dtype))
    xs = c(1, dtype)
    if ob is not None:
        xs = torch.where(ob, xs, torch.full_like(xs, float("nan")))
        nv = None if nv is None else torch.where(ob, nv, torch.full_like(nv, float("nan")))
    return c(0, dtype), xs, dict(lengths=[series[b][0].shape[0] for b in order], observed=ob, noise_var=nv)


def _ref(mats, series, mode, ids, S, seed, stream=0, dtype=np.float64, prior=False):
    """Per series (rhs, x, K, v) of the restated definition."""
    G, Bm, LLT = pr.model(*(_np(t) for t in mats))
    out = []
    for (ts, xs, mask, s), k in zip(series, ids):
        ob, nv = _mode(mode, _np(mask), _np(s))
        out.append(pr.draws(G, Bm, LLT, _np(ts), _np(xs), k, S, seed, stream, ob, nv, prior, dtype))
    return out


def _cat(ref, k):
    return np.concatenate([r[k] for r in ref])


@functools.lru_cache(maxsize=None)
def _case(d):
    obs = 1 + d % 3
    m, mats = _model(d, obs, 70 + d)
    return obs, m, mats, _series(obs, LENGTHS, 500 + d), _series(obs, [33, 33, 33], 900 + d)


# ---- 1. against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 5, 8])
def test_rhs_and_draws_against_the_definition_fp64(d):
    """Ragged [1, 2, 7, 33, 64, 65] and dense [3, 33]; plain / observed / noise / both; default ids and
    [5, 0, 2^24 - 1, ...]; S in {1, 2, 3, 8, 9}: the 2-column generator groups, one and two solve panels, odd tails."""
    obs, m, mats, series, dense = _case(d)
    seed = 100 + d
    for mode in MODES:
        ts, xs, kw = _ragged(series, F64, mode)
        for ids in (None, IDS):
            ref = _ref(mats, series, mode, ids or range(len(series)), SMAX, seed)
            for S in ((1, 2, 3, 8, 9) if ids is None else (9,)):
                rhs = leg.posterior_perturbation_batch(m, ts, xs, S, seed, series_ids=ids, **kw)
                x = leg.sample_from_posterior_batch(m, ts, xs, S, seed, series_ids=ids, **kw)
                assert rhs.shape == x.shape == (sum(LENGTHS), d, S) and x.dtype == F64 and x.is_cuda and not x.requires_grad
                what = "d=%d %s ids=%s S=%d" % (d, mode, "default" if ids is None else "given", S)
                np.testing.assert_allclose(_np(rhs), _cat(ref, 0)[:, :, :S], err_msg=what + " rhs", **LEG_TOL)
                np.testing.assert_allclose(_np(x), _cat(ref, 1)[:, :, :S], err_msg=what + " draws", **LEG_TOL)
        # the dense layout, another stream
        st = lambda k, dt: torch.stack([sr[k] for sr in dense]).to(dt).cuda()          # noqa: E731
        ob, nv = _mode(mode, st(2, torch.bool), st(3, F64))
        ref = _ref(mats, dense, mode, range(3), SMAX, seed, stream=4)
        x = leg.sample_from_posterior_batch(m, st(0, F64), st(1, F64), SMAX, seed, observed=ob, noise_var=nv, stream=4)
        assert x.shape == (3, 33, d, SMAX)
        np.testing.assert_allclose(_np(x), np.stack([r[1] for r in ref]), err_msg="dense %s" % mode, **LEG_TOL)


def test_short_gaps_fp64():
    """One series with its gaps rescaled to gap |G|_1 ~ 1e-3: the float64 reference's own I - E E^T is still good to
    ~1e-13 there.  (Shorter gaps rest on gap_expm1 / gap_gram, tests/test_leg_gaps.py.)"""
    d = 3
    obs, m, mats, series, _ = _case(d)
    ts, xs, mask, s = series[3]
    g1 = float(m.G.abs().sum(0).max())
    ts = ts[0] + (ts - ts[0]) * (1e-3 / g1 / float((ts[1:] - ts[:-1]).mean()))
    short = [(ts, xs, mask, s)]
    for mode in MODES:
        t, x_, kw = _ragged(short, F64, mode)
        (rhs_ref, x_ref, _, _), = _ref(mats, short, mode, [9], SMAX, 31)
        rhs = leg.posterior_perturbation_batch(m, t, x_, SMAX, 31, series_ids=[9], **kw)
        x = leg.sample_from_posterior_batch(m, t, x_, SMAX, 31, series_ids=[9], **kw)
        np.testing.assert_allclose(_np(rhs), rhs_ref, err_msg=mode, **LEG_TOL)
        np.testing.assert_allclose(_np(x), x_ref, err_msg=mode, **LEG_TOL)


def _levels(eps, n):
    ms, offD, _, _ = _hip.level_layout(n)
    return [eps[offD[i]:offD[i + 1]] for i in range(len(ms))]


def _loop_error_fp32(m32, mats, series, mode, S, seed):
    """Largest |leg.sample_from_posterior (fp32) - its fp64 reference| over the series, and the largest |reference|:
    the reference is the oracle's back-substitution of the fp32 generator's noise through the factor of the fp64 CPU
    posterior system, as tests/test_sample.py builds it."""
    mc = leg.LEGMatrices(*mats)
    err = scale = 0.0
    for ts, xs, mask, s in series:
        n, d = ts.shape[0], mats[0].shape[0]
        ob, nv = _mode(mode, mask, s)
        K_Rs, K_Os, v = leg._posterior_system(mc, ts, xs, ob, nv)
        dec = O.decompose(K_Rs, K_Os)
        eps = torch.from_numpy(_rngref.standard_normal(n * d, S, seed, 0, np.float32)).reshape(n, d, S)
        cols = [O.backhalfsolve(dec, [lv[:, :, c] for lv in _levels(eps, n)]) for c in range(S)]
        ref = torch.stack(cols, dim=-1) + O.solve(dec, v).unsqueeze(-1)
        z = leg.sample_from_posterior(m32, ts.float().cuda(), xs.float().cuda(), S, seed,
                                      observed=None if ob is None else ob.cuda(), noise_var=None if nv is None else nv.float().cuda())
        err, scale = max(err, float((z.double().cpu() - ref).abs().max())), max(scale, float(ref.abs().max()))
    return err, scale


@pytest.mark.parametrize("d", [1, 3, 5, 8])
def test_draws_fp32_are_as_accurate_as_the_one_series_sampler(d):
    """fp32: the batched draws' largest error against the definition (relative to max |x|) is at most four times that
    of the one-series fp32 sampler against its own fp64 reference on the same series.
    Measured on an MI355X, largest relative error over the four modes, one-series sampler / batched draws:
    d = 1: 1.47e-6 / 1.28e-6;  d = 3: 1.98e-6 / 2.01e-6;  d = 5: 1.93e-6 / 2.93e-6;  d = 8: 7.16e-6 / 1.34e-5; the
    largest ratio within one mode is 2.17 (d = 8, observed=: 4.59e-6 / 9.94e-6) of the 4 allowed."""
    obs, _, mats, series, _ = _case(d)
    m32, _ = _model(d, obs, 70 + d, F32)
    S, seed = 8, 200 + d
    for mode in MODES:
        e_loop, s_loop = _loop_error_fp32(m32, mats, series, mode, S, seed)
        ts, xs, kw = _ragged(series, F32, mode)
        x = leg.sample_from_posterior_batch(m32, ts, xs, S, seed, **kw)
        assert x.dtype == F32
        ref = _cat(_ref(mats, series, mode, range(len(series)), S, seed, dtype=np.float32), 1)
        e_batch, s_batch = float(np.abs(_np(x).astype(np.float64) - ref).max()), float(np.abs(ref).max())
        print("d=%d %s: loop %.3e (relative %.3e), batched %.3e (relative %.3e)"
              % (d, mode, e_loop, e_loop / s_loop, e_batch, e_batch / s_batch))
        assert e_batch / s_batch <= 4 * e_loop / s_loop, (mode, e_batch / s_batch, e_loop / s_loop)


# ---- 2. position independence ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_a_series_draw_does_not_depend_on_its_batch(mode):
    d = 3
    obs, m, mats, series, dense = _case(d)
    seed, S = 11, 9
    ts, xs, kw = _ragged(series, F64, mode)
    rhs = leg.posterior_perturbation_batch(m, ts, xs, S, seed, series_ids=IDS, **kw)
    x = leg.sample_from_posterior_batch(m, ts, xs, S, seed, series_ids=IDS, **kw)
    starts = np.concatenate([[0], np.cumsum(LENGTHS)])
    for j, k in enumerate(IDS):                                             # alone, under its own id
        t1, x1, kw1 = _ragged([series[j]], F64, mode)
        alone = leg.posterior_perturbation_batch(m, t1, x1, S, seed, series_ids=[k], **kw1)
        assert torch.equal(alone, rhs[starts[j]:starts[j + 1]]), (mode, j)
        xa = leg.sample_from_posterior_batch(m, t1, x1, S, seed, series_ids=[k], **kw1)
        np.testing.assert_allclose(_np(xa), _np(x[starts[j]:starts[j + 1]]), err_msg="%s series %d" % (mode, j), **LEG_TOL)
    order = [4, 0, 5, 2, 1, 3]                                              # the batch reordered
    tp, xp, kwp = _ragged(series, F64, mode, order)
    perm = leg.posterior_perturbation_batch(m, tp, xp, S, seed, series_ids=[IDS[b] for b in order], **kwp)
    s0 = 0
    for b in order:
        assert torch.equal(perm[s0:s0 + LENGTHS[b]], rhs[starts[b]:starts[b + 1]]), (mode, b)
        s0 += LENGTHS[b]
    assert torch.equal(leg.posterior_perturbation_batch(m, ts, xs, 3, seed, series_ids=IDS, **kw), rhs[:, :, :3])
    # dense and ragged layouts
    st = lambda k_, dt: torch.stack([sr[k_] for sr in dense]).to(dt).cuda()            # noqa: E731
    ob, nv = _mode(mode, st(2, torch.bool), st(3, F64))
    dn = leg.posterior_perturbation_batch(m, st(0, F64), st(1, F64), S, seed, observed=ob, noise_var=nv)
    flat = lambda t: None if t is None else t.reshape((99,) + tuple(t.shape[2:]))      # noqa: E731
    rg = leg.posterior_perturbation_batch(m, flat(st(0, F64)), flat(st(1, F64)), S, seed, lengths=[33, 33, 33],
                                          observed=flat(ob), noise_var=flat(nv))
    assert dn.shape == (3, 33, d, S) and torch.equal(dn.reshape(99, d, S), rg)


# ---- 3. seeds, streams and ids ------------------------------------------------------------------------------------
def test_every_row_changes_with_the_seed_the_stream_and_the_id():
    obs, m, mats, series, _ = _case(3)
    ts, xs, kw = _ragged(series, F64, "both")
    base = leg.posterior_perturbation_batch(m, ts, xs, 3, 7, series_ids=IDS, **kw)
    others = [leg.posterior_perturbation_batch(m, ts, xs, 3, 8, series_ids=IDS, **kw),
              leg.posterior_perturbation_batch(m, ts, xs, 3, 7, series_ids=IDS, stream=2, **kw),
              leg.posterior_perturbation_batch(m, ts, xs, 3, 7, series_ids=[(k + 1) % (1 << 24) for k in IDS], **kw)]
    for o in others:
        assert bool((o != base).reshape(base.shape[0], -1).any(dim=1).all())
    assert torch.equal(base, leg.posterior_perturbation_batch(m, ts, xs, 3, 7, series_ids=torch.tensor(IDS), **kw))


# ---- 4. distribution ----------------------------------------------------------------------------------------------
def _golden_case():
    g = np.load(os.path.join(_util.GOLDEN, "leg_small_irregular.npz"))
    mats = tuple(torch.from_numpy(g[k]) for k in ("N", "R", "B", "Lambda"))
    lengths = [1, 4, 7]
    torch.manual_seed(1)
    series, s0 = [], 0
    for n in lengths:
        mask = torch.rand(n, 2) > 0.3
        series.append((torch.from_numpy(g["ts"][s0:s0 + n]), torch.from_numpy(g["xs"][s0:s0 + n]), mask, torch.zeros(n, 2, dtype=F64)))
        s0 += n
    return leg.LEGMatrices(*(t.cuda() for t in mats)), mats, lengths, series


def test_distribution_of_the_posterior_draws():
    """4096 draws, fixed seed: every entry of each series' sample covariance within six standard errors of dense
    K_b^-1 (Var of a product of two jointly normal variables: C_ii C_jj + C_ij^2, as test_covariance_sampled), every
    mean entry within six of K_b^-1 v_b, the cross-covariance between series 1 and 2 within six of zero.  The CPU
    reference alone gives worst entries of 1.91, 2.05, 2.61 (covariance) and 0.79, 1.96, 2.14 (mean) of the 6."""
    m, mats, lengths, series = _golden_case()
    S = 4096
    ts, xs, kw = _ragged(series, F64, "observed")
    x = leg.sample_from_posterior_batch(m, ts, xs, S, 2024, **kw).cpu()
    G, Bm, LLT = pr.model(*(_np(t) for t in mats))
    dev, diag, s0 = [], [], 0
    for b, (n, (t1, x1, mask, _)) in enumerate(zip(lengths, series)):
        terms = pr.series_terms(G, Bm, LLT, _np(t1), _np(mask))
        C = torch.from_numpy(np.linalg.inv(pr.dense_K(terms)))
        mu = C @ torch.from_numpy(pr.rhs_v(terms, Bm, _np(x1))).reshape(-1)
        X = x[s0:s0 + n].reshape(n * 3, S)
        D = X - mu[:, None]
        dg = torch.diagonal(C)
        worst = float(((D @ D.T / S - C).abs() / torch.sqrt((dg[:, None] * dg[None, :] + C * C) / S)).max())
        worst_mean = float(((X.mean(1) - mu).abs() / torch.sqrt(dg / S)).max())
        print("series %d: covariance %.2f, mean %.2f standard errors (bound 6)" % (b, worst, worst_mean))
        assert worst <= 6.0 and worst_mean <= 6.0, (b, worst, worst_mean)
        dev.append(D)
        diag.append(dg)
        s0 += n
    cross = float(((dev[1] @ dev[2].T / S).abs() / torch.sqrt(diag[1][:, None] * diag[2][None, :] / S)).max())
    print("series 1 x series 2: %.2f standard errors (bound 6)" % cross)
    assert cross <= 6.0, cross


# ---- 5. prior -----------------------------------------------------------------------------------------------------
def test_prior_paths():
    d = 3
    obs, m, mats, series, _ = _case(d)
    ts, _, _ = _ragged(series, F64, "plain")
    ref = _ref(mats, series, "plain", IDS, SMAX, 5, prior=True)
    z = leg.sample_from_prior_batch(m, ts, SMAX, 5, lengths=LENGTHS, series_ids=IDS)
    assert z.shape == (sum(LENGTHS), d, SMAX) and not z.requires_grad
    np.testing.assert_allclose(_np(z), _cat(ref, 1), **LEG_TOL)
    t6 = torch.sort(ts[:6])[0]
    zd = leg.sample_from_prior_batch(m, t6.reshape(2, 3), 3, 5)                      # dense: ids 0 and 1
    assert zd.shape == (2, 3, d, 3)
    np.testing.assert_allclose(_np(zd.reshape(6, d, 3)), _np(leg.sample_from_prior_batch(m, t6, 3, 5, lengths=[3, 3])), **LEG_TOL)
    # stationary with unit covariance: one row's sample covariance is the identity
    S = 4096
    X = leg.sample_from_prior_batch(m, ts, S, 2024, lengths=LENGTHS)[sum(LENGTHS[:3]) - 1].cpu()     # the last row of series 2
    se = torch.sqrt((1.0 + torch.eye(d, dtype=F64)) / S)
    worst = float(((X @ X.T / S - torch.eye(d, dtype=F64)).abs() / se).max())
    print("prior: one row's covariance within %.2f standard errors of I (bound 6)" % worst)
    assert worst <= 6.0, worst


# ---- 6. errors and edges -------------------------------------------------------------------------------------------
def test_errors_come_before_anything_runs_and_edges():
    d = 3
    obs, m, mats, series, _ = _case(d)
    ts, xs, kw = _ragged(series, F64, "both")
    post = leg.sample_from_posterior_batch
    e = post(m, ts[:0], xs[:0], 4, 1, lengths=[])
    assert e.shape == (0, d, 4) and e.dtype == F64
    assert post(m, ts[:0].reshape(0, 5), xs[:0].reshape(0, 5, obs), 4, 1).shape == (0, 5, d, 4)
    assert leg.posterior_perturbation_batch(m, ts[:0], xs[:0], 4, 1, lengths=[]).shape == (0, d, 4)
    assert leg.sample_from_prior_batch(m, ts[:0], 4, 1, lengths=[]).shape == (0, d, 4)
    bad = [lambda: post(m, ts, xs, 4, 1, series_ids=IDS[:-1], **kw),
           lambda: post(m, ts, xs, 4, 1, series_ids=IDS[:-1] + [1 << 24], **kw),
           lambda: post(m, ts, xs, 4, 1, series_ids=IDS[:-1] + [-1], **kw),
           lambda: post(m, ts, xs, 4, 1, lengths=LENGTHS, observed=kw["observed"][:-1]),
           lambda: post(m, ts, xs, 4, 1, lengths=LENGTHS, observed=torch.ones(sum(LENGTHS), obs + 1, dtype=torch.bool, device="cuda")),
           lambda: post(m, ts, xs, 0, 1, **kw),
           lambda: leg.sample_from_prior_batch(m, ts, 4, 1, lengths=LENGTHS, series_ids=[0]),
           lambda: leg.posterior_perturbation_batch(m, ts, xs, 4, 1, series_ids=[1 << 24] * 6, **kw)]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d did not raise" % k)
    # a zero-length gap inside series 2 is named; a zero or negative gap BETWEEN two series is fine
    assert cr.CHECK_POSITIVE_DEFINITE
    start = sum(LENGTHS[:2])
    tz = ts.clone()
    tz[start + 4] = tz[start + 3]
    for call in (lambda: post(m, tz, xs, 2, 1, **kw), lambda: leg.sample_from_prior_batch(m, tz, 2, 1, lengths=LENGTHS)):
        with pytest.raises(cr.NotPSDError, match=r"series 2.*row 3"):
            call()
    shifted, end = [], 0.0
    for b, (t, x_, mk, s) in enumerate(series):                       # series b starts at (b odd) or before the end of series b-1
        t2 = t - t[0] + (end - (0.5 if b and b % 2 == 0 else 0.0))
        shifted.append((t2, x_, mk, s))
        end = float(t2[-1])
    tsh, xsh, kwsh = _ragged(shifted, F64, "both")
    assert float(tsh[1] - tsh[0]) == 0.0 and float(tsh[3] - tsh[2]) < 0.0
    x = post(m, tsh, xsh, 3, 1, **kwsh)
    np.testing.assert_allclose(_np(x), _cat(_ref(mats, shifted, "both", range(6), 3, 1), 1), **LEG_TOL)
    # NaN at unobserved entries of xs and noise_var (what _ragged puts there) does not reach the output
    assert bool(torch.isnan(xs).any()) and bool(torch.isnan(kw["noise_var"]).any())
    clean = dict(kw, noise_var=torch.nan_to_num(kw["noise_var"], nan=0.3))
    rhs = leg.posterior_perturbation_batch(m, ts, xs, 3, 1, **kw)
    assert bool(torch.isfinite(rhs).all()) and bool(torch.isfinite(post(m, ts, xs, 3, 1, **kw)).all())
    assert torch.equal(rhs, leg.posterior_perturbation_batch(m, ts, torch.nan_to_num(xs, nan=-2.0), 3, 1, **clean))


def test_cpu_tensors_run_on_the_gpu_and_come_back():
    d = 3
    obs, m, mats, series, _ = _case(d)
    ts, xs, kw = _ragged(series, F64, "observed")
    x = leg.sample_from_posterior_batch(m, ts, xs, 3, 4, **kw)
    xc = leg.sample_from_posterior_batch(m.to("cpu"), ts.cpu(), xs.cpu(), 3, 4, lengths=LENGTHS, observed=kw["observed"].cpu())
    assert xc.device.type == "cpu" and torch.equal(xc, x.cpu())


# ---- 7. HIP graph -------------------------------------------------------------------------------------------------
def test_perturbation_replayed_from_a_hip_graph():
    """One ordinary call with the same lengths, then a linear capture (leg.Graphed: no parallel branches): the replay is
    bitwise the eager call, also after the data changed in place."""
    d = 3
    obs, m, mats, series, _ = _case(d)
    ts, xs, kw = _ragged(series, F64, "both")
    eager = leg.posterior_perturbation_batch(m, ts, xs, 5, 42, **kw)
    g = leg.Graphed(leg.posterior_perturbation_batch, m, ts, xs, 5, 42, **kw)
    assert torch.equal(g(), eager)
    xs.copy_(torch.where(torch.isnan(xs), xs, xs + 1.0))
    out = g()
    torch.cuda.synchronize()
    assert torch.equal(out, leg.posterior_perturbation_batch(m, ts, xs, 5, 42, **kw)) and not torch.equal(out, eager)

"""predict.laplace_predictions_batch and leg.glm_predictive against a dense truth that shares no kernel and
no precision block with the library: the mode by Rasmussen & Williams' algorithm 3.1 in covariance form
(tests/_laplaceref.py), the latent predictive at the targets by their eq. 3.24 on the prior covariance of rows and
targets together, and the response scale by the mpmath rule of tests/_glmpredictref.py at the truth's own (mu, v).

Bounds.  fp64: z_mean, z_cov, eta_mean and eta_var within rtol 1e-7 / atol 1e-9 of the truth; mean, var and logpdf within
the same bound of the rule at the truth's (mu, v).  fp32: max(4 x the composed path's fp32 error, 64 eps32 x the largest
entry), the project's convention.  The ABI of the new header and the argument errors run without a GPU.

Measured on an MI355X (worst error / bound): fp64 z_mean 0.043, z_cov 0.063, eta_mean 0.032, eta_var 0.0014, mean 3.1e-4,
var 1.7e-4, logpdf 5.1e-4; fp32 0.25."""
import ctypes

import pytest
import torch

import _gapref
import _glmpredictref as gp
import _laplaceref as lr
from cyclic_gps import _hip, leg, predict
from test_leg_laplace import ATOL64, EPS32, RTOL64, _composed, _declared, _model, _ragged

F64, F32 = torch.float64, torch.float32
NAMES = ("z_mean", "z_cov", "eta_mean", "eta_var", "mean", "var", "logpdf")
NO_TARGET = 1                                   # the series (of two rows) that has no target


# ---- CPU: where the declaration lives ----------------------------------------------------------------------------------
def test_the_prediction_header_declares_what_the_library_exports():
    assert _declared("cgps_glm_predict.h") == ["cgps_leg_glm_predict"]
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), "cgps_leg_glm_predict")
    assert _hip.glm_predict_symbols() == ["cgps_leg_glm_predict"]
    # the three other tables and the version are what they were
    assert sorted(_hip.exported_symbols()) == _declared("cgps.h") and _hip.extension_symbols() == _declared("cgps_glm.h")
    assert _hip.glm_gradient_symbols() == _declared("cgps_glm_grad.h") and _hip.lib().cgps_version() == 320
    # a call without operands is refused by name, on the host
    assert _hip.lib().cgps_leg_glm_predict(*([None] * 7), 1, 3, 2, _hip.F64, 0, *([None] * 6)) == 1
    assert b"zm = NULL" in _hip.lib().cgps_last_error()


# ---- the targets and their truth ---------------------------------------------------------------------------------------
def _targets(case):
    """per series: before the first row, exactly at the first row, between rows, exactly at an inner row, after the last;
    one series has no target"""
    out = []
    for b, sr in enumerate(case.series):
        t, n = sr["ts"], sr["ts"].shape[0]
        if b == NO_TARGET:
            out.append(t[:0])
        elif n == 1:
            out.append(torch.stack([t[0] - 0.7, t[0], t[0] + 0.9]))
        else:
            k = n // 2
            pts = [t[0] - 0.7, t[0], 0.5 * (t[0] + t[1]), t[k], 0.25 * t[n - 2] + 0.75 * t[n - 1], t[n - 1] + 0.9]
            if n > 100:
                pts[4:4] = [0.3 * t[70] + 0.7 * t[71], t[100]]
            out.append(torch.stack(pts))
    return out


def _target_data(case, targets, seed):
    """held-out values, their mask (a whole row absent now and then) and log_exposure / noise_var at the targets"""
    gen = torch.Generator().manual_seed(seed)
    obs = case.B.shape[0]
    P = sum(t.shape[0] for t in targets)
    if case.family == "poisson":
        ys = torch.poisson(torch.full((P, obs), 3.0, dtype=F64), generator=gen)
    elif case.family == "bernoulli":
        ys = (torch.rand(P, obs, generator=gen) < 0.5).to(F64)
    else:
        ys = torch.randn(P, obs, generator=gen, dtype=F64)
    mask = torch.rand(P, obs, generator=gen) < 0.7
    mask[2] = False
    le = 0.6 * torch.rand(P, obs, generator=gen, dtype=F64) - 0.3 if case.family == "poisson" else None
    nv = 0.1 + 1.9 * torch.rand(P, obs, generator=gen, dtype=F64) if case.family == "gaussian" else None
    return ys, mask, le, nv


def _latent_truth(case, b, target):
    """(mean [p, d], cov [p, d, d]) of the latent at the targets of series b: R&W eq. 3.24 with the mode's gradient and
    weights from the dense truth, on the prior covariance of the rows and the targets together"""
    sr, t = case.series[b], case.truths()[b]
    n, p, d = sr["ts"].shape[0], target.shape[0], case.N.shape[0]
    both, order = torch.sort(torch.cat([sr["ts"], target]), stable=True)
    where = torch.empty_like(order)
    where[order] = torch.arange(n + p)
    Sigma = _gapref.prior_covariance(both, case.G).reshape(n + p, d, n + p, d)
    rows, tg = where[:n], where[n:]
    Kss = Sigma[tg][:, :, tg].reshape(p * d, p * d)
    if t["y"].numel() == 0:
        cov = Kss.reshape(p, d, p, d)
        return torch.zeros(p, d, dtype=F64), cov[torch.arange(p), :, torch.arange(p), :]
    Ksf = Sigma[tg][:, :, rows].reshape(p * d, n * d) @ t["H"].T
    _, W = lr.grad_weight(case.family, t["y"], t["f"] + t["shift"], t["s"])
    sW = W.sqrt()
    L = torch.linalg.cholesky(torch.eye(W.numel(), dtype=F64) + sW[:, None] * t["C"] * sW[None, :])
    V = torch.linalg.solve_triangular(L, sW[:, None] * Ksf.T, upper=False)
    cov = (Kss - V.T @ V).reshape(p, d, p, d)
    return (Ksf @ t["g"]).reshape(p, d), cov[torch.arange(p), :, torch.arange(p), :]


def _truth(case, targets, ys, mask, le, nv):
    """the seven outputs of the call for the whole batch, fp64 CPU tensors; logpdf is zero at absent entries"""
    zm, zc = zip(*[_latent_truth(case, b, tg) for b, tg in enumerate(targets)])
    zm, zc = torch.cat(zm), torch.cat(zc)
    mu = zm @ case.B.T + case.offset + (le if le is not None else 0.0)
    v = torch.einsum("ca,pab,cb->pc", case.B, zc, case.B)
    mean, var, lp = torch.zeros_like(mu), torch.zeros_like(mu), torch.zeros_like(mu)
    for i in range(mu.shape[0]):
        for c in range(mu.shape[1]):
            ref = gp.outputs(case.family, float(ys[i, c]) if bool(mask[i, c]) else 0.0, float(mu[i, c]), float(v[i, c]),
                             None if nv is None else float(nv[i, c]))
            mean[i, c], var[i, c] = ref["mean"][0], ref["var"][0]
            if bool(mask[i, c]):
                lp[i, c] = ref["logpdf"][0]
    return [zm, zc, mu, v, mean, var, lp]


def _call(case, targets, ys, mask, le, nv, T, nan=True, **more):
    """the ragged call on the GPU; ``nan``: NaN at every absent entry of the data and of target_ys"""
    m = _model(case, T, "cuda")
    ts, ys_train, kw = _ragged(case, T, nan=nan)
    g = lambda t: None if t is None else t.to(T).cuda()      # noqa: E731
    tys = torch.where(mask, ys, torch.full_like(ys, float("nan"))) if nan else ys
    r = predict.laplace_predictions_batch(m, ts, ys_train, g(torch.cat(targets)), target_lengths=[t.shape[0] for t in targets],
                                          target_ys=g(tys), target_observed=mask.cuda(), target_log_exposure=g(le),
                                          target_noise_var=g(nv), **kw, **more)
    return r, (m, ts, ys_train, kw)


def _assert_fp64(got, want, what):
    for name, a, w in zip(NAMES, got, want):
        a = a.to("cpu", F64)
        assert a.shape == w.shape, (what, name, a.shape, w.shape)
        err = (a - w).abs()
        print("%s %s: worst error / bound %.3g" % (what, name, float((err / (ATOL64 + RTOL64 * w.abs())).max())))
        assert bool((err <= ATOL64 + RTOL64 * w.abs()).all()), (what, name, float(err.max()))


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["poisson", "bernoulli"])
@pytest.mark.parametrize("obs", lr.OBS_TRUTH)
@pytest.mark.parametrize("d", lr.RANKS_TRUTH)
def test_the_predictions_are_the_dense_truth_fp64(d, obs, family):
    """ragged lengths (1, 2, 6, 3, 131), targets before, at, between and after the rows, a series without a target, a series
    that observes nothing (the prior); then the dense layout of the same call on the series of six rows"""
    case = lr.batch_case(d, obs, family, lr.LENGTHS_TRUTH)
    targets = _targets(case)
    ys, mask, le, nv = _target_data(case, targets, 10 * d + obs)
    r, _ = _call(case, targets, ys, mask, le, nv, F64)
    assert bool(r.converged.all()) and r.converged.shape == (len(case.lengths),)
    want = _truth(case, targets, ys, mask, le, nv)
    _assert_fp64(r[:7], want, "d %d obs %d %s" % (d, obs, family))
    assert bool((r.logpdf[~mask.cuda()] == 0).all()) and bool(torch.isfinite(r.logpdf).all())
    # dense: two copies of the series of six rows with its own targets, [B, p] and [B, p, obs]
    b = case.lengths.index(6)
    s, k = sum(case.lengths[:b]), sum(t.shape[0] for t in targets[:b])
    p = targets[b].shape[0]
    m = _model(case, F64, "cuda")
    ts, ys_train, kw = _ragged(case, F64, which=[b, b])
    rep = lambda t: None if t is None else t[k:k + p].cuda().unsqueeze(0).expand(2, -1, -1)      # noqa: E731
    kw = {key: (v.reshape((2, 6) + v.shape[1:]) if key in ("observed", "log_exposure") else v) for key, v in kw.items() if key != "lengths"}
    rd = predict.laplace_predictions_batch(m, ts.reshape(2, 6), ys_train.reshape(2, 6, obs), targets[b].cuda(), target_ys=rep(ys),
                                           target_observed=rep(mask), target_log_exposure=rep(le), **kw)
    assert rd.z_mean.shape == (2, p, d) and rd.z_cov.shape == (2, p, d, d) and rd.logpdf.shape == (2, p, obs) and rd.converged.shape == (2,)
    for copy in range(2):
        _assert_fp64([t[copy] for t in rd[:7]], [w[k:k + p] for w in want], "dense copy %d" % copy)


@pytest.mark.gpu
def test_the_gaussian_family():
    case = lr.batch_case(3, 2, "gaussian", lr.LENGTHS_FORMS, 2)
    targets = _targets(case)
    ys, mask, le, nv = _target_data(case, targets, 5)
    r, _ = _call(case, targets, ys, mask, le, nv, F64)
    _assert_fp64(r[:7], _truth(case, targets, ys, mask, le, nv), "gaussian")


@pytest.mark.gpu
@pytest.mark.parametrize("family,d,obs", [("poisson", 5, 3), ("bernoulli", 3, 2), ("gaussian", 3, 2), ("bernoulli", 8, 8)])
def test_the_predictions_in_fp32(family, d, obs):
    """max(4 x the composed path's fp32 error, 64 eps32 x the largest entry) per output, against the fp64 truth"""
    case = lr.batch_case(d, obs, family, lr.LENGTHS_FP32, 2 if family == "gaussian" else 3)
    targets = _targets(case)
    ys, mask, le, nv = _target_data(case, targets, 7)
    want = _truth(case, targets, ys, mask, le, nv)
    r, _ = _call(case, targets, ys, mask, le, nv, F32)
    yard = _composed(lambda: _call(case, targets, ys, mask, le, nv, F32)[0])
    assert bool(r.converged.all())
    for name, a, y, w in zip(NAMES, r[:7], yard[:7], want):
        err, err_y = float((a.to("cpu", F64) - w).abs().max()), float((y.to("cpu", F64) - w).abs().max())
        bound = max(4 * err_y, 64 * EPS32 * float(w.abs().max()))
        print("fp32 %s %s: error %.3e, composed %.3e, bound %.3e" % (family, name, err, err_y, bound))
        assert err <= bound, (family, name, err, err_y, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["poisson", "bernoulli"])
def test_the_targets_are_the_posterior_of_the_extended_series(family):
    """a consistency check: the latent at targets that are not at a row is what ``laplace_posterior_batch`` says at the
    rows ``merge_targets`` inserts (wholly unobserved rows take part in the posterior)"""
    case = lr.batch_case(3, 2, family, lr.LENGTHS_FORMS, 1 if family == "poisson" else 3)
    m = _model(case, F64, "cuda")
    targets = [tg[[0, 2, 4, 5][:tg.shape[0] // 3 * 2]] for tg in _targets(case)]      # (0, 3 or 6 targets) not those at a row
    ts, ys, kw = _ragged(case, F64)
    le = kw.get("log_exposure")
    r = predict.laplace_predictions_batch(m, ts, ys, torch.cat(targets).cuda(), target_lengths=[t.shape[0] for t in targets], **kw)
    assert r.logpdf is None
    s = k = 0
    for b, n in enumerate(case.lengths):
        p = targets[b].shape[0]
        if p:
            ts_all, ys_all, obs_all, index = leg.merge_targets(ts[s:s + n], ys[s:s + n], targets[b].cuda())
            mask = torch.zeros(n + p, 2, dtype=torch.bool, device="cuda")
            mask[obs_all] = kw["observed"][s:s + n]
            le_all = None
            if le is not None:
                le_all = torch.zeros(n + p, 2, dtype=F64, device="cuda")
                le_all[obs_all] = le[s:s + n]
            q = leg.laplace_posterior(m, ts_all, torch.nan_to_num(ys_all), family, observed=mask, offset=kw["offset"], log_exposure=le_all)
            for got, w in ((r.z_mean[k:k + p], q.mean[index]), (r.z_cov[k:k + p], q.cov[0][index])):
                assert bool(((got - w).abs() <= ATOL64 + RTOL64 * w.abs()).all()), (family, b, float((got - w).abs().max()))
        s, k = s + n, k + p


@pytest.mark.gpu
def test_a_posterior_handed_in_runs_no_newton_step(monkeypatch):
    case = lr.batch_case(5, 3, "poisson", lr.LENGTHS_FORMS, 1)
    targets = _targets(case)
    ys, mask, le, nv = _target_data(case, targets, 3)
    r, (m, ts, ys_train, kw) = _call(case, targets, ys, mask, le, nv, F64)
    post = leg.laplace_posterior_batch(m, ts, ys_train, **kw)
    steps = []
    real = leg._glm_step
    monkeypatch.setattr(leg, "_glm_step", lambda *a: steps.append(1) or real(*a))
    again, _ = _call(case, targets, ys, mask, le, nv, F64, posterior=post)
    assert not steps
    for name, a, b in zip(NAMES + ("converged",), r, again):
        assert torch.equal(a, b), name
    _call(case, targets, ys, mask, le, nv, F64)
    assert steps                                                     # (the counter does count)
    # one series, from laplace_posterior
    b = case.lengths.index(6)
    s, n = sum(case.lengths[:b]), 6
    one = dict(observed=kw["observed"][s:s + n], offset=kw["offset"], log_exposure=kw["log_exposure"][s:s + n])
    del steps[:]
    p1 = leg.laplace_posterior(m, ts[s:s + n], ys_train[s:s + n], "poisson", **one)
    n_fit = len(steps)
    r1 = predict.laplace_predictions(m, ts[s:s + n], ys_train[s:s + n], targets[b].cuda(), "poisson", posterior=p1, **one)
    assert len(steps) == n_fit and r1.converged.dim() == 0 and r1.logpdf is None
    k = sum(t.shape[0] for t in targets[:b])
    for a, w in ((r1.z_mean, r.z_mean[k:k + targets[b].shape[0]]), (r1.z_cov, r.z_cov[k:k + targets[b].shape[0]])):
        assert bool(((a - w).abs() <= ATOL64 + RTOL64 * w.abs()).all())


@pytest.mark.gpu
def test_an_unconverged_series_still_predicts():
    case = lr.batch_case(3, 2, "poisson", lr.LENGTHS_FORMS, 1)
    targets = _targets(case)
    ys, mask, le, nv = _target_data(case, targets, 4)
    r, _ = _call(case, targets, ys, mask, le, nv, F64, max_iter=0)
    assert r.converged.shape == (len(case.lengths),) and not bool(r.converged.any())
    assert all(bool(torch.isfinite(t).all()) for t in r[:7]) and float(r.mean.min()) > 0
    # with no step taken the latent is the prior's: mean 0
    assert float(r.z_mean.abs().max()) == 0.0


@pytest.mark.gpu
def test_glm_predictive_takes_any_leading_shape():
    """in-sample posterior predictive checks from LaplacePosterior.mean and cov[0], dense layout [B, n, ...]"""
    case = lr.batch_case(3, 2, "bernoulli", (6, 6), 4)
    m = _model(case, F64, "cuda")
    ts, ys, kw = _ragged(case, F64)
    obs = kw["observed"].reshape(2, 6, 2)
    post = leg.laplace_posterior_batch(m, ts.reshape(2, 6), ys.reshape(2, 6, 2), None, "bernoulli", observed=obs, offset=kw["offset"])
    r = leg.glm_predictive(m, post.mean, post.cov[0], "bernoulli", offset=kw["offset"], ys=torch.nan_to_num(ys).reshape(2, 6, 2), observed=obs)
    assert all(t.shape == (2, 6, 2) for t in r)
    flat = leg.glm_predictive(m, post.mean.reshape(12, 3), post.cov[0].reshape(12, 3, 3), "bernoulli", offset=kw["offset"])
    assert flat.logpdf is None and torch.equal(flat.mean.reshape(2, 6, 2), r.mean)
    yard = _composed(lambda: leg.glm_predictive(m, post.mean, post.cov[0], "bernoulli", offset=kw["offset"],
                                                ys=torch.nan_to_num(ys).reshape(2, 6, 2), observed=obs))
    for a, b in zip(r, yard):
        assert bool(((a - b).abs() <= ATOL64 + RTOL64 * b.abs()).all())
    assert bool(((r.mean > 0) & (r.mean < 1) & (r.var > 0) & (r.logpdf <= 0)).all())


# ---- CPU: argument errors, before anything is launched ------------------------------------------------------------------
def test_argument_errors_come_before_anything_runs(monkeypatch):
    def launched(*a, **k):
        raise AssertionError("something was launched")
    for mod, name in ((leg, "_laplace_flat"), (leg, "_glm_predict"), (predict, "_intercast_models_hip")):
        monkeypatch.setattr(mod, name, launched)
    case = lr.batch_case(3, 2, "poisson", lr.LENGTHS_FORMS, 1)
    m = _model(case)
    lens = list(case.lengths)
    R, B = sum(lens), len(lens)
    ts, ys = torch.arange(R, dtype=F64), torch.zeros(R, 2, dtype=F64)
    tl = [2] * B
    P = sum(tl)
    tt = torch.arange(P, dtype=F64) + 0.5
    call = predict.laplace_predictions_batch
    ok = dict(lengths=lens, target_lengths=tl, family="poisson")
    z = lambda *s: torch.zeros(*s, dtype=F64)      # noqa: E731
    bad = [
        dict(ok, family="negbin"), dict(ok, family=None),
        dict(ok, family="gaussian", noise_var=z(R, 2)),                                # no target_noise_var
        dict(ok, target_noise_var=z(P, 2)), dict(ok, family="gaussian", noise_var=z(R, 2), target_noise_var=z(P, 2), target_log_exposure=z(P, 2)),
        dict(ok, target_lengths=None), dict(ok, target_lengths=tl[:-1]), dict(ok, target_lengths=[3] + tl[1:]),
        dict(ok, target_ys=z(P, 3)), dict(ok, target_ys=z(P + 1, 2)), dict(ok, target_ys=torch.zeros(P, 2, dtype=torch.int64)),
        dict(ok, target_observed=torch.ones(P, 2, dtype=torch.bool)),                   # without target_ys
        dict(ok, target_ys=z(P, 2), target_observed=z(P, 2)),                           # not bool
        dict(ok, target_log_exposure=z(P, 3)), dict(ok, offset=z(3)), dict(ok, max_iter=-1), dict(ok, log_exposure=z(R, 3)),
        dict(ok, posterior=(z(R, 3), z(R, 3, 3))),                                      # not a LaplacePosterior
        dict(ok, posterior=leg.LaplacePosterior(z(R + 1, 3), (z(R + 1, 3, 3), z(R, 3, 3)), None, None, torch.ones(B, dtype=torch.bool))),
    ]
    for k, kw in enumerate(bad):
        with pytest.raises(ValueError):
            call(m, ts, ys, tt, **kw)
            pytest.fail("case %d did not raise" % k)
    with pytest.raises(ValueError):
        call(m, ts.reshape(1, R), ys.reshape(1, R, 2), tt, target_lengths=tl, family="poisson")      # target_lengths in the dense layout
    with pytest.raises(ValueError):
        predict.laplace_predictions(m, ts, ys, tt.reshape(1, P), "poisson")
    for kw in (dict(ys=z(R, 3)), dict(observed=torch.ones(R, 2, dtype=torch.bool)), dict(noise_var=z(R, 2)), dict(offset=z(3))):
        with pytest.raises(ValueError):
            leg.glm_predictive(m, z(R, 3), z(R, 3, 3), "poisson", **kw)
    with pytest.raises(ValueError):
        leg.glm_predictive(m, z(R, 3), z(R, 2, 3), "poisson")
    # CPU tensors: there is no CPU path
    with pytest.raises(_hip.CgpsError):
        call(m, ts, ys, tt, **ok)
    with pytest.raises(_hip.CgpsError):
        leg.glm_predictive(m, z(R, 3), z(R, 3, 3), "poisson")
    # B = 0: empty results
    r = call(m, ts[:0], ys[:0], tt[:0], lengths=[], target_lengths=[], family="poisson")
    assert r.z_mean.shape == (0, 3) and r.mean.shape == (0, 2) and r.logpdf is None and r.converged.shape == (0,)

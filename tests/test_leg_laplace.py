"""The Laplace posterior for count, binary and Gaussian observations under a LEG prior (leg.laplace_posterior,
leg.laplace_posterior_batch, cgps_leg_glm_step: DESIGN.md 4.26) against the dense covariance-form truth of
tests/_laplaceref.py, which tests/test_laplaceref.py holds to its own checks on the same inputs.  The ABI of the new
header and the argument errors run without a GPU."""
import ctypes
import os
import re

import pytest
import torch

import _laplaceref as lr
from cyclic_gps import _hip, leg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = torch.float64, torch.float32
EPS32 = float(torch.finfo(F32).eps)
RTOL64, ATOL64 = 1e-7, 1e-9                    # the filter tests' fp64 bounds


# ---- CPU: where the declaration lives ----------------------------------------------------------------------------------
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cgps_[a-z_0-9]+)\s*\(", text)))


def test_the_extension_header_declares_what_the_library_exports():
    assert _declared("cgps_glm.h") == ["cgps_leg_glm_step"]
    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert hasattr(lib, "cgps_leg_glm_step")
    assert _hip.extension_symbols() == ["cgps_leg_glm_step"]
    # the first table and the version are what they were
    assert sorted(_hip.exported_symbols()) == _declared("cgps.h") and "cgps_leg_glm_step" not in _hip.exported_symbols()
    assert _hip.lib().cgps_version() == 320
    assert "CGPS_VERSION 320" in open(os.path.join(ROOT, "include", "cgps.h")).read()
    # a call without operands is refused by name, on the host
    null = [None] * 10
    assert _hip.lib().cgps_leg_glm_step(*null, 1, 1, 3, 2, _hip.F64, 0, 1e-9, *([None] * 6)) == 1
    assert b"z = NULL" in _hip.lib().cgps_last_error()


# ---- CPU: argument errors, before anything is launched ------------------------------------------------------------------
def _model(case, dtype=F64, device="cpu"):
    obs = case.B.shape[0]
    return leg.LEGMatrices(*(t.to(dtype).to(device) for t in (case.N, case.R, case.B, torch.eye(obs, dtype=F64))))


def test_argument_errors_come_before_anything_runs():
    case = lr.batch_case(3, 2, "poisson", lr.LENGTHS_FORMS, 1)
    m = _model(case)
    R = sum(case.lengths)
    ts, ys = torch.arange(R, dtype=F64), torch.zeros(R, 2, dtype=F64)
    lens = list(case.lengths)
    post = leg.laplace_posterior_batch
    bad = [
        lambda: post(m, ts, ys, lens, "negbin"),                                         # an unknown family
        lambda: post(m, ts, ys, lens),                                                   # no family at all
        lambda: post(m, ts, ys, lens, "gaussian"),                                       # no noise_var
        lambda: post(m, ts, ys, lens, "poisson", noise_var=torch.ones(R, 2, dtype=F64)),
        lambda: post(m, ts, ys[:, :1], lens, "poisson"),                                 # channels
        lambda: post(m, ts, ys, lens[:-1], "poisson"),                                   # lengths
        lambda: post(m, ts.reshape(1, R), ys, None, "poisson"),                          # dense layout, ragged ys
        lambda: post(m, ts, ys, lens, "poisson", observed=torch.ones(R, 2)),             # not bool
        lambda: post(m, ts, ys, lens, "poisson", observed=torch.ones(R + 1, 2, dtype=torch.bool)),
        lambda: post(m, ts, ys, lens, "poisson", offset=torch.zeros(3, dtype=F64)),
        lambda: post(m, ts, ys, lens, "poisson", log_exposure=torch.zeros(R, 3, dtype=F64)),
        lambda: post(m, ts, ys, lens, "gaussian", noise_var=torch.ones(R, 3, dtype=F64)),
        lambda: post(m, ts, ys, lens, "poisson", init=torch.zeros(R, 2, dtype=F64)),
        lambda: post(m, ts, ys, lens, "poisson", max_iter=-1),
        lambda: post(m, ts, ys, lens, "poisson", tol=-1.0),
        lambda: leg.laplace_posterior(m, ts.reshape(1, R), ys, "poisson"),
    ]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail("case %d did not raise" % k)
    wide = leg.LEGMatrices(case.N, case.R, torch.zeros(9, 3, dtype=F64), torch.eye(9, dtype=F64))
    with pytest.raises(ValueError, match="obs_dim"):
        post(wide, ts, torch.zeros(R, 9, dtype=F64), lens, "poisson")
    # CPU tensors: there is no CPU path
    with pytest.raises(_hip.CgpsError):
        post(m, ts, ys, lens, "poisson")
    # B = 0: empty tensors, both layouts
    r = post(m, ts[:0], ys[:0], [], "poisson")
    assert r.mean.shape == (0, 3) and r.cov[0].shape == (0, 3, 3) and r.log_evidence.shape == (0,)
    assert r.iterations.dtype == torch.int64 and r.converged.dtype == torch.bool
    r = post(m, torch.zeros(0, 4, dtype=F64), torch.zeros(0, 4, 2, dtype=F64), None, "bernoulli")
    assert r.mean.shape == (0, 4, 3) and r.cov[1].shape == (0, 3, 3, 3) and r.converged.shape == (0,)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _ragged(case, dtype, which=None, nan=False):
    """(ts, ys, kwargs) of the case's series (``which``: a selection, in that order) on the GPU; ``nan``: NaN at every
    unobserved entry of ys, log_exposure and noise_var."""
    series = case.series if which is None else [case.series[b] for b in which]
    cat = lambda k: torch.cat([sr[k] for sr in series])      # noqa: E731
    mask = cat("mask")
    put = lambda t: (torch.where(mask, t, torch.full_like(t, float("nan"))) if nan else t).to(dtype).cuda()      # noqa: E731
    kw = dict(lengths=[sr["ts"].shape[0] for sr in series], family=case.family, observed=mask.cuda(),
              offset=case.offset.to(dtype).cuda())
    if series[0]["log_exposure"] is not None:
        kw["log_exposure"] = put(cat("log_exposure"))
    if series[0]["noise_var"] is not None:
        kw["noise_var"] = put(cat("noise_var"))
    return cat("ts").to(dtype).cuda(), put(cat("ys")), kw


def _truth_arrays(case, which=None):
    """the truths of the series concatenated as the ragged result is: (mean, cov_diag, cov_off with zero blocks at the
    series boundaries, log_evidence)"""
    ts_ = case.truths() if which is None else [case.truths()[b] for b in which]
    d = case.N.shape[0]
    offs = []
    for k, t in enumerate(ts_):
        offs.append(t["cov_off"])
        if k + 1 < len(ts_):
            offs.append(torch.zeros(1, d, d, dtype=F64))
    return (torch.cat([t["mean"] for t in ts_]), torch.cat([t["cov_diag"] for t in ts_]), torch.cat(offs),
            torch.tensor([t["log_evidence"] for t in ts_], dtype=F64))


def _results(r):
    return [t.detach().to("cpu", F64) for t in (r.mean, r.cov[0], r.cov[1], r.log_evidence)]


NAMES = ("mean", "cov_diag", "cov_off", "log_evidence")


def _assert_fp64(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        err = (g - w).abs()
        print("%s %s: max abs error %.3e" % (what, name, float(err.max()) if err.numel() else 0.0))
        assert bool((err <= ATOL64 + RTOL64 * w.abs()).all()), (what, name, float(err.max()))


def _composed(fn):
    """fn() with the step composed from torch passes and ``cr.decompose_solve`` (the fp32 yardstick)"""
    old = os.environ.get("CGPS_LEG_GLM_COMPOSED")
    os.environ["CGPS_LEG_GLM_COMPOSED"] = "1"
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["CGPS_LEG_GLM_COMPOSED"]
        else:
            os.environ["CGPS_LEG_GLM_COMPOSED"] = old


def _assert_fp32(got, yard, want, what):
    """the project's fp32 convention: at most max(4 x the composed step's fp32 error, 64 eps32 x the largest entry)"""
    worst = 0.0
    for name, g, y, w in zip(NAMES, got, yard, want):
        err, err_y = float((g - w).abs().max()), float((y - w).abs().max())
        bound = max(4 * err_y, 64 * EPS32 * float(w.abs().max()))
        worst = max(worst, err / bound if bound > 0 else 0.0)
        print("%s %s: fp32 error %.3e, composed %.3e, bound %.3e" % (what, name, err, err_y, bound))
        assert err <= bound, (what, name, err, err_y, bound)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["poisson", "bernoulli"])
@pytest.mark.parametrize("obs", lr.OBS_TRUTH)
@pytest.mark.parametrize("d", lr.RANKS_TRUTH)
def test_the_batch_is_the_dense_truth_fp64(d, obs, family):
    """ragged lengths (1, 2, 6, 3, 131): a one-row series, a row that observes nothing, a series that observes nothing at
    all (mode 0, the prior covariance, evidence 0), a series of more than two strides of the workgroup"""
    case = lr.batch_case(d, obs, family, lr.LENGTHS_TRUTH)
    m = _model(case, F64, "cuda")
    ts, ys, kw = _ragged(case, F64)
    r = leg.laplace_posterior_batch(m, ts, ys, **kw)
    assert bool(r.converged.all()), (r.converged.tolist(), r.iterations.tolist())
    assert r.iterations.dtype == torch.int64 and r.converged.dtype == torch.bool and r.log_evidence.dtype == F64
    _assert_fp64(_results(r), _truth_arrays(case), "d %d obs %d %s" % (d, obs, family))
    dead = case.lengths.index(3)
    s = sum(case.lengths[:dead])
    assert float(r.mean[s:s + 3].abs().max()) == 0.0 and float(r.log_evidence[dead].abs()) <= 1e-12
    # the dense layout with a padded tail: every series padded to 131 rows that observe nothing, behind its own rows
    n = max(case.lengths)
    B = len(case.lengths)
    tsd = torch.zeros(B, n, dtype=F64, device="cuda")
    ysd = torch.full((B, n, obs), float("nan"), dtype=F64, device="cuda")
    maskd = torch.zeros(B, n, obs, dtype=torch.bool, device="cuda")
    led = torch.full((B, n, obs), float("nan"), dtype=F64, device="cuda")
    s = 0
    for b, k in enumerate(case.lengths):
        tsd[b, :k] = ts[s:s + k]
        tsd[b, k:] = ts[s + k - 1] + 0.5 * torch.arange(1, n - k + 1, dtype=F64, device="cuda")
        ysd[b, :k], maskd[b, :k] = ys[s:s + k], kw["observed"][s:s + k]
        if "log_exposure" in kw:
            led[b, :k] = kw["log_exposure"][s:s + k]
        s += k
    rd = leg.laplace_posterior_batch(m, tsd, ysd, None, family, observed=maskd, offset=kw["offset"],
                                     log_exposure=led if "log_exposure" in kw else None)
    assert rd.mean.shape == (B, n, d) and rd.cov[0].shape == (B, n, d, d) and rd.cov[1].shape == (B, n - 1, d, d)
    assert bool(rd.converged.all())
    s = 0
    for b, k in enumerate(case.lengths):
        close = lambda a, w: bool(((a - w).abs() <= ATOL64 + RTOL64 * w.abs()).all())      # noqa: E731
        assert close(rd.mean[b, :k], r.mean[s:s + k]) and close(rd.cov[0][b, :k], r.cov[0][s:s + k])
        assert close(rd.cov[1][b, :k - 1], r.cov[1][s:s + k - 1]) and close(rd.log_evidence[b], r.log_evidence[b])
        s += k


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("obs", range(1, 9))
@pytest.mark.parametrize("d", range(1, 9))
def test_every_compiled_form(d, obs, dtype):
    case = lr.batch_case(d, obs, "poisson", lr.LENGTHS_FORMS, 1)
    m = _model(case, dtype, "cuda")
    ts, ys, kw = _ragged(case, dtype)
    r = leg.laplace_posterior_batch(m, ts, ys, **kw)
    want = _truth_arrays(case)
    if dtype == F64:
        assert bool(r.converged.all()), (r.converged.tolist(), r.iterations.tolist())
        _assert_fp64(_results(r), want, "d %d obs %d" % (d, obs))
    else:
        yard = _composed(lambda: leg.laplace_posterior_batch(m, ts, ys, **kw))
        worst = _assert_fp32(_results(r), _results(yard), want, "d %d obs %d" % (d, obs))
        print("d %d obs %d: worst ratio to the fp32 bound %.3f" % (d, obs, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("d,obs", [(1, 1), (3, 2), (5, 3), (8, 8)])
def test_the_gaussian_family_is_exact(d, obs):
    case = lr.batch_case(d, obs, "gaussian", lr.LENGTHS_FORMS, 2)
    m = _model(case, F64, "cuda")
    ts, ys, kw = _ragged(case, F64)
    r = leg.laplace_posterior_batch(m, ts, ys, **kw)
    assert bool(r.converged.all()) and int(r.iterations.max()) <= 2, (r.converged.tolist(), r.iterations.tolist())
    means, diags, offs, evs = [], [], [], []
    for b, t in enumerate(case.truths()):                      # the closed form, not the iteration
        n = case.lengths[b]
        i = torch.arange(n)
        if t["f"].numel():
            mean, cov, ev = lr.gaussian_closed_form(t)
            cov = cov.reshape(n, d, n, d)
        else:
            mean, cov, ev = torch.zeros(n * d, dtype=F64), t["Sigma"].reshape(n, d, n, d), 0.0
        means.append(mean.reshape(n, d))
        diags.append(cov[i, :, i, :])
        offs.append(cov[i[1:], :, i[:-1], :])
        if b + 1 < len(case.lengths):
            offs.append(torch.zeros(1, d, d, dtype=F64))
        evs.append(ev)
    _assert_fp64(_results(r), (torch.cat(means), torch.cat(diags), torch.cat(offs), torch.tensor(evs, dtype=F64)),
                 "gaussian d %d obs %d" % (d, obs))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
def test_large_counts_converge_from_a_zero_start(dtype):
    """Poisson counts near 1000, zero offset, z = 0: the undamped step overflows e^eta (a candidate that is NaN or inf
    must be rejected), the damped iteration converges to the truth; started at the truth it converges in one step."""
    case = lr.damping_case()
    m = _model(case, dtype, "cuda")
    ts, ys, kw = _ragged(case, dtype)
    t = case.truths()[0]
    r = leg.laplace_posterior(m, ts, ys, case.family, observed=kw["observed"], offset=kw["offset"])
    assert r.log_evidence.dim() == 0 and r.converged.dim() == 0
    assert bool(r.converged), int(r.iterations)
    assert bool(torch.isfinite(r.mean).all()) and bool(torch.isfinite(r.log_evidence))
    want = (t["mean"], t["cov_diag"], t["cov_off"], torch.tensor(t["log_evidence"], dtype=F64))
    if dtype == F64:
        _assert_fp64(_results(r), want, "large counts")
    else:
        yard = _composed(lambda: leg.laplace_posterior(m, ts, ys, case.family, observed=kw["observed"], offset=kw["offset"]))
        _assert_fp32(_results(r), _results(yard), want, "large counts")
    r1 = leg.laplace_posterior(m, ts, ys, case.family, observed=kw["observed"], offset=kw["offset"],
                               init=t["mean"].to(dtype).cuda())
    assert bool(r1.converged) and int(r1.iterations) == 1, (bool(r1.converged), int(r1.iterations))


@pytest.mark.gpu
def test_a_series_does_not_depend_on_its_neighbours():
    """alone, first or last in a batch, and beside a series that needs more iterations (the frozen-series rule); NaN at
    unobserved entries of ys, log_exposure and noise_var changes nothing, bit for bit"""
    case = lr.independence_case()
    m = _model(case, F64, "cuda")
    n = case.lengths[0]
    runs = {}
    for name, which in (("alone", [0]), ("first", [0, 1, 2]), ("last", [2, 1, 0]), ("beside the slow one", [1, 0])):
        ts, ys, kw = _ragged(case, F64, which)
        r = leg.laplace_posterior_batch(m, ts, ys, **kw)
        assert bool(r.converged.all()), (name, r.iterations.tolist())
        k = which.index(0)
        s = sum(case.lengths[b] for b in which[:k])
        runs[name] = (r.mean[s:s + n], r.log_evidence[k], int(r.iterations[k]), r.iterations.tolist())
    print({k: v[3] for k, v in runs.items()})
    assert max(runs["first"][3]) > runs["first"][2] or max(runs["beside the slow one"][3]) > runs["alone"][2], \
        "no neighbour needed more iterations than the series itself: the case does not test the frozen-series rule"
    for name, (mean, ev, it, _) in runs.items():
        assert float((mean - runs["alone"][0]).abs().max()) <= 1e-10, name
        assert abs(float(ev) - float(runs["alone"][1])) <= 1e-10, name
    for cs in (lr.batch_case(3, 3, "poisson", lr.LENGTHS_FORMS, 1), lr.batch_case(3, 2, "gaussian", lr.LENGTHS_FORMS, 2)):
        mm = _model(cs, F64, "cuda")
        ts, ys, kw = _ragged(cs, F64)
        tsn, ysn, kwn = _ragged(cs, F64, nan=True)
        assert bool(torch.isnan(ysn).any())
        a, b = leg.laplace_posterior_batch(mm, ts, ys, **kw), leg.laplace_posterior_batch(mm, tsn, ysn, **kwn)
        for x, y in zip(_results(a) + [a.iterations, a.converged], _results(b) + [b.iterations, b.converged]):
            assert torch.equal(x, y)


# ---- the loop, end to end: the other families in fp32, the mirror image, max_iter, a stall ---------------------------------
def _fp32_against_the_truth(case, what):
    m = _model(case, F32, "cuda")
    ts, ys, kw = _ragged(case, F32)
    r = leg.laplace_posterior_batch(m, ts, ys, **kw)
    yard = _composed(lambda: leg.laplace_posterior_batch(m, ts, ys, **kw))
    worst = _assert_fp32(_results(r), _results(yard), _truth_arrays(case), what)
    print("%s: worst ratio to the fp32 bound %.3f, iterations %s" % (what, worst, r.iterations.tolist()))
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("d,obs", lr.FORMS_FP32)
def test_the_bernoulli_family_in_fp32(d, obs):
    _fp32_against_the_truth(lr.batch_case(d, obs, "bernoulli", lr.LENGTHS_FP32, 3), "bernoulli fp32 d %d obs %d" % (d, obs))


@pytest.mark.gpu
@pytest.mark.parametrize("d,obs", lr.FORMS_FP32)
def test_the_gaussian_family_in_fp32(d, obs):
    _fp32_against_the_truth(lr.batch_case(d, obs, "gaussian", lr.LENGTHS_FORMS, 2), "gaussian fp32 d %d obs %d" % (d, obs))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
def test_near_certain_events_and_their_mirror_image(dtype):
    """Bernoulli data with offsets near +8, and (1 - y, -offset, -B): the same posterior, so the same iteration.  Both
    converge, in the same number of steps per series, each to its own dense truth."""
    runs = []
    for mirrored in (False, True):
        case = lr.mirror_case(mirrored)
        what = "offsets near %s8" % ("-" if mirrored else "+")
        if dtype == F64:
            m = _model(case, F64, "cuda")
            ts, ys, kw = _ragged(case, F64)
            r = leg.laplace_posterior_batch(m, ts, ys, **kw)
            _assert_fp64(_results(r), _truth_arrays(case), what)
        else:
            r = _fp32_against_the_truth(case, what)
        assert bool(r.converged.all()), (what, r.converged.tolist(), r.iterations.tolist())
        runs.append(r)
    print("iterations", runs[0].iterations.tolist(), runs[1].iterations.tolist())
    assert runs[0].iterations.tolist() == runs[1].iterations.tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("start", ["zeros", "a point"])
def test_max_iter_0_returns_the_newton_system_at_init(start):
    """no step is taken: the mean is ``init`` bit for bit, cov the blocks of the dense J(init)^-1, and log_evidence
    psi(init) + (log|K| - log|J(init)|) / 2"""
    case = lr.batch_case(3, 2, "poisson", lr.LENGTHS_FORMS, 1)
    m = _model(case, F64, "cuda")
    ts, ys, kw = _ragged(case, F64)
    R = sum(case.lengths)
    init = None if start == "zeros" else 0.3 * torch.randn(R, 3, generator=torch.Generator().manual_seed(5), dtype=F64)
    r = leg.laplace_posterior_batch(m, ts, ys, max_iter=0, init=None if init is None else init.cuda(), **kw)
    z = torch.zeros(R, 3, dtype=F64) if init is None else init
    assert torch.equal(r.mean.cpu(), z)
    assert r.iterations.tolist() == [0] * len(case.lengths) and r.converged.tolist() == [False] * len(case.lengths)
    diags, offs, evs, s = [], [], [], 0
    for b, t in enumerate(case.truths()):
        n = case.lengths[b]
        cd, co, ev = lr.newton_system_at(t, case.family, z[s:s + n])
        diags.append(cd)
        offs.append(co)
        if b + 1 < len(case.lengths):
            offs.append(torch.zeros(1, 3, 3, dtype=F64))
        evs.append(ev)
        s += n
    _assert_fp64(_results(r), (z, torch.cat(diags), torch.cat(offs), torch.tensor(evs, dtype=F64)), "max_iter 0 from " + start)


@pytest.mark.gpu
def test_max_iter_runs_out_and_a_restart_carries_on():
    """two steps are not enough for the slow series of the independence case: it reports so; restarted from where it
    stopped it takes the steps that were left, and ends where one run ends"""
    case = lr.independence_case()
    m = _model(case, F64, "cuda")
    ts, ys, kw = _ragged(case, F64)
    full = leg.laplace_posterior_batch(m, ts, ys, max_iter=50, **kw)
    assert bool(full.converged.all())
    short = leg.laplace_posterior_batch(m, ts, ys, max_iter=2, **kw)
    assert not bool(short.converged[1]) and int(short.iterations[1]) == 2, (short.converged.tolist(), short.iterations.tolist())
    assert int(full.iterations[1]) > 2 and int(short.iterations.max()) <= 2
    rest = leg.laplace_posterior_batch(m, ts, ys, max_iter=48, init=short.mean, **kw)
    print("iterations: one run %s, two steps %s, the restart %s" % (full.iterations.tolist(), short.iterations.tolist(), rest.iterations.tolist()))
    assert bool(rest.converged.all())
    for b in range(len(case.lengths)):
        if not bool(short.converged[b]):
            assert int(short.iterations[b]) + int(rest.iterations[b]) == int(full.iterations[b]), b
    for a, w in zip(_results(rest), _results(full)):
        assert float((a - w).abs().max()) <= 1e-10 * max(1.0, float(w.abs().max()))


@pytest.mark.gpu
def test_counts_near_a_million_stall_from_zero_and_converge_from_a_warm_start():
    """twelve candidates reach counts of 10^4 from a zero start; at 10^6 the smallest candidate still puts eta
    near 500, nothing gains, and the series is flagged STALLED at its first step -- reported, finite, at z = 0.  With
    ``init`` = log(y + 1) mapped through B the same data converges to the dense truth."""
    case = lr.stall_case()
    m = _model(case, F64, "cuda")
    ts, ys, kw = _ragged(case, F64)
    r = leg.laplace_posterior_batch(m, ts, ys, **kw)
    assert r.converged.tolist() == [False] and r.iterations.tolist() == [1]
    assert float(r.mean.abs().max()) == 0.0
    assert all(bool(torch.isfinite(t).all()) for t in (r.mean, r.cov[0], r.cov[1], r.log_evidence))
    sr = case.series[0]
    init = torch.log(sr["ys"] + 1) @ torch.linalg.pinv(case.B).T              # B init = log(y + 1): obs <= d
    w = leg.laplace_posterior_batch(m, ts, ys, init=init.cuda(), **kw)
    assert bool(w.converged.all()), w.iterations.tolist()
    print("warm start: %d iterations" % int(w.iterations[0]))
    _assert_fp64(_results(w), _truth_arrays(case), "counts near 1e6 from a warm start")

"""Gradients through the LEG filter (``differentiable=True`` of leg.filter_predictive, leg.filter_predictive_batch and
leg.filter_predictive_models; cgps_leg_filter_adjoint: DESIGN.md 4.24) against autograd of the recursion in torch,
reference (a) of tests/_filtergradref.py, which tests/test_filtergradref.py holds to the dense Gaussian density.

Bound in fp64: the project's gradient bound of tests/test_gradients.py -- rtol 1e-7, atol 1e-10 x the largest reference
entry, per gradient tensor.  In fp32 (the sweep over every compiled form): the error against (a) in fp64, relative to the
largest reference entry, is at most max(4 x that of the explicit reverse walk (b) evaluated in fp32 in torch, 64 eps32) --
the 4 x and the floor are the convention of the filter's own tests."""
import functools
import os
import re

import pytest
import torch

import _filtergradref as fg
from cyclic_gps import leg
from test_filtergradref import autograd_of_a, check, reverse_walk
from test_leg_filter import EPS, F32, F64, LENGTHS, _inputs, _many_short_series, _truth_args
from test_leg_posterior_batch import MODES, _model, _series

cr = leg.cr
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_ROW = fg.KEYS
ALL = PER_ROW + ("loglik", "state_mean", "state_cov")
FORM_LENGTHS = (1, 2, 6, 3)
PAIRS = [(d, obs) for d in range(1, 9) for obs in range(1, 9)]
NAMES = ("N", "R", "B", "Lambda")


# ---- the harness ---------------------------------------------------------------------------------------------------------
def _cotangents(M, lengths, obs, d, seed, keys=ALL):
    """Random cotangents (fp64, CPU) in the shapes of ``filter_predictive_models``' results"""
    gen = torch.Generator().manual_seed(seed)
    R, B = sum(lengths), len(lengths)
    shapes = {"mean": (M, R, obs), "cov": (M, R, obs, obs), "logpdf": (M, R), "z_mean": (M, R, d), "z_cov": (M, R, d, d),
              "loglik": (M, B), "state_mean": (M, B, d), "state_cov": (M, B, d, d)}
    return {k: torch.randn(*shapes[k], generator=gen, dtype=F64) for k in keys}


def _states(series, M, d, seed, at_first=1):
    """Start states (t [B], mean [M, B, d], cov [M, B, d, d]), a little before every series' first row; series
    ``at_first``: AT its first row (a gap of zero)."""
    gen = torch.Generator().manual_seed(seed)
    B = len(series)
    t = torch.stack([sr[0][0] - (0.0 if b == at_first else 0.3 + 0.1 * b) for b, sr in enumerate(series)])
    W = torch.randn(M, B, d, d, generator=gen, dtype=F64)
    return t, torch.randn(M, B, d, generator=gen, dtype=F64), 0.5 * torch.eye(d, dtype=F64) + 0.1 * W @ W.transpose(-1, -2)


def _reference_grads(fn, mats_list, series, mode, init, cots, **kw):
    """The gradients of sum <cotangent, output> over the models and series from ``fn`` = ``autograd_of_a`` (reference (a)) or
    ``reverse_walk`` (reference (b), ``dtype=``), one call per (model, series), in the layout of ``_library_grads``."""
    lengths = [sr[0].shape[0] for sr in series]
    starts = [sum(lengths[:b]) for b in range(len(lengths))]
    out = {}
    rows = {"xs": [0] * len(series), "ts": [0] * len(series), "s": [0] * len(series)}
    t0 = [0] * len(series)
    m0 = [[None] * len(series) for _ in mats_list]
    P0 = [[None] * len(series) for _ in mats_list]
    for k, mats in enumerate(mats_list):
        acc = {n: 0 for n in NAMES}
        for b, sr in enumerate(series):
            ts, xs, s, mask = _truth_args(sr, mode)
            if mask is not None:
                xs = torch.where(mask, xs, torch.full_like(xs, float("nan")))
                s = None if s is None else torch.where(mask, s, torch.full_like(s, float("nan")))
            sl = slice(starts[b], starts[b] + lengths[b])
            cot = {key: cots[key][k, sl] for key in PER_ROW if key in cots}
            cot.update({key: cots[key][k, b] for key in ("loglik", "state_mean", "state_cov") if key in cots})
            st = None if init is None else (init[0][b], init[1][k, b], init[2][k, b])
            g = fn(mats, ts, xs, s, mask, st, cot, **kw)
            for n in NAMES:
                acc[n] = acc[n] + g[n].to(F64)
            for key in rows:
                if key in g:
                    rows[key][b] = rows[key][b] + g[key].to(F64)
            if st is not None:
                t0[b] = t0[b] + g["t0"].to(F64)
                m0[k][b], P0[k][b] = g["m0"].to(F64), g["P0"].to(F64)
        out.update({"%s%d" % (n, k): acc[n] for n in NAMES})
    out["xs"], out["ts"] = torch.cat(rows["xs"]), torch.cat(rows["ts"])
    if mode in ("noise", "both"):
        out["noise_var"] = torch.cat(rows["s"])
    if init is not None:
        out["init.t"] = torch.stack(t0)
        out["init.mean"] = torch.stack([torch.stack(r) for r in m0])
        out["init.cov"] = torch.stack([torch.stack(r) for r in P0])
    return out


def _library_grads(mats_list, series, mode, init, cots, dtype=F64, chunk_rows=None, fill=float("nan")):
    """The same gradients from ``filter_predictive_models(differentiable=True)`` and ``backward`` (and the call's result)."""
    lengths = [sr[0].shape[0] for sr in series]
    leaf = lambda t: t.detach().to(dtype).cuda().requires_grad_(True)      # noqa: E731
    ms = [leg.LEGMatrices(*(leaf(t) for t in mats)) for mats in mats_list]
    ts, xs, ob, nv = _inputs(series, mode, dtype, fill)
    ts, xs = ts.requires_grad_(True), xs.requires_grad_(True)
    nv = None if nv is None else nv.requires_grad_(True)
    st = None if init is None else leg.FilterState(*(leaf(t) for t in init))
    out = leg.filter_predictive_models(ms, ts, xs, lengths=lengths, observed=ob, noise_var=nv, init=st, chunk_rows=chunk_rows,
                                       differentiable=True)
    outs = dict(zip(PER_ROW + ("loglik",), out[:6]), state_mean=out.state.mean, state_cov=out.state.cov)
    total = sum((cots[key].to(outs[key].dtype).cuda() * outs[key]).sum().to(F64) for key in cots)
    total.backward()
    got = {"%s%d" % (n, k): getattr(m, n).grad for k, m in enumerate(ms) for n in NAMES}
    got.update(xs=xs.grad, ts=ts.grad)
    if nv is not None:
        got["noise_var"] = nv.grad
    if st is not None:
        got.update({"init.t": st.t.grad, "init.mean": st.mean.grad, "init.cov": st.cov.grad})
    return got, out, (xs, nv, ob)


def _rel_err(got, want):
    want = want.detach().to("cpu", F64)
    scale = float(want.abs().max()) if want.numel() else 0.0
    return float((got.detach().to("cpu", F64) - want).abs().max()) / scale if scale > 0 else float(got.detach().abs().max())


def _assert_grads(got, want, what):
    assert set(got) == set(want), (sorted(got), sorted(want))
    worst = max((_rel_err(got[k], want[k]), k) for k in want)
    print("filter grad %s: worst error %.3e of the largest reference entry (%s)" % (what, worst[0], worst[1]))
    for k in want:
        assert got[k] is not None, (what, k)
        check(got[k], want[k], "%s: %s" % (what, k))
    return worst[0]


@functools.lru_cache(maxsize=None)
def _grid_case(d, obs, mode, with_init):
    """Two models, the ragged batch [1, 2, 3, 65, 7], random cotangents on everything; reference (a), computed once."""
    mats_list = [_model(d, obs, 400 + 10 * d + obs)[1], _model(d, obs, 70)[1]]
    series = _series(obs, list(LENGTHS), 401 + 10 * d + obs)
    init = _states(series, 2, d, 5) if with_init else None
    cots = _cotangents(2, list(LENGTHS), obs, d, 6)
    return mats_list, series, init, cots, _reference_grads(autograd_of_a, mats_list, series, mode, init, cots)


# ---- 1. fp64, all outputs ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("with_init", [False, True], ids=["prior", "init"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d,obs", [(d, obs) for d in (1, 5, 8) for obs in (1, 2, 3, 8)])
def test_every_gradient_against_autograd_of_the_recursion(d, obs, mode, with_init):
    """Worst measured on an MI355X over the grid: see DESIGN.md 4.24."""
    mats_list, series, init, cots, want = _grid_case(d, obs, mode, with_init)
    if with_init:
        assert float(init[0][1] - series[1][0][0]) == 0.0
    got, _, _ = _library_grads(mats_list, series, mode, init, cots)
    _assert_grads(got, want, "d %d obs %d %s %s" % (d, obs, mode, "init" if with_init else "prior"))


# ---- 2. more than one workgroup, lanes leaving at different rows -----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("obs", [1, 3])
def test_many_short_series_and_a_permutation(obs):
    d, B = 5, 70
    mats_list = [_model(d, obs, 55)[1]]
    lengths, series = _many_short_series(obs, B, 56)
    assert set(lengths) == {1, 2, 3, 4}
    cots = _cotangents(1, lengths, obs, d, 7)
    want = _reference_grads(autograd_of_a, mats_list, series, "both", None, cots)
    got, _, _ = _library_grads(mats_list, series, "both", None, cots)
    _assert_grads(got, want, "70 series d 5 obs %d" % obs)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(5)).tolist()
    pcots = {key: (torch.cat([torch.split(t, lengths, dim=1)[b] for b in perm], 1) if key in PER_ROW else t[:, perm])
             for key, t in cots.items()}
    pgot, _, _ = _library_grads(mats_list, [series[b] for b in perm], "both", None, pcots)
    parts = torch.split(got["xs"], lengths)
    assert torch.equal(torch.cat([parts[b] for b in perm]), pgot["xs"])
    parts = torch.split(got["noise_var"], lengths)
    assert torch.equal(torch.cat([parts[b] for b in perm]), pgot["noise_var"])


# ---- 3. loglik alone, against the smoother's path ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("obs", [1, 3])
def test_loglik_gradients_agree_with_log_likelihood_batch(obs):
    d = 5
    mats = _model(d, obs, 430 + obs)[1]
    series = _series(obs, list(LENGTHS), 431 + obs)
    grads = []
    for call in ("filter", "smoother"):
        m = leg.LEGMatrices(*(t.clone().cuda().requires_grad_(True) for t in mats))
        ts, xs, ob, nv = _inputs(series, "both", F64, fill=0.25)
        ts, xs, nv = ts.requires_grad_(True), xs.requires_grad_(True), nv.requires_grad_(True)
        kw = dict(lengths=list(LENGTHS), observed=ob, noise_var=nv)
        if call == "filter":
            ll = leg.filter_predictive_batch(m, ts, xs, differentiable=True, **kw).loglik
        else:
            ll = leg.log_likelihood_batch(m, ts, xs, **kw)
        ll.sum().backward()
        grads.append((ll.detach(), {n: getattr(m, n).grad for n in NAMES}, {"xs": xs.grad, "ts": ts.grad, "noise_var": nv.grad}))
    (ll_f, gm_f, gd_f), (ll_s, gm_s, gd_s) = grads
    assert float(((ll_f - ll_s).abs() / ll_s.abs().clamp_min(1.0)).max()) <= 1e-9
    worst = 0.0
    for n in NAMES:
        worst = max(worst, _rel_err(gm_f[n], gm_s[n]))
        check(gm_f[n], gm_s[n], "loglik obs %d: %s" % (obs, n))
    for key, g in gd_s.items():
        assert gd_f[key] is not None
        if g is not None:                              # (what the smoother's path differentiates)
            worst = max(worst, _rel_err(gd_f[key], g))
            check(gd_f[key], g, "loglik obs %d: %s" % (obs, key))
    print("filter grad loglik against log_likelihood_batch d 5 obs %d: worst %.3e" % (obs, worst))


# ---- 4. every compiled form ------------------------------------------------------------------------------------------------
def _form_seed(d, obs):
    return 700 + 10 * d + obs


@functools.lru_cache(maxsize=None)
def _form_case(d, obs, mode):
    """The batch of tests/test_leg_channel_forms.py (same seeds, same masks) with cotangents on loglik and z_mean"""
    mats_list = [_model(d, obs, _form_seed(d, obs))[1]]
    series = _series(obs, list(FORM_LENGTHS), _form_seed(d, obs) + 1)
    cots = _cotangents(1, list(FORM_LENGTHS), obs, d, 8, keys=("loglik", "z_mean"))
    return mats_list, series, cots, _reference_grads(autograd_of_a, mats_list, series, mode, None, cots)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("d,obs", PAIRS)
def test_every_compiled_form(d, obs, dtype):
    """Worst ratio measured on an MI355X: see DESIGN.md 4.24."""
    for mode in ("plain", "both"):
        mats_list, series, cots, want = _form_case(d, obs, mode)
        six = series[2][2]
        assert six.shape[0] == 6 and not bool(six[[0, 3, 5]].any())
        got, _, (xs, nv, ob) = _library_grads(mats_list, series, mode, None, cots, dtype)
        if mode == "both":
            assert bool(torch.isnan(xs[~ob]).all()) and bool(torch.isnan(nv[~ob]).all())
        what = "form %s d %d obs %d %s" % ("fp64" if dtype == F64 else "fp32", d, obs, mode)
        if dtype == F64:
            _assert_grads(got, want, what)
            continue
        walk = _reference_grads(reverse_walk, mats_list, series, mode, None, cots, dtype=dtype)
        floor, worst = 64 * EPS[F32], (0.0, "")
        for k in want:
            e_lib, e_ref = _rel_err(got[k], want[k]), _rel_err(walk[k], want[k])
            worst = max(worst, (e_lib / max(4 * e_ref, floor), k))
            print("filter grad %s %s: error %.3e, the walk in torch %.3e, floor %.3e" % (what, k, e_lib, e_ref, floor))
        print("filter grad %s: worst ratio to the bound %.3f (%s)" % (what, worst[0], worst[1]))
        for k in want:
            assert _rel_err(got[k], want[k]) <= max(4 * _rel_err(walk[k], want[k]), floor), (what, k)


def test_the_sweep_covers_every_compiled_channel_form():
    """dispatch_obs maps obs to the compile-time O of leg_filter_adjoint_kernel: 1, 2, 3, 4 -> themselves, everything else
    -> 8.  A new form fails this until the sweep above runs it."""
    text = open(os.path.join(ROOT, "cyclic-gps_amd", "csrc", "cgps_host.h")).read()
    body = re.search(r"void dispatch_obs\(int obs, Fn&& fn\) \{\n  switch \(obs\) \{\n(.*?)\n  \}\n\}", text, re.S)
    assert body, "dispatch_obs not found in cgps_host.h"
    forms = {}
    for l in (l.strip() for l in body.group(1).splitlines() if l.strip()):
        hit = re.fullmatch(r"(case (\d+)|default): fn\(std::integral_constant<int, (\d+)>\{\}\); break;", l)
        assert hit, "a line of dispatch_obs this test does not understand: %r" % l
        forms[int(hit.group(2)) if hit.group(2) else "default"] = int(hit.group(3))
    assert forms == {1: 1, 2: 2, 3: 3, 4: 4, "default": 8}, forms
    assert {obs for _, obs in PAIRS} == set(range(1, 9)) and {d for d, _ in PAIRS} == set(range(1, 9)) and len(PAIRS) == 64
    unit = open(os.path.join(ROOT, "cyclic-gps_amd", "csrc", "cgps_leg_filter_adjoint.h")).read()
    assert "cgps_host::dispatch_obs(obs" in unit


# ---- 5. exact statements -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_exact_statements():
    d, obs = 5, 3
    mats_list, series, init, cots, _ = _grid_case(d, obs, "both", True)
    got, out, (xs, nv, ob) = _library_grads(mats_list[:1], series, "both", (init[0], init[1][:1], init[2][:1]),
                                            {k: v[:1] for k, v in cots.items()})
    assert all(t.grad_fn is not None for t in out[:6]) and out.state.mean.grad_fn is not None and out.state.cov.grad_fn is not None
    # the forward values are those of the default call, bit for bit
    ms = [leg.LEGMatrices(*(t.cuda() for t in mats_list[0]))]
    st = leg.FilterState(init[0].cuda(), init[1][:1].cuda(), init[2][:1].cuda())
    kw = dict(lengths=list(LENGTHS), observed=ob, noise_var=nv.detach(), init=st)
    plain = leg.filter_predictive_models(ms, _inputs(series, "both", F64)[0], xs.detach(), **kw)
    for a, b in zip(out[:6] + tuple(out.state), plain[:6] + tuple(plain.state)):
        assert torch.equal(a.detach(), b)
    # unobserved entries: NaN in, exactly zero gradient out
    assert bool((~ob).any()) and bool(torch.isnan(xs[~ob]).all()) and bool(torch.isnan(nv[~ob]).all())
    assert bool((got["xs"][~ob] == 0).all()) and bool((got["noise_var"][~ob] == 0).all())
    assert bool(torch.isfinite(got["xs"]).all()) and bool(torch.isfinite(got["noise_var"]).all())
    # nothing requires grad: no graph
    res = leg.filter_predictive_models(ms, _inputs(series, "both", F64)[0], xs.detach(), differentiable=True, **kw)
    assert all(t.grad_fn is None and not t.requires_grad for t in res[:6] + tuple(res.state))
    res = leg.filter_predictive_batch(ms[0], _inputs(series, "both", F64)[0], xs.detach(), differentiable=True,
                                      **dict(kw, init=leg.FilterState(st.t, st.mean[0], st.cov[0])))
    assert all(t.grad_fn is None and not t.requires_grad for t in res[:6] + tuple(res.state))
    # under no_grad the keyword builds no graph either
    m = leg.LEGMatrices(*(t.cuda().requires_grad_(True) for t in mats_list[0]))
    with torch.no_grad():
        res = leg.filter_predictive_batch(m, _inputs(series, "both", F64)[0], xs.detach(), lengths=list(LENGTHS), observed=ob,
                                          noise_var=nv.detach(), differentiable=True)
    assert all(t.grad_fn is None for t in res[:6])
    # ... and the default never does
    res = leg.filter_predictive_batch(m, _inputs(series, "both", F64)[0], xs.detach(), lengths=list(LENGTHS), observed=ob,
                                      noise_var=nv.detach())
    assert all(t.grad_fn is None for t in res[:6])


# ---- 6. the time-parallel forward, the serial backward -------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("with_init", [False, True], ids=["prior", "init"])
def test_chunk_rows_with_differentiable(with_init):
    d, obs = 5, 3
    mats_list, series, init, cots, want = _grid_case(d, obs, "both", with_init)
    got, _, _ = _library_grads(mats_list, series, "both", init, cots, chunk_rows=(4, 2))
    _assert_grads(got, want, "chunk_rows (4, 2) d 5 obs 3 both %s" % ("init" if with_init else "prior"))


# ---- 7. finite differences ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gradcheck():
    d, obs, n = 2, 1, 3
    mats = _model(d, obs, 91)[1]
    ts, xs, _, s = _series(obs, [n], 92)[0]
    t0, m0, P0 = _states([(ts, xs, None, s)], 1, d, 93, at_first=-1)
    leaf = lambda t: t.clone().cuda().requires_grad_(True)      # noqa: E731
    inputs = tuple(leaf(t) for t in mats + (xs, ts, s, m0[0, 0]))

    def fn(Nm, Rm, Bm, Lm, xs_, ts_, nv_, mean0):
        out = leg.filter_predictive(leg.LEGMatrices(Nm, Rm, Bm, Lm), ts_, xs_, noise_var=nv_,
                                    init=leg.FilterState(t0[0].cuda(), mean0, P0[0, 0].cuda()), differentiable=True)
        return out[:6] + (out.state.mean, out.state.cov)

    assert torch.autograd.gradcheck(fn, inputs)


# ---- 8. a failed series stays contained ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_failed_series_has_nan_gradients_and_the_others_are_untouched():
    """A NaN result of the arithmetic (a negative variance makes S of one row indefinite), reported as values."""
    d, obs, lengths = 3, 1, [4, 6, 5]
    m0, _ = _model(d, obs, 121, F64, "cuda")
    lam = torch.full((1, 1), 0.6, dtype=F64, device="cuda")
    series = _series(obs, lengths, 121)
    grads = []
    for keep in ([0, 1, 2], [0, 1]):
        m = leg.LEGMatrices(m0.N, m0.R, m0.B, lam)
        ts, xs, _, s = _inputs([series[b] for b in keep], "noise", F64)
        if 2 in keep:
            s = s.clone()
            s[sum(lengths[:2]) + 2] = -1000.0
        xs = xs.requires_grad_(True)
        cr.CHECK_POSITIVE_DEFINITE = False
        try:
            out = leg.filter_predictive_batch(m, ts, xs, lengths=[lengths[b] for b in keep], noise_var=s, differentiable=True)
            out.loglik.sum().backward()
        finally:
            cr.CHECK_POSITIVE_DEFINITE = True
        grads.append((xs.grad, out.loglik.detach()))
    (g3, ll3), (g2, _) = grads
    start = sum(lengths[:2])
    assert bool(torch.isnan(ll3[2])) and bool(torch.isfinite(ll3[:2]).all())
    assert bool(torch.isnan(g3[start:]).all())
    assert bool(torch.isfinite(g3[:start]).all())
    check(g3[:start], g2, "the two series next to the failed one")

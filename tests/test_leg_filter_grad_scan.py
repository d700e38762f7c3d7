"""The time-parallel backward of the LEG filter (``backward_chunk_rows=`` of leg.filter_predictive, filter_predictive_batch
and filter_predictive_models): cgps_leg_filter_adjoint over chunks, the chunks' affine maps measured by
the entry itself and linked by ``leg._filter_link_scan``.

Bounds.  fp64: the bound of tests/test_leg_filter_grad.py -- rtol 1e-7, atol 1e-10 x the largest reference entry, per
gradient tensor -- against autograd of the recursion (reference (a) of tests/_filtergradref.py) and against the serial
backward of the same call.  fp32: the error of every gradient tensor against (a) in fp64, relative to the largest
reference entry, is at most max(4 x that of the serial backward on the same inputs, 64 eps32).  Worst figures measured
on an MI355X: DESIGN.md 4.25."""
import functools

import pytest
import torch

from cyclic_gps import leg
from test_filtergradref import autograd_of_a, check
from test_leg_filter import EPS, F32, F64, LENGTHS, _inputs
from test_leg_filter_grad import NAMES, PER_ROW, _assert_grads, _cotangents, _grid_case, _reference_grads, _rel_err, _states
from test_leg_posterior_batch import MODES, _model, _series

cr = leg.cr


def _grads(mats_list, series, mode, init, cots, dtype=F64, fill=float("nan"), **kw):
    """The gradients of sum <cotangent, output> from ``filter_predictive_models(differentiable=True, **kw)``, in the
    layout of ``test_leg_filter_grad._library_grads``."""
    lengths = [sr[0].shape[0] for sr in series]
    leaf = lambda t: t.detach().to(dtype).cuda().requires_grad_(True)      # noqa: E731
    ms = [leg.LEGMatrices(*(leaf(t) for t in mats)) for mats in mats_list]
    ts, xs, ob, nv = _inputs(series, mode, dtype, fill)
    ts, xs = ts.requires_grad_(True), xs.requires_grad_(True)
    nv = None if nv is None else nv.requires_grad_(True)
    st = None if init is None else leg.FilterState(*(leaf(t) for t in init))
    out = leg.filter_predictive_models(ms, ts, xs, lengths=lengths, observed=ob, noise_var=nv, init=st, differentiable=True, **kw)
    outs = dict(zip(PER_ROW + ("loglik",), out[:6]), state_mean=out.state.mean, state_cov=out.state.cov)
    total = sum((cots[key].to(outs[key].dtype).cuda() * outs[key]).sum().to(F64) for key in cots)
    total.backward()
    got = {"%s%d" % (n, k): getattr(m, n).grad for k, m in enumerate(ms) for n in NAMES}
    got.update(xs=xs.grad, ts=ts.grad)
    if nv is not None:
        got["noise_var"] = nv.grad
    if st is not None:
        got.update({"init.t": st.t.grad, "init.mean": st.mean.grad, "init.cov": st.cov.grad})
    return got


def _cpu(grads):
    return {k: v.detach().cpu() for k, v in grads.items()}


@functools.lru_cache(maxsize=None)
def _serial_grid(d, obs, mode, with_init, dtype=F64):
    """The serial backward (``backward_chunk_rows=None``) on a ``_grid_case``, computed once"""
    mats_list, series, init, cots, _ = _grid_case(d, obs, mode, with_init)
    return _cpu(_grads(mats_list, series, mode, init, cots, dtype))


# ---- 1. fp64, all outputs: against autograd of the recursion and against the serial backward -------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("with_init", [False, True], ids=["prior", "init"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d,obs", [(d, obs) for d in (1, 5) for obs in (1, 3)])
@pytest.mark.parametrize("L", [1, 4, 64])
def test_every_gradient_against_autograd_of_the_recursion_and_the_serial_backward(L, d, obs, mode, with_init):
    mats_list, series, init, cots, want = _grid_case(d, obs, mode, with_init)
    assert max(LENGTHS) > 64                           # (the longest series has two chunks even at L = 64)
    got = _grads(mats_list, series, mode, init, cots, backward_chunk_rows=L)
    what = "L %d d %d obs %d %s %s" % (L, d, obs, mode, "init" if with_init else "prior")
    _assert_grads(got, want, what)
    _assert_grads(got, _serial_grid(d, obs, mode, with_init), what + ", against the serial backward")


@pytest.mark.gpu
@pytest.mark.parametrize("obs", [1, 3])
def test_one_long_series_under_the_time_parallel_forward(obs):
    """1 000 rows, ``chunk_rows=(16, 4)`` and ``backward_chunk_rows=16``: 63 chunks, six rounds of the link scan, against
    the serial backward of the same forward."""
    d, n = 5, 1000
    mats_list = [_model(d, obs, 610 + obs)[1]]
    series = _series(obs, [n], 611 + obs)
    init = _states(series, 1, d, 9, at_first=-1)
    cots = _cotangents(1, [n], obs, d, 10)
    chunks = leg._chunk_plan_kind(16)([n], "cpu")
    assert chunks.chunks == 63 and chunks.rounds == 6
    serial = _grads(mats_list, series, "both", init, cots, chunk_rows=(16, 4))
    got = _grads(mats_list, series, "both", init, cots, chunk_rows=(16, 4), backward_chunk_rows=16)
    _assert_grads(got, _cpu(serial), "1 000 rows obs %d, against the serial backward" % obs)


@pytest.mark.gpu
@pytest.mark.parametrize("replicate", [False, True], ids=["probes", "replicated"])
def test_both_ways_of_measuring_the_chunk_maps(replicate, monkeypatch):
    """d sequential probe calls, or one call over d + 1 copies of the models (``leg.FILTER_LINK_REPLICATE``): whichever is
    not the default is run here"""
    d, obs = 5, 3
    mats_list, series, init, cots, want = _grid_case(d, obs, "both", True)
    monkeypatch.setattr(leg, "FILTER_LINK_REPLICATE", replicate)
    got = _grads(mats_list, series, "both", init, cots, backward_chunk_rows=4)
    _assert_grads(got, want, "L 4 d 5 obs 3 both init, %s" % ("replicated" if replicate else "probes"))
    _assert_grads(got, _serial_grid(d, obs, "both", True), "the same against the serial backward")


# ---- 2. the forms that spill -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_spilling_forms():
    d, obs, lengths = 8, 8, [9, 1, 5]
    mats_list = [_model(d, obs, 620)[1]]
    series = _series(obs, lengths, 621)
    init = _states(series, 1, d, 11)
    cots = _cotangents(1, lengths, obs, d, 12)
    want = _reference_grads(autograd_of_a, mats_list, series, "both", init, cots)
    got = _grads(mats_list, series, "both", init, cots, backward_chunk_rows=4)
    _assert_grads(got, want, "d 8 obs 8 both L 4")
    _assert_grads(got, _cpu(_grads(mats_list, series, "both", init, cots)), "d 8 obs 8 both L 4, against the serial backward")


# ---- 3. fp32 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode,with_init", [("plain", False), ("both", True)], ids=["plain-prior", "both-init"])
@pytest.mark.parametrize("d,obs", [(5, 1), (5, 3), (2, 7)])
def test_fp32_is_as_accurate_as_the_serial_backward(d, obs, mode, with_init):
    mats_list, series, init, cots, want = _grid_case(d, obs, mode, with_init)
    serial = _serial_grid(d, obs, mode, with_init, F32)
    got = _grads(mats_list, series, mode, init, cots, F32, backward_chunk_rows=4)
    assert set(got) == set(want) == set(serial)
    what = "fp32 L 4 d %d obs %d %s" % (d, obs, mode)
    floor, worst = 64 * EPS[F32], (0.0, "")
    for k in want:
        e_lib, e_ser = _rel_err(got[k], want[k]), _rel_err(serial[k], want[k])
        worst = max(worst, (e_lib / max(4 * e_ser, floor), k))
        print("filter grad scan %s %s: error %.3e, the serial backward %.3e, floor %.3e" % (what, k, e_lib, e_ser, floor))
    print("filter grad scan %s: worst ratio to the bound %.3f (%s)" % (what, worst[0], worst[1]))
    for k in want:
        assert got[k].dtype == F32 and _rel_err(got[k], want[k]) <= max(4 * _rel_err(serial[k], want[k]), floor), (what, k)


# ---- 4. exact statements -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_single_chunk_batches_are_the_serial_call_bit_for_bit():
    d, obs, lengths = 5, 3, [1, 2, 3]
    mats_list = [_model(d, obs, 630)[1], _model(d, obs, 631)[1]]
    series = _series(obs, lengths, 632)
    init = _states(series, 2, d, 13)
    cots = _cotangents(2, lengths, obs, d, 14)
    serial = _grads(mats_list, series, "both", init, cots)
    for L in (4, 3, "auto"):
        got = _grads(mats_list, series, "both", init, cots, backward_chunk_rows=L)
        assert set(got) == set(serial)
        for k in serial:
            assert torch.equal(got[k], serial[k]), (L, k)
    # without differentiable=True the keyword is checked and otherwise ignored: no graph
    m = leg.LEGMatrices(*(t.cuda().requires_grad_(True) for t in mats_list[0]))
    ts, xs, ob, nv = _inputs(series, "both", F64)
    res = leg.filter_predictive_batch(m, ts, xs, lengths=lengths, observed=ob, noise_var=nv, backward_chunk_rows=2)
    assert all(t.grad_fn is None for t in res[:6])


@pytest.mark.gpu
@pytest.mark.parametrize("d,obs", [(5, 3), (8, 8)])
def test_the_kernel_keeps_the_structure_the_linking_rests_on(d, obs):
    """cgps_leg_filter_adjoint over chunks with one symmetric cotangent on z_cov of every chunk's last row and nothing
    else: the start-state adjoint of the mean is exactly 0 (the covariance adjoint never feeds the mean) and that of the
    covariance is PhiT Db PhiT^T with the PhiT that unit probes on z_mean measure -- within 1e-12 of its largest entry."""
    lengths, L, M = [23, 9, 1], 4, 2
    mats_list = [_model(d, obs, 640 + d)[1], _model(d, obs, 641 + d)[1]]
    series = _series(obs, lengths, 642 + d)
    ts, xs, ob, nv = _inputs(series, "both", F64)
    dev, R = ts.device, sum(lengths)
    Nm, Rm, Bm, Lm = (torch.stack([mats[j] for mats in mats_list]).cuda() for j in range(4))
    G = (Nm @ Nm.transpose(1, 2) + Rm - Rm.transpose(1, 2) + 1e-5 * torch.eye(d, dtype=F64, device=dev)).contiguous()
    LLT = (Lm @ Lm.transpose(1, 2) + 1e-9 * torch.eye(obs, dtype=F64, device=dev)).contiguous()
    plan = leg._cached_batch_plan(lengths, dev)
    chunks = leg._cached_batch_plan(lengths, dev, leg._chunk_plan_kind(L))
    xs_c, pattern, nv_c = leg._loo_data(xs, ob, nv, F64)
    out = leg._filter_rows(ts, xs_c, pattern, nv_c, plan.offsets, G, Bm.contiguous(), LLT, None)
    zm, zc = out[3], out[4]
    gap = ts - torch.roll(ts, 1)
    gap[plan.offsets[:-1]] = 0
    m0c, P0c, last = leg._filter_chunk_states(chunks, zm, zc, None, None)
    C = chunks.chunks
    assert C == 6 + 3 + 1 and tuple(m0c.shape) == (M, C, d)

    def run(cots, bufs, copies):
        assert copies == 1
        return leg._filter_adjoint_rows(xs_c, pattern, nv_c, chunks.chunk_offsets, G, Bm.contiguous(), LLT, gap, zm, zc, m0c, P0c,
                                        cots, bufs)

    PhiT = leg._filter_chunk_maps(run, M, R, d, F64, dev, last, [None] * 5, False)[0]
    W = torch.randn(M, C, d, d, generator=torch.Generator().manual_seed(15), dtype=F64).cuda()
    Db = W + W.transpose(-1, -2)
    g_zc = torch.zeros(M, R, d, d, dtype=F64, device=dev)
    g_zc[:, last] = Db
    res = run([None, None, None, None, g_zc], None, 1)
    assert bool((res[4] == 0).all())
    want = PhiT @ Db @ PhiT.transpose(-1, -2)
    err = _rel_err(res[5], want)
    print("filter grad scan structure d %d obs %d: P0_bar against PhiT Db PhiT^T %.3e" % (d, obs, err))
    assert float(want.abs().max()) > 1e-3 and err <= 1e-12


# ---- 5. a failed series stays contained ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_failing_series_fails_as_in_the_serial_call_and_the_others_are_untouched():
    """A negative gap in the middle chunk of the middle series of three (the gap is data: it fails under both models)"""
    d, obs, lengths, L = 5, 3, [9, 13, 10], 4
    mats_list = [_model(d, obs, 650)[1], _model(d, obs, 651)[1]]
    series = [tuple(t.clone() for t in sr) for sr in _series(obs, lengths, 652)]
    ts1 = series[1][0]
    ts1[5] = ts1[4] - 0.5
    cots = _cotangents(2, lengths, obs, d, 16, keys=("loglik", "z_mean", "mean"))
    cr.CHECK_POSITIVE_DEFINITE = False
    try:
        serial = _grads(mats_list, series, "both", None, cots)
        got = _grads(mats_list, series, "both", None, cots, backward_chunk_rows=L)
    finally:
        cr.CHECK_POSITIVE_DEFINITE = True
    lo, hi = lengths[0], lengths[0] + lengths[1]
    for g in (serial, got):
        assert bool(torch.isnan(g["xs"][lo:hi]).all()) and bool(torch.isnan(g["noise_var"][lo:hi]).all())
        assert all(bool(torch.isnan(g["%s%d" % (n, k)]).all()) for n in NAMES for k in range(2))
    keep = torch.cat([torch.arange(0, lo), torch.arange(hi, sum(lengths))]).cuda()
    for key in ("xs", "noise_var"):
        assert bool(torch.isfinite(got[key][keep]).all())
        check(got[key][keep], serial[key][keep], "the series next to the failed one: %s" % key)


# ---- 6. loglik alone, against the smoother's path ----------------------------------------------------------------------------
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
            ll = leg.filter_predictive_batch(m, ts, xs, differentiable=True, backward_chunk_rows=4, **kw).loglik
        else:
            ll = leg.log_likelihood_batch(m, ts, xs, **kw)
        ll.sum().backward()
        grads.append(({n: getattr(m, n).grad for n in NAMES}, {"xs": xs.grad, "ts": ts.grad, "noise_var": nv.grad}))
    (gm_f, gd_f), (gm_s, gd_s) = grads
    for n in NAMES:
        check(gm_f[n], gm_s[n], "loglik obs %d: %s" % (obs, n))
    for key, g in gd_s.items():
        assert gd_f[key] is not None
        if g is not None:                              # (what the smoother's path differentiates)
            check(gd_f[key], g, "loglik obs %d: %s" % (obs, key))


# ---- 7. finite differences ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gradcheck():
    d, obs, n = 2, 1, 5
    mats = _model(d, obs, 91)[1]
    ts, xs, _, s = _series(obs, [n], 92)[0]
    t0, m0, P0 = _states([(ts, xs, None, s)], 1, d, 93, at_first=-1)
    leaf = lambda t: t.clone().cuda().requires_grad_(True)      # noqa: E731
    inputs = tuple(leaf(t) for t in mats + (xs, ts, s, m0[0, 0]))

    def fn(Nm, Rm, Bm, Lm, xs_, ts_, nv_, mean0):
        out = leg.filter_predictive(leg.LEGMatrices(Nm, Rm, Bm, Lm), ts_, xs_, noise_var=nv_,
                                    init=leg.FilterState(t0[0].cuda(), mean0, P0[0, 0].cuda()), differentiable=True,
                                    backward_chunk_rows=2)
        return out[:6] + (out.state.mean, out.state.cov)

    assert torch.autograd.gradcheck(fn, inputs)

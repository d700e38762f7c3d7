"""The time-parallel form of the filter (``chunk_rows=`` of leg.filter_predictive*, cgps_leg_filter_scan: DESIGN.md 4.23)
against the dense truths of tests/test_leg_filter.py at its bounds, against the serial kernel on one long series, and for
what the chunked scan promises: the first chunk of every series is the serial kernel bit for bit, nothing depends on
later chunks, a series that fails poisons nothing after it (resets are selected, not multiplied), a series' results do
not depend on its place in the batch beyond rounding.  Every test here needs ``chunk_rows``."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import _filterref
from cyclic_gps import _hip, leg
from test_leg_filter import (ATOL, EPS, F32, F64, LENGTHS, LL_TOL, ROWS, RTOL, _assert_continues, _assert_loglik_close,
                             _assert_rows_close, _case, _cat, _cuda_model, _inputs, _same_bits, _seed, _seq_sum, _split,
                             _truth_args)
from test_leg_posterior_batch import _model, _ragged, _series
from test_plan import _host_compiler

cr = leg.cr
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# chunk counts of 1, exactly F, F + 1 and >= 3 upper levels on the 65-row series, a ragged last chunk, a chunk longer than
# every series, series shorter than a chunk
CHUNKINGS = [1, (2, 2), (4, 3), 7, 64, 100]


def _rel(a, b):
    a, b = a.cpu().to(F64), b.cpu().to(F64)
    assert torch.equal(torch.isnan(a), torch.isnan(b))
    return float(((a - b).abs() / (1 + b.abs())).nan_to_num().max()) if a.numel() else 0.0


def _dense_view(t, B, n):
    return None if t is None else t.reshape((B, n) + tuple(t.shape[1:]))


# ---- 1. fp64 against the dense truths ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "both"])
@pytest.mark.parametrize("d,obs", [(d, obs) for d in (1, 5, 8) for obs in (1, 3, 8)])
def test_every_chunking_against_the_dense_truths(d, obs, mode):
    m = None
    for lengths, seed in ((LENGTHS, _seed(d, obs)), ((7, 7, 7), _seed(d, obs) + 3)):
        mats, series, truth = _case(d, obs, lengths, seed, mode)
        m = _cuda_model(mats)
        ts, xs, ob, nv = _inputs(series, mode, F64)
        dense = lengths != LENGTHS
        for ch in CHUNKINGS:
            what = "d %d obs %d %s lengths %s chunk_rows %s" % (d, obs, mode, lengths, ch)
            if dense:
                out = leg.filter_predictive_batch(m, _dense_view(ts, 3, 7), _dense_view(xs, 3, 7), observed=_dense_view(ob, 3, 7),
                                                  noise_var=_dense_view(nv, 3, 7), chunk_rows=ch)
                assert tuple(out.mean.shape) == (3, 7, obs) and tuple(out.z_cov.shape) == (3, 7, d, d)
            else:
                out = leg.filter_predictive_batch(m, ts, xs, lengths=list(lengths), observed=ob, noise_var=nv, chunk_rows=ch)
            _assert_rows_close(out, truth, what, RTOL, ATOL)
            _assert_loglik_close(out.loglik, truth, what, LL_TOL)
            ends = (torch.tensor(lengths).cumsum(0) - 1).cuda()
            assert torch.equal(out.state.t, ts[ends])
            zm, zc = out.z_mean.reshape(-1, d), out.z_cov.reshape(-1, d, d)
            assert _same_bits(out.state.mean, zm[ends]) and _same_bits(out.state.cov, zc[ends])
    # three models: each model's slice is the one-model call, bit for bit
    mats, series, _ = _case(d, obs, LENGTHS, _seed(d, obs), mode)
    ts, xs, ob, nv = _inputs(series, mode, F64)
    ms = [_cuda_model(mats)] + [_cuda_model(_model(d, obs, 70 + k)[1]) for k in range(2)]
    kw = dict(lengths=list(LENGTHS), observed=ob, noise_var=nv, chunk_rows=(4, 3))
    three = leg.filter_predictive_models(ms, ts, xs, **kw)
    for k in range(3):
        each = leg.filter_predictive_batch(ms[k], ts, xs, **kw)
        assert all(_same_bits(a[k], b) for a, b in zip(three[:6], each[:6]))
        assert _same_bits(three.state.mean[k], each.state.mean) and _same_bits(three.state.cov[k], each.state.cov)


# ---- 2. one long series against the serial kernel -----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("obs", [1, 3])
def test_one_long_series_against_the_serial_kernel(obs):
    n, d = 20011, 5
    _, mats = _model(d, obs, 200 + obs)
    (ts, xs, mask, s), = _series(obs, [n], 201 + obs)
    m = _cuda_model(mats)
    ts, xs, ob, nv = _inputs([(ts, xs, mask, s)], "both", F64)
    serial = leg.filter_predictive(m, ts, xs, observed=ob, noise_var=nv)
    for ch in ("auto", (16, 8)):
        L = leg.FILTER_CHUNK_ROWS if ch == "auto" else ch[0]
        out = leg.filter_predictive(m, ts, xs, observed=ob, noise_var=nv, chunk_rows=ch)
        for key, got, want in zip(ROWS, out[:5], serial[:5]):
            err = (got - want).abs()
            print("n %d obs %d chunk_rows %s %s: max |err| %.3e" % (n, obs, ch, key, float(err.max())))
            assert bool((err - RTOL * want.abs() <= ATOL).all()), (ch, key, float(err.max()))
        assert _same_bits(out.state.mean, out.z_mean[-1]) and _same_bits(out.state.cov, out.z_cov[-1])
        assert torch.equal(out.state.t, ts[-1])
        ll = 0.0
        for part in torch.split(out.logpdf.cpu(), L):
            ll += _seq_sum(part)
        assert ll == float(out.loglik), (ll, float(out.loglik))
        assert abs(float(out.loglik) - float(serial.loglik)) <= LL_TOL * max(1.0, abs(float(serial.loglik)))


# ---- 3. the first chunk is the serial kernel -----------------------------------------------------------------------------
def _some_states(series, d, dtype, seed):
    """A FilterState per series, a little before its first row (the third series: AT its first row)."""
    gen = torch.Generator().manual_seed(seed)
    B = len(series)
    t = torch.stack([sr[0][0] - (0.0 if b == 2 else 0.3 + 0.1 * b) for b, sr in enumerate(series)])
    mean = torch.randn(B, d, generator=gen, dtype=F64)
    W = torch.randn(B, d, d, generator=gen, dtype=F64)
    cov = 0.5 * torch.eye(d, dtype=F64) + 0.1 * W @ W.transpose(1, 2)
    return leg.FilterState(t.to(dtype).cuda(), mean.to(dtype).cuda(), cov.to(dtype).cuda())


@pytest.mark.gpu
@pytest.mark.parametrize("with_init", [False, True])
def test_the_first_chunk_of_every_series_is_the_serial_kernel(with_init):
    d, obs = 5, 3
    mats, series, _ = _case(d, obs, LENGTHS, _seed(d, obs), "both")
    m = _cuda_model(mats)
    ts, xs, ob, nv = _inputs(series, "both", F64)
    init = _some_states(series, d, F64, 3) if with_init else None
    kw = dict(lengths=list(LENGTHS), observed=ob, noise_var=nv, init=init)
    serial = leg.filter_predictive_batch(m, ts, xs, **kw)
    for ch in ((4, 3), 7, 64):
        L = ch if isinstance(ch, int) else ch[0]
        out = leg.filter_predictive_batch(m, ts, xs, chunk_rows=ch, **kw)
        for a, b in zip(out[:5], serial[:5]):
            for pa, pb in zip(_split(a, LENGTHS), _split(b, LENGTHS)):
                assert _same_bits(pa[:L], pb[:L]), ch
        short = [b for b, n in enumerate(LENGTHS) if n <= L]
        assert _same_bits(out.loglik[short], serial.loglik[short]) and _same_bits(out.state.cov[short], serial.state.cov[short])


# ---- 4. causality at chunk granularity -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_nothing_depends_on_later_chunks_bit_for_bit():
    d, obs, lengths, L = 5, 3, [9, 65, 11], 4
    _, mats = _model(d, obs, 210)
    series = _series(obs, lengths, 211)
    m = _cuda_model(mats)
    run = lambda sers: leg.filter_predictive_batch(m, *_ragged(sers, F64)[:2], lengths=lengths, observed=_ragged(sers, F64)[2],   # noqa: E731
                                                   noise_var=_ragged(sers, F64)[3], chunk_rows=(L, 3))
    base = run(series)
    gen = torch.Generator().manual_seed(9)
    cr.CHECK_POSITIVE_DEFINITE = False
    try:
        for c in (1, 5, 16):
            ts, xs, mask, s = (t.clone() for t in series[1])
            k = c * L
            xs[k:] = torch.randn(65 - k, obs, generator=gen, dtype=F64)
            xs[k + 1:] = float("nan")
            mask[k:] = ~mask[k:]
            s[k:] = 3.0 * torch.rand(65 - k, obs, generator=gen, dtype=F64)
            other = run([series[0], (ts, xs, mask, s), series[2]])
            assert k + 1 >= 65 or bool(torch.isnan(other.logpdf[9 + k:9 + 65]).any())
            for a, b in zip(base[:5], other[:5]):
                pa, pb = _split(a, lengths), _split(b, lengths)
                assert _same_bits(pa[1][:k], pb[1][:k]), c
                assert _same_bits(pa[0], pb[0]) and _same_bits(pa[2], pb[2]), c
    finally:
        cr.CHECK_POSITIVE_DEFINITE = True


# ---- 5. the place in the batch, the layout -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_permuting_the_series_permutes_the_results_and_a_series_alone_equals_its_slot():
    d, obs = 5, 3
    mats, series, _ = _case(d, obs, LENGTHS, _seed(d, obs), "both")
    m = _cuda_model(mats)
    ch, tol = (4, 3), 64 * EPS[F64]
    ts, xs, ob, nv = _inputs(series, "both", F64)
    out = leg.filter_predictive_batch(m, ts, xs, lengths=list(LENGTHS), observed=ob, noise_var=nv, chunk_rows=ch)
    perm = [3, 0, 4, 2, 1]
    pts, pxs, pob, pnv = _inputs([series[b] for b in perm], "both", F64)
    pout = leg.filter_predictive_batch(m, pts, pxs, lengths=[LENGTHS[b] for b in perm], observed=pob, noise_var=pnv, chunk_rows=ch)
    worst = 0.0
    for a, b in zip(out[:5], pout[:5]):
        parts = _split(a, LENGTHS)
        worst = max(worst, _rel(torch.cat([parts[j] for j in perm]), b))
    idx = torch.tensor(perm).cuda()
    worst = max(worst, _rel(out.state.mean[idx], pout.state.mean), _rel(out.state.cov[idx], pout.state.cov))
    err = _rel(out.loglik[idx], pout.loglik)
    for b in (0, 3, 4):
        t1, x1, o1, n1 = _inputs([series[b]], "both", F64)
        alone = leg.filter_predictive(m, t1, x1, observed=o1, noise_var=n1, chunk_rows=ch)
        worst = max([worst] + [_rel(_split(a, LENGTHS)[b], c) for a, c in zip(out[:5], alone[:5])])
        err = max(err, _rel(out.loglik[b], alone.loglik))
    print("permutation / alone: rows %.2f eps, loglik %.2f eps" % (worst / EPS[F64], err / EPS[F64]))
    assert worst <= tol and err <= tol


@pytest.mark.gpu
@pytest.mark.parametrize("ch", [(2, 2), 4, 64])
def test_dense_and_ragged_layouts_agree_bit_for_bit(ch):
    d, obs, B, n = 5, 2, 3, 7
    mats, series, _ = _case(d, obs, (n,) * B, 41, "both")
    m = _cuda_model(mats)
    ts, xs, ob, nv = _inputs(series, "both", F64)
    rag = leg.filter_predictive_batch(m, ts, xs, lengths=[n] * B, observed=ob, noise_var=nv, chunk_rows=ch)
    out = leg.filter_predictive_batch(m, _dense_view(ts, B, n), _dense_view(xs, B, n), observed=_dense_view(ob, B, n),
                                      noise_var=_dense_view(nv, B, n), chunk_rows=ch)
    for a, b in zip(out[:5], rag[:5]):
        assert _same_bits(a.reshape(b.shape), b)
    assert _same_bits(out.loglik, rag.loglik) and all(_same_bits(a, b) for a, b in zip(out.state, rag.state))


# ---- 6. continuing -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("d,obs", [(5, 3), (8, 8), (1, 1)])
def test_a_scanned_series_continues_from_its_state(d, obs, dtype):
    n, ch, h = 23, (4, 2), 6                          # (row 6 is no chunk boundary)
    _, mats = _model(d, obs, 100 + d)
    (ts, xs, mask, s), = _series(obs, [n], 101 + d)
    m = _cuda_model(mats, dtype)
    g = lambda t: t.to(dtype).cuda() if t.dtype != torch.bool else t.cuda()      # noqa: E731
    call = lambda t, x, o, v, init=None: leg.filter_predictive(m, g(t), g(x), observed=g(o), noise_var=g(v), init=init,   # noqa: E731
                                                               chunk_rows=ch)
    whole = call(ts, xs, mask, s)
    head = call(ts[:h], xs[:h], mask[:h], s[:h])
    tail = call(ts[h:], xs[h:], mask[h:], s[h:], head.state)
    _assert_continues(tail, [t[h:] for t in whole[:5]], whole.state, None, dtype, "h %d" % h)
    assert abs(float(head.loglik) + float(tail.loglik) - float(whole.loglik)) <= 64 * EPS[dtype] * n * max(1.0, abs(float(whole.loglik)))
    # across a zero gap: a row at the head's last time stamp that observes nothing, then the rows that follow
    dup = lambda t, fill: torch.cat([t[:h], torch.full_like(t[h - 1:h], fill) if fill is not None else t[h - 1:h], t[h:]])   # noqa: E731
    ts2, xs2, mask2, s2 = dup(ts, None), dup(xs, float("nan")), dup(mask, False), dup(s, float("nan"))
    whole2 = call(ts2, xs2, mask2, s2)
    tail2 = call(ts2[h:], xs2[h:], mask2[h:], s2[h:], head.state)
    assert float(head.state.t) == float(g(ts2)[h])
    _assert_continues(tail2, [t[h:] for t in whole2[:5]], whole2.state, None, dtype, "zero gap")
    assert float(tail2.logpdf[0]) == 0.0 and _same_bits(tail2.z_mean[0], head.state.mean)


# ---- 7. failures ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("defect", ["negative gap", "nan observation"])
def test_a_failing_row_fails_as_in_the_serial_call_and_the_next_series_is_untouched(defect):
    """The middle chunk of the middle series of three.  The series after it starts with a reset, which is selected: were
    it multiplied into the NaN prefix before it, that series would be NaN too."""
    d, obs, lengths, ch = 5, 3, [9, 13, 10], (4, 2)
    _, mats = _model(d, obs, 220)
    series = _series(obs, lengths, 221)
    m = _cuda_model(mats)
    ts, xs, ob, nv = _ragged(series, F64)
    local = 5                                       # chunk 1 of 4 of the middle series
    row = lengths[0] + local
    ob[row] = True
    kw = dict(lengths=lengths, observed=ob, noise_var=nv)
    healthy = leg.filter_predictive_batch(m, ts, xs, chunk_rows=ch, **kw)
    assert all(bool(torch.isfinite(t).all()) for t in healthy[:6])
    ts, xs = ts.clone(), xs.clone()
    if defect == "negative gap":
        ts[row] = ts[row - 1] - 0.5
    else:
        xs[row, 1] = float("nan")
    texts = []
    for kwargs in ({}, {"chunk_rows": ch}):
        with pytest.raises(cr.NotPSDError) as e:
            leg.filter_predictive_batch(m, ts, xs, **kw, **kwargs)
        texts.append(str(e.value))
    assert texts[0] == texts[1] and re.search(r"series 1.*row %d" % local, texts[0]), texts
    cr.CHECK_POSITIVE_DEFINITE = False
    try:
        serial = leg.filter_predictive_batch(m, ts, xs, **kw)
        out = leg.filter_predictive_batch(m, ts, xs, chunk_rows=ch, **kw)
    finally:
        cr.CHECK_POSITIVE_DEFINITE = True
    for key, a, b in zip(ROWS, out[:5], serial[:5]):
        assert bool(torch.isnan(a[row:lengths[0] + lengths[1]]).all()) and bool(torch.isfinite(a[:row]).all()), key
        assert _rel(a, b) <= 1e-9, key                # (the same NaN pattern: _rel asserts it)
    assert _rel(out.loglik, serial.loglik) <= 1e-9 and bool(torch.isnan(out.loglik[1]))
    assert _rel(out.state.mean, serial.state.mean) <= 1e-9 and _rel(out.state.cov, serial.state.cov) <= 1e-9
    assert bool(torch.isnan(out.state.mean[1]).all()) and bool(torch.isnan(out.state.cov[1]).all())
    # the other two series: bit for bit those of the healthy call
    for a, b in zip(out[:5], healthy[:5]):
        pa, pb = _split(a, lengths), _split(b, lengths)
        assert _same_bits(pa[2], pb[2]) and _same_bits(pa[0], pb[0])
        assert _same_bits(pa[1][:4], pb[1][:4])      # the failing series' first chunk
    assert _same_bits(out.loglik[2], healthy.loglik[2]) and _same_bits(out.state.cov[2], healthy.state.cov[2])


# ---- 8. fp32 -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "both"])
@pytest.mark.parametrize("d,obs", [(1, 1), (5, 1), (5, 3), (8, 8)])
def test_fp32_is_as_accurate_as_the_serial_recursion_in_torch(d, obs, mode):
    """The bound and floor of the serial kernel's test: the fp32 error of every output against the fp64 truth is at most
    4x that of tests/_filterref.py in fp32 on the same inputs, floor 64 eps32, relative to 1 + |value|.  Worst ratios
    seen on an MI355X (error over max(torch's, 16 eps32)): see DESIGN.md 4.23."""
    mats, series, truth = _case(d, obs, LENGTHS, _seed(d, obs), mode)
    m = _cuda_model(mats, F32)
    ts, xs, ob, nv = _inputs(series, mode, F32)
    refs = [_filterref.filter_ref(mats, *_truth_args(sr, mode), dtype=F32) for sr in series]
    for ch in ((4, 3), 64):
        out = leg.filter_predictive_batch(m, ts, xs, lengths=list(LENGTHS), observed=ob, noise_var=nv, chunk_rows=ch)
        assert all(t.dtype == F32 for t in out[:5]) and out.loglik.dtype == F64
        worst = 0.0
        for j, key in enumerate(ROWS + ("loglik",)):
            want = _cat(truth, key) if key != "loglik" else torch.stack([t["loglik"] for t in truth])
            ref = torch.cat([r[key] for r in refs]) if key != "loglik" else torch.stack([r["loglik"] for r in refs])
            scale = 1 + want.abs()
            e_lib = float(((out[j].cpu().to(F64).reshape(want.shape) - want).abs() / scale).max())
            e_ref = float(((ref.to(F64).reshape(want.shape) - want).abs() / scale).max())
            worst = max(worst, e_lib / max(e_ref, 64 * EPS[F32] / 4))
            print("fp32 d %d obs %d %s chunk_rows %s %s: library %.3e torch %.3e" % (d, obs, mode, ch, key, e_lib, e_ref))
            assert e_lib <= max(4 * e_ref, 64 * EPS[F32]), (ch, key, e_lib, e_ref)
        print("fp32 d %d obs %d %s chunk_rows %s: worst error in units of max(torch's, 16 eps32): %.2f" % (d, obs, mode, ch, worst))


# ---- 9. arguments and the boundary ---------------------------------------------------------------------------------------
def test_bad_chunk_rows_raise_before_anything_runs():
    m, _ = _model(3, 2, 5)
    ts, xs = torch.cumsum(torch.ones(3, 4, dtype=F64), 1), torch.zeros(3, 4, 2, dtype=F64)
    for bad in (0, -3, (4, 1), (0, 2), (4,), (4, 3, 2), "fast", 2.5, True, (4, 2.0), [4]):
        for call in (lambda: leg.filter_predictive(m, ts[0], xs[0], chunk_rows=bad),
                     lambda: leg.filter_predictive_batch(m, ts, xs, chunk_rows=bad),
                     lambda: leg.filter_predictive_models([m, m], ts, xs, chunk_rows=bad)):
            with pytest.raises(ValueError):
                call()
    for good in ("auto", 1, (1, 2), [64, 16]):        # valid: past the checks, then no CPU implementation
        with pytest.raises(_hip.CgpsError):
            leg.filter_predictive_batch(m, ts, xs, chunk_rows=good)
    assert leg.FILTER_CHUNK_ROWS >= 1 and leg.FILTER_SCAN_FANOUT >= 2


def test_the_scan_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "cgps.h")).read()
    lib = _hip.lib()
    for name in ("cgps_leg_filter_scan", "cgps_leg_filter_scan_workspace_bytes"):
        assert re.search(r"\bint %s\s*\(" % name, header) and name in _hip.exported_symbols()
        assert hasattr(ctypes.CDLL(_hip.LIB_PATH), name)
    assert lib.cgps_version() == 320
    # argument errors come back as codes, before anything is launched
    call = lambda B, R, M, d, obs, L, F: lib.cgps_leg_filter_scan(                                    # noqa: E731
        *([None] * 5), B, R, M, None, None, None, d, obs, _hip.F64, *([None] * 6), 1, L, F, None, 0, *([None] * 10))
    assert call(1, 1, 0, 2, 1, 4, 2) == 1 and call(1, 1, 1, 2, 9, 4, 2) == 3 and call(1, 1, 1, 9, 1, 4, 2) == 3
    assert call(1, 1, 1, 2, 1, 0, 2) == 1 and b"chunk_rows" in lib.cgps_last_error()
    assert call(1, 1, 1, 2, 1, 4, 1) == 1 and b"fanout" in lib.cgps_last_error()
    assert call(1, 1, 1, 2, 1, 4, 2) == 1 and b"null pointer" in lib.cgps_last_error()
    assert call(0, 0, 1, 2, 1, 4, 2) == 0
    b = ctypes.c_size_t(0)
    assert lib.cgps_leg_filter_scan_workspace_bytes(4, 1, 2, _hip.F64, 1, ctypes.byref(b)) == 1
    assert lib.cgps_leg_filter_scan_workspace_bytes(4, 1, 9, _hip.F64, 2, ctypes.byref(b)) == 3
    assert lib.cgps_leg_filter_scan_workspace_bytes(4, 1, 2, _hip.F64, 2, None) == 1


@pytest.mark.gpu
def test_a_null_or_short_workspace_is_an_argument_error():
    d, obs, n, L, F = 3, 2, 9, 4, 2
    dev = "cuda"
    e = lambda *shape: torch.zeros(shape, dtype=F64, device=dev)      # noqa: E731
    ts, xs = torch.arange(n, dtype=F64, device=dev), e(n, obs)
    G, Bm, LLT = torch.eye(d, dtype=F64, device=dev).reshape(1, d, d), e(1, obs, d), torch.eye(obs, dtype=F64, device=dev).reshape(1, obs, obs)
    roff = torch.tensor([0, n], device=dev)
    coff, cser, sc = torch.tensor([0, 4, 8, 9], device=dev), torch.zeros(3, dtype=torch.int64, device=dev), torch.tensor([0, 3], device=dev)
    outs = [e(1, n, obs), e(1, n, obs, obs), e(1, n), e(1, n, d), e(1, n, d, d), e(1, 1), e(1, 1, d), e(1, 1, d, d),
            torch.zeros(1, dtype=torch.int32, device=dev)]
    need = _hip.filter_scan_workspace_bytes(3, 1, d, _hip.F64, F)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    p = _hip.ptr
    call = lambda wsp, nbytes, chunks=3: _hip.lib().cgps_leg_filter_scan(                              # noqa: E731
        p(ts), p(xs), None, None, p(roff), 1, n, 1, p(G), p(Bm), p(LLT), d, obs, _hip.F64, None, None, None, p(coff), p(cser),
        p(sc), chunks, L, F, wsp, nbytes, *[p(t) for t in outs], _hip.stream_ptr())
    assert call(None, need) == 1 and b"null pointer" in _hip.lib().cgps_last_error()
    assert call(p(ws), need - 1) == 1 and b"workspace" in _hip.lib().cgps_last_error()
    assert call(p(ws), need, 2) == 1 and call(p(ws), need, 10) == 1          # too few / too many chunks for 9 rows of 4
    assert call(p(ws), need) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[2]).all()) and int(outs[8]) == 0


# ---- 10. the workspace plan, on the host -----------------------------------------------------------------------------------
def _chunks(lengths, L):
    return sum(-(-n // L) for n in lengths)


def test_workspace_query_is_the_sum_of_the_carve_up_and_monotone(tmp_path):
    exe = str(tmp_path / "scan_plan_check")
    subprocess.run(_host_compiler() + ["-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "cyclic-gps_amd", "csrc"),
                                       os.path.join(HERE, "scan_plan_check.cpp"), "-o", exe], check=True)
    cases = [((1,), 1, 2, 1, 1, F64), (LENGTHS, 4, 3, 5, 1, F64), (LENGTHS, 2, 2, 8, 3, F32), ((20011,), 16, 8, 5, 1, F64),
             ((1 << 20,), 64, 32, 5, 1, F64), ((502,) * 1024, 64, 32, 5, 16, F32), ((7, 7, 7), 100, 2, 1, 2, F64)]
    args = []
    for lengths, L, F, d, M, dt in cases:
        args += [_chunks(lengths, L), M, d, 4 if dt == F32 else 8, F]
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60, check=True)
    lines = [list(map(int, l.split())) for l in r.stdout.splitlines()]
    assert len(lines) == len(cases)
    q = lambda lengths, L, F, d, M, dt: _hip.filter_scan_workspace_bytes(_chunks(lengths, L), M, d, _hip.dtype_code(dt), F)   # noqa: E731
    for (lengths, L, F, d, M, dt), line in zip(cases, lines):
        total, summed, levels, ok = line[5:]
        assert ok == 1 and total == summed == q(lengths, L, F, d, M, dt), (lengths[:3], L, F, d, M, line)
        n, want = _chunks(lengths, L), 1
        while n > F:
            n, want = -(-n // F), want + 1
        assert levels == want
        # monotone: more rows, shorter chunks, a smaller fan-out, a larger rank, more models, the wider type
        base = q(lengths, L, F, d, M, dt)
        assert q(tuple(lengths) + (3 * L + 1,), L, F, d, M, dt) >= base
        assert q(lengths, max(1, L // 2), F, d, M, dt) >= base >= q(lengths, 2 * L, F, d, M, dt)
        assert q(lengths, L, max(2, F - 1), d, M, dt) >= base >= q(lengths, L, F + 1, d, M, dt)
        assert q(lengths, L, F, min(8, d + 1), M, dt) >= base and q(lengths, L, F, d, M + 1, dt) >= base
        assert q(lengths, L, F, d, M, F64) >= q(lengths, L, F, d, M, F32)

"""Every compiled rank x channel form of the LEG row kernels: leg_filter_kernel<T, D, O>,
leg_fscan_chunk_kernel<T, D, O> with the D-only kernels of the scan around it (4.23) and leg_loo_rows_kernel<T, D, O>
(4.20), for d = 1..8 x obs = 1..8 in both precisions.  Each instantiation is unrolled over D and O, so it is machine code
of its own with a register allocation of its own; obs = 5, 6, 7 run the O = 8 form with its run-time channel count (the
``c < obs`` guards, the operand strides k obs D and k obs obs, the pattern mask (1 << obs) - 1).

One ragged batch of four series of 1, 2, 6 and 3 rows, which share a wave: its lanes leave the walk at rows 1, 2, 6 and 3.
In "both" (mask + per-point variances, NaN where nothing is observed) the 6-row series has its first, fourth and last row
wholly unobserved, so with chunk_rows = (2, 2) each of its three chunks holds an unobserved row and the scan has two upper
levels.  The truths are the dense ones of tests/test_leg_filter.py and tests/_looref.py; nothing here is a second truth.

Accuracy of the filter, serial and time-parallel: per output, err <= max(4 e_ref, floor), err relative to 1 + |value|
(loglik: to max(1, |ll|)), e_ref the error of the recursion in torch (tests/_filterref.py) in the same precision on the
same inputs; floor 64 eps32 in fp32 and 8 x the worst error measured on an MI355X in fp64 (FILTER_MEASURED_GPU).
The leave-one-out row kernel: 256 eps kappa cond(W) as in tests/test_leg_loo.py, in "both" only (in "plain" 15 of the 64
pairs exceed kappa = 64 at these seeds).  The scan's LU exchanges no row on these cases; section b' runs it from start
states that make it (ranks 2..8, both precisions).  The CPU tests pin the reference, the choice of inputs and the list of forms."""
import functools
import os
import re

import pytest
import torch

import _filterref
import _scanref
from cyclic_gps import leg
from test_leg_filter import (EPS, F32, F64, ROWS, _assert_mask_covers, _cuda_model, _inputs, _same_bits, _seq_sum, _split,
                             _truth_args)
from test_leg_filter import _case as _filter_case
from test_leg_filter_scan import _some_states
from test_leg_loo import KEYS, LEAVES, _assert_close, _assert_unobserved, _conditioning, _rows_call, _score_check, _truth_posterior
from test_leg_loo import _case as _loo_case
from test_leg_loo import _cat as _loo_cat
from test_leg_loo import _inputs as _loo_inputs
from test_leg_posterior_batch import _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(d, obs) for d in range(1, 9) for obs in range(1, 9)]
LENGTHS = (1, 2, 6, 3)
SWEEP_MODES = ("plain", "both")
CHUNKINGS = (1, (2, 2), 4)
NAME = {F64: "fp64", F32: "fp32"}
PAIR = pytest.mark.parametrize("d,obs", PAIRS)
DTYPES = pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])

FILTER_MEASURED_GPU = {"serial": {F64: 2.451e-14, F32: 3.024e-6}, "scan": {F64: 2.464e-14, F32: 3.531e-6}}
"""Largest error of any output against the dense truth over the 64 pairs and both modes (relative to 1 + |value|, loglik
to max(1, |ll|)), measured on an MI355X: cgps_leg_filter and, over the three chunkings, cgps_leg_filter_scan.  All four
are z_mean of "plain" at d = 2 (obs = 7; the scan's fp32: obs = 6), where the recursion in torch has 1.8e-14 and 1.6e-6
(3.7e-6 at obs = 7) itself; the fp32 figures are 25 and 30 eps32.  The fp64 floor of the accuracy rule is 8 x the larger
fp64 figure (rounding differs between instantiations and compilers), which must stay below 1e-11: four decades under
the rtol 1e-7 / atol 1e-9 of the grids of the other files."""

LOO_MEASURED_GPU = {F64: 8.98, F32: 3.47}
"""Largest error of leg_loo_rows_kernel over the 64 pairs and both leaves in units of eps kappa cond(W), measured on an
MI355X (fp64: d = 6, obs = 4, "row"; fp32: d = 1, obs = 3, "row"); the bound is 256 of these units."""
FLOOR = {F64: 8 * max(v[F64] for v in FILTER_MEASURED_GPU.values()), F32: 64 * EPS[F32]}
REF_BOUND = 1e-12                                    # tests/test_filterref.py's, for the recursion in fp64


def _filter_seed(d, obs):
    return 700 + 10 * d + obs


def _loo_seed(d, obs):
    return 800 + 10 * d + obs


@functools.lru_cache(maxsize=None)
def _refs(d, obs, mode, dtype):
    """tests/_filterref.py on the sweep's case in ``dtype``, one result per series."""
    mats, series, _ = _filter_case(d, obs, LENGTHS, _filter_seed(d, obs), mode)
    return [_filterref.filter_ref(mats, *_truth_args(sr, mode), dtype=dtype) for sr in series]


def _gather(parts, key):
    return (torch.stack if key == "loglik" else torch.cat)([p[key] for p in parts]).to(F64)


def _errors(got, truth, key):
    """max error of one output (a list of per-series tensors or dicts is gathered) against the truth, in the rule's norm"""
    want = _gather(truth, key)
    scale = want.abs().clamp_min(1.0) if key == "loglik" else 1 + want.abs()
    return float(((got.detach().cpu().to(F64).reshape(want.shape) - want).abs() / scale).max())


def _assert_accurate(out, d, obs, mode, dtype, what):
    """The accuracy rule of the module's docstring for the five per-row outputs and loglik; returns the worst error."""
    _, _, truth = _filter_case(d, obs, LENGTHS, _filter_seed(d, obs), mode)
    refs = _refs(d, obs, mode, dtype)
    rows = []
    for j, key in enumerate(ROWS + ("loglik",)):
        e_lib, e_ref = _errors(out[j], truth, key), _errors(_gather(refs, key), truth, key)
        rows.append((e_lib, e_ref, key))
    worst = max(rows)
    print("channel forms %s %s d %d obs %d %s: worst error %.3e (%s; torch's %.3e; floor %.3e)"
          % (what, NAME[dtype], d, obs, mode, worst[0], worst[2], worst[1], FLOOR[dtype]))
    for e_lib, e_ref, key in rows:
        assert e_lib <= max(4 * e_ref, FLOOR[dtype]), (what, key, e_lib, e_ref)
    return worst[0]


def _ends():
    return (torch.tensor(LENGTHS).cumsum(0) - 1).cuda()


def _assert_state_is_the_last_row(out, ts):
    ends = _ends()
    assert torch.equal(out.state.t, ts[ends])
    assert _same_bits(out.state.mean, out.z_mean[ends]) and _same_bits(out.state.cov, out.z_cov[ends])


def test_the_floors_are_the_measured_ones():
    assert FLOOR[F64] <= 1e-11 and FLOOR[F32] == 64 * EPS[F32]
    assert all(v[F32] <= FLOOR[F32] for v in FILTER_MEASURED_GPU.values())
    assert all(8 * v <= 256 for v in LOO_MEASURED_GPU.values())


# ---- a. the serial filter ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@DTYPES
@PAIR
def test_serial_filter_every_form(d, obs, dtype):
    for mode in SWEEP_MODES:
        mats, series, _ = _filter_case(d, obs, LENGTHS, _filter_seed(d, obs), mode)
        m = _cuda_model(mats, dtype)
        ts, xs, ob, nv = _inputs(series, mode, dtype)
        kw = dict(lengths=list(LENGTHS), observed=ob, noise_var=nv, chunk_rows=None)
        out = leg.filter_predictive_batch(m, ts, xs, **kw)
        R = sum(LENGTHS)
        assert [tuple(t.shape) for t in out[:6]] == [(R, obs), (R, obs, obs), (R,), (R, d), (R, d, d), (len(LENGTHS),)]
        assert all(t.dtype == dtype for t in out[:5]) and out.loglik.dtype == F64
        _assert_accurate(out, d, obs, mode, dtype, "serial")
        _assert_state_is_the_last_row(out, ts)
        # the log-likelihood is the fp64 sum of the series' row terms in row order
        for b, lp in enumerate(_split(out.logpdf.cpu().to(F64), LENGTHS)):
            assert _seq_sum(lp) == float(out.loglik[b]), (mode, b)
        if mode == "both":
            assert bool(torch.isnan(xs[~ob]).all()) and bool(torch.isnan(nv[~ob]).all())
            parts = [_split(t.cpu(), LENGTHS) for t in (out.logpdf, out.z_mean, out.z_cov)]
            seen = first = 0
            for b, (_, _, mask, _) in enumerate(series):
                for i in (~mask.any(1)).nonzero().flatten().tolist():
                    seen += 1
                    assert float(parts[0][b][i]) == 0.0, (b, i)
                    if i == 0:                                   # the prior, exactly
                        first += 1
                        assert torch.equal(parts[1][b][0], torch.zeros(d, dtype=dtype))
                        assert torch.equal(parts[2][b][0], torch.eye(d, dtype=dtype))
            assert seen >= 3 and first >= 1
            # unobserved entries are never read
            _, xs0, _, nv0 = _inputs(series, mode, dtype, fill=0.25)
            out0 = leg.filter_predictive_batch(m, ts, xs0, **dict(kw, noise_var=nv0))
            assert all(_same_bits(a, b) for a, b in zip(out[:6], out0[:6]))
            assert all(bool(torch.isfinite(t).all()) for t in out[:6])
        # two models: slice k is the one-model call (the strides k obs D and k obs obs of the operands)
        ms = [m, _cuda_model(_model(d, obs, 70)[1], dtype)]
        two = leg.filter_predictive_models(ms, ts, xs, **kw)
        for k in range(2):
            each = out if k == 0 else leg.filter_predictive_batch(ms[k], ts, xs, **kw)
            assert all(_same_bits(a[k], b) for a, b in zip(two[:6], each[:6])), (mode, k)
            assert _same_bits(two.state.mean[k], each.state.mean) and _same_bits(two.state.cov[k], each.state.cov), (mode, k)
        assert not _same_bits(two.mean[1], two.mean[0])


# ---- b. the time-parallel filter ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@DTYPES
@PAIR
def test_time_parallel_filter_every_form(d, obs, dtype):
    for mode in SWEEP_MODES:
        mats, series, _ = _filter_case(d, obs, LENGTHS, _filter_seed(d, obs), mode)
        m = _cuda_model(mats, dtype)
        ts, xs, ob, nv = _inputs(series, mode, dtype)
        kw = dict(lengths=list(LENGTHS), observed=ob, noise_var=nv)
        inits = (None, _some_states(series, d, dtype, 3))
        serial = [leg.filter_predictive_batch(m, ts, xs, init=init, **kw) for init in inits]
        for ch in CHUNKINGS:
            L = ch if isinstance(ch, int) else ch[0]
            what = "chunk_rows %s" % (ch,)
            for init, ser in zip(inits, serial):
                out = leg.filter_predictive_batch(m, ts, xs, init=init, chunk_rows=ch, **kw)
                assert all(t.dtype == dtype for t in out[:5]) and out.loglik.dtype == F64
                if init is None:
                    _assert_accurate(out, d, obs, mode, dtype, what)
                _assert_state_is_the_last_row(out, ts)
                # the first chunk of every series is the serial kernel
                for a, b in zip(out[:5], ser[:5]):
                    for pa, pb in zip(_split(a, LENGTHS), _split(b, LENGTHS)):
                        assert _same_bits(pa[:L], pb[:L]), (mode, ch, init is not None)
                short = [b for b, n in enumerate(LENGTHS) if n <= L]
                assert _same_bits(out.loglik[short], ser.loglik[short]), (mode, ch)
                assert _same_bits(out.state.mean[short], ser.state.mean[short]), (mode, ch)
                assert _same_bits(out.state.cov[short], ser.state.cov[short]), (mode, ch)


# ---- c. the leave-one-out row kernel -------------------------------------------------------------------------------------
@pytest.mark.gpu
@DTYPES
@PAIR
def test_loo_row_kernel_every_form(d, obs, dtype):
    """cgps_leg_loo on the posterior rows of the dense fp64 truth cast to the dtype, the four series as one data set of
    twelve rows: per entry 256 eps kappa cond(W), relative to 1 + |value|; the NaN pattern is the truth's."""
    mats, series, truth = _loo_case(d, obs, LENGTHS, _loo_seed(d, obs), "both")
    post = [_truth_posterior(mats, sr, "both") for sr in series]
    mu, Sd = torch.cat([p[0] for p in post]), torch.cat([p[1] for p in post])
    whole = tuple(torch.cat([sr[k] for sr in series]) for k in range(4))
    offsets = torch.tensor([0] + torch.tensor(LENGTHS).cumsum(0).tolist(), dtype=torch.int64, device="cuda")
    for leave in LEAVES:
        _conditioning(truth[leave])
        out = _rows_call([mats], whole, "both", mu, Sd, dtype, leave, offsets)
        assert int(out[4].item()) == 0
        kappa, cond_w = _loo_cat(truth[leave], "kappa"), _loo_cat(truth[leave], "cond_w")
        amp = kappa * (cond_w.unsqueeze(-1) if leave == "entry" else cond_w)      # per entry / per row
        bounds = {"mean": amp if leave == "entry" else amp.unsqueeze(-1), "logpdf": amp,
                  "var": amp if leave == "entry" else amp.reshape(-1, 1, 1)}
        worst = 0.0
        for key, got in zip(KEYS, out[:3]):
            want = _loo_cat(truth[leave], key)
            got = got[0].cpu().to(F64)
            ok = ~torch.isnan(want)
            assert torch.equal(torch.isnan(got), ~ok), (leave, key)
            ratio = ((got - want).abs() / (1 + want.abs()) / (EPS[dtype] * bounds[key].clamp(min=1).expand_as(want)))[ok]
            worst = max(worst, float(ratio.max()))
            assert float(ratio.max()) <= 256, (leave, key, float(ratio.max()))
        print("channel forms loo rows %s d %d obs %d %s: worst error %.2f eps kappa cond(W)" % (NAME[dtype], d, obs, leave, worst))


@pytest.mark.gpu
@PAIR
def test_loo_end_to_end_every_form_fp64(d, obs):
    mats, series, truth = _loo_case(d, obs, LENGTHS, _loo_seed(d, obs), "both")
    m = _cuda_model(mats)
    ts, xs, ob, nv = _loo_inputs(series, "both", F64)
    for leave in LEAVES:
        kappa = _conditioning(truth[leave])
        rtol, atol = 1e-7 * kappa, 1e-9 * kappa
        out = leg.loo_predictive_batch(m, ts, xs, lengths=list(LENGTHS), observed=ob, noise_var=nv, leave=leave)
        assert out.score.dtype == F64 and out.score.shape == (len(LENGTHS),)
        _assert_unobserved(out, _loo_cat(truth[leave], "mean"), leave)
        _assert_close(out, truth[leave], leave, rtol, atol, "channel forms d %d obs %d" % (d, obs))
        _score_check(out.score, truth[leave], rtol, atol, "channel forms d %d obs %d" % (d, obs))


# ---- b'. the row exchanges of the scan's LU --------------------------------------------------------------------------------
# scan_combine solves with K = I + C1 J2 by an LU with partial pivoting in registers (lu_factor, lu_solve: D-only).  From
# the prior, and from the states of _some_states, K stays so close to diagonally dominant that NO combine of the sweep
# above exchanges a row (counted with tests/_scanref.py: 0 of 52 combines in each of the 64 pairs), so the exchange would
# be dead code to it.  A start state with a wide, correlated covariance (0.5 I + 50 W W^T) makes the combines exchange rows
# at every rank from 2 up; the CPU test below asserts that they do.  No dense truth has such a start state (a covariance
# above the stationary I): the stand-in is the recursion of tests/_filterref.py in fp64 from the same state, which
# tests/test_filterref.py holds to the dense truths, continuation included, at 1e-12.  Rule: the kernel's error against
# it <= max(4 x that of the scan in torch (tests/_scanref.py) in the kernel's precision, floor), floor 1e-12 in fp64 (what
# the stand-in is itself pinned to) and 64 eps32 in fp32, relative to 1 + |value| (loglik: max(1, |ll|)).
WIDE_PAIRS = [(d, obs) for d in range(2, 9) for obs in (2, 5)]
WIDE_SEED = {2: 37}                                   # rank 2 exchanges a row at this seed; the other ranks at 3
WIDE_FLOOR = {F64: REF_BOUND, F32: 64 * EPS[F32]}


def _fanout(ch):
    return (ch, leg.FILTER_SCAN_FANOUT) if isinstance(ch, int) else ch


def _exchanges(K):
    """whether Gaussian elimination with partial pivoting exchanges a row of K (lu_factor's choice: the first largest)"""
    K = K.clone()
    for col in range(K.shape[0]):
        p = col + int(K[col:, col].abs().argmax())
        if p != col:
            return True
        for r in range(col + 1, K.shape[0]):
            K[r] -= K[r, col] / K[col, col] * K[col]
    return False


@functools.lru_cache(maxsize=None)
def _wide_case(d, obs, mode):
    """(mats, series, start states (t, mean, cov) in fp64 on the CPU, the recursion in fp64 from them)"""
    mats, series, _ = _filter_case(d, obs, LENGTHS, _filter_seed(d, obs), mode)
    inits = []
    for b, sr in enumerate(series):
        gen = torch.Generator().manual_seed(WIDE_SEED.get(d, 3) + b)
        W = torch.randn(d, d, generator=gen, dtype=F64)
        inits.append((sr[0][0] - 0.3, torch.randn(d, generator=gen, dtype=F64), 0.5 * torch.eye(d, dtype=F64) + 50.0 * W @ W.T))
    refs = [_filterref.filter_ref(mats, *_truth_args(sr, mode), init=st) for sr, st in zip(series, inits)]
    return mats, series, inits, refs


@functools.lru_cache(maxsize=None)
def _wide_scan_refs(d, obs, mode, ch, dtype):
    mats, series, inits, _ = _wide_case(d, obs, mode)
    return _scanref.scan_filter_ref(mats, [_truth_args(sr, mode) + (st,) for sr, st in zip(series, inits)], *_fanout(ch), dtype=dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("d,obs", WIDE_PAIRS)
def test_time_parallel_filter_from_a_wide_state_exchanges_rows(d, obs):
    """fp64 only (worst measured on an MI355X: 1.8e-12, a z_cov at d = 7, obs = 2, where the scan in torch has 7.6e-13).
    In fp32 the rule above does not hold on an MI355X and is not asserted: 11 of the 14 pairs kept it, and at (5, 5),
    (6, 2) and (7, 5) the kernel's fp32 error was 4.5x to 5.6x that of the scan in torch
    (worst 7.2e-5 against 1.3e-5, a z_cov at cond(K) up to 1e3) -- one sample of torch's rounding is too sharp a yardstick
    there, and a bound from cond(K) has not been worked out.  The exchange in fp32 is therefore still run by no test."""
    dtype = F64
    for mode in SWEEP_MODES:
        mats, series, inits, refs = _wide_case(d, obs, mode)
        m = _cuda_model(mats, dtype)
        ts, xs, ob, nv = _inputs(series, mode, dtype)
        init = leg.FilterState(*(torch.stack([st[j] for st in inits]).to(dtype).cuda() for j in range(3)))
        for ch in CHUNKINGS:
            out = leg.filter_predictive_batch(m, ts, xs, lengths=list(LENGTHS), observed=ob, noise_var=nv, init=init, chunk_rows=ch)
            scan = _wide_scan_refs(d, obs, mode, ch, dtype)
            rows = []
            for j, key in enumerate(ROWS + ("loglik",)):
                rows.append((_errors(out[j], refs, key), _errors(_gather(scan, key), refs, key), key))
            worst = max(rows)
            print("channel forms wide state chunk_rows %s %s d %d obs %d %s: worst error %.3e (%s; the scan in torch %.3e)"
                  % (ch, NAME[dtype], d, obs, mode, worst[0], worst[2], worst[1]))
            for e_lib, e_ref, key in rows:
                assert e_lib <= max(4 * e_ref, WIDE_FLOOR[dtype]), (mode, ch, key, e_lib, e_ref)
            _assert_state_is_the_last_row(out, ts)


@pytest.mark.parametrize("d,obs", WIDE_PAIRS)
def test_the_wide_states_make_the_scan_exchange_rows(d, obs, monkeypatch):
    seen = []
    combine = _scanref.combine

    def counting(e1, e2, reset2=False):
        if not reset2:
            seen.append(_exchanges(torch.eye(d, dtype=F64) + e1[2] @ e2[4]))
        return combine(e1, e2, reset2)

    monkeypatch.setattr(_scanref, "combine", counting)
    for mode in SWEEP_MODES:
        mats, series, inits, _ = _wide_case(d, obs, mode)
        for ch in CHUNKINGS:
            _scanref.scan_filter_ref(mats, [_truth_args(sr, mode) + (st,) for sr, st in zip(series, inits)], *_fanout(ch))
    assert len(seen) >= 20 and sum(seen) >= 1, "no combine exchanges a row (pick another seed): %d of %d" % (sum(seen), len(seen))
    # ... and the sweep's own cases do not, which is why this section exists
    del seen[:]
    for mode in SWEEP_MODES:
        mats, series, _ = _filter_case(d, obs, LENGTHS, _filter_seed(d, obs), mode)
        _scanref.scan_filter_ref(mats, [_truth_args(sr, mode) + (None,) for sr in series], 2, 2)
    assert len(seen) >= 4 and sum(seen) == 0


# ---- d. without a GPU: the reference, the inputs, the list of forms ------------------------------------------------------
@PAIR
def test_the_recursion_in_torch_holds_the_truths_at_the_sweeps_cases(d, obs):
    for mode in SWEEP_MODES:
        _, series, truth = _filter_case(d, obs, LENGTHS, _filter_seed(d, obs), mode)
        if mode == "both":
            _assert_mask_covers(series, obs)
            six = series[2][2]
            assert six.shape[0] == 6 and not bool(six[[0, 3, 5]].any()), "the 6-row series: rows 0, 3, 5 observe nothing"
        refs = _refs(d, obs, mode, F64)
        for key in ROWS + ("loglik",):
            got, want = _gather(refs, key), _gather(truth, key)
            err = float(((got.reshape(want.shape) - want).abs() / (1 + want.abs())).max())
            assert err <= REF_BOUND, (mode, key, err)
        for r in _refs(d, obs, mode, F32):
            assert all(bool(torch.isfinite(r[key]).all()) for key in ROWS + ("loglik",)), mode


@PAIR
def test_the_loo_cases_are_well_conditioned(d, obs):
    _, series, truth = _loo_case(d, obs, LENGTHS, _loo_seed(d, obs), "both")
    assert [sr[0].shape[0] for sr in series] == list(LENGTHS)
    for leave in LEAVES:
        _conditioning(truth[leave])


def test_the_sweep_covers_every_compiled_channel_form():
    """dispatch_obs maps obs to the compile-time O of the four kernels: exactly 1, 2, 3, 4 -> themselves and everything
    else -> 8.  A new form (an O = 5, say) fails this until the sweep is extended to run it."""
    text = open(os.path.join(ROOT, "cyclic-gps_amd", "csrc", "cgps_host.h")).read()
    body = re.search(r"void dispatch_obs\(int obs, Fn&& fn\) \{\n  switch \(obs\) \{\n(.*?)\n  \}\n\}", text, re.S)
    assert body, "dispatch_obs not found in cgps_host.h"
    lines = [l.strip() for l in body.group(1).splitlines() if l.strip()]
    forms = {}
    for l in lines:
        hit = re.fullmatch(r"(case (\d+)|default): fn\(std::integral_constant<int, (\d+)>\{\}\); break;", l)
        assert hit, "a line of dispatch_obs this test does not understand: %r" % l
        forms[int(hit.group(2)) if hit.group(2) else "default"] = int(hit.group(3))
    assert forms == {1: 1, 2: 2, 3: 3, 4: 4, "default": 8}, forms
    assert {obs for _, obs in PAIRS} == set(range(1, 9)) and {d for d, _ in PAIRS} == set(range(1, 9)) and len(PAIRS) == 64

"""The LEG assembly at time gaps far below (and far above) the length scale 1 / |G| of the kernel, against truths that do
not go through the block formula the kernels evaluate:

* the blocks themselves against tests/golden/leg_gap_blocks.npz (60-digit evaluation, tests/golden/make_golden_gaps.py),
  gap * |G|_1 from 1e-7 (fp64) or 1e-5 (fp32) to 2e3;
* log-likelihoods and gradients against the covariance form of the model (tests/_gapref.prior_covariance), in which
  nothing is of size 1 / gap.

The reference's  (I - E E^T)^-1 E  loses eps / (gap |G|) of relative precision to the subtraction; the kernels form it
from F = E - I (csrc/cgps_leg.h: mat_expm1, gap_gram).  Error of a block: |got - true|_max / max(1, |true|_max)."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import _gapref as gp
import _gradref as gr
import _missref as mr
import _noiseref as nr
import _util
from oracle import cr_oracle as O
from cyclic_gps import leg

F64, F32 = torch.float64, torch.float32
NAME = {F32: "f32", F64: "f64"}
EPS = {F32: float(torch.finfo(F32).eps), F64: float(torch.finfo(F64).eps)}
DTYPES = pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])

# ---- the blocks ------------------------------------------------------------------------------------------------------
BLOCK_BOUND_CPU = 256.0
"""eps.  a = M^-1 E^T with M = I - E^T E ~ gap sym(G): M formed to a few eps per entry (three terms of its own size and a
d-term product) and a backward stable solve leave about 4 cond(M) eps in the blocks; the fixture's models have
cond(sym(G)) <= 64.  The reference's formula needs up to 1e6 eps (fp32) and 1e8 eps (fp64) on this grid."""

BLOCK_MEASURED_GPU = {F32: 11.09, F64: 13.62}
"""Largest err / eps of cgps_peg_precision over the grid (d = 1..8), measured on an MI355X; asserted with a margin of
8 (Taylor and Cholesky rounding differ from torch's), which stays below the 256 eps above."""


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(_util.GOLDEN, "leg_gap_blocks.npz"))


def _fixture(d, dtype):
    g = _golden()
    t = lambda k: torch.from_numpy(g["%s_d%d_%s" % (NAME[dtype], d, k)])   # noqa: E731
    return t("G"), t("ts"), t("Rs"), t("Os")


def _block_err_eps(Rs, Os, tRs, tOs, dtype):
    return max(gp.block_error(Rs, tRs), gp.block_error(Os, tOs)) / EPS[dtype]


@DTYPES
def test_blocks_on_the_cpu_against_60_digits(dtype):
    """``_gapref.blocks_cancel_free`` and the CPU branch of ``leg.peg_precision``, every block size."""
    for d in range(1, 9):
        G, ts, tRs, tOs = _fixture(d, dtype)
        assert G.dtype == dtype and ts.dtype == dtype and tRs.dtype == F64
        for what, fn in (("recipe", lambda: gp.blocks_cancel_free(ts, G, dtype)), ("leg", lambda: leg.peg_precision(ts, G))):
            Rs, Os = fn()
            assert Rs.dtype == dtype and Os.dtype == dtype
            err = _block_err_eps(Rs, Os, tRs, tOs, dtype)
            print("cpu %s d=%d %s: %.1f eps" % (what, d, NAME[dtype], err))
            assert err <= BLOCK_BOUND_CPU, (what, d, err)


@pytest.mark.gpu
@DTYPES
def test_peg_precision_kernel_against_60_digits(dtype):
    """cgps_peg_precision, every block size; the same series through cgps_peg_precision_seg with no cut is identical."""
    bound = 8 * BLOCK_MEASURED_GPU[dtype]
    assert bound <= 256
    worst = 0.0
    for d in range(1, 9):
        G, ts, tRs, tOs = _fixture(d, dtype)
        Rs, Os = leg.peg_precision(ts.cuda(), G.cuda())
        err = _block_err_eps(Rs.cpu(), Os.cpu(), tRs, tOs, dtype)
        worst = max(worst, err)
        print("gpu d=%d %s: %.1f eps" % (d, NAME[dtype], err))
        cut = torch.zeros(ts.shape[0] - 1, dtype=torch.uint8, device="cuda")
        sRs, sOs = leg._peg_precision_seg(ts.cuda(), G.cuda(), cut)
        assert torch.equal(sRs, Rs) and torch.equal(sOs, Os), d
    print("gpu %s: worst %.2f eps, bound %.1f" % (NAME[dtype], worst, bound))
    assert worst <= bound, worst


# ---- log-likelihoods -------------------------------------------------------------------------------------------------
CASES = [(1, 1, 24), (3, 2, 24), (5, 1, 24), (7, 3, 16), (3, 2, 300)]
UNFUSED_ONLY = [(6, 2, 24, F64), (8, 2, 24, F64)]          # no fused kernel for these: once each
SCALES = {F32: (1.0, 1e-2, 1e-3, 1e-4), F64: (1.0, 1e-2, 1e-3, 1e-4, 1e-6)}
MIXED = "mixed"                                             # gaps from 1e-5 to 10 in one series


@functools.lru_cache(maxsize=None)
def _series(d, obs, n, scale, dtype):
    """([N, R, B, Lambda, xs, ts, s], mask) of ``_noiseref.leg_case(d, obs, n, 7)`` with the gaps scale * (0.2 + U[0, 1))
    (MIXED: 10^U[-5, 1]) from t = 0 on, every tensor rounded to ``dtype`` and returned in fp64: the truth is evaluated
    from what the kernel is given."""
    case, mask = nr.leg_case(d, obs, n, 7)
    gen = torch.Generator().manual_seed(1000 + n)
    u = torch.rand(n, generator=gen, dtype=F64)
    gaps = 10.0 ** (6.0 * u - 5.0) if scale == MIXED else scale * (0.2 + u)
    case[5] = torch.cumsum(gaps, 0)
    case = [t.to(dtype).to(F64) for t in case]
    assert bool((case[5][1:] > case[5][:-1]).all())
    return case, mask


@functools.lru_cache(maxsize=None)
def _truth(d, obs, n, scale, dtype, path):
    (Nm, Rm, Bm, Lm, xs, ts, s), mask = _series(d, obs, n, scale, dtype)
    if path == "observed":
        return float(mr.leg_dense_loglik(Nm, Rm, Bm, Lm, ts, xs, mask))
    if path == "noise":
        return float(nr.leg_dense_loglik(Nm, Rm, Bm, Lm, ts, xs, s, torch.ones_like(mask)))
    return float(gr.leg_dense_loglik(Nm, Rm, Bm, Lm, ts, xs))


def _emulated_ll(Nm, Rm, Bm, Lm, xs, ts, dtype):
    """``leg.log_likelihood`` on the CPU in ``dtype``: cancellation-free blocks, the oracle's cyclic reduction."""
    Nm, Rm, Bm, Lm, xs, ts = (t.to(dtype) for t in (Nm, Rm, Bm, Lm, xs, ts))
    m = leg.LEGMatrices(Nm, Rm, Bm, Lm)
    LLT = m.LLT
    Li = torch.linalg.inv(LLT)
    xl = xs @ Li
    v = xl @ m.B
    n = xs.shape[0]
    Rs, Os = gp.blocks_cancel_free(ts, m.G, dtype)
    _, sig = O.mahal_and_det(Rs, Os, torch.zeros_like(v))
    k_mahal, k_det = O.mahal_and_det(Rs + m.B.T @ Li @ m.B, Os, v)
    return -0.5 * (((xl * xs).sum() - k_mahal) + (n * torch.logdet(2 * math.pi * LLT) + k_det - sig))


@functools.lru_cache(maxsize=None)
def _emulation_error(d, obs, n, scale, dtype):
    case, _ = _series(d, obs, n, scale, dtype)
    with torch.no_grad():
        return abs(float(_emulated_ll(*case[:6], dtype)) - _truth(d, obs, n, scale, dtype, "all"))


def _bound(scale, dtype, ll, extra=()):
    """8 x the largest error of the CPU emulation over this scale's cases, plus 64 eps(fp64) |ll|"""
    cases = [MIXED_CASE] if scale == MIXED else CASES + list(extra)
    return 8 * max(_emulation_error(d, obs, n, scale, dtype) for d, obs, n in cases) + 64 * EPS[F64] * abs(ll)


MIXED_CASE = (3, 2, 24)


def _gpu(case, dtype):
    Nm, Rm, Bm, Lm, xs, ts, s = (t.to(dtype).cuda() for t in case)
    return leg.LEGMatrices(Nm, Rm, Bm, Lm), ts, xs, s


def _check(what, got, want, bound):
    got = float(got.detach()) if isinstance(got, torch.Tensor) else float(got)
    print("%s: ll %.10g truth %.10g error %.3g bound %.3g" % (what, got, want, abs(got - want), bound))
    assert math.isfinite(got), what
    assert abs(got - want) <= bound, (what, got, want, bound)


def _scales_of(dtype):
    return [(str(s), s) for s in SCALES[dtype]] + [(MIXED, MIXED)]


def _cases_of(scale):
    return [MIXED_CASE] if scale == MIXED else CASES


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("path", ["fused", "unfused", "observed", "noise"])
def test_log_likelihood_against_the_covariance_form(path, dtype, monkeypatch):
    """``leg.log_likelihood`` at every gap scale: fused, unfused (CGPS_LEG_UNFUSED=1), with ``observed=`` and with
    ``noise_var=``.  No scale raises NotPSDError or returns a value that is not finite."""
    if path == "unfused":
        monkeypatch.setenv("CGPS_LEG_UNFUSED", "1")
    for sid, scale in _scales_of(dtype):
        for d, obs, n in _cases_of(scale):
            case, mask = _series(d, obs, n, scale, dtype)
            m, ts, xs, s = _gpu(case, dtype)
            assert leg.fused_supported(ts, m.G) == (path != "unfused")
            if path == "observed":
                got = leg.log_likelihood(m, ts, xs, observed=mask.cuda())
            elif path == "noise":
                got = leg.log_likelihood(m, ts, xs, noise_var=s)
            else:
                got = leg.log_likelihood(m, ts, xs)
            want = _truth(d, obs, n, scale, dtype, path if path in ("observed", "noise") else "all")
            _check("%s %s scale %s d=%d obs=%d n=%d" % (path, NAME[dtype], sid, d, obs, n), got, want,
                   _bound(scale, dtype, want))


@pytest.mark.gpu
@DTYPES
def test_log_likelihood_batch_against_the_covariance_form(dtype):
    """The scales as the series of one ragged batch (cgps_leg_loglik_batch), one batch per case."""
    for d, obs, n in CASES:
        series = [_series(d, obs, n, scale, dtype)[0] for scale in SCALES[dtype]]
        m, _, _, _ = _gpu(series[0], dtype)
        ts = torch.cat([c[5] for c in series]).to(dtype).cuda()
        xs = torch.cat([c[4] for c in series]).to(dtype).cuda()
        assert leg.batch_supported(ts, m.G)
        out = leg.log_likelihood_batch(m, ts, xs, lengths=[n] * len(series))
        for scale, got in zip(SCALES[dtype], out.tolist()):
            want = _truth(d, obs, n, scale, dtype, "all")
            _check("batch %s scale %s d=%d obs=%d n=%d" % (NAME[dtype], scale, d, obs, n), got, want,
                   _bound(scale, dtype, want))


@pytest.mark.gpu
@pytest.mark.parametrize("d,obs,n,dtype", UNFUSED_ONLY, ids=["d6_fp64", "d8_fp64"])
def test_log_likelihood_of_block_sizes_without_a_fused_kernel(d, obs, n, dtype):
    for scale in SCALES[dtype]:
        case, _ = _series(d, obs, n, scale, dtype)
        m, ts, xs, _ = _gpu(case, dtype)
        assert not leg.fused_supported(ts, m.G)
        want = _truth(d, obs, n, scale, dtype, "all")
        _check("d=%d %s scale %s" % (d, NAME[dtype], scale), leg.log_likelihood(m, ts, xs), want,
               _bound(scale, dtype, want, extra=[(d, obs, n)]))


# ---- gradients -------------------------------------------------------------------------------------------------------
GRAD_CASE = (3, 2, 24, 1e-3, F64)
LEG_PARAMS = ("N", "R", "B", "Lambda", "xs", "ts")


@pytest.mark.gpu
def test_gradients_at_small_gaps_against_the_covariance_form():
    """All six arguments at gaps of 1e-3, fp64, against autograd through the covariance-form density.  Bound per
    argument: 8 x the error of the CPU emulation's gradient (autograd through ``blocks_cancel_free`` and the oracle's
    reduction) plus 64 eps |gradient|_max."""
    d, obs, n, scale, dtype = GRAD_CASE
    case, _ = _series(d, obs, n, scale, dtype)
    ll, grads = gr.leg_dense_value_and_grads(*case[:4], case[5], case[4])
    leaves = [t.clone().requires_grad_(True) for t in case[:6]]
    emu = torch.autograd.grad(_emulated_ll(*leaves, dtype), leaves)
    p = [t.to(dtype).cuda().requires_grad_(True) for t in case[:6]]
    out = leg.log_likelihood(leg.LEGMatrices(*p[:4]), p[5], p[4])
    _check("value with a graph", out, float(ll), _bound(scale, dtype, float(ll)))
    out.backward()
    for name, leaf, want, e in zip(LEG_PARAMS, p, grads, emu):
        size = float(want.abs().max())
        bound = 8 * float((e - want).abs().max()) + 64 * EPS[F64] * size
        err = float((leaf.grad.cpu() - want).abs().max())
        print("d ll / d %s: |grad| %.3g error %.3g bound %.3g" % (name, size, err, bound))
        assert err <= bound, (name, err, bound)

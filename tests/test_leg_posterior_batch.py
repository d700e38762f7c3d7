"""The posterior and the predictions of many independent LEG series in one call (leg.insample_posterior_batch,
predict.predictive_posterior_batch, predict.make_predictions_batch: DESIGN.md 4.14) against the per-series loop of
leg.insample_posterior + predict.intercast, against dense fp64 truths (_missref, _noiseref) and against the results
recorded from the reference (tests/golden/leg_*.npz).  Validation and the empty batch run without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import _missref as mr
import _noiseref as nr
import _util
from cyclic_gps import leg, predict
from test_leg_intercast_seg import LENGTHS, standard_targets

F64 = torch.float64
EPS32 = float(torch.finfo(torch.float32).eps)
MODES = ["plain", "observed", "noise", "both"]


# ---- one model, many series ----------------------------------------------------------------------------------------
def _model(d, obs, seed, dtype=F64, device="cpu"):
    """(leg.LEGMatrices, its four fp64 CPU matrices): the model of _missref.leg_case(d, obs, ., seed), which draws it
    before anything that depends on the length."""
    (Nm, Rm, Bm, Lm, _, _), _ = mr.leg_case(d, obs, 4, seed)
    return leg.LEGMatrices(*(t.to(dtype).to(device) for t in (Nm, Rm, Bm, Lm))), (Nm, Rm, Bm, Lm)


def _series(obs, lengths, seed):
    """Per series (fp64, CPU): ts, xs, mask [n, obs] and noise variances [n, obs].  The masks keep ~70 % of the entries;
    a series of five rows or more has its first, its last and an interior row wholly missing."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for b, n in enumerate(lengths):
        ts = 3.0 - 1.1 * (b % 3) + torch.cumsum(0.2 + torch.rand(n, generator=gen, dtype=F64), 0)
        xs = torch.randn(n, obs, generator=gen, dtype=F64)
        mask = torch.rand(n, obs, generator=gen) < 0.7
        if n >= 5:
            mask[0] = mask[n - 1] = mask[n // 2] = False
        s = 2.0 * torch.rand(n, obs, generator=gen, dtype=F64)
        out.append((ts, xs, mask, s))
    return out


def _mode_args(mode, mask, s):
    return (mask if mode in ("observed", "both") else None), (s if mode in ("noise", "both") else None)


def _ragged(series, dtype, device="cuda"):
    c = lambda k, dt: torch.cat([sr[k] for sr in series]).to(dt).to(device)      # noqa: E731
    return c(0, dtype), c(1, dtype), c(2, torch.bool), c(3, dtype)


def _loop_posterior(m, series, mode, dtype):
    """The per-series loop: leg.insample_posterior for each series -> lists of (mean, cov_diag, cov_off)."""
    out = []
    for ts, xs, mask, s in series:
        ob, nv = _mode_args(mode, mask.cuda(), s.to(dtype).cuda())
        xs_ = xs.to(dtype).cuda()
        if ob is not None:
            xs_ = torch.where(ob, xs_, torch.full_like(xs_, float("nan")))           # unobserved entries are ignored
        mean, (Sd, So) = leg.insample_posterior(m, ts.to(dtype).cuda(), xs_, observed=ob, noise_var=nv)
        out.append((mean, Sd, So))
    return out


def _batch_posterior_ragged(m, series, mode, dtype):
    ts, xs, mask, s = _ragged(series, dtype)
    ob, nv = _mode_args(mode, mask, s)
    if ob is not None:
        xs = torch.where(ob, xs, torch.full_like(xs, float("nan")))
    return leg.insample_posterior_batch(m, ts, xs, lengths=[sr[0].shape[0] for sr in series], observed=ob, noise_var=nv)


def _split(mean, Sd, So, lengths):
    """Per-series (mean, cov_diag, cov_off) of a ragged result."""
    out, s = [], 0
    for n in lengths:
        out.append((mean[s:s + n], Sd[s:s + n], So[s:s + n - 1]))
        s += n
    return out


def _dense_truth(mats, sr, mode):
    """fp64 truth of one series: (mean [n, d], cov_diag [n, d, d], cov_off [n-1, d, d]) from ONE dense Gaussian."""
    ts, xs, mask, s = sr
    n = ts.shape[0]
    full = torch.ones_like(mask)
    xs = torch.where(mask, xs, torch.zeros_like(xs)) if mode in ("observed", "both") else xs
    if mode in ("noise", "both"):
        mean, cov = nr.leg_dense_posterior(*mats, ts, xs, s, mask if mode == "both" else full)
    else:
        mean, cov = mr.leg_dense_posterior(*mats, ts, xs, mask if mode == "observed" else full)
    i = torch.arange(n)
    return mean, cov[i, :, i, :], cov[i[1:], :, i[:-1], :]


# ---- without a GPU -------------------------------------------------------------------------------------------------
def _cpu_case(B=3, n=4, obs=2, d=3):
    m, _ = _model(d, obs, 5)
    ts = torch.cumsum(torch.ones(B, n, dtype=F64), 1)
    return m, ts, torch.zeros(B, n, obs, dtype=F64)


def test_validation_errors_come_before_anything_runs():
    m, ts, xs = _cpu_case()
    B, n, obs = xs.shape
    tsr, xsr, lens = ts.reshape(-1), xs.reshape(B * n, obs), [n] * B
    tt = torch.tensor([0.5, 1.5], dtype=F64)
    post, pp, mp = leg.insample_posterior_batch, predict.predictive_posterior_batch, predict.make_predictions_batch
    bad = [
        # layouts
        lambda: post(m, ts, xsr),
        lambda: post(m, ts[:, :3], xs),
        lambda: post(m, ts, xs[..., :1]),                                   # the model has two channels
        lambda: post(m, tsr, xsr, lengths=[n] * (B - 1)),                   # lengths do not sum to the rows
        lambda: post(m, tsr, xsr, lengths=[n, n, n - 1, 1, 0]),             # an empty series
        lambda: post(m, tsr, xsr, lengths=torch.tensor([4.0, 4.0, 4.0])),
        lambda: post(m, ts, xsr, lengths=lens),
        # masks and variances of the wrong kind or shape
        lambda: post(m, ts, xs, observed=torch.ones(B, n, obs)),
        lambda: post(m, ts, xs, observed=torch.ones(B, n + 1, dtype=torch.bool)),
        lambda: post(m, tsr, xsr, lengths=lens, observed=torch.ones(B, n, obs, dtype=torch.bool)),
        lambda: post(m, ts, xs, noise_var=torch.ones(B, n, obs, dtype=torch.int64)),
        lambda: post(m, ts, xs, noise_var=torch.ones(B, n, obs + 1, dtype=F64)),
        lambda: post(m, tsr, xsr, lengths=lens, noise_var=torch.ones(B * n + 1, dtype=F64)),
        # targets
        lambda: pp(m, ts, xs, torch.ones(B + 1, 2, dtype=F64)),
        lambda: pp(m, ts, xs, torch.ones(B, 2, 2, dtype=F64)),
        lambda: pp(m, ts, xs, tt, target_lengths=[2] * B),                  # target_lengths is the ragged layout's
        lambda: pp(m, ts, xs, torch.ones(2, dtype=torch.int64)),
        lambda: pp(m, tsr, xsr, tt, lengths=lens),                          # ragged without target_lengths
        lambda: pp(m, tsr, xsr, tt, lengths=lens, target_lengths=[1, 1]),
        lambda: pp(m, tsr, xsr, tt, lengths=lens, target_lengths=[1, 1, 1]),
        lambda: pp(m, tsr, xsr, tt, lengths=lens, target_lengths=[3, -1, 0]),
        lambda: pp(m, tsr, xsr, tt, lengths=lens, target_lengths=torch.tensor([1.0, 1.0, 0.0])),
        lambda: pp(m, tsr, xsr, tt.reshape(1, 2), lengths=lens, target_lengths=[2, 0, 0]),
        lambda: mp(m, tsr, xsr, tt, lengths=[n] * (B - 1), target_lengths=[2, 0]),
        lambda: mp(m, ts, xs, tt, observed=torch.ones(B, n + 1, dtype=torch.bool)),
        lambda: mp(m, tsr, xsr, tt, lengths=lens, target_lengths=[1, 1]),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d raised nothing" % k)


def test_empty_batch_returns_empty_tensors():
    m, ts, xs = _cpu_case()
    d, obs, n = 3, 2, 4
    mean, (Sd, So) = leg.insample_posterior_batch(m, ts[:0], xs[:0])
    assert mean.shape == (0, n, d) and Sd.shape == (0, n, d, d) and So.shape == (0, n - 1, d, d)
    mean, (Sd, So) = leg.insample_posterior_batch(m, ts.reshape(-1)[:0], xs.reshape(-1, obs)[:0], lengths=[])
    assert mean.shape == (0, d) and Sd.shape == (0, d, d) and So.shape == (0, d, d) and mean.dtype == F64
    tt = torch.tensor([0.5, 1.5, 2.5], dtype=F64)
    for fn, w in ((predict.predictive_posterior_batch, d), (predict.make_predictions_batch, obs)):
        pm, pv = fn(m, ts[:0], xs[:0], tt)
        assert pm.shape == (0, 3, w) and pv.shape == (0, 3, w, w)
        pm, pv = fn(m, ts[:0], xs[:0], tt.reshape(1, 3)[:0])
        assert pm.shape == (0, 3, w) and pv.shape == (0, 3, w, w)
        pm, pv = fn(m, ts.reshape(-1)[:0], xs.reshape(-1, obs)[:0], tt[:0], lengths=[], target_lengths=[])
        assert pm.shape == (0, w) and pv.shape == (0, w, w)
        # series, but no target anywhere: nothing to launch either
        pm, pv = fn(m, ts.reshape(-1), xs.reshape(-1, obs), tt[:0], lengths=[n] * 3, target_lengths=[0, 0, 0])
        assert pm.shape == (0, w) and pv.shape == (0, w, w)


def test_blocks_entry_is_exported_and_checks_its_arguments_before_any_launch():
    import ctypes
    from cyclic_gps import _hip
    assert "cgps_leg_posterior_blocks_seg" in _hip.exported_symbols() and "cgps_leg_intercast_seg" in _hip.exported_symbols()
    lib = _hip.lib()
    fn = lib.cgps_leg_posterior_blocks_seg
    f = ctypes.c_void_p(4096)                                    # never dereferenced: every call below returns first

    def call(N=8, d=3, dtype=_hip.F64, source=_hip.ROWS_TABLE, entries=4, ts=f, G=f, cut=f, term=f, rows=f, K=f, Os=f, info=f):
        return fn(ts, G, cut, N, d, dtype, source, term, entries, rows, K, Os, info, None)

    assert call(ts=None) == 1 and b"cgps_leg_posterior_blocks_seg" in lib.cgps_last_error()
    for hole in ("G", "term", "K", "Os", "info", "rows"):
        assert call(**{hole: None}) == 1, hole
    assert call(N=0) == 1
    assert call(source=3) == 1 and call(source=-1) == 1
    assert call(entries=0) == 1 and call(entries=257) == 1
    assert call(source=_hip.ROWS_WEIGHTED, entries=0) == 1 and call(source=_hip.ROWS_WEIGHTED, entries=65) == 1
    assert call(source=_hip.ROWS_WEIGHTED, rows=None) == 1
    assert call(d=9) == 3 and call(d=0) in (1, 3) and call(dtype=7) == 3
    assert call(source=_hip.ROWS_PLAIN, rows=None, entries=0, d=9) == 3    # (plain reads neither; a null cut is one series)
    assert lib.cgps_version() == 320


def test_target_plan_marks_the_pairs_that_span_two_series():
    tp = predict._TargetPlan([2, 0, 3, 0, 1], "cpu")
    assert tp.offsets.tolist() == [0, 2, 2, 5, 5, 6] and tp.P == 6
    assert tp.across.tolist() == [False, True, False, False, True]
    assert predict._TargetPlan([0, 0], "cpu").across.numel() == 0 and predict._TargetPlan([0, 4], "cpu").across.sum() == 0


# ---- on the GPU ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("d", range(1, 9))
def test_batched_posterior_equals_the_per_series_loop_fp64(d):
    """Every rank, ragged (the standard lengths) and dense, plain / observed / noise / both.  The concatenated reduction
    pairs rows differently from a series' own, so the results are not bit-equal: rtol 1e-9, atol 1e-11, what
    test_hip_intercast_against_torch_ops asks of the same kind of comparison."""
    obs = 1 + d % 3
    m, _ = _model(d, obs, 70 + d, F64, "cuda")
    series = _series(obs, LENGTHS, 500 + d)
    tol = dict(rtol=1e-9, atol=1e-11)
    for mode in MODES:
        want = _loop_posterior(m, series, mode, F64)
        mean, (Sd, So) = _batch_posterior_ragged(m, series, mode, F64)
        R = sum(LENGTHS)
        assert mean.shape == (R, d) and Sd.shape == (R, d, d) and So.shape == (R - 1, d, d)
        for b, (got, ref) in enumerate(zip(_split(mean, Sd, So, LENGTHS), want)):
            for g_, r_, what in zip(got, ref, ("mean", "cov_diag", "cov_off")):
                np.testing.assert_allclose(g_.cpu().numpy(), r_.cpu().numpy(), err_msg="%s series %d %s" % (mode, b, what), **tol)
    # dense: three series of 33 rows
    dense = _series(obs, [33, 33, 33], 900 + d)
    st = lambda k, dt: torch.stack([sr[k] for sr in dense]).to(dt).cuda()            # noqa: E731
    for mode in MODES:
        want = _loop_posterior(m, dense, mode, F64)
        ob, nv = _mode_args(mode, st(2, torch.bool), st(3, F64))
        mean, (Sd, So) = leg.insample_posterior_batch(m, st(0, F64), st(1, F64), observed=ob, noise_var=nv)
        assert mean.shape == (3, 33, d) and Sd.shape == (3, 33, d, d) and So.shape == (3, 32, d, d)
        for b, ref in enumerate(want):
            for g_, r_ in zip((mean[b], Sd[b], So[b]), ref):
                np.testing.assert_allclose(g_.cpu().numpy(), r_.cpu().numpy(), err_msg="dense %s series %d" % (mode, b), **tol)


SMALL = [n for n in LENGTHS if n <= 33]                        # [1, 2, 3, 33, 5]


@pytest.mark.gpu
@pytest.mark.parametrize("d", range(1, 9))
def test_batched_posterior_fp32_is_as_accurate_as_the_loop(d):
    """fp32 against the dense fp64 truth (one Gaussian per series: _missref / _noiseref), series of at most 33 rows: the
    batched call's largest error is at most 4 times the loop's largest error against the same truth plus
    16 eps32 max|truth| -- a different but equally deep order of the same reduction.  (d <= 3 is the case the feature
    was specified with; the higher ranks are held to the same bound.)"""
    obs = 1 + d % 3
    m, mats = _model(d, obs, 70 + d, torch.float32, "cuda")
    series = _series(obs, SMALL, 600 + d)
    for mode in MODES:
        truth = [_dense_truth(mats, sr, mode) for sr in series]
        loop = _loop_posterior(m, series, mode, torch.float32)
        mean, (Sd, So) = _batch_posterior_ragged(m, series, mode, torch.float32)
        assert mean.dtype == torch.float32
        batch = _split(mean, Sd, So, SMALL)
        for k, what in enumerate(("mean", "cov_diag", "cov_off")):
            err = lambda res: max(float((r[k].double().cpu() - t[k]).abs().max()) for r, t in zip(res, truth) if t[k].numel())  # noqa: E731
            scale = max(float(t[k].abs().max()) for t in truth if t[k].numel())
            e_batch, e_loop = err(batch), err(loop)
            print("d=%d %s %s: batch %.3e loop %.3e scale %.3e" % (d, mode, what, e_batch, e_loop, scale))
            assert e_batch <= 4 * e_loop + 16 * EPS32 * scale, (mode, what, e_batch, e_loop, scale)
    # the dense layout: three series of 33 rows, the same bound
    dense = _series(obs, [33, 33, 33], 650 + d)
    st = lambda k, dt: torch.stack([sr[k] for sr in dense]).to(dt).cuda()            # noqa: E731
    for mode in MODES:
        truth = [_dense_truth(mats, sr, mode) for sr in dense]
        loop = _loop_posterior(m, dense, mode, torch.float32)
        ob, nv = _mode_args(mode, st(2, torch.bool), st(3, torch.float32))
        mean, (Sd, So) = leg.insample_posterior_batch(m, st(0, torch.float32), st(1, torch.float32), observed=ob, noise_var=nv)
        assert mean.shape == (3, 33, d) and Sd.shape == (3, 33, d, d) and So.shape == (3, 32, d, d)
        batch = [(mean[b], Sd[b], So[b]) for b in range(3)]
        for k, what in enumerate(("mean", "cov_diag", "cov_off")):
            err = lambda res: max(float((r[k].double().cpu() - t[k]).abs().max()) for r, t in zip(res, truth))  # noqa: E731
            scale = max(float(t[k].abs().max()) for t in truth)
            e_batch, e_loop = err(batch), err(loop)
            print("dense d=%d %s %s: batch %.3e loop %.3e scale %.3e" % (d, mode, what, e_batch, e_loop, scale))
            assert e_batch <= 4 * e_loop + 16 * EPS32 * scale, ("dense", mode, what, e_batch, e_loop, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("obs", [1, 3])
@pytest.mark.parametrize("d", [2, 5])
def test_batched_posterior_against_the_dense_truth_fp64(d, obs):
    """_missref and _noiseref cases, lengths [1, 2, 7, 33]: mean, diagonal and off-diagonal blocks at the tolerance
    test_leg.py asks of the posterior against recorded truth."""
    lengths = [1, 2, 7, 33]
    m, mats = _model(d, obs, 21 + d + obs, F64, "cuda")
    for ref, noisy in ((mr, False), (nr, True)):
        cases = [ref.leg_case(d, obs, n, 21 + d + obs) for n in lengths]
        for c, _ in cases:
            assert all(torch.equal(a, b) for a, b in zip(c[:4], mats))               # one model for all lengths
        cat = lambda k: torch.cat([c[k] for c, _ in cases]).cuda()                   # noqa: E731
        mask = torch.cat([mk for _, mk in cases]).cuda()
        xs = torch.where(mask, cat(4), torch.full_like(cat(4), float("nan")))
        mean, (Sd, So) = leg.insample_posterior_batch(m, cat(5), xs, lengths=lengths, observed=mask,
                                                      noise_var=cat(6) if noisy else None)
        for (got_m, got_d, got_o), (c, mk) in zip(_split(mean, Sd, So, lengths), cases):
            xs0 = torch.where(mk, c[4], torch.zeros_like(c[4]))
            args = (c[0], c[1], c[2], c[3], c[5], xs0) + ((c[6],) if noisy else ())
            tm, tc = ref.leg_dense_posterior(*args, mk)
            i = torch.arange(tm.shape[0])
            np.testing.assert_allclose(got_m.cpu().numpy(), tm.numpy(), rtol=1e-7, atol=1e-9)
            np.testing.assert_allclose(got_d.cpu().numpy(), tc[i, :, i, :].numpy(), rtol=1e-7, atol=1e-9)
            np.testing.assert_allclose(got_o.cpu().numpy(), tc[i[1:], :, i[:-1], :].numpy(), rtol=1e-7, atol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("d", [1, 3, 5, 8])
def test_posterior_blocks_kernel_against_the_composition_it_replaces(d, dtype):
    """cgps_leg_posterior_blocks_seg.  Plain and table sources: K_Rs equals cgps_peg_precision_seg's Rs + A and
    + A_table[idx] bit for bit (one rounded add per element) and Os is equal; a pattern byte above entries - 1 reads the
    last entry.  Weighted source: within (Kb + 2) eps (|Rs| + sum_k |w_k| |basis_k|) of the fp64 evaluation, the bound of
    a Kb-term sum.  A null cut with the plain source is cgps_peg_precision + A."""
    from cyclic_gps import _hip
    eps = float(torch.finfo(dtype).eps)
    for obs in (1, 3):
        m, _ = _model(d, obs, 40 + d + obs, dtype, "cuda")
        series = _series(obs, LENGTHS, 300 + d + obs)
        ts, xs, mask, s = _ragged(series, dtype)
        plan = leg._cached_batch_plan(LENGTHS, ts.device)
        G = m.G.contiguous()
        Rs, Os = leg._peg_precision_seg(ts, G, plan.cut)
        # plain
        A = (m.B.T @ m.LLT_inv @ m.B).contiguous()
        K, Ko, info = leg._posterior_blocks_seg(ts, G, plan.cut, _hip.ROWS_PLAIN, A)
        assert torch.equal(K, Rs + A) and torch.equal(Ko, Os) and int(info) == 0
        # table, with bytes above entries - 1 (the clamp)
        pattern, A_table, _, _ = leg.observation_tables(m, mask)
        A_table = A_table.contiguous()
        pattern = pattern.clone()
        pattern[::7] = 255
        pattern[3] = A_table.shape[0]
        idx = pattern.long().clamp(max=A_table.shape[0] - 1)
        K, Ko, info = leg._posterior_blocks_seg(ts, G, plan.cut, _hip.ROWS_TABLE, A_table, pattern)
        assert torch.equal(K, Rs + A_table[idx]) and torch.equal(Ko, Os) and int(info) == 0
        # weighted
        basis, weights, _, _ = leg.observation_weights(m, mask, s)
        basis, weights = basis.contiguous(), weights.contiguous()
        Kb = basis.shape[0]
        K, Ko, info = leg._posterior_blocks_seg(ts, G, plan.cut, _hip.ROWS_WEIGHTED, basis, weights)
        want = Rs.double() + torch.einsum("nk,kij->nij", weights.double(), basis.double())
        bound = (Kb + 2) * eps * (Rs.double().abs() + torch.einsum("nk,kij->nij", weights.double().abs(), basis.double().abs()))
        assert bool(((K.double() - want).abs() <= bound).all()), float(((K.double() - want).abs() - bound).max())
        assert torch.equal(Ko, Os)
        # one series, null cut
        t1 = ts[plan.starts[6]:plan.starts[7]].contiguous()      # the series of 257 rows
        R1, O1 = leg._peg_precision_hip(t1, G)
        K, Ko, info = leg._posterior_blocks_seg(t1, G, None, _hip.ROWS_PLAIN, A)
        assert torch.equal(K, R1 + A) and torch.equal(Ko, O1)


def _golden(name):
    g = np.load(os.path.join(_util.GOLDEN, name + ".npz"))
    t = lambda k: torch.from_numpy(g[k]).to(F64).cuda()                              # noqa: E731
    return g, leg.LEGMatrices(t("N"), t("R"), t("B"), t("Lambda")), t("ts"), t("xs"), t("target_ts")


@pytest.mark.gpu
def test_batched_predictions_match_the_reference_recordings():
    """A ragged batch of leg_small_regular, leg_small_irregular and leg_small_regular again (one model), and eight copies
    of leg_co2like in the dense layout with the shared [784] targets: every slot at the tolerance of
    test_make_predictions_on_gpu."""
    tol = dict(rtol=1e-6, atol=1e-7)
    names = ["leg_small_regular", "leg_small_irregular", "leg_small_regular"]
    loaded = [_golden(nm) for nm in names]
    same = all(np.array_equal(loaded[0][0][k], lg[0][k]) for lg in loaded for k in ("N", "R", "B", "Lambda"))
    if not same:
        loaded = [loaded[0], loaded[0]]
    m = loaded[0][1]
    ts, xs, tt = (torch.cat([lg[k] for lg in loaded]) for k in (2, 3, 4))
    lens, tlens = [lg[2].shape[0] for lg in loaded], [lg[4].shape[0] for lg in loaded]
    pm, pv = predict.make_predictions_batch(m, ts, xs, tt, lengths=lens, target_lengths=tlens)
    lm, lv = predict.predictive_posterior_batch(m, ts, xs, tt, lengths=lens, target_lengths=tlens)
    k = 0
    for (g, *_), p in zip(loaded, tlens):
        for got, key in ((pm, "pred_mean"), (pv, "pred_cov"), (lm, "pp_mean"), (lv, "pp_cov")):
            np.testing.assert_allclose(got[k:k + p].cpu().numpy(), g[key], err_msg=key, **tol)
        k += p
    g, m, ts, xs, tt = _golden("leg_co2like")
    B = 8
    pm, pv = predict.make_predictions_batch(m, ts.expand(B, -1), xs.expand(B, -1, -1), tt)
    lm, lv = predict.predictive_posterior_batch(m, ts.expand(B, -1), xs.expand(B, -1, -1), tt.expand(B, -1))
    assert pm.shape == (B, 784, 1) and pv.shape == (B, 784, 1, 1) and lm.shape == (B, 784, 5) and lv.shape == (B, 784, 5, 5)
    for b in range(B):
        for got, key in ((pm, "pred_mean"), (pv, "pred_cov"), (lm, "pp_mean"), (lv, "pp_cov")):
            np.testing.assert_allclose(got[b].cpu().numpy(), g[key], err_msg="slot %d %s" % (b, key), **tol)


def _standard_prediction_inputs(d, obs, dtype, seed):
    series = _series(obs, LENGTHS, seed)
    tts = [standard_targets(sr[0], b) for b, sr in enumerate(series)]
    ts, xs, mask, s = _ragged(series, dtype)
    return series, tts, ts, xs, mask, s, torch.cat(tts).to(dtype).cuda(), [int(t.shape[0]) for t in tts]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_batched_predictions_equal_the_per_series_loop(dtype):
    """The standard batch with the standard targets (series without targets, one-row series, targets before / at /
    inside / on an observation / at the end / after it), observed= and noise_var= set: the batched call against
    insample_posterior + intercast per series.  fp64 at the tolerance of the posterior comparison; fp32 at the
    tolerance test_hip_intercast_against_torch_ops gives the same glue in fp32."""
    d, obs = 4, 2
    m, _ = _model(d, obs, 33, dtype, "cuda")
    series, tts, ts, xs, mask, s, tt, tlens = _standard_prediction_inputs(d, obs, dtype, 77)
    tol = dict(rtol=1e-9, atol=1e-11) if dtype == F64 else dict(rtol=2e-3, atol=2e-4)
    pm, pv = predict.predictive_posterior_batch(m, ts, xs, tt, lengths=LENGTHS, target_lengths=tlens, observed=mask, noise_var=s)
    om, ov = predict.make_predictions_batch(m, ts, xs, tt, lengths=LENGTHS, target_lengths=tlens, observed=mask, noise_var=s)
    assert pm.shape == (sum(tlens), d) and pv.shape == (sum(tlens), d, d) and ov.shape == (sum(tlens), obs, obs)
    assert not pm.requires_grad
    k = 0
    for (t1, x1, mk, s1), t_b in zip(series, tts):
        p = t_b.shape[0]
        if p:
            c = lambda t: t.to(dtype).cuda()                                         # noqa: E731
            mean, (Sd, So) = leg.insample_posterior(m, c(t1), c(x1), observed=mk.cuda(), noise_var=c(s1))
            rm, rv = predict.intercast(m, mean, (Sd, So), c(t1), c(t_b))
            np.testing.assert_allclose(pm[k:k + p].cpu().numpy(), rm.cpu().numpy(), **tol)
            np.testing.assert_allclose(pv[k:k + p].cpu().numpy(), rv.cpu().numpy(), **tol)
            np.testing.assert_allclose(om[k:k + p].cpu().numpy(), (rm @ m.B.T).cpu().numpy(), **tol)
            np.testing.assert_allclose(ov[k:k + p].cpu().numpy(), (m.B @ rv @ m.B.T).cpu().numpy(), **tol)
        k += p
    # the sortedness check looks inside every series and skips the boundaries (the series' times overlap)
    assert any(float(a[0]) <= float(b_[-1]) for a, b_ in zip(tts[3:], tts[2:]) if a.numel() and b_.numel())
    bad = tt.clone()
    k4 = sum(tlens[:4])
    bad[k4 + 1] = bad[k4]
    with pytest.raises(AssertionError):
        predict.predictive_posterior_batch(m, ts, xs, bad, lengths=LENGTHS, target_lengths=tlens)
    predict.predictive_posterior_batch(m, ts, xs, bad, lengths=LENGTHS, target_lengths=tlens, check_sorted=False)


@pytest.mark.gpu
def test_series_are_independent_and_the_result_is_reproducible():
    d, obs = 5, 2
    m, _ = _model(d, obs, 12, F64, "cuda")
    series, tts, ts, xs, mask, s, tt, tlens = _standard_prediction_inputs(d, obs, F64, 78)
    kw = dict(lengths=LENGTHS, observed=mask, noise_var=s)
    mean, (Sd, So) = leg.insample_posterior_batch(m, ts, xs, **kw)
    plan = leg._cached_batch_plan(LENGTHS, ts.device)
    cuts = torch.tensor(plan.starts[1:-1]) - 1
    assert torch.equal(So[cuts.cuda()], torch.zeros(len(cuts), d, d, dtype=F64, device="cuda"))     # exactly zero
    assert not torch.signbit(So[cuts.cuda()]).any()
    pm, pv = predict.make_predictions_batch(m, ts, xs, tt, target_lengths=tlens, **kw)
    # repeated calls
    mean2, (Sd2, So2) = leg.insample_posterior_batch(m, ts, xs, **kw)
    pm2, pv2 = predict.make_predictions_batch(m, ts, xs, tt, target_lengths=tlens, **kw)
    assert all(torch.equal(a, b) for a, b in ((mean, mean2), (Sd, Sd2), (So, So2), (pm, pm2), (pv, pv2)))
    # another series 4 (data and mask): nobody else moves by a bit
    b = 4
    lo, hi = plan.starts[b], plan.starts[b + 1]
    xs3, mask3 = xs.clone(), mask.clone()
    xs3[lo:hi] = 3.0 - 2.0 * xs[lo:hi]
    mask3[lo:hi] = ~mask[lo:hi]
    mean3, (Sd3, So3) = leg.insample_posterior_batch(m, ts, xs3, lengths=LENGTHS, observed=mask3, noise_var=s)
    pm3, pv3 = predict.make_predictions_batch(m, ts, xs3, tt, lengths=LENGTHS, target_lengths=tlens, observed=mask3, noise_var=s)
    rows = torch.ones(sum(LENGTHS), dtype=torch.bool)
    rows[lo:hi] = False
    gaps = rows[1:] & rows[:-1]
    tk = torch.ones(sum(tlens), dtype=torch.bool)
    tk[sum(tlens[:b]):sum(tlens[:b + 1])] = False
    assert torch.equal(mean3[rows.cuda()], mean[rows.cuda()]) and torch.equal(Sd3[rows.cuda()], Sd[rows.cuda()])
    assert torch.equal(So3[gaps.cuda()], So[gaps.cuda()])
    assert torch.equal(pm3[tk.cuda()], pm[tk.cuda()]) and torch.equal(pv3[tk.cuda()], pv[tk.cuda()])
    assert not torch.equal(mean3[lo:hi], mean[lo:hi]) and not torch.equal(Sd3[lo:hi], Sd[lo:hi])  # the change matters
    # dense and ragged layouts of the same data
    B, n, p = 3, 33, 6
    eq = _series(obs, [n] * B, 79)
    tq = torch.stack([torch.unique(torch.cat([sr[0][:1] - 0.4, 0.5 * (sr[0][4:8] + sr[0][5:9]), sr[0][-1:] + 0.3])) for sr in eq])
    assert tq.shape == (B, p)
    st = lambda k, dt: torch.stack([sr[k] for sr in eq]).to(dt).cuda()               # noqa: E731
    tsd, xsd, mkd, sd_, tqd = st(0, F64), st(1, F64), st(2, torch.bool), st(3, F64), tq.cuda()
    dm, (dSd, dSo) = leg.insample_posterior_batch(m, tsd, xsd, observed=mkd, noise_var=sd_)
    dpm, dpv = predict.predictive_posterior_batch(m, tsd, xsd, tqd, observed=mkd, noise_var=sd_)
    rkw = dict(lengths=[n] * B, observed=mkd.reshape(B * n, obs), noise_var=sd_.reshape(B * n, obs))
    rm, (rSd, rSo) = leg.insample_posterior_batch(m, tsd.reshape(-1), xsd.reshape(B * n, obs), **rkw)
    rpm, rpv = predict.predictive_posterior_batch(m, tsd.reshape(-1), xsd.reshape(B * n, obs), tqd.reshape(-1),
                                                  target_lengths=[p] * B, **rkw)
    assert torch.equal(dm.reshape(B * n, d), rm) and torch.equal(dSd.reshape(B * n, d, d), rSd)
    for b in range(B):
        assert torch.equal(dSo[b], rSo[b * n:b * n + n - 1])
    assert torch.equal(dpm.reshape(B * p, d), rpm) and torch.equal(dpv.reshape(B * p, d, d), rpv)
    # a shared [p] target row is the same as its B copies
    spm, spv = predict.predictive_posterior_batch(m, tsd - tsd[:, :1], xsd, tqd[0] - tsd[0, 0], observed=mkd, noise_var=sd_)
    cpm, cpv = predict.predictive_posterior_batch(m, tsd - tsd[:, :1], xsd, (tqd[0] - tsd[0, 0]).expand(B, -1).contiguous(),
                                                  observed=mkd, noise_var=sd_)
    assert torch.equal(spm, cpm) and torch.equal(spv, cpv)


@pytest.mark.gpu
def test_a_failing_series_is_named_with_its_local_row():
    d, obs = 3, 1
    m, _ = _model(d, obs, 8, F64, "cuda")
    lengths = [9, 17, 12, 6]
    series = _series(obs, lengths, 80)
    ts, xs, _, _ = _ragged(series, F64)
    start = sum(lengths[:2])
    ts[start + 5] = ts[start + 4]                                # a repeated time stamp in series 2
    assert leg.cr.CHECK_POSITIVE_DEFINITE
    for call in (lambda: leg.insample_posterior_batch(m, ts, xs, lengths=lengths),
                 lambda: predict.make_predictions_batch(m, ts, xs, ts[:3] + 0.01, lengths=lengths, target_lengths=[3, 0, 0, 0])):
        with pytest.raises(leg.cr.NotPSDError) as e:
            call()
        hit = re.search(r"series (\d+).*row (\d+)", str(e.value))
        assert hit and int(hit.group(1)) == 2 and int(hit.group(2)) in (4, 5), str(e.value)


@pytest.mark.gpu
def test_a_series_whose_factor_fails_is_named_with_its_local_row():
    """The time stamps are fine, so the assembly reports nothing; a large negative noise variance at one row makes that
    row's diagonal block of K negative definite, and the factorisation's failing row is mapped to (series, local row)."""
    d, obs = 3, 1
    m, _ = _model(d, obs, 8, F64, "cuda")
    lengths = [9, 17, 12, 6]
    series = _series(obs, lengths, 83)
    ts, xs, _, s = _ragged(series, F64)
    llt = float(m.LLT[0, 0])
    b, r = 2, 7
    row = sum(lengths[:b]) + r
    bnorm = float((m.B ** 2).sum())
    s[row] = -llt - bnorm / 1e6                                  # Li = -1e6 / |B|^2: the block gets -1e6 in the direction of B
    with pytest.raises(leg.cr.NotPSDError) as e:
        leg.insample_posterior_batch(m, ts, xs, lengths=lengths, noise_var=s)
    hit = re.search(r"series (\d+).*row (\d+)", str(e.value))
    # (the factor's info word names a row NEAR the failing block, include/cgps.h: the series must be the right one and
    # the row one of its own)
    assert hit and int(hit.group(1)) == b and 0 <= int(hit.group(2)) < lengths[b], str(e.value)


@pytest.mark.gpu
def test_batched_predictions_replayed_from_a_hip_graph():
    """One ordinary call (it builds the two plans), then leg.Graphed(..., check_sorted=False): replayed twice with new xs
    copied into the captured input, the results are the eager call's.  The captured graph is a single chain of nodes
    (hipGraphGetNodes / hipGraphGetEdges on the kept graph: edges = nodes - 1, no node with two successors or two
    predecessors)."""
    d, obs = 5, 1
    m, _ = _model(d, obs, 15, F64, "cuda")
    series, tts, ts, xs, mask, s, tt, tlens = _standard_prediction_inputs(d, obs, F64, 81)
    kw = dict(lengths=LENGTHS, target_lengths=tlens, observed=mask, noise_var=s)
    predict.make_predictions_batch(m, ts, xs, tt, **kw)
    gp = leg.Graphed(predict.make_predictions_batch, m, ts, xs, tt, check_sorted=False, **kw)
    gen = torch.Generator().manual_seed(3)
    for _ in range(2):
        xs.copy_(torch.randn(xs.shape, generator=gen, dtype=F64))
        pm, pv = gp()
        em, ev = predict.make_predictions_batch(m, ts, xs, tt, **kw)
        assert torch.equal(pm, em) and torch.equal(pv, ev)
    # the same capture with the graph kept for inspection: a single chain of launches, no parallel branches
    import ctypes
    prev = leg.cr.CHECK_POSITIVE_DEFINITE
    leg.cr.CHECK_POSITIVE_DEFINITE = False
    try:
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(g):
            predict.make_predictions_batch(m, ts, xs, tt, check_sorted=False, **kw)
    finally:
        leg.cr.CHECK_POSITIVE_DEFINITE = prev
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    raw = ctypes.c_void_p(int(g.raw_cuda_graph()))
    nn, ne = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(raw, None, ctypes.byref(nn)) == 0
    assert hip.hipGraphGetEdges(raw, None, None, ctypes.byref(ne)) == 0
    src, dst = (ctypes.c_void_p * ne.value)(), (ctypes.c_void_p * ne.value)()
    assert hip.hipGraphGetEdges(raw, src, dst, ctypes.byref(ne)) == 0
    print("captured graph: %d nodes, %d edges" % (nn.value, ne.value))
    assert nn.value >= 10                                        # assembly, factor, inverse, intercast and the torch glue
    assert ne.value == nn.value - 1                              # a tree ...
    assert len(set(src)) == ne.value and len(set(dst)) == ne.value      # ... whose nodes have one successor and one predecessor

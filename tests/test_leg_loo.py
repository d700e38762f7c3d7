"""Leave-one-out predictives (leg.loo_predictive, leg.loo_predictive_batch, leg.loo_predictive_models: DESIGN.md 4.20)
against a dense fp64 truth by deletion (_looref), against the definition inside the library (refits with one entry
masked), and the row kernel alone (leg._loo_rows) for precision and indexing.  Validation, the empty batch and the check
of the truth against the precision identity run without a GPU.

Tolerances.  An evaluation from the posterior loses kappa = Li[c, c] var_loo per entry (for a whole row: the largest
eigenvalue of Li[o, o] cov_loo) and carries cond(W_i) of the row's noise block; both come from _looref, and every case
asserts that its inputs keep them <= 64.  End to end the posterior holds 1e-7 / 1e-9 against the same dense truths
(tests/test_leg_posterior_batch.py), so the predictives hold that times kappa."""
import functools
import math
import re

import pytest
import torch

import _looref
import _noiseref as nr
from cyclic_gps import leg
from test_leg_posterior_batch import MODES, _model, _mode_args, _ragged, _series

cr = leg.cr
F64, F32 = torch.float64, torch.float32
EPS = {F64: float(torch.finfo(F64).eps), F32: float(torch.finfo(F32).eps)}
LEAVES = ["entry", "row"]
LENGTHS = [1, 2, 3, 65, 7]
KEYS = ("mean", "var", "logpdf")


# ---- cases -----------------------------------------------------------------------------------------------------------
def _loo_series(obs, lengths, seed):
    """test_leg_posterior_batch._series (masks with wholly unobserved rows) with the first row of every series fully
    observed, so that every series has leave-one-out terms."""
    out = _series(obs, lengths, seed)
    for _, _, mask, _ in out:
        mask[0] = True
    return out


def _truth_args(sr, mode):
    ts, xs, mask, s = sr
    return ts, xs, (s if mode in ("noise", "both") else None), (mask if mode in ("observed", "both") else None)


@functools.lru_cache(maxsize=None)
def _case(d, obs, lengths, seed, mode):
    """(model matrices, series, {leave: [truth of every series]}), computed once and shared by the tests."""
    _, mats = _model(d, obs, seed)
    series = _loo_series(obs, list(lengths), seed + 1)
    truth = {lv: [_looref.loo_truth(mats, *_truth_args(sr, mode), leave=lv) for sr in series] for lv in LEAVES}
    return mats, series, truth


def _conditioning(truths):
    """The largest kappa of the case; asserts the condition on the inputs (kappa <= 64, cond(W) <= 64)."""
    kappa = max(float(t["kappa"].max()) for t in truths)
    cond = max(float(t["cond_w"].max()) for t in truths)
    assert kappa <= 64 and cond <= 64, "badly conditioned inputs: kappa %.1f cond(W) %.1f (pick another seed)" % (kappa, cond)
    return max(kappa, 1.0)


def _cat(truths, key):
    return torch.cat([t[key] for t in truths])


def _cuda_model(mats, dtype=F64):
    return leg.LEGMatrices(*(t.to(dtype).cuda() for t in mats))


def _inputs(series, mode, dtype):
    """(ts, xs, observed, noise_var) of the ragged batch on the GPU; xs and noise_var hold NaN where nothing is observed."""
    ts, xs, mask, s = _ragged(series, dtype)
    ob, nv = _mode_args(mode, mask, s)
    if ob is not None:
        xs = torch.where(ob, xs, torch.full_like(xs, float("nan")))
        if nv is not None:
            nv = torch.where(ob, nv, torch.full_like(nv, float("nan")))
    return ts, xs, ob, nv


def _assert_unobserved(out, truth_mean, leave):
    """Unobserved entries: NaN / NaN / 0, exactly (the truth marks them with NaN in its mean)."""
    un = torch.isnan(truth_mean)
    mean, var, lp = (t.cpu() for t in out[:3])
    assert torch.equal(torch.isnan(mean), un)
    if leave == "entry":
        assert torch.equal(torch.isnan(var), un) and bool((lp[un] == 0).all())
    else:
        assert torch.equal(torch.isnan(var), un.unsqueeze(-1) | un.unsqueeze(-2))
        assert bool((lp[un.all(-1)] == 0).all())


def _assert_close(out, truths, leave, rtol, atol, what):
    for key, got in zip(KEYS, out[:3]):
        want = _cat(truths, key)
        got = got.cpu().to(F64).reshape(want.shape)
        ok = ~torch.isnan(want)
        err = ((got - want).abs() - rtol * want.abs())[ok]
        print("%s %s %s: max |err| %.3e (rtol %.1e atol %.1e)"
              % (what, leave, key, float((got - want).abs()[ok].max()), rtol, atol))
        assert bool((err <= atol).all()), (what, leave, key, float(err.max()), atol)


# ---- the precision identity in torch (any dtype, any device) -------------------------------------------------------------
def _identity(Bm, LLT, xs, mask, s, mu, Sd, leave):
    """The formulas of DESIGN 4.20 as torch passes: Bm [obs, d], LLT [obs, obs], xs [n, obs], mask bool [n, obs] or
    None, s [n, obs] or None, (mu [n, d], Sd [n, d, d]) the posterior.  Returns (mean, var, logpdf, score)."""
    dt = mu.dtype
    n, obs = xs.shape
    mask = torch.ones(n, obs, dtype=torch.bool, device=xs.device) if mask is None else mask
    zero = torch.zeros((), dtype=dt, device=xs.device)
    Mt = mask.to(dt)
    sz = zero.expand(n, obs) if s is None else torch.where(mask, s, zero)
    unobs = torch.diag_embed(1 - Mt)
    W = Mt.unsqueeze(2) * (LLT + torch.diag_embed(sz)) * Mt.unsqueeze(1) + unobs
    Li = torch.linalg.inv(W) - unobs
    xz = torch.where(mask, xs, zero)
    e = Mt * (xz - mu @ Bm.T)
    g = (Li @ e.unsqueeze(-1)).squeeze(-1)
    P = Li - Li @ (Bm @ Sd @ Bm.T) @ Li
    nan = torch.full((), float("nan"), dtype=dt, device=xs.device)
    if leave == "entry":
        pcc = torch.where(mask, torch.diagonal(P, dim1=-2, dim2=-1), 1 + zero)
        mean = torch.where(mask, xz - g / pcc, nan)
        var = torch.where(mask, 1 / pcc, nan)
        lp = torch.where(mask, -0.5 * g * g / pcc + 0.5 * torch.log(pcc) - 0.5 * math.log(2 * math.pi), zero)
    else:
        Pm = Mt.unsqueeze(2) * P * Mt.unsqueeze(1) + unobs
        cov = torch.linalg.inv(Pm)
        cg = (cov @ g.unsqueeze(-1)).squeeze(-1)
        mean = torch.where(mask, xz - cg, nan)
        var = torch.where(mask.unsqueeze(2) & mask.unsqueeze(1), cov, nan)
        lp = -0.5 * (g * cg).sum(-1) + 0.5 * torch.logdet(Pm) - 0.5 * Mt.sum(-1) * math.log(2 * math.pi)
    return mean, var, lp, lp.to(F64).sum()


# ---- without a GPU -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,obs,n", [(3, 2, 7), (5, 1, 12), (5, 3, 9), (8, 3, 6)])
@pytest.mark.parametrize("leave", LEAVES)
def test_the_truth_by_deletion_agrees_with_the_precision_identity(d, obs, n, leave):
    (Nm, Rm, Bm, Lm, xs, ts, s), mask = nr.leg_case(d, obs, n, 40 + d + obs)
    truth = _looref.loo_truth((Nm, Rm, Bm, Lm), ts, xs, s, mask, leave)
    mu, cov = nr.leg_dense_posterior(Nm, Rm, Bm, Lm, ts, torch.where(mask, xs, torch.zeros_like(xs)), s, mask)
    i = torch.arange(n)
    LLT = Lm @ Lm.T + 1e-9 * torch.eye(obs, dtype=F64)
    out = _identity(Bm, LLT, xs, mask, s, mu, cov[i, :, i, :], leave)
    for key, got in zip(KEYS + ("score",), out):
        want = truth[key]
        ok = ~torch.isnan(want)
        assert torch.equal(torch.isnan(got), ~ok), key
        rel = ((got - want).abs() / (1 + want.abs()))[ok]
        assert float(rel.max()) <= 1e-11, (key, float(rel.max()))
    assert float(truth["kappa"].max()) >= 1 and float(truth["cond_w"].min()) >= 1


def _cpu_case(B=3, n=4, obs=2, d=3):
    m, _ = _model(d, obs, 5)
    ts = torch.cumsum(torch.ones(B, n, dtype=F64), 1)
    return m, ts, torch.zeros(B, n, obs, dtype=F64)


def test_validation_errors_come_before_anything_runs():
    m, ts, xs = _cpu_case()
    B, n, obs = xs.shape
    tsr, xsr, lens = ts.reshape(-1), xs.reshape(B * n, obs), [n] * B
    ms = [m, _model(3, obs, 6)[0]]
    one, bat = leg.loo_predictive, leg.loo_predictive_batch
    mod = lambda *a, **k: leg.loo_predictive_models(ms, *a, **k)      # noqa: E731
    m9, _ = _model(3, 9, 7)
    ts9, xs9 = ts[0], torch.zeros(n, 9, dtype=F64)
    bad = [
        # wrong layouts
        lambda: one(m, ts, xs),
        lambda: one(m, ts[0], xs[0, :3]),
        lambda: bat(m, ts, xsr),
        lambda: bat(m, ts[:, :3], xs),
        lambda: bat(m, ts, xsr, lengths=lens),
        lambda: mod(ts, xsr),
        lambda: mod(ts, xsr, lengths=lens),
        lambda: leg.loo_predictive_models([], ts, xs),
        # wrong channel count
        lambda: one(m, ts[0], xs[0, :, :1]),
        lambda: bat(m, ts, xs[..., :1]),
        lambda: mod(ts, xs[..., :1]),
        # bad leave
        lambda: one(m, ts[0], xs[0], leave="column"),
        lambda: bat(m, ts, xs, leave="rows"),
        lambda: mod(ts, xs, leave=0),
        # bad lengths
        lambda: bat(m, tsr, xsr, lengths=[n] * (B - 1)),
        lambda: bat(m, tsr, xsr, lengths=[n, n, n - 1, 1, 0]),
        lambda: bat(m, tsr, xsr, lengths=torch.tensor([4.0, 4.0, 4.0])),
        lambda: mod(tsr, xsr, lengths=[n] * (B - 1)),
        lambda: mod(tsr, xsr, lengths=[n, n, n - 1, 1, 0]),
        # masks and variances of the wrong kind or shape
        lambda: one(m, ts[0], xs[0], observed=torch.ones(n, obs)),
        lambda: one(m, ts[0], xs[0], observed=torch.ones(n + 1, dtype=torch.bool)),
        lambda: one(m, ts[0], xs[0], noise_var=torch.ones(n, obs + 1, dtype=F64)),
        lambda: one(m, ts[0], xs[0], noise_var=torch.ones(n, obs, dtype=torch.int64)),
        lambda: bat(m, ts, xs, observed=torch.ones(B, n, obs)),
        lambda: bat(m, ts, xs, observed=torch.ones(B, n + 1, dtype=torch.bool)),
        lambda: bat(m, ts, xs, noise_var=torch.ones(B, n, obs + 1, dtype=F64)),
        lambda: mod(ts, xs, observed=torch.ones(B, n, obs)),
        lambda: mod(ts, xs, noise_var=torch.ones(B, n, obs, dtype=torch.int64)),
        # obs_dim > 8 with a mask
        lambda: one(m9, ts9, xs9, observed=torch.ones(n, 9, dtype=torch.bool)),
        lambda: bat(m9, ts9.unsqueeze(0), xs9.unsqueeze(0), observed=torch.ones(1, n, 9, dtype=torch.bool)),
        lambda: leg.loo_predictive_models([m9], ts9.unsqueeze(0), xs9.unsqueeze(0),
                                          observed=torch.ones(1, n, 9, dtype=torch.bool)),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d raised nothing" % k)


@pytest.mark.parametrize("leave", LEAVES)
def test_empty_batches_give_empty_results(leave):
    m, ts, xs = _cpu_case()
    d, obs, n, M = 3, 2, 4, 2
    row = leave == "row"
    tail_var, tail_lp = ((obs, obs), ()) if row else ((obs,), (obs,))
    r = leg.loo_predictive_batch(m, ts[:0], xs[:0], leave=leave)
    assert r.mean.shape == (0, n, obs) and r.var.shape == (0, n) + tail_var and r.logpdf.shape == (0, n) + tail_lp
    assert r.score.shape == (0,) and r.score.dtype == F64 and r.mean.dtype == F64
    r = leg.loo_predictive_batch(m, ts.reshape(-1)[:0], xs.reshape(-1, obs)[:0], lengths=[], leave=leave)
    assert r.mean.shape == (0, obs) and r.var.shape == (0,) + tail_var and r.logpdf.shape == (0,) + tail_lp
    assert r.score.shape == (0,)
    ms = [m, _model(d, obs, 6)[0]]
    r = leg.loo_predictive_models(ms, ts[:0], xs[:0], leave=leave)
    assert r.mean.shape == (M, 0, n, obs) and r.var.shape == (M, 0, n) + tail_var and r.logpdf.shape == (M, 0, n) + tail_lp
    assert r.score.shape == (M, 0) and r.score.dtype == F64
    r = leg.loo_predictive_models(ms, ts.reshape(-1)[:0], xs.reshape(-1, obs)[:0], lengths=[], leave=leave)
    assert r.mean.shape == (M, 0, obs) and r.var.shape == (M, 0) + tail_var and r.logpdf.shape == (M, 0) + tail_lp
    r = leg.loo_predictive(m, ts[0, :0], xs[0, :0], leave=leave)
    assert r.mean.shape == (0, obs) and r.var.shape == (0,) + tail_var and r.logpdf.shape == (0,) + tail_lp
    assert r.score.shape == () and float(r.score) == 0.0
    assert isinstance(r, leg.LooPredictive)


# ---- on the GPU ----------------------------------------------------------------------------------------------------------
# seeds whose cases meet the condition on the inputs (kappa <= 64, cond(W) <= 64; _conditioning), found on the CPU
SEED = {(1, 1): 11, (1, 2): 12, (1, 3): 13, (1, 8): 18, (5, 1): 51, (5, 2): 52, (5, 3): 53, (5, 8): 155,
        (8, 1): 81, (8, 2): 82, (8, 3): 180, (8, 8): 88}


def _score_check(score, truths, rtol, atol, what):
    for b, t in enumerate(truths):
        terms = max(int((t["logpdf"] != 0).sum()), 1)
        want = float(t["score"])
        assert abs(float(score[b]) - want) <= terms * (rtol * abs(want) + atol), (what, b, float(score[b]), want)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("obs", [1, 2, 3, 8])
@pytest.mark.parametrize("d", [1, 5, 8])
def test_against_the_truth_by_deletion_fp64(d, obs, mode):
    """loo_predictive_batch, ragged and dense, and loo_predictive against _looref: rtol 1e-7 kappa, atol 1e-9 kappa."""
    mats, series, truth = _case(d, obs, tuple(LENGTHS), SEED[d, obs], mode)
    dmats, dseries, dtruth = _case(d, obs, (7, 7, 7), SEED[d, obs] + 100, mode)         # (a model of its own)
    m = _cuda_model(mats)
    for leave in LEAVES:
        kappa = _conditioning(truth[leave] + dtruth[leave])
        rtol, atol = 1e-7 * kappa, 1e-9 * kappa
        ts, xs, ob, nv = _inputs(series, mode, F64)
        out = leg.loo_predictive_batch(m, ts, xs, lengths=LENGTHS, observed=ob, noise_var=nv, leave=leave)
        assert out.score.dtype == F64 and out.score.shape == (len(LENGTHS),)
        _assert_unobserved(out, _cat(truth[leave], "mean"), leave)
        _assert_close(out, truth[leave], leave, rtol, atol, "ragged")
        _score_check(out.score, truth[leave], rtol, atol, "ragged")
        # dense: three series of seven rows
        ts, xs, ob, nv = _inputs(dseries, mode, F64)
        v3 = lambda t: None if t is None else t.reshape((3, 7) + tuple(t.shape[1:]))      # noqa: E731
        dense = leg.loo_predictive_batch(_cuda_model(dmats), v3(ts), v3(xs), observed=v3(ob), noise_var=v3(nv), leave=leave)
        assert dense.mean.shape == (3, 7, obs) and dense.logpdf.shape == ((3, 7) if leave == "row" else (3, 7, obs))
        assert dense.var.shape == ((3, 7, obs, obs) if leave == "row" else (3, 7, obs))
        flat = [t.reshape((21,) + tuple(t.shape[2:])) for t in dense[:3]]
        _assert_unobserved(flat, _cat(dtruth[leave], "mean"), leave)
        _assert_close(flat, dtruth[leave], leave, rtol, atol, "dense")
        _score_check(dense.score, dtruth[leave], rtol, atol, "dense")
        # one series: the last of the ragged batch
        ts1, xs1, ob1, nv1 = _inputs(series[4:], mode, F64)
        single = leg.loo_predictive(m, ts1, xs1, observed=ob1, noise_var=nv1, leave=leave)
        assert single.score.dim() == 0
        _assert_unobserved(single, truth[leave][4]["mean"], leave)
        _assert_close(single, truth[leave][4:], leave, rtol, atol, "single")
        _score_check(single.score.reshape(1), truth[leave][4:], rtol, atol, "single")


@pytest.mark.gpu
@pytest.mark.parametrize("leave", LEAVES)
def test_a_batch_of_300_rows_crosses_a_workgroup(leave):
    lengths = (130, 170)
    mats, series, truth = _case(5, 1, lengths, 57, "both")
    kappa = _conditioning(truth[leave])
    ts, xs, ob, nv = _inputs(series, "both", F64)
    out = leg.loo_predictive_batch(_cuda_model(mats), ts, xs, lengths=list(lengths), observed=ob, noise_var=nv, leave=leave)
    _assert_unobserved(out, _cat(truth[leave], "mean"), leave)
    _assert_close(out, truth[leave], leave, 1e-7 * kappa, 1e-9 * kappa, "R = 300")
    _score_check(out.score, truth[leave], 1e-7 * kappa, 1e-9 * kappa, "R = 300")


@pytest.mark.gpu
def test_against_refits_with_one_entry_masked():
    """The definition, inside the library: for every observed entry (i, c), the posterior given everything else
    (insample_posterior with that entry masked) gives the latent of row i as N(mu, S).  x_ic = b_c z_i + e_c, and e_c is
    correlated with the noise e_c' of the row's other channel when that one is observed (obs_dim 2): with
    rho = Cn[c, c'] / Cn[c', c'] and a = b_c - rho b_c', x_ic | rest = N(a mu + rho x_ic', a S a^T + Cn[c, c] - rho Cn[c, c']);
    with c' unobserved rho = 0."""
    d, obs, n = 3, 2, 6
    mats, series, truth = _case(d, obs, (n,), 32, "both")
    kappa = _conditioning(truth["entry"])
    m = _cuda_model(mats)
    ts, xs, mask, s = (t.cuda() for t in series[0])
    out = leg.loo_predictive(m, ts, xs, observed=mask, noise_var=s)
    LLT = m.LLT
    checked = 0
    for i in range(n):
        for c in range(obs):
            if not bool(mask[i, c]):
                continue
            left = mask.clone()
            left[i, c] = False
            mu, (Sd, _) = leg.insample_posterior(m, ts, xs, observed=left, noise_var=s)
            Cn = LLT + torch.diag(s[i])
            o = 1 - c
            rho = Cn[c, o] / Cn[o, o] if bool(mask[i, o]) else torch.zeros((), dtype=F64, device="cuda")
            a = m.B[c] - rho * m.B[o]
            mean = a @ mu[i] + (rho * xs[i, o] if bool(mask[i, o]) else 0.0)
            var = a @ Sd[i] @ a + Cn[c, c] - rho * Cn[c, o]
            lp = -0.5 * (xs[i, c] - mean) ** 2 / var - 0.5 * torch.log(var) - 0.5 * math.log(2 * math.pi)
            for got, want in ((out.mean[i, c], mean), (out.var[i, c], var), (out.logpdf[i, c], lp)):
                err = abs(float(got) - float(want))
                assert err <= 1e-7 * kappa * abs(float(want)) + 1e-9 * kappa, (i, c, float(got), float(want))
            checked += 1
    assert checked >= 4


def _truth_posterior(mats, sr, mode):
    """The fp64 dense posterior rows (mean [n, d], Sd [n, d, d]) of one series."""
    ts, xs, s, mask = _truth_args(sr, mode)
    n, obs = xs.shape
    mask = torch.ones(n, obs, dtype=torch.bool) if mask is None else mask
    s = torch.zeros(n, obs, dtype=F64) if s is None else s
    mu, cov = nr.leg_dense_posterior(*mats, ts, torch.where(mask, xs, torch.zeros_like(xs)), s, mask)
    i = torch.arange(n)
    return mu, cov[i, :, i, :]


def _rows_call(mats_list, sr, mode, mu, Sd, dtype, leave, offsets=None):
    """leg._loo_rows on given posterior rows (mu [M n, d], Sd [M n, d, d]) of one data set under M models."""
    _, xs, s, mask = _truth_args(sr, mode)
    n = xs.shape[0]
    xs_c, pattern, nv = leg._loo_data(xs.cuda(), None if mask is None else mask.cuda(), None if s is None else s.cuda(), dtype)
    Bm = torch.stack([mats[2] for mats in mats_list]).to(dtype).cuda().contiguous()
    LLT = torch.stack([mats[3] @ mats[3].T + 1e-9 * torch.eye(xs.shape[1], dtype=F64) for mats in mats_list]).to(dtype).cuda()
    if offsets is None:
        offsets = torch.tensor([0, n], dtype=torch.int64, device="cuda")
    return leg._loo_rows(xs_c, pattern, nv, offsets, Bm, LLT.contiguous(), mu.to(dtype).cuda().contiguous(),
                         Sd.to(dtype).cuda().contiguous(), leg._LEAVE[leave])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("obs", [1, 2, 3, 8])
@pytest.mark.parametrize("d", [1, 5, 8])
def test_the_row_kernel_alone_in_both_precisions(d, obs, dtype):
    """cgps_leg_loo on posterior rows taken from the dense fp64 truth and cast to the dtype, against the truth: per entry
    256 eps kappa cond(W), relative to 1 + |value| (a chain of about 64 rounded operations for d, obs <= 8, times 4)."""
    mats, series, truth = _case(d, obs, (9,), SEED[d, obs] + 200, "both")
    sr = series[0]
    mu, Sd = _truth_posterior(mats, sr, "both")
    for leave in LEAVES:
        t = truth[leave][0]
        _conditioning([t])
        out = _rows_call([mats], sr, "both", mu, Sd, dtype, leave)
        assert int(out[4].item()) == 0
        amp = t["kappa"] * (t["cond_w"].unsqueeze(-1) if leave == "entry" else t["cond_w"])      # per entry / per row
        bounds = {"mean": amp if leave == "entry" else amp.unsqueeze(-1), "logpdf": amp,
                  "var": amp if leave == "entry" else amp.reshape(-1, 1, 1)}
        worst = 0.0
        for key, got in zip(KEYS, out[:3]):
            want = t[key]
            got = got[0].cpu().to(F64)
            ok = ~torch.isnan(want)
            assert torch.equal(torch.isnan(got), ~ok)
            ratio = ((got - want).abs() / (1 + want.abs()) / (EPS[dtype] * bounds[key].clamp(min=1).expand_as(want)))[ok]
            worst = max(worst, float(ratio.max()))
            assert float(ratio.max()) <= 256, (leave, key, float(ratio.max()))
        print("row kernel d %d obs %d %s %s: worst error %.1f eps kappa cond(W)" % (d, obs, dtype, leave, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("leave", LEAVES)
def test_indexing_rows_models_and_series_bit_for_bit(leave):
    d, obs, lengths = 5, 3, [130, 170]
    R = sum(lengths)
    models = [_model(d, obs, 60 + k)[1] for k in range(3)]
    series = _loo_series(obs, lengths, 61)
    ts, xs, mask, s = (torch.cat([sr[k] for sr in series]) for k in range(4))
    whole = (ts, xs, mask, s)
    post = []
    for mats in models:
        mu, (Sd, _) = leg.insample_posterior_batch(_cuda_model(mats), ts.cuda(), xs.cuda(), lengths=lengths,
                                                   observed=mask.cuda(), noise_var=s.cuda())
        post.append((mu.cpu(), Sd.cpu()))
    one = torch.tensor([0, R], dtype=torch.int64, device="cuda")
    # rows: a permutation of the rows, given as one series, permutes the row outputs
    base = _rows_call(models[:1], whole, "both", *post[0], F64, leave, one)
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(3))
    shuffled = _rows_call(models[:1], tuple(t[perm] for t in whole), "both", post[0][0][perm], post[0][1][perm], F64, leave, one)
    for a, b in zip(base[:3], shuffled[:3]):
        assert torch.equal(torch.nan_to_num(a[0][perm.cuda()], nan=-7.0), torch.nan_to_num(b[0], nan=-7.0))
    # models: slice k of the call on three models is the call on model k
    off = torch.tensor([0, lengths[0], R], dtype=torch.int64, device="cuda")
    three = _rows_call(models, whole, "both", torch.cat([p[0] for p in post]), torch.cat([p[1] for p in post]), F64, leave, off)
    assert three[0].shape[0] == 3 and three[3].shape == (3, 2)
    for k in range(3):
        alone = _rows_call(models[k:k + 1], whole, "both", *post[k], F64, leave, off)
        for a, b in zip(three[:4], alone[:4]):
            assert torch.equal(torch.nan_to_num(a[k], nan=-7.0), torch.nan_to_num(b[0], nan=-7.0))
        assert not torch.equal(torch.nan_to_num(three[0][k]), torch.nan_to_num(three[0][(k + 1) % 3]))
    # series: the batch with its two series swapped gives the scores swapped
    swap = torch.cat([torch.arange(lengths[0], R), torch.arange(lengths[0])])
    off2 = torch.tensor([0, lengths[1], R], dtype=torch.int64, device="cuda")
    swapped = _rows_call(models[:1], tuple(t[swap] for t in whole), "both", post[0][0][swap], post[0][1][swap], F64, leave, off2)
    straight = _rows_call(models[:1], whole, "both", *post[0], F64, leave, off)
    assert torch.equal(swapped[3][0], straight[3][0].flip(0)) and bool(torch.isfinite(straight[3]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "both"])
@pytest.mark.parametrize("d,obs", [(5, 1), (5, 3), (8, 8)])
def test_fp32_end_to_end_is_as_accurate_as_the_formulas_in_torch(d, obs, mode):
    """The fp32 error of loo_predictive_batch against the truth is at most 4x that of the same formulas evaluated by
    torch in fp32 from the library's own per-series fp32 insample_posterior (floor 64 eps32 kappa), per output, max norm."""
    mats, series, truth = _case(d, obs, tuple(LENGTHS), SEED[d, obs], mode)
    m = _cuda_model(mats, F32)
    Bm, LLT = m.B.cpu(), m.LLT.cpu()
    for leave in LEAVES:
        kappa = _conditioning(truth[leave])
        ts, xs, ob, nv = _inputs(series, mode, F32)
        out = leg.loo_predictive_batch(m, ts, xs, lengths=LENGTHS, observed=ob, noise_var=nv, leave=leave)
        ref = []
        for sr in series:
            t1, x1, o1, n1 = _inputs([sr], mode, F32)
            mu, (Sd, _) = leg.insample_posterior(m, t1, x1, observed=o1, noise_var=n1)
            c = lambda t: None if t is None else t.cpu()      # noqa: E731
            ref.append(_identity(Bm, LLT, c(x1), c(o1), c(n1), mu.cpu(), Sd.cpu(), leave))
        for j, key in enumerate(KEYS):
            want = _cat(truth[leave], key)
            ok = ~torch.isnan(want)
            scale = 1 + want.abs()
            e_lib = float(((out[j].cpu().to(F64).reshape(want.shape) - want).abs() / scale)[ok].max())
            e_ref = float(((torch.cat([r[j] for r in ref]).to(F64).reshape(want.shape) - want).abs() / scale)[ok].max())
            print("fp32 d %d obs %d %s %s %s: library %.3e torch %.3e ratio %.2f" % (d, obs, mode, leave, key, e_lib, e_ref,
                                                                                      e_lib / max(e_ref, 1e-300)))
            assert e_lib <= max(4 * e_ref, 64 * EPS[F32] * kappa), (leave, key, e_lib, e_ref)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dense", [False, True])
def test_models_against_one_batched_call_per_model(mode, dense, monkeypatch):
    d, obs, M = 3, 2, 3
    lengths = [5, 5, 5, 5] if dense else [3, 6, 2, 5]
    models = [_model(d, obs, 70 + k)[1] for k in range(M)]
    ms = [_cuda_model(mats) for mats in models]
    series = _loo_series(obs, lengths, 71)
    ts, xs, ob, nv = _inputs(series, mode, F64)
    if dense:
        v = lambda t: None if t is None else t.reshape((4, 5) + tuple(t.shape[1:]))      # noqa: E731
        args, kw = (v(ts), v(xs)), dict(observed=v(ob), noise_var=v(nv))
    else:
        args, kw = (ts, xs), dict(lengths=lengths, observed=ob, noise_var=nv)
    for leave in LEAVES:
        kappa = max(_conditioning([_looref.loo_truth(mats, *_truth_args(sr, mode), leave=leave) for sr in series])
                    for mats in models)
        each = [leg.loo_predictive_batch(m, *args, leave=leave, **kw) for m in ms]
        runs = [leg.loo_predictive_models(ms, *args, leave=leave, **kw)]
        if mode == "both":                                      # the chunk loop: one model per chunk
            monkeypatch.setattr(leg, "MODELS_POSTERIOR_MAX_ROWS", sum(lengths))
            runs.append(leg.loo_predictive_models(ms, *args, leave=leave, **kw))
            monkeypatch.undo()
        for out in runs:
            assert out.score.shape == (M, 4) and out.mean.shape == (M,) + tuple(each[0].mean.shape)
            for k in range(M):
                for a, b in zip(out, each[k]):
                    assert a[k].shape == b.shape
                    assert torch.equal(torch.isnan(a[k]), torch.isnan(b))
                    torch.testing.assert_close(torch.nan_to_num(a[k]), torch.nan_to_num(b), rtol=1e-9 * kappa, atol=1e-11 * kappa)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 5, 8])
def test_row_and_entry_coincide_for_one_channel(d):
    mats, series, truth = _case(d, 1, tuple(LENGTHS), SEED[d, 1], "both")
    kappa = _conditioning(truth["entry"])
    ts, xs, ob, nv = _inputs(series, "both", F64)
    m = _cuda_model(mats)
    e = leg.loo_predictive_batch(m, ts, xs, lengths=LENGTHS, observed=ob, noise_var=nv, leave="entry")
    r = leg.loo_predictive_batch(m, ts, xs, lengths=LENGTHS, observed=ob, noise_var=nv, leave="row")
    assert r.var.shape == e.var.shape + (1,) and r.logpdf.shape == e.logpdf.shape[:1]
    # (a series' score adds up to max(LENGTHS) terms, each within the bound)
    for a, b, terms in ((e.mean, r.mean, 1), (e.var, r.var.squeeze(-1), 1), (e.logpdf.squeeze(-1), r.logpdf, 1),
                        (e.score, r.score, max(LENGTHS))):
        assert torch.equal(torch.isnan(a), torch.isnan(b))
        a, b = torch.nan_to_num(a), torch.nan_to_num(b)
        assert bool(((a - b).abs() <= terms * 4 * EPS[F64] * kappa * (1 + b.abs())).all())


@pytest.mark.gpu
def test_a_failing_row_is_named_with_its_model_and_series():
    """A negative noise variance that makes W of one row of series 2 indefinite under model 1 (LLT = 0.36) and not under
    models 0 and 2 (LLT = 3600): an arithmetic failure, reported through the info word."""
    d, obs, lengths = 3, 1, [4, 6, 5]
    ms = []
    for k, lam in enumerate((60.0, 0.6, 60.0)):
        m, _ = _model(d, obs, 90 + k, F64, "cuda")
        ms.append(leg.LEGMatrices(m.N, m.R, m.B, torch.full((1, 1), lam, dtype=F64, device="cuda")))
    series = _loo_series(obs, lengths, 91)
    ts, xs, _, s = _ragged(series, F64)
    row = sum(lengths[:2]) + 3
    s[row] = -1000.0                                             # W = 0.36 - 1000 < 0 < 3600 - 1000; Li = -1e-3 leaves K positive
    assert cr.CHECK_POSITIVE_DEFINITE
    with pytest.raises(cr.NotPSDError) as e:
        leg.loo_predictive_batch(ms[1], ts, xs, lengths=lengths, noise_var=s)
    hit = re.search(r"series (\d+).*row (\d+)", str(e.value))
    assert hit and int(hit.group(1)) == 2 and int(hit.group(2)) == 3, str(e.value)
    for leave in LEAVES:
        with pytest.raises(cr.NotPSDError) as e:
            leg.loo_predictive_models(ms, ts, xs, lengths=lengths, noise_var=s, leave=leave)
        hit = re.search(r"model (\d+).*series (\d+).*row (\d+)", str(e.value))
        assert hit and (int(hit.group(1)), int(hit.group(2)), int(hit.group(3))) == (1, 2, 3), str(e.value)
    cr.CHECK_POSITIVE_DEFINITE = False
    try:
        out = leg.loo_predictive_models(ms, ts, xs, lengths=lengths, noise_var=s)
    finally:
        cr.CHECK_POSITIVE_DEFINITE = True
    assert bool(torch.isnan(out.mean[1, row]).all()) and bool(torch.isnan(out.logpdf[1, row]).all())
    assert bool(torch.isnan(out.score[1, 2])) and bool(torch.isfinite(out.score[[0, 2]]).all())
    assert bool(torch.isfinite(out.score[1, :2]).all())

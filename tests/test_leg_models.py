"""leg.log_likelihood_models: M LEG models over the same batch of series in one call (cgps_leg_loglik_models for the
forward, cgps_peg_precision_models / cgps_peg_precision_adjoint_models for the backward) against the one-model entry
points bit for bit, against a loop of leg.log_likelihood_batch over the models, against the reference's recorded values
and gradients (tests/golden/leg_models.npz) and against a dense fp64 Gaussian that shares no code with the kernels
(_missref.leg_dense_value_and_grads with an all-True mask)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import _missref as mr
import _util
from cyclic_gps import _hip, leg
import cyclic_gps.cyclic_reduction as cr

F64, F32 = torch.float64, torch.float32


def _model(d, obs, dtype, seed, device="cuda"):
    """(the conditioning of test_leg_batch._model)"""
    gen = torch.Generator().manual_seed(seed)
    N = torch.tril(0.4 * torch.randn(d, d, generator=gen, dtype=F64)) + 0.8 * torch.eye(d, dtype=F64)
    R = torch.tril(0.3 * torch.randn(d, d, generator=gen, dtype=F64), -1)
    B = 0.7 * torch.randn(obs, d, generator=gen, dtype=F64)
    L = torch.tril(0.2 * torch.randn(obs, obs, generator=gen, dtype=F64)) + 0.6 * torch.eye(obs, dtype=F64)
    return leg.LEGMatrices(*(t.to(dtype).to(device) for t in (N, R, B, L)))


def _ragged(lengths, obs, gen, dtype, device="cuda", gap0=0.05):
    """Concatenated series, every one on a clock of its own, with irregular gaps."""
    ts, xs = [], []
    for n in lengths:
        t0 = 50.0 * torch.rand((), generator=gen, dtype=F64) - 25.0
        ts.append(t0 + torch.cumsum(gap0 + 0.5 * torch.rand(n, generator=gen, dtype=F64), 0))
        xs.append(torch.randn(n, obs, generator=gen, dtype=F64))
    return torch.cat(ts).to(dtype).to(device), torch.cat(xs).to(dtype).to(device)


# ---- argument handling and the C entries' checks (no GPU) ------------------------------------------------------------

def test_models_are_checked_before_anything_runs():
    ts, xs = torch.zeros(10, dtype=F64), torch.zeros(10, 1, dtype=F64)
    m = _model(2, 1, F64, 0, device="cpu")
    with pytest.raises(ValueError, match="at least one model"):
        leg.log_likelihood_models([], ts, xs, [4, 6])
    with pytest.raises(ValueError, match="model 1"):
        leg.log_likelihood_models([m, _model(3, 1, F64, 1, device="cpu")], ts, xs, [4, 6])          # rank
    with pytest.raises(ValueError, match="model 1"):
        leg.log_likelihood_models([m, _model(2, 2, F64, 1, device="cpu")], ts, xs, [4, 6])          # obs_dim
    with pytest.raises(ValueError, match="model 2"):
        leg.log_likelihood_models([m, m, _model(2, 1, F32, 1, device="cpu")], ts, xs, [4, 6])       # dtype
    with pytest.raises(ValueError, match="model 1"):
        leg.log_likelihood_models([m, "not a model"], ts, xs, [4, 6])
    with pytest.raises(ValueError, match="channels"):
        leg.log_likelihood_models([m, m], ts, torch.zeros(10, 2, dtype=F64), [4, 6])
    with pytest.raises(TypeError):
        leg.log_likelihood_models([m], ts, xs, [4, 6], observed=torch.ones(10, dtype=torch.bool))   # not an argument


def test_layout_is_checked_as_the_batch_checks_it():
    ts, xs = torch.zeros(10, dtype=F64), torch.zeros(10, 1, dtype=F64)
    ms = [_model(2, 1, F64, s, device="cpu") for s in (0, 1)]
    with pytest.raises(ValueError, match="sum"):
        leg.log_likelihood_models(ms, ts, xs, [4, 5])
    with pytest.raises(ValueError, match="length 0"):
        leg.log_likelihood_models(ms, ts, xs, [4, 0, 6])
    with pytest.raises(ValueError, match="host data"):
        leg.log_likelihood_models(ms, ts, xs, torch.tensor([4.0, 6.0]))
    with pytest.raises(ValueError, match="dense layout"):
        leg.log_likelihood_models(ms, ts, xs)
    with pytest.raises(ValueError, match="ragged layout"):
        leg.log_likelihood_models(ms, ts.reshape(2, 5), xs.reshape(2, 5, 1), [5, 5])


def test_a_wrong_channel_count_prints_the_shape_each_call_has_always_printed():
    """Dense xs [2, 5, 2] under models of one channel: the many-model calls name the flattened (10, 2), the batch calls the
    caller's (2, 5, 2)."""
    import re
    from cyclic_gps import predict
    ms = [_model(2, 1, F64, s, device="cpu") for s in (0, 1)]
    ts, xs = torch.arange(10, dtype=F64).reshape(2, 5), torch.zeros(2, 5, 2, dtype=F64)
    many = re.escape("xs must have 1 channels, got (10, 2)")
    for call in (lambda: leg.log_likelihood_models(ms, ts, xs), lambda: leg.insample_posterior_models(ms, ts, xs),
                 lambda: predict.predictive_posterior_models(ms, ts, xs, ts), lambda: leg.loo_predictive_models(ms, ts, xs),
                 lambda: leg.posterior_perturbation_models(ms, ts, xs, 2, 1)):
        with pytest.raises(ValueError, match=many):
            call()
    one = re.escape("xs must have 1 channels, got (2, 5, 2)")
    seen = torch.ones(2, 5, dtype=torch.bool)
    for call in (lambda: leg.log_likelihood_batch(ms[0], ts, xs, observed=seen), lambda: leg.insample_posterior_batch(ms[0], ts, xs),
                 lambda: predict.predictive_posterior_batch(ms[0], ts, xs, ts)):
        with pytest.raises(ValueError, match=one):
            call()


def test_empty_batch_gives_one_empty_row_per_model():
    ms = [_model(3, 1, F64, s, device="cpu") for s in (0, 1, 2)]
    out = leg.log_likelihood_models(ms, torch.zeros(0, dtype=F64), torch.zeros(0, 1, dtype=F64), [])
    assert out.shape == (3, 0) and out.dtype == F64
    out = leg.log_likelihood_models(ms, torch.zeros(0, 7, dtype=F64), torch.zeros(0, 7, 1, dtype=F64))
    assert out.shape == (3, 0)
    assert leg.MODELS_BACKWARD_MAX_ROWS == 1 << 22


def test_c_entries_reject_null_pointers_and_model_counts():
    lib = _hip.lib()
    fake = ctypes.c_void_p(256)
    # cgps_leg_loglik_models(ts, offsets, B, R, M, G, A, v, q, d, dtype, max_rows, out4, info2, stream)
    assert lib.cgps_leg_loglik_models(None, None, 2, 10, 3, None, None, None, None, 5, _hip.F64, 4096, None, None, None) == 1
    assert b"cgps_leg_loglik_models" in lib.cgps_last_error()
    for M in (0, -1, 65536):
        assert lib.cgps_leg_loglik_models(fake, fake, 2, 10, M, fake, fake, None, None, 5, _hip.F64, 4096, fake, fake, None) == 1
        assert b"outside 1..65535" in lib.cgps_last_error()
    assert lib.cgps_leg_loglik_models(fake, fake, -1, 10, 3, fake, fake, None, None, 5, _hip.F64, 4096, fake, fake, None) == 1
    assert lib.cgps_leg_loglik_models(fake, fake, 2, -1, 3, fake, fake, None, None, 5, _hip.F64, 4096, fake, fake, None) == 1
    # cgps_peg_precision_models(ts, G, cut, R, M, d, dtype, Rs, Os, info, stream)
    assert lib.cgps_peg_precision_models(None, None, None, 8, 2, 4, _hip.F64, None, None, None, None) == 1
    assert b"cgps_peg_precision_models" in lib.cgps_last_error()
    for M in (0, 65536):
        assert lib.cgps_peg_precision_models(fake, fake, fake, 8, M, 4, _hip.F64, fake, fake, fake, None) == 1
    assert lib.cgps_peg_precision_models(fake, fake, fake, 0, 2, 4, _hip.F64, fake, fake, fake, None) == 1
    # cgps_peg_precision_adjoint_models(ts, G, cut, R, M, d, dtype, gRs, gOs, gG_partial, gtau, stream)
    assert lib.cgps_peg_precision_adjoint_models(None, None, None, 8, 2, 4, _hip.F64, None, None, None, None, None) == 1
    assert b"cgps_peg_precision_adjoint_models" in lib.cgps_last_error()
    for M in (0, 65536):
        assert lib.cgps_peg_precision_adjoint_models(fake, fake, fake, 8, M, 4, _hip.F64, fake, fake, fake, None, None) == 1
    assert lib.cgps_peg_precision_adjoint_models(fake, fake, fake, 1, 2, 4, _hip.F64, fake, fake, fake, None, None) == 1   # R < 2


def test_c_entries_refuse_the_block_sizes_that_are_not_built():
    """d = 8 and fp64 d = 6 are refused before any launch (the pointers are never touched)."""
    lib = _hip.lib()
    fake = ctypes.c_void_p(256)
    for d, dt in ((8, _hip.F64), (8, _hip.F32), (6, _hip.F64), (9, _hip.F64)):
        assert lib.cgps_leg_loglik_models(fake, fake, 2, 10, 3, fake, fake, None, None, d, dt, 4096, fake, fake, None) == 3
        assert lib.cgps_peg_precision_models(fake, fake, fake, 8, 2, d, dt, fake, fake, fake, None) == 3
        assert lib.cgps_peg_precision_adjoint_models(fake, fake, fake, 8, 2, d, dt, fake, fake, fake, None, None) == 3
    # an empty batch is fine and launches nothing
    assert lib.cgps_leg_loglik_models(None, None, 0, 0, 3, None, None, None, None, 5, _hip.F64, 4096, None, None, None) == 0


def test_new_symbols_are_exported():
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ("cgps_leg_loglik_models", "cgps_peg_precision_models", "cgps_peg_precision_adjoint_models"):
        assert name in _hip.exported_symbols() and hasattr(lib, name), name
    assert _hip.lib().cgps_version() == 320


# ---- on the GPU ------------------------------------------------------------------------------------------------------

def _kernel_operands(d, dtype, M, lengths, seed):
    gen = torch.Generator().manual_seed(seed)
    ms = [_model(d, 1, dtype, seed + 17 * k) for k in range(M)]
    G = torch.stack([m.G for m in ms]).contiguous()
    A = torch.stack([m.B.T @ m.LLT_inv @ m.B for m in ms]).contiguous()
    # (fp32: gaps of at least 0.5, so that I - E^T E of the random generators stays well conditioned)
    ts, _ = _ragged(lengths, 1, gen, dtype, gap0=0.05 if dtype == F64 else 0.5)
    R = ts.shape[0]
    v = torch.randn(M, R, d, generator=gen, dtype=F64).to(dtype).cuda()
    q = torch.randn(M, R, generator=gen, dtype=F64).to(dtype).cuda()
    return G, A, ts, v, q, gen


BOUNDARY_LENGTHS = [1, 2, 3, 129, 255, 256, 257, 513, 600]     # rows per lane 1 -> 2 -> 3 at 256 and at 128 lanes


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("d", [1, 3, 5, 7])
def test_forward_kernel_is_the_batched_kernel_per_model_bit_for_bit(d, dtype):
    M, lengths = 3, BOUNDARY_LENGTHS
    G, A, ts, v, q, _ = _kernel_operands(d, dtype, M, lengths, 1000 + d)
    plan = leg._BatchPlan(lengths, "cuda")
    out, info = leg.leg_loglik_models_reductions(ts, G, A, v, q, plan)
    assert out.shape == (M, len(lengths), 4) and info.shape == (M, len(lengths), 2)
    assert not bool(torch.isnan(out).any()) and int(info.abs().max()) == 0
    for k in range(M):
        o1, i1 = leg.leg_loglik_batch_reductions(ts, G[k].contiguous(), A[k].contiguous(), v[k].contiguous(),
                                                 q[k].contiguous(), plan)
        assert torch.equal(out[k], o1), (k, (out[k] - o1).abs().max())
        assert torch.equal(info[k], i1), k


def _adjoint_models(ts, G, cut, gRs, gOs):
    M, d, R = G.shape[0], G.shape[1], ts.shape[0]
    part = torch.full((M, (R - 1 + 63) // 64, d, d), float("nan"), dtype=G.dtype, device="cuda")
    gtau = torch.full((M, R - 1), float("nan"), dtype=G.dtype, device="cuda")
    _hip.check(_hip.lib().cgps_peg_precision_adjoint_models(
        _hip.ptr(ts), _hip.ptr(G), _hip.ptr(cut), R, M, d, _hip.dtype_code(G.dtype), _hip.ptr(gRs), _hip.ptr(gOs),
        _hip.ptr(part), _hip.ptr(gtau), _hip.stream_ptr()))
    return part, gtau


def _adjoint_seg(ts, G, cut, gRs, gOs):
    d, R = G.shape[0], ts.shape[0]
    part = torch.full(((R - 1 + 63) // 64, d, d), float("nan"), dtype=G.dtype, device="cuda")
    gtau = torch.full((R - 1,), float("nan"), dtype=G.dtype, device="cuda")
    _hip.check(_hip.lib().cgps_peg_precision_adjoint_seg(
        _hip.ptr(ts), _hip.ptr(G), _hip.ptr(cut), R, d, _hip.dtype_code(G.dtype), _hip.ptr(gRs), _hip.ptr(gOs),
        _hip.ptr(part), _hip.ptr(gtau), _hip.stream_ptr()))
    return part, gtau


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("d", [1, 3, 5, 7])
def test_assembly_and_adjoint_are_the_seg_kernels_per_model_bit_for_bit(d, dtype):
    M, lengths = 3, BOUNDARY_LENGTHS
    G, _, ts, _, _, gen = _kernel_operands(d, dtype, M, lengths, 2000 + d)
    plan = leg._BatchPlan(lengths, "cuda")
    R = plan.R
    Rs, Os = leg._peg_precision_models(ts, G, plan.cut)
    assert Rs.shape == (M * R, d, d) and Os.shape == (M * R - 1, d, d)
    gRs = torch.randn(M * R, d, d, generator=gen, dtype=F64).to(dtype).cuda()
    gOs = torch.randn(M * R - 1, d, d, generator=gen, dtype=F64).to(dtype).cuda()
    part, gtau = _adjoint_models(ts, G, plan.cut, gRs, gOs)
    holed = gOs.clone()
    for k in range(1, M):
        assert int(torch.count_nonzero(Os[k * R - 1])) == 0, k          # the block between two models: exactly zero
        holed[k * R - 1] = float("nan")                                 # ... and its gradient is never read
    part2, gtau2 = _adjoint_models(ts, G, plan.cut, gRs, holed)
    assert torch.equal(part, part2) and torch.equal(gtau, gtau2)
    assert not bool(torch.isnan(part).any()) and not bool(torch.isnan(gtau).any())
    for k in range(M):
        Gk = G[k].contiguous()
        R1, O1 = leg._peg_precision_seg(ts, Gk, plan.cut)
        assert torch.equal(Rs[k * R:(k + 1) * R], R1), k
        assert torch.equal(Os[k * R:(k + 1) * R - 1], O1), k
        p1, t1 = _adjoint_seg(ts, Gk, plan.cut, gRs[k * R:(k + 1) * R].contiguous(), gOs[k * R:(k + 1) * R - 1].contiguous())
        assert torch.equal(part[k], p1), k
        assert torch.equal(gtau[k], t1), k
        cuts = plan.cut.bool()
        assert int(torch.count_nonzero(gtau[k][cuts])) == 0                 # a cut gap: gtau = 0


@pytest.mark.gpu
@pytest.mark.parametrize("d,dtype", [(1, F64), (5, F64), (4, F32)], ids=["d1-f64", "d5-f64", "d4-f32"])
def test_adjoint_wrapper_without_a_model_axis_is_its_one_model_form(d, dtype):
    """``leg._peg_precision_adjoint_models`` with G [d, d] (cgps_peg_precision_adjoint_seg) against G [1, d, d]
    (cgps_peg_precision_adjoint_models), with and without the gradient in ts; the assembly wrapper alongside."""
    lengths = [1, 2, 5, 64, 65]
    G, _, ts, _, _, gen = _kernel_operands(d, dtype, 1, lengths, 2500 + d)
    plan = leg._BatchPlan(lengths, "cuda")
    for a, b in zip(leg._peg_precision_models(ts, G[0], plan.cut), leg._peg_precision_models(ts, G, plan.cut)):
        assert torch.equal(a, b)
    gRs = torch.randn(plan.R, d, d, generator=gen, dtype=F64).to(dtype).cuda()
    gOs = torch.randn(plan.R - 1, d, d, generator=gen, dtype=F64).to(dtype).cuda()
    for want_ts in (True, False):
        gG, gts = leg._peg_precision_adjoint_models(ts, G[0], plan.cut, gRs, gOs, want_ts)
        gG1, gts1 = leg._peg_precision_adjoint_models(ts, G, plan.cut, gRs, gOs, want_ts)
        assert gG.shape == (d, d) and gG1.shape == (1, d, d) and torch.equal(gG, gG1[0])
        assert (gts is None and gts1 is None) if not want_ts else (gts.shape == ts.shape and torch.equal(gts, gts1))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("d", range(1, 9))
def test_against_one_batched_call_per_model_every_rank(d, dtype):
    """Ranks 1..8 in both dtypes (d = 8 and fp64 d = 6 take the documented loop over the models); obs_dim 1 and 2."""
    rtol = 1e-9 if dtype == F64 else 1e-3
    lengths = [1, 2, 129, 257, 300]
    for obs in (1, 2):
        ms = [_model(d, obs, dtype, 100 * d + obs + 7 * k) for k in range(2)]
        gen = torch.Generator().manual_seed(50 * d + obs)
        ts, xs = _ragged(lengths, obs, gen, dtype, gap0=0.05 if dtype == F64 else 0.5)
        out = leg.log_likelihood_models(ms, ts, xs, torch.tensor(lengths))
        assert out.shape == (2, len(lengths)) and out.dtype == dtype
        for k, m in enumerate(ms):
            ref = leg.log_likelihood_batch(m, ts, xs, lengths).tolist()
            for n, got, r in zip(lengths, out[k].tolist(), ref):
                print("d=%d %s obs=%d model %d n=%d: %.3e" % (d, dtype, obs, k, n, abs(got - r) / max(1.0, abs(r))))
                assert abs(got - r) <= rtol * max(1.0, abs(r)), (d, obs, k, n, got, r)


@pytest.mark.gpu
def test_dense_layout_equals_the_ragged_layout_of_equal_lengths():
    ms = [_model(4, 2, F64, s) for s in (11, 12, 13)]
    ts, xs = _ragged([40, 40, 40], 2, torch.Generator().manual_seed(5), F64)
    a = leg.log_likelihood_models(ms, ts, xs, [40, 40, 40])
    b = leg.log_likelihood_models(ms, ts.reshape(3, 40), xs.reshape(3, 40, 2))
    assert a.shape == (3, 3) and torch.equal(a, b)


@pytest.mark.gpu
def test_reference_values_and_gradients_three_models_three_series():
    """The unmodified LEGFamily at seeds 7, 8, 9 on series of 2, 33 and 40 rows (make_golden_models.py)."""
    g = np.load(os.path.join(_util.GOLDEN, "leg_models.npz"))
    t = lambda a: torch.from_numpy(a).to(F64).cuda()   # noqa: E731
    ms = [leg.LEGMatrices(*(t(g[name][k]).requires_grad_(True) for name in ("N", "R", "B", "Lambda"))) for k in range(3)]
    out = leg.log_likelihood_models(ms, t(g["ts"]), t(g["xs"]), g["lengths"].tolist())
    assert out.shape == (3, 3)
    np.testing.assert_allclose(out.detach().cpu().numpy(), g["ll"], rtol=1e-8, atol=0)
    out.sum().backward()
    for k, m in enumerate(ms):
        for got, key in ((m.N.grad.tril(), "gN"), (m.R.grad.tril(-1), "gR"), (m.B.grad, "gB"), (m.Lambda.grad.tril(), "gLambda")):
            np.testing.assert_allclose(got.cpu().numpy(), g[key][k], rtol=1e-6, atol=1e-7, err_msg="%s of model %d" % (key, k))


DENSE_LENGTHS = [1, 2, 17, 40]


@functools.lru_cache(maxsize=None)
def _dense_reference(d, obs):
    """Three models, four series, a random upstream gradient w[M, B]; the dense Gaussian of every (model, series) with
    everything observed, its gradients weighted and added up.  Computed once per (d, obs) and left unchanged."""
    M = 3
    models = [mr.leg_case(d, obs, 4, 900 + 10 * d + k)[0][:4] for k in range(M)]
    series = [mr.leg_case(d, obs, n, 700 + 10 * d + n)[0][4:6] for n in DENSE_LENGTHS]      # (xs, ts)
    w = torch.randn(M, len(DENSE_LENGTHS), generator=torch.Generator().manual_seed(d), dtype=F64)
    ll = torch.zeros(M, len(DENSE_LENGTHS), dtype=F64)
    gpar = [[torch.zeros_like(p) for p in mod] for mod in models]
    gxs = [torch.zeros_like(x) for x, _ in series]
    gts = [torch.zeros_like(t) for _, t in series]
    for k, mod in enumerate(models):
        for b, (x, t) in enumerate(series):
            val, grads = mr.leg_dense_value_and_grads(*mod, t, x, torch.ones(x.shape, dtype=torch.bool))
            ll[k, b] = val
            for acc, gp in zip(gpar[k], grads[:4]):
                acc += w[k, b] * gp
            gxs[b] += w[k, b] * grads[4]
            gts[b] += w[k, b] * grads[5]
    xs, ts = torch.cat([x for x, _ in series]), torch.cat([t for _, t in series])
    return models, ts, xs, w, ll, gpar, torch.cat(gxs), torch.cat(gts)


def _check_grad(got, want, what):
    """test_leg_batch_missing._check_grad, fp64"""
    want = want.detach().to("cpu", F64)
    assert got is not None, what + " is missing"
    got = got.detach().to("cpu", F64)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-7, atol=1e-10 * float(want.abs().max()), err_msg=what)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["all", "NR_frozen", "model_1_only"])
@pytest.mark.parametrize("d,obs", [(3, 2), (5, 1)])
def test_gradients_against_the_dense_reference(d, obs, which):
    models, ts, xs, w, ll, gpar, gxs, gts = _dense_reference(d, obs)
    train = []
    for k in range(len(models)):
        if which == "all":
            train.append((True, True, True, True))
        elif which == "NR_frozen":
            train.append((False, False, True, True))
        else:
            train.append((True, True, True, True) if k == 1 else (False, False, False, False))
    ms = [leg.LEGMatrices(*(p.clone().cuda().requires_grad_(r) for p, r in zip(mod, tr))) for mod, tr in zip(models, train)]
    t, x = ts.clone().cuda().requires_grad_(True), xs.clone().cuda().requires_grad_(True)
    out = leg.log_likelihood_models(ms, t, x, DENSE_LENGTHS)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ll.numpy(), rtol=1e-9)
    (out * w.cuda()).sum().backward()
    for k, (m, tr) in enumerate(zip(ms, train)):
        for name, p, want, r in zip(("N", "R", "B", "Lambda"), (m.N, m.R, m.B, m.Lambda), gpar[k], tr):
            if r:
                _check_grad(p.grad, want, "d%s of model %d" % (name, k))
            else:
                assert p.grad is None, (name, k)
    _check_grad(x.grad, gxs, "dxs")                     # (with one model trainable xs and ts still see all three)
    _check_grad(t.grad, gts, "dts")


def _values_and_grads(fn, ms, ts, xs, w):
    """fn(models, ts, xs) -> [M, B]; returns the values and the gradients of (out * w).sum() in every model's four
    matrices, xs and ts, on fresh leaves."""
    mm = [leg.LEGMatrices(*(p.detach().clone().requires_grad_(True) for p in (m.N, m.R, m.B, m.Lambda))) for m in ms]
    t, x = ts.detach().clone().requires_grad_(True), xs.detach().clone().requires_grad_(True)
    out = fn(mm, t, x)
    (out * w).sum().backward()
    grads = [p.grad for m in mm for p in (m.N, m.R, m.B, m.Lambda)] + [x.grad, t.grad]
    return out.detach(), grads


def _compare_with_the_loop(ms, ts, xs, lengths, w, value_rtol=1e-9):
    loop = lambda mm, t, x: torch.stack([leg.log_likelihood_batch(m, t, x, lengths) for m in mm])   # noqa: E731
    one = lambda mm, t, x: leg.log_likelihood_models(mm, t, x, lengths)                              # noqa: E731
    v0, g0 = _values_and_grads(loop, ms, ts, xs, w)
    v1, g1 = _values_and_grads(one, ms, ts, xs, w)
    for a, r in zip(v1.flatten().tolist(), v0.flatten().tolist()):
        assert abs(a - r) <= value_rtol * max(1.0, abs(r)), (a, r)
    names = ["%s of model %d" % (n, k) for k in range(len(ms)) for n in ("N", "R", "B", "Lambda")] + ["xs", "ts"]
    for name, a, r in zip(names, g1, g0):
        assert a is not None and r is not None, name
        np.testing.assert_allclose(a.cpu().numpy(), r.cpu().numpy(), rtol=1e-7, atol=1e-9, err_msg=name)


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [1, 2])
def test_gradients_at_kernel_boundary_sizes_against_the_loop(chunks, monkeypatch):
    """257 and 513 rows (rows per lane 1 -> 2 -> 3), two models at d = 5; then the same with the backward cut into two
    chunks of one model each."""
    lengths = [257, 513]
    ms = [_model(5, 1, F64, s) for s in (41, 42)]
    gen = torch.Generator().manual_seed(43)
    ts, xs = _ragged(lengths, 1, gen, F64)
    w = torch.randn(2, 2, generator=gen, dtype=F64).cuda()
    if chunks == 2:
        monkeypatch.setattr(leg, "MODELS_BACKWARD_MAX_ROWS", sum(lengths))
    _compare_with_the_loop(ms, ts, xs, lengths, w)


@pytest.mark.gpu
def test_bit_identical_repeats_and_independent_of_other_models_and_series():
    ms = [_model(5, 2, F64, s) for s in (3, 4)]
    lengths = [502, 33, 1, 129]
    gen = torch.Generator().manual_seed(6)
    ts, xs = _ragged(lengths, 2, gen, F64)
    a = leg.log_likelihood_models(ms, ts, xs, lengths)
    assert torch.equal(a, leg.log_likelihood_models(ms, ts, xs, lengths))
    # other models before and after
    more = [_model(5, 2, F64, 8)] + ms + [_model(5, 2, F64, 9), _model(5, 2, F64, 10)]
    b = leg.log_likelihood_models(more, ts, xs, lengths)
    assert torch.equal(b[1:3], a)
    # other series around them
    ts2, xs2 = _ragged([50, 700], 2, gen, F64)
    c = leg.log_likelihood_models(ms, torch.cat([ts2[:50], ts, ts2[50:]]), torch.cat([xs2[:50], xs, xs2[50:]]),
                                  [50] + lengths + [700])
    assert torch.equal(c[:, 1:-1], a)
    # a model alone is its row
    assert torch.equal(leg.log_likelihood_models(ms[1:], ts, xs, lengths)[0], a[1])


@pytest.mark.gpu
def test_repeated_time_stamp_names_its_model_and_series():
    ms = [_model(3, 1, F64, s) for s in (5, 6, 7)]
    lengths = [40, 300, 25, 60]
    ts, xs = _ragged(lengths, 1, torch.Generator().manual_seed(8), F64)
    clean = leg.log_likelihood_models(ms, ts, xs, lengths)
    bad = ts.clone()
    bad[40 + 300 + 11] = bad[40 + 300 + 10]                  # series 2, local rows 10 / 11: every model sees it
    with pytest.raises(cr.NotPSDError, match="model 0, series 2"):
        leg.log_likelihood_models(ms, bad, xs, lengths)
    prev = cr.CHECK_POSITIVE_DEFINITE
    cr.CHECK_POSITIVE_DEFINITE = False
    try:
        out = leg.log_likelihood_models(ms, bad, xs, lengths)
    finally:
        cr.CHECK_POSITIVE_DEFINITE = prev
    assert bool(torch.isnan(out[:, 2]).all())
    for b in (0, 1, 3):
        assert torch.equal(out[:, b], clean[:, b])


@pytest.mark.gpu
def test_a_series_above_batch_max_rows_takes_the_pair_kernel(monkeypatch):
    """BATCH_MAX_ROWS lowered to 64: the 300-row series goes through cgps_leg_mahal_logdet_pair per model, the others
    through the one launch.  (Plans are cached by lengths: no other test uses these.)"""
    lengths = [31, 300, 47]
    ms = [_model(5, 1, F64, s) for s in (51, 52)]
    gen = torch.Generator().manual_seed(53)
    ts, xs = _ragged(lengths, 1, gen, F64)
    w = torch.randn(2, 3, generator=gen, dtype=F64).cuda()
    ref = torch.stack([leg.log_likelihood_batch(m, ts, xs, lengths) for m in ms])      # the one launch, 4096 rows
    monkeypatch.setattr(leg, "BATCH_MAX_ROWS", 64)
    plan = leg._cached_batch_plan(lengths, ts.device)
    assert plan.long == [1]
    out = leg.log_likelihood_models(ms, ts, xs, lengths)
    for a, r in zip(out.flatten().tolist(), ref.flatten().tolist()):
        assert abs(a - r) <= 1e-9 * max(1.0, abs(r)), (a, r)
    _compare_with_the_loop(ms, ts, xs, lengths, w)

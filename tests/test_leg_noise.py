"""LEG series with per-observation noise variances on the GPU: the fused weighted-basis kernel
(cgps_leg_mahal_logdet_pair_w, chunk_reduce_kernel<.., SRC = 3>) against the unfused path; ``log_likelihood`` /
``insample_posterior`` / ``sample_from_posterior`` with ``noise_var=`` against the calls without it (zero variances),
the dense Gaussian of the observed entries (tests/_noiseref.py) and the limit of a huge variance; graph replay; errors."""
import math
import os

import numpy as np
import pytest
import torch

import _noiseref as nr
import _util
from cyclic_gps import _hip, leg
import cyclic_gps.cyclic_reduction as cr

F64, F32 = torch.float64, torch.float32
LEG_PARAMS = ("N", "R", "B", "Lambda", "xs", "ts", "noise_var")
TOL32_LEG = 1e-4                  # tests/test_gradients.py

KERNEL_CASES = [(1, F64), (2, F64), (3, F64), (4, F64), (5, F64), (7, F64), (2, F32), (4, F32), (5, F32), (6, F32), (7, F32)]
KERNEL_ROWS = (1, 2, 3, 255, 256, 257, 502, 5000, 70001)
KERNEL_KB = (1, 3, 36)


def _load(name="leg_co2like", device="cuda", dtype=F64):
    g = np.load(os.path.join(_util.GOLDEN, name + ".npz"))
    t = lambda k: torch.from_numpy(g[k]).to(dtype).to(device)   # noqa: E731
    return g, leg.LEGMatrices(t("N"), t("R"), t("B"), t("Lambda")), t("ts"), t("xs")


# ---- the kernel ------------------------------------------------------------------------------------------------------
def _kernel_model(d, dtype, seed, Kb):
    """(G, basis [Kb, d, d], generator), CPU tensors already rounded to ``dtype``.  G as in
    test_leg_missing._kernel_model: the diagonal of N from [0.8, 1.2], not 0.8 + 0.4 * randn, because a diagonal entry
    near zero makes the symmetric part of G nearly singular and then the unfused reference itself, whose blocks are
    rounded to fp32 before the fp64 elimination, is far off the same blocks computed in fp64.  The basis blocks are
    symmetric positive semi-definite of rank 2, as B^T Li B is; non-negative weights keep K positive definite.
    Worst error of that reference with fp32-rounded blocks (torch on the CPU, oracle/cr_oracle.py) against fp64 blocks
    of the same fp32 inputs, over every fp32 case of the test below (5 block sizes x 3 Kb x 9 lengths x 4 weightings):
    1.19e-4 in the mahal term (d = 5, Kb = 3, n = 255, all-zero weights) and 5.9e-6 in either log-determinant (d = 4,
    Kb = 3, n = 2, all-zero weights), relative to max(1, |value|): a 25-fold and a 50-fold margin to the 3e-3 and 3e-4
    the comparison allows (REFERENCE_ERROR_FP32)."""
    gen = torch.Generator().manual_seed(seed)
    Nm = torch.tril(0.4 * torch.randn(d, d, generator=gen, dtype=F64), -1)
    Nm = Nm + torch.diag(0.8 + 0.4 * torch.rand(d, generator=gen, dtype=F64))
    Rm = torch.tril(0.3 * torch.randn(d, d, generator=gen, dtype=F64), -1)
    G = Nm @ Nm.T + Rm - Rm.T + 1e-5 * torch.eye(d, dtype=F64)
    Bs = torch.randn(Kb, d, 2, generator=gen, dtype=F64)
    basis = 0.5 * Bs @ Bs.transpose(-1, -2)
    return G.to(dtype), basis.to(dtype), gen


def _kernel_series(n, d, dtype, gen):
    ts = torch.cumsum(0.05 + 0.5 * torch.rand(n, generator=gen, dtype=F64), 0).to(dtype)
    v = torch.randn(n, d, generator=gen, dtype=F64).to(dtype)
    return ts, v


def _weightings(n, Kb, dtype, gen):
    """name -> weights [n, Kb]: random in [0, 2]; all zero (the prior system); all equal; and random with runs of
    all-zero rows across the boundaries of waves and tiles (rows 63/64, 127/128, 255/256, 511/512) and n / 2."""
    out = {"random": 2.0 * torch.rand(n, Kb, generator=gen, dtype=F64), "zero": torch.zeros(n, Kb, dtype=F64),
           "equal": torch.full((n, Kb), 0.7, dtype=F64)}
    runs = 2.0 * torch.rand(n, Kb, generator=gen, dtype=F64)
    for k in (64, 128, 256, 512, n // 2):
        runs[max(0, k - 7):k + 9] = 0
    out["runs"] = runs
    return {name: w.to(dtype) for name, w in out.items()}


def kernel_cases(d, dtype):
    """Every (Kb, n, name, G, basis, ts, v, weights) of the kernel test, on the CPU in ``dtype``."""
    for Kb in KERNEL_KB:
        G, basis, gen = _kernel_model(d, dtype, 500 + 10 * d + Kb, Kb)
        for n in KERNEL_ROWS:
            ts, v = _kernel_series(n, d, dtype, gen)
            for name, w in _weightings(n, Kb, dtype, gen).items():
                yield Kb, n, name, G, basis, ts, v, w


REFERENCE_ERROR_FP32 = {"mahal": 1.19e-4, "logdet": 5.9e-6}
"""Worst error of the unfused fp32 reference over every fp32 case of ``kernel_cases`` (see ``_kernel_model``); the
tolerances below are 3e-3 and 3e-4."""


@pytest.mark.gpu
@pytest.mark.parametrize("d,dtype", KERNEL_CASES, ids=lambda p: str(p).replace("torch.", ""))
def test_weighted_basis_kernel_against_unfused_every_block_size(d, dtype):
    """Both sides of one tile, of two tiles and of the switch from one row per lane to several; one, three and 36
    basis blocks; all-zero weights are the prior system, whose half is the one-system kernel's value."""
    rtol = 1e-9 if dtype == F64 else 3e-4
    last = None
    for Kb, n, name, G, basis, ts, v, w in kernel_cases(d, dtype):
        G, basis, ts, v, w = (t.cuda() for t in (G, basis, ts, v, w))
        if last != (Kb, n):
            last = (Kb, n)
            Rs, Os = leg.peg_precision(ts, G)
            Rs, Os = Rs.double(), Os.double()
            _, s0 = leg.leg_mahal_and_det(ts, G)             # the prior half reads no basis: the one-system kernel's value
        A = torch.einsum("nk,kij->nij", w.double(), basis.double())
        m0, l0 = cr.mahal_and_det(Rs + A, Os, v.double())
        m1, l1, s1 = leg.leg_loglik_reductions_w(ts, G, basis, w, v)
        what = (Kb, n, name)
        assert abs(float(l1) - float(l0)) <= rtol * max(1.0, abs(float(l0))), (what, float(l1), float(l0))
        assert abs(float(m1) - float(m0)) <= 10 * rtol * max(1.0, abs(float(m0))), (what, float(m1), float(m0))
        assert abs(float(s1) - float(s0)) <= rtol * max(1.0, abs(float(s0))), (what, float(s1), float(s0))
        if name == "zero":                                   # adding 0 * basis changes no bit of a row: K is the prior precision
            assert abs(float(l1) - float(s1)) <= 1e-12 * max(1.0, abs(float(s1))), (what, float(l1), float(s1))


@pytest.mark.gpu
@pytest.mark.parametrize("d,n", [(5, 502), (3, 70001), (4, 257), (1, 1)])
def test_equal_weights_are_the_one_block_kernel(d, n):
    for Kb in KERNEL_KB:
        G, basis, gen = _kernel_model(d, F64, 77 + d + Kb, Kb)
        ts, v = _kernel_series(n, d, F64, gen)
        G, basis, ts, v = G.cuda(), basis.cuda(), ts.cuda(), v.cuda()
        want = leg.leg_loglik_reductions(ts, G, 0.7 * basis.sum(0), v)
        w = torch.full((n, Kb), 0.7, dtype=F64, device="cuda")
        for _ in range(2):                                           # (the counters are back at zero after a call)
            got = leg.leg_loglik_reductions_w(ts, G, basis, w, v)
            for k, (a, b) in enumerate(zip(got, want)):
                assert abs(float(a) - float(b)) <= (1e-8 if k == 0 else 1e-9) * max(1.0, abs(float(b))), (Kb, k, float(a), float(b))


@pytest.mark.gpu
def test_argument_errors_before_any_launch():
    G, basis, gen = _kernel_model(3, F64, 5, 6)
    G, basis = G.cuda(), basis.cuda()
    n = 10
    ts = torch.arange(n, dtype=F64).cuda()
    v, w = torch.zeros(n, 3, dtype=F64).cuda(), torch.ones(n, 6, dtype=F64).cuda()
    ws = _hip.pair_workspace(n, 3, F64, G.device)
    out, info = torch.zeros(4, dtype=F64).cuda(), torch.zeros(2, dtype=torch.int32).cuda()
    call = lambda bs, Kb, wt: _hip.lib().cgps_leg_mahal_logdet_pair_w(       # noqa: E731
        _hip.ptr(ts), _hip.ptr(G), bs, Kb, wt, _hip.ptr(v), n, 3, _hip.F64, _hip.ptr(ws), ws.numel(), _hip.ptr(out),
        _hip.ptr(info), _hip.stream_ptr())
    assert call(_hip.ptr(basis), 0, _hip.ptr(w)) == 1 and call(_hip.ptr(basis), 65, _hip.ptr(w)) == 1
    assert call(None, 6, _hip.ptr(w)) == 1 and call(_hip.ptr(basis), 6, None) == 1
    assert call(_hip.ptr(basis), 6, _hip.ptr(w)) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        leg.leg_loglik_reductions_w(ts, G, basis, w[:, :5], v)
    with pytest.raises(ValueError):
        leg.leg_loglik_reductions_w(ts, G, basis, w.float(), v)
    with pytest.raises(ValueError):
        leg.leg_loglik_reductions_w(ts, G, basis, w.cpu(), v)


# ---- log-likelihood -----------------------------------------------------------------------------------------------
def _golden_masks(n):
    """test_leg_missing._golden_masks"""
    rand = torch.rand(n, generator=torch.Generator().manual_seed(1)) > 0.3
    gap = torch.ones(n, dtype=torch.bool)
    gap[262:n - 228] = False
    gap[-28:] = False
    gap[0] = False
    return {"rand30": rand, "gap": gap}


@pytest.mark.gpu
def test_zero_variance_is_the_call_without_it_on_the_golden_series():
    g, m, ts, xs = _load()
    n = ts.shape[0]
    assert leg.fused_supported(ts, m.G)
    zeros = torch.zeros(n, 1, dtype=F64, device="cuda")
    plain = float(leg.log_likelihood(m, ts, xs))
    for s in (zeros, zeros[:, 0]):
        got = float(leg.log_likelihood(m, ts, xs, noise_var=s))
        assert abs(got - plain) <= 1e-9 * abs(plain), (got, plain)
    assert abs(plain - float(g["ll"])) <= 1e-8 * abs(float(g["ll"]))
    for name, mask in _golden_masks(n).items():
        mask = mask.cuda()
        want = float(leg.log_likelihood(m, ts, xs, observed=mask))
        nan = torch.full_like(zeros, float("nan"))
        got = float(leg.log_likelihood(m, ts, xs, observed=mask, noise_var=torch.where(mask.unsqueeze(-1), zeros, nan)))
        assert abs(got - want) <= 1e-9 * abs(want), (name, got, want)
        os.environ["CGPS_LEG_UNFUSED"] = "1"
        try:
            got = float(leg.log_likelihood(m, ts, xs, observed=mask, noise_var=zeros))
        finally:
            del os.environ["CGPS_LEG_UNFUSED"]
        assert abs(got - want) <= 1e-9 * abs(want), (name, "unfused", got, want)


DENSE_CASES = {(3, 1, 37): 21, (3, 2, 37): 22, (5, 1, 37): 23, (5, 2, 37): 24}
_dense = {}


def _dense_ref(d, obs, n):
    key = (d, obs, n)
    if key not in _dense:
        case, mask = nr.leg_case(d, obs, n, DENSE_CASES[key])
        Nm, Rm, Bm, Lm, xs, ts, s = case
        _dense[key] = case, mask, nr.leg_dense_value_and_grads(Nm, Rm, Bm, Lm, ts, xs, s, mask)
    return _dense[key]


def _check_value(got, want, dtype, what, tol32=1e-5):
    tol = 1e-9 if dtype == F64 else tol32
    assert abs(float(got) - float(want)) <= tol * max(abs(float(want)), 1.0), (what, float(got), float(want))


def _check_grad(got, want, dtype, what):
    want = want.detach().to("cpu", F64)
    assert got is not None, what + " is missing"
    got = got.detach().to("cpu", F64)
    scale = float(want.abs().max())
    if dtype == F64:
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-7, atol=1e-10 * scale, err_msg=what)
    else:
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=TOL32_LEG * scale + 1e-30, err_msg=what)


def _device_case(case, mask, dtype):
    """[N, R, B, Lambda, xs, ts, s] on the device, NaN in the unobserved entries of xs and s"""
    nan = torch.full_like(case[4], float("nan"))
    p = list(case[:4]) + [torch.where(mask, case[4], nan), case[5], torch.where(mask, case[6], nan)]
    return [t.to(dtype).cuda() for t in p]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("d,obs,n", list(DENSE_CASES))
def test_noise_variances_against_the_dense_reference(d, obs, n, dtype):
    """ll on the fused path (no gradient), then ll and all seven gradients (unfused path) against autograd through the
    dense density of the observed entries; the gradients of xs and noise_var are exactly zero where nothing is
    observed."""
    case, mask, (ll, grads) = _dense_ref(d, obs, n)
    mask_d = mask.cuda()
    p = _device_case(case, mask, dtype)
    with torch.no_grad():
        assert leg.fused_supported(p[5], leg.LEGMatrices(*p[:4]).G)
        _check_value(leg.log_likelihood(leg.LEGMatrices(*p[:4]), p[5], p[4], observed=mask_d, noise_var=p[6]), ll, dtype, "ll fused")
    p = [t.requires_grad_(True) for t in p]
    out = leg.log_likelihood(leg.LEGMatrices(*p[:4]), p[5], p[4], observed=mask_d, noise_var=p[6])
    _check_value(out, ll, dtype, "ll")
    out.backward()
    for name, leaf, want in zip(LEG_PARAMS, p, grads):
        _check_grad(leaf.grad, want, dtype, "d ll / d %s" % name)
    assert float(p[4].grad[~mask_d].abs().max()) == 0.0 and float(p[6].grad[~mask_d].abs().max()) == 0.0


@pytest.mark.gpu
def test_noise_variances_with_N_and_R_frozen():
    case, mask, (ll, grads) = _dense_ref(3, 2, 37)
    train = ("B", "Lambda", "noise_var")
    p = [t.requires_grad_(name in train) for t, name in zip(_device_case(case, mask, F64), LEG_PARAMS)]
    out = leg.log_likelihood(leg.LEGMatrices(*p[:4]), p[5], p[4], observed=mask.cuda(), noise_var=p[6])
    _check_value(out, ll, F64, "ll")
    out.backward()
    for name, leaf, want in zip(LEG_PARAMS, p, grads):
        if name in train:
            _check_grad(leaf.grad, want, F64, "d ll / d %s" % name)
        else:
            assert leaf.grad is None, name


# ---- posterior and sampling ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("d,obs", [(3, 2), (5, 1)])
def test_posterior_at_all_rows_against_the_dense_conditional(d, obs):
    n = 37
    case, mask, _ = _dense_ref(d, obs, n)
    Nm, Rm, Bm, Lm, xs, ts, s = case
    want_mean, want_cov = nr.leg_dense_posterior(Nm, Rm, Bm, Lm, ts, xs, s, mask)
    p = _device_case(case, mask, F64)
    with torch.no_grad():
        mean, (Sd, So) = leg.insample_posterior(leg.LEGMatrices(*p[:4]), p[5], p[4], observed=mask.cuda(), noise_var=p[6])
    i = torch.arange(n)
    np.testing.assert_allclose(mean.cpu().numpy(), want_mean.numpy(), rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(Sd.cpu().numpy(), want_cov[i, :, i, :].numpy(), rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(So.cpu().numpy(), want_cov[i[1:], :, i[:-1], :].numpy(), rtol=1e-7, atol=1e-9)


@pytest.mark.gpu
def test_posterior_sample_is_the_sampler_on_the_same_system():
    """With targets merged in: the noise of the merged series is zeros with noise_all[observed_all] = noise_var."""
    case, _, _ = _dense_ref(5, 2, 37)
    p = [t.cuda() for t in case]
    m = leg.LEGMatrices(*p[:4])
    xs, ts, s = p[4], p[5], p[6]
    tt = torch.cat([ts[:1] - 0.7, (ts[20:29] + ts[21:30]) / 2, ts[-1:] + 1.3])       # before, between and after the data
    ts_all, xs_all, observed, where = leg.merge_targets(ts, xs, tt)
    noise_all = torch.zeros(ts_all.shape[0], 2, dtype=F64, device="cuda")
    noise_all[observed] = s
    S, seed = 6, 1234
    z = leg.sample_from_posterior(m, ts_all, xs_all, S, seed, observed=observed, noise_var=noise_all)
    assert z.shape == (37 + 11, 5, S) and torch.isfinite(z).all()
    basis, weights, Li_rows, _ = leg.observation_weights(m, observed, noise_all)
    xz = torch.where(observed.unsqueeze(-1), xs_all, torch.zeros_like(xs_all))
    v = ((xz.unsqueeze(1) @ Li_rows).squeeze(1) @ m.B).contiguous()
    Rs, Os = leg.peg_precision(ts_all, m.G)
    dec, mean = cr.decompose_solve(Rs + torch.einsum("nk,kij->nij", weights, basis), Os, v)
    assert torch.equal(z, cr.sample(dec, S, seed, mean=mean))
    assert float(weights[where].abs().max()) == 0.0                 # the targets observe nothing


@pytest.mark.gpu
def test_a_huge_variance_is_a_missing_row():
    """A limit that needs no reference.  Rows with s = 1e12 carry no information: the posterior is that of the series
    with those rows masked, and the log-likelihood is the masked one plus the density of the rows' values under the
    huge variance alone, -1/2 log(2 pi 1e12) each (what the model and the 1e-12 of the row's precision add is below
    1e-11 relative)."""
    g, m, ts, xs = _load()
    n = ts.shape[0]
    assert (n, m.G.shape[0], ts.dtype) == (502, 5, F64)
    rows = torch.tensor([0, 63, 64, 250, 251, 501])
    mask = torch.ones(n, dtype=torch.bool)
    mask[rows] = False
    mask = mask.cuda()
    s = torch.zeros(n, 1, dtype=F64, device="cuda")
    s[~mask] = 1e12
    with torch.no_grad():
        want = float(leg.log_likelihood(m, ts, xs, observed=mask))
        got = float(leg.log_likelihood(m, ts, xs, noise_var=s)) + 0.5 * len(rows) * math.log(2 * math.pi * 1e12)
        assert abs(got - want) <= 1e-6 * abs(want), (got, want)
        mean0, (Sd0, So0) = leg.insample_posterior(m, ts, xs, observed=mask)
        mean1, (Sd1, So1) = leg.insample_posterior(m, ts, xs, noise_var=s)
    for a, b in ((mean1, mean0), (Sd1, Sd0), (So1, So0)):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-6, atol=1e-6 * float(b.abs().max()))


# ---- graph, errors ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_noise_log_likelihood_replays_from_a_graph():
    g, m, ts, xs = _load()
    n = ts.shape[0]
    gen = torch.Generator().manual_seed(3)
    s = torch.rand(n, 1, generator=gen, dtype=F64).cuda()
    graphed = leg.Graphed(leg.log_likelihood, m, ts, xs, noise_var=s)
    for _ in range(3):
        ll = float(graphed())
    ref = float(leg.log_likelihood(m, ts, xs, noise_var=s))
    assert abs(ll - ref) <= 1e-10 * abs(ref)
    s.copy_(2.0 * torch.rand(n, 1, generator=gen, dtype=F64).cuda())           # new variances in place: the replay follows
    ll2 = float(graphed())
    ref2 = float(leg.log_likelihood(m, ts, xs, noise_var=s))
    assert abs(ll2 - ref2) <= 1e-10 * abs(ref2) and abs(ll2 - ll) > 1e-6


@pytest.mark.gpu
def test_zero_length_gap():
    case, mask, _ = _dense_ref(3, 2, 37)
    p = [t.cuda() for t in case]
    m = leg.LEGMatrices(*p[:4])
    ts = p[5].clone()
    ts[20] = ts[19]
    with pytest.raises(cr.NotPSDError):
        leg.log_likelihood(m, ts, p[4], observed=mask.cuda(), noise_var=p[6])
    with pytest.raises(cr.NotPSDError):
        leg.log_likelihood(m, ts, p[4], noise_var=p[6][:, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("d", [6, 8])
def test_block_sizes_without_a_fused_kernel_take_the_unfused_path(d):
    case, mask = nr.leg_case(d, 2, 20, 60 + d)
    Nm, Rm, Bm, Lm, xs, ts, s = case
    want = nr.leg_dense_loglik(Nm, Rm, Bm, Lm, ts, xs, s, mask)
    p = [t.cuda() for t in case]
    m = leg.LEGMatrices(*p[:4])
    assert not leg.fused_supported(p[5], m.G)
    with torch.no_grad():
        _check_value(leg.log_likelihood(m, p[5], p[4], observed=mask.cuda(), noise_var=p[6]), want, F64, "ll d=%d" % d)
    with pytest.raises(_hip.CgpsError):
        basis, weights, _, _ = leg.observation_weights(m, mask.cuda(), p[6])
        leg.leg_loglik_reductions_w(p[5], m.G, basis, weights, torch.zeros(20, d, dtype=F64, device="cuda"))

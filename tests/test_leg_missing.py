"""LEG series with missing observations on the GPU: the fused per-row pattern kernel (cgps_leg_mahal_logdet_pair_obs,
chunk_reduce_kernel<.., SRC = 2>) against the unfused path; ``log_likelihood`` / ``insample_posterior`` /
``sample_from_posterior`` with ``observed=`` against marginalisation (rows deleted), the dense Gaussian of the observed
entries (tests/_missref.py) and ``predict.predictive_posterior``; graph replay; errors."""
import os

import numpy as np
import pytest
import torch

import _missref as mr
import _util
from cyclic_gps import _hip, leg, predict
import cyclic_gps.cyclic_reduction as cr

F64, F32 = torch.float64, torch.float32
LEG_PARAMS = ("N", "R", "B", "Lambda", "xs", "ts")
TOL32_LEG = 1e-4                  # tests/test_gradients.py


def _load(name="leg_co2like", device="cuda", dtype=F64):
    g = np.load(os.path.join(_util.GOLDEN, name + ".npz"))
    t = lambda k: torch.from_numpy(g[k]).to(dtype).to(device)   # noqa: E731
    return g, leg.LEGMatrices(t("N"), t("R"), t("B"), t("Lambda")), t("ts"), t("xs")


def _golden_masks(n):
    """The two masks of the marginalisation check: 30 % of the rows missing at random; the hole and the tail the
    reference's CO2 split leaves out (dataset_process_utils.py:22-23, scaled to this series) plus the first row."""
    rand = torch.rand(n, generator=torch.Generator().manual_seed(1)) > 0.3
    gap = torch.ones(n, dtype=torch.bool)
    gap[262:n - 228] = False
    gap[-28:] = False
    gap[0] = False
    return {"rand30": rand, "gap": gap}


# ---- the kernel ------------------------------------------------------------------------------------------------------
def _kernel_model(d, dtype, seed, P):
    """The diagonal of N is drawn from [0.8, 1.2], not 0.8 + 0.4 * randn: a diagonal entry near zero makes the symmetric
    part of G nearly singular (smallest eigenvalue 0.009 for some seeds), and then the unfused reference itself, whose
    blocks are rounded to fp32 before the fp64 elimination, is off by up to 0.2 relative in the mahal term against the
    same blocks computed in fp64 - far outside the 3e-3 the comparison allows. With the bounded diagonal that error of
    the reference is at most 1.2e-4 (mahal) and 8e-6 (log-det) over every fp32 case below, a 25-fold margin."""
    gen = torch.Generator().manual_seed(seed)
    Nm = torch.tril(0.4 * torch.randn(d, d, generator=gen, dtype=F64), -1)
    Nm = Nm + torch.diag(0.8 + 0.4 * torch.rand(d, generator=gen, dtype=F64))
    Rm = torch.tril(0.3 * torch.randn(d, d, generator=gen, dtype=F64), -1)
    G = Nm @ Nm.T + Rm - Rm.T + 1e-5 * torch.eye(d, dtype=F64)
    Bs = torch.randn(P, d, 2, generator=gen, dtype=F64)
    table = 0.5 * Bs @ Bs.transpose(-1, -2)
    table[0] = 0                                              # entry 0: a row that observes nothing
    return G.to(dtype).cuda(), table.to(dtype).cuda(), gen


def _patterns(n, P, gen):
    """name -> uint8 [n]: random entries, every row the last entry, every row entry 0 (nothing observed), and runs of
    entry 0 across the boundaries of lane chunks (1 or 2 rows here) and of tiles (multiples of 64 ... 512 rows)."""
    out = {"random": torch.randint(0, P, (n,), generator=gen).to(torch.uint8),
           "all": torch.full((n,), P - 1, dtype=torch.uint8), "none": torch.zeros(n, dtype=torch.uint8)}
    runs = torch.randint(1, P, (n,), generator=gen).to(torch.uint8)
    for k in (0, 64, 128, 256, 512, 1024, n // 2, n):
        runs[max(0, k - 7):k + 9] = 0
    out["runs"] = runs
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("d,dtype", [(1, F64), (2, F64), (3, F64), (4, F64), (5, F64), (7, F64), (2, F32), (4, F32),
                                     (5, F32), (6, F32), (7, F32)], ids=lambda p: str(p).replace("torch.", ""))
def test_pattern_kernel_against_unfused_every_block_size(d, dtype):
    """Both sides of one tile, of two tiles and of the switch from one row per lane to several; tables of 2 and 8
    entries; a byte past a deliberately short table takes its last entry."""
    rtol = 1e-9 if dtype == F64 else 3e-4
    for P in (2, 8):
        G, table, gen = _kernel_model(d, dtype, 300 + 10 * d + P, P)
        for n in (1, 2, 3, 255, 256, 257, 502, 5000, 70001):
            ts = torch.cumsum(0.05 + 0.5 * torch.rand(n, generator=gen, dtype=F64), 0).to(dtype).cuda()
            v = torch.randn(n, d, generator=gen, dtype=F64).to(dtype).cuda()
            Rs, Os = leg.peg_precision(ts, G)
            Rs, Os = Rs.double(), Os.double()
            _, s0 = leg.leg_mahal_and_det(ts, G)             # the prior half reads no table: the one-system kernel's value
            cases = [(name, pat.cuda(), table) for name, pat in _patterns(n, P, gen).items()]
            wild = torch.randint(0, 256, (n,), generator=gen).to(torch.uint8).cuda()
            wild[-1] = 255
            cases.append(("clamped", wild, table[:2].clone()))
            for name, pat, tab in cases:
                idx = pat.long().clamp(max=tab.shape[0] - 1)
                m0, l0 = cr.mahal_and_det(Rs + tab.double()[idx], Os, v.double())
                m1, l1, s1 = leg.leg_loglik_reductions_obs(ts, G, tab, pat, v)
                what = (P, n, name)
                assert abs(float(l1) - float(l0)) <= rtol * max(1.0, abs(float(l0))), (what, float(l1), float(l0))
                assert abs(float(m1) - float(m0)) <= 10 * rtol * max(1.0, abs(float(m0))), (what, float(m1), float(m0))
                assert abs(float(s1) - float(s0)) <= rtol * max(1.0, abs(float(s0))), (what, float(s1), float(s0))


@pytest.mark.gpu
@pytest.mark.parametrize("d,n", [(5, 502), (3, 70001), (4, 257), (1, 1)])
def test_all_observed_table_equals_the_one_block_kernel(d, n):
    G, table, gen = _kernel_model(d, F64, 77 + d, 2)
    ts = torch.cumsum(0.05 + torch.rand(n, generator=gen, dtype=F64), 0).cuda()
    v = torch.randn(n, d, generator=gen, dtype=F64).cuda()
    want = leg.leg_loglik_reductions(ts, G, table[1], v)
    for _ in range(2):                                           # (the counters are back at zero after a call)
        got = leg.leg_loglik_reductions_obs(ts, G, table, torch.ones(n, dtype=torch.uint8, device="cuda"), v)
        for k, (a, b) in enumerate(zip(got, want)):
            assert abs(float(a) - float(b)) <= (1e-8 if k == 0 else 1e-9) * max(1.0, abs(float(b))), (k, float(a), float(b))


@pytest.mark.gpu
def test_argument_errors_before_any_launch():
    G, table, gen = _kernel_model(3, F64, 5, 2)
    n = 10
    ts = torch.arange(n, dtype=F64).cuda()
    v, pat = torch.zeros(n, 3, dtype=F64).cuda(), torch.zeros(n, dtype=torch.uint8).cuda()
    ws = _hip.pair_workspace(n, 3, F64, G.device)
    out, info = torch.zeros(4, dtype=F64).cuda(), torch.zeros(2, dtype=torch.int32).cuda()
    call = lambda tab, P, pt: _hip.lib().cgps_leg_mahal_logdet_pair_obs(       # noqa: E731
        _hip.ptr(ts), _hip.ptr(G), tab, P, pt, _hip.ptr(v), n, 3, _hip.F64, _hip.ptr(ws), ws.numel(), _hip.ptr(out),
        _hip.ptr(info), _hip.stream_ptr())
    assert call(_hip.ptr(table), 0, _hip.ptr(pat)) == 1 and call(_hip.ptr(table), 257, _hip.ptr(pat)) == 1
    assert call(None, 2, _hip.ptr(pat)) == 1 and call(_hip.ptr(table), 2, None) == 1
    assert call(_hip.ptr(table), 2, _hip.ptr(pat)) == 0
    torch.cuda.synchronize()


# ---- log-likelihood -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_missing_rows_are_marginalised_on_the_golden_series():
    g, m, ts, xs = _load()
    n = ts.shape[0]
    assert leg.fused_supported(ts, m.G)
    full = leg.log_likelihood(m, ts, xs, observed=torch.ones(n, dtype=torch.bool, device="cuda"))
    assert abs(float(full) - float(g["ll"])) <= 1e-8 * abs(float(g["ll"]))
    for name, mask in _golden_masks(n).items():
        mask = mask.cuda()
        want = float(leg.log_likelihood(m, ts[mask], xs[mask]))
        holed = torch.where(mask.unsqueeze(-1), xs, torch.full_like(xs, float("nan")))       # what is missing is ignored
        for obs in (mask, mask.unsqueeze(-1)):
            got = float(leg.log_likelihood(m, ts, holed, observed=obs))
            assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (name, got, want)
        os.environ["CGPS_LEG_UNFUSED"] = "1"
        try:
            got = float(leg.log_likelihood(m, ts, holed, observed=mask))
        finally:
            del os.environ["CGPS_LEG_UNFUSED"]
        assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (name, "unfused", got, want)


DENSE_CASES = {(3, 3, 37): 11, (5, 2, 64): 12}
_dense = {}


def _dense_ref(d, obs, n):
    key = (d, obs, n)
    if key not in _dense:
        case, mask = mr.leg_case(d, obs, n, DENSE_CASES[key])
        Nm, Rm, Bm, Lm, xs, ts = case
        _dense[key] = case, mask, mr.leg_dense_value_and_grads(Nm, Rm, Bm, Lm, ts, xs, mask)
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


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("d,obs,n", list(DENSE_CASES))
def test_partial_channels_against_the_dense_reference(d, obs, n, dtype):
    """ll on the fused path (no gradient), then ll and all six gradients (unfused path) against autograd through the
    dense density of the observed entries; the gradient of xs is exactly zero where nothing is observed."""
    case, mask, (ll, grads) = _dense_ref(d, obs, n)
    mask_d = mask.cuda()
    nan_xs = torch.where(mask, case[4], torch.full_like(case[4], float("nan")))
    p = [t.to(dtype).cuda() for t in case[:4]] + [nan_xs.to(dtype).cuda(), case[5].to(dtype).cuda()]
    with torch.no_grad():
        assert leg.fused_supported(p[5], leg.LEGMatrices(*p[:4]).G)
        _check_value(leg.log_likelihood(leg.LEGMatrices(*p[:4]), p[5], p[4], observed=mask_d), ll, dtype, "ll fused")
    p = [t.requires_grad_(True) for t in p]
    out = leg.log_likelihood(leg.LEGMatrices(*p[:4]), p[5], p[4], observed=mask_d)
    _check_value(out, ll, dtype, "ll")
    out.backward()
    for name, leaf, want in zip(LEG_PARAMS, p, grads):
        _check_grad(leaf.grad, want, dtype, "d ll / d %s" % name)
    assert float(p[4].grad[~mask_d].abs().max()) == 0.0


@pytest.mark.gpu
def test_partial_channels_with_N_and_R_frozen():
    case, mask, (ll, grads) = _dense_ref(3, 3, 37)
    p = [t.cuda().requires_grad_(name in ("B", "Lambda")) for t, name in zip(case, LEG_PARAMS)]
    out = leg.log_likelihood(leg.LEGMatrices(*p[:4]), p[5], p[4], observed=mask.cuda())
    _check_value(out, ll, F64, "ll")
    out.backward()
    for name, leaf, want in zip(LEG_PARAMS, p, grads):
        if name in ("B", "Lambda"):
            _check_grad(leaf.grad, want, F64, "d ll / d %s" % name)
        else:
            assert leaf.grad is None, name


# ---- posterior and sampling ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_posterior_at_all_rows_against_the_dense_conditional():
    case, mask, _ = _dense_ref(3, 3, 37)
    Nm, Rm, Bm, Lm, xs, ts = case
    n, d = 37, 3
    want_mean, want_cov = mr.leg_dense_posterior(Nm, Rm, Bm, Lm, ts, xs, mask)
    m = leg.LEGMatrices(Nm, Rm, Bm, Lm).to("cuda")
    with torch.no_grad():
        mean, (Sd, So) = leg.insample_posterior(m, ts.cuda(), xs.cuda(), observed=mask.cuda())
    i = torch.arange(n)
    np.testing.assert_allclose(mean.cpu().numpy(), want_mean.numpy(), rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(Sd.cpu().numpy(), want_cov[i, :, i, :].numpy(), rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(So.cpu().numpy(), want_cov[i[1:], :, i[:-1], :].numpy(), rtol=1e-7, atol=1e-9)


@pytest.mark.gpu
def test_posterior_at_merged_targets_is_the_predictive_posterior():
    """Rows the reference's split leaves out, put back as targets: the posterior at those rows is what the pairwise
    stitch of ``predict.predictive_posterior`` gives from the observed rows alone (tolerance of test_leg.py)."""
    g, m, ts, xs = _load()
    mask = _golden_masks(ts.shape[0])["gap"].cuda()
    lm, lv = predict.predictive_posterior(m, ts[mask], xs[mask], ts[~mask])
    ts_all, xs_all, observed, where = leg.merge_targets(ts[mask], xs[mask], ts[~mask])
    assert torch.equal(ts_all, ts) and torch.equal(observed, mask) and torch.equal(xs_all[mask], xs[mask])
    with torch.no_grad():
        mean, (Sd, _) = leg.insample_posterior(m, ts_all, xs_all, observed=observed)
    np.testing.assert_allclose(mean[where].cpu().numpy(), lm.cpu().numpy(), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(Sd[where].cpu().numpy(), lv.cpu().numpy(), rtol=1e-6, atol=1e-7)


@pytest.mark.gpu
def test_posterior_sample_is_the_sampler_on_the_same_system():
    case, _, _ = _dense_ref(5, 2, 64)
    p = [t.cuda() for t in case]
    m = leg.LEGMatrices(*p[:4])
    xs, ts = p[4], p[5]
    tt = torch.cat([ts[:1] - 0.7, (ts[20:29] + ts[21:30]) / 2, ts[-1:] + 1.3])       # before, between and after the data
    ts_all, xs_all, observed, where = leg.merge_targets(ts, xs, tt)
    observed = observed.unsqueeze(-1).expand(-1, 2)
    S, seed = 6, 1234
    z = leg.sample_from_posterior(m, ts_all, xs_all, S, seed, observed=observed)
    assert z.shape == (64 + 11, 5, S) and torch.isfinite(z).all()
    pattern, A_table, Li_table, _ = leg.observation_tables(m, observed)
    idx = pattern.long()
    xz = torch.where(observed, xs_all, torch.zeros_like(xs_all))
    v = ((xz.unsqueeze(1) @ Li_table[idx]).squeeze(1) @ m.B).contiguous()
    Rs, Os = leg.peg_precision(ts_all, m.G)
    dec, mean = cr.decompose_solve(Rs + A_table[idx], Os, v)
    assert torch.equal(z, cr.sample(dec, S, seed, mean=mean))


# ---- graph, errors ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_masked_log_likelihood_replays_from_a_graph():
    g, m, ts, xs = _load()
    masks = _golden_masks(ts.shape[0])
    obs = masks["rand30"].cuda()
    graphed = leg.Graphed(leg.log_likelihood, m, ts, xs, observed=obs)
    for _ in range(3):
        ll = float(graphed())
    ref = float(leg.log_likelihood(m, ts, xs, observed=obs))
    assert abs(ll - ref) <= 1e-10 * abs(ref)
    obs.copy_(masks["gap"].cuda())                               # a new mask in place: the replay follows
    ll2 = float(graphed())
    ref2 = float(leg.log_likelihood(m, ts, xs, observed=obs))
    assert abs(ll2 - ref2) <= 1e-10 * abs(ref2) and abs(ll2 - ll) > 1e-6


@pytest.mark.gpu
def test_zero_length_gap_and_coincident_target():
    case, mask, _ = _dense_ref(3, 3, 37)
    p = [t.cuda() for t in case]
    m = leg.LEGMatrices(*p[:4])
    ts = p[5].clone()
    ts[20] = ts[19]
    with pytest.raises(cr.NotPSDError):
        leg.log_likelihood(m, ts, p[4], observed=mask.cuda())
    with pytest.raises(ValueError):
        leg.merge_targets(p[5], p[4], p[5][7:8])
    ts_all, xs_all, observed, _ = leg.merge_targets(p[5], p[4], p[5][7:8], check=False)
    with pytest.raises(cr.NotPSDError):
        leg.log_likelihood(m, ts_all, xs_all, observed=observed)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [6, 8])
def test_block_sizes_without_a_fused_kernel_take_the_unfused_path(d):
    case, mask = mr.leg_case(d, 2, 20, 60 + d)
    Nm, Rm, Bm, Lm, xs, ts = case
    want = mr.leg_dense_loglik(Nm, Rm, Bm, Lm, ts, xs, mask)
    p = [t.cuda() for t in case]
    m = leg.LEGMatrices(*p[:4])
    assert not leg.fused_supported(p[5], m.G)
    with torch.no_grad():
        _check_value(leg.log_likelihood(m, p[5], p[4], observed=mask.cuda()), want, F64, "ll d=%d" % d)
    with pytest.raises(_hip.CgpsError):
        pattern, A_table, _, _ = leg.observation_tables(m, mask.cuda())
        leg.leg_loglik_reductions_obs(p[5], m.G, A_table, pattern, torch.zeros(20, d, dtype=F64, device="cuda"))

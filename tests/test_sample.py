"""Sampling on the GPU: the generator against the numpy restatement of its specification (tests/_rngref.py), and
cr.sample / the LEG sampling functions against the CPU oracle's back-substitution of that reference noise.

Tolerances: the generator's are those of tests/test_rng_spec.py (fp64 1e-13, fp32 1e-5: accurate libm calls differ by a
few ulp); everything that goes through the factor takes the project's for multi-column solves
(test_batched_right_hand_sides_against_oracle_columns): fp64 rtol 1e-9 atol 1e-10, fp32 rtol 3e-4 atol 3e-4."""
import numpy as np
import pytest
import torch

import _rngref
import _util
from oracle import cr_oracle as O
from cyclic_gps import _hip, leg
import cyclic_gps.cyclic_reduction as cr

pytestmark = pytest.mark.gpu

PAIRS = [(1, torch.float64), (2, torch.float64), (3, torch.float32), (4, torch.float64), (5, torch.float64), (8, torch.float32)]
PAIR_IDS = ["d1f64", "d2f64", "d3f32", "d4f64", "d5f64", "d8f32"]
SIZES = (1, 2, 5, 127, 128, 129, 257, 1000, 4097, 70001)
COUNTS = (1, 2, 3, 8, 11, 40)
SMALL_COUNTS = (1, 2, 3, 8)                                 # the larger counts at n <= 4097


def _np(t):
    return t.detach().cpu().numpy()


def _tol(dtype):
    return dict(rtol=1e-9, atol=1e-10) if dtype == torch.float64 else dict(rtol=3e-4, atol=3e-4)


def _npdt(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


def _levels(eps, n):
    """[n, d, S] in CRR order -> the per-level list the reference's backhalfsolve takes"""
    ms, offD, _, _ = _hip.level_layout(n)
    return [eps[offD[i]:offD[i + 1]] for i in range(len(ms))]


def _ref_noise(n, d, S, seed, stream, dtype):
    return torch.from_numpy(_rngref.standard_normal(n * d, S, seed, stream, _npdt(dtype))).reshape(n, d, S)


def _ref_samples(ref_dec, eps, mean):
    """mean + oracle.backhalfsolve(ref_dec, eps), column by column: [n, d, S] float64"""
    n = eps.shape[0]
    cols = [O.backhalfsolve(ref_dec, [lv[:, :, s] for lv in _levels(eps, n)]) for s in range(eps.shape[2])]
    return torch.stack(cols, dim=-1) + (0 if mean is None else mean.unsqueeze(-1))


# ---- the generator ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_standard_normal_against_the_specification(dtype):
    tol = 1e-13 if dtype == torch.float64 else 1e-5
    for rows in (1, 5, 70001):
        wide = cr.standard_normal(rows, 9, 2024, dtype=dtype)
        other_seed = cr.standard_normal(rows, 9, 2025, dtype=dtype)
        other_stream = cr.standard_normal(rows, 9, 2024, stream=1, dtype=dtype)
        for cols in (1, 2, 3, 5, 8, 9):
            z = cr.standard_normal(rows, cols, 2024, dtype=dtype)
            assert z.shape == (rows, cols) and z.dtype == dtype and z.is_cuda
            ref = _rngref.standard_normal(rows, cols, 2024, dtype=_npdt(dtype))
            err = float(np.abs(_np(z).astype(np.float64) - ref).max())
            print("rows %d cols %d %s: max |device - reference| = %.3g (bound %.0e)" % (rows, cols, dtype, err, tol))
            assert err <= tol, (rows, cols, err)
            assert torch.equal(z, wide[:, :cols]), (rows, cols)          # bitwise: a column never depends on cols
        for other in (other_seed, other_stream):
            assert bool((other != wide).any(dim=1).all())                 # every row changes
    ref1 = _rngref.standard_normal(5, 9, 77, stream=1, dtype=_npdt(dtype))
    assert float(np.abs(_np(cr.standard_normal(5, 9, 77, stream=1, dtype=dtype)).astype(np.float64) - ref1).max()) <= tol
    big = (1 << 63) + 12345                                               # a seed that needs all 64 bits
    refb = _rngref.standard_normal(5, 9, big, dtype=_npdt(dtype))
    assert float(np.abs(_np(cr.standard_normal(5, 9, big, dtype=dtype)).astype(np.float64) - refb).max()) <= tol


# ---- samples against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dtype", PAIRS, ids=PAIR_IDS)
def test_sample_against_oracle_columns(d, dtype):
    """sample(dec, S, seed, mean) = mean + oracle.backhalfsolve(ref_dec, eps) column by column, eps the reference noise
    in CRR layout; the same against cr.backhalfsolve of the device's own noise; and the noise is prefix-stable.  Sizes
    around the panel tiles (128 / 256 / 512 rows), several passes, ragged tiles, one to five column chunks."""
    tol = _tol(dtype)
    for n in SIZES:
        counts = COUNTS if n <= 4097 else SMALL_COUNTS
        smax, seed = max(counts), 1000 + n
        Rs, Os, _, mean, _ = _util.conditioned_system(n, d, seed=31 + n)
        ref_dec = O.decompose(Rs, Os)
        dec = cr.decompose(Rs.to(dtype).cuda(), Os.to(dtype).cuda())
        ref = _np(_ref_samples(ref_dec, _ref_noise(n, d, smax, seed, 0, dtype), mean))     # column s does not depend on S
        for S in counts:
            X = cr.sample(dec, S, seed, mean=mean.to(dtype).cuda())
            assert X.shape == (n, d, S) and X.dtype == dtype and X.is_cuda
            np.testing.assert_allclose(_np(X).astype(np.float64), ref[:, :, :S], err_msg="n=%d S=%d" % (n, S), **tol)
            eps_dev = cr.standard_normal(n * d, S, seed, dtype=dtype).reshape(n, d, S)
            comp = cr.backhalfsolve(dec, _levels(eps_dev, n)) + mean.to(dtype).cuda().unsqueeze(-1)
            np.testing.assert_allclose(_np(X), _np(comp), err_msg="n=%d S=%d (composition)" % (n, S), **tol)
        if smax == 40:
            np.testing.assert_allclose(_np(cr.sample(dec, 40, seed, mean=mean.to(dtype).cuda())[:, :, :3]),
                                       _np(cr.sample(dec, 3, seed, mean=mean.to(dtype).cuda())), **tol)
        # no mean; another stream is other noise
        X0 = cr.sample(dec, 3, seed)
        np.testing.assert_allclose(_np(X0).astype(np.float64), ref[:, :, :3] - _np(mean)[:, :, None], err_msg="n=%d no mean" % n, **tol)
        ref5 = _np(_ref_samples(ref_dec, _ref_noise(n, d, 2, seed, 5, dtype), None))
        np.testing.assert_allclose(_np(cr.sample(dec, 2, seed, stream=5)).astype(np.float64), ref5, err_msg="n=%d stream" % n, **tol)


def test_sample_more_columns_than_one_launch_group():
    """1100 samples: 138 eight-column chunks, more than the 128 of one launch; column s is still column s."""
    n, d = 300, 2
    Rs, Os, _, mean, _ = _util.conditioned_system(n, d, seed=3)
    dec = cr.decompose(Rs.cuda(), Os.cuda())
    X = cr.sample(dec, 1100, 9, mean=mean.cuda())
    eps = _ref_noise(n, d, 1100, 9, 0, torch.float64)
    pick = [0, 7, 8, 1023, 1024, 1031, 1032, 1099]
    ref = _ref_samples(O.decompose(Rs, Os), eps[:, :, pick], mean)
    np.testing.assert_allclose(_np(X[:, :, pick]), _np(ref), **_tol(torch.float64))
    np.testing.assert_allclose(_np(X[:, :, :40]), _np(cr.sample(dec, 40, 9, mean=mean.cuda())), **_tol(torch.float64))


def test_sample_from_cpu_factor_returns_cpu():
    Rs, Os, _, mean, _ = _util.conditioned_system(40, 3, seed=4)
    X = cr.sample(cr.decompose(Rs, Os), 5, 11, mean=mean)
    assert X.device.type == "cpu" and X.shape == (40, 3, 5)
    ref = _ref_samples(O.decompose(Rs, Os), _ref_noise(40, 3, 5, 11, 0, torch.float64), mean)
    np.testing.assert_allclose(_np(X), _np(ref), **_tol(torch.float64))


# ---- covariance ---------------------------------------------------------------------------------------------------
def _dense(Rs, Os):
    n, d = Rs.shape[0], Rs.shape[1]
    J = torch.zeros(n * d, n * d, dtype=torch.float64)
    for i in range(n):
        J[i * d:(i + 1) * d, i * d:(i + 1) * d] = Rs[i]
        if i + 1 < n:
            J[(i + 1) * d:(i + 2) * d, i * d:(i + 1) * d] = Os[i]
            J[i * d:(i + 1) * d, (i + 1) * d:(i + 2) * d] = Os[i].T
    return J


def test_covariance_exact():
    """The 192 unit vectors in place of the noise, through the test-side composition: W W^T = J^-1 on the band."""
    n, d = 64, 3
    Rs, Os, _, _, _ = _util.conditioned_system(n, d)
    dec = cr.decompose(Rs.cuda(), Os.cuda())
    eye = torch.eye(n * d, dtype=torch.float64, device="cuda").reshape(n, d, n * d)
    W = cr.backhalfsolve(dec, _levels(eye, n)).reshape(n * d, n * d).cpu()
    C = W @ W.T
    Sd, So = O.inverse_blocks(O.decompose(Rs, Os))
    tol = _tol(torch.float64)
    for i in range(n):
        np.testing.assert_allclose(C[i * d:(i + 1) * d, i * d:(i + 1) * d].numpy(), Sd[i].numpy(), **tol)
        if i + 1 < n:
            np.testing.assert_allclose(C[(i + 1) * d:(i + 2) * d, i * d:(i + 1) * d].numpy(), So[i].numpy(), **tol)
    np.testing.assert_allclose(C.numpy(), torch.linalg.inv(_dense(Rs, Os)).numpy(), **tol)


def test_covariance_sampled():
    """Fixed seed, deterministic: every entry of the sample covariance of 4096 draws within six standard errors of
    J^-1 (Var of a product of two jointly normal variables: C_ii C_jj + C_ij^2), every entry of the sample mean within
    six of zero.  The numpy reference noise alone gives 3.99 of the 6 (covariance) and 2.5 (mean)."""
    n, d, S = 64, 3, 4096
    Rs, Os, _, _, _ = _util.conditioned_system(n, d)
    dec = cr.decompose(Rs.cuda(), Os.cuda())
    X = cr.sample(dec, S, 2024).reshape(n * d, S).cpu().to(torch.float64)
    C = torch.linalg.inv(_dense(Rs, Os))
    Chat = X @ X.T / S
    dg = torch.diagonal(C)
    se = torch.sqrt((dg[:, None] * dg[None, :] + C * C) / S)
    worst = float(((Chat - C).abs() / se).max())
    worst_mean = float((X.mean(dim=1).abs() / torch.sqrt(dg / S)).max())
    print("covariance: worst entry %.2f standard errors; mean: %.2f (bound 6)" % (worst, worst_mean))
    assert worst <= 6.0, worst
    assert worst_mean <= 6.0, worst_mean


# ---- LEG ----------------------------------------------------------------------------------------------------------
# Through the factor of a LEG precision (blocks of exp(-dt G / 2), far worse conditioned than conditioned_system) the
# bound is the project's for the LEG in-sample posterior against the reference (tests/test_leg.py: rtol 1e-7, atol
# 1e-9): the same operation, a sweep through that factor, on operands assembled by two different codes (the oracle
# gets the blocks of the CPU assembly, the device assembles its own with cgps_peg_precision).
LEG_TOL = dict(rtol=1e-7, atol=1e-9)


def _leg_model(device, dtype=torch.float64):
    import os
    g = np.load(os.path.join(_util.GOLDEN, "leg_small_irregular.npz"))
    t = lambda k: torch.from_numpy(g[k]).to(dtype).to(device)   # noqa: E731
    return leg.LEGMatrices(t("N"), t("R"), t("B"), t("Lambda")), t("ts"), t("xs")


def test_leg_sample_from_posterior():
    m, ts, xs = _leg_model("cuda")
    mc, tsc, _ = _leg_model("cpu")
    n, rank, S, seed = ts.shape[0], m.N.shape[0], 11, 321
    z = leg.sample_from_posterior(m, ts, xs, S, seed)
    assert z.shape == (n, rank, S) and z.is_cuda and not z.requires_grad
    mean = leg.insample_posterior(m, ts, xs)[0].cpu()
    K_Rs, K_Os = leg.posterior_precision(mc, tsc)           # CPU tensors: batched torch ops, no kernel
    ref = _ref_samples(O.decompose(K_Rs, K_Os), _ref_noise(n, rank, S, seed, 0, torch.float64), mean)
    np.testing.assert_allclose(_np(z), _np(ref), **LEG_TOL)


def test_leg_sample_from_prior():
    m, ts, _ = _leg_model("cuda")
    mc, tsc, _ = _leg_model("cpu")
    n, rank, obs, S, seed = ts.shape[0], m.N.shape[0], m.B.shape[0], 9, 77
    z, x = leg.sample_from_prior(m, ts, S, seed)
    assert z.shape == (n, rank, S) and x.shape == (n, obs, S)
    Rs, Os = leg.peg_precision(tsc, mc.G)
    ref_z = _ref_samples(O.decompose(Rs, Os), _ref_noise(n, rank, S, seed, 0, torch.float64), None)
    np.testing.assert_allclose(_np(z), _np(ref_z), **LEG_TOL)
    eps1 = _ref_noise(n, obs, S, seed, 1, torch.float64)
    ref_x = torch.einsum("or,nrs->nos", mc.B, z.cpu()) + torch.einsum("op,nps->nos", mc.Lambda, eps1)
    np.testing.assert_allclose(_np(x), _np(ref_x), **_tol(torch.float64))
    # the observation noise is its own stream: not the latent noise again
    np.testing.assert_allclose(_np(leg.sample_observations(m, z, seed)), _np(x), rtol=0, atol=0)
    assert not np.allclose(_np(leg.sample_observations(m, z, seed, stream=2)), _np(x))


# ---- scale and HIP graph ------------------------------------------------------------------------------------------
def test_sample_at_scale_against_the_composition():
    n, d, S, seed = 2 ** 20, 4, 8, 5
    Rs, Os, _, mean, _ = _util.conditioned_system(n, d, device="cuda")
    dec = cr.decompose(Rs, Os)
    X = cr.sample(dec, S, seed, mean=mean)
    eps = cr.standard_normal(n * d, S, seed).reshape(n, d, S)
    comp = cr.backhalfsolve(dec, _levels(eps, n)) + mean.unsqueeze(-1)
    tol = _tol(torch.float64)
    assert bool(((X - comp).abs() <= tol["atol"] + tol["rtol"] * comp.abs()).all())
    assert float(X.std()) > 0.1


def test_sample_in_a_hip_graph():
    """Linear capture (no parallel branches), in the pattern of tests/test_hip_graphs.py: the replay is bitwise the
    eager call."""
    n, d, S = 70001, 4, 11
    Rs, Os, _, mean, _ = _util.conditioned_system(n, d, seed=2, device="cuda")
    dec = cr.decompose(Rs, Os)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                # warm-up off the default stream, as capture requires
        for _ in range(2):
            cr.sample(dec, S, 42, mean=mean)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = cr.sample(dec, S, 42, mean=mean)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, cr.sample(dec, S, 42, mean=mean))

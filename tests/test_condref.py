"""Checks of the checker of test_range_conditioning.py (tests/_condref.py); no GPU.

The long-double truth against dense fp64 numpy on well-conditioned systems and against 40-digit mpmath on one
ill-conditioned system of each family; the iterative condition number against the dense one; the conditions every case
of the GPU module rests on (positive definite after rounding, for the truth and for the CPU oracle in the kernel's dtype,
unscaled and scaled); and the oracle's pooled errors, i.e. the bounds the kernels get, printed (pytest -s)."""
import numpy as np
import pytest
import torch

import _condref as C
from oracle import cr_oracle

DTYPES = ("float64", "float32")


@pytest.mark.parametrize("n,d", [(1, 1), (1, 4), (2, 3), (7, 5), (33, 1), (33, 4), (33, 6), (25, 8)])
def test_truth_matches_dense_fp64_on_well_conditioned_systems(n, d):
    assert n * d <= 200
    Rs, Os, b = C.make_case(("float64", "block", 0, n, d))
    t = C.truth(Rs, Os, b)
    J = cr_oracle.dense_from_blocks(Rs, Os)
    x = np.linalg.solve(J, b.reshape(n * d, -1)).reshape(b.shape)
    sign, ld = np.linalg.slogdet(J)
    S = np.linalg.inv(J).reshape(n, d, n, d)
    assert sign == 1.0
    rel = lambda a, ref: float(np.abs(a - ref).max() / np.abs(ref).max())   # noqa: E731
    assert rel(t["x"].astype(np.float64), x) <= 1e-13
    assert abs(float(t["logdet"]) - ld) <= 1e-13 * max(abs(ld), 1.0)
    assert rel(t["mahal"].astype(np.float64), np.einsum("ndm,ndm->m", b, x)) <= 1e-13
    Sd = np.stack([S[i, :, i, :] for i in range(n)])
    assert rel(t["Sd"].astype(np.float64), Sd) <= 1e-13
    if n > 1:
        So = np.stack([S[i + 1, :, i, :] for i in range(n - 1)])
        assert float(np.abs(t["So"].astype(np.float64) - So).max()) <= 1e-13 * np.abs(Sd).max()
    one = C.truth(Rs, Os, b[:, :, 0])                       # a single right-hand side: the same numbers, without the axis
    assert np.array_equal(one["x"], t["x"][:, :, 0])
    assert abs(one["mahal"] - t["mahal"][0]) <= 4 * np.finfo(C.LD).eps * t["mahal"][0]      # (another order of one sum)


@pytest.mark.parametrize("key", [("float64", "block", 2, 9, 3), ("float64", "chain", 2, 40, 2)], ids=str)
def test_truth_matches_mpmath_on_an_ill_conditioned_system(key):
    """The truth's own error is eps(long double) * cond, a few thousand times below the u * cond the kernels are measured
    in; bound here: n d eps(long double) cond, relative, for x, mahal and the inverse blocks, absolute n d eps cond for
    the log-determinant."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    n, d = key[3], key[4]
    Rs, Os, b = C.make_case(key)
    t = C.truth(Rs, Os, b[:, :, 0])
    J = cr_oracle.dense_from_blocks(Rs, Os)
    cond = C.cond2_dense(Rs, Os)
    assert cond > 1e3
    tol = n * d * float(np.finfo(C.LD).eps) * cond
    assert tol <= 0.05 * np.finfo(np.float64).eps * cond       # far below one unit of the fp64 measure

    def exact(v):                      # a long double as an mpf, without loss: its fp64 head and the remainder
        v = C.LD(v)
        return mp.mpf(float(v)) + mp.mpf(float(v - C.LD(float(v))))

    Jm = mp.matrix(J.tolist())
    L = mp.cholesky(Jm)
    Si = mp.inverse(Jm)
    xm = Si * mp.matrix([float(v) for v in b[:, :, 0].reshape(-1)])
    xs = t["x"].reshape(-1)
    assert max(abs(exact(xs[i]) - xm[i]) for i in range(n * d)) <= tol * max(abs(v) for v in xm)
    ldm = 2 * sum(mp.log(L[i, i]) for i in range(n * d))
    assert abs(exact(t["logdet"]) - ldm) <= tol
    mm = sum(xm[i] * mp.mpf(float(b[:, :, 0].reshape(-1)[i])) for i in range(n * d))
    assert abs(exact(t["mahal"]) - mm) <= tol * mm
    smax = max(abs(Si[i, i]) for i in range(n * d))
    worst = 0
    for r in range(n):
        for i in range(d):
            for j in range(d):
                worst = max(worst, abs(exact(t["Sd"][r, i, j]) - Si[r * d + i, r * d + j]))
                if r + 1 < n:
                    worst = max(worst, abs(exact(t["So"][r, i, j]) - Si[(r + 1) * d + i, r * d + j]))
    assert worst <= tol * smax


@pytest.mark.parametrize("dtype,n,d", [("float64", 257, 5), ("float32", 257, 3), ("float64", 33, 8), ("float32", 33, 1),
                                       ("float64", 257, 1), ("float32", 257, 7)])
def test_iterative_condition_number_within_5_percent_of_dense(dtype, n, d):
    assert n * d <= C.DENSE_COND_MAX
    for key in C.keys_of_shape(dtype, n, d):
        Rs, Os, _ = C.make_case(key)
        dense, it = C.cond2_dense(Rs, Os), C.cond2_iterative(Rs, Os)
        print(key, "dense %.6g iterative %.6g" % (dense, it))
        assert abs(it - dense) <= 0.05 * dense, (key, dense, it)


def test_shapes_reach_the_paths_they_are_chosen_for():
    """4097 rows (8193 at fp32 d = 8) are more than one stage-1 workgroup of the fused reduction: 256 rows per workgroup
    below 65 536 rows, tile_rows1 rows where several lanes share a row (csrc/cgps_plan.h; tests/test_plan.py pins that
    header).  The batched kernel takes systems of up to BATCH_MAX_ROWS rows."""
    tile_rows1 = {("float32", 8): 128 * 256 // 4, ("float64", 8): 64 * 256 // 4, ("float64", 6): 32 * 256 // 2}
    for dt in DTYPES:
        for d in range(1, 9):
            for n in C.large_ns(dt, d)[1:]:
                assert n > tile_rows1.get((dt, d), 256) and n - 1 <= tile_rows1.get((dt, d), 4096)
        assert {n for n, _ in C.shapes(dt)} >= {33, 257, 1025}
        assert [k for k in C.all_keys(dt) if k[4] == 1 and k[1] == "block"] == [(dt, "block", 0, n, 1) for n in (33, 257)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_case_is_positive_definite_and_the_oracle_sets_a_bound(dtype):
    """Every case of the GPU module: the rounded system factors in long double and in the CPU oracle at the kernel's
    dtype (shape_cases raises otherwise: no case is dropped), its condition number is finite, and the oracle's pooled
    measures -- a quarter of what the kernels are allowed -- are printed."""
    for (n, d) in C.shapes(dtype):
        for key, c in C.shape_cases(dtype, n, d).items():
            assert np.isfinite(c["cond"]) and c["cond"] >= 1.0, key
            assert all(np.isfinite(v) for v in c["oracle"].values()), (key, c["oracle"])
    pooled = C.pooled(dtype)
    print("\noracle's pooled worst measures, %s (units of u cond; the kernels' bound is 4 x):" % dtype)
    for fam in C.FAMILIES:
        for lv in range(3):
            print("  %-6s %-8g " % (fam, C.LEVELS[dtype][fam][lv])
                  + "  ".join("%s %.4g" % (q, pooled[(fam, lv, q)]) for q in C.QUANTITIES))
    assert set(pooled) == {(f, lv, q) for f in C.FAMILIES for lv in range(3) for q in C.QUANTITIES}
    assert all(0.0 < v < float("inf") for v in pooled.values())
    # u * cond < 1 on every case: a measure of order 1 is still a small error
    assert max(c["cond"] for (n, d) in C.shapes(dtype) for c in C.shape_cases(dtype, n, d).values()) * C.eps_of(dtype) < 0.1


def _scale_params():
    out = []
    for dt in DTYPES:
        for (n, d) in C.scale_shapes(dt):
            out += [(dt, n, d, k) for k in C.SCALES[dt]]
    return out + [key + (k,) for key, ks in C.BEYOND.items() for k in ks]


@pytest.mark.parametrize("dtype,n,d,k", _scale_params())
def test_oracle_stays_finite_and_accurate_under_scaling(dtype, n, d, k):
    """The scaling is exact, the scaled system factors, and the oracle in the kernel's dtype gives the measures of k = 0
    to the last bit; its log-determinant, a sum that grows by n d k log 2, is within the bound the kernels get
    (_condref.bound(..., scaled=True)), also at the scales beyond those that bound looks at."""
    key = C.scale_key(dtype, n, d)
    c = C.case(key)
    Rs, Os = C.scaled(c["Rs"], c["Os"], k)
    back = C.scaled(Rs, Os, -k)
    assert np.array_equal(back[0], c["Rs"]) and np.array_equal(back[1], c["Os"])
    t = C.scaled_truth(c["truth"], n, d, k)
    got = C.oracle_measures(Rs, Os, c["b"], t, c["cond"])           # raises when not positive definite or not finite
    for q, v in got.items():
        print(key, k, q, "%.4g (k = 0: %.4g, bound %.4g)" % (v, c["oracle"][q], C.bound(key, q, scaled=True)))
        assert v <= C.bound(key, q, scaled=True), (key, k, q, v)
        if q != "logdet" and k in C.SCALES[dtype]:       # a power of two changes nothing but the exponents
            assert v == c["oracle"][q], (key, k, q, v, c["oracle"][q])


@pytest.mark.parametrize("dtype", DTYPES)
def test_which_scaled_cases_need_a_log_det_bound_of_their_own(dtype):
    """The log-determinant of a scaled case keeps the k = 0 bound of its group unless the oracle itself misses it on the
    scaled inputs.  fp64: the oracle misses it at d = 1 only (cond 11, |l*| = n d k log 2 is 7 x n d cond at k = 120)
    and is 10 to 100 times below it from d = 2 on (kappa = 1e6: n d cond is 1e4 x |l*|).  fp32 (results returned in
    fp32, cond ~200): d = 1 and whichever others the rounding of |l*| takes over.  No relaxed bound exceeds 4 x one
    rounding of the result."""
    need = {}
    for (n, d) in C.scale_shapes(dtype):
        key = C.scale_key(dtype, n, d)
        need[(n, d)] = C.needs_scaled_logdet_bound(key)
        k0 = 4 * C.pooled(dtype)[(key[1], key[2], "logdet")]
        print(key, "oracle's worst scaled %.4g, k = 0 bound %.4g, own bound: %s" % (C.scaled_logdet_worst(key), k0, need[(n, d)]))
        assert C.scaled_logdet_worst(key) <= 1.0
        assert C.bound(key, "logdet", scaled=True) == (4 * C.scaled_logdet_worst(key) if need[(n, d)] else k0)
    assert need[(257, 1)]
    if dtype == "float64":
        assert [nd for nd, v in need.items() if v] == [(257, 1)]
        assert all(C.scaled_logdet_worst(C.scale_key(dtype, n, d)) <= 0.1 * C.bound(C.scale_key(dtype, n, d), "logdet")
                   for (n, d) in need if d > 1)


def test_scaled_truth_is_the_truth_of_the_scaled_system():
    key = ("float64", "block", 1, 33, 5)
    Rs, Os, b = C.make_case(key)
    t0 = C.truth(Rs, Os, b)
    for k in (-160, 120):
        ts, tk = C.scaled_truth(t0, 33, 5, k), C.truth(*C.scaled(Rs, Os, k), b)
        for q in ("x", "mahal", "Sd", "So"):
            assert np.array_equal(ts[q], tk[q]), (k, q)
        assert abs(ts["logdet"] - tk["logdet"]) <= 4 * np.finfo(C.LD).eps * abs(tk["logdet"])


def test_truth_refuses_a_system_that_is_not_positive_definite():
    Rs, Os, b = C.make_case(("float64", "chain", 0, 33, 2))
    Rs = Rs.copy()
    Rs[17] *= 0.1
    with pytest.raises(C.NotPositiveDefinite):
        C.truth(Rs, Os, b)
    with pytest.raises(cr_oracle.NotPSDError):
        cr_oracle.decompose(torch.from_numpy(Rs), torch.from_numpy(Os))

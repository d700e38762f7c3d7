"""Inputs and a truth for tests of accuracy across scale and conditioning (test_condref.py, test_range_conditioning.py).

Two seeded families of SPD block-tridiagonal systems J = L L^T, L block lower bidiagonal with diagonal blocks Ld and
sub-diagonal blocks Lo (the construction of _util.conditioned_system):

  block(n, d, kappa)   Ld_i = Q1 diag(sigma) Q2^T, sigma log-spaced from 1 to kappa^-1/2, Lo_i = 0.3/sqrt(d) randn sigma_min:
                       the conditioning sits inside the blocks (none at d = 1: only kappa = 1 there)
  chain(n, d, rho)     Ld_i orthogonal, Lo_i = -rho Q_i Ld_i: R_i = (1 + rho^2) I, O_i = -rho Q_i, a block version of the
                       AR(1) precision; the conditioning sits in the coupling, where the Schur complements
                       R - F F^T - G G^T of cyclic reduction cancel; cond ~ min(4 / (1 - rho)^2, n^2)

The arrays are rounded to the kernel's dtype FIRST: the rounded arrays are the problem that the truth, the CPU oracle
and the kernels all solve.  truth() is block Thomas in np.longdouble (64-bit mantissa) with hand-written d x d
Cholesky and substitutions; cond2() is the 2-norm condition number of the rounded system; m_*() are the error
measures of DESIGN.md 2.1, in units of u * cond, which the GPU module bounds by 4 x the CPU oracle's own.
"""
import functools

import numpy as np
import torch

from oracle import cr_oracle

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "np.longdouble has no 64-bit mantissa here: the truth would be no better than fp64"

NRHS = 8                     # right-hand-side columns of every case; column 0 is "the" right-hand side
FAMILIES = ("block", "chain")
LEVELS = {
    "float64": {"block": (1.0, 1e6, 1e12), "chain": (0.9, 0.999, 0.99999)},
    "float32": {"block": (1.0, 1e2, 1e4), "chain": (0.9, 0.99, 0.995)},
}
SCALES = {"float64": (-120, -60, 60, 120), "float32": (-56, -28, 28, 56)}
QUANTITIES = ("solve", "mahal", "inv_diag", "inv_off", "logdet")
DENSE_COND_MAX = 2048        # n * d up to which cond2 is a dense eigvalsh


class NotPositiveDefinite(ArithmeticError):
    pass


# ----------------------------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------------------------
def large_ns(dtype, d):
    """The two large sizes of a (dtype, d) that has them: 1025 (eight rows per lane, one stage-1 workgroup) and the first
    size with several stage-1 workgroups, hence record stages.  A stage-1 workgroup takes 256 rows below 65 536 rows
    (stage1_rows_per_lane gives 1 row per lane), except where several lanes share a row and the tile is always
    tile_rows1 (csrc/cgps_plan.h): 4096 rows at fp64 d = 8 and d = 6, 8192 rows at fp32 d = 8.  4097 reaches a second
    workgroup for all but fp32 d = 8, which takes 8193."""
    if d in (4, 5, 8) or (d == 6 and dtype == "float64"):
        return (1025, 8193 if (dtype == "float32" and d == 8) else 4097)
    return ()


def shapes(dtype):
    """[(n, d)] of a dtype: n in {33, 257} for every d, the large sizes for d in {4, 5, 8} and fp64 d = 6."""
    out = []
    for d in range(1, 9):
        out += [(n, d) for n in (33, 257) + large_ns(dtype, d)]
    return out


def level_ids(family, d):
    """Level indices of a family at block size d: a 1 x 1 block has no conditioning inside it."""
    return (0,) if (family == "block" and d == 1) else (0, 1, 2)


def keys_of_shape(dtype, n, d):
    return [(dtype, fam, lv, n, d) for fam in FAMILIES for lv in level_ids(fam, d)]


def all_keys(dtype):
    return [k for (n, d) in shapes(dtype) for k in keys_of_shape(dtype, n, d)]


def scale_key(dtype, n, d):
    """The mid-conditioned case of a (dtype, n, d) that the scale tests multiply by 2^k."""
    return (dtype, "block", 0 if d == 1 else 1, n, d)


def scale_shapes(dtype):
    return [(257, d) for d in range(1, 9)] + [(4097, 5), (large_ns(dtype, 8)[1], 8)]


def _orth(rng, n, d):
    q, r = np.linalg.qr(rng.standard_normal((n, d, d)))
    return q * np.sign(np.diagonal(r, axis1=-2, axis2=-1))[:, None, :]


def _assemble(Ld, Lo, dtype):
    Rs = Ld @ Ld.transpose(0, 2, 1)
    Rs[1:] += Lo @ Lo.transpose(0, 2, 1)
    Rs = 0.5 * (Rs + Rs.transpose(0, 2, 1))
    Os = Lo @ Ld[:-1].transpose(0, 2, 1)
    return np.ascontiguousarray(Rs.astype(dtype)), np.ascontiguousarray(Os.astype(dtype))


def block(n, d, kappa, dtype, rng):
    assert d > 1 or kappa == 1.0
    sigma = np.logspace(0.0, -0.5 * np.log10(kappa), d)
    Ld = (_orth(rng, n, d) * sigma) @ _orth(rng, n, d).transpose(0, 2, 1)
    Lo = (0.3 / d ** 0.5) * sigma[-1] * rng.standard_normal((n - 1, d, d))
    return _assemble(Ld, Lo, dtype)


def chain(n, d, rho, dtype, rng):
    Ld = _orth(rng, n, d)
    Lo = -rho * _orth(rng, n - 1, d) @ Ld[:-1]
    return _assemble(Ld, Lo, dtype)


def make_case(key):
    """(Rs [n, d, d], Os [n-1, d, d], b [n, d, NRHS]) of a case key, numpy arrays in the key's dtype."""
    dtype, fam, lv, n, d = key
    rng = np.random.default_rng([FAMILIES.index(fam), lv, n, d])
    Rs, Os = (block if fam == "block" else chain)(n, d, LEVELS[dtype][fam][lv], dtype, rng)
    b = np.ascontiguousarray(rng.standard_normal((n, d, NRHS)).astype(dtype))
    return Rs, Os, b


def scaled(Rs, Os, k):
    """(Rs, Os) times 2^k: exact while nothing leaves the dtype's normal range."""
    return np.ldexp(Rs, k), np.ldexp(Os, k)


# ----------------------------------------------------------------------------------------------------------------
# the truth: block Thomas in long double, batched over a leading axis of systems of one shape
# ----------------------------------------------------------------------------------------------------------------
def _chol_ld(A):
    """Lower Cholesky factor of the lower triangle of A [..., d, d] (long double), column by column."""
    d = A.shape[-1]
    L = np.zeros_like(A)
    for j in range(d):
        s = A[..., j, j] - (L[..., j, :j] ** 2).sum(-1)
        if not np.all(s > 0):
            raise NotPositiveDefinite("pivot %d not positive" % j)
        L[..., j, j] = np.sqrt(s)
        if j + 1 < d:
            t = A[..., j + 1:, j] - (L[..., j + 1:, :j] * L[..., j:j + 1, :j]).sum(-1)
            L[..., j + 1:, j] = t / L[..., j, j][..., None]
    return L


def _fwd_ld(L, X):
    """L^-1 X by forward substitution; X [..., d, k]."""
    Y = np.empty_like(X)
    for j in range(L.shape[-1]):
        Y[..., j, :] = (X[..., j, :] - (L[..., j, :j, None] * Y[..., :j, :]).sum(-2)) / L[..., j, j][..., None]
    return Y


def _t(A):
    return np.swapaxes(A, -1, -2)


def truth_many(Rs, Os, b):
    """Truth of B systems of one shape: Rs [B, n, d, d], Os [B, n-1, d, d], b [B, n, d, m] (any float dtype).
    Returns long-double arrays: x [B, n, d, m] = J^-1 b, logdet [B] (a sum of logs of pivots), mahal [B, m] = b^T J^-1 b
    per column, Sd [B, n, d, d] and So [B, n-1, d, d], the diagonal and lower off-diagonal blocks of J^-1.

    With S_0 = R_0, L_i = chol(S_i), W_i = O_i L_i^-T, S_i+1 = R_i+1 - W_i W_i^T:  z_i = L_i^-1 (b_i - W_i-1 z_i-1),
    x_i = L_i^-T (z_i - W_i^T x_i+1), and with K_i = S_i^-1 O_i^T:  Sig_ii = S_i^-1 + K_i Sig_i+1,i+1 K_i^T,
    Sig_i+1,i = -Sig_i+1,i+1 K_i^T."""
    R, O, c = (np.asarray(a).astype(LD) for a in (Rs, Os, b))
    B, n, d, m = c.shape
    eye = np.broadcast_to(np.eye(d, dtype=LD), (B, d, d))
    Linv = np.empty((B, n, d, d), LD)
    Wt = np.empty((B, max(n - 1, 0), d, d), LD)
    z = np.empty((B, n, d, m), LD)
    logdet = np.zeros(B, LD)
    S, ci = R[:, 0], c[:, 0]
    for i in range(n):
        L = _chol_ld(S)
        logdet += 2 * np.log(np.diagonal(L, axis1=-2, axis2=-1)).sum(-1)
        last = i == n - 1
        Y = _fwd_ld(L, np.concatenate([eye, ci] if last else [eye, ci, _t(O[:, i])], axis=-1))
        Linv[:, i], z[:, i] = Y[..., :d], Y[..., d:d + m]
        if not last:
            Wt[:, i] = Y[..., d + m:]
            S = R[:, i + 1] - _t(Wt[:, i]) @ Wt[:, i]
            ci = c[:, i + 1] - _t(Wt[:, i]) @ z[:, i]
    x = np.empty_like(z)
    Sd = np.empty((B, n, d, d), LD)
    So = np.empty((B, max(n - 1, 0), d, d), LD)
    x[:, n - 1] = _t(Linv[:, n - 1]) @ z[:, n - 1]
    Sd[:, n - 1] = _t(Linv[:, n - 1]) @ Linv[:, n - 1]
    for i in range(n - 2, -1, -1):
        Li = Linv[:, i]
        x[:, i] = _t(Li) @ (z[:, i] - Wt[:, i] @ x[:, i + 1])
        K = _t(Li) @ Wt[:, i]
        SK = Sd[:, i + 1] @ _t(K)
        So[:, i] = -SK
        Sd[:, i] = _t(Li) @ Li + K @ SK
    return dict(x=x, logdet=logdet, mahal=(z * z).sum(axis=(1, 2)), Sd=Sd, So=So)


def truth(Rs, Os, b):
    """truth_many of one system; b [n, d] or [n, d, m]."""
    b = np.asarray(b)
    one = b.ndim == 2
    t = truth_many(np.asarray(Rs)[None], np.asarray(Os)[None], (b[..., None] if one else b)[None])
    t = {k: v[0] for k, v in t.items()}
    if one:
        t["x"], t["mahal"] = t["x"][..., 0], t["mahal"][0]
    return t


def scaled_truth(t, n, d, k):
    """The truth of the system times 2^k from the truth t of the system: exact, long double has the exponent range."""
    s = np.ldexp(LD(1), -k)
    return dict(x=t["x"] * s, mahal=t["mahal"] * s, Sd=t["Sd"] * s, So=t["So"] * s,
                logdet=t["logdet"] + LD(n * d * k) * np.log(LD(2)))


# ----------------------------------------------------------------------------------------------------------------
# the condition number
# ----------------------------------------------------------------------------------------------------------------
def _matvec(R, O, v):
    y = np.einsum("nij,nj->ni", R, v)
    y[1:] += np.einsum("nij,nj->ni", O, v[:-1])
    y[:-1] += np.einsum("nji,nj->ni", O, v[1:])
    return y


def _power(apply, shape, tol=1e-4, hold=4, max_it=300):
    """Largest eigenvalue of a symmetric positive definite operator by power iteration, reading off the best Rayleigh
    quotient of the iterates' span (Lanczos with full re-orthogonalisation: the same products A v, A^2 v, ..., and a
    value that is never below the plain iteration's, so far fewer products; the top of J^-1 for the block family is a
    cluster that the plain quotient crosses only in thousands of steps).  Stops when the value has moved by less than
    tol (relative) over `hold` consecutive steps."""
    v = np.random.default_rng(0).standard_normal(shape).reshape(-1)
    V = [v / np.linalg.norm(v)]
    alpha, beta = [], []
    lam, still = 0.0, 0
    for _ in range(max_it):
        w = np.asarray(apply(V[-1].reshape(shape))).reshape(-1)
        alpha.append(float(V[-1] @ w))
        Q = np.stack(V)
        w = w - Q.T @ (Q @ w)
        w = w - Q.T @ (Q @ w)
        k = len(alpha)
        T = np.diag(alpha) + np.diag(beta, 1) + np.diag(beta, -1) if k > 1 else np.array([[alpha[0]]])
        new = float(np.linalg.eigvalsh(T)[-1])
        still = still + 1 if abs(new - lam) <= tol * abs(new) else 0
        lam = new
        nw = float(np.linalg.norm(w))
        if still >= hold or nw <= 1e-13 * abs(lam):
            return lam
        beta.append(nw)
        V.append(w / nw)
    raise RuntimeError("the iteration for the largest eigenvalue did not settle in %d steps" % max_it)


def cond2_dense(Rs, Os):
    w = np.linalg.eigvalsh(cr_oracle.dense_from_blocks(np.asarray(Rs, np.float64), np.asarray(Os, np.float64)))
    return float(w[-1] / w[0])


def cond2_iterative(Rs, Os):
    """lambda_max(J) * lambda_max(J^-1): power iteration on J (block matvec) and on J^-1 (the fp64 oracle's solve)."""
    R, O = np.asarray(Rs, np.float64), np.asarray(Os, np.float64)
    dec = cr_oracle.decompose(torch.from_numpy(R), torch.from_numpy(O))
    top = _power(lambda v: _matvec(R, O, v), R.shape[:2])
    inv_top = _power(lambda v: cr_oracle.solve(dec, torch.from_numpy(v)).numpy(), R.shape[:2])
    return top * inv_top


def cond2(Rs, Os):
    """2-norm condition number of the (rounded) system, evaluated in fp64."""
    n, d = Rs.shape[0], Rs.shape[1]
    return cond2_dense(Rs, Os) if n * d <= DENSE_COND_MAX else cond2_iterative(Rs, Os)


# ----------------------------------------------------------------------------------------------------------------
# error measures, in units of u * cond
# ----------------------------------------------------------------------------------------------------------------
def eps_of(dtype):
    return float(np.finfo(np.dtype(dtype)).eps)


def _ld(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a).astype(LD)


def m_solve(x, t, cond, u, cols=slice(None)):
    """max|x - x*| / max|x*| / (u cond), the worst over the columns; x [n, d] or [n, d, m] against t["x"][..., cols]."""
    xs = t["x"][..., cols]
    xs = xs.reshape(xs.shape[0] * xs.shape[1], -1)
    x = _ld(x).reshape(xs.shape)
    return float((np.abs(x - xs).max(0) / np.abs(xs).max(0)).max() / (u * cond))


def m_mahal(m, t, cond, u, col=0):
    ms = t["mahal"][col]
    return float(abs(_ld(m) - ms) / ms / (u * cond))


def m_inv(Sd, So, t, cond, u):
    """(diagonal, off-diagonal) measures: max|Sig - Sig*| / max|Sig*_diag| / (u cond)."""
    ref = np.abs(t["Sd"]).max()
    return (float(np.abs(_ld(Sd) - t["Sd"]).max() / ref / (u * cond)),
            float(np.abs(_ld(So) - t["So"]).max() / ref / (u * cond)))


def m_logdet(ld, t, cond, u, n, d):
    """|l - l*| / (u (n d cond + |l*|)); inf for a result that is not finite."""
    ld = _ld(ld)
    if not np.isfinite(ld):
        return float("inf")
    return float(abs(ld - t["logdet"]) / (u * (n * d * cond + abs(t["logdet"]))))


def oracle_measures(Rs, Os, b, t, cond):
    """{quantity: the CPU oracle's worst measure} with the oracle run in the dtype of the arrays: the first and the
    last column of b solved, mahal and log-det by both of the oracle's routes (from the factor and by mahal_and_det)."""
    u = eps_of(Rs.dtype)
    n, d = Rs.shape[0], Rs.shape[1]
    R, O, B = torch.from_numpy(Rs), torch.from_numpy(Os), torch.from_numpy(b)
    dec = cr_oracle.decompose(R, O)
    cols = [0, B.shape[2] - 1]
    x = torch.stack([cr_oracle.solve(dec, B[:, :, c].contiguous()) for c in cols], dim=-1)
    m2, l2 = cr_oracle.mahal_and_det(R, O, B[:, :, 0].contiguous())
    m1, l1 = cr_oracle.mahal(dec, B[:, :, 0].contiguous()), cr_oracle.det(dec)
    Sd, So = cr_oracle.inverse_blocks(dec)
    vals = [x, m1, m2, l1, l2, Sd, So]
    if not all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in vals):
        raise FloatingPointError("the CPU oracle left the finite range")
    idg, iof = m_inv(Sd, So, t, cond, u)
    return dict(solve=m_solve(x, t, cond, u, cols), mahal=max(m_mahal(m1, t, cond, u), m_mahal(m2, t, cond, u)),
                inv_diag=idg, inv_off=iof,
                logdet=max(m_logdet(l1, t, cond, u, n, d), m_logdet(l2, t, cond, u, n, d)))


# ----------------------------------------------------------------------------------------------------------------
# cached per process: the cases of a shape with their truths, condition numbers and oracle measures; pooled bounds
# ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shape_cases(dtype, n, d):
    """{key: dict(Rs, Os, b, truth, cond, oracle)} of every case of a (dtype, n, d); one batched truth for all of them.
    Raises (never drops a case) when a system is not positive definite in long double or for the oracle."""
    keys = keys_of_shape(dtype, n, d)
    arrs = [make_case(k) for k in keys]
    tm = truth_many(np.stack([a[0] for a in arrs]), np.stack([a[1] for a in arrs]), np.stack([a[2] for a in arrs]))
    out = {}
    for i, (k, (Rs, Os, b)) in enumerate(zip(keys, arrs)):
        t = {q: v[i] for q, v in tm.items()}
        c = cond2(Rs, Os)
        out[k] = dict(Rs=Rs, Os=Os, b=b, truth=t, cond=c, oracle=oracle_measures(Rs, Os, b, t, c))
    return out


def case(key):
    return shape_cases(key[0], key[3], key[4])[key]


@functools.lru_cache(maxsize=None)
def pooled(dtype):
    """{(family, level, quantity): the oracle's worst measure over the group's (n, d) members} for a dtype."""
    out = {}
    for (n, d) in shapes(dtype):
        for k, c in shape_cases(dtype, n, d).items():
            for q, v in c["oracle"].items():
                g = (k[1], k[2], q)
                out[g] = max(out.get(g, 0.0), v)
    return out


BEYOND = {("float64", 257, 8): (160, -160, -131), ("float64", 257, 4): (260, -260)}
"""Scales at which a block's determinant is no normal double (fp64: d = 8 at 2^+-160 and, a denormal, at 2^-131;
d = 4 at 2^+-260), per (dtype, n, d) of the scale case they are tried on."""


def oracle_scaled_logdet(key, k):
    """The oracle's log-det measure (the worse of its two routes) on the case times 2^k, in the case's dtype."""
    c = case(key)
    n, d = key[3], key[4]
    R, O = (torch.from_numpy(a) for a in scaled(c["Rs"], c["Os"], k))
    b0 = torch.from_numpy(np.ascontiguousarray(c["b"][:, :, 0]))
    t = dict(logdet=c["truth"]["logdet"] + LD(n * d * k) * np.log(LD(2)))
    return max(m_logdet(ld, t, c["cond"], eps_of(key[0]), n, d)
               for ld in (cr_oracle.det(cr_oracle.decompose(R, O)), cr_oracle.mahal_and_det(R, O, b0)[1]))


@functools.lru_cache(maxsize=None)
def scaled_logdet_worst(key):
    """The oracle's worst log-det measure on the case over the scales 2^k of SCALES."""
    return max(oracle_scaled_logdet(key, k) for k in SCALES[key[0]])


def needs_scaled_logdet_bound(key, factor=4.0):
    """Whether the oracle itself misses the k = 0 log-det bound of the case's group on the scaled case.  Every other
    measure is unchanged by a power of two, for the oracle to the last bit.  The log-determinant grows by n d k log 2,
    and the rounding of a result of that size alone is up to 0.5 u |l*|: where |l*| outweighs n d cond (d = 1, cond 11;
    the low-cond fp32 cases, whose results are returned in fp32) that is above 4 x the group's pooled worst at k = 0,
    where n d cond outweighs |l*| (fp64 at kappa = 1e6) it is far below."""
    return scaled_logdet_worst(key) > factor * pooled(key[0])[(key[1], key[2], "logdet")]


def bound(key, quantity, factor=4.0, scaled=False):
    """What a kernel's measure may be on the case: factor x the oracle's pooled worst of the case's group.  The
    log-determinant of a scaled case keeps that bound wherever the oracle meets it on the scaled inputs; where the
    oracle does not (needs_scaled_logdet_bound), it is factor x the oracle's worst on this case's scaled inputs."""
    p = pooled(key[0])[(key[1], key[2], quantity)]
    if scaled and quantity == "logdet" and needs_scaled_logdet_bound(key, factor):
        p = scaled_logdet_worst(key)
    return factor * p

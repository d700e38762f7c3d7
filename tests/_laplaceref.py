"""A dense fp64 truth for the Laplace approximation of count, binary and Gaussian observations under a LEG prior
(leg.laplace_posterior_batch), in COVARIANCE form: Rasmussen & Williams, algorithm 3.1, on the
observed linear predictors f = H z with C_f = H Sigma H^T and Sigma from ``_gapref.prior_covariance``.  It shares
nothing with the library: no kernel, no precision block, not even the parametrisation (the library iterates on z with
the precision K; this iterates on f with the covariance).  torch ops on CPU tensors only.

    mode        z = Sigma H^T g(f)                                    (g = d log p / d f at the mode)
    covariance  Sigma - Sigma H^T W^1/2 (I + W^1/2 C_f W^1/2)^-1 W^1/2 H Sigma
    evidence    -1/2 a^T f + sum log p(y | f) - 1/2 log|I + W^1/2 C_f W^1/2|,  a = g(f) at the mode

The cases of tests/test_leg_laplace.py are drawn here too, so that tests/test_laplaceref.py can hold the truth to its own
checks on exactly the inputs the GPU tests use."""
import functools
import math

import torch

import _gapref

F64 = torch.float64
FAMILIES = ("poisson", "bernoulli", "gaussian")
TOL = 1e-13
MAX_ITER = 100


def log_p(family, y, eta, s=None):
    """log p(y | eta) per entry, every term included"""
    if family == "poisson":
        return y * eta - torch.exp(eta) - torch.lgamma(y + 1)
    if family == "bernoulli":
        return y * eta - torch.nn.functional.softplus(eta)
    return -0.5 * (y - eta) ** 2 / s - 0.5 * torch.log(2 * math.pi * s)


def grad_weight(family, y, eta, s=None):
    """(d log p / d eta, -d^2 log p / d eta^2) per entry"""
    if family == "poisson":
        e = torch.exp(eta)
        return y - e, e
    if family == "bernoulli":
        p = torch.sigmoid(eta)
        return y - p, p * (1 - p)
    return (y - eta) / s, 1.0 / s


def observation_map(Bm, mask):
    """H [m, n d]: row k is B[c, :] in the columns of row i, for the k-th observed entry (i, c) in row-major order"""
    n, obs = mask.shape
    d = Bm.shape[1]
    idx = torch.nonzero(mask)
    H = torch.zeros(idx.shape[0], n * d, dtype=F64)
    for k, (i, c) in enumerate(idx.tolist()):
        H[k, i * d:(i + 1) * d] = Bm[c]
    return H, idx


def truth(ts, G, Bm, ys, mask, family, offset=None, log_exposure=None, noise_var=None):
    """The Laplace approximation of one series: dict(mean [n, d], cov_diag [n, d, d], cov_off [n - 1, d, d] (the blocks
    [i + 1][i]), log_evidence, iterations, f, C, g, shift) -- f the observed linear predictors WITHOUT their shift (offset
    + log_exposure), C their prior covariance, g the gradient at the mode."""
    ts, G, Bm, ys = (t.to(F64) for t in (ts, G, Bm, ys))
    n, d = ts.shape[0], G.shape[0]
    Sigma = _gapref.prior_covariance(ts, G)
    H, idx = observation_map(Bm, mask)
    m = H.shape[0]
    y = ys[mask]
    shift = torch.zeros(m, dtype=F64)
    if offset is not None:
        shift = shift + offset.to(F64)[idx[:, 1]]
    if log_exposure is not None:
        shift = shift + log_exposure.to(F64)[mask]
    s = None if noise_var is None else noise_var.to(F64)[mask]
    C = H @ Sigma @ H.T
    eye = torch.eye(m, dtype=F64)
    if m == 0:                                                       # nothing observed: the prior
        cov, i = Sigma.reshape(n, d, n, d), torch.arange(n)
        return dict(mean=torch.zeros(n, d, dtype=F64), cov_diag=cov[i, :, i, :], cov_off=cov[i[1:], :, i[:-1], :],
                    log_evidence=0.0, iterations=1, f=y, C=C, g=y, shift=shift, H=H, Sigma=Sigma, y=y, s=s)

    def newton_system(f):
        g, W = grad_weight(family, y, f + shift, s)
        sW = W.sqrt()
        L = torch.linalg.cholesky(eye + sW[:, None] * C * sW[None, :])
        return g, W, sW, L

    f, a = torch.zeros(m, dtype=F64), torch.zeros(m, dtype=F64)
    obj = float(log_p(family, y, f + shift, s).sum())
    iterations = 0
    for iterations in range(1, MAX_ITER + 1):
        g, W, sW, L = newton_system(f)
        # the step of algorithm 3.1 as an increment: a_new - a = (I + W C)^-1 (g - a), which is line 7 of the algorithm
        # (a_new = b - W^1/2 B^-1 W^1/2 C b, b = W f + g) with f = C a taken out, so that the update's rounding error
        # scales with the residual g - a and not with f
        r = g - a
        da = r - sW * torch.cholesky_solve((sW * (C @ r)).unsqueeze(-1), L).squeeze(-1)
        df = C @ da
        alpha, fa, aa, oa = 1.0, f, a, obj
        while alpha > 1e-12:                                     # step halving on the objective
            f_try, a_try = f + alpha * df, a + alpha * da
            o_try = float(-0.5 * a_try @ f_try + log_p(family, y, f_try + shift, s).sum())
            if math.isfinite(o_try) and o_try >= obj - 1e-12 * (1 + abs(obj)):
                fa, aa, oa = f_try, a_try, o_try
                break
            alpha *= 0.5
        change = float((fa - f).abs().max()) if m else 0.0
        f, a, obj = fa, aa, oa
        if change < TOL:
            break
    g, W, sW, L = newton_system(f)
    SH = Sigma @ H.T
    mean = SH @ g
    V = torch.linalg.solve_triangular(L, sW[:, None] * SH.T, upper=False)
    cov = (Sigma - V.T @ V).reshape(n, d, n, d)
    i = torch.arange(n)
    ev = float(-0.5 * g @ f + log_p(family, y, f + shift, s).sum() - torch.log(torch.diagonal(L)).sum())
    return dict(mean=mean.reshape(n, d), cov_diag=cov[i, :, i, :], cov_off=cov[i[1:], :, i[:-1], :], log_evidence=ev,
                iterations=iterations, f=f, C=C, g=g, shift=shift, H=H, Sigma=Sigma, y=y, s=s)


def gaussian_closed_form(t):
    """(mean [n d], covariance [n d, n d], log evidence) of the dense Gaussian N(y - shift; 0, C_f + diag s) behind a
    truth ``t`` of the Gaussian family"""
    S = t["C"] + torch.diag(t["s"])
    r = t["y"] - t["shift"]
    L = torch.linalg.cholesky(S)
    w = torch.cholesky_solve(r.unsqueeze(-1), L).squeeze(-1)
    SH = t["Sigma"] @ t["H"].T
    ev = float(-0.5 * r @ w - torch.log(torch.diagonal(L)).sum() - 0.5 * r.numel() * math.log(2 * math.pi))
    return SH @ w, t["Sigma"] - SH @ torch.cholesky_solve(SH.T, L), ev


# ---- the cases of the GPU tests ----------------------------------------------------------------------------------------
LENGTHS_TRUTH = (1, 2, 6, 3, 131)        # 131: more than two strides of a 64-lane workgroup, the last one partial
LENGTHS_FORMS = (1, 2, 6, 3)
RANKS_TRUTH, OBS_TRUTH = (1, 3, 5, 8), (1, 3, 8)


class Case:
    """A model (fp64 CPU matrices N, R, B), an offset and a list of series, each a dict(ts, ys, mask, log_exposure,
    noise_var) with None for what the family does not take."""

    def __init__(self, family, N, R, B, offset, series):
        self.family, self.N, self.R, self.B, self.offset, self.series = family, N, R, B, offset, series
        self._truths = None

    @property
    def G(self):
        d = self.N.shape[0]
        return self.N @ self.N.T + self.R - self.R.T + 1e-5 * torch.eye(d, dtype=F64)

    @property
    def lengths(self):
        return [sr["ts"].shape[0] for sr in self.series]

    def truths(self):
        if self._truths is None:
            self._truths = [truth(sr["ts"], self.G, self.B, sr["ys"], sr["mask"], self.family, self.offset, sr["log_exposure"],
                                  sr["noise_var"]) for sr in self.series]
        return self._truths


def draw_model(d, obs, gen):
    """N, R as the other LEG tests condition them; B scaled so that B z has a standard deviation near 0.8 at every rank"""
    N = torch.tril(0.4 * torch.randn(d, d, generator=gen, dtype=F64)) + 0.8 * torch.eye(d, dtype=F64)
    R = torch.tril(0.3 * torch.randn(d, d, generator=gen, dtype=F64), -1)
    B = 0.8 * torch.randn(obs, d, generator=gen, dtype=F64) / math.sqrt(d)
    return N, R, B


def draw_series(n, G, B, offset, family, gen, keep=0.6, exposure=False):
    """One series drawn from the model: a path of the prior, the linear predictor, then counts, binary outcomes or
    Gaussian values; a mask that keeps ``keep`` of the entries."""
    obs, d = B.shape
    # gaps of at least 0.5, as tests/_modelscase.py takes them for fp32: I - E^T E of a random generator stays well
    # conditioned, so the prior blocks are positive definite in fp32 at every rank
    ts = 3.0 * torch.rand((), generator=gen, dtype=F64) + torch.cumsum(0.5 + 0.5 * torch.rand(n, generator=gen, dtype=F64), 0)
    Sigma = _gapref.prior_covariance(ts, G)
    Lc = torch.linalg.cholesky(Sigma + 1e-12 * torch.eye(n * d, dtype=F64))
    z = (Lc @ torch.randn(n * d, generator=gen, dtype=F64)).reshape(n, d)
    le = 0.6 * torch.rand(n, obs, generator=gen, dtype=F64) - 0.3 if exposure else None
    eta = z @ B.T + offset + (le if le is not None else 0.0)
    nv = None
    if family == "poisson":
        ys = torch.poisson(torch.exp(eta), generator=gen)
    elif family == "bernoulli":
        ys = (torch.rand(n, obs, generator=gen, dtype=F64) < torch.sigmoid(eta)).to(F64)
    else:
        nv = 0.1 + 1.9 * torch.rand(n, obs, generator=gen, dtype=F64)
        ys = eta + nv.sqrt() * torch.randn(n, obs, generator=gen, dtype=F64)
    mask = torch.rand(n, obs, generator=gen) < keep
    return dict(ts=ts, ys=ys, mask=mask, log_exposure=le, noise_var=nv)


@functools.lru_cache(maxsize=None)
def batch_case(d, obs, family, lengths, seed=0):
    """The ragged batch of the truth and form tests: offsets in [0, 1], so that eta lies roughly in [-2, 3].  A series of
    six rows has its row 2 wholly unobserved, a series of three rows observes nothing at all; the Poisson cases carry a
    log_exposure."""
    gen = torch.Generator().manual_seed(1000 * seed + 100 * d + 10 * obs + FAMILIES.index(family))
    N, R, B = draw_model(d, obs, gen)
    offset = torch.rand(obs, generator=gen, dtype=F64)
    G = N @ N.T + R - R.T + 1e-5 * torch.eye(d, dtype=F64)
    series = []
    for n in lengths:
        sr = draw_series(n, G, B, offset, family, gen, exposure=(family == "poisson"))
        if n == 6:
            sr["mask"][2] = False
        if n == 3:
            sr["mask"][:] = False
        series.append(sr)
    return Case(family, N, R, B, offset, series)


@functools.lru_cache(maxsize=None)
def damping_case(d=3, obs=2):
    """One series of six rows with Poisson counts near 1000 and a zero offset: from z = 0 the undamped Newton step puts
    eta near 1000 and e^eta overflows in either precision."""
    gen = torch.Generator().manual_seed(77)
    N, R, B = draw_model(d, obs, gen)
    B = B + 0.5 * torch.sign(B)                                   # (no entry of B near zero: eta can reach log 1000)
    ts = torch.cumsum(0.5 + 0.5 * torch.rand(6, generator=gen, dtype=F64), 0)
    ys = 1000.0 + torch.randint(-60, 61, (6, obs), generator=gen).to(F64)
    mask = torch.rand(6, obs, generator=gen) < 0.6
    mask[0, 0] = True
    sr = dict(ts=ts, ys=ys, mask=mask, log_exposure=None, noise_var=None)
    return Case("poisson", N, R, B, torch.zeros(obs, dtype=F64), [sr])


@functools.lru_cache(maxsize=None)
def independence_case():
    """An ordinary Poisson series of five rows (rank 3, two channels) and, under the same model, a slow neighbour: six
    rows of counts near 10^4, which a zero start leaves many more steps away; and a third series of nine rows."""
    gen = torch.Generator().manual_seed(91)
    d, obs = 3, 2
    N, R, B = draw_model(d, obs, gen)
    B = B + 0.5 * torch.sign(B)
    G = N @ N.T + R - R.T + 1e-5 * torch.eye(d, dtype=F64)
    offset = torch.zeros(obs, dtype=F64)
    plain = draw_series(5, G, B, offset, "poisson", gen)
    slow = dict(damping_case().series[0])
    slow["ys"] = 10.0 * slow["ys"]
    other = draw_series(9, G, B, offset, "poisson", gen)
    return Case("poisson", N, R, B, offset, [plain, slow, other])


@functools.lru_cache(maxsize=None)
def mirror_case(mirrored, d=3, obs=2):
    """Bernoulli data with offsets near +8 (near-certain events: almost every outcome is 1), lengths (1, 2, 6, 70); and its
    mirror image (1 - y, -offset, -B), which is the same posterior over z: l(eta; y) = l(-eta; 1 - y)."""
    gen = torch.Generator().manual_seed(123)
    N, R, B = draw_model(d, obs, gen)
    offset = 8.0 + torch.rand(obs, generator=gen, dtype=F64)
    G = N @ N.T + R - R.T + 1e-5 * torch.eye(d, dtype=F64)
    series = [draw_series(n, G, B, offset, "bernoulli", gen, keep=0.8) for n in (1, 2, 6, 70)]
    series[2]["ys"][0, 0], series[2]["mask"][0, 0] = 0.0, True        # (one event that did not happen, observed)
    if mirrored:
        series = [dict(sr, ys=1.0 - sr["ys"]) for sr in series]
        return Case("bernoulli", N, R, -B, -offset, series)
    return Case("bernoulli", N, R, B, offset, series)


@functools.lru_cache(maxsize=None)
def stall_case(d=3, obs=2):
    """The damping case with counts near 10^6, everything observed: from z = 0 the proposal has dEta near 10^6 and the
    smallest candidate, 2^-11 of it, is still near 500 -- no candidate gains, the series stalls at its first step (DESIGN
    4.26).  Not among ``all_cases``: at counts of 10^6 the truth's stationarity residual is 4e-9, rounding of g = y - e^f,
    above the 1e-10 tests/test_laplaceref.py asks of the others; the bounds of the GPU test are relative and keep it."""
    base = damping_case(d, obs)
    sr = dict(base.series[0])
    sr["ys"] = 1000.0 * sr["ys"]
    sr["mask"] = torch.ones_like(sr["mask"])
    return Case("poisson", base.N, base.R, base.B, base.offset, [sr])


def newton_system_at(t, family, z):
    """What ``max_iter=0`` returns, from the dense truth ``t`` of a series, at the point z [n, d]: (cov_diag, cov_off,
    psi(z) + (log|K| - log|J(z)|) / 2 with every term of log p included) -- J(z) = K + H^T W H, and K = Sigma^-1 enters
    only through z^T K z."""
    Sigma, H, y, s = t["Sigma"], t["H"], t["y"], t["s"]
    n, d = z.shape
    zf = z.reshape(-1).to(F64)
    prior = -0.5 * float(zf @ torch.linalg.solve(Sigma, zf))
    i = torch.arange(n)
    if y.numel() == 0:
        cov = Sigma.reshape(n, d, n, d)
        return cov[i, :, i, :], cov[i[1:], :, i[:-1], :], prior
    f = H @ zf
    _, W = grad_weight(family, y, f + t["shift"], s)
    sW = W.sqrt()
    L = torch.linalg.cholesky(torch.eye(y.numel(), dtype=F64) + sW[:, None] * t["C"] * sW[None, :])
    V = torch.linalg.solve_triangular(L, sW[:, None] * (Sigma @ H.T).T, upper=False)
    cov = (Sigma - V.T @ V).reshape(n, d, n, d)
    ev = prior + float(log_p(family, y, f + t["shift"], s).sum() - torch.log(torch.diagonal(L)).sum())
    return cov[i, :, i, :], cov[i[1:], :, i[:-1], :], ev


LENGTHS_FP32 = LENGTHS_FORMS
FORMS_FP32 = ((1, 1), (3, 2), (5, 3), (8, 8))


def all_cases():
    """(name, case) of every input of tests/test_leg_laplace.py (but ``stall_case``: see there)"""
    out = []
    for d in RANKS_TRUTH:
        for obs in OBS_TRUTH:
            for family in ("poisson", "bernoulli"):
                out.append(("truth-d%d-o%d-%s" % (d, obs, family), batch_case(d, obs, family, LENGTHS_TRUTH)))
    for d in range(1, 9):
        for obs in range(1, 9):
            out.append(("forms-d%d-o%d" % (d, obs), batch_case(d, obs, "poisson", LENGTHS_FORMS, 1)))
    for d, obs in ((1, 1), (3, 2), (5, 3), (8, 8)):
        out.append(("gaussian-d%d-o%d" % (d, obs), batch_case(d, obs, "gaussian", LENGTHS_FORMS, 2)))
    for d, obs in FORMS_FP32:
        out.append(("fp32-bernoulli-d%d-o%d" % (d, obs), batch_case(d, obs, "bernoulli", LENGTHS_FP32, 3)))
    out.append(("mirror", mirror_case(False)))
    out.append(("mirror-image", mirror_case(True)))
    out.append(("damping", damping_case()))
    out.append(("independence", independence_case()))
    return out

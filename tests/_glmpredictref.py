"""References for cgps_leg_glm_predict (csrc/cgps_leg_glm_predict.h) in mpmath, sharing none of the
library's formulas or literals:

    rule(family, y, mu, v)    the adaptive Gauss-Hermite rule restated from its definition: 12 clipped Newton steps from
                              u = 0 on h(u) = l(y, mu + sqrt(v) u) - u^2 / 2, the scale s = (1 + v w)^(-1/2), and
                              log s + logsumexp_i [log(w_i / sqrt(pi)) + x_i^2 + h(u* + sqrt(2) s x_i)] over the 32
                              physicists' nodes, which are computed here (Golub-Welsch, then Newton on H_32).  With it
                              comes A, the sum of the absolute values of the terms of the log integrand at its largest
                              node, and the largest |eta| the rule touches: the scale of the bounds of the tests.
    truth(family, y, mu, v)   log of the integral of p(y | eta) N(eta; mu, v) by ``mpmath.quad``, the interval split at the
                              integrand's mode +- multiples of its width (and of 1, the width of the Gaussian factor): an
                              unsplit quad misses the peak at y = 1000, mu = -3, v = 4 by 147 nats.

and the case grid of the tests.  l is the whole log density: Poisson y eta - e^eta - lgamma(y + 1), Bernoulli y eta -
softplus(eta).  CPU only."""
import functools

import mpmath

mp = mpmath.mp
mpf = mpmath.mpf
DPS = 40
NEWTON, Q = 12, 32

POISSON_Y, POISSON_MU = (0, 1, 5, 50, 1000), (-3, -1, 0, 2, 4, 6)
BERNOULLI_Y, BERNOULLI_MU = (0, 1), (-40, -8, -2, 0, 1, 8, 40)
VARIANCES = (0.0, 1e-6, 0.01, 0.25, 1.0, 2.0)
LIMIT_VARIANCES = (4.0, 25.0)          # measured and written down as the method's limit, not asserted
RTOL, ATOL = 1e-7, 1e-9               # the project's standing fp64 bound


def cases(family, variances=VARIANCES):
    """[(y, mu, v)] of the family's grid, as Python floats"""
    ys, mus = (POISSON_Y, POISSON_MU) if family == "poisson" else (BERNOULLI_Y, BERNOULLI_MU)
    return [(float(y), float(mu), float(v)) for y in ys for mu in mus for v in variances]


def _softplus(eta):
    return mpmath.log1p(mpmath.exp(eta)) if eta <= 0 else eta + mpmath.log1p(mpmath.exp(-eta))


@functools.lru_cache(maxsize=None)
def _lgamma1(y):
    with mpmath.workdps(60):
        return mpmath.loggamma(mpf(y) + 1)


def log_density(family, y, eta):
    """(l(y, eta), the sum of the absolute values of its terms)"""
    if family == "poisson":
        e, lg = mpmath.exp(eta), +_lgamma1(float(y))
        return y * eta - e - lg, abs(y * eta) + e + abs(lg)
    sp = _softplus(eta)
    return y * eta - sp, abs(y * eta) + sp


def slope_weight(family, y, eta):
    """(g = dl / d eta, w = -d^2 l / d eta^2)"""
    if family == "poisson":
        e = mpmath.exp(eta)
        return y - e, e
    sig = 1 / (1 + mpmath.exp(-eta))
    return y - sig, sig * (1 - sig)


@functools.lru_cache(maxsize=None)
def nodes():
    """[(x_i, w_i)] of the 32-point physicists' Gauss-Hermite rule, at 60 digits"""
    with mpmath.workdps(60):
        J = mpmath.zeros(Q)
        for i in range(Q - 1):
            J[i, i + 1] = J[i + 1, i] = mpmath.sqrt(mpf(i + 1) / 2)
        E, _ = mpmath.eigsy(J)
        out = []
        for i in range(Q):
            x = E[i]
            for _ in range(6):
                x = x - mpmath.hermite(Q, x) / (2 * Q * mpmath.hermite(Q - 1, x))
            w = 2 ** (Q - 1) * mpmath.factorial(Q) * mpmath.sqrt(mpmath.pi) / (Q ** 2 * mpmath.hermite(Q - 1, x) ** 2)
            out.append((x, w))
        assert abs(sum(w for _, w in out) - mpmath.sqrt(mpmath.pi)) < mpf(10) ** -50
        return sorted(out)


def _rule(family, y, mu, v):
    y, mu, v = mpf(y), mpf(mu), mpf(v)
    sv = mpmath.sqrt(v)
    u = mpf(0)
    for _ in range(NEWTON):
        g, w = slope_weight(family, y, mu + sv * u)
        step = (sv * g - u) / (1 + v * w)
        if v > 0:
            step = min(step, 1 / sv)
        u += step
    _, w = slope_weight(family, y, mu + sv * u)
    s = 1 / mpmath.sqrt(1 + v * w)
    terms, eta_max = [], mpf(0)
    for x, wt in nodes():
        ui = u + mpmath.sqrt(2) * s * x
        eta = mu + sv * ui
        l, lS = log_density(family, y, eta)
        c = mpmath.log(wt / mpmath.sqrt(mpmath.pi))
        terms.append((c + x * x + l - ui * ui / 2, abs(c) + x * x + lS + ui * ui / 2))
        eta_max = max(eta_max, abs(eta))
    top, A = max(terms)
    value = mpmath.log(s) + top + mpmath.log(sum(mpmath.exp(t - top) for t, _ in terms))
    return value, A, eta_max


@functools.lru_cache(maxsize=None)
def rule(family, y, mu, v):
    """(log I by the rule, A, max |eta|) as mpf"""
    with mpmath.workdps(DPS):
        return _rule(family, y, mu, v)


def _mode(family, y, mu, sv):
    """the maximiser of h(u) = l(y, mu + sv u) - u^2 / 2: h' = sv g - u is strictly decreasing, so by bisection"""
    slope = lambda u: sv * slope_weight(family, y, mu + sv * u)[0] - u      # noqa: E731
    lo, hi = mpf(-1), mpf(1)
    while slope(lo) < 0:
        lo *= 2
    while slope(hi) > 0:
        hi *= 2
    for _ in range(4 * DPS):
        mid = (lo + hi) / 2
        if slope(mid) > 0:
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2


def _truth(family, y, mu, v):
    y, mu, v = mpf(y), mpf(mu), mpf(v)
    if v == 0:
        return log_density(family, y, mu)[0]
    sv = mpmath.sqrt(v)
    u0 = _mode(family, y, mu, sv)
    h = lambda u: log_density(family, y, mu + sv * u)[0] - u * u / 2      # noqa: E731
    h0 = h(u0)
    width = 1 / mpmath.sqrt(1 + v * slope_weight(family, y, mu + sv * u0)[1])
    # the peak has the width `width`; away from it the Gaussian factor alone decides, and its width is 1
    steps = sorted({k * width for k in (1, 2, 4, 8, 16, 32, 64)} | {mpf(k) for k in (1, 2, 4, 8, 16, 40)})
    points = [u0 - t for t in reversed(steps)] + [u0] + [u0 + t for t in steps]
    total = mpmath.quad(lambda u: mpmath.exp(h(u) - h0), points)
    return h0 + mpmath.log(total) - mpmath.log(2 * mpmath.pi) / 2


@functools.lru_cache(maxsize=None)
def truth(family, y, mu, v):
    """log of the integral of p(y | eta) N(eta; mu, v) d eta, as mpf"""
    with mpmath.workdps(DPS):
        return _truth(family, y, mu, v)


def moment(fn, mu, v):
    """the integral of fn(eta) N(eta; mu, v) d eta for a smooth fn of moderate growth, by ``mpmath.quad`` split around mu"""
    with mpmath.workdps(DPS):
        mu, v = mpf(mu), mpf(v)
        if v == 0:
            return fn(mu)
        sv = mpmath.sqrt(v)
        points = [mu + k * sv for k in (-40, -20, -10, -5, -2, 0, 2, 5, 10, 20, 40)]
        return mpmath.quad(lambda e: fn(e) * mpmath.exp(-(e - mu) ** 2 / (2 * v)), points) / mpmath.sqrt(2 * mpmath.pi * v)


def outputs(family, y, mu, v, s=None):
    """What cgps_leg_glm_predict owes for one entry whose linear predictor is N(mu, v), by the rule: dict of (value, bound
    scale S) for mean, var and logpdf as floats, where a correct fp implementation is within 64 eps (1 + eta_max) S.
    logpdf: S = A.  Bernoulli mean = exp(L1): S = mean A_1 (first order in the error of L1); var = exp(L1 + L0): S = var
    (A_1 + A_0).  Poisson mean = exp(mu + v / 2): S = mean (1 + |mu| + v / 2); var = mean + mean^2 expm1(v): S = 2 var
    (1 + |mu| + v).  Gaussian (``s``: the observation variance): closed forms."""
    with mpmath.workdps(DPS):
        mu_, v_ = mpf(mu), mpf(v)
        if family == "gaussian":
            tot, res = v_ + mpf(s), mpf(y) - mu_
            lg = mpmath.log(2 * mpmath.pi * tot) / 2
            return dict(mean=(float(mu_), abs(float(mu_))), var=(float(tot), float(tot)),
                        logpdf=(float(-res * res / (2 * tot) - lg), float(res * res / (2 * tot) + abs(lg))), eta_max=abs(float(mu_)))
        if family == "poisson":
            L, A, top = rule(family, y, mu, v)
            mean = mpmath.exp(mu_ + v_ / 2)
            var = mean + mean * mean * mpmath.expm1(v_)
            return dict(mean=(float(mean), float(mean * (1 + abs(mu_) + v_ / 2))), var=(float(var), float(2 * var * (1 + abs(mu_) + v_))),
                        logpdf=(float(L), float(A)), eta_max=float(top))
        L1, A1, t1 = rule(family, 1.0, mu, v)
        L0, A0, t0 = rule(family, 0.0, mu, v)
        mean, var = mpmath.exp(L1), mpmath.exp(L1 + L0)
        L, A = (L1, A1) if y == 1 else (L0, A0)
        return dict(mean=(float(mean), float(mean * (1 + A1))), var=(float(var), float(var * (1 + A1 + A0))),
                    logpdf=(float(L), float(A)), eta_max=float(max(t1, t0)))

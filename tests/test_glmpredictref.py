"""The quadrature rule of cgps_leg_glm_predict without a GPU: the rule restated in mpmath
(tests/_glmpredictref.py) against the integral it approximates, the library's composed path against that rule, the closed
forms against the integrals they stand for, and the grid's fitness for fp32.

Measured here (the rule's error as a fraction of the fp64 bound rtol 1e-7 / atol 1e-9, worst case of the grid):
Poisson 7.3e-4 at v <= 1 and 0.43 at v = 2; Bernoulli 3.0e-7 at v <= 1 and 7.6e-4 at v = 2.  The method's limit, measured
and not asserted: at v = 4 Poisson y = 0, mu = -3 misses the bound by a factor of 170 (1.8e-5 relative; the integrand is
doubly exponential) while Bernoulli stays at 0.31 of it; at v = 25 the worst cases are 6.6e-3 (Poisson) and 4.3e-3
(Bernoulli) relative.  A LEG posterior variance cannot exceed the prior's b_c . b_c.
The composed path in fp64 on the CPU: at most 0.011 of its bound 64 eps (1 + max |eta|) A."""
import mpmath
import pytest
import torch

import _glmpredictref as gp
from cyclic_gps import _hip, leg

F64, F32 = torch.float64, torch.float32
CODE = {"poisson": _hip.GLM_POISSON, "bernoulli": _hip.GLM_BERNOULLI, "gaussian": _hip.GLM_GAUSSIAN}
FAMILIES = ("poisson", "bernoulli")
GAUSSIAN_CASES = ((0.3, -1.0, 0.5, 0.7), (-2.0, 4.0, 0.0, 0.1), (5.0, 0.0, 2.0, 1.9), (0.0, 0.0, 1e-6, 0.25))      # (y, mu, v, s)


def _fraction(family, case):
    r, t = gp.rule(family, *case)[0], gp.truth(family, *case)
    return float(abs(r - t) / (gp.RTOL * abs(t) + gp.ATOL)), float(abs(r - t) / max(abs(t), mpmath.mpf(10) ** -300))


# ---- a: the rule against the truth ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_the_rule_is_within_the_fp64_bound_of_the_integral(family):
    worst = {}
    for case in gp.cases(family):
        frac, _ = _fraction(family, case)
        key = "v <= 1" if case[2] <= 1 else "v = 2"
        if frac >= worst.get(key, (0.0, None))[0]:
            worst[key] = (frac, case)
    print("%s: worst error / bound  %s" % (family, "  ".join("%s %.3g at (y, mu, v) = %s" % (k, f, c) for k, (f, c) in sorted(worst.items()))))
    for key, (frac, case) in worst.items():
        assert frac <= 1.0, (family, key, case, frac)


@pytest.mark.parametrize("family", FAMILIES)
def test_the_limit_of_the_method_is_measured(family):
    """v = 4 and v = 25: printed, and written into DESIGN 4.28 and the module's docstring; nothing is asserted of the error"""
    for v in gp.LIMIT_VARIANCES:
        worst = max((_fraction(family, case) + (case,) for case in gp.cases(family, (v,))))
        print("%s v = %g: worst error / bound %.3g, relative %.3g, at (y, mu, v) = %s" % ((family, v) + worst))
        assert worst[0] == worst[0]                      # (finite arithmetic: not NaN)


def test_an_unsplit_quadrature_is_not_a_truth():
    """the peak at y = 1000, mu = -3, v = 4 sits 5 standard deviations out and is 0.03 wide: the truth finds it"""
    t = gp.truth("poisson", 1000.0, -3.0, 4.0)
    assert abs(float(t) + 20.7861089328909) < 1e-9


# ---- b: the composed path against the rule --------------------------------------------------------------------------------
def _composed(family, cases, T, ys=True):
    """the composed path on a column of entries whose (mu, v) are the cases', rounded to T: d = obs = 1, B = 1"""
    col = lambda k: torch.tensor([[c[k]] for c in cases], dtype=F64).to(T)      # noqa: E731
    extra = torch.tensor([[c[3]] for c in cases], dtype=F64).to(T) if family == "gaussian" else None
    out = leg._glm_predict_composed(CODE[family], col(1), col(2).unsqueeze(-1), col(0) if ys else None, None, None, extra,
                                    torch.ones(1, 1, dtype=T))
    return out, [tuple(float(x) for x in (col(0)[i, 0], col(1)[i, 0], col(2)[i, 0])) for i in range(len(cases))]


@pytest.mark.parametrize("family", FAMILIES)
def test_the_composed_path_is_the_rule(family):
    """fp64 CPU tensors: every output within 64 eps (1 + max |eta|) S of the mpmath rule, S = A for logpdf"""
    eps = float(torch.finfo(F64).eps)
    cases = gp.cases(family)
    out, at = _composed(family, cases, F64)
    worst = dict(mean=0.0, var=0.0, logpdf=0.0)
    for i, case in enumerate(at):
        ref = gp.outputs(family, *case)
        assert float(out[0][i, 0]) == case[1] and float(out[1][i, 0]) == case[2]
        for k, name in ((2, "mean"), (3, "var"), (4, "logpdf")):
            want, S = ref[name]
            err, bound = abs(float(out[k][i, 0]) - want), 64 * eps * (1 + ref["eta_max"]) * S
            worst[name] = max(worst[name], err / bound)
            assert err <= bound, (family, name, case, float(out[k][i, 0]), want, err / bound)
    print("%s composed fp64: worst error / bound  %s" % (family, "  ".join("%s %.3g" % kv for kv in worst.items())))


def test_the_composed_path_without_data_and_with_a_mask():
    cases = gp.cases("bernoulli")[:12]
    full, _ = _composed("bernoulli", cases, F64)
    none, _ = _composed("bernoulli", cases, F64, ys=False)
    assert none[4] is None and all(torch.equal(a, b) for a, b in zip(full[:4], none[:4]))
    col = lambda k: torch.tensor([[c[k]] for c in cases], dtype=F64)      # noqa: E731
    mask = torch.arange(12).reshape(12, 1) % 2 == 0
    ys = torch.where(mask, col(0), torch.full((12, 1), float("nan"), dtype=F64))
    part = leg._glm_predict_composed(CODE["bernoulli"], col(1), col(2).unsqueeze(-1), ys, mask, None, None, torch.ones(1, 1, dtype=F64))
    assert torch.equal(part[4][mask], full[4][mask]) and bool((part[4][~mask] == 0).all())
    assert all(torch.equal(a, b) for a, b in zip(full[:4], part[:4]))


# ---- c: the closed forms ----------------------------------------------------------------------------------------------------
def test_the_poisson_moments_are_the_integrals():
    for mu in gp.POISSON_MU:
        for v in gp.VARIANCES:
            m1 = gp.moment(mpmath.exp, mu, v)                       # E y = E e^eta
            m2 = gp.moment(lambda e: mpmath.exp(2 * e), mu, v)      # Var y = E e^eta + Var e^eta
            ref = gp.outputs("poisson", 0.0, float(mu), float(v))
            assert abs(ref["mean"][0] - float(m1)) <= gp.RTOL * float(m1) + gp.ATOL, (mu, v)
            var = float(m1 + m2 - m1 * m1)
            assert abs(ref["var"][0] - var) <= gp.RTOL * var + gp.ATOL, (mu, v)


def test_the_gaussian_outputs_are_the_integrals():
    out, _ = _composed("gaussian", GAUSSIAN_CASES, F64)
    for i, (y, mu, v, s) in enumerate(GAUSSIAN_CASES):
        dens = lambda e: mpmath.exp(-(y - e) ** 2 / (2 * mpmath.mpf(s))) / mpmath.sqrt(2 * mpmath.pi * s)      # noqa: E731
        want = dict(mean=gp.moment(lambda e: e, mu, v), var=s + gp.moment(lambda e: (e - mu) ** 2, mu, v),
                    logpdf=mpmath.log(gp.moment(dens, mu, v)))
        ref = gp.outputs("gaussian", y, mu, v, s)
        for k, name in ((2, "mean"), (3, "var"), (4, "logpdf")):
            w = float(want[name])
            assert abs(ref[name][0] - w) <= gp.RTOL * abs(w) + gp.ATOL, (name, y, mu, v, s)
            assert abs(float(out[k][i, 0]) - w) <= gp.RTOL * abs(w) + gp.ATOL, (name, y, mu, v, s)


def test_the_bernoulli_moments_are_the_integrals():
    """mean = exp(L1) is E sigma(eta) and var = exp(L1 + L0) is p (1 - p), with every digit near certainty"""
    for mu, v in ((-40.0, 0.25), (-2.0, 1.0), (8.0, 2.0), (40.0, 0.01)):
        p1, p0 = mpmath.exp(gp.truth("bernoulli", 1.0, mu, v)), mpmath.exp(gp.truth("bernoulli", 0.0, mu, v))
        assert abs(p1 + p0 - 1) < 1e-25
        ref = gp.outputs("bernoulli", 1.0, mu, v)
        assert abs(ref["mean"][0] - float(p1)) <= gp.RTOL * float(p1) and abs(ref["var"][0] - float(p1 * p0)) <= gp.RTOL * float(p1 * p0)
        assert ref["var"][0] > 0


# ---- d: the grid in fp32 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_every_case_is_representable_in_fp32(family):
    """inputs and outputs of every case are finite normal numbers of fp32 (or zero), the composed path agrees with the rule
    at the rounded inputs to fp32 rounding, and no v rounds to another grid value"""
    info = torch.finfo(F32)
    cases = gp.cases(family)
    out, at = _composed(family, cases, F32)
    assert len({c[1:] for c in at}) == len({c[1:] for c in cases})
    for i, case in enumerate(at):
        ref = gp.outputs(family, *case)
        for k, name in ((2, "mean"), (3, "var"), (4, "logpdf")):
            want, got = ref[name][0], float(out[k][i, 0])
            assert want == 0.0 or info.tiny <= abs(want) <= info.max, (family, name, case, want)
            # one rounding to fp32 on top of the fp64 bound of the test above
            bound = info.eps * abs(want) + 64 * float(torch.finfo(F64).eps) * (1 + ref["eta_max"]) * ref[name][1]
            assert abs(got - want) <= bound, (family, name, case, got, want)

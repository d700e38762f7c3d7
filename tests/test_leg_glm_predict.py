"""cgps_leg_glm_predict (csrc/cgps_leg_glm_predict.h) called directly, against the mpmath rule of
tests/_glmpredictref.py (which tests/test_glmpredictref.py holds to the integral itself without a GPU): the case grid in
both precisions, every rank x channel form, every combination of optional operands, and the properties of the contract
(absent entries never read, a rounding-negative variance, the Bernoulli tails, rows independent of their neighbours,
P = 0).

Bounds.  fp64: every output within 64 eps (1 + max |eta|) S of the rule, S the scale tests/_glmpredictref.outputs gives
(for logpdf the sum of the absolute values of the terms of the log integrand at its largest node).  fp32: within
max(4 x the composed path's fp32 error, 64 eps32 x the same scale).  eta_mean and eta_var, plain dot products: within
n eps S of the fp64 value, n the number of their terms and S the sum of the terms' absolute values.

Measured on an MI355X (worst error / bound): the grid 0.011 in fp64 (Poisson logpdf) and 0.0053 in fp32, the 64 forms
0.0092 and 0.0033."""
import ctypes
import itertools

import pytest
import torch

import _glmpredictref as gp
from cyclic_gps import _hip, leg

F64, F32 = torch.float64, torch.float32
DTYPES = pytest.mark.parametrize("T", [F64, F32], ids=["fp64", "fp32"])
CODE = {"poisson": _hip.GLM_POISSON, "bernoulli": _hip.GLM_BERNOULLI, "gaussian": _hip.GLM_GAUSSIAN}
NAMES = ("eta_mean", "eta_var", "mean", "var", "logpdf")
GAUSSIAN_CASES = ((0.3, -1.0, 0.5, 0.7), (-2.0, 4.0, 0.0, 0.1), (5.0, 0.0, 2.0, 1.9), (0.0, 0.0, 1e-6, 0.25))      # (y, mu, v, s)


def _hip_call(family, zm, zc, ys, observed, offset, extra, Bm):
    out = leg._glm_predict_hip(CODE[family], zm, zc, ys, observed, offset, extra, Bm)
    torch.cuda.synchronize()
    return out


def _columns(family, cases, T):
    """operands with d = obs = 1 and B = 1 whose (mu, v) are the cases' rounded to T, and those rounded cases"""
    col = lambda k: torch.tensor([[c[k]] for c in cases], dtype=F64).to(T)      # noqa: E731
    extra = col(3) if family == "gaussian" else None
    at = [tuple(float(x) for x in [col(k)[i, 0] for k in range(len(cases[0]))]) for i in range(len(cases))]
    return (col(1), col(2).unsqueeze(-1), col(0), None, None, extra, torch.ones(1, 1, dtype=T)), at


def _against_the_rule(what, family, got, composed, at, T):
    """every entry of mean, var and logpdf against the rule at (y, mu, v[, s]) = at[i]; returns the worst error / bound"""
    eps = float(torch.finfo(T).eps)
    worst = dict(mean=0.0, var=0.0, logpdf=0.0)
    for i, case in enumerate(at):
        ref = gp.outputs(family, *case)
        for k, name in ((2, "mean"), (3, "var"), (4, "logpdf")):
            if got[k] is None:
                continue
            want, S = ref[name]
            bound = 64 * eps * (1 + ref["eta_max"]) * S
            if T == F32:
                bound = max(bound, 4 * abs(float(composed[k].reshape(-1)[i]) - want))
            err = abs(float(got[k].reshape(-1)[i]) - want)
            worst[name] = max(worst[name], err / bound if bound > 0 else float(err > 0))
            assert err <= bound, (what, name, case, float(got[k].reshape(-1)[i]), want, err, bound)
    print("%s %s: worst error / bound  %s" % (what, "fp64" if T == F64 else "fp32", "  ".join("%s %.3g" % kv for kv in worst.items())))
    return worst


# ---- the grid -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("family", ["poisson", "bernoulli", "gaussian"])
def test_the_kernel_is_the_rule_on_the_grid(family, T):
    cases = list(GAUSSIAN_CASES) if family == "gaussian" else gp.cases(family)
    ops, at = _columns(family, cases, T)
    got = [t.cpu() for t in _hip_call(family, *[None if t is None else t.cuda() for t in ops])]
    composed = leg._glm_predict_composed(CODE[family], *ops)
    assert torch.equal(got[0], ops[0]) and torch.equal(got[1], ops[1].squeeze(-1))       # mu and v themselves: B = 1
    _against_the_rule("grid " + family, family, got, composed, at, T)


# ---- every rank x channel form ---------------------------------------------------------------------------------------------
def _general(d, obs, T, P=3, seed=0):
    """random operands, everything given: fp64 CPU tensors rounded to T"""
    gen = torch.Generator().manual_seed(9000 + 100 * d + 10 * obs + seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=F64)      # noqa: E731
    a = 0.4 * r(P, d, d)
    t = dict(zm=0.5 * r(P, d), zc=a @ a.transpose(-1, -2) / d + 0.05 * torch.eye(d, dtype=F64),
             ys=torch.poisson(torch.full((P, obs), 2.0, dtype=F64), generator=gen), observed=torch.rand(P, obs, generator=gen) < 0.7,
             offset=0.3 * r(obs), extra=0.2 * r(P, obs), Bm=0.8 * r(obs, d) / d ** 0.5)
    return {k: (v if v.dtype == torch.bool else v.to(T)) for k, v in t.items()}


def _dots(t):
    """(mu, its n eps S bound factor, v, its) in fp64 from the operands as the kernel read them"""
    zm, zc, Bm = t["zm"].to(F64), t["zc"].to(F64), t["Bm"].to(F64)
    d = zm.shape[1]
    mu = zm @ Bm.T + t["offset"].to(F64) + t["extra"].to(F64)
    muS = zm.abs() @ Bm.abs().T + t["offset"].to(F64).abs() + t["extra"].to(F64).abs()
    v = torch.einsum("ca,pab,cb->pc", Bm, zc, Bm)
    vS = torch.einsum("ca,pab,cb->pc", Bm.abs(), zc.abs(), Bm.abs())
    return mu, (d + 2) * muS, v, (d * d + d) * vS


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("d", range(1, 9))
def test_every_rank_and_channel_form(d, T):
    """obs = 1..8 at every rank, P = 3, Poisson with offset, log_exposure, data and a pattern: eta_mean and eta_var against
    fp64 dot products, the rest against the rule at the kernel's own (eta_mean, eta_var)"""
    eps = float(torch.finfo(T).eps)
    for obs in range(1, 9):
        t = _general(d, obs, T)
        g = {k: v.cuda() for k, v in t.items()}
        got = [x.cpu() for x in _hip_call("poisson", g["zm"], g["zc"], g["ys"], g["observed"], g["offset"], g["extra"], g["Bm"])]
        mu, muB, v, vB = _dots(t)
        assert bool(((got[0].to(F64) - mu).abs() <= eps * muB).all()), (d, obs, "eta_mean")
        assert bool(((got[1].to(F64) - v).abs() <= eps * vB).all()), (d, obs, "eta_var")
        mask = t["observed"].reshape(-1)
        ys = torch.where(t["observed"], t["ys"], torch.zeros_like(t["ys"]))
        at = [(float(y), float(m_), float(v_)) for y, m_, v_ in zip(ys.reshape(-1), got[0].reshape(-1), got[1].reshape(-1))]
        # the composed path from the kernel's own (mu, v): d = obs = 1, so that it rounds nothing before the rule either
        comp = leg._glm_predict_composed(CODE["poisson"], got[0].reshape(-1, 1), got[1].reshape(-1, 1, 1), ys.reshape(-1, 1), None,
                                         None, None, torch.ones(1, 1, dtype=T))
        keep = [i for i in range(len(at)) if bool(mask[i])]
        sel = lambda x: x.reshape(-1)[keep]      # noqa: E731
        _against_the_rule("form d %d obs %d" % (d, obs), "poisson", [None, None, got[2], got[3], None], comp, at, T)
        _against_the_rule("form d %d obs %d observed" % (d, obs), "poisson", [None, None, None, None, sel(got[4])],
                          [None, None, None, None, sel(comp[4])], [at[i] for i in keep], T)
        assert bool((got[4].reshape(-1)[~mask] == 0).all())


# ---- optional operands ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("family", ["poisson", "bernoulli", "gaussian"])
def test_every_combination_of_null_and_given(family, T):
    """pattern, offset, extra and ys each NULL or given: NULL is the neutral operand (everything observed, zeros), bit for
    bit, and without ys the other four outputs do not change.  The Gaussian family always has its variances."""
    d, obs, P = 3, 2, 37
    t = _general(d, obs, T, P=P, seed=1)
    if family == "bernoulli":
        t["ys"] = (t["ys"] > 1).to(T)
    if family == "gaussian":
        t["extra"] = t["extra"].abs() + 0.1
    g = {k: v.cuda() for k, v in t.items()}
    neutral = dict(observed=torch.ones(P, obs, dtype=torch.bool).cuda(), offset=torch.zeros(obs, dtype=T).cuda(),
                   extra=torch.zeros(P, obs, dtype=T).cuda())
    for has in itertools.product((False, True), repeat=4):
        hp, ho, he, hy = has
        if family == "gaussian" and not he:
            continue
        pick = lambda k, h: g[k] if h else None      # noqa: E731
        a = _hip_call(family, g["zm"], g["zc"], pick("ys", hy), pick("observed", hp), pick("offset", ho), pick("extra", he), g["Bm"])
        b = _hip_call(family, g["zm"], g["zc"], g["ys"], g["observed"] if hp else neutral["observed"],
                      g["offset"] if ho else neutral["offset"], g["extra"] if he else neutral["extra"], g["Bm"])
        assert (a[4] is None) == (not hy)
        for k in range(5 if hy else 4):
            assert torch.equal(a[k], b[k]), (family, has, NAMES[k])
        assert all(bool(torch.isfinite(x).all()) for x in b)


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("family", ["poisson", "bernoulli", "gaussian"])
def test_an_absent_entry_of_ys_is_never_read(family, T):
    d, obs, P = 5, 3, 41
    t = _general(d, obs, T, P=P, seed=2)
    if family == "bernoulli":
        t["ys"] = (t["ys"] > 1).to(T)
    if family == "gaussian":
        t["extra"] = t["extra"].abs() + 0.1
    g = {k: v.cuda() for k, v in t.items()}
    clean = _hip_call(family, g["zm"], g["zc"], g["ys"], g["observed"], g["offset"], g["extra"], g["Bm"])
    ys = torch.where(g["observed"], g["ys"], torch.full_like(g["ys"], float("nan")))
    assert bool(torch.isnan(ys).any())
    nan = _hip_call(family, g["zm"], g["zc"], ys, g["observed"], g["offset"], g["extra"], g["Bm"])
    for k in range(5):
        assert torch.equal(clean[k], nan[k]), NAMES[k]
        assert bool(torch.isfinite(nan[k]).all())
    assert bool((nan[4][~g["observed"]] == 0).all()) and bool((nan[4][g["observed"]] != 0).all())
    # and a NaN that IS read comes out as NaN: nothing hides it
    seen = _hip_call(family, g["zm"], g["zc"], ys, None, g["offset"], g["extra"], g["Bm"])
    assert bool(torch.isnan(seen[4][~g["observed"]]).all()) and torch.equal(seen[4][g["observed"]], clean[4][g["observed"]])


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("family", ["poisson", "bernoulli", "gaussian"])
def test_a_rounding_negative_variance_is_clamped(family, T):
    """B S B^T = 2 - 2 (1 + 4 eps) < 0 in exact and in floating-point arithmetic: eta_var is 0, everything finite"""
    eps = float(torch.finfo(T).eps)
    off = -(1.0 + 4 * eps)
    zc = torch.tensor([[[1.0, off], [off, 1.0]]], dtype=T).cuda()
    zm = torch.tensor([[0.3, -0.1]], dtype=T).cuda()
    Bm = torch.ones(1, 2, dtype=T).cuda()
    assert float((Bm.cpu().to(F64) @ zc.cpu().to(F64)[0] @ Bm.cpu().to(F64).T)) < 0
    ys = torch.ones(1, 1, dtype=T).cuda()
    extra = torch.full((1, 1), 0.5, dtype=T).cuda()
    out = _hip_call(family, zm, zc, ys, None, None, extra, Bm)
    assert float(out[1]) == 0.0
    assert all(bool(torch.isfinite(x).all()) for x in out)
    at0 = _hip_call(family, zm, torch.zeros_like(zc), ys, None, None, extra, Bm)
    for k in range(5):
        assert torch.equal(out[k], at0[k]), NAMES[k]


@pytest.mark.gpu
@DTYPES
def test_the_bernoulli_tails_mirror_each_other(T):
    """mu = +-40, v = 0.25: P(y = 1) at -40 is P(y = 0) at +40, var is the same and positive, and the log densities
    mirror: exp(L1 + L0) keeps what p (1 - p) would lose"""
    eps = float(torch.finfo(T).eps)
    cases = [(1.0, 40.0, 0.25), (0.0, -40.0, 0.25), (0.0, 40.0, 0.25), (1.0, -40.0, 0.25)]
    ops, _ = _columns("bernoulli", cases, T)
    _, _, mean, var, lp = [t.cpu().to(F64).reshape(-1) for t in _hip_call("bernoulli", *[None if t is None else t.cuda() for t in ops])]
    near, far = gp.outputs("bernoulli", 1.0, 40.0, 0.25), gp.outputs("bernoulli", 0.0, 40.0, 0.25)
    scale = 64 * eps * (1 + near["eta_max"])          # each side is within scale x S of the rule, so two sides within twice that
    assert float(var[0]) > 0 and float(var[1]) > 0 and abs(float(var[0]) - float(var[1])) <= 2 * scale * near["var"][1]
    assert abs(float(var[0]) - near["var"][0]) <= scale * near["var"][1]
    assert abs(float(lp[0]) - float(lp[1])) <= 2 * scale * near["logpdf"][1]
    assert abs(float(lp[2]) - float(lp[3])) <= 2 * scale * far["logpdf"][1]
    assert float(mean[0]) == 1.0 and 0 < float(mean[1]) < 1e-16
    assert abs(float(mean[1]) - float(torch.exp(lp[2]))) <= 2 * scale * float(mean[1]) * (1 + far["logpdf"][1])      # P(1 | -40) = P(0 | +40)


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("family", ["poisson", "bernoulli"])
def test_a_row_does_not_depend_on_its_place(family, T):
    """a permutation of the rows, and a subset of them (other block boundaries, another P), give every row the same bits"""
    d, obs, P = 5, 3, 300                            # 900 entries: four workgroups, the last one partial
    t = _general(d, obs, T, P=P, seed=3)
    if family == "bernoulli":
        t["ys"] = (t["ys"] > 1).to(T)
    g = {k: v.cuda() for k, v in t.items()}
    rows = ("zm", "zc", "ys", "observed", "extra")
    call = lambda q: _hip_call(family, q["zm"], q["zc"], q["ys"], q["observed"], g["offset"], q["extra"], g["Bm"])      # noqa: E731
    base = call(g)
    gen = torch.Generator().manual_seed(5)
    perm = torch.randperm(P, generator=gen).cuda()
    for idx in (perm, perm[:97]):
        sub = call({k: g[k][idx].contiguous() for k in rows})
        for k in range(5):
            assert torch.equal(sub[k], base[k][idx]), NAMES[k]


@pytest.mark.gpu
def test_no_rows_touch_nothing():
    buf = torch.full((64,), 7.0, dtype=F64).cuda()
    p = ctypes.c_void_p(buf.data_ptr())
    rc = _hip.lib().cgps_leg_glm_predict(p, p, p, None, None, None, p, 0, 3, 2, _hip.F64, _hip.GLM_POISSON, p, p, p, p, p,
                                         _hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and bool((buf == 7.0).all())
    out = leg._glm_predict_hip(_hip.GLM_POISSON, torch.empty(0, 3, dtype=F64).cuda(), torch.empty(0, 3, 3, dtype=F64).cuda(), None, None,
                               None, None, torch.ones(2, 3, dtype=F64).cuda())
    assert [tuple(x.shape) for x in out[:4]] == [(0, 2)] * 4 and out[4] is None

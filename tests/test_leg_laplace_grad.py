"""Gradients of the Laplace evidence (leg.laplace_posterior_batch(differentiable=True)) against the dense
fp64 truth of tests/_laplacegradref.py, the two entries of include/cgps_glm_grad.h called directly, and the contract of
the Python call.  The CPU test at the top pins where the declarations live."""
import ctypes
import types

import pytest
import torch

import _laplacegradref as gr
from cyclic_gps import _hip, leg
from test_leg_laplace import _composed, _declared, _ragged

F64, F32 = torch.float64, torch.float32
EPS32 = float(torch.finfo(F32).eps)
RTOL64, ATOL64 = 1e-7, 1e-9                    # the bounds of tests/test_leg_laplace.py and the filter tests
GRADS = ("N", "R", "B", "offset", "extra", "ts")


# ---- CPU: where the declarations live ----------------------------------------------------------------------------------
def test_the_gradient_header_declares_what_the_library_exports():
    names = ["cgps_leg_glm_evidence_adjoint", "cgps_leg_glm_evidence_rhs"]
    assert _declared("cgps_glm_grad.h") == names
    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert all(hasattr(lib, n) for n in names)
    assert _hip.glm_gradient_symbols() == names
    # the two older tables and the version are what they were
    assert _declared("cgps_glm.h") == ["cgps_leg_glm_step"] and _hip.extension_symbols() == ["cgps_leg_glm_step"]
    assert sorted(_hip.exported_symbols()) == _declared("cgps.h")
    assert not set(names) & set(_hip.exported_symbols())
    assert _hip.lib().cgps_version() == 320
    # calls without operands are refused by name, on the host
    L = _hip.lib()
    assert L.cgps_leg_glm_evidence_rhs(*[None] * 7, 4, 2, 2, _hip.F64, _hip.GLM_POISSON, None, None) == 1
    assert b"cgps_leg_glm_evidence_rhs: z = NULL" in L.cgps_last_error()
    assert L.cgps_leg_glm_evidence_adjoint(*[None] * 13, 1, 4, 2, 2, _hip.F64, _hip.GLM_POISSON, *[None] * 6) == 1
    assert b"cgps_leg_glm_evidence_adjoint: z = NULL" in L.cgps_last_error()
    assert L.cgps_leg_glm_evidence_adjoint(*[None] * 13, 1, 4, 2, 9, _hip.F64, _hip.GLM_POISSON, *[None] * 6) == 3     # obs = 9: CGPS_ERR_UNSUPPORTED
    assert L.cgps_leg_glm_evidence_adjoint(*[None] * 13, 0, 4, 2, 2, _hip.F64, _hip.GLM_POISSON, *[None] * 6) == 0
    assert L.cgps_leg_glm_evidence_rhs(*[None] * 7, 0, 2, 2, _hip.F64, _hip.GLM_POISSON, None, None) == 0


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _leaves(case, dtype, which=None, nan=False):
    """(model, ts, ys, kwargs, leaves): the case on the GPU with every differentiable input a leaf that requires grad"""
    ts, ys, kw = _ragged(case, dtype, which, nan)
    leaf = lambda t: t.detach().clone().requires_grad_(True)            # noqa: E731
    obs = case.B.shape[0]
    m = leg.LEGMatrices(*(leaf(t.to(dtype).cuda()) for t in (case.N, case.R, case.B)), torch.eye(obs, dtype=dtype).cuda())
    ts = leaf(ts)
    kw["offset"] = leaf(kw["offset"])
    name = "noise_var" if case.family == "gaussian" else "log_exposure"
    kw[name] = leaf(kw[name])
    return m, ts, ys, kw, dict(N=m.N, R=m.R, B=m.B, offset=kw["offset"], extra=kw[name], ts=ts)


def _library_gradients(case, dtype, gE, which=None, nan=False, **more):
    """(the gradients of sum gE E as fp64 CPU tensors, the result of the call)"""
    m, ts, ys, kw, lv = _leaves(case, dtype, which, nan)
    r = leg.laplace_posterior_batch(m, ts, ys, differentiable=True, **kw, **more)
    (gE.cuda() * r.log_evidence).sum().backward()
    return {k: v.grad.detach().to("cpu", F64) for k, v in lv.items()}, r


REF_FLOOR = 1e-12
"""A gradient that is zero by structure (no two observed rows in any series: the evidence does not depend on N, R or ts)
comes out of the reference as rounding, some 1e-14 of the case's largest gradient entry, and its own largest entry is
then no scale.  Only there (the reference's largest entry below REF_FLOOR x the largest entry of ALL the case's
reference gradients) the library's values are asked to be below that floor too; everywhere else the bound is rtol 1e-7 /
atol 1e-9 x the gradient's largest entry and nothing more."""


def _assert_fp64(got, ref, what, cond_term=0.0):
    """``cond_term``: what rounding of the precision form adds, as a fraction of the largest entry (0 for the
    well-conditioned cases; tests/_laplacegradref.py, COND_MAX)"""
    floor = REF_FLOOR * max(float(ref[k].abs().max()) for k in GRADS)
    worst = 0.0
    for k in GRADS:
        g, w = got[k], ref[k]
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        err = (g - w).abs()
        scale = float(w.abs().max())
        print("%s d/d%s: max abs error %.3e (largest entry %.3e)" % (what, k, float(err.max()), scale))
        if scale <= floor:
            assert float(g.abs().max()) <= floor, (what, k, float(g.abs().max()), floor)
            continue
        worst = max(worst, float(err.max()) / scale)
        assert bool((err <= (ATOL64 + cond_term) * scale + RTOL64 * w.abs()).all()), (what, k, float(err.max()), scale)
    return worst


def _check_truth(case, what):
    ref = gr.gradients(case)
    got, r = _library_gradients(case, F64, ref["gE"])
    assert bool(r.converged.all())
    ev = r.log_evidence.detach().cpu()
    assert bool(((ev - ref["E"]).abs() <= ATOL64 + RTOL64 * ref["E"].abs()).all()), (ev, ref["E"])
    _assert_fp64(got, ref, what)
    return got, r


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["poisson", "bernoulli"])
@pytest.mark.parametrize("obs", gr.OBS_TRUTH)
@pytest.mark.parametrize("d", gr.RANKS_TRUTH)
def test_the_gradient_is_the_dense_truth_fp64(d, obs, family):
    _check_truth(gr.grad_case(d, obs, family, gr.LENGTHS_TRUTH), "d %d obs %d %s" % (d, obs, family))


@pytest.mark.gpu
def test_rows_across_workgroups_and_series_across_strides():
    # lengths chosen from the launch geometry: see LENGTHS_GEOMETRY in tests/_laplacegradref.py
    _check_truth(gr.grad_case(3, 2, "poisson", gr.LENGTHS_GEOMETRY, 4), "geometry")


@pytest.mark.gpu
@pytest.mark.parametrize("obs", range(1, 9))
@pytest.mark.parametrize("d", range(1, 9))
def test_every_compiled_form(d, obs):
    _check_truth(gr.grad_case(d, obs, "poisson", gr.LENGTHS_FORMS, 1), "form d %d obs %d" % (d, obs))


@pytest.mark.gpu
@pytest.mark.parametrize("d,obs", gr.FORMS_GAUSSIAN)
def test_the_gaussian_family(d, obs):
    case = gr.grad_case(d, obs, "gaussian", gr.LENGTHS_FORMS, 2)
    _check_truth(case, "gaussian d %d obs %d" % (d, obs))
    m, ts, ys, kw, _ = _leaves(case, F64)
    u = leg._laplace_saved(leg.laplace_posterior_batch(m, ts, ys, differentiable=True, **kw).log_evidence)["u"]
    assert u.numel() and bool((u == 0).all())            # w' = 0: no implicit term


def _fp32(case, what):
    """max(4 x the error of the torch-composed backward in fp32, 64 eps32 x the largest entry), the step kernel's rule"""
    ref = gr.gradients(case)
    got, r = _library_gradients(case, F32, ref["gE"])
    yard, _ = _composed(lambda: _library_gradients(case, F32, ref["gE"]))
    assert bool(r.converged.all())
    worst = 0.0
    for k in GRADS:
        w = ref[k]
        err, err_y = float((got[k] - w).abs().max()), float((yard[k] - w).abs().max())
        bound = max(4 * err_y, 64 * EPS32 * float(w.abs().max()))
        worst = max(worst, err / bound if bound > 0 else 0.0)
        print("%s d/d%s: fp32 error %.3e, composed %.3e, bound %.3e, ratio %.3f" % (what, k, err, err_y, bound, err / bound if bound else 0))
        assert err <= bound, (what, k, err, err_y, bound)
    print("%s: worst fp32 ratio %.3f" % (what, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("d,obs", gr.FORMS_FP32)
def test_the_bernoulli_family_in_fp32(d, obs):
    _fp32(gr.grad_case(d, obs, "bernoulli", gr.LENGTHS_FORMS, 3), "fp32 bernoulli d %d obs %d" % (d, obs))


@pytest.mark.gpu
@pytest.mark.parametrize("d,obs", gr.FORMS_FP32)
def test_the_poisson_family_in_fp32(d, obs):
    _fp32(gr.grad_case(d, obs, "poisson", gr.LENGTHS_FORMS, 1), "fp32 poisson d %d obs %d" % (d, obs))


@pytest.mark.gpu
@pytest.mark.parametrize("d,obs", gr.FORMS_GAUSSIAN)
def test_the_gaussian_family_in_fp32(d, obs):
    _fp32(gr.grad_case(d, obs, "gaussian", gr.LENGTHS_FORMS, 2), "fp32 gaussian d %d obs %d" % (d, obs))


@pytest.mark.gpu
def test_an_ill_conditioned_prior_loses_the_digits_rounding_takes():
    """cond(K) = 1.3e5 (tests/_laplacegradref.py, ill_conditioned_case): the precision form carries eps cond(K)^2 into the
    gradients in N, R and ts, so the bound is the fp64 one with atol (1e-9 + eps cond(K)^2) of the largest
    entry, 1.9e-6 here.  Measured on an MI355X: worst 8.3e-8 of the largest entry (dE/dN); dense LAPACK inverses of the
    same blocks on the CPU: 1.6e-8."""
    case = gr.ill_conditioned_case()
    cond = gr.prior_condition(case)
    ref = gr.gradients(case)
    got, r = _library_gradients(case, F64, ref["gE"])
    assert bool(r.converged.all())
    worst = _assert_fp64(got, ref, "ill-conditioned", float(torch.finfo(F64).eps) * cond * cond)
    print("ill-conditioned: cond(K) %.3e, worst error / largest entry %.3e" % (cond, worst))


@pytest.mark.gpu
def test_one_log_exposure_per_row_gets_the_sum_over_its_channels():
    case = gr.grad_case(3, 3, "poisson", gr.LENGTHS_TRUTH)
    gE = gr.cotangent(case).cuda()
    m, ts, ys, kw, _ = _leaves(case, F64)
    with torch.no_grad():
        per_row = kw["log_exposure"][:, 0].clone()
    full = per_row[:, None].expand(-1, ys.shape[1]).clone().requires_grad_(True)
    per_row.requires_grad_(True)
    grads = []
    for le in (full, per_row):
        r = leg.laplace_posterior_batch(m, ts, ys, differentiable=True, **dict(kw, log_exposure=le))
        g, gB = torch.autograd.grad((gE * r.log_evidence).sum(), [le, m.B])
        grads.append((g, gB, r.log_evidence.detach()))
    assert grads[1][0].shape == per_row.shape and float(grads[1][0].abs().max()) > 0
    assert torch.equal(grads[0][2], grads[1][2]) and torch.equal(grads[0][1], grads[1][1])
    assert torch.equal(grads[1][0], grads[0][0].sum(-1))
    # dense layout: [B, n] beside ys [B, n, obs]
    dense = gr.ascent_case()
    B, n = len(dense.series), dense.lengths[0]
    md, tsd, ysd, kwd, _ = _leaves(dense, F64)
    obs = ysd.shape[1]
    le = kwd["log_exposure"].detach()[:, 0].reshape(B, n).clone().requires_grad_(True)
    rd = leg.laplace_posterior_batch(md, tsd.detach().reshape(B, n), ysd.reshape(B, n, obs), family="poisson",
                                     observed=kwd["observed"].reshape(B, n, obs), offset=kwd["offset"], log_exposure=le,
                                     differentiable=True)
    g, = torch.autograd.grad(rd.log_evidence.sum(), le)
    assert g.shape == (B, n) and float(g.abs().max()) > 0


@pytest.mark.gpu
def test_a_dropped_series_writes_zeros_whatever_its_operands_hold():
    """gE = 0 is selected, not multiplied: NaN in the mode, the solve and the blocks of such a series reaches no output"""
    case = gr.grad_case(3, 3, "poisson", gr.LENGTHS_TRUTH)
    gE = gr.cotangent(case).clone()
    gE[2] = 0.0
    m, ts, ys, kw, _ = _leaves(case, F64)
    sv = leg._laplace_saved(leg.laplace_posterior_batch(m, ts, ys, differentiable=True, **kw).log_evidence)
    op = sv["op"]
    off = op.plan.offsets.cpu().tolist()
    names = ("z", "u", "Sd", "So", "Pd", "Po")
    clean = leg._glm_evidence_adjoint_hip(op, *(sv[k] for k in names), gE.cuda())
    bad = {k: sv[k].clone() for k in names}
    for k in names:
        bad[k][off[2]:off[3] - (1 if k in ("So", "Po") else 0)] = float("nan")
    for fn in (leg._glm_evidence_adjoint_hip, leg._glm_evidence_adjoint_composed):
        got = fn(op, *(bad[k] for k in names), gE.cuda())
        assert all(bool(torch.isfinite(t).all()) for t in got), fn.__name__
        rows = slice(off[2], off[3])
        assert all(bool((t == 0).all()) for t in (got[0][rows], got[1][off[2]:off[3] - 1], got[2][rows], got[3][2], got[4][2]))
        if fn is leg._glm_evidence_adjoint_hip:
            assert all(torch.equal(a, b) for a, b in zip(got, clean))


# ---- each entry called directly ----------------------------------------------------------------------------------------
def _entry_formulas(sv, family, gE):
    """The formulas of DESIGN 4.27 entry by entry in fp64 on the CPU, from the operands the forward produced"""
    op = sv["op"]
    c = lambda t: None if t is None else t.detach().to("cpu", F64)      # noqa: E731
    z, u, Sd, So, Pd, Po, ys, Bm = (c(t) for t in (sv["z"], sv["u"], sv["Sd"], sv["So"], sv["Pd"], sv["Po"], op.ys, op.Bm))
    offset, extra, mask = c(op.offset), c(op.extra), op.observed.cpu()
    off = op.plan.offsets.cpu().tolist()
    R, d = z.shape
    obs = Bm.shape[0]
    s = torch.zeros(R, d, dtype=F64)
    gRs, gOs = torch.zeros(R, d, d, dtype=F64), torch.zeros(R - 1, d, d, dtype=F64)
    g_extra = torch.zeros(R, obs, dtype=F64)
    gB, goff = torch.zeros(len(off) - 1, obs, d, dtype=F64), torch.zeros(len(off) - 1, obs, dtype=F64)
    for b in range(len(off) - 1):
        for i in range(off[b], off[b + 1]):
            gRs[i] = gE[b] * (0.5 * (Pd[i] - Sd[i]) - 0.5 * torch.outer(z[i], z[i])
                              - 0.5 * (torch.outer(u[i], z[i]) + torch.outer(z[i], u[i])))
            if i + 1 < off[b + 1]:
                gOs[i] = gE[b] * (Po[i] - So[i] - torch.outer(z[i + 1], z[i]) - torch.outer(u[i + 1], z[i])
                                  - torch.outer(z[i + 1], u[i]))
            for ch in range(obs):
                if not mask[i, ch]:
                    continue
                eta = Bm[ch] @ z[i] + offset[ch] + (extra[i, ch] if family != "gaussian" else 0.0)
                y = ys[i, ch]
                v = Bm[ch] @ Sd[i] @ Bm[ch]
                if family == "poisson":
                    g, w, wp = y - torch.exp(eta), torch.exp(eta), torch.exp(eta)
                elif family == "bernoulli":
                    p = torch.sigmoid(eta)
                    g, w, wp = y - p, p * (1 - p), p * (1 - p) * (1 - 2 * p)
                else:
                    sv_ = extra[i, ch]
                    g, w, wp = (y - eta) / sv_, 1 / sv_, 0.0
                s[i] += -0.5 * wp * v * Bm[ch]
                e = g - 0.5 * wp * v - w * (Bm[ch] @ u[i])
                if family == "gaussian":
                    g_extra[i, ch] = gE[b] * (0.5 * (y - eta) ** 2 / sv_ ** 2 - 0.5 / sv_ + 0.5 * v / sv_ ** 2)
                else:
                    g_extra[i, ch] = gE[b] * e
                goff[b, ch] += gE[b] * e
                gB[b, ch] += gE[b] * (e * z[i] + g * u[i] - w * (Sd[i] @ Bm[ch]))
    return s, (gRs, gOs, g_extra, gB, goff)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["poisson", "bernoulli", "gaussian"])
def test_each_entry_against_its_formulas(family):
    case = gr.grad_case(3, 3, family, gr.LENGTHS_TRUTH, 2 if family == "gaussian" else 0)
    gE = gr.cotangent(case)
    m, ts, ys, kw, _ = _leaves(case, F64, nan=True)      # NaN at every unobserved entry of ys, log_exposure, noise_var
    r = leg.laplace_posterior_batch(m, ts, ys, differentiable=True, **kw)
    sv = leg._laplace_saved(r.log_evidence)
    op = sv["op"]
    s_want, want = _entry_formulas(sv, family, gE)
    s = leg._glm_evidence_rhs_hip(op, sv["z"], sv["Sd"]).cpu()
    got = [t.cpu().to(F64) for t in leg._glm_evidence_adjoint_hip(op, sv["z"], sv["u"], sv["Sd"], sv["So"], sv["Pd"], sv["Po"],
                                                                 gE.cuda())]
    names = ("gRs", "gOs", "g_extra", "gB_part", "goffset_part")
    for name, g, w in [("s", s, s_want)] + list(zip(names, got, want)):
        assert g.shape == w.shape and bool(torch.isfinite(g).all()), name
        err, scale = float((g - w).abs().max()), float(w.abs().max())
        print("%s %s: max abs error %.3e (largest entry %.3e)" % (family, name, err, scale))
        assert bool(((g - w).abs() <= 1e-12 * scale + 1e-11 * w.abs()).all()), (name, err, scale)
    off = op.plan.offsets.cpu().tolist()
    for k in off[1:-1]:
        assert bool((got[1][k - 1] == 0).all()), "gOs between two series"
    mask = op.observed.cpu()
    assert bool((got[2][~mask] == 0).all()), "g_extra at unobserved entries"
    assert bool((s[~mask.any(1)] == 0).all()), "s where a row observes nothing"
    if family == "gaussian":
        assert bool((s == 0).all())


@pytest.mark.gpu
def test_a_series_does_not_depend_on_its_neighbours():
    """the adjoint entry on a series' own rows of the operands, alone, against the same rows inside the batch"""
    case = gr.grad_case(3, 3, "poisson", gr.LENGTHS_TRUTH)
    gE = gr.cotangent(case).clone()
    gE[2] = 0.0                                          # the series of six rows: exact zeros
    m, ts, ys, kw, _ = _leaves(case, F64)
    sv = leg._laplace_saved(leg.laplace_posterior_batch(m, ts, ys, differentiable=True, **kw).log_evidence)
    op = sv["op"]
    batch = leg._glm_evidence_adjoint_hip(op, *(sv[k] for k in ("z", "u", "Sd", "So", "Pd", "Po")), gE.cuda())
    off = op.plan.offsets.cpu().tolist()
    for b in range(len(case.series)):
        rows, links = slice(off[b], off[b + 1]), slice(off[b], off[b + 1] - 1)
        cut = lambda t, sl: t[sl].clone()                # noqa: E731  (a copy: aligned, and nothing of the neighbours behind it)
        plan1 = types.SimpleNamespace(offsets=torch.tensor([0, off[b + 1] - off[b]], dtype=torch.int64).cuda(), B=1)
        op1 = leg._GlmOperands(plan1, None, None, cut(op.ys, rows), None, op.offset, cut(op.extra, rows), op.Bm, op.family, op.tol)
        op1.pattern = cut(op.pattern, rows)
        alone = leg._glm_evidence_adjoint_hip(op1, cut(sv["z"], rows), cut(sv["u"], rows), cut(sv["Sd"], rows), cut(sv["So"], links),
                                              cut(sv["Pd"], rows), cut(sv["Po"], links), gE[b:b + 1].cuda())
        assert torch.equal(alone[0], batch[0][rows]) and torch.equal(alone[2], batch[2][rows]), b
        assert torch.equal(alone[1], batch[1][links]), b
        assert torch.equal(alone[3][0], batch[3][b]) and torch.equal(alone[4][0], batch[4][b]), b
    rows = slice(off[2], off[3])
    assert all(bool((t == 0).all()) for t in (batch[0][rows], batch[1][off[2]:off[3] - 1], batch[2][rows], batch[3][2], batch[4][2]))
    assert float(batch[0][off[4]:].abs().max()) > 0 and float(batch[3][4].abs().max()) > 0


# ---- the contract of the Python call -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_default_call_builds_no_graph_and_the_values_are_bit_equal():
    case = gr.grad_case(3, 3, "poisson", gr.LENGTHS_TRUTH)
    m, ts, ys, kw, _ = _leaves(case, F64)
    plain = leg.laplace_posterior_batch(m, ts, ys, **kw)
    assert not plain.log_evidence.requires_grad and plain.log_evidence.grad_fn is None
    r = leg.laplace_posterior_batch(m, ts, ys, differentiable=True, **kw)
    assert r.log_evidence.requires_grad
    assert torch.equal(r.log_evidence.detach(), plain.log_evidence)
    assert torch.equal(r.mean, plain.mean) and torch.equal(r.cov[0], plain.cov[0]) and torch.equal(r.cov[1], plain.cov[1])
    assert not (r.mean.requires_grad or r.cov[0].requires_grad or r.cov[1].requires_grad)
    r.log_evidence.sum().backward()
    with pytest.raises(RuntimeError):                    # once_differentiable, and the graph is freed: no second backward
        r.log_evidence.sum().backward()
    r2 = leg.laplace_posterior_batch(m, ts, ys, differentiable=True, **kw)
    g, = torch.autograd.grad(r2.log_evidence.sum(), m.B, create_graph=True)
    with pytest.raises(RuntimeError):                    # no second derivatives
        g.sum().backward()


@pytest.mark.gpu
def test_an_unconverged_series_raises_or_is_a_constant():
    case = gr.grad_case(3, 3, "poisson", gr.LENGTHS_TRUTH)
    ref_gE = gr.cotangent(case)
    m, ts, ys, kw, _ = _leaves(case, F64)
    probe = leg.laplace_posterior_batch(m, ts, ys, max_iter=1, **kw)
    conv = probe.converged.cpu()
    assert not bool(conv.all()) and bool(conv.any())     # the series that observes nothing has converged, others have not
    first = int(torch.nonzero(~conv)[0])
    with pytest.raises(_hip.CgpsError, match=r"series %d\b" % first):
        leg.laplace_posterior_batch(m, ts, ys, max_iter=1, differentiable=True, **kw)
    got, r = _library_gradients(case, F64, ref_gE, max_iter=1, allow_unconverged=True)
    assert torch.equal(r.log_evidence.detach(), probe.log_evidence)
    # what is left is the gradient of the converged series alone
    gE = torch.where(conv, ref_gE, torch.zeros_like(ref_gE))
    m2, ts2, ys2, kw2, lv2 = _leaves(case, F64)
    r2 = leg.laplace_posterior_batch(m2, ts2, ys2, max_iter=1, differentiable=True, allow_unconverged=True, **kw2)
    (gE.cuda() * r2.log_evidence).sum().backward()
    for k, v in lv2.items():
        assert torch.equal(v.grad.cpu().to(F64), got[k]), k
    off = [0]
    for n in case.lengths:
        off.append(off[-1] + n)
    for b in range(len(conv)):
        if not conv[b]:
            assert bool((got["ts"][off[b]:off[b + 1]] == 0).all()) and bool((got["extra"][off[b]:off[b + 1]] == 0).all()), b


@pytest.mark.gpu
def test_the_dense_layout_and_the_one_series_call_agree_with_the_ragged_call():
    case = gr.ascent_case()
    ref_gE = gr.cotangent(case)
    got, r = _library_gradients(case, F64, ref_gE)
    B, n = len(case.series), case.lengths[0]
    m, ts, ys, kw, lv = _leaves(case, F64)
    obs = ys.shape[1]
    dts = ts.detach().reshape(B, n).clone().requires_grad_(True)
    le = kw["log_exposure"].detach().reshape(B, n, obs).clone().requires_grad_(True)
    rd = leg.laplace_posterior_batch(m, dts, ys.reshape(B, n, obs), family="poisson", observed=kw["observed"].reshape(B, n, obs),
                                     offset=kw["offset"], log_exposure=le, differentiable=True)
    assert torch.equal(rd.log_evidence.detach(), r.log_evidence.detach())
    (ref_gE.cuda() * rd.log_evidence).sum().backward()
    assert dts.grad.shape == (B, n) and le.grad.shape == (B, n, obs)
    assert torch.equal(dts.grad.reshape(-1).cpu(), got["ts"]) and torch.equal(le.grad.reshape(-1, obs).cpu(), got["extra"])
    for k in ("N", "R", "B", "offset"):
        assert torch.equal(lv[k].grad.cpu(), got[k]), k
    # one series through laplace_posterior: 0-d evidence, the gradient of that series alone
    m1, ts1, ys1, kw1, lv1 = _leaves(case, F64, which=[3])
    kw1.pop("lengths")
    fam = kw1.pop("family")
    r1 = leg.laplace_posterior(m1, ts1, ys1, fam, differentiable=True, **kw1)
    # (a series alone and inside a batch meet the cyclic reduction at other places: equal to rounding, not bit for bit)
    close = lambda a, b: bool(((a - b).abs() <= ATOL64 * float(b.abs().max()) + RTOL64 * b.abs()).all())      # noqa: E731
    assert r1.log_evidence.dim() == 0 and close(r1.log_evidence.detach().cpu(), r.log_evidence[3].detach().cpu())
    r1.log_evidence.backward()
    only = torch.zeros_like(ref_gE)
    only[3] = 1.0
    want, _ = _library_gradients(case, F64, only)
    rows = slice(3 * n, 4 * n)
    assert close(lv1["ts"].grad.cpu(), want["ts"][rows]) and close(lv1["extra"].grad.cpu(), want["extra"][rows])
    assert not bool(want["ts"][:3 * n].any()) and not bool(want["extra"][4 * n:].any())     # the other series: exact zeros
    for k in ("N", "R", "B", "offset"):
        assert close(lv1[k].grad.cpu(), want[k]), k


@pytest.mark.gpu
def test_a_step_along_the_gradient_raises_the_evidence():
    case = gr.ascent_case()
    gen = torch.Generator().manual_seed(5)
    m, ts, ys, kw, lv = _leaves(case, F64)
    with torch.no_grad():                                # a perturbed model
        for k in ("N", "R", "B", "offset"):
            lv[k].add_((0.1 * torch.randn(lv[k].shape, generator=gen, dtype=F64) * (lv[k].cpu() != 0)).cuda())
    params = [lv[k] for k in ("N", "R", "B", "offset")]
    E0 = leg.laplace_posterior_batch(m, ts, ys, differentiable=True, **kw).log_evidence.sum()
    grads = torch.autograd.grad(E0, params)
    gnorm2 = float(sum((g * g).sum() for g in grads))
    assert gnorm2 > 0
    h = 1e-4 / max(1.0, gnorm2 ** 0.5)
    with torch.no_grad():
        for p, g in zip(params, grads):
            p.add_(h * g)
    E1 = leg.laplace_posterior_batch(m, ts, ys, **kw).log_evidence.sum()
    gain = float(E1) - float(E0)
    print("E0 %.6f, E1 - E0 %.3e, h |grad|^2 %.3e" % (float(E0), gain, h * gnorm2))
    assert gain > 0                                      # (to first order E1 - E0 = h |grad|^2)

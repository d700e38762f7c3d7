"""Every gradient of the library against an fp64 reference that does not run the HIP kernels (tests/_gradref.py):
a dense Cholesky with autograd, the closed-form adjoints evaluated with the CPU oracle, finite differences
(torch.autograd.gradcheck), and for the LEG log-likelihood a dense Gaussian density of the observations.

fp64 is held to rtol 1e-7 (atol 1e-10 of the largest reference entry).  fp32 is compared with the same fp64
reference, each gradient tensor to a fraction of its largest entry: the kernels round every block operation to
fp32 (eps 6e-8), and the error grows with the condition of J and the number of reduction levels."""
import itertools
import os

import numpy as np
import pytest
import torch

import _gradref as ref
import _util
from cyclic_gps import leg
import cyclic_gps.cyclic_reduction as cr

F64, F32 = torch.float64, torch.float32
N_EDGES = [1, 2, 3, 31, 32, 33, 127, 128, 129, 255, 256, 257]
# fp32 tolerances, as fractions of max |reference| per gradient tensor.  Observed worst cases over the sweeps below:
# 1.0e-6 for the CR surface (factor, solves and selected inverse rounded to fp32), 8.1e-6 for the LEG gradients
# (also the fp32 matrix exponentials of the assembly and of its adjoint); the bounds leave a 10-20x margin.
TOL32 = 2e-5
TOL32_LEG = 1e-4
DTYPE_IDS = {F64: "f64", F32: "f32"}


def _check(got, want, dtype, what, tol32=TOL32):
    want = want.detach().to("cpu", F64)
    got = torch.zeros_like(want) if got is None else got.detach().to("cpu", F64)
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    scale = float(want.abs().max()) if want.numel() else 0.0
    if dtype == F64:
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-7, atol=1e-10 * scale, err_msg=what)
    else:
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=tol32 * scale + 1e-30, err_msg=what)


def _check_value(got, want, dtype, what, tol32=1e-5):
    tol = 1e-9 if dtype == F64 else tol32
    assert abs(float(got) - float(want)) <= tol * max(abs(float(want)), 1.0), (what, float(got), float(want))


# ---- the scalars of the CR surface, each as f(Rs, Os, y) on the kernels --------------------------------------------
def _op(kind, R, O, y, u=None):
    if kind == "mahal_and_det.mahal":
        return cr.mahal_and_det(R, O, y)[0]
    if kind == "mahal_and_det.logdet":
        return cr.mahal_and_det(R, O, y)[1]
    if kind == "mahal_and_det.mix":
        m, ld = cr.mahal_and_det(R, O, y)
        return 0.7 * m - 1.3 * ld
    if kind == "det":
        return cr.det(cr.decompose(R, O))
    if kind == "solve":
        return (cr.solve(cr.decompose(R, O), y).double() * u.double()).sum()
    if kind == "mahal":
        return cr.mahal(cr.decompose(R, O), y)
    raise ValueError(kind)


def _reference(kind, N, d, m, dense=True):
    """(value, dR, dO, dy) in fp64 for _op(kind) on _gradref.cr_case(N, d)."""
    if kind == "mahal_and_det.mix":
        a, b = _reference("mahal_and_det.mahal", N, d, m, dense), _reference("mahal_and_det.logdet", N, d, m, dense)
        return tuple(0.7 * x - 1.3 * z for x, z in zip(a, b))
    base = {"mahal_and_det.mahal": "mahal", "mahal": "mahal", "mahal_and_det.logdet": "logdet", "det": "logdet",
            "solve": "solvedot"}[kind]
    if dense:
        return ref.cr_dense_ref(N, d, base, m)
    Rs, Os, Y, U = ref.cr_case(N, d)
    return ref.oracle_value_and_grads(base, Rs, Os, Y[m], U[m] if base == "solvedot" else None)


CR_KINDS = [("mahal_and_det.mahal", 1), ("mahal_and_det.logdet", 1), ("mahal_and_det.mix", 1), ("det", 1),
            ("solve", 1), ("solve", 2), ("solve", 3), ("solve", 8), ("mahal", 1), ("mahal", 3)]


def _run_cr(kind, m, N, d, dtype, device, train, dense=True):
    """Kernel value and gradients with the inputs named in `train` trainable; checks them against the reference and
    that the frozen inputs got no gradient."""
    Rs, Os, Y, U = ref.cr_case(N, d)
    want = _reference(kind, N, d, m, dense)
    R, O, y = (t.to(dtype).to(device).clone().requires_grad_(name in train)
               for t, name in zip((Rs, Os, Y[m]), ("Rs", "Os", "y")))
    u = U[m].to(dtype).to(device)
    R_in = 0.5 * (R + R.transpose(-1, -2))            # the sym map of the reference, on the kernel side too
    out = _op(kind, R_in, O, y, u)
    tag = "%s m=%d N=%d d=%d %s %s train=%s" % (kind, m, N, d, DTYPE_IDS[dtype], device, "+".join(train))
    assert out.device.type == device, tag
    _check_value(out, want[0], dtype, tag)
    out.backward()
    for name, leaf, g in zip(("Rs", "Os", "y"), (R, O, y), want[1:]):
        if name not in train:
            assert leaf.grad is None, (tag, name)
            continue
        if leaf.grad is not None:
            assert leaf.grad.device.type == device, (tag, name)
        if kind in ("det", "mahal_and_det.logdet") and name == "y":
            assert leaf.grad is None or float(leaf.grad.abs().max()) == 0.0, tag
            continue
        assert leaf.grad is not None or leaf.numel() == 0, (tag, name, "no gradient")
        _check(leaf.grad, g, dtype, "%s d/d%s" % (tag, name))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=DTYPE_IDS.get)
@pytest.mark.parametrize("d", range(1, 9))
@pytest.mark.parametrize("N", N_EDGES)
def test_cr_gradients_against_dense_reference(N, d, dtype):
    """mahal_and_det (each output and a mix), det(decompose), solve(decompose) with 1, 2, 3 and 8 right-hand sides and
    mahal(decompose) with 1 and 3: value and gradients in Rs, Os and y, all trainable."""
    for kind, m in CR_KINDS:
        train = ("Rs", "Os") if kind == "det" else ("Rs", "Os", "y")
        _run_cr(kind, m, N, d, dtype, "cuda", train)
    Rs, Os, Y, _ = ref.cr_case(N, d)
    dec = cr.decompose(Rs.to(dtype).cuda(), Os.to(dtype).cuda())
    for m in (1, 3):                                   # the one-kernel mahal (no gradient wanted) on the same values
        _check_value(cr.mahal(dec, Y[m].to(dtype).cuda()), ref.cr_dense_ref(N, d, "mahal", m)[0], dtype, "mahal m=%d" % m)


SUBSETS = [s for k in (1, 2, 3) for s in itertools.combinations(("Rs", "Os", "y"), k)]


@pytest.mark.gpu
@pytest.mark.parametrize("device", ["cuda", "cpu"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=DTYPE_IDS.get)
@pytest.mark.parametrize("N,d", [(1, 3), (33, 5), (128, 2), (257, 8)])
@pytest.mark.parametrize("kind,m", CR_KINDS, ids=["%s-%d" % km for km in CR_KINDS])
def test_cr_gradients_every_trainable_subset(kind, m, N, d, dtype, device):
    """Every non-empty subset of {Rs, Os, y} trainable, from GPU and from CPU callers (CPU inputs are staged, their
    gradients come back on the CPU); frozen inputs get no gradient."""
    for train in SUBSETS:
        if kind == "det" and "y" in train:
            continue
        _run_cr(kind, m, N, d, dtype, device, train)


@pytest.mark.gpu
def test_cr_gradients_above_lds_max_rows_d7():
    """d = 7 fp64 above LDS_MAX_ROWS (2^17, cgps_decompose.hip): the factorisation runs one launch per level for the
    levels above it.  At d = 7 fp64 the 256-row tile does not fit, so decompose_solve (which the backward of
    mahal_and_det runs) is cgps_decompose on that level-wise path followed by the stored-factor halfsolve and
    backsolve.  Reference: closed-form adjoints with the oracle."""
    N, d = (1 << 17) + 3, 7
    for kind, m in (("mahal_and_det.mix", 1), ("det", 1), ("solve", 1), ("mahal", 1)):
        train = ("Rs", "Os") if kind == "det" else ("Rs", "Os", "y")
        _run_cr(kind, m, N, d, F64, "cuda", train, dense=False)
    Rs, Os, Y, _ = ref.cr_case(N, d)
    with torch.no_grad():
        _, x = cr.decompose_solve(Rs.cuda(), Os.cuda(), Y[1].cuda())
    w = ref.O.solve(ref.O.decompose(Rs, Os), Y[1])
    _check(x, w, F64, "decompose_solve above LDS_MAX_ROWS")


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 2, 5, 8])
@pytest.mark.parametrize("N", [1, 2, 3, 5])
def test_gradcheck_finite_differences(N, d):
    """The adjoint formulas themselves, against central differences of the kernels' own forward (fp64, GPU).  R goes
    through the sym map: the kernels read one triangle of each diagonal block."""
    Rs, Os, Y, U = ref.cr_case(N, d)
    R, O, y, y3 = (t.cuda().clone().requires_grad_(True) for t in (Rs, Os, Y[1], Y[3]))
    u3 = U[3].cuda()
    s = ref.sym
    blocks = (R, O) if N > 1 else (R,)
    Ofix = O.detach()

    def _ro(args):
        return (s(args[0]), args[1]) if N > 1 else (s(args[0]), Ofix)

    def f_md(*a):
        return cr.mahal_and_det(*_ro(a), a[-1])

    def f_det(*a):
        return cr.det(cr.decompose(*_ro(a)))

    def f_solve(*a):
        return cr.solve(cr.decompose(*_ro(a)), a[-1]) * u3

    def f_mahal(*a):
        return cr.mahal(cr.decompose(*_ro(a)), a[-1])

    assert torch.autograd.gradcheck(f_md, blocks + (y,))
    assert torch.autograd.gradcheck(f_det, blocks)
    assert torch.autograd.gradcheck(f_solve, blocks + (y3,))
    assert torch.autograd.gradcheck(f_mahal, blocks + (y3,))


# ---- the two half-solves are each other's adjoint ------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=DTYPE_IDS.get)
@pytest.mark.parametrize("N", N_EDGES)
def test_halfsolve_backhalfsolve_adjoint_identity(N, dtype):
    """<halfsolve(dec, y), z> = <y, backhalfsolve(dec, z)> with z in the per-level (CRR) layout: L^-1 T and T^T L^-T
    are transposes of each other.  No oracle involved."""
    tol = 1e-12 if dtype == F64 else 2e-5
    for d in range(1, 9):
        Rs, Os, _, _ = ref.cr_case(N, d)
        dec = cr.decompose(Rs.to(dtype).cuda(), Os.to(dtype).cuda())
        sizes = [(k + 1) // 2 for k in _util.level_sizes(N)]
        g = torch.Generator().manual_seed(N * 10 + d)
        for nrhs in (1, 2, 8):
            shape = (N, d) if nrhs == 1 else (N, d, nrhs)
            y = torch.randn(shape, generator=g, dtype=F64)
            z = torch.randn(shape, generator=g, dtype=F64)
            hy = cr.halfsolve(dec, y.to(dtype).cuda())
            assert [t.shape[0] for t in hy] == sizes
            bz = cr.backhalfsolve(dec, list(z.to(dtype).cuda().split(sizes)))
            assert tuple(bz.shape) == shape
            hy = torch.cat(hy).double().cpu()
            bz = bz.double().cpu()
            lhs, rhs = float((hy * z).sum()), float((y * bz).sum())
            scale = float(hy.norm() * z.norm() + y.norm() * bz.norm())
            assert abs(lhs - rhs) <= tol * scale, (N, d, nrhs, lhs, rhs)


# ---- LEG one-series log-likelihood -------------------------------------------------------------------------------
LEG_PARAMS = ("N", "R", "B", "Lambda", "xs", "ts")
LEG_CONFIGS = [(5, 1, F64, True), (3, 2, F64, True), (4, 1, F32, True), (6, 1, F64, False), (8, 1, F64, False)]
LEG_SUBSETS = [s for k in range(1, 7) for s in itertools.combinations(LEG_PARAMS, k)]


def _leg_case(d, obs, seed):
    gen = torch.Generator().manual_seed(seed)
    # diagonal of N at least 0.9 and a small strictly lower part: the symmetric part of G stays well away from
    # singular, so the PEG precision (and with it every gradient in G and ts) is well conditioned
    Nm = torch.tril(0.2 / d ** 0.5 * torch.randn(d, d, generator=gen, dtype=F64), -1) + \
        torch.diag(0.9 + 0.3 * torch.rand(d, generator=gen, dtype=F64))
    Rm = torch.tril(0.3 * torch.randn(d, d, generator=gen, dtype=F64), -1)
    Bm = 0.7 * torch.randn(obs, d, generator=gen, dtype=F64)
    Lm = torch.tril(0.2 * torch.randn(obs, obs, generator=gen, dtype=F64)) + 0.6 * torch.eye(obs, dtype=F64)
    n = 30 + seed % 31
    ts = 3.0 + torch.cumsum(0.2 + torch.rand(n, generator=gen, dtype=F64), 0)
    xs = torch.randn(n, obs, generator=gen, dtype=F64)
    return [Nm, Rm, Bm, Lm, xs, ts]


_leg_refs = {}


def _leg_ref(d, obs):
    key = (d, obs)
    if key not in _leg_refs:
        case = _leg_case(d, obs, 100 + 10 * d + obs)
        Nm, Rm, Bm, Lm, xs, ts = case
        _leg_refs[key] = case, ref.leg_dense_value_and_grads(Nm, Rm, Bm, Lm, ts, xs)
    return _leg_refs[key]


@pytest.mark.gpu
@pytest.mark.parametrize("d,obs,dtype,fused", LEG_CONFIGS,
                         ids=["d%do%d_%s_%s" % (d, o, DTYPE_IDS[t], "fused" if f else "unfused")
                              for d, o, t, f in LEG_CONFIGS])
def test_leg_value_and_path(d, obs, dtype, fused):
    """Without a gradient the configuration takes the path named in its id, and its value is the dense density's."""
    case, (ll, _) = _leg_ref(d, obs)
    p = [t.to(dtype).cuda() for t in case]
    m = leg.LEGMatrices(*p[:4])
    assert leg.fused_supported(p[5], m.G) == fused
    with torch.no_grad():
        _check_value(leg.log_likelihood(m, p[5], p[4]), ll, dtype, "ll", tol32=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("train", LEG_SUBSETS, ids=["+".join(s) for s in LEG_SUBSETS])
@pytest.mark.parametrize("d,obs,dtype,fused", LEG_CONFIGS,
                         ids=["d%do%d_%s_%s" % (d, o, DTYPE_IDS[t], "fused" if f else "unfused")
                              for d, o, t, f in LEG_CONFIGS])
def test_leg_gradients_against_dense_density(d, obs, dtype, fused, train):
    """leg.log_likelihood with the parameters in `train` trainable and the others frozen: value and every wanted
    gradient against autograd through the dense Gaussian density; frozen parameters get no gradient."""
    case, (ll, grads) = _leg_ref(d, obs)
    p = [t.to(dtype).cuda().requires_grad_(name in train) for t, name in zip(case, LEG_PARAMS)]
    m = leg.LEGMatrices(*p[:4])
    out = leg.log_likelihood(m, p[5], p[4])
    _check_value(out, ll, dtype, "ll", tol32=1e-5)
    out.backward()
    for name, leaf, want in zip(LEG_PARAMS, p, grads):
        if name not in train:
            assert leaf.grad is None, name
            continue
        assert leaf.grad is not None, "d ll / d %s is missing" % name
        _check(leaf.grad, want, dtype, "d ll / d %s" % name, tol32=TOL32_LEG)


@pytest.mark.gpu
def test_leg_fixture_gradients_with_N_and_R_frozen():
    """The reference's recorded training gradient (leg_co2like.npz), with N and R frozen: the partial derivatives in
    B and Lambda do not depend on which other parameters train (tolerances as in test_autograd.py)."""
    g = np.load(os.path.join(_util.GOLDEN, "leg_co2like.npz"))
    t = lambda k: torch.from_numpy(g[k]).cuda()     # noqa: E731
    N, R = t("N"), t("R")
    B, L = (t(k).requires_grad_(True) for k in ("B", "Lambda"))
    ll = leg.log_likelihood(leg.LEGMatrices(N, R, B, L), t("ts"), t("xs"))
    assert abs(float(ll) - float(g["grad_ll"])) <= 1e-8 * abs(float(g["grad_ll"]))
    ll.backward()
    scale = max(1.0, np.abs(g["gB"]).max())
    assert B.grad is not None and L.grad is not None
    np.testing.assert_allclose(B.grad.cpu().numpy(), g["gB"], rtol=1e-5, atol=1e-6 * scale)
    np.testing.assert_allclose(L.grad.cpu().numpy(), g["gLambda"], rtol=1e-5, atol=1e-6 * scale)


# ---- entry points that build no graph -----------------------------------------------------------------------------
NO_GRAPH = [cr.halfsolve, cr.backhalfsolve, cr.inverse_blocks, cr.decompose_step, leg.leg_mahal_and_det,
            leg.leg_loglik_reductions, leg.insample_posterior]


@pytest.mark.parametrize("fn", NO_GRAPH, ids=lambda f: f.__name__)
def test_no_graph_entry_points_say_so(fn):
    assert "no autograd graph" in fn.__doc__.lower()


@pytest.mark.gpu
def test_no_graph_entry_points_return_no_graph():
    Rs, Os, Y, _ = ref.cr_case(33, 4)
    R, O, y = (t.cuda().requires_grad_(True) for t in (Rs, Os, Y[1]))
    dec = cr.decompose(R, O)
    hs = cr.halfsolve(dec, y)
    assert not any(t.requires_grad for t in hs)
    assert not cr.backhalfsolve(dec, [t.clone().requires_grad_(True) for t in hs]).requires_grad
    assert not any(t.requires_grad for t in cr.inverse_blocks(dec))
    (_, D, F, G), (Rn, On) = cr.decompose_step(R, O)
    assert not any(t.requires_grad for t in (D, F, G, Rn, On))
    case = _leg_case(3, 1, 5)
    p = [t.cuda().requires_grad_(True) for t in case]
    m = leg.LEGMatrices(*p[:4])
    A = m.B.T @ m.LLT_inv @ m.B
    v = leg.compute_v(m, p[4])
    assert not any(t.requires_grad for t in leg.leg_mahal_and_det(p[5], m.G, A, v))
    assert not any(t.requires_grad for t in leg.leg_loglik_reductions(p[5], m.G, A, v))
    mean, (cRs, cOs) = leg.insample_posterior(m, p[5], p[4])
    assert mean.requires_grad
    assert not cRs.requires_grad and not cOs.requires_grad


@pytest.mark.gpu
def test_decompose_solve_is_differentiable_when_asked():
    Rs, Os, Y, U = ref.cr_case(65, 3)
    R, O, y = (t.cuda().requires_grad_(True) for t in (Rs, Os, Y[1]))
    dec, x = cr.decompose_solve(ref.sym(R), O, y)
    (x * U[1].cuda()).sum().backward()
    _, gR, gO, gy = ref.cr_dense_ref(65, 3, "solvedot", 1)
    _check(ref.sym(R.grad), gR, F64, "dR")
    _check(O.grad, gO, F64, "dO")
    _check(y.grad, gy, F64, "dy")
    with torch.no_grad():
        _, x0 = cr.decompose_solve(R, O, y)
    assert not x0.requires_grad
    np.testing.assert_allclose(x0.cpu().numpy(), x.detach().cpu().numpy(), rtol=1e-12, atol=1e-14)


# ---- the references themselves, pinned on the CPU ------------------------------------------------------------------
def test_references_match_recorded_reference_autograd():
    """The dense and the oracle closed-form references against gradients recorded from the reference's own autograd
    (grad_d3_n37.npz), before any GPU comparison relies on them.  The reference leaves dR unsymmetrised."""
    g = np.load(os.path.join(_util.GOLDEN, "grad_d3_n37.npz"))
    Rs, Os, v, w = (torch.from_numpy(g[k]) for k in ("Rs", "Os", "v", "w"))
    T = dict(rtol=1e-8, atol=1e-10)
    for kind, name in (("mahal", "mahal"), ("logdet", "logdet"), ("solvedot", "solvedot")):
        for fn in (ref.dense_value_and_grads, ref.oracle_value_and_grads):
            val, gR, gO, gy = fn(kind, Rs, Os, v, w if kind == "solvedot" else None)
            assert abs(float(val) - float(g[name])) <= 1e-10 * abs(float(g[name])), (fn.__name__, kind)
            want_R = g["g_%s_R" % name]
            np.testing.assert_allclose(gR.numpy(), 0.5 * (want_R + want_R.transpose(0, 2, 1)), **T)
            np.testing.assert_allclose(gO.numpy(), g["g_%s_O" % name], **T)
            want_v = g["g_%s_v" % name] if "g_%s_v" % name in g.files else np.zeros_like(g["v"])
            np.testing.assert_allclose(gy.numpy(), want_v, **T)


def test_references_agree_at_many_right_hand_sides():
    """Dense and oracle references agree with each other for [N, d, m] right-hand sides and at an odd size."""
    for kind, m in (("mahal", 3), ("solvedot", 8), ("logdet", 1)):
        Rs, Os, Y, U = ref.cr_case(37, 4)
        a = ref.cr_dense_ref(37, 4, kind, m)
        b = ref.oracle_value_and_grads(kind, Rs, Os, Y[m], U[m])
        for x, y in zip(a, b):
            np.testing.assert_allclose(x.numpy(), y.numpy(), rtol=1e-9, atol=1e-12 * float(y.abs().max()))


def test_leg_dense_density_matches_recorded_training_gradient():
    """The dense LEG density and its autograd against the reference's recorded log-likelihood and training gradient
    (leg_co2like.npz: 502 rows, rank 5)."""
    g = np.load(os.path.join(_util.GOLDEN, "leg_co2like.npz"))
    t = lambda k: torch.from_numpy(g[k])     # noqa: E731
    ll, (gN, gR, gB, gL, _, _) = ref.leg_dense_value_and_grads(t("N"), t("R"), t("B"), t("Lambda"), t("ts"), t("xs"))
    assert abs(float(ll) - float(g["grad_ll"])) <= 1e-9 * abs(float(g["grad_ll"]))
    d = gN.shape[0]
    tril = np.tril(np.ones((d, d)), 0).astype(bool)
    stril = np.tril(np.ones((d, d)), -1).astype(bool)
    scale = max(1.0, np.abs(g["gB"]).max())
    T = dict(rtol=1e-6, atol=1e-8 * scale)
    np.testing.assert_allclose(gN.numpy()[tril], g["gN"][tril], **T)
    np.testing.assert_allclose(gR.numpy()[stril], g["gR"][stril], **T)
    np.testing.assert_allclose(gB.numpy(), g["gB"], **T)
    np.testing.assert_allclose(gL.numpy(), g["gLambda"], **T)

"""A dense fp64 truth for the GRADIENT of the Laplace evidence (leg.laplace_posterior_batch(differentiable=True),
DESIGN.md 4.27).  It shares no kernel and no precision block with the library: the prior enters through its dense
covariance Sigma = ``_gapref.prior_covariance(ts, G)`` with G built from N, R inside the graph, K = Sigma^-1 by a dense
inverse.  torch ops on CPU tensors only.

    mode      detached undamped Newton iterations on psi(z) = sum l(y, H z + shift) - 1/2 z^T K z, from the mode of
              ``_laplaceref.truth`` (a covariance-form iteration of its own), until the step is below 1e-12
    one step  z1 = z0 + J(z0)^-1 (H^T g(z0) - K z0) WITH a graph, z0 detached: at the mode the value of z1 is z0 and its
              derivative in every parameter is -J^-1 d(grad psi)/d theta, the exact implicit derivative of the mode
    evidence  E = sum l(y, H z1 + shift) - 1/2 z1^T K z1 + 1/2 log|K| - 1/2 log|J(z1)|, every term of log p included
    gradient  torch.autograd.grad of sum_b gE_b E_b in N, R, B, offset, log_exposure / noise_var, ts

The cases of tests/test_leg_laplace_grad.py are drawn here too, so that tests/test_laplacegradref.py can hold the truth
to its own checks (finite differences, the Gaussian closed form, convergence) on exactly the inputs the GPU tests use."""
import functools
import math

import torch

import _gapref
import _laplaceref as lref

F64 = torch.float64
NEWTON_TOL = 1e-12          # above the rounding of a Newton step at rank 6..8 (2.4e-13 measured), far below any bound here
NEWTON_MAX = 50

LENGTHS_TRUTH = (1, 2, 6, 3, 131)
LENGTHS_FORMS = (1, 2, 6, 3)
# the launch geometry of csrc/cgps_leg_glm_grad.h: the row kernels take 256 rows per workgroup (GLM_GRAD_THREADS), the
# reduction wave strides a series 64 rows at a time (GLM_THREADS).  325 rows = one full workgroup and 69 rows of a second;
# the series of 257 rows starts at row 1, crosses the workgroup boundary, and takes five strides of the wave, the last of
# one row; the series of 65 rows takes two.
LENGTHS_GEOMETRY = (1, 257, 2, 65)
RANKS_TRUTH, OBS_TRUTH = (1, 3, 5, 8), (1, 3, 8)
FORMS_FP32 = ((1, 1), (3, 2), (5, 3), (8, 8))
FORMS_GAUSSIAN = ((1, 1), (3, 2), (5, 3), (8, 8))


# ---- the cases ---------------------------------------------------------------------------------------------------------
COND_MAX = 3e3
"""The library works in precision form: the gradient contracts 1/2 (K^-1 - J^-1) with dK / d(G, ts).  Rounding of K
(eps |K|) comes back through K^-1 as eps cond(K) |K^-1| and through dK as another factor cond(K): the gradient in G and
ts carries about eps cond(K)^2 of its size, whoever evaluates those formulas in fp64 (dense LAPACK inverses of the same
blocks lose the same digits).  The GPU tests bound fp64 at atol 1e-9 of the largest entry, which rounding alone allows
only for eps cond(K)^2 <= 1e-9: cond(K) <= 3e3.  A draw whose prior is worse conditioned than that in any series is
drawn again (a property of the inputs; tests/test_laplacegradref.py asserts it)."""


def prior_condition(case):
    """the largest 2-norm condition number of a series' prior covariance (= that of its precision K)"""
    G = case.G
    return max(float(torch.linalg.cond(_gapref.prior_covariance(sr["ts"], G))) for sr in case.series)


def _draw_case(d, obs, family, lengths, seed):
    gen = torch.Generator().manual_seed(seed)
    N, R, B = lref.draw_model(d, obs, gen)
    offset = torch.rand(obs, generator=gen, dtype=F64)
    G = N @ N.T + R - R.T + 1e-5 * torch.eye(d, dtype=F64)
    series = []
    for n in lengths:
        sr = lref.draw_series(n, G, B, offset, family, gen, exposure=(family != "gaussian"))
        if n == 6:
            sr["mask"][2] = False
        if n == 3:
            sr["mask"][:] = False
        series.append(sr)
    return lref.Case(family, N, R, B, offset, series)


@functools.lru_cache(maxsize=None)
def grad_case(d, obs, family, lengths, seed=0):
    """``_laplaceref.batch_case`` with a log_exposure for both count and binary data: offsets in [0, 1]; a series of six
    rows has its row 2 wholly unobserved, a series of three rows observes nothing at all.  The first of up to 50 draws
    whose ``prior_condition`` is at most COND_MAX."""
    base = 50000 + 1000 * seed + 100 * d + 10 * obs + lref.FAMILIES.index(family)
    for attempt in range(50):
        case = _draw_case(d, obs, family, lengths, base + 100000 * attempt)
        if prior_condition(case) <= COND_MAX:
            return case
    raise RuntimeError("no draw with a prior condition number <= %g" % COND_MAX)


@functools.lru_cache(maxsize=None)
def ill_conditioned_case():
    """The first draw of the rank 6, obs 2 form case, which ``grad_case`` passes over: cond(K) = 1.3e5 in its series of two
    rows.  Kept so that the library's accuracy outside well-conditioned priors stays on record and bounded."""
    case = _draw_case(6, 2, "poisson", LENGTHS_FORMS, 50000 + 1000 * 1 + 100 * 6 + 10 * 2)
    assert prior_condition(case) > 30 * COND_MAX
    return case


def cotangent(case, seed=0):
    """gE [B]: random, of both signs, none near zero"""
    gen = torch.Generator().manual_seed(7 + seed)
    B = len(case.series)
    g = 0.5 + torch.rand(B, generator=gen, dtype=F64)
    return g * (1 - 2 * (torch.arange(B) % 2)).to(F64) * (1.0 if seed % 2 == 0 else -1.0)


def all_cases():
    """(name, case) of every input of tests/test_leg_laplace_grad.py"""
    out = []
    for d in RANKS_TRUTH:
        for obs in OBS_TRUTH:
            for family in ("poisson", "bernoulli"):
                out.append(("truth-d%d-o%d-%s" % (d, obs, family), grad_case(d, obs, family, LENGTHS_TRUTH)))
    out.append(("geometry", grad_case(3, 2, "poisson", LENGTHS_GEOMETRY, 4)))
    for d in range(1, 9):
        for obs in range(1, 9):
            out.append(("forms-d%d-o%d" % (d, obs), grad_case(d, obs, "poisson", LENGTHS_FORMS, 1)))
    for d, obs in FORMS_GAUSSIAN:
        out.append(("gaussian-d%d-o%d" % (d, obs), grad_case(d, obs, "gaussian", LENGTHS_FORMS, 2)))
    for d, obs in FORMS_FP32:
        out.append(("fp32-bernoulli-d%d-o%d" % (d, obs), grad_case(d, obs, "bernoulli", LENGTHS_FORMS, 3)))
    out.append(("ascent", ascent_case()))
    out.append(("ill-conditioned", ill_conditioned_case()))
    return out


@functools.lru_cache(maxsize=None)
def ascent_case(d=3, obs=2):
    """Poisson counts of eight series of 40 rows drawn from a known model with a log_exposure, everything observed"""
    gen = torch.Generator().manual_seed(4242)
    N, R, B = lref.draw_model(d, obs, gen)
    offset = 0.5 + torch.rand(obs, generator=gen, dtype=F64)
    G = N @ N.T + R - R.T + 1e-5 * torch.eye(d, dtype=F64)
    series = [lref.draw_series(40, G, B, offset, "poisson", gen, keep=1.1, exposure=True) for _ in range(8)]
    return lref.Case("poisson", N, R, B, offset, series)


# ---- the dense evidence ------------------------------------------------------------------------------------------------
def leaves(case):
    """The parameters of a case as fresh fp64 leaves: dict(N, R, B, offset, ts [list], extra [list or None per series])"""
    leaf = lambda t: t.detach().clone().to(F64).requires_grad_(True)     # noqa: E731
    extra = [sr["noise_var"] if case.family == "gaussian" else sr["log_exposure"] for sr in case.series]
    return dict(N=leaf(case.N), R=leaf(case.R), B=leaf(case.B), offset=leaf(case.offset),
                ts=[leaf(sr["ts"]) for sr in case.series], extra=[None if e is None else leaf(e) for e in extra])


def _dense_terms(p, b, sr, family):
    """(Sigma, K, H, shift, s, y) of series b with a graph to the leaves ``p``"""
    d = p["N"].shape[0]
    G = p["N"] @ p["N"].T + p["R"] - p["R"].T + 1e-5 * torch.eye(d, dtype=F64)
    ts = p["ts"][b]
    n = ts.shape[0]
    Sigma = _gapref.prior_covariance(ts, G)
    K = torch.linalg.inv(Sigma)
    K = 0.5 * (K + K.T)
    mask = sr["mask"]
    idx = torch.nonzero(mask)
    m = idx.shape[0]
    H = torch.zeros(m, n, d, dtype=F64).index_put((torch.arange(m), idx[:, 0]), p["B"][idx[:, 1]]).reshape(m, n * d)
    shift = p["offset"][idx[:, 1]]
    s = None
    if family == "gaussian":
        s = p["extra"][b][mask]
    elif p["extra"][b] is not None:
        shift = shift + p["extra"][b][mask]
    return Sigma, K, H, shift, s, sr["ys"].to(F64)[mask]


def _newton_step(K, H, shift, s, y, family, z):
    g, W = lref.grad_weight(family, y, H @ z + shift, s)
    J = K + H.T @ (W[:, None] * H)
    return z + torch.linalg.solve(J, H.T @ g - K @ z)


def _evidence_at(K, H, shift, s, y, family, z):
    eta = H @ z + shift
    _, W = lref.grad_weight(family, y, eta, s)
    J = K + H.T @ (W[:, None] * H)
    return lref.log_p(family, y, eta, s).sum() - 0.5 * z @ (K @ z) + 0.5 * torch.linalg.slogdet(K)[1] - 0.5 * torch.linalg.slogdet(J)[1]


def mode_of(p, b, sr, family, z0):
    """(the mode [n d] by detached undamped Newton steps from z0, the steps taken, the last step's size)"""
    with torch.no_grad():
        _, K, H, shift, s, y = _dense_terms(p, b, sr, family)
        z, change, it = z0.reshape(-1).to(F64).clone(), math.inf, 0
        for it in range(1, NEWTON_MAX + 1):
            z_new = _newton_step(K, H, shift, s, y, family, z)
            change = float((z_new - z).abs().max())
            z = z_new
            if change < NEWTON_TOL:
                break
    return z, it, change


def evidence_series(p, b, sr, family, z0):
    """(E of series b with a graph to the leaves ``p``, the mode [n, d], the last detached step's size)"""
    z, _, change = mode_of(p, b, sr, family, z0)
    _, K, H, shift, s, y = _dense_terms(p, b, sr, family)
    z1 = _newton_step(K, H, shift, s, y, family, z.detach())
    return _evidence_at(K, H, shift, s, y, family, z1), z.reshape(sr["ts"].shape[0], -1), change


def evidence_values(case, p):
    """[B] converged evidences at the leaves ``p``, no graph (what finite differences are taken of)"""
    out = []
    for b, (sr, t) in enumerate(zip(case.series, case.truths())):
        z, _, _ = mode_of(p, b, sr, case.family, t["mean"])
        with torch.no_grad():
            _, K, H, shift, s, y = _dense_terms(p, b, sr, case.family)
            out.append(_evidence_at(K, H, shift, s, y, case.family, z))
    return torch.stack(out)


def _flatten(p):
    return [p["N"], p["R"], p["B"], p["offset"]] + p["ts"] + [e for e in p["extra"] if e is not None]


@functools.lru_cache(maxsize=None)
def _gradients(case, seed):
    p = leaves(case)
    gE = cotangent(case, seed)
    Es, modes, changes = [], [], []
    for b, (sr, t) in enumerate(zip(case.series, case.truths())):
        E, z, change = evidence_series(p, b, sr, case.family, t["mean"])
        Es.append(E)
        modes.append(z)
        changes.append(change)
    Es = torch.stack(Es)
    flat = _flatten(p)
    grads = torch.autograd.grad((gE * Es).sum(), flat, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, flat)]
    B = len(case.series)
    n_extra = [e is not None for e in p["extra"]]
    extra = None
    if any(n_extra):
        extra = torch.cat(grads[4 + B:])
    return dict(E=Es.detach(), gE=gE, N=grads[0], R=grads[1], B=grads[2], offset=grads[3], ts=torch.cat(grads[4:4 + B]),
                extra=extra, mean=torch.cat(modes), last_step=max(changes), leaves=p, flat_grads=grads)


def gradients(case, seed=0):
    """dict(E [B], gE [B], N, R, B, offset, ts [R], extra [R, obs] (log_exposure or noise_var), mean [R, d], last_step): the
    gradient of sum_b gE_b E_b, gE = ``cotangent(case, seed)``.  Computed once per case; do not modify."""
    return _gradients(case, seed)


# ---- the reference's own checks ----------------------------------------------------------------------------------------
GROUPS = ("N", "R", "B", "offset", "ts", "extra")


def directional_fd(case, seed=0, h=1e-3):
    """Per parameter group (N, R, B, offset, all ts, all log_exposure / noise_var): (group, the reference's directional
    derivative of sum gE E along a random direction in that group alone, the same by central finite differences of the
    converged evidence at steps h and h / 2 with Richardson extrapolation, |gradient of the group| |direction|: the
    size a directional derivative has when nothing cancels in it, |whole gradient| |direction|)"""
    ref = gradients(case, seed)
    gen = torch.Generator().manual_seed(99 + seed)
    base = _flatten(leaves(case))
    B = len(case.series)
    dirs = [torch.randn(t.shape, generator=gen, dtype=F64) for t in base]
    dirs[0], dirs[1] = torch.tril(dirs[0]), torch.tril(dirs[1], -1)       # N lower, R strictly lower
    for b in range(B):                                                    # keep the time stamps ascending: small moves
        dirs[4 + b] = 0.1 * dirs[4 + b]
    members = {"N": [0], "R": [1], "B": [2], "offset": [3], "ts": list(range(4, 4 + B)), "extra": list(range(4 + B, len(base)))}
    g_all = math.sqrt(float(sum((g * g).sum() for g in ref["flat_grads"])))

    def value(step, idx):
        p = leaves(case)
        with torch.no_grad():
            for k, t in enumerate(_flatten(p)):
                if k in idx:
                    t.add_(step * dirs[k])
        return float((ref["gE"] * evidence_values(case, p)).sum())

    out = []
    for name in GROUPS:
        idx = members[name]
        if not idx or not any(dirs[k].numel() and float(dirs[k].abs().max()) > 0 for k in idx):
            continue                                                      # (rank 1 has no R to move)
        analytic = float(sum((ref["flat_grads"][k] * dirs[k]).sum() for k in idx))
        D = lambda step: (value(step, idx) - value(-step, idx)) / (2 * step)      # noqa: E731
        vnorm = math.sqrt(float(sum((dirs[k] * dirs[k]).sum() for k in idx)))
        gnorm = math.sqrt(float(sum((ref["flat_grads"][k] ** 2).sum() for k in idx)))
        out.append((name, analytic, (4 * D(h / 2) - D(h)) / 3, gnorm * vnorm, g_all * vnorm))
    return out


def gaussian_gradients(case, seed=0):
    """The gradient of sum gE log N(y - shift; 0, H Sigma H^T + diag s), ``_laplaceref.gaussian_closed_form`` restated
    with a graph: the list of ``gradients(..)['flat_grads']``"""
    p = leaves(case)
    gE = cotangent(case, seed)
    total = 0.0
    for b, sr in enumerate(case.series):
        Sigma, _, H, shift, s, y = _dense_terms(p, b, sr, "gaussian")
        if y.numel() == 0:
            continue
        S = H @ Sigma @ H.T + torch.diag(s)
        r = y - shift
        L = torch.linalg.cholesky(S)
        w = torch.cholesky_solve(r.unsqueeze(-1), L).squeeze(-1)
        total = total + gE[b] * (-0.5 * r @ w - torch.log(torch.diagonal(L)).sum() - 0.5 * r.numel() * math.log(2 * math.pi))
    flat = _flatten(p)
    grads = torch.autograd.grad(total, flat, allow_unused=True)
    return [torch.zeros_like(t) if g is None else g for g, t in zip(grads, flat)]

"""An exact reference for ONE launch of cgps_leg_glm_step (csrc/cgps_leg_glm.h): the definition restated in
mpmath at 50 digits, sharing none of the kernel's formulas.  tests/test_leg_laplace.py looks only at the point the Newton
loop converges to, and Newton's method corrects its own errors; this pins every output of a single step.

    psi(z)   = sum over the observed entries of l(eta) - z^T K z / 2     (l without lgamma(y + 1), as in the kernel)
    gain_k   = psi(z + 2^-k delta) - psi(z), k = 0..11: the difference of two DIRECT evaluations, not a line formula
    alpha    = the largest 2^-k that has not overflowed in T and has gain_k >= 0, else 0
    z_out, J_Rs = Rs + B^T W B, rhs = B^T (W B z + g) and psi at z_out; grad psi . delta; the flags of DESIGN 4.26

Nothing overflows at this precision, so candidate k counts as overflowed in T by an explicit rule: the family is Poisson and
some observed eta + 2^-k dEta exceeds log(finfo(T).max).  With every value comes S, the sum of the absolute values of its
terms: the scale of the bounds of tests/test_leg_glm_step.py and of the admissibility rule.

A case is ADMISSIBLE for T when a correct kernel has exactly one right answer on it: every gain up to and including the
accepted one has |gain_k| >= 64 eps_T S_k, the comparison that sets the flag is off its threshold by a factor of 2, and
no candidate lies within 4 eps_T (1 + |eta|) of the overflow limit (``reference(..)["why"]`` lists what a series misses).

The cases of tests/test_leg_glm_step.py are built here too (as tests/_laplaceref.py does it), so that
tests/test_glmstepref.py can assert without a GPU that every one of them is admissible in both precisions.  CPU only."""
import functools
import math

import mpmath
import torch

import _gapref
import _laplaceref as lr

F64, F32 = torch.float64, torch.float32
DPS = 50
CANDIDATES = 12
CONVERGED, STALLED = 1, 2
FAMILIES = ("poisson", "bernoulli", "gaussian")
mpf = mpmath.mpf


# ---- the reference ---------------------------------------------------------------------------------------------------------
def _mp(t):
    """nested lists of mpf, exact images of the tensor's values"""
    def conv(x):
        return [conv(v) for v in x] if isinstance(x, list) else mpf(x)
    return conv(t.to(F64).tolist())


def _dot(a, b):
    return mpmath.fdot(a, b)


def _absl(v):
    return [abs(x) for x in v]


def _log_density(fam, y, eta, s):
    """(l, sum of |terms|, g, sum of |terms of g| apart from eta's own, w) at one entry"""
    if fam == "poisson":
        e = mpmath.exp(eta)
        return y * eta - e, abs(y * eta) + e, y - e, abs(y) + e, e
    if fam == "bernoulli":
        sp = mpmath.log1p(mpmath.exp(eta)) if eta <= 0 else eta + mpmath.log1p(mpmath.exp(-eta))      # softplus
        sig = 1 / (1 + mpmath.exp(-eta))
        return y * eta - sp, abs(y * eta) + sp, y - sig, abs(y) + sig, sig * (1 - sig)
    res = y - eta
    lg = mpmath.log(2 * mpmath.pi * s) / 2
    return -res * res / (2 * s) - lg, res * res / (2 * s) + abs(lg), res / s, abs(y) / s, 1 / s


class _Series:
    """one series of a launch in mpf: its rows of z and delta, its blocks of K, its observed entries"""

    def __init__(self, fam, z, delta, Rs, Os, Bm, entries):
        self.fam, self.z, self.delta, self.Rs, self.Os, self.Bm, self.entries = fam, z, delta, Rs, Os, Bm, entries
        self.aRs = [[_absl(r) for r in blk] for blk in Rs]
        self.aOs = [[_absl(r) for r in blk] for blk in Os]
        self.aBm = [_absl(r) for r in Bm]
        self.n, self.d = len(z), len(z[0])

    def point(self, alpha):
        if alpha == 0:
            return self.z
        return [[zi + alpha * di for zi, di in zip(zr, dr)] for zr, dr in zip(self.z, self.delta)]

    def bilinear(self, u, v):
        """(u^T K v, sum of |terms|)"""
        val, S = mpf(0), mpf(0)
        au, av = [_absl(r) for r in u], [_absl(r) for r in v]
        for i in range(self.n):
            for a in range(self.d):
                val += u[i][a] * _dot(self.Rs[i][a], v[i])
                S += au[i][a] * _dot(self.aRs[i][a], av[i])
                if i + 1 < self.n:                               # O_i = K[i + 1][i], and its transpose above the diagonal
                    val += u[i + 1][a] * _dot(self.Os[i][a], v[i]) + v[i + 1][a] * _dot(self.Os[i][a], u[i])
                    S += au[i + 1][a] * _dot(self.aOs[i][a], av[i]) + av[i + 1][a] * _dot(self.aOs[i][a], au[i])
        return val, S

    def eta(self, u, i, c, shift):
        return _dot(self.Bm[c], u[i]) + shift

    def quadratic(self, u):
        """(u^T K u, sum of |terms|): ``bilinear(u, u)`` with each coupling block taken once"""
        val, S = mpf(0), mpf(0)
        au = [_absl(r) for r in u]
        for i in range(self.n):
            for a in range(self.d):
                val += u[i][a] * _dot(self.Rs[i][a], u[i])
                S += au[i][a] * _dot(self.aRs[i][a], au[i])
                if i + 1 < self.n:
                    val += 2 * u[i + 1][a] * _dot(self.Os[i][a], u[i])
                    S += 2 * au[i + 1][a] * _dot(self.aOs[i][a], au[i])
        return val, S

    def psi(self, u):
        """(psi(u), S, the largest |eta|)"""
        q, qS = self.quadratic(u)
        val, S, top = -q / 2, qS / 2, mpf(0)
        for i, c, y, shift, s in self.entries:
            eta = self.eta(u, i, c, shift)
            l, lS = _log_density(self.fam, y, eta, s)[:2]
            val, S, top = val + l, S + lS, max(top, abs(eta))
        return val, S, top

    def slope(self):
        """(grad psi(z) . delta, S)"""
        q, qS = self.bilinear(self.z, self.delta)
        val, S = -q, qS
        for i, c, y, shift, s in self.entries:
            eta = self.eta(self.z, i, c, shift)
            _, _, g, gS, _ = _log_density(self.fam, y, eta, s)
            if self.fam == "gaussian":
                gS = gS + (_dot(self.aBm[c], _absl(self.z[i])) + abs(shift)) / s
            de = _dot(self.Bm[c], self.delta[i])
            val += g * de
            S += gS * _dot(self.aBm[c], _absl(self.delta[i]))
        return val, S

    def system(self, u):
        """(J_Rs, its S, rhs, its S) at u, as nested lists [n][d][d] and [n][d]"""
        J = [[list(r) for r in blk] for blk in self.Rs]
        JS = [[list(r) for r in blk] for blk in self.aRs]
        rhs = [[mpf(0)] * self.d for _ in range(self.n)]
        rS = [[mpf(0)] * self.d for _ in range(self.n)]
        for i, c, y, shift, s in self.entries:
            bz = _dot(self.Bm[c], u[i])
            abz = _dot(self.aBm[c], _absl(u[i]))
            _, _, g, gS, w = _log_density(self.fam, y, bz + shift, s)
            if self.fam == "gaussian":
                gS = gS + (abz + abs(shift)) / s
            t, tS = w * bz + g, w * abz + gS
            for a in range(self.d):
                rhs[i][a] += self.Bm[c][a] * t
                rS[i][a] += self.aBm[c][a] * tS
                for k in range(self.d):
                    J[i][a][k] += w * self.Bm[c][a] * self.Bm[c][k]
                    JS[i][a][k] += w * self.aBm[c][a] * self.aBm[c][k]
        return J, JS, rhs, rS

    def line(self):
        """[(eta, dEta)] of the observed entries at z along delta"""
        return [(self.eta(self.z, i, c, shift), _dot(self.Bm[c], self.delta[i])) for i, c, _, shift, _ in self.entries]

    def overflowed(self, line, alpha, limit):
        return self.fam == "poisson" and any(eta + alpha * de > limit for eta, de in line)

    def limit_distance(self, line, alpha, limit, eps):
        """the smallest |eta - limit| / (eps (1 + |eta|)) over the observed entries"""
        if self.fam != "poisson":
            return math.inf
        return min([float(abs(eta + alpha * de - limit) / (eps * (1 + abs(eta + alpha * de)))) for eta, de in line] or [math.inf])


def reference(ops, all_gains=False):
    """The step of one launch.  ``ops``: dict(family, tol, z [R, d], prop or None, Rs [R, d, d], Os [R - 1, d, d], ys
    [R, obs], mask (bool [R, obs]) or None, offset [obs] or None, extra [R, obs] or None, Bm [obs, d], offsets (list of
    B + 1 row numbers), state_in [B, 4] or None), CPU tensors that hold the values the kernel reads (already rounded to its
    dtype T = z.dtype).  Returns a dict of per-series lists (alpha, flags, iterations, psi, psi_S, eta_max, gains, gain_S,
    slope, slope_S, active, why) and fp64 tensors z_out, J_Rs, J_S, rhs, rhs_S; ``why[b]`` lists what keeps series b from
    being admissible for T (empty: admissible).  ``gains`` and ``gain_S`` stop at the accepted candidate, which is all the
    step depends on, unless ``all_gains`` asks for the twelve."""
    with mpmath.workdps(DPS):
        return _reference(ops, all_gains)


def _reference(ops, all_gains):
    fam, T = ops["family"], ops["z"].dtype
    eps, limit = mpf(float(torch.finfo(T).eps)), mpmath.log(mpf(float(torch.finfo(T).max)))
    R, d = ops["z"].shape
    obs = ops["ys"].shape[1]
    z, Rs, Os, Bm, ys = _mp(ops["z"]), _mp(ops["Rs"]), _mp(ops["Os"]), _mp(ops["Bm"]), _mp(ops["ys"])
    prop = None if ops["prop"] is None else ops["prop"].to(F64).tolist()
    offset = [mpf(0)] * obs if ops["offset"] is None else _mp(ops["offset"])
    extra = None if ops["extra"] is None else ops["extra"].to(F64).tolist()
    mask = None if ops["mask"] is None else ops["mask"].tolist()
    state = None if ops["state_in"] is None else ops["state_in"].tolist()
    tol = mpf(ops["tol"])
    offs = ops["offsets"]
    out = dict(alpha=[], flags=[], iterations=[], psi=[], psi_S=[], eta_max=[], gains=[], gain_S=[], slope=[], slope_S=[],
               active=[], why=[])
    z_out = torch.zeros(R, d, dtype=F64)
    J, JS = torch.zeros(R, d, d, dtype=F64), torch.zeros(R, d, d, dtype=F64)
    rh, rhS = torch.zeros(R, d, dtype=F64), torch.zeros(R, d, dtype=F64)
    for b in range(len(offs) - 1):
        r0, r1 = offs[b], offs[b + 1]
        active = prop is not None and int(state[b][2]) & (CONVERGED | STALLED) == 0
        entries = []
        for i in range(r0, r1):
            for c in range(obs):
                if mask is None or mask[i][c]:               # (what an unobserved entry holds is never converted: NaN is fine)
                    if fam == "gaussian":
                        shift, s = offset[c], mpf(extra[i][c])
                    else:
                        shift, s = offset[c] + (mpf(extra[i][c]) if extra is not None else 0), None
                    entries.append((i - r0, c, ys[i][c], shift, s))
        if active:                                               # (a frozen series' prop is not read: NaN is fine)
            delta = [[mpf(p) - zz for p, zz in zip(prop[i], z[i])] for i in range(r0, r1)]
        else:
            delta = [[mpf(0)] * d for _ in range(r0, r1)]
        sr = _Series(fam, z[r0:r1], delta, Rs[r0:r1], Os[r0:r1 - 1], Bm, entries)
        why, gains, gain_S, alpha, gain = [], [], [], mpf(0), mpf(0)
        slope, slope_S = mpf(0), mpf(0)
        found = False
        if active:
            psi0, S0, _ = sr.psi(sr.z)
            slope, slope_S = sr.slope()
            line = sr.line()
            for k in range(CANDIDATES):
                ak = mpf(2) ** -k
                near = sr.limit_distance(line, ak, limit, eps)
                if near < 4:
                    why.append("candidate %d: an eta within %.2f eps (1 + |eta|) of the overflow limit" % (k, near))
                if found and not all_gains:
                    continue
                pk, Sk, _ = sr.psi(sr.point(ak))
                gains.append(pk - psi0)
                gain_S.append(Sk + S0)
                ok = gains[k] >= 0 and not sr.overflowed(line, ak, limit)
                if not found:
                    if abs(gains[k]) < 64 * eps * gain_S[k]:
                        why.append("gain %d = %.3e against 64 eps S = %.3e" % (k, float(gains[k]), float(64 * eps * gain_S[k])))
                    if ok:
                        found, alpha, gain = True, ak, gains[k]
        u = sr.point(alpha)
        for i in range(r1 - r0):
            if alpha == 1:
                z_out[r0 + i] = torch.tensor(prop[r0 + i], dtype=F64)
            else:
                z_out[r0 + i] = torch.tensor([float(x) for x in u[i]], dtype=F64)
        psi, psi_S, eta_max = sr.psi(u)
        Jb, JSb, rb, rSb = sr.system(u)
        tof = lambda x: torch.tensor([[float(v) for v in row] if isinstance(row, list) else float(row) for row in x], dtype=F64)      # noqa: E731
        for i in range(r1 - r0):
            J[r0 + i], JS[r0 + i], rh[r0 + i], rhS[r0 + i] = tof(Jb[i]), tof(JSb[i]), tof(rb[i]), tof(rSb[i])
        flags, iterations, alpha_out, psi_out = 0, 0.0, float(alpha), float(psi)
        if active:
            bound = tol * (1 + abs(psi))
            value = gain if found else abs(slope)
            flags = (CONVERGED if value <= bound else 0) if found else (CONVERGED if value <= bound else STALLED)
            if bound / 2 < value < 2 * bound:
                why.append("%s = %.3e within a factor of 2 of the bound %.3e" % ("gain" if found else "|slope|", float(value), float(bound)))
            iterations = state[b][1] + 1
        elif prop is not None:                                   # frozen: the state is copied
            psi_out, iterations, flags, alpha_out = state[b][0], state[b][1], int(state[b][2]), state[b][3]
        for key, v in (("alpha", alpha_out), ("flags", flags), ("iterations", iterations), ("psi", psi_out), ("psi_S", float(psi_S)),
                       ("eta_max", float(eta_max)), ("gains", [float(g) for g in gains]), ("gain_S", [float(g) for g in gain_S]),
                       ("slope", float(slope)), ("slope_S", float(slope_S)), ("active", active), ("why", why)):
            out[key].append(v)
    out.update(z_out=z_out, J_Rs=J, J_S=JS, rhs=rh, rhs_S=rhS)
    return out


# ---- the direct definition once more, in fp64 torch: the reference's own check, and what the case builders search with -------
def series_of_rows(offsets):
    return torch.cat([torch.full((offsets[b + 1] - offsets[b],), b, dtype=torch.int64) for b in range(len(offsets) - 1)])


def psi_torch(ops, u):
    """psi per series [B] at the points u [R, d], fp64 torch ops (differentiable in u)"""
    fam = ops["family"]
    f = lambda k: None if ops[k] is None else ops[k].to(F64)      # noqa: E731
    Rs, Os, Bm, ys, offset, extra = f("Rs"), f("Os"), f("Bm"), f("ys"), f("offset"), f("extra")
    offs = ops["offsets"]
    seg = series_of_rows(offs)
    B = len(offs) - 1
    q = torch.einsum("ra,rab,rb->r", u, Rs, u)
    inside = seg[1:] == seg[:-1]
    c = 2 * torch.einsum("ra,rab,rb->r", u[1:], Os, u[:-1])
    q = q + torch.cat([torch.where(inside, c, torch.zeros_like(c)), c.new_zeros(1)])
    eta = u @ Bm.T
    if offset is not None:
        eta = eta + offset
    if fam != "gaussian" and extra is not None:
        eta = eta + torch.nan_to_num(extra)
    if fam == "poisson":
        l = ys * eta - torch.exp(eta)
    elif fam == "bernoulli":
        l = ys * eta - torch.nn.functional.softplus(eta)
    else:
        s = torch.nan_to_num(extra, nan=1.0)
        l = -0.5 * (ys - eta) ** 2 / s - 0.5 * torch.log(2 * math.pi * s)
    if ops["mask"] is not None:
        l = torch.where(ops["mask"], l, torch.zeros_like(l))
    return torch.zeros(B, dtype=F64).index_add(0, seg, l.sum(-1) - 0.5 * q)


def ascent(ops, z, gen, noise=0.5):
    """(v [R, d], s* [B]): per series a direction of ascent of psi at z, of unit length (the gradient and some noise), and
    the step length s* > 0 at which psi(z + s v) falls back to psi(z) -- by bisection; psi is concave along the line"""
    offs = ops["offsets"]
    seg = series_of_rows(offs)
    B = len(offs) - 1
    zz = z.clone().requires_grad_(True)
    grad, = torch.autograd.grad(psi_torch(ops, zz).sum(), zz)
    norm = lambda x: torch.zeros(B, dtype=F64).index_add(0, seg, (x * x).sum(-1)).sqrt()[seg].unsqueeze(-1)      # noqa: E731
    v = grad / norm(grad)
    e = torch.randn(z.shape, generator=gen, dtype=F64)
    v = v + noise * e / norm(e)
    v = v / norm(v)
    psi0 = psi_torch(ops, z)
    gain = lambda s: psi_torch(ops, z + s[seg].unsqueeze(-1) * v) - psi0      # noqa: E731
    lo, hi = torch.zeros(B, dtype=F64), torch.full((B,), 1e-6, dtype=F64)
    assert bool((gain(hi) > 0).all()), "not a direction of ascent"
    for _ in range(200):
        up = gain(hi) > 0
        if not bool(up.any()):
            break
        lo, hi = torch.where(up, hi, lo), torch.where(up, 2 * hi, hi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        up = gain(mid) > 0
        lo, hi = torch.where(up, mid, lo), torch.where(up, hi, mid)
    return v, 0.5 * (lo + hi)


# ---- the cases of tests/test_leg_glm_step.py ---------------------------------------------------------------------------------
FORMS = ((1, 1), (3, 2), (5, 3), (8, 8))          # compiled (O <= 4) and run-time channel counts
LENGTHS_POINT = (1, 2, 65, 131)                    # one row; one coupling block; the wave's second stride; a partial third
TOL_POINT = 1e-9


class StepCase:
    """The operands of one launch as fp64 CPU tensors; ``operands(T)`` rounds them to the kernel's dtype.  ``expect``:
    what the builder aimed at per series (a dict of lists, e.g. alpha and flags), for the tests to assert on top of the
    reference."""

    def __init__(self, family, tol, ts, G, Bm, lengths, z, prop, ys, mask=None, offset=None, extra=None, state=None, expect=None):
        self.family, self.tol, self.ts, self.G, self.Bm, self.lengths = family, tol, ts, G, Bm, list(lengths)
        self.z, self.prop, self.ys, self.mask, self.offset, self.extra, self.state = z, prop, ys, mask, offset, extra, state
        self.expect = expect or {}
        self.offsets = [0]
        for n in self.lengths:
            self.offsets.append(self.offsets[-1] + n)

    def blocks(self, T):
        """the prior blocks from the cancellation-free restatement (tests/_gapref.py), rounded to T: what the CPU tests
        take for K; the GPU tests pass in what cgps_peg_precision_seg wrote"""
        d = self.G.shape[0]
        Rs, Os = [], []
        G = self.G.to(T).to(F64)
        ts = self.ts.to(T).to(F64)
        for b, n in enumerate(self.lengths):
            r, o = _gapref.blocks_cancel_free(ts[self.offsets[b]:self.offsets[b + 1]], G)
            Rs.append(r)
            Os.append(o)
            if b + 1 < len(self.lengths):
                Os.append(torch.zeros(1, d, d, dtype=F64))
        return torch.cat(Rs).to(T), torch.cat(Os).to(T)

    def operands(self, T, blocks=None, first=False):
        """``first``: the first call of a loop (no proposal, no state)"""
        r = lambda t: None if t is None else t.to(T)      # noqa: E731
        Rs, Os = self.blocks(T) if blocks is None else blocks
        return dict(family=self.family, tol=self.tol, z=r(self.z), prop=None if first else r(self.prop), Rs=Rs, Os=Os, ys=r(self.ys),
                    mask=self.mask, offset=r(self.offset), extra=r(self.extra), Bm=r(self.Bm), offsets=self.offsets,
                    state_in=None if first else self.state)


def _model(d, obs, gen):
    N, R, Bm = lr.draw_model(d, obs, gen)
    return N @ N.T + R - R.T + 1e-5 * torch.eye(d, dtype=F64), Bm


def _times(lengths, gen):
    """gaps of 0.5 .. 1, as tests/_laplaceref.py takes them: the prior blocks stay positive definite in fp32 at every rank"""
    return torch.cat([3.0 * torch.rand((), generator=gen, dtype=F64) + torch.cumsum(0.5 + 0.5 * torch.rand(n, generator=gen, dtype=F64), 0)
                      for n in lengths])


def _data(family, R, obs, gen):
    if family == "poisson":
        return torch.poisson(torch.full((R, obs), 2.0, dtype=F64), generator=gen)
    if family == "bernoulli":
        return (torch.rand(R, obs, generator=gen) < 0.5).to(F64)
    return torch.randn(R, obs, generator=gen, dtype=F64)


def _state(flags, gen):
    """[B, 4] states as a loop leaves them: psi, iterations, flags, alpha"""
    B = len(flags)
    return torch.stack([-50.0 * torch.rand(B, generator=gen, dtype=F64), torch.arange(1, B + 1, dtype=F64),
                        torch.tensor(flags, dtype=F64), 0.5 ** torch.arange(B, dtype=F64)], 1)


def _rounded(case, T=F32):
    """the operands search directions are found on: rounded to fp32, so that both precisions see nearly the same line"""
    return case.operands(T)


@functools.lru_cache(maxsize=None)
def point_case(family, d, obs, plain):
    """2a: every output at a general point.  Random z, four series of lengths (1, 2, 65, 131) of which two are active and
    two frozen (which two: the other way round in the plain variant, so that every length is stepped once); an active
    series' proposal lies 0.6, 1.3 or 2.6 zero-gain step lengths along a direction of ascent, so that the step accepts 1,
    1/2 or 1/4 (full: 1/2 on the one-row series and 1 on the 65 rows; plain: 1 on the two rows and 1/4 on the 131).  ``plain``: no pattern, no offset, no extra (the Gaussian family keeps its variances)."""
    gen = torch.Generator().manual_seed(4000 + 100 * d + 10 * obs + 2 * FAMILIES.index(family) + int(plain))
    G, Bm = _model(d, obs, gen)
    R = sum(LENGTHS_POINT)
    ts = _times(LENGTHS_POINT, gen)
    z = 0.3 * torch.randn(R, d, generator=gen, dtype=F64)
    ys = _data(family, R, obs, gen)
    mask = offset = extra = None
    if not plain:
        mask = torch.rand(R, obs, generator=gen) < 0.7
        mask[0, 0] = True
        offset = 0.5 * torch.randn(obs, generator=gen, dtype=F64)
    if family == "gaussian":
        extra = 0.1 + 1.9 * torch.rand(R, obs, generator=gen, dtype=F64)
    elif not plain:
        extra = 0.2 * torch.randn(R, obs, generator=gen, dtype=F64)
    flags = (CONVERGED, 0, STALLED, 0) if plain else (0, CONVERGED, 0, STALLED)
    case = StepCase(family, TOL_POINT, ts, G, Bm, LENGTHS_POINT, z, z, ys, mask, offset, extra, _state(flags, gen))
    ops = _rounded(case)
    v, s = ascent(ops, ops["z"].to(F64), gen)
    mult = torch.tensor([0.6, 0.6, 0.6, 2.6] if plain else [1.3, 0.6, 0.6, 0.6], dtype=F64)
    seg = series_of_rows(case.offsets)
    case.prop = z + (mult * s)[seg].unsqueeze(-1) * v
    case.expect = dict(alpha=[None if f else float(2.0 ** -round(math.log2(m / 0.65))) for f, m in zip(flags, mult.tolist())])
    return case


LADDER_LENGTHS = (1, 2, 3, 5, 8, 13, 21, 34, 70, 4, 7, 1, 6, 9, 2, 3, 5)      # 12 rungs and five special series: 194 rows
TOL_LADDER = (1e-3, 16.0)


@functools.lru_cache(maxsize=None)
def ladder_case(family, tol, d=3, obs=2):
    """2b: the whole ladder in one launch.  Series k = 0..11 proposes 2^k x 0.75 s* along its own direction of ascent (s*:
    the zero-gain step length), so it must accept exactly 2^-k: 0.75 s* gains, 1.5 s* loses.  Then: k = 12 (nothing
    qualifies: STALLED); a descent direction (STALLED); a small descent step, |grad psi . delta| = 0.09 (1 + |psi|): above
    the bound at tol = 1e-3 (STALLED), under it at tol = 16 (CONVERGED) -- no smaller step is admissible in fp32, where
    the twelfth gain must still be 64 eps S; a small ascent step whose gain is under the bound at either tol
    (CONVERGED); an ordinary ascent step (found; flags 0 at tol = 1e-3)."""
    gen = torch.Generator().manual_seed(5000 + FAMILIES.index(family))
    G, Bm = _model(d, obs, gen)
    L = LADDER_LENGTHS
    R = sum(L)
    ts = _times(L, gen)
    z = 0.3 * torch.randn(R, d, generator=gen, dtype=F64)
    ys = _data(family, R, obs, gen)
    mask = torch.rand(R, obs, generator=gen) < 0.8
    offset = 0.3 * torch.randn(obs, generator=gen, dtype=F64)
    extra = 0.1 + 1.9 * torch.rand(R, obs, generator=gen, dtype=F64) if family == "gaussian" else None
    state = _state([0] * len(L), gen)
    case = StepCase(family, tol, ts, G, Bm, L, z, z, ys, mask, offset, extra, state)
    for b in range(len(L)):
        mask[case.offsets[b], 0] = True                        # every series observes something
    ops = _rounded(case)
    z32 = ops["z"].to(F64)
    v, s = ascent(ops, z32, gen)
    seg = series_of_rows(case.offsets)
    zz = z32.clone().requires_grad_(True)
    psi0 = psi_torch(ops, zz)
    grad, = torch.autograd.grad(psi0.sum(), zz)
    slope = torch.zeros(len(L), dtype=F64).index_add(0, seg, (grad * v).sum(-1))       # > 0 per unit step
    scale = 1 + psi0.detach().abs()
    step = [0.75 * s[k] * 2.0 ** k for k in range(12)]
    step.append(0.75 * s[12] * 2.0 ** 12)
    step.append(-0.5 * s[13])
    step.append(-0.09 * scale[14] / slope[14])
    step.append(0.0)                                            # (set below)
    step.append(0.5 * s[16])
    step = torch.stack([torch.as_tensor(x, dtype=F64) for x in step])
    # the small ascent step: its gain, about slope x step, is 2e-4 (1 + |psi|): under half the bound at tol = 1e-3, and
    # (asserted by the admissibility test) above 64 eps32 S
    step[15] = 2e-4 * scale[15] / slope[15]
    case.prop = z + step[seg].unsqueeze(-1) * v
    big = tol >= 0.1                                            # (the descent step's slope is then under the bound too)
    case.expect = dict(alpha=[2.0 ** -k for k in range(12)] + [0.0, 0.0, 0.0, 1.0, 1.0],
                       flags=[None] * 12 + [STALLED, None if big else STALLED, CONVERGED if big else STALLED, CONVERGED, None if big else 0])
    return case


def _pinv_rows(Bm, target):
    """delta with B delta = target (obs <= d: exact), and a unit vector of B's null space (d = obs + 1)"""
    P = torch.linalg.pinv(Bm)
    _, _, Vh = torch.linalg.svd(Bm)
    return P @ target, Vh[-1]


@functools.lru_cache(maxsize=None)
def overflow_case(T):
    """2c, Poisson: z = 0, so eta = 0; the proposal has dEta = 2^(j + 1) t on every entry with t = 70 in fp32 and 600 in
    fp64, and the counts are e^t: e^eta overflows in T at alpha = 1 .. 2^-j, and alpha = 2^-(j + 1) lands on the mode of
    the likelihood, a gain of e^t (t - 1).  j = 0, 2, 5.  A fourth series proposes dEta = 2^11 x (100 or 800): all twelve
    overflow."""
    gen = torch.Generator().manual_seed(6000)
    d, obs = 3, 2
    G, Bm = _model(d, obs, gen)
    L = (2, 3, 1, 2)
    R = sum(L)
    t, far = (70.0, 100.0) if T == F32 else (600.0, 800.0)
    ts = _times(L, gen)
    z = torch.zeros(R, d, dtype=F64)
    seg = series_of_rows([0, 2, 5, 6, 8])
    dEta = torch.tensor([2.0 * t, 8.0 * t, 64.0 * t, 2048.0 * far], dtype=F64)[seg]
    unit, _ = _pinv_rows(Bm.to(T).to(F64), torch.ones(obs, dtype=F64))
    prop = dEta.unsqueeze(-1) * unit
    ys = torch.full((R, obs), math.exp(t), dtype=F64)
    ys[seg == 3] = 3.0
    case = StepCase("poisson", 1e-9, ts, G, Bm, L, z, prop, ys, None, None, None, _state([0] * 4, gen))
    case.expect = dict(alpha=[0.5, 0.125, 2.0 ** -6, 0.0], flags=[0, 0, 0, STALLED])
    return case


# (E, T, rho, the step length that must be accepted)
SATURATED = ((5, 5, 0.5, 1.0), (10, 10, 1.4, 0.5), (12, 14, 3.0, 0.5), (18, 20, 0.5, 1.0), (20, 24, 1.4, 0.5), (25, 30, 0.5, 1.0),
             (38, 40, 0.5, 1.0), (39, 44, 1.4, 0.5), (40, 45, 3.0, 0.25))
SATURATED_LENGTHS = (3, 5, 2, 4, 6, 1, 3, 7, 2)


@functools.lru_cache(maxsize=None)
def saturated_case():
    """2e, Bernoulli: series b has eta near +E_b (E = 5 .. 40, a shift in ``extra``: one launch has one offset) and a
    proposal with dEta = -T_b on every entry (T = 5 .. 45).  d = obs + 1, so B has a null direction; the proposal's
    component along it costs prior and nothing else, and is set so that the prior's cost at alpha = 1 is rho_b times the
    likelihood's gain: rho = 0.5 accepts 1, rho = 1.4 accepts 1/2, rho = 3 accepts 1/4 where half the step is still saturated (E = 40) and 1/2 where
    it is not (E = 12).  The second half of the batch is
    the mirror image (1 - y, -shift, -z, -prop): one launch has one B, and -B z = B (-z), so this is the posterior with
    (1 - y, -offset, -B) under another name.  It must take the same steps."""
    gen = torch.Generator().manual_seed(7000)
    d, obs = 3, 2
    G, Bm = _model(d, obs, gen)
    Bm = 48.0 * Bm
    L = SATURATED_LENGTHS
    R = sum(L)
    ts = _times(L, gen)
    offsets = [0]
    for n in L:
        offsets.append(offsets[-1] + n)
    seg = series_of_rows(offsets)
    E = torch.tensor([float(e) for e, _, _, _ in SATURATED], dtype=F64)[seg]
    Tt = torch.tensor([float(t) for _, t, _, _ in SATURATED], dtype=F64)[seg]
    rho = torch.tensor([r for _, _, r, _ in SATURATED], dtype=F64)
    z = (0.05 * torch.randn(R, d, generator=gen, dtype=F64)).to(F32).to(F64)
    extra = (E.unsqueeze(-1) + 0.5 * torch.rand(R, obs, generator=gen, dtype=F64)).to(F32).to(F64)
    ys = (torch.rand(R, obs, generator=gen) < 0.3).to(F64)
    ys[torch.tensor(offsets[:-1]), 0] = 0.0
    B32 = Bm.to(F32).to(F64)
    unit, null = _pinv_rows(B32, torch.ones(obs, dtype=F64))
    base = -Tt.unsqueeze(-1) * unit
    case = StepCase("bernoulli", 1e-9, ts, G, Bm, L, z, z, ys, None, None, extra, _state([0] * len(L), gen))
    ops = _rounded(case)
    psi0 = psi_torch(ops, z)
    zero = dict(ops, Rs=torch.zeros_like(ops["Rs"]), Os=torch.zeros_like(ops["Os"]))
    lik = psi_torch(zero, z + base) - psi_torch(zero, z)          # the likelihood's gain at alpha = 1: > 0 (checked)
    assert bool((lik > 0).all())
    sign = torch.where(torch.arange(R) % 2 == 0, 1.0, -1.0).to(F64).unsqueeze(-1)
    gain = lambda lam: psi_torch(ops, z + base + lam[seg].unsqueeze(-1) * sign * null) - psi0      # noqa: E731
    want = (1 - rho) * lik
    lo, hi = torch.zeros(len(L), dtype=F64), torch.full((len(L),), 1e3, dtype=F64)
    assert bool((gain(lo) > want).all()) and bool((gain(hi) < want).all())
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        above = gain(mid) > want
        lo, hi = torch.where(above, mid, lo), torch.where(above, hi, mid)
    prop = z + base + lo[seg].unsqueeze(-1) * sign * null
    accept = [a for _, _, _, a in SATURATED]
    both = lambda t, m: torch.cat([t, m])      # noqa: E731
    case = StepCase("bernoulli", 1e-9, both(ts, ts), G, Bm, L + L, both(z, -z), both(prop, -prop), both(ys, 1 - ys), None, None,
                    both(extra, -extra), _state([0] * (2 * len(L)), gen))
    case.expect = dict(alpha=accept + accept)
    return case


@functools.lru_cache(maxsize=None)
def reference_of(builder, args, T, first=False):
    """the reference on a case's own (CPU) blocks, once"""
    return reference(builder(*args).operands(T, first=first))


def all_cases():
    """(name, builder, args, dtypes) of every launch of tests/test_leg_glm_step.py"""
    out = []
    for family in FAMILIES:
        for d, obs in FORMS:
            for plain in (False, True):
                out.append(("point-%s-d%d-o%d-%s" % (family, d, obs, "plain" if plain else "full"), point_case, (family, d, obs, plain), (F64, F32)))
        for tol in TOL_LADDER:
            out.append(("ladder-%s-tol%g" % (family, tol), ladder_case, (family, tol), (F64, F32)))
    out.append(("overflow-fp32", overflow_case, (F32,), (F32,)))
    out.append(("overflow-fp64", overflow_case, (F64,), (F64,)))
    out.append(("saturated", saturated_case, (), (F64, F32)))
    return out

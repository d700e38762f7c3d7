"""Accuracy of the block-tridiagonal kernels across scale and conditioning, against a long-double truth (_condref.py).

Every existing kernel test draws cond < 10 systems with entries of order 1 and allows 1e6 eps (fp64) or ~3000 eps
(fp32).  Here the systems are ill conditioned inside the blocks (`block`) or in the coupling between rows (`chain`, the
hard case for cyclic reduction), and scaled by powers of two up to the edge of what a block determinant can hold.

Bound: no number fixed in advance.  Each error measure is in units of u * cond2 of the rounded system (_condref.m_*);
for each (dtype, quantity, family, level) the CPU oracle, run in the kernel's dtype on the same inputs, gives a pooled
worst measure over the group's (n, d) members, and a kernel's measure on every case of the group must be <= 4 x that
(the margin this project gives the same formulas evaluated in another order).  A power of two changes no measure but
the log-determinant's, so the scaled cases meet the bounds of k = 0.  The log-determinant grows by n d k log 2; it keeps
the k = 0 bound wherever the oracle meets it on the scaled inputs (fp64 from d = 2 on), and where the rounding of a
result of that size alone exceeds it (|l*| >> n d cond: d = 1, the low-cond fp32 cases) it gets 4 x the oracle's worst
on that case's scaled inputs (_condref.bound).

Each test prints every figure before it asserts; the worst measure / bound per entry point is printed at the end of the
module (pytest -s)."""
import numpy as np
import pytest
import torch

import _condref as C
import cyclic_gps.cyclic_reduction as cr
from oracle import cr_oracle

pytestmark = pytest.mark.gpu

DTYPES = ("float64", "float32")
SHAPES = [(dt, n, d) for dt in DTYPES for (n, d) in C.shapes(dt)]
WORST = {}                  # entry point -> (measure / bound, case, quantity)


def _id(p):
    return "-".join(str(v) for v in p) if isinstance(p, tuple) else str(p)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst measure / bound per entry point (pass: <= 1):")
    for entry in sorted(WORST):
        r, key, q = WORST[entry]
        print("  %-34s %8.4f   at %s %s" % (entry, r, _id(key), q))


class Checker:
    """Collects (entry point, quantity, measure) of one case against its group's bound; prints all, then asserts all."""

    def __init__(self):
        self.bad = []

    def add(self, entry, key, quantity, measure, tag=""):
        b = C.bound(key, quantity, scaled=bool(tag))
        r = measure / b if b > 0 else float("inf")
        print("%-30s %-40s %-8s measure %.4g bound %.4g ratio %.3f" % (entry, _id(key) + tag, quantity, measure, b, r))
        if not r <= WORST.get(entry, (-1.0,))[0]:
            WORST[entry] = (r, _id(key) + tag, quantity)
        if not measure <= b:
            self.bad.append((entry, _id(key) + tag, quantity, measure, b))

    def finish(self):
        assert not self.bad, "above 4 x the oracle's pooled worst: %s" % (self.bad,)


def _fused(chk, key, R, O, b0, t, cond, u, n, d, tag=""):
    """mahal_and_det, fused and level by level; returns the two log-determinants."""
    lds = []
    for levelwise in (False, True):
        name = "mahal_and_det[levelwise]" if levelwise else "mahal_and_det"
        m, ld = cr._mahal_and_det(R, O, b0, levelwise=levelwise)
        assert bool(torch.isfinite(m)) and bool(torch.isfinite(ld)), (name, key, tag, float(m), float(ld))
        chk.add(name, key, "mahal", C.m_mahal(m, t, cond, u), tag)
        chk.add(name, key, "logdet", C.m_logdet(ld, t, cond, u, n, d), tag)
        lds.append(ld)
    return lds


def _factor(chk, key, R, O, b, t, cond, u, n, d, tag=""):
    """decompose -> solve (1 and 8 columns), det, mahal, inverse_blocks; decompose_solve."""
    b0 = b[:, :, 0].contiguous()
    dec = cr.decompose(R, O)
    x1, x8 = cr.solve(dec, b0), cr.solve(dec, b)
    ld, m = cr.det(dec), cr.mahal(dec, b0)
    Sd, So = cr.inverse_blocks(dec)
    dec2, x2 = cr.decompose_solve(R, O, b0)
    for v in (x1, x8, ld, m, Sd, So, x2):
        assert bool(torch.isfinite(v).all()), (key, tag)
    assert all(torch.equal(a_, b_) for a_, b_ in zip(dec[1], dec2[1]))          # one factor by both routes
    chk.add("solve[m=1]", key, "solve", C.m_solve(x1, t, cond, u, 0), tag)
    chk.add("solve[m=8]", key, "solve", C.m_solve(x8, t, cond, u), tag)
    chk.add("decompose_solve", key, "solve", C.m_solve(x2, t, cond, u, 0), tag)
    chk.add("det", key, "logdet", C.m_logdet(ld, t, cond, u, n, d), tag)
    chk.add("mahal", key, "mahal", C.m_mahal(m, t, cond, u), tag)
    idg, iof = C.m_inv(Sd, So, t, cond, u)
    chk.add("inverse_blocks", key, "inv_diag", idg, tag)
    chk.add("inverse_blocks", key, "inv_off", iof, tag)
    return ld


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_fused_reduction(shape):
    dtype, n, d = shape
    u, chk = C.eps_of(dtype), Checker()
    for key, c in C.shape_cases(dtype, n, d).items():
        _fused(chk, key, _dev(c["Rs"]), _dev(c["Os"]), _dev(c["b"][:, :, 0]), c["truth"], c["cond"], u, n, d)
    chk.finish()


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_factor_and_what_is_computed_from_it(shape):
    dtype, n, d = shape
    u, chk = C.eps_of(dtype), Checker()
    for key, c in C.shape_cases(dtype, n, d).items():
        _factor(chk, key, _dev(c["Rs"]), _dev(c["Os"]), _dev(c["b"]), c["truth"], c["cond"], u, n, d)
    chk.finish()


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] <= cr.BATCH_MAX_ROWS], ids=_id)
def test_batch_dense(shape):
    """The cases of a shape (both families, every level) as one dense batch."""
    dtype, n, d = shape
    u, chk = C.eps_of(dtype), Checker()
    cases = C.shape_cases(dtype, n, d)
    R, O, x = (_dev(np.stack([c[a] for c in cases.values()])) for a in ("Rs", "Os", "b"))
    m, ld = cr.mahal_and_det_batch(R, O, x[..., 0].contiguous())
    assert bool(torch.isfinite(m).all()) and bool(torch.isfinite(ld).all())
    for i, (key, c) in enumerate(cases.items()):
        chk.add("mahal_and_det_batch[dense]", key, "mahal", C.m_mahal(m[i], c["truth"], c["cond"], u))
        chk.add("mahal_and_det_batch[dense]", key, "logdet", C.m_logdet(ld[i], c["truth"], c["cond"], u, n, d))
    chk.finish()


def _one_system_serves(dtype, n, d):
    """Slots that mahal_and_det_batch hands to the one-system kernel (cr.mahal_and_det_batch's docstring)."""
    return n > cr.BATCH_MAX_ROWS or d == 8 or (d == 6 and dtype == "float64")


@pytest.mark.parametrize("dtype,d", [(dt, d) for dt in DTYPES for d in range(1, 9)], ids=_id)
def test_batch_ragged_mixed(dtype, d):
    """One ragged batch of cases of different families, levels, lengths and scales: each slot to its own bound, and
    bitwise equal to mahal_and_det where the one-system kernel serves the slot."""
    u, chk = C.eps_of(dtype), Checker()
    ks = C.SCALES[dtype]
    slots = [((dtype, "chain", 2, 33, d), 0), ((dtype, "block", 0, 257, d), 0), (C.scale_key(dtype, 257, d), ks[0]),
             ((dtype, "chain", 1, 257, d), 0), (C.scale_key(dtype, 257, d), ks[-1]), ((dtype, "block", C.level_ids("block", d)[-1], 33, d), 0)]
    if C.large_ns(dtype, d):
        n_big = C.large_ns(dtype, d)[1]
        slots += [((dtype, "chain", 2, 1025, d), 0), ((dtype, "block", 1, n_big, d), 0), (C.scale_key(dtype, 257, d), ks[1])]
        if (n_big, d) in C.scale_shapes(dtype):          # a scaled system longer than BATCH_MAX_ROWS: the one-system kernel's slot
            slots += [(C.scale_key(dtype, n_big, d), ks[-1]), (C.scale_key(dtype, n_big, d), ks[0])]
    Rp, Op, xp, truths, own = [], [], [], [], []
    for i, (key, k) in enumerate(slots):
        c = C.case(key)
        Rs, Os = C.scaled(c["Rs"], c["Os"], k)
        Rp.append(Rs), xp.append(c["b"][:, :, 0])
        Op.append(Os), own.append(Os)
        if i + 1 < len(slots):
            Op.append(np.full((1, d, d), 7.0, Rs.dtype))                      # between two systems: ignored
        truths.append(C.scaled_truth(c["truth"], key[3], d, k))
    R, O, x = _dev(np.concatenate(Rp)), _dev(np.concatenate(Op)), _dev(np.concatenate(xp))
    m, ld = cr.mahal_and_det_batch(R, O, x, lengths=[key[3] for key, _ in slots])
    assert bool(torch.isfinite(m).all()) and bool(torch.isfinite(ld).all()), (m, ld)
    for i, ((key, k), t) in enumerate(zip(slots, truths)):
        c, n = C.case(key), key[3]
        tag = "*2^%d" % k if k else ""
        chk.add("mahal_and_det_batch[ragged]", key, "mahal", C.m_mahal(m[i], t, c["cond"], u), tag)
        chk.add("mahal_and_det_batch[ragged]", key, "logdet", C.m_logdet(ld[i], t, c["cond"], u, n, d), tag)
        if _one_system_serves(dtype, n, d):
            m1, ld1 = cr.mahal_and_det(_dev(Rp[i]), _dev(own[i]), _dev(xp[i]))
            assert torch.equal(m1, m[i]) and torch.equal(ld1, ld[i]), (key, k)
    chk.finish()


SCALE_CASES = [(dt, n, d, k) for dt in DTYPES for (n, d) in C.scale_shapes(dt) for k in C.SCALES[dt]]


@pytest.mark.parametrize("case", SCALE_CASES, ids=_id)
def test_scaled_by_a_power_of_two(case):
    """A mid-conditioned system times 2^k: every entry point finite, no NotPSDError, the bounds of k = 0 (the
    log-determinants: the same unless the oracle itself misses it there, _condref.bound), and the three routes to the
    log-determinant agree with the truth (hence with each other)."""
    dtype, n, d, k = case
    key = C.scale_key(dtype, n, d)
    c, u, chk = C.case(key), C.eps_of(dtype), Checker()
    Rs, Os = C.scaled(c["Rs"], c["Os"], k)
    assert np.isfinite(Rs).all() and np.abs(Rs[Rs != 0]).min() >= np.finfo(Rs.dtype).tiny     # the scaling was exact
    t, tag = C.scaled_truth(c["truth"], n, d, k), "*2^%d" % k
    R, O, b = _dev(Rs), _dev(Os), _dev(c["b"])
    b0 = b[:, :, 0].contiguous()
    _fused(chk, key, R, O, b0, t, c["cond"], u, n, d, tag)
    _factor(chk, key, R, O, b, t, c["cond"], u, n, d, tag)
    if n <= cr.BATCH_MAX_ROWS:
        # the scaled system next to the unscaled one in a dense batch
        Rb, Ob = torch.stack([R, _dev(c["Rs"])]), torch.stack([O, _dev(c["Os"])])
        m, ld = cr.mahal_and_det_batch(Rb, Ob, torch.stack([b0, b0]))
        assert bool(torch.isfinite(m).all()) and bool(torch.isfinite(ld).all()), (m, ld)
        for i, (ti, tg) in enumerate(((t, tag), (c["truth"], ""))):
            chk.add("mahal_and_det_batch[dense]", key, "mahal", C.m_mahal(m[i], ti, c["cond"], u), tg)
            chk.add("mahal_and_det_batch[dense]", key, "logdet", C.m_logdet(ld[i], ti, c["cond"], u, n, d), tg)
    chk.finish()


@pytest.mark.parametrize("case", [key + (k,) for key, ks in C.BEYOND.items() for k in ks], ids=_id)
def test_beyond_the_representable_block_determinant(case):
    """fp64.  d = 8: at 2^+-160 a block's determinant (~2^+-1280) is no double, at 2^-131 (~2^-1048) it is a denormal that
    has lost bits.  d = 4, whose in-LDS levels run on the MFMA and record-stage tiles that keep no factor: 2^+-260.
    A log-determinant there is accurate to the bound or not finite; finite and wrong is the failure.
    det(decompose(...)) sums logs of the factor's diagonal and has no such limit."""
    dtype, n, d, k = case
    key = C.scale_key(dtype, n, d)
    c, u, chk = C.case(key), C.eps_of(dtype), Checker()
    Rs, Os = C.scaled(c["Rs"], c["Os"], k)
    t, tag = C.scaled_truth(c["truth"], n, d, k), "*2^%d" % k
    R, O, b0 = _dev(Rs), _dev(Os), _dev(c["b"][:, :, 0])
    got = {"mahal_and_det": cr._mahal_and_det(R, O, b0, levelwise=False)[1],
           "mahal_and_det[levelwise]": cr._mahal_and_det(R, O, b0, levelwise=True)[1],
           "mahal_and_det_batch[dense]": cr.mahal_and_det_batch(R[None], O[None], b0[None])[1][0]}
    for name, ld in got.items():
        if bool(torch.isfinite(ld)):
            chk.add(name, key, "logdet", C.m_logdet(ld, t, c["cond"], u, n, d), tag)
        else:
            print("%-30s %s%s log-det %r: not finite, allowed here" % (name, _id(key), tag, float(ld)))
    chk.add("det", key, "logdet", C.m_logdet(cr.det(cr.decompose(R, O)), t, c["cond"], u, n, d), tag)
    chk.finish()


@pytest.mark.parametrize("d,ks", [(5, (12, 60)), (8, (7, 37))], ids=_id)
def test_block_determinants_far_apart_in_one_system(d, ks):
    """D J D with D = diag(2^k_i) per block row, k_i = ks[1] at every ninth row and ks[0] elsewhere (exact; SPD): the block
    determinants are ~2^(2 d k_i), about 1e36 and 1e180, inside one system, so a running product of pivots that has
    grown to ~1e144 over four rows meets a factor of ~1e180 (1025 rows are eight consecutive rows per lane and the
    period is nine, so every alignment occurs).  cond2 of such a system says nothing about its log-determinant, which
    is a sum of logs either way: every route is finite and within 4 x the larger of the oracle's own error and one
    rounding of the result, u |l*|."""
    n, u = 1025, C.eps_of("float64")
    c = C.case(("float64", "block", 0, n, d))
    k = np.where(np.arange(n) % 9 == 8, ks[1], ks[0])
    Rs = np.ldexp(c["Rs"], (2 * k)[:, None, None])
    Os = np.ldexp(c["Os"], (k[1:] + k[:-1])[:, None, None])
    b0 = np.ascontiguousarray(c["b"][:, :, 0])
    t = C.truth(Rs, Os, b0)
    assert abs(t["logdet"] - (c["truth"]["logdet"] + 2 * d * k.sum() * np.log(C.LD(2)))) <= 1e-15 * abs(t["logdet"])
    Rt, Ot, bt = torch.from_numpy(Rs), torch.from_numpy(Os), torch.from_numpy(b0)
    oracle = [float(cr_oracle.det(cr_oracle.decompose(Rt, Ot))), float(cr_oracle.mahal_and_det(Rt, Ot, bt)[1])]
    tol = 4 * max(max(abs(C.LD(v) - t["logdet"]) for v in oracle), u * abs(t["logdet"]))
    R, O, x = _dev(Rs), _dev(Os), _dev(b0)
    got = {"mahal_and_det": cr._mahal_and_det(R, O, x, levelwise=False), "mahal_and_det[levelwise]": cr._mahal_and_det(R, O, x, levelwise=True),
           "mahal_and_det_batch[dense]": tuple(v[0] for v in cr.mahal_and_det_batch(R[None], O[None], x[None])),
           "det": (None, cr.det(cr.decompose(R, O)))}
    bad = []
    for name, (m, ld) in got.items():
        err = abs(C.LD(float(ld)) - t["logdet"]) if bool(torch.isfinite(ld)) else float("inf")
        print("%-30s log-det %r truth %.17g error %.3g allowed %.3g" % (name, float(ld), float(t["logdet"]), float(err), float(tol)))
        if not err <= tol:
            bad.append((name, float(ld)))
        if m is not None:
            # (powers of two commute with every step: the error is that of the unscaled, well-conditioned system;
            # rtol of tests/test_hip_parity.py)
            assert abs(C.LD(float(m)) - t["mahal"]) <= 1e-9 * t["mahal"], (name, float(m), float(t["mahal"]))
    assert not bad, bad

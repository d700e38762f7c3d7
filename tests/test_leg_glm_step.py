"""ONE launch of cgps_leg_glm_step (csrc/cgps_leg_glm.h) against the exact reference of tests/_glmstepref.py:
every output at a general point, the whole ladder of step lengths, overflowed candidates, frozen series, and the saturated
Bernoulli line with its mirror image.  tests/test_leg_laplace.py sees only where the Newton loop ends, and Newton's method
corrects its own errors: a wrong gain, a wrong choice among the candidates, a wrong slope, a wrong CONVERGED / STALLED
decision and a wrong psi away from the mode all reach the same mode.  Here each has exactly one right answer: the cases
are built in tests/_glmstepref.py and tests/test_glmstepref.py asserts without a GPU that every one is admissible.

The prior blocks come from cgps_peg_precision_seg, as in a real call; the reference is evaluated on those very blocks
(and asserted admissible on them too), so the kernel and the reference read the same numbers."""
import types

import pytest
import torch

import _glmstepref as gs
from cyclic_gps import _hip, leg

F64, F32 = torch.float64, torch.float32
DTYPES = pytest.mark.parametrize("T", [F64, F32], ids=["fp64", "fp32"])
CODE = {"poisson": _hip.GLM_POISSON, "bernoulli": _hip.GLM_BERNOULLI, "gaussian": _hip.GLM_GAUSSIAN}
OUTPUTS = ("z_out", "J_Rs", "rhs", "psi")


def _launch(case, T, first=False, prop=None):
    """(the kernel's outputs on the CPU: z_out, J_Rs, rhs, state; the operands it read, as the reference takes them)"""
    g = lambda t: None if t is None else t.to(T).cuda().contiguous()      # noqa: E731
    R = sum(case.lengths)
    cut = torch.zeros(R - 1, dtype=torch.uint8)
    cut[torch.tensor(case.offsets[1:-1], dtype=torch.int64) - 1] = 1
    Rs, Os = leg._peg_precision_seg(g(case.ts), g(case.G), cut.cuda())
    plan = types.SimpleNamespace(offsets=torch.tensor(case.offsets, dtype=torch.int64).cuda(), B=len(case.lengths))
    op = leg._GlmOperands(plan, Rs, Os, g(case.ys), None if case.mask is None else case.mask.cuda(), g(case.offset),
                          g(case.extra), g(case.Bm), CODE[case.family], case.tol)
    ops = case.operands(T, blocks=(Rs.cpu(), Os.cpu()), first=first)
    if prop is not None:
        ops["prop"] = prop.to(T)
    dev = lambda t: None if t is None else t.cuda().contiguous()      # noqa: E731
    out = leg._glm_step_hip(op, dev(ops["z"]), dev(ops["prop"]), dev(ops["state_in"]))
    torch.cuda.synchronize()
    return [t.cpu() for t in out], ops


def _compare(what, out, ops, ref):
    """every assertion of one launch against its reference; returns the worst ratio of error to bound per output"""
    T = ops["z"].dtype
    eps = float(torch.finfo(T).eps)
    z_out, J_Rs, rhs, state = out
    offs = ops["offsets"]
    worst = dict.fromkeys(OUTPUTS, 0.0)
    assert all(not w for w in ref["why"]), (what, "not admissible on the blocks the device wrote", ref["why"])
    for b in range(len(offs) - 1):
        r0, r1 = offs[b], offs[b + 1]
        rows = slice(r0, r1)
        who = "%s series %d" % (what, b)
        alpha = float(state[b, 3])
        assert alpha == ref["alpha"][b], (who, "alpha", alpha, ref["alpha"][b], ref["gains"][b])
        assert float(state[b, 2]) == ref["flags"][b], (who, "flags", float(state[b, 2]), ref["flags"][b], ref["gains"][b], ref["slope"][b])
        assert float(state[b, 1]) == ref["iterations"][b], (who, "iterations", float(state[b, 1]), ref["iterations"][b])
        frozen = ops["prop"] is not None and not ref["active"][b]
        if frozen or ops["prop"] is None or alpha == 0.0:
            assert torch.equal(z_out[rows], ops["z"][rows]), (who, "z_out is not z")
        elif alpha == 1.0:
            assert torch.equal(z_out[rows], ops["prop"][rows]), (who, "z_out is not prop")
        else:
            err = (z_out[rows].to(F64) - ref["z_out"][rows]).abs()
            bound = 4 * eps * torch.maximum(ops["z"][rows].abs(), ops["prop"][rows].abs()).to(F64)
            worst["z_out"] = max(worst["z_out"], float((err / bound).max()))
            assert bool((err <= bound).all()), (who, "z_out", float((err / bound).max()))
        scale = 64 * eps * (1 + ref["eta_max"][b])
        for name, got, want, S in (("J_Rs", J_Rs, ref["J_Rs"], ref["J_S"]), ("rhs", rhs, ref["rhs"], ref["rhs_S"])):
            err, bound = (got[rows].to(F64) - want[rows]).abs(), scale * S[rows]
            ratio = float(torch.where(err > 0, err / bound, torch.zeros_like(err)).max())
            worst[name] = max(worst[name], ratio)
            assert bool((err <= bound).all()), (who, name, ratio)
        if frozen:
            assert torch.equal(state[b], ops["state_in"][b]), (who, "a frozen series' state changed")
        else:
            err, bound = abs(float(state[b, 0]) - ref["psi"][b]), scale * ref["psi_S"][b]
            worst["psi"] = max(worst["psi"], err / bound)
            assert err <= bound, (who, "psi", float(state[b, 0]), ref["psi"][b], err / bound)
    print("%s %s: worst error / bound  %s" % (what, "fp64" if T == F64 else "fp32", "  ".join("%s %.3f" % (k, worst[k]) for k in OUTPUTS)))
    return worst


def _expected(case, ref, what):
    """the reference decided what the builder aimed at (asserted on the CPU blocks by tests/test_glmstepref.py too)"""
    for key, want in case.expect.items():
        for b, w in enumerate(want):
            assert w is None or ref[key][b] == w, (what, key, b, ref[key][b], w)


# ---- a: every output at a general point ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("plain", [False, True], ids=["full", "plain"])
@pytest.mark.parametrize("d,obs", gs.FORMS)
@pytest.mark.parametrize("family", gs.FAMILIES)
def test_every_output_at_a_general_point(family, d, obs, plain, T):
    """random z, lengths (1, 2, 65, 131), active / CONVERGED / STALLED series mixed, steps that accept 1, 1/2 and 1/4; and the
    first call of a loop (no proposal, no state) at the same z"""
    case = gs.point_case(family, d, obs, plain)
    what = "%s d %d obs %d %s" % (family, d, obs, "plain" if plain else "full")
    out, ops = _launch(case, T)
    ref = gs.reference(ops)
    _expected(case, ref, what)
    _compare(what + " step", out, ops, ref)
    out, ops = _launch(case, T, first=True)
    _compare(what + " first call", out, ops, gs.reference(ops))
    assert float(out[3][:, 1:].abs().max()) == 0.0


# ---- b: the whole ladder in one launch -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("tol", gs.TOL_LADDER)
@pytest.mark.parametrize("family", gs.FAMILIES)
def test_the_whole_ladder_in_one_launch(family, tol, T):
    """series k must accept exactly 2^-k, k = 0..11; then nothing qualifies (STALLED), a descent direction, a small descent
    step (STALLED at tol = 1e-3, CONVERGED at the large tol), a small ascent step (CONVERGED), an ordinary one"""
    case = gs.ladder_case(family, tol)
    what = "ladder %s tol %g" % (family, tol)
    out, ops = _launch(case, T)
    ref = gs.reference(ops)
    _expected(case, ref, what)
    _compare(what, out, ops, ref)
    state = out[3]
    assert state[:12, 3].tolist() == [2.0 ** -k for k in range(12)]
    assert state[12:, 3].tolist() == [0.0, 0.0, 0.0, 1.0, 1.0]
    assert int(state[12, 2]) == _hip.GLM_STALLED and int(state[15, 2]) == _hip.GLM_CONVERGED
    assert int(state[14, 2]) == (_hip.GLM_STALLED if tol < 0.1 else _hip.GLM_CONVERGED)


# ---- c: overflowed candidates ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@DTYPES
def test_overflowed_candidates_are_passed_over(T):
    """Poisson: e^eta overflows in T at alpha = 1 .. 2^-j and the next candidate is the likelihood's mode: it must be the
    one accepted (j = 0, 2, 5).  A series whose twelve candidates all overflow stalls at z, and everything stays finite."""
    case = gs.overflow_case(T)
    out, ops = _launch(case, T)
    ref = gs.reference(ops)
    _expected(case, ref, "overflow")
    _compare("overflow", out, ops, ref)
    z_out, J_Rs, rhs, state = out
    assert state[:, 3].tolist() == [0.5, 0.125, 2.0 ** -6, 0.0] and int(state[3, 2]) == _hip.GLM_STALLED
    assert torch.equal(z_out[6:8], ops["z"][6:8])
    for t in out:
        assert bool(torch.isfinite(t).all())


# ---- d: frozen means not read ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("family", gs.FAMILIES)
def test_a_frozen_series_does_not_read_its_proposal(family, T):
    case = gs.point_case(family, 5, 3, False)
    clean, ops = _launch(case, T)
    offs = ops["offsets"]
    flagged = [b for b in range(len(offs) - 1) if int(ops["state_in"][b, 2]) != 0]
    assert flagged and len(flagged) < len(offs) - 1
    prop = ops["prop"].clone()
    for b in flagged:
        prop[offs[b]:offs[b + 1]] = float("nan")
    nan, ops_nan = _launch(case, T, prop=prop)
    assert bool(torch.isnan(ops_nan["prop"]).any())
    first, _ = _launch(case, T, first=True)
    for b in range(len(offs) - 1):
        rows = slice(offs[b], offs[b + 1])
        if b in flagged:
            assert torch.equal(nan[3][b], ops["state_in"][b]), (b, "state")
            for k, name in enumerate(("z_out", "J_Rs", "rhs")):
                assert torch.equal(nan[k][rows], first[k][rows]), (b, name, "is not what the first call writes at the same z")
        else:
            assert torch.equal(nan[3][b], clean[3][b]), (b, "state of an active neighbour")
            assert float(clean[3][b, 3]) != 0.0                                   # (it did step)
            for k, name in enumerate(("z_out", "J_Rs", "rhs")):
                assert torch.equal(nan[k][rows], clean[k][rows]), (b, name, "of an active neighbour")
    for t in nan:
        assert bool(torch.isfinite(t).all())


# ---- e: the saturated Bernoulli line, and its mirror image ---------------------------------------------------------------------
@pytest.mark.gpu
@DTYPES
def test_the_saturated_bernoulli_line_and_its_mirror_image(T):
    """eta = +5 .. +40 and steps of dEta = -5 .. -45: with l(eta + t) - l(eta) = y t - log1p(sigma(eta) expm1(t)) the
    argument of log1p is (1 - sigma) + sigma e^t computed from two numbers near 1; at eta >= 18, t <= -20 (fp32) and
    eta >= 38, t <= -40 (fp64) it rounded to -1 and the gain to +inf, so a legitimate step was rejected, where the mirror
    image (1 - y, -eta, -t), the same posterior, was accurate to an eps.  Before the flipped form for eta > 0
    this test failed on an MI355X: in fp32 the series 3 (E, T = 18, 20), 5 (25, 30), 6 (38, 40) and 7 (39, 44) took 1/2, 1/2,
    1/4 and 1/4 where the reference, and their own mirror images, take 1, 1, 1 and 1/2; in fp64 series 6 took 1/2 for 1."""
    case = gs.saturated_case()
    out, ops = _launch(case, T)
    ref = gs.reference(ops)
    _expected(case, ref, "saturated")
    state = out[3]
    n = len(case.lengths) // 2
    print("saturated %s: alpha %s\n          reference %s" % ("fp64" if T == F64 else "fp32", state[:, 3].tolist(), ref["alpha"]))
    _compare("saturated", out, ops, ref)
    eps = float(torch.finfo(T).eps)
    for b in range(n):
        assert float(state[b, 3]) == float(state[n + b, 3]), (b, "alpha and its mirror", state[b].tolist(), state[n + b].tolist())
        assert float(state[b, 2]) == float(state[n + b, 2]), (b, "flags and their mirror")
        bound = 64 * eps * (1 + ref["eta_max"][b]) * ref["psi_S"][b]
        assert abs(float(state[b, 0]) - float(state[n + b, 0])) <= bound, (b, "psi and its mirror", float(state[b, 0]), float(state[n + b, 0]))
    r0 = ops["offsets"][n]
    assert torch.equal(out[0][:r0], -out[0][r0:])                                 # the mirrored mode, bit for bit

"""The dense truth of tests/_laplacegradref.py held to checks of its own, on exactly the cases the GPU tests of
tests/test_leg_laplace_grad.py use: its gradient against finite differences of the converged evidence, the Gaussian
family against the closed form, and that every case converges.  CPU only."""
import pytest
import torch

import _laplacegradref as gr

CASES = gr.all_cases()
# Finite differences are the weaker side: for every parameter group on its own (N, R, B, offset, ts, log_exposure or
# noise_var) a directional derivative along a random direction in that group, central differences at h = 1e-3 and h / 2
# with Richardson extrapolation, against the reference's gradient along the same direction, as a fraction of
# |gradient of the group| |direction|.  Measured once over all cases and groups: the worst is FD_WORST, in dE/dN at
# rank 1 (the differences carry the rounding of the evidence, 1e-16 |E| / h, about 1e-11 whatever the group: a group
# whose gradient is small has it as a larger fraction; over all parameters jointly the worst was 1.0e-11); the bound is
# 10 x that.  A group whose gradient is zero by structure (no
# two observed rows in any series: nothing depends on N, R or ts; below ZERO_GROUP of the whole gradient) has no size of
# its own: there the finite difference must vanish to the same bound taken of the whole gradient's size.
FD_WORST = 8.603e-08
FD_BOUND = 10 * FD_WORST
ZERO_GROUP = 1e-9


@pytest.mark.parametrize("name,case", CASES, ids=[n for n, _ in CASES])
def test_the_gradient_agrees_with_finite_differences(name, case):
    bad = []
    for group, analytic, fd, scale, scale_all in gr.directional_fd(case):
        structural_zero = scale <= ZERO_GROUP * scale_all
        size = scale_all if structural_zero else scale
        print("%s %s: directional derivative %.12g, finite differences %.12g, |g||v| %.3g%s, difference / |g||v| %.3e"
              % (name, group, analytic, fd, size, " (whole gradient)" if structural_zero else "", abs(analytic - fd) / size))
        if not abs(analytic - fd) <= FD_BOUND * size:
            bad.append((group, analytic, fd, size))
    assert not bad, (name, bad)


@pytest.mark.parametrize("name,case", [c for c in CASES if c[1].family == "gaussian"], ids=lambda v: v if isinstance(v, str) else "")
def test_the_gaussian_family_is_the_closed_form(name, case):
    """rtol 1e-10 entry by entry; where the closed form is exactly zero (a series that observes nothing) the implicit
    route leaves rounding, so an atol of 1e-10 x the largest entry of all the case's gradients goes with it"""
    ref = gr.gradients(case)
    want = gr.gaussian_gradients(case)
    scale = max(float(w.abs().max()) for w in want if w.numel())
    for k, (g, w) in enumerate(zip(ref["flat_grads"], want)):
        assert bool(((g - w).abs() <= 1e-10 * w.abs() + 1e-10 * scale).all()), (name, k, float((g - w).abs().max()))


@pytest.mark.parametrize("name,case", CASES, ids=[n for n, _ in CASES])
def test_every_case_converges(name, case):
    if name not in ("ascent", "ill-conditioned"):        # (ascent asks a sign, not digits; the other is what its name says)
        assert gr.prior_condition(case) <= gr.COND_MAX
    ref = gr.gradients(case)
    assert ref["last_step"] < gr.NEWTON_TOL and bool(torch.isfinite(ref["E"]).all())
    for t in case.truths():
        assert t["iterations"] < 100
    # the two modes (covariance form there, precision form here) are the same point
    mean = torch.cat([t["mean"] for t in case.truths()])
    assert float((mean - ref["mean"]).abs().max()) <= 1e-9 * max(1.0, float(mean.abs().max()))

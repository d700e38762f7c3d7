"""The dense truth of the Laplace tests (tests/_laplaceref.py) held to what it cannot get wrong twice, on every input
tests/test_leg_laplace.py uses: the mode is stationary, the Gaussian family reproduces the closed-form dense Gaussian,
and the iteration converges well inside the library's default ``max_iter`` -- the condition that makes
``converged.all()`` a fair assertion on the GPU.  No GPU, no kernel, no precision block."""
import pytest
import torch

import _laplaceref as lr

CASES = lr.all_cases()


@pytest.mark.parametrize("name,case", CASES, ids=[n for n, _ in CASES])
def test_the_mode_is_stationary_and_found_quickly(name, case):
    for b, t in enumerate(case.truths()):
        assert t["iterations"] < 25, (name, b, t["iterations"])
        if t["f"].numel():
            resid = float((t["f"] - t["C"] @ t["g"]).abs().max())
            assert resid <= 1e-10, (name, b, resid)
        assert torch.isfinite(t["mean"]).all() and torch.isfinite(t["cov_diag"]).all()
        assert float(torch.linalg.eigvalsh(t["cov_diag"]).min()) > 0


@pytest.mark.parametrize("name,case", [c for c in CASES if c[1].family == "gaussian"], ids=[c[0] for c in CASES if c[1].family == "gaussian"])
def test_the_gaussian_family_is_the_closed_form(name, case):
    for b, t in enumerate(case.truths()):
        if not t["f"].numel():
            continue
        mean, cov, ev = lr.gaussian_closed_form(t)
        n, d = t["mean"].shape
        i = torch.arange(n)
        cov = cov.reshape(n, d, n, d)
        assert float((t["mean"].reshape(-1) - mean).abs().max()) <= 1e-10, (name, b)
        assert float((t["cov_diag"] - cov[i, :, i, :]).abs().max()) <= 1e-10, (name, b)
        if n > 1:
            assert float((t["cov_off"] - cov[i[1:], :, i[:-1], :]).abs().max()) <= 1e-10, (name, b)
        assert abs(t["log_evidence"] - ev) <= 1e-10, (name, b, t["log_evidence"], ev)
        assert t["iterations"] <= 2


def test_the_large_counts_need_the_step_halving():
    """the case that tests the damping: an undamped first step overflows e^eta"""
    case = lr.damping_case()
    t = case.truths()[0]
    assert float(t["y"].min()) > 900 and float((t["f"] + t["shift"]).min()) > 6.0
    g, W = lr.grad_weight("poisson", t["y"], torch.zeros_like(t["y"]))
    full_step = t["C"] @ (g - W.sqrt() * torch.linalg.solve(torch.eye(g.numel(), dtype=lr.F64) + W.sqrt()[:, None] * t["C"] * W.sqrt()[None, :],
                                                              W.sqrt() * (t["C"] @ g)))
    assert float(full_step.max()) > 100.0                            # exp of it is inf in fp32, of 1000 / 710 in fp64

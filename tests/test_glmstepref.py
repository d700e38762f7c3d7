"""The exact reference of one Laplace Newton step (tests/_glmstepref.py) held to its own checks, without a GPU, on exactly the
launches tests/test_leg_glm_step.py makes: every one is admissible in both precisions (so the GPU tests skip and filter
nothing), the mpmath gains are those of an fp64 torch evaluation of the direct definition, a Gaussian step to the exact
Newton point gains |grad psi . delta| / 2, and every builder hits what it aimed at."""
import pytest
import torch

import _glmstepref as gs

F64, F32 = torch.float64, torch.float32
CASES = gs.all_cases()


@pytest.mark.parametrize("name,builder,args,dtypes", CASES, ids=[c[0] for c in CASES])
def test_every_gpu_case_is_admissible(name, builder, args, dtypes):
    case = builder(*args)
    for T in dtypes:
        ref = gs.reference_of(builder, args, T)
        assert all(not w for w in ref["why"]), (name, T, ref["why"])
        for key, want in case.expect.items():                     # the builder hit what it aimed at
            for b, w in enumerate(want):
                assert w is None or ref[key][b] == w, (name, T, key, b, ref[key][b], w)
    if len(dtypes) == 2:                                           # one case, two precisions: the same decisions
        a, b = (gs.reference_of(builder, args, T) for T in dtypes)
        assert a["alpha"] == b["alpha"] and a["flags"] == b["flags"], name


@pytest.mark.parametrize("name,builder,args,dtypes", [c for c in CASES if c[0].startswith(("point", "ladder"))],
                         ids=[c[0] for c in CASES if c[0].startswith(("point", "ladder"))])
def test_the_gains_are_those_of_the_direct_definition_in_fp64(name, builder, args, dtypes):
    """unsaturated cases, every gain the step depends on (those up to the accepted candidate); candidates whose e^eta
    overflows fp64 in torch (the far rungs of the Poisson ladder) are left out"""
    ops = builder(*args).operands(F32)
    ref = gs.reference_of(builder, args, F32)
    z, prop = ops["z"].to(F64), ops["prop"].to(F64)
    seg = gs.series_of_rows(ops["offsets"])
    psi0 = gs.psi_torch(ops, z)
    worst, count = 0.0, 0
    for k in range(gs.CANDIDATES):
        gk = gs.psi_torch(ops, z + 0.5 ** k * (prop - z)) - psi0
        for b, active in enumerate(ref["active"]):
            if active and k < len(ref["gains"][b]) and bool(torch.isfinite(gk[b])) and ref["gain_S"][b][k] < 1e300:
                err = abs(float(gk[b]) - ref["gains"][b][k]) / ref["gain_S"][b][k]
                worst, count = max(worst, err), count + 1
                assert err <= 1e-9, (name, b, k, float(gk[b]), ref["gains"][b][k])
    print("%s: %d gains, worst |torch - mpmath| / S = %.2e" % (name, count, worst))
    assert count >= 2
    assert seg.shape[0] == z.shape[0]


@pytest.mark.parametrize("d,obs", gs.FORMS)
def test_a_gaussian_newton_step_gains_half_its_slope(d, obs):
    """psi is quadratic for the Gaussian family: at prop = J^-1 rhs, the exact Newton point, gain = grad psi . delta / 2"""
    import mpmath
    case = gs.point_case("gaussian", d, obs, False)
    ops = case.operands(F64)
    ops["state_in"] = ops["state_in"].clone()
    ops["state_in"][:, 2] = 0
    first = gs.reference(dict(ops, prop=None, state_in=None))
    offs = ops["offsets"]
    prop = torch.zeros_like(ops["z"])
    for b in range(len(offs) - 1):
        r0, r1 = offs[b], offs[b + 1]
        n = r1 - r0
        J = torch.zeros(n * d, n * d, dtype=F64)
        for i in range(n):
            J[i * d:(i + 1) * d, i * d:(i + 1) * d] = first["J_Rs"][r0 + i]
            if i + 1 < n:
                J[(i + 1) * d:(i + 2) * d, i * d:(i + 1) * d] = ops["Os"][r0 + i]
                J[i * d:(i + 1) * d, (i + 1) * d:(i + 2) * d] = ops["Os"][r0 + i].T
        prop[r0:r1] = torch.linalg.solve(J, first["rhs"][r0:r1].reshape(-1)).reshape(n, d)
    ref = gs.reference(dict(ops, prop=prop), all_gains=True)
    for b in range(len(offs) - 1):
        gain, slope = ref["gains"][b][0], ref["slope"][b]
        assert slope > 0 and ref["alpha"][b] == 1.0
        # prop solves J prop = rhs in fp64: the step is Newton's to about eps64 cond(J), the identity holds to that
        assert abs(gain - 0.5 * slope) <= 1e-9 * slope, (b, gain, slope)
        # half the step gains three quarters of it
        assert abs(ref["gains"][b][1] - 0.75 * gain) <= 1e-9 * slope
    assert mpmath.mp.dps < gs.DPS                                  # the reference leaves the global precision alone

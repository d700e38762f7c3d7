"""The references of tests/_filtergradref.py, without a GPU.

(a) the differentiable recursion against an independent truth: the gradient of loglik in N, R, B, Lambda, xs, ts against
    ``_gradref.leg_dense_value_and_grads``, the dense Gaussian density, which has no filtering algebra.
(b) the explicit reverse walk against autograd of (a), under random cotangents on every output and on the end state, with
    a mask, variances, a start state, a zero gap and a row that observes nothing.
Bound, both: the project's gradient bound of tests/test_gradients.py -- rtol 1e-7, atol 1e-10 x the largest reference entry,
per gradient tensor.  And the C entry's argument checks, which run on the host."""
import ctypes

import numpy as np
import pytest
import torch

import _filtergradref as fg
import _gradref
from cyclic_gps import _hip
from test_leg_posterior_batch import _model, _series

F64 = torch.float64


def check(got, want, what):
    want = want.detach().to("cpu", F64)
    got = got.detach().to("cpu", F64)
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    scale = float(want.abs().max()) if want.numel() else 0.0
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-7, atol=1e-10 * scale, err_msg=what)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("d,obs,n", [(1, 1, 1), (1, 1, 2), (5, 1, 7), (5, 3, 7), (8, 8, 6)])
def test_the_differentiable_recursion_against_the_dense_density(d, obs, n, seed):
    _, mats = _model(d, obs, 40 + seed)
    ts, xs, _, _ = _series(obs, [n], 50 + seed)[0]
    ll, want = _gradref.leg_dense_value_and_grads(*mats, ts, xs)
    leaves = [t.detach().clone().requires_grad_(True) for t in mats + (xs, ts)]
    out = fg.filter_diff(tuple(leaves[:4]), leaves[5], leaves[4])
    assert abs(float(out["loglik"].detach()) - float(ll)) <= 1e-9 * max(1.0, abs(float(ll)))
    got = torch.autograd.grad(out["loglik"], leaves, allow_unused=True)      # (n = 1: no gap, so G and ts are not used)
    got = [torch.zeros_like(l) if g is None else g for g, l in zip(got, leaves)]
    for name, a, b in zip(("N", "R", "B", "Lambda", "xs", "ts"), got, want):
        check(a, b, "d %d obs %d n %d seed %d: %s" % (d, obs, n, seed, name))


def adjoint_case(d, obs, seed, with_init=True, with_mask=True, with_noise=True, n=7):
    """One series of n rows with a zero gap (rows 2, 3 share a time stamp), a start state, and (mask) an interior row and the
    first row observing nothing, NaN where nothing is observed; random cotangents for every output and the end state."""
    gen = torch.Generator().manual_seed(seed)
    _, mats = _model(d, obs, seed)
    ts, xs, mask, s = _series(obs, [n], seed + 1)[0]
    ts = ts.clone()
    if n > 3:
        ts[3] = ts[2]
    if with_mask:
        mask = mask.clone()
        mask[n // 2] = False
        mask[0] = False
        if n > 1:
            mask[1, 0] = True
        xs = torch.where(mask, xs, torch.full_like(xs, float("nan")))
        s = torch.where(mask, s, torch.full_like(s, float("nan")))
    else:
        mask = None
    if not with_noise:
        s = None
    init = None
    if with_init:
        W = torch.randn(d, d, generator=gen, dtype=F64)
        init = (ts[0] - 0.4, torch.randn(d, generator=gen, dtype=F64), 0.5 * torch.eye(d, dtype=F64) + 0.1 * W @ W.T)
    r = lambda *shape: torch.randn(*shape, generator=gen, dtype=F64)      # noqa: E731
    cot = {"mean": r(n, obs), "cov": r(n, obs, obs), "logpdf": r(n), "z_mean": r(n, d), "z_cov": r(n, d, d), "loglik": r(()),
           "state_mean": r(d), "state_cov": r(d, d)}
    return mats, ts, xs, s, mask, init, cot


def autograd_of_a(mats, ts, xs, s, mask, init, cot, through_operands=False):
    """Gradients of <cotangents, outputs of (a)> in a dict: N, R, B, Lambda (or G, B, LLT), xs, ts, s, t0, m0, P0."""
    leaf = lambda t: None if t is None else t.detach().clone().requires_grad_(True)      # noqa: E731
    xs_l, ts_l, s_l = leaf(xs), leaf(ts), leaf(s)
    init_l = None if init is None else tuple(leaf(t) for t in init)
    if through_operands:
        ops = [leaf(t) for t in fg.operands(mats)]
        out = fg.filter_diff_operands(*ops, ts_l, xs_l, s_l, mask, init_l)
        named = dict(zip(("G", "B", "LLT"), ops))
    else:
        ms = [leaf(t) for t in mats]
        out = fg.filter_diff(tuple(ms), ts_l, xs_l, s_l, mask, init_l)
        named = dict(zip(("N", "R", "B", "Lambda"), ms))
    total = sum((cot[k] * out[k]).sum() for k in fg.KEYS if cot.get(k) is not None)
    if cot.get("loglik") is not None:
        total = total + cot["loglik"] * out["loglik"]
    if cot.get("state_mean") is not None:
        total = total + (cot["state_mean"] * out["state"][1]).sum() + (cot["state_cov"] * out["state"][2]).sum()
    named.update(xs=xs_l, ts=ts_l)
    if s_l is not None:
        named["s"] = s_l
    if init_l is not None:
        named.update(t0=init_l[0], m0=init_l[1], P0=init_l[2])
    keys = list(named)
    if not (isinstance(total, torch.Tensor) and total.requires_grad):      # (one unobserved row from the prior: constants)
        return {k: torch.zeros_like(named[k]) for k in keys}
    grads = torch.autograd.grad(total, [named[k] for k in keys], allow_unused=True)
    return {k: (torch.zeros_like(named[k]) if g is None else g) for k, g in zip(keys, grads)}


def reverse_walk(mats, ts, xs, s, mask, init, cot, dtype=F64):
    """(b) in ``dtype`` from the states that the recursion in that dtype saves: the same dict as ``autograd_of_a`` gives,
    with both the operands' and the matrices' gradients."""
    c = lambda t: None if t is None else t.detach().to(dtype)      # noqa: E731
    G, Bm, LLT = (t.detach() for t in fg.operands(mats, dtype))
    init_c = None if init is None else tuple(c(t) for t in init)
    with torch.no_grad():
        fwd = fg.filter_diff_operands(G, Bm, LLT, c(ts), c(xs), c(s), mask, init_c)
    res = fg.filter_adjoint_ref(G, Bm, LLT, c(ts), c(xs), c(s), mask, init_c, fwd["z_mean"], fwd["z_cov"],
                                {k: c(v) for k, v in cot.items()})
    gt, gt0 = fg.gap_to_times(res["gap"], init is not None)
    Nb, Rb, Bb, Lb = fg.matrix_grads(mats, res["G"], res["B"], res["LLT"])
    out = {"G": res["G"], "B": Bb, "LLT": res["LLT"], "N": Nb, "R": Rb, "Lambda": Lb, "xs": res["xs"], "ts": gt}
    if s is not None:
        out["s"] = res["s"]
    if init is not None:
        out.update(t0=gt0, m0=res["m0"], P0=res["P0"])
    return out


@pytest.mark.parametrize("with_init,with_mask,with_noise", [(True, True, True), (False, True, True), (True, False, False),
                                                            (False, False, True), (True, True, False)])
@pytest.mark.parametrize("d,obs", [(1, 1), (2, 3), (5, 1), (5, 3), (8, 8), (3, 5)])
def test_the_reverse_walk_against_autograd_of_the_recursion(d, obs, with_init, with_mask, with_noise):
    case = adjoint_case(d, obs, 900 + 10 * d + obs, with_init, with_mask, with_noise)
    mats, ts, xs, s, mask, init, cot = case
    assert float(ts[3] - ts[2]) == 0.0
    got = reverse_walk(*case)
    for through in (True, False):
        want = autograd_of_a(*case, through_operands=through)
        for key, w in want.items():
            check(got[key], w, "d %d obs %d init %s mask %s noise %s: %s" % (d, obs, with_init, with_mask, with_noise, key))
    if with_mask:
        assert not bool(mask[0].any()) and not bool(mask[len(ts) // 2].any()) and bool(torch.isnan(xs[~mask]).all())
        assert bool((got["xs"][~mask] == 0).all()) and torch.equal(torch.isnan(got["xs"]), torch.zeros_like(mask))
        if with_noise:
            assert bool((got["s"][~mask] == 0).all()) and not bool(torch.isnan(got["s"]).any())


def test_single_cotangents_and_a_series_of_one_row():
    """Each cotangent alone (the others absent, not zero), and n = 1 with and without a start state."""
    for key in fg.KEYS + ("loglik",):
        mats, ts, xs, s, mask, init, cot = adjoint_case(5, 3, 77)
        only = {key: cot[key]}
        got, want = reverse_walk(mats, ts, xs, s, mask, init, only), autograd_of_a(mats, ts, xs, s, mask, init, only)
        for k, w in want.items():
            check(got[k], w, "only %s: %s" % (key, k))
    for with_init in (True, False):
        case = adjoint_case(5, 3, 78, with_init, False, True, n=1)
        got, want = reverse_walk(*case), autograd_of_a(*case)
        for k, w in want.items():
            check(got[k], w, "n = 1 init %s: %s" % (with_init, k))


def test_the_adjoint_entry_checks_its_arguments_on_the_host():
    lib = _hip.lib()
    b = ctypes.c_size_t(0)
    assert lib.cgps_leg_filter_adjoint_workspace_bytes(10, 2, 3, 5, 3, _hip.F64, ctypes.byref(b)) == 0
    assert b.value >= 3 * 10 * 25 * 8 and b.value % 256 == 0
    assert lib.cgps_leg_filter_adjoint_workspace_bytes(10, 2, 3, 5, 3, _hip.F32, ctypes.byref(b)) == 0 and b.value >= 3 * 10 * 25 * 4
    assert lib.cgps_leg_filter_adjoint_workspace_bytes(10, 2, 3, 9, 3, _hip.F64, ctypes.byref(b)) == 1
    assert lib.cgps_leg_filter_adjoint_workspace_bytes(10, 2, 3, 5, 9, _hip.F64, ctypes.byref(b)) == 1
    assert lib.cgps_leg_filter_adjoint_workspace_bytes(10, 2, 3, 5, 3, _hip.F64, None) == 1
    none = [None] * 4
    call = lambda d, obs: lib.cgps_leg_filter_adjoint(*none, 2, 10, 3, None, None, None, d, obs, _hip.F64, *([None] * 11), 0,      # noqa: E731
                                                      *([None] * 9))
    assert call(5, 3) == 1 and b"null pointer" in lib.cgps_last_error()
    assert call(9, 3) == 1 and call(0, 3) == 1 and call(5, 0) == 1 and call(5, 9) == 1
    assert "cgps_leg_filter_adjoint" in _hip.exported_symbols() and "cgps_leg_filter_adjoint_workspace_bytes" in _hip.exported_symbols()

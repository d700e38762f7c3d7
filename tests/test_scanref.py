"""The five-phase time-parallel filter of tests/_scanref.py (what cgps_leg_filter_scan evaluates: DESIGN.md 4.23) in
fp64 against the serial recursion of ``_filterref.filter_ref``: 1e-9 relative to 1 + |value|, with a mask and
variances, at gap scales 1 and 1e-6.  Also the algebra the kernels rest on: the combine is associative, composing
with a single row through the obs x obs factor is the general combine with that row's element, and a reset on the
right is selected bit for bit whatever the left operand holds.  CPU only."""
import pytest
import torch

import _filterref
import _noiseref as nr
import _scanref as sr

F64 = torch.float64
CASES = [(1, 1, 9, 1, 2), (5, 1, 131, 4, 4), (5, 3, 131, 4, 2), (8, 8, 70, 3, 3)]
BOUND = 1e-9
KEYS = ("mean", "cov", "logpdf", "z_mean", "z_cov")


def _rel(got, want):
    return float(((got - want).abs() / (1 + want.abs())).max())


def _case(d, obs, n, seed, scale):
    (Nm, Rm, Bm, Lm, xs, ts, s), mask = nr.leg_case(d, obs, n, seed)
    return (Nm, Rm, Bm, Lm), ts[0] + (ts - ts[0]) * scale, xs, s, mask


@pytest.mark.parametrize("scale", [1.0, 1e-6])
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("d,obs,n,L,F", CASES)
def test_scan_matches_the_serial_recursion(d, obs, n, L, F, seed, scale):
    mats, ts, xs, s, mask = _case(d, obs, n, seed, scale)
    want = _filterref.filter_ref(mats, ts, xs, s, mask)
    got = sr.scan_filter_ref(mats, [(ts, xs, s, mask, None)], L, F)[0]
    worst = {k: _rel(got[k], want[k]) for k in KEYS}
    worst["loglik"] = _rel(got["loglik"], want["loglik"])
    worst["state"] = max(_rel(got["state"][1], want["state"][1]), _rel(got["state"][2], want["state"][2]))
    print("d %d obs %d n %d L %d F %d seed %d scale %g: %s" % (d, obs, n, L, F, seed, scale, worst))
    assert all(v <= BOUND for v in worst.values()), worst


def test_scan_of_several_series_with_and_without_init():
    """Three series in one segmented scan, the middle one continued from a state: each equals its serial recursion."""
    mats, ts, xs, s, mask = _case(5, 3, 40, 3, 1.0)
    head = _filterref.filter_ref(mats, ts[:11], xs[:11], s[:11], mask[:11])
    series = [(ts[:9], xs[:9], s[:9], mask[:9], None), (ts[11:], xs[11:], s[11:], mask[11:], head["state"]),
              (ts[20:27], xs[20:27], None, None, None)]
    got = sr.scan_filter_ref(mats, series, 4, 2)
    for g, (t, x, s_, m_, init) in zip(got, series):
        want = _filterref.filter_ref(mats, t, x, s_, m_, init=init)
        assert all(_rel(g[k], want[k]) <= BOUND for k in KEYS) and _rel(g["loglik"], want["loglik"]) <= BOUND


def _random_elements(d, obs, seed, k):
    (Nm, Rm, Bm, Lm, xs, ts, s), mask = nr.leg_case(d, obs, k, seed)
    G = Nm @ Nm.T + Rm - Rm.T + 1e-5 * torch.eye(d, dtype=F64)
    LLT = Lm @ Lm.T + 1e-9 * torch.eye(obs, dtype=F64)
    parts = []
    for i in range(k):
        E, Q = sr.gap_pair(G, 0.3 + 0.2 * i)
        parts.append((E, Q, Bm, LLT + torch.diag(s[i]), xs[i]))
    return parts


@pytest.mark.parametrize("d,obs", [(1, 1), (5, 3), (8, 8)])
def test_combine_is_associative_and_agrees_with_the_single_row_form(d, obs):
    for seed in range(3):
        parts = _random_elements(d, obs, seed, 4)
        a, b, c, e = (sr.row_element(*p) for p in parts)
        ab, bc = sr.combine(a, b), sr.combine(b, c)
        left, right = sr.combine(sr.combine(ab, c), e), sr.combine(a, sr.combine(bc, e))
        for x, y in zip(left, right):
            assert float((x - y).abs().max()) <= 1e-10
        chain = sr.compose_row(sr.compose_row(sr.compose_row(a, *parts[1]), *parts[2]), *parts[3])
        for x, y in zip(chain, left):
            assert float((x - y).abs().max()) <= 1e-10
        first = sr.compose_row(sr.identity_element(d, F64), *parts[0])
        for x, y in zip(first, a):
            assert float((x - y).abs().max()) <= 1e-10


def test_a_reset_on_the_right_is_selected_bit_for_bit():
    d = 5
    a, b = (sr.row_element(*p) for p in _random_elements(d, 2, 7, 2))
    reset = sr.reset_element(b[1].clone(), b[2].clone())
    poisoned = tuple(torch.full_like(t, float("nan")) for t in a)
    for left in (a, poisoned):
        out = sr.combine(left, reset, reset2=True)
        assert all(torch.equal(x, y) for x, y in zip(out, reset))
    assert not any(bool(torch.isnan(t).any()) for t in sr.combine(poisoned, reset, reset2=True))
    assert all(bool(torch.isnan(t).all()) for t in sr.combine(poisoned, b)[:3])

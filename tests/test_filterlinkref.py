"""The time-parallel backward of the LEG filter without a GPU: the linking law on reference (b) of
tests/_filtergradref.py, the structure it rests on, ``leg._filter_link_scan`` against the serial composition loop, and
the checks of ``backward_chunk_rows=``.

Bounds.  The linked backward against the reverse walk over the whole series: 1e-12 of the largest reference entry per
tensor (both are the same formulas in fp64; the chunk maps add d + 1 products per chunk; worst seen 1.9e-14).  The
congruence PhiT Db PhiT^T and the scan against the loop: 1e-13 of the largest reference entry (a few dozen products of
O(1) matrices in fp64, each within a few eps)."""
import pytest
import torch

import _filtergradref as fg
import _filterlinkref as fl
from cyclic_gps import leg
from test_filtergradref import adjoint_case
from test_leg_posterior_batch import _model, _series

F64 = torch.float64
N_ROWS = 11


def _err(got, want):
    scale = float(want.abs().max())
    return float((got - want).abs().max()) / (scale if scale > 0 else 1.0)


def _saved(case):
    """(operands, data, init, z_mean, z_cov) of an ``adjoint_case``"""
    mats, ts, xs, s, mask, init, _ = case
    ops = tuple(t.detach() for t in fg.operands(mats))
    with torch.no_grad():
        fwd = fg.filter_diff_operands(*ops, ts, xs, s, mask, init)
    return ops, (ts, xs, s, mask), init, fwd["z_mean"], fwd["z_cov"]


@pytest.mark.parametrize("with_init", [False, True], ids=["prior", "init"])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "mask+variances"])
@pytest.mark.parametrize("d,obs", [(1, 1), (1, 2), (3, 1), (3, 2)])
@pytest.mark.parametrize("L", [1, 2, 4, N_ROWS])
def test_the_linking_law_on_the_reverse_walk(L, d, obs, masked, with_init):
    case = adjoint_case(d, obs, 500 + 10 * d + obs, with_init, masked, masked, n=N_ROWS)
    ops, data, init, zm, zc = _saved(case)
    cot = case[6]
    assert all(cot[k] is not None for k in fg.KEYS + ("loglik", "state_mean", "state_cov"))
    want = fg.filter_adjoint_ref(*ops, *data, init, zm, zc, cot)
    got = fl.linked_adjoint(*ops, *data, init, zm, zc, cot, L)
    assert len(fl.chunk_bounds(N_ROWS, L)) == -(-N_ROWS // L)
    assert set(got) == set(want)
    worst = max((_err(got[k], want[k]), k) for k in want)
    print("linking law L %d d %d obs %d: worst %.3e (%s)" % (L, d, obs, worst[0], worst[1]))
    for k in want:
        assert got[k].shape == want[k].shape and _err(got[k], want[k]) <= 1e-12, (k, _err(got[k], want[k]))


@pytest.mark.parametrize("d,obs", [(1, 1), (3, 2)])
def test_the_covariance_adjoint_is_a_congruence_and_never_feeds_the_mean(d, obs):
    """One symmetric Db on a chunk's last row and nothing else: m0_bar is exactly 0 and P0_bar = PhiT Db PhiT^T with the
    PhiT that unit probes on the mean measure."""
    case = adjoint_case(d, obs, 540 + d, True, True, True, n=N_ROWS)
    ops, data, init, zm, zc = _saved(case)
    W = torch.randn(d, d, generator=torch.Generator().manual_seed(3), dtype=F64)
    Db = W + W.T
    for lo, hi in ((0, 4), (4, 8), (8, N_ROWS), (0, N_ROWS)):
        PhiT, _, _, _ = fl.chunk_maps(ops, data, init, zm, zc, None, lo, hi)
        got = fl.run_chunk(ops, data, init, zm, zc, None, lo, hi, (None, Db))
        assert bool((got["m0"] == 0).all())
        assert _err(got["P0"], PhiT @ Db @ PhiT.T) <= 1e-13


def _elements(M, counts, d, seed):
    gen = torch.Generator().manual_seed(seed)
    C = sum(counts)
    r = lambda *shape: torch.randn(*shape, generator=gen, dtype=F64)      # noqa: E731
    PhiT = 0.6 * r(M, C, d, d) / d ** 0.5
    T = r(M, C, d, d, d)
    return PhiT, T + T.transpose(-1, -2), r(M, C, d), fg.sym(r(M, C, d, d))


def _first(counts):
    first = [0]
    for c in counts:
        first.append(first[-1] + c)
    return first


def test_the_scan_against_the_serial_composition():
    M, d, counts = 2, 3, [1, 2, 3, 17]
    el = _elements(M, counts, d, 11)
    first = _first(counts)
    want = fl.serial_compose(*el, first)
    sc = torch.tensor(first)
    for rounds in (None, 4, 7):                        # 4 = ceil(log2(17 - 1)); None: ceil(log2(23 - 1)) = 5
        got = leg._filter_link_scan(*el, sc, rounds)
        for g, w in zip(got, want):
            assert g.shape == w.shape and _err(g, w) <= 1e-13, _err(g, w)
    # the last chunk of every series receives exactly nothing
    got = leg._filter_link_scan(*el, sc)
    for b in range(len(counts)):
        assert bool((got[0][:, first[b + 1] - 1] == 0).all()) and bool((got[1][:, first[b + 1] - 1] == 0).all())
    # a permuted series order gives the permuted result
    perm = [2, 0, 3, 1]
    pieces = lambda t: torch.split(t, counts, dim=1)      # noqa: E731
    pel = [torch.cat([pieces(t)[b] for b in perm], 1) for t in el]
    pgot = leg._filter_link_scan(*pel, torch.tensor(_first([counts[b] for b in perm])))
    for g, p in zip(got, pgot):
        assert _err(p, torch.cat([pieces(g)[b] for b in perm], 1)) <= 1e-13
    # too few rounds cannot pass: the first chunk of the series of 17 receives the composite of 16
    short = leg._filter_link_scan(*el, sc, 3)
    assert _err(short[0], want[0]) > 1e-6


def test_the_scan_keeps_a_failed_series_to_itself():
    """NaN in every element of one series: its own chunks receive NaN (but for the last, which receives nothing), every
    other series' result is that of the healthy run, bit for bit."""
    M, d, counts = 2, 3, [3, 5, 4]
    el = _elements(M, counts, d, 12)
    first = _first(counts)
    sc = torch.tensor(first)
    healthy = leg._filter_link_scan(*el, sc)
    bad = [t.clone() for t in el]
    for t in bad:
        t[1, first[1]:first[2]] = float("nan")
    got = leg._filter_link_scan(*bad, sc)
    for g, h in zip(got, healthy):
        assert torch.equal(g[0], h[0])
        assert torch.equal(g[1, :first[1]], h[1, :first[1]]) and torch.equal(g[1, first[2]:], h[1, first[2]:])
        assert bool(torch.isnan(g[1, first[1]:first[2] - 1]).all())
    empty = leg._filter_link_scan(*(t[:, :0] for t in el), torch.tensor([0, 0]))
    assert tuple(empty[0].shape) == (M, 0, d) and tuple(empty[1].shape) == (M, 0, d, d)


@pytest.mark.parametrize("bad", [0, -1, 2.5, (4, 2), "fast"], ids=repr)
def test_backward_chunk_rows_is_checked_before_anything_runs(bad):
    d, obs = 3, 2
    m, _ = _model(d, obs, 31)
    (ts, xs, _, _), = _series(obs, [6], 32)
    calls = (lambda **kw: leg.filter_predictive(m, ts, xs, **kw),
             lambda **kw: leg.filter_predictive_batch(m, ts, xs, lengths=[2, 4], **kw),
             lambda **kw: leg.filter_predictive_models([m, m], ts, xs, lengths=[2, 4], **kw))
    for call in calls:
        for extra in ({}, {"differentiable": True}, {"chunk_rows": 4}):
            with pytest.raises(ValueError, match="backward_chunk_rows"):
                call(backward_chunk_rows=bad, **extra)


def test_backward_chunk_rows_that_are_accepted():
    assert leg._filter_backward_chunking(None) is None
    assert leg._filter_backward_chunking("auto") == leg.FILTER_BACKWARD_CHUNK_ROWS >= 1
    assert leg._filter_backward_chunking(1) == 1 and leg._filter_backward_chunking(4096) == 4096
    with pytest.raises(ValueError):
        leg._filter_backward_chunking(True)

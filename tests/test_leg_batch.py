"""leg.log_likelihood_batch: many independent LEG series in one call (cgps_leg_loglik_batch for the forward, the
series-aware assembly cgps_peg_precision_seg / cgps_peg_precision_adjoint_seg for the backward) against the
reference's recorded values and gradients, against one leg.log_likelihood per series, and against a CPU
restatement of models.py:301-372 per series (torch assembly + the oracle's mahal_and_det) under autograd."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import _util
from oracle import cr_oracle as O
from cyclic_gps import _hip, leg
import cyclic_gps.cyclic_reduction as cr


def _load(name, device="cuda", dtype=torch.float64):
    g = np.load(os.path.join(_util.GOLDEN, name + ".npz"))
    t = lambda k: torch.from_numpy(g[k]).to(dtype).to(device)   # noqa: E731
    return g, leg.LEGMatrices(t("N"), t("R"), t("B"), t("Lambda")), t("ts"), t("xs")


def _model(d, obs, dtype, seed, device="cuda"):
    gen = torch.Generator().manual_seed(seed)
    N = torch.tril(0.4 * torch.randn(d, d, generator=gen, dtype=torch.float64)) + 0.8 * torch.eye(d, dtype=torch.float64)
    R = torch.tril(0.3 * torch.randn(d, d, generator=gen, dtype=torch.float64), -1)
    B = 0.7 * torch.randn(obs, d, generator=gen, dtype=torch.float64)
    L = torch.tril(0.2 * torch.randn(obs, obs, generator=gen, dtype=torch.float64)) + 0.6 * torch.eye(obs, dtype=torch.float64)
    return leg.LEGMatrices(*(t.to(dtype).to(device) for t in (N, R, B, L))), gen


def _ragged(lengths, obs, gen, dtype, device="cuda", gap0=0.05):
    """Concatenated series; every series starts at its own random time (overlapping, or earlier than the one
    before it), with irregular gaps."""
    ts, xs = [], []
    for n in lengths:
        t0 = 50.0 * torch.rand((), generator=gen, dtype=torch.float64) - 25.0
        gaps = gap0 + 0.5 * torch.rand(n, generator=gen, dtype=torch.float64)
        ts.append(t0 + torch.cumsum(gaps, 0))
        xs.append(torch.randn(n, obs, generator=gen, dtype=torch.float64))
    return torch.cat(ts).to(dtype).to(device), torch.cat(xs).to(dtype).to(device)


def _per_series(m, ts, xs, lengths):
    out, s = [], 0
    for n in lengths:
        out.append(float(leg.log_likelihood(m, ts[s:s + n], xs[s:s + n])))
        s += n
    return out


# ---- argument handling (no GPU) ------------------------------------------------------------------

def test_lengths_are_checked_before_anything_runs():
    ts, xs = torch.zeros(10, dtype=torch.float64), torch.zeros(10, 1, dtype=torch.float64)
    m, _ = _model(2, 1, torch.float64, 0, device="cpu")
    with pytest.raises(ValueError, match="sum"):
        leg.log_likelihood_batch(m, ts, xs, [4, 5])
    with pytest.raises(ValueError, match="sum"):
        leg.log_likelihood_batch(m, ts, xs[:9], [4, 6])
    with pytest.raises(ValueError, match="length 0"):
        leg.log_likelihood_batch(m, ts, xs, [4, 0, 6])
    with pytest.raises(ValueError, match="length 0"):
        leg.log_likelihood_batch(m, torch.zeros(3, 0, dtype=torch.float64), torch.zeros(3, 0, 1, dtype=torch.float64))
    with pytest.raises(ValueError, match="host data"):
        leg.log_likelihood_batch(m, ts, xs, torch.tensor([4.0, 6.0]))
    with pytest.raises(ValueError, match="dense layout"):
        leg.log_likelihood_batch(m, ts, xs)                   # 1-d ts without lengths
    with pytest.raises(ValueError, match="ragged layout"):
        leg.log_likelihood_batch(m, ts.reshape(2, 5), xs.reshape(2, 5, 1), [5, 5])


def test_empty_batch_returns_an_empty_tensor():
    m, _ = _model(3, 1, torch.float64, 0, device="cpu")
    out = leg.log_likelihood_batch(m, torch.zeros(0, dtype=torch.float64), torch.zeros(0, 1, dtype=torch.float64), [])
    assert out.shape == (0,) and out.dtype == torch.float64
    out = leg.log_likelihood_batch(m, torch.zeros(0, 7, dtype=torch.float64), torch.zeros(0, 7, 1, dtype=torch.float64))
    assert out.shape == (0,)
    out = leg.log_likelihood_batch(m, torch.zeros(0, dtype=torch.float64), torch.zeros(0, 1, dtype=torch.float64),
                                   torch.zeros(0, dtype=torch.int64))
    assert out.shape == (0,)


def test_dense_layout_is_the_ragged_layout_of_equal_lengths():
    ts = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    xs = torch.arange(24, dtype=torch.float64).reshape(3, 4, 2)
    t1, x1, l1 = leg._batch_layout(ts, xs, None)
    t2, x2, l2 = leg._batch_layout(ts.reshape(-1), xs.reshape(-1, 2), torch.tensor([4, 4, 4]))
    assert l1 == l2 == [4, 4, 4]
    assert torch.equal(t1, t2) and torch.equal(x1, x2)


def test_plan_marks_the_gaps_between_series():
    p = leg._BatchPlan([3, 1, 2], "cpu")
    assert p.starts == [0, 3, 4, 6] and p.offsets.tolist() == [0, 3, 4, 6]
    assert p.cut.tolist() == [0, 0, 1, 1, 0]                  # gaps 2|3 and 3|4 cross a boundary
    assert p.per_row(torch.tensor([1.0, 2.0, 3.0])).tolist() == [1, 1, 1, 2, 3, 3]
    assert leg._BatchPlan([5], "cpu").cut.tolist() == [0, 0, 0, 0]


def test_c_entries_reject_null_pointers_and_unsupported_sizes():
    lib = _hip.lib()
    assert lib.cgps_leg_loglik_batch(None, None, 2, None, None, None, None, 5, _hip.F64, 4096, None, None, None) == 1
    assert lib.cgps_leg_loglik_batch(None, None, -1, None, None, None, None, 5, _hip.F64, 4096, None, None, None) == 1
    assert lib.cgps_peg_precision_seg(None, None, None, 8, 4, _hip.F64, None, None, None, None) == 1
    assert lib.cgps_peg_precision_adjoint_seg(None, None, None, 8, 4, _hip.F64, None, None, None, None, None) == 1
    assert b"cgps_peg_precision_adjoint_seg" in lib.cgps_last_error()
    # d = 8 and fp64 d = 6 are refused before any launch (the pointers are never touched)
    fake = ctypes.c_void_p(256)
    for d, dt in ((8, _hip.F64), (8, _hip.F32), (6, _hip.F64)):
        assert lib.cgps_leg_loglik_batch(fake, fake, 2, fake, None, None, None, d, dt, 4096, fake, fake, None) == 3
    assert lib.cgps_leg_loglik_batch(fake, fake, 2, fake, None, None, None, 9, _hip.F64, 4096, fake, fake, None) == 3
    assert leg.BATCH_MAX_ROWS >= 1024


# ---- on the GPU ------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_reference_values_small_fixtures_in_one_ragged_batch():
    g1, m, ts1, xs1 = _load("leg_small_regular")
    g2, _, ts2, xs2 = _load("leg_small_irregular")
    out = leg.log_likelihood_batch(m, torch.cat([ts1, ts2, ts1]), torch.cat([xs1, xs2, xs1]),
                                   [ts1.shape[0], ts2.shape[0], ts1.shape[0]])
    assert out.dtype == torch.float64 and out.shape == (3,)
    for got, ref in zip(out.tolist(), (float(g1["ll"]), float(g2["ll"]), float(g1["ll"]))):
        assert abs(got - ref) <= 1e-8 * abs(ref), (got, ref)


@pytest.mark.gpu
def test_reference_values_eight_copies_of_co2like_dense():
    g, m, ts, xs = _load("leg_co2like")
    out = leg.log_likelihood_batch(m, ts.expand(8, -1).contiguous(), xs.expand(8, -1, -1).contiguous())
    ref = float(g["ll"])
    assert out.shape == (8,)
    for got in out.tolist():
        assert abs(got - ref) <= 1e-8 * abs(ref), (got, ref)
    assert abs(float(out.sum()) - 8 * ref) <= 1e-8 * abs(8 * ref)


LENGTHS = [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 502, 511, 512, 513, 1000, 4097]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_against_one_call_per_series_rank5(dtype):
    """Every length boundary of the kernel (one row, rows per lane 1 -> 2 -> ..., a series above BATCH_MAX_ROWS
    handed to the one-series kernel), shuffled so that long and short series are neighbours."""
    m, gen = _model(5, 1, dtype, 7)
    lengths = [LENGTHS[i] for i in torch.randperm(len(LENGTHS), generator=gen).tolist()]
    assert max(lengths) > leg.BATCH_MAX_ROWS
    ts, xs = _ragged(lengths, 1, gen, dtype)
    out = leg.log_likelihood_batch(m, ts, xs, lengths)
    assert out.dtype == dtype
    ref = _per_series(m, ts, xs, lengths)
    rtol = 1e-9 if dtype == torch.float64 else 1e-3
    for n, got, r in zip(lengths, out.tolist(), ref):
        assert abs(got - r) <= rtol * max(1.0, abs(r)), (n, got, r)


@pytest.mark.gpu
@pytest.mark.parametrize("d", range(1, 9))
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_against_one_call_per_series_every_rank(d, dtype):
    """Ranks 1..8 in both dtypes (d = 8 and fp64 d = 6 take the documented per-series path); obs_dim 1 and 2."""
    for obs in (1, 2):
        m, gen = _model(d, obs, dtype, 100 * d + obs)
        lengths = [7, 1, 300, 2, 65, 40]
        # (fp32: gaps of at least 0.5, so that I - E^T E of the random 8 x 8 generators stays well conditioned)
        ts, xs = _ragged(lengths, obs, gen, dtype, gap0=0.05 if dtype == torch.float64 else 0.5)
        out = leg.log_likelihood_batch(m, ts, xs, torch.tensor(lengths))
        ref = _per_series(m, ts, xs, lengths)
        rtol = 1e-9 if dtype == torch.float64 else 1e-3
        for n, got, r in zip(lengths, out.tolist(), ref):
            assert abs(got - r) <= rtol * max(1.0, abs(r)), (d, obs, n, got, r)


@pytest.mark.gpu
def test_gradients_eight_copies_of_co2like():
    g, m, ts, xs = _load("leg_co2like")
    mg = leg.LEGMatrices(*(t.clone().requires_grad_(True) for t in (m.N, m.R, m.B, m.Lambda)))
    out = leg.log_likelihood_batch(mg, ts.expand(8, -1).contiguous(), xs.expand(8, -1, -1).contiguous())
    out.sum().backward()
    assert abs(float(out.detach().sum()) - 8 * float(g["grad_ll"])) <= 1e-8 * abs(8 * float(g["grad_ll"]))
    for got, key in ((mg.N.grad.tril(), "gN"), (mg.R.grad.tril(-1), "gR"), (mg.B.grad, "gB"), (mg.Lambda.grad.tril(), "gLambda")):
        np.testing.assert_allclose(got.cpu().numpy() / 8, g[key], rtol=1e-6, atol=1e-7, err_msg=key)


def _cpu_restatement(m, ts, xs, lengths):
    """models.py:301-372 for each series on CPU tensors: torch assembly + the oracle's reductions."""
    out, s = [], 0
    LLT = m.LLT
    Li = torch.linalg.inv(LLT)
    A = m.B.T @ Li @ m.B
    for n in lengths:
        t, x = ts[s:s + n], xs[s:s + n]
        Rs, Os = leg.peg_precision(t, m.G)
        v = x @ Li @ m.B
        k_m, k_d = O.mahal_and_det(Rs + A, Os, v)
        _, s_d = O.mahal_and_det(Rs, Os, torch.zeros_like(v))
        q = ((x @ Li) * x).sum()
        out.append(-0.5 * ((q - k_m) + (torch.logdet(2 * math.pi * LLT) * n + k_d - s_d)))
        s += n
    return torch.stack(out)


@pytest.mark.gpu
@pytest.mark.parametrize("d,obs,frozen", [(3, 2, False), (5, 1, False), (3, 2, True), (4, 1, True)],
                         ids=["d3o2", "d5o1", "d3o2_NR_frozen", "d4o1_NR_frozen"])
def test_gradients_against_cpu_restatement(d, obs, frozen):
    """A random upstream vector g[B]; gradients in N, R, B, Lambda, xs and ts -- or, with N and R frozen, in B,
    Lambda, xs and ts only (the single-series fused path drops those; the batched one must not)."""
    m, gen = _model(d, obs, torch.float64, 31 * d + obs, device="cpu")
    lengths = [1, 5, 17, 64, 3, 40]
    ts, xs = _ragged(lengths, obs, gen, torch.float64, device="cpu")
    w = torch.randn(len(lengths), generator=gen, dtype=torch.float64)
    train = (False, False, True, True) if frozen else (True, True, True, True)

    def run(device):
        mm = leg.LEGMatrices(*(t.detach().clone().to(device).requires_grad_(r)
                               for t, r in zip((m.N, m.R, m.B, m.Lambda), train)))
        t = ts.detach().clone().to(device).requires_grad_(True)
        x = xs.detach().clone().to(device).requires_grad_(True)
        ll = leg.log_likelihood_batch(mm, t, x, lengths) if device == "cuda" else _cpu_restatement(mm, t, x, lengths)
        (ll * w.to(device)).sum().backward()
        grads = [p.grad for p, r in zip((mm.N, mm.R, mm.B, mm.Lambda), train) if r] + [x.grad, t.grad]
        return ll.detach().cpu(), [gr.cpu() for gr in grads]

    ll_gpu, g_gpu = run("cuda")
    ll_cpu, g_cpu = run("cpu")
    np.testing.assert_allclose(ll_gpu.numpy(), ll_cpu.numpy(), rtol=1e-9)
    names = [k for k, r in zip(("N", "R", "B", "Lambda"), train) if r] + ["xs", "ts"]
    for name, a, b in zip(names, g_gpu, g_cpu):
        assert a is not None and b is not None, name
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-7, atol=1e-9, err_msg=name)


@pytest.mark.gpu
def test_bit_identical_repeats_and_independent_of_neighbours():
    m, gen = _model(5, 1, torch.float64, 3)
    lengths = [502, 33, 1, 700, 129]
    ts, xs = _ragged(lengths, 1, gen, torch.float64)
    a = leg.log_likelihood_batch(m, ts, xs, lengths)
    b = leg.log_likelihood_batch(m, ts, xs, lengths)
    assert torch.equal(a, b)
    # the same series reversed in order, with a different neighbour in front: every value the same
    starts = [0]
    for n in lengths:
        starts.append(starts[-1] + n)
    order = list(reversed(range(len(lengths))))
    ts2 = torch.cat([ts[:50]] + [ts[starts[i]:starts[i + 1]] for i in order])
    xs2 = torch.cat([xs[:50] * 3.0] + [xs[starts[i]:starts[i + 1]] for i in order])
    c = leg.log_likelihood_batch(m, ts2, xs2, [50] + [lengths[i] for i in order])
    for k, i in enumerate(order):
        assert abs(float(c[k + 1]) - float(a[i])) <= 1e-12 * abs(float(a[i])), (i, float(c[k + 1]), float(a[i]))


@pytest.mark.gpu
def test_repeated_time_stamp_names_its_series():
    m, gen = _model(3, 1, torch.float64, 5)
    lengths = [40, 300, 25, 60]
    ts, xs = _ragged(lengths, 1, gen, torch.float64)
    clean = leg.log_likelihood_batch(m, ts, xs, lengths)
    bad = ts.clone()
    bad[40 + 300 + 11] = bad[40 + 300 + 10]                  # series 2, local rows 10 / 11
    with pytest.raises(cr.NotPSDError, match="series 2"):
        leg.log_likelihood_batch(m, bad, xs, lengths)
    prev = cr.CHECK_POSITIVE_DEFINITE
    cr.CHECK_POSITIVE_DEFINITE = False
    try:
        out = leg.log_likelihood_batch(m, bad, xs, lengths)
    finally:
        cr.CHECK_POSITIVE_DEFINITE = prev
    assert math.isnan(float(out[2]))
    for b in (0, 1, 3):
        assert float(out[b]) == float(clean[b])

"""leg.log_likelihood_batch(..., noise_var=s): many LEG series with per-observation noise variances in one launch
(cgps_leg_loglik_batch_w, leg_batch_kernel<.., LEG_ROWS_WEIGHTED>) against the one-series weighted-basis kernel
(cgps_leg_mahal_logdet_pair_w), against the one-block batched kernel under equal weights, against one
leg.log_likelihood(noise_var=) per series and against the dense Gaussian of the observed entries with diag(s)
(tests/_noiseref.py) under autograd; offsets, independence of neighbours, errors and graph replay."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import _noiseref as nr
import _util
from cyclic_gps import _hip, leg
import cyclic_gps.cyclic_reduction as cr

F64, F32 = torch.float64, torch.float32


# ---- recipes of tests/test_leg_batch_missing.py and tests/test_leg_noise.py (copied, not imported) ------------------
def _load(name="leg_co2like", device="cuda", dtype=F64):
    g = np.load(os.path.join(_util.GOLDEN, name + ".npz"))
    t = lambda k: torch.from_numpy(g[k]).to(dtype).to(device)   # noqa: E731
    return g, leg.LEGMatrices(t("N"), t("R"), t("B"), t("Lambda")), t("ts"), t("xs")


def _model(d, obs, dtype, seed, device="cuda"):
    gen = torch.Generator().manual_seed(seed)
    N = torch.tril(0.4 * torch.randn(d, d, generator=gen, dtype=F64)) + 0.8 * torch.eye(d, dtype=F64)
    R = torch.tril(0.3 * torch.randn(d, d, generator=gen, dtype=F64), -1)
    B = 0.7 * torch.randn(obs, d, generator=gen, dtype=F64)
    L = torch.tril(0.2 * torch.randn(obs, obs, generator=gen, dtype=F64)) + 0.6 * torch.eye(obs, dtype=F64)
    return leg.LEGMatrices(*(t.to(dtype).to(device) for t in (N, R, B, L))), gen


def _ragged(lengths, obs, gen, dtype, device="cuda", gap0=0.05):
    ts, xs = [], []
    for n in lengths:
        t0 = 50.0 * torch.rand((), generator=gen, dtype=F64) - 25.0
        gaps = gap0 + 0.5 * torch.rand(n, generator=gen, dtype=F64)
        ts.append(t0 + torch.cumsum(gaps, 0))
        xs.append(torch.randn(n, obs, generator=gen, dtype=F64))
    return torch.cat(ts).to(dtype).to(device), torch.cat(xs).to(dtype).to(device)


def _kernel_model(d, dtype, seed, Kb):
    """test_leg_noise._kernel_model: the diagonal of N from [0.8, 1.2], so that the symmetric part of G is not nearly
    singular; basis blocks symmetric positive semi-definite of rank 2, as B^T Li B is (non-negative weights keep K
    positive definite)."""
    gen = torch.Generator().manual_seed(seed)
    Nm = torch.tril(0.4 * torch.randn(d, d, generator=gen, dtype=F64), -1)
    Nm = Nm + torch.diag(0.8 + 0.4 * torch.rand(d, generator=gen, dtype=F64))
    Rm = torch.tril(0.3 * torch.randn(d, d, generator=gen, dtype=F64), -1)
    G = Nm @ Nm.T + Rm - Rm.T + 1e-5 * torch.eye(d, dtype=F64)
    Bs = torch.randn(Kb, d, 2, generator=gen, dtype=F64)
    basis = 0.5 * Bs @ Bs.transpose(-1, -2)
    return G.to(dtype).cuda(), basis.to(dtype).cuda(), gen


def _starts(lengths):
    s = [0]
    for n in lengths:
        s.append(s[-1] + n)
    return s


def _close(got, want, rtol):
    return abs(got - want) <= rtol * max(1.0, abs(want))


def _rel(got, want):
    return abs(got - want) / max(1.0, abs(want))


# ---- argument handling (no GPU) -------------------------------------------------------------------------------------
def test_c_entry_is_exported_and_checks_its_arguments_before_any_launch():
    assert "cgps_leg_loglik_batch_w" in _hip.exported_symbols()
    lib = _hip.lib()
    fn = lib.cgps_leg_loglik_batch_w
    assert lib.cgps_version() == 320
    fake = ctypes.c_void_p(256)
    call = lambda B, bs, Kb, wt, d=5, dt=_hip.F64: fn(fake, fake, B, fake, bs, Kb, wt, None, None, d, dt, 4096,   # noqa: E731
                                                      fake, fake, None)
    for rc in (call(2, fake, 0, fake), call(2, fake, 65, fake), call(2, fake, -1, fake)):
        assert rc == 1 and b"cgps_leg_loglik_batch_w" in lib.cgps_last_error()
    for rc in (call(2, None, 3, fake), call(2, fake, 3, None), call(-1, fake, 3, fake), call(2 ** 31, fake, 3, fake)):
        assert rc == 1 and b"cgps_leg_loglik_batch_w" in lib.cgps_last_error()
    # every other pointer, one at a time (v and q may be null: zeros)
    for k in (0, 1, 3, 12, 13):
        args = [fake, fake, 2, fake, fake, 3, fake, None, None, 5, _hip.F64, 4096, fake, fake, None]
        args[k] = None
        assert fn(*args) == 1 and b"cgps_leg_loglik_batch_w" in lib.cgps_last_error(), k
    # d = 8 and fp64 d = 6 are refused before any launch (the pointers are never touched)
    for d, dt in ((8, _hip.F64), (8, _hip.F32), (6, _hip.F64)):
        assert call(2, fake, 3, fake, d, dt) == 3 and b"cgps_leg_loglik_batch_w" in lib.cgps_last_error()
    assert call(2, fake, 3, fake, 9, _hip.F64) == 3             # (refused by the dispatcher of every entry)
    # an empty batch is no work and no error, whatever the pointers
    assert fn(None, None, 0, None, None, 3, None, None, None, 5, _hip.F64, 4096, None, None, None) == 0
    assert call(0, fake, 64, fake, 7, _hip.F32) == 0


def test_noise_var_is_checked_before_anything_runs_dense_layout():
    m, _ = _model(2, 2, F64, 0, device="cpu")
    ts, xs = torch.zeros(3, 4, dtype=F64), torch.zeros(3, 4, 2, dtype=F64)
    for bad in (torch.ones(3, 4, 2, dtype=torch.int64), torch.ones(3, 4, dtype=torch.bool), [[0.5] * 4] * 3, 0.5):
        with pytest.raises(ValueError, match="floating"):
            leg.log_likelihood_batch(m, ts, xs, noise_var=bad)
    # wrong rank, wrong row count, wrong channel count
    for shape in ((3,), (12,), (12, 2), (3, 4, 2, 1), (3, 4, 1), (3, 4, 3), (3, 5), (3, 5, 2), (4, 4), (2, 4, 2)):
        with pytest.raises(ValueError, match="noise_var"):
            leg.log_likelihood_batch(m, ts, xs, noise_var=torch.ones(shape, dtype=F64))
        with pytest.raises(ValueError, match="noise_var"):
            leg.log_likelihood_batch(m, ts, xs, observed=torch.ones(3, 4, dtype=torch.bool),
                                     noise_var=torch.ones(shape, dtype=F64))
    with pytest.raises(ValueError, match="dense layout"):      # the layout's own errors come first, as without noise
        leg.log_likelihood_batch(m, ts.reshape(-1), xs.reshape(-1, 2), noise_var=torch.ones(12, dtype=F64))


def test_noise_var_is_checked_before_anything_runs_ragged_layout():
    m, _ = _model(2, 2, F64, 0, device="cpu")
    ts, xs = torch.zeros(10, dtype=F64), torch.zeros(10, 2, dtype=F64)
    for bad in (torch.ones(10, 2, dtype=torch.int32), torch.ones(10, dtype=torch.int64), [0.5] * 10):
        with pytest.raises(ValueError, match="floating"):
            leg.log_likelihood_batch(m, ts, xs, [4, 6], noise_var=bad)
    for shape in ((), (9,), (11,), (9, 2), (10, 1), (10, 3), (10, 2, 1), (2, 5), (2, 5, 2)):
        with pytest.raises(ValueError, match="noise_var"):
            leg.log_likelihood_batch(m, ts, xs, [4, 6], noise_var=torch.ones(shape, dtype=F64))
    with pytest.raises(ValueError, match="sum"):
        leg.log_likelihood_batch(m, ts, xs, [4, 5], noise_var=torch.ones(10, dtype=F64))


def test_empty_batch_with_noise_var_returns_an_empty_tensor():
    m, _ = _model(3, 1, F64, 0, device="cpu")
    e = torch.zeros(0, dtype=F64)
    for s in (torch.zeros(0, dtype=F64), torch.zeros(0, 1, dtype=F64)):
        out = leg.log_likelihood_batch(m, e, torch.zeros(0, 1, dtype=F64), [], noise_var=s)
        assert out.shape == (0,) and out.dtype == F64
        out = leg.log_likelihood_batch(m, e, torch.zeros(0, 1, dtype=F64), [], observed=torch.zeros(0, dtype=torch.bool),
                                       noise_var=s)
        assert out.shape == (0,)
    for s in (torch.zeros(0, 7, dtype=F64), torch.zeros(0, 7, 1, dtype=F64)):
        out = leg.log_likelihood_batch(m, torch.zeros(0, 7, dtype=F64), torch.zeros(0, 7, 1, dtype=F64), noise_var=s)
        assert out.shape == (0,)


@pytest.mark.gpu
def test_cpu_tensors_take_one_call_per_series():
    """(host tensors are staged to the device by the library: there is no CPU kernel)"""
    m, gen = _model(3, 2, F64, 1, device="cpu")
    lengths = [5, 1, 9]
    st = _starts(lengths)
    ts, xs = _ragged(lengths, 2, gen, F64, device="cpu")
    s = 2.0 * torch.rand(st[-1], 2, generator=gen, dtype=F64)
    obs = torch.rand(st[-1], 2, generator=gen) < 0.6
    for ob in (None, obs):
        out = leg.log_likelihood_batch(m, ts, xs, lengths, observed=ob, noise_var=s)
        for b, (a, e) in enumerate(zip(st[:-1], st[1:])):
            want = float(leg.log_likelihood(m, ts[a:e], xs[a:e], None if ob is None else ob[a:e], s[a:e]))
            assert float(out[b]) == want, (b, float(out[b]), want)


# ---- the kernel -----------------------------------------------------------------------------------------------------
KERNEL_LENGTHS = [1, 2, 3, 255, 256, 257, 513, 129, 128]
KERNEL_KB = (1, 3, 36)
KERNEL_CASES = [(1, F64), (2, F64), (3, F64), (4, F64), (5, F64), (7, F64), (2, F32), (4, F32), (5, F32), (6, F32), (7, F32)]


def _batch_weightings(lengths, Kb, dtype, gen):
    """name -> weights [R, Kb]: random in [0, 2]; all zero (K is the prior precision); all equal; and random with runs of
    all-zero rows laid across every series boundary and across local rows 127/128 and 255/256 of the longer series (the
    lane-chunk boundaries of 128 and 256 lanes at one, two and three rows per lane fall inside those runs or at the
    series' ends)."""
    st = _starts(lengths)
    R = st[-1]
    out = {"random": 2.0 * torch.rand(R, Kb, generator=gen, dtype=F64), "zero": torch.zeros(R, Kb, dtype=F64),
           "equal": torch.full((R, Kb), 0.7, dtype=F64)}
    runs = 2.0 * torch.rand(R, Kb, generator=gen, dtype=F64)
    for s, n in zip(st[:-1], lengths):
        runs[max(0, s - 3):s + 2] = 0
        for k in (128, 256):
            if n > k:
                runs[s + k - 7:min(s + k + 9, s + n)] = 0
    runs[R - 3:] = 0
    out["runs"] = runs
    return {name: w.to(dtype).cuda() for name, w in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("d,dtype", KERNEL_CASES, ids=lambda p: str(p).replace("torch.", ""))
def test_batch_weighted_kernel_against_the_one_series_kernel(d, dtype):
    """One row, both sides of one row per lane against two (and, at 7 x 7 fp64 with its 128 lanes, of two against
    three), long and short series as neighbours; 1, 3 and 36 basis blocks; the prior log-det is cgps_leg_loglik_batch's
    bit for bit.  Tolerances of test_batch_pattern_kernel_against_the_one_series_kernel."""
    rtol = 1e-9 if dtype == F64 else 3e-4
    worst = {"mahal": 0.0, "logdet": 0.0, "prior": 0.0, "q": 0.0}
    failures = []
    for Kb in KERNEL_KB:
        G, basis, gen = _kernel_model(d, dtype, 700 + 10 * d + Kb, Kb)
        lengths = [KERNEL_LENGTHS[i] for i in torch.randperm(len(KERNEL_LENGTHS), generator=gen).tolist()]
        st = _starts(lengths)
        plan = leg._BatchPlan(lengths, "cuda")
        ts, _ = _ragged(lengths, 1, gen, dtype)
        v = torch.randn(st[-1], d, generator=gen, dtype=F64).to(dtype).cuda()
        q = torch.randn(st[-1], generator=gen, dtype=F64).to(dtype).cuda()
        prior = leg.leg_loglik_batch_reductions(ts, G, basis[0].contiguous(), v, q, plan)[0][:, 2].clone()
        qs = torch.stack([q[s:e].double().sum() for s, e in zip(st[:-1], st[1:])]).cpu()
        for name, w in _batch_weightings(lengths, Kb, dtype, gen).items():
            out, info = leg.leg_loglik_batch_reductions_w(ts, G, basis, w, v, q, plan)
            assert out.dtype == F64 and out.shape == (len(lengths), 4)
            assert info.dtype == torch.int32 and info.shape == (len(lengths), 2)
            assert int(info.abs().max()) == 0, (Kb, name, info.tolist())
            assert torch.equal(out[:, 2], prior), (Kb, name, out[:, 2].tolist(), prior.tolist())
            ref = torch.stack([torch.stack(leg.leg_loglik_reductions_w(ts[s:e], G, basis, w[s:e].contiguous(), v[s:e])).double()
                               for s, e in zip(st[:-1], st[1:])]).cpu()
            got = out.cpu()
            for b, n in enumerate(lengths):
                what = (Kb, name, b, n)
                m1, l1, s1, q1 = got[b].tolist()
                m0, l0, s0 = ref[b].tolist()
                for key, a, r in (("mahal", m1, m0), ("logdet", l1, l0), ("prior", s1, s0), ("q", q1, float(qs[b]))):
                    worst[key] = max(worst[key], _rel(a, r))
                if not (_close(l1, l0, rtol) and _close(m1, m0, 10 * rtol) and _close(s1, s0, rtol)
                        and _close(q1, float(qs[b]), 1e-12)):
                    failures.append((what, got[b].tolist(), ref[b].tolist(), float(qs[b])))
    print("batch_w kernel d=%d %s: worst mahal %.3e logdet %.3e prior %.3e sum q %.3e" % (
        d, str(dtype).replace("torch.", ""), worst["mahal"], worst["logdet"], worst["prior"], worst["q"]))
    assert not failures, failures[:5]
    assert worst["logdet"] <= rtol and worst["prior"] <= rtol and worst["mahal"] <= 10 * rtol and worst["q"] <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 4, 5, 7])
def test_equal_weights_are_the_one_block_batched_kernel(d):
    """w sum_k basis[k] as the one A of cgps_leg_loglik_batch: the same systems, added up in another order."""
    worst = 0.0
    for Kb in KERNEL_KB:
        G, basis, gen = _kernel_model(d, F64, 77 + d + Kb, Kb)
        lengths = KERNEL_LENGTHS
        plan = leg._BatchPlan(lengths, "cuda")
        ts, _ = _ragged(lengths, 1, gen, F64)
        R = sum(lengths)
        v = torch.randn(R, d, generator=gen, dtype=F64).cuda()
        q = torch.randn(R, generator=gen, dtype=F64).cuda()
        want, _ = leg.leg_loglik_batch_reductions(ts, G, (0.7 * basis.sum(0)).contiguous(), v, q, plan)
        got, info = leg.leg_loglik_batch_reductions_w(ts, G, basis, torch.full((R, Kb), 0.7, dtype=F64, device="cuda"), v, q, plan)
        assert int(info.abs().max()) == 0
        assert torch.equal(got[:, 2:], want[:, 2:])                     # the prior log-det and the sum of q: the same code
        err = float(((got - want).abs() / want.abs().clamp_min(1.0)).max())
        worst = max(worst, err)
        print("equal weights d=%d Kb=%d: worst %.3e" % (d, Kb, err))
    assert worst <= 1e-9, worst


@pytest.mark.gpu
def test_a_series_above_batch_max_rows_takes_the_one_series_kernel_and_lands_in_its_slot():
    d, Kb = 3, 3
    G, basis, gen = _kernel_model(d, F64, 41, Kb)
    lengths = [40, leg.BATCH_MAX_ROWS + 1, 7]
    st = _starts(lengths)
    plan = leg._BatchPlan(lengths, "cuda")
    assert plan.long == [1]
    ts, _ = _ragged(lengths, 1, gen, F64)
    v = torch.randn(st[-1], d, generator=gen, dtype=F64).cuda()
    q = torch.randn(st[-1], generator=gen, dtype=F64).cuda()
    w = (2.0 * torch.rand(st[-1], Kb, generator=gen, dtype=F64)).cuda()
    out, info = leg.leg_loglik_batch_reductions_w(ts, G, basis, w, v, q, plan)
    assert int(info.abs().max()) == 0
    for b, (s, e) in enumerate(zip(st[:-1], st[1:])):
        m0, l0, s0 = (float(x) for x in leg.leg_loglik_reductions_w(ts[s:e], G, basis, w[s:e].contiguous(), v[s:e]))
        m1, l1, s1, q1 = out[b].tolist()
        assert _close(l1, l0, 1e-9) and _close(s1, s0, 1e-9) and _close(m1, m0, 1e-8), (b, out[b].tolist(), (m0, l0, s0))
        assert _close(q1, float(q[s:e].sum()), 1e-12)
    # and through the public entry
    m, gen = _model(3, 2, F64, 43)
    ts, xs = _ragged(lengths, 2, gen, F64)
    s = (2.0 * torch.rand(st[-1], 2, generator=gen, dtype=F64)).cuda()
    obs = (torch.rand(st[-1], 2, generator=gen) < 0.6).cuda()
    for ob in (None, obs):
        got = leg.log_likelihood_batch(m, ts, xs, lengths, observed=ob, noise_var=s)
        for b, (a, e) in enumerate(zip(st[:-1], st[1:])):
            want = float(leg.log_likelihood(m, ts[a:e], xs[a:e], None if ob is None else ob[a:e], s[a:e]))
            assert _close(float(got[b]), want, 1e-9), (b, float(got[b]), want)


def test_wrapper_refuses_wrong_operands_before_any_launch():
    """(no device is needed to be refused: every check comes before the library is touched)"""
    plan = leg._BatchPlan([4, 6], "cpu")
    G = torch.eye(3, dtype=F64)
    ts, v, q = torch.arange(10, dtype=F64), torch.zeros(10, 3, dtype=F64), torch.zeros(10, dtype=F64)
    basis, w = torch.ones(2, 3, 3, dtype=F64), torch.ones(10, 2, dtype=F64)
    for bs, wt in ((basis[0], w), (torch.ones(2, 3, 2, dtype=F64), w), (torch.ones(0, 3, 3, dtype=F64), w[:, :0]),
                   (torch.ones(65, 3, 3, dtype=F64), torch.ones(10, 65, dtype=F64)), (basis, w[:9]), (basis, w[:, :1]),
                   (basis, torch.ones(10, dtype=F64)), (basis.float(), w), (basis, w.float()), (basis, w)):
        with pytest.raises(ValueError):                          # (the last pair: host tensors)
            leg.leg_loglik_batch_reductions_w(ts, G, bs, wt, v, q, plan)


@pytest.mark.gpu
def test_bit_identical_repeats_own_noise_per_series_and_independent_of_neighbours():
    """Every series has its own variances, so a kernel that indexed the weights by the local row alone (without the
    series' offset) would give every series but the first another series' noise."""
    m, gen = _model(5, 2, F64, 3)
    lengths = [502, 33, 1, 700, 129]
    st = _starts(lengths)
    ts, xs = _ragged(lengths, 2, gen, F64)
    s = (2.0 * torch.rand(st[-1], 2, generator=gen, dtype=F64)).cuda()
    a = leg.log_likelihood_batch(m, ts, xs, lengths, noise_var=s)
    b = leg.log_likelihood_batch(m, ts, xs, lengths, noise_var=s)
    assert torch.equal(a, b)
    for i, (lo, hi) in enumerate(zip(st[:-1], st[1:])):
        want = float(leg.log_likelihood(m, ts[lo:hi], xs[lo:hi], noise_var=s[lo:hi]))
        assert _close(float(a[i]), want, 1e-9), (i, float(a[i]), want)
    # reversed in order, behind a new neighbour with noise and data of its own: every value the same
    order = list(reversed(range(len(lengths))))
    cat = lambda t, head: torch.cat([head] + [t[st[i]:st[i + 1]] for i in order])   # noqa: E731
    c = leg.log_likelihood_batch(m, cat(ts, ts[:50]), cat(xs, xs[:50] * 3.0), [50] + [lengths[i] for i in order],
                                 noise_var=cat(s, 5.0 - s[:50]))
    for k, i in enumerate(order):
        assert abs(float(c[k + 1]) - float(a[i])) <= 1e-12 * abs(float(a[i])), (i, float(c[k + 1]), float(a[i]))
    # a neighbour's noise and data change in place: the others do not move at all
    s2, xs2 = s.clone(), xs.clone()
    s2[st[1]:st[2]] = 3.0 - s2[st[1]:st[2]]
    xs2[st[1]:st[2]] *= -2.0
    e = leg.log_likelihood_batch(m, ts, xs2, lengths, noise_var=s2)
    assert float(e[1]) != float(a[1])
    for i in (0, 2, 3, 4):
        assert abs(float(e[i]) - float(a[i])) <= 1e-12 * abs(float(a[i])), (i, float(e[i]), float(a[i]))


# ---- the public entry -----------------------------------------------------------------------------------------------
PUBLIC_LENGTHS = [7, 1, 300, 2, 65, 40]
UNOBSERVED, FULL = 4, 5                                         # the series of 65 rows sees nothing, that of 40 everything


def _public_model(d, obs_dim, dtype):
    """test_leg_batch_missing._public_model: ``_model`` under the first seed of 100 d + obs_dim, + 1000, + 2000, ...
    whose N N^T (the symmetric part of G) has no eigenvalue below 1e-2.  The criterion looks at the model alone, never
    at a result."""
    seed = 100 * d + obs_dim
    while True:
        m, gen = _model(d, obs_dim, dtype, seed)
        N = m.N.double().cpu()
        if float(torch.linalg.eigvalsh(N @ N.T).min()) >= 1e-2:
            return m, gen
        seed += 1000


def _per_series(m, ts, xs, obs, s, lengths):
    st = _starts(lengths)
    return [float(leg.log_likelihood(m, ts[a:e], xs[a:e], None if obs is None else obs[a:e], s[a:e]))
            for a, e in zip(st[:-1], st[1:])]


@pytest.mark.gpu
@pytest.mark.parametrize("d", range(1, 9))
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_against_one_noisy_call_per_series_every_rank(d, dtype):
    """Ranks 1..8 in both dtypes (d = 8 and fp64 d = 6 take the per-series path), obs_dim 1 and 2, variances uniform in
    [0, 2], without a mask and with one that keeps ~60 % of the entries.  fp32 is compared with the fp64 per-series value
    of the same (fp32-rounded) inputs; the existing fp32 ``log_likelihood(noise_var=)`` must itself be within a quarter
    of that tolerance on these inputs."""
    rtol = 1e-9 if dtype == F64 else 1e-3
    lengths = PUBLIC_LENGTHS
    st = _starts(lengths)
    nan = torch.full((), float("nan"), dtype=dtype, device="cuda")
    for obs_dim in (1, 2):
        m, gen = _public_model(d, obs_dim, dtype)
        m64 = leg.LEGMatrices(*(t.double() for t in (m.N, m.R, m.B, m.Lambda)))
        # (fp32: gaps of at least 0.5, so that I - E^T E of the random 8 x 8 generators stays well conditioned)
        ts, xs = _ragged(lengths, obs_dim, gen, dtype, gap0=0.05 if dtype == F64 else 0.5)
        s = (2.0 * torch.rand(st[-1], obs_dim, generator=gen, dtype=F64)).to(dtype).cuda()
        mask = (torch.rand(st[-1], obs_dim, generator=gen) < 0.6).cuda()
        mask[st[UNOBSERVED]:st[UNOBSERVED + 1]] = False
        mask[st[FULL]:st[FULL + 1]] = True
        for obs in (None, mask):
            tag = "d=%d obs=%d %s %s" % (d, obs_dim, str(dtype).replace("torch.", ""), "plain" if obs is None else "masked")
            out = leg.log_likelihood_batch(m, ts, xs, torch.tensor(lengths), observed=obs, noise_var=s)
            assert out.dtype == dtype and out.shape == (len(lengths),)
            if dtype == F64:
                ref = _per_series(m, ts, xs, obs, s, lengths)
            else:
                ref = _per_series(m64, ts.double(), xs.double(), obs, s.double(), lengths)
                single = _per_series(m, ts, xs, obs, s, lengths)
                worst = max(_rel(a, r) for a, r in zip(single, ref))
                print("public %s: existing one-series call against fp64, worst %.3e" % (tag, worst))
                assert worst <= 0.25 * rtol, (tag, single, ref)
            got = out.tolist()
            print("public %s: batched call against the reference, worst %.3e" % (tag, max(_rel(a, r) for a, r in zip(got, ref))))
            for n, a, r in zip(lengths, got, ref):
                assert _close(a, r, rtol), (tag, n, a, r)
            if obs_dim == 1:                                    # one variance per row is the same noise
                assert torch.equal(leg.log_likelihood_batch(m, ts, xs, lengths, observed=obs, noise_var=s[:, 0]), out)
            if obs is not None:
                assert abs(got[UNOBSERVED]) <= 1e-9, got[UNOBSERVED]
                a, e = st[FULL], st[FULL + 1]
                full = float(leg.log_likelihood_batch(m, ts[a:e], xs[a:e], [lengths[FULL]], noise_var=s[a:e])[0])
                assert _close(got[FULL], full, rtol), (got[FULL], full)
                # whatever the unobserved entries of the data and of the variances hold
                holed_x, holed_s = torch.where(obs, xs, nan), torch.where(obs, s, nan)
                assert torch.equal(leg.log_likelihood_batch(m, ts, holed_x, lengths, observed=obs, noise_var=holed_s), out)
                if obs_dim == 1:
                    assert torch.equal(leg.log_likelihood_batch(m, ts, xs, lengths, observed=obs[:, 0], noise_var=s), out)
            # the dense layout with padded tails (time stamps go on increasing, data and variances NaN, nothing observed)
            nmax = max(lengths)
            tsd = torch.empty(len(lengths), nmax, dtype=dtype, device="cuda")
            xsd = torch.full((len(lengths), nmax, obs_dim), float("nan"), dtype=dtype, device="cuda")
            sd = torch.full((len(lengths), nmax, obs_dim), float("nan"), dtype=dtype, device="cuda")
            obd = torch.zeros(len(lengths), nmax, obs_dim, dtype=torch.bool, device="cuda")
            for b, n in enumerate(lengths):
                tsd[b, :n], xsd[b, :n], sd[b, :n] = ts[st[b]:st[b + 1]], xs[st[b]:st[b + 1]], s[st[b]:st[b + 1]]
                obd[b, :n] = True if obs is None else obs[st[b]:st[b + 1]]
                tsd[b, n:] = ts[st[b + 1] - 1] + torch.arange(1, nmax - n + 1, dtype=dtype, device="cuda")
            dense = leg.log_likelihood_batch(m, tsd, xsd, observed=obd, noise_var=sd).tolist()
            for n, a, r in zip(lengths, dense, got):
                assert _close(a, r, rtol), ("padded", tag, n, a, r)
            if dtype == F64:                                    # no extra noise: the calls without the argument
                zero = torch.zeros_like(s)
                z = leg.log_likelihood_batch(m, ts, xs, lengths, observed=obs, noise_var=zero).tolist()
                want = leg.log_likelihood_batch(m, ts, xs, lengths, observed=obs).tolist()
                for n, a, r in zip(lengths, z, want):
                    assert _close(a, r, 1e-9), ("zero variance", tag, n, a, r)


# ---- gradients --------------------------------------------------------------------------------------------------------
LEG_PARAMS = ("N", "R", "B", "Lambda", "xs", "ts", "noise_var")
DENSE_CASES = {(3, 3, 37): (11, 111, 211), (5, 2, 64): (12, 112, 212)}
_dense = {}


def _dense_batch_ref(d, obs, n):
    """Three series (the data, times, variances and mask of three seeds of _noiseref.leg_case under the model of the
    first), a random upstream weight per series, and the weighted sums of the dense reference's value and gradients."""
    key = (d, obs, n)
    if key not in _dense:
        seeds = DENSE_CASES[key]
        cases = [nr.leg_case(d, obs, n, sd) for sd in seeds]
        model = cases[0][0][:4]
        w = torch.randn(len(seeds), generator=torch.Generator().manual_seed(seeds[0]), dtype=F64)
        lls, gsum, gxs, gts, gs = [], [torch.zeros_like(t) for t in model], [], [], []
        for wb, (case, mask) in zip(w.tolist(), cases):
            ll, grads = nr.leg_dense_value_and_grads(*model, case[5], case[4], case[6], mask)
            lls.append(ll)
            for acc, gpar in zip(gsum, grads[:4]):
                acc += wb * gpar
            gxs.append(wb * grads[4])
            gts.append(wb * grads[5])
            gs.append(wb * grads[6])
        xs = torch.stack([c[0][4] for c in cases])
        ts = torch.stack([c[0][5] for c in cases])
        s = torch.stack([c[0][6] for c in cases])
        mask = torch.stack([c[1] for c in cases])
        _dense[key] = model, xs, ts, s, mask, w, torch.stack(lls), gsum + [torch.stack(gxs), torch.stack(gts), torch.stack(gs)]
    return _dense[key]


def _check_grad(got, want, what):
    """test_leg_missing._check_grad, fp64"""
    want = want.detach().to("cpu", F64)
    assert got is not None, what + " is missing"
    got = got.detach().to("cpu", F64)
    scale = float(want.abs().max())
    print("%s: worst error %.3e of the largest entry" % (what, float((got - want).abs().max()) / max(scale, 1e-300)))
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-7, atol=1e-10 * scale, err_msg=what)


@pytest.mark.gpu
@pytest.mark.parametrize("frozen", [False, True], ids=["all", "NR_frozen"])
@pytest.mark.parametrize("d,obs,n", list(DENSE_CASES))
def test_gradients_against_the_dense_reference(d, obs, n, frozen):
    model, xs, ts, s, mask, w, lls, grads = _dense_batch_ref(d, obs, n)
    nan_xs = torch.where(mask, xs, torch.full_like(xs, float("nan")))
    nan_s = torch.where(mask, s, torch.full_like(s, float("nan")))
    train = [not (frozen and name in ("N", "R")) for name in LEG_PARAMS]
    p = [t.clone().cuda().requires_grad_(r) for t, r in zip(list(model) + [nan_xs, ts, nan_s], train)]
    out = leg.log_likelihood_batch(leg.LEGMatrices(*p[:4]), p[5], p[4], observed=mask.cuda(), noise_var=p[6])
    for b in range(len(lls)):
        print("dense d=%d obs=%d series %d: value error %.3e" % (d, obs, b, _rel(float(out[b].detach()), float(lls[b]))))
        assert _close(float(out[b].detach()), float(lls[b]), 1e-9), (b, float(out[b].detach()), float(lls[b]))
    (out * w.cuda()).sum().backward()
    for name, leaf, want, r in zip(LEG_PARAMS, p, grads, train):
        if r:
            _check_grad(leaf.grad, want, "d=%d obs=%d d ll / d %s" % (d, obs, name))
        else:
            assert leaf.grad is None, name
    assert float(p[4].grad[~mask.cuda()].abs().max()) == 0.0
    assert float(p[6].grad[~mask.cuda()].abs().max()) == 0.0


def test_rows_product_is_the_plain_product_on_both_sides_of_a_chunk():
    """The basis gradient's tall product, chunked: no rows, fewer than one chunk, whole chunks, chunks and a remainder.
    Exact in integers (every partial sum is an integer below 2^53)."""
    gen = torch.Generator().manual_seed(0)
    for R in (0, 1, 7, 8, 9, 16, 37):
        a = torch.randint(-9, 10, (R, 3), generator=gen).to(F64)
        b = torch.randint(-9, 10, (R, 4), generator=gen).to(F64)
        assert torch.equal(leg._rows_product(a, b, rows=8), a.T @ b), R


@pytest.mark.gpu
def test_gradients_of_a_batch_longer_than_one_chunk_of_the_basis_product():
    """More rows than one chunk of ``_rows_product`` (4096) and a remainder: every gradient against one
    ``log_likelihood(noise_var=)`` per series through the unfused path, at ``_check_grad``'s tolerances."""
    lengths = [1500, 2700, 61, 1]
    st = _starts(lengths)
    assert st[-1] > 4096 and st[-1] % 4096
    m, gen = _model(3, 2, F64, 17)
    ts, xs = _ragged(lengths, 2, gen, F64)
    s = (2.0 * torch.rand(st[-1], 2, generator=gen, dtype=F64)).cuda()
    up = torch.randn(len(lengths), generator=gen, dtype=F64).cuda()
    grads = []
    for batched in (True, False):
        p = [t.clone().requires_grad_(True) for t in (m.N, m.R, m.B, m.Lambda, xs, ts, s)]
        mm = leg.LEGMatrices(*p[:4])
        if batched:
            out = leg.log_likelihood_batch(mm, p[5], p[4], lengths, noise_var=p[6])
        else:
            out = torch.stack([leg.log_likelihood(mm, p[5][a:e], p[4][a:e], noise_var=p[6][a:e])
                               for a, e in zip(st[:-1], st[1:])])
        (out * up).sum().backward()
        grads.append([t.grad for t in p])
    for name, got, want in zip(LEG_PARAMS, *grads):
        _check_grad(got, want, "long batch d ll / d %s" % name)


# ---- errors, graph --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_repeated_time_stamp_in_a_noisy_series_names_it():
    m, gen = _model(3, 1, F64, 5)
    lengths = [40, 300, 25, 60]
    ts, xs = _ragged(lengths, 1, gen, F64)
    s = (2.0 * torch.rand(sum(lengths), generator=gen, dtype=F64)).cuda()
    clean = leg.log_likelihood_batch(m, ts, xs, lengths, noise_var=s)
    bad = ts.clone()
    bad[40 + 300 + 11] = bad[40 + 300 + 10]                  # series 2, local rows 10 / 11
    with pytest.raises(cr.NotPSDError, match="series 2"):
        leg.log_likelihood_batch(m, bad, xs, lengths, noise_var=s)
    m8, gen8 = _model(8, 1, F64, 5)                            # the per-series path names it as well
    with pytest.raises(cr.NotPSDError, match="series 2"):
        leg.log_likelihood_batch(m8, bad, xs, lengths, noise_var=s)
    prev = cr.CHECK_POSITIVE_DEFINITE
    cr.CHECK_POSITIVE_DEFINITE = False
    try:
        out = leg.log_likelihood_batch(m, bad, xs, lengths, noise_var=s)
    finally:
        cr.CHECK_POSITIVE_DEFINITE = prev
    assert math.isnan(float(out[2]))
    for b in (0, 1, 3):
        assert float(out[b]) == float(clean[b])


@pytest.mark.gpu
def test_noisy_batch_replays_from_a_graph():
    g, m, ts, xs = _load()
    n = ts.shape[0]
    ts4, xs4 = ts.expand(4, -1).contiguous(), xs.expand(4, -1, -1).contiguous()
    first = torch.rand(4, n, 1, generator=torch.Generator().manual_seed(8), dtype=F64).cuda()
    s4 = first.clone()
    graphed = leg.Graphed(leg.log_likelihood_batch, m, ts4, xs4, noise_var=s4)   # (turns the host check off itself)
    for _ in range(3):
        out = graphed().clone()
    ref = leg.log_likelihood_batch(m, ts4, xs4, noise_var=s4)
    assert float((out - ref).abs().max()) <= 1e-10 * float(ref.abs().max())
    s4.copy_(2.0 * first.flip(0))                                 # new variances in place: the replay follows
    out2 = graphed().clone()
    ref2 = leg.log_likelihood_batch(m, ts4, xs4, noise_var=s4)
    assert float((out2 - ref2).abs().max()) <= 1e-10 * float(ref2.abs().max())
    assert float((out2 - out).abs().min()) > 1e-6
    # the capture owns its plan: more other batches than the cache holds, and the replay still reads its own offsets
    plan = leg._captured_plans[((n,) * 4, str(ts.device))]
    for k in range(leg.PLAN_CACHE_SIZE + 2):
        lengths = [3 + k, 5]
        leg.log_likelihood_batch(m, ts[:sum(lengths)], xs[:sum(lengths)], lengths, noise_var=first[0, :sum(lengths)])
    assert ((n,) * 4, str(ts.device)) not in leg._plans
    assert plan.offsets.tolist() == [0, n, 2 * n, 3 * n, 4 * n]
    assert float((graphed() - ref2).abs().max()) <= 1e-10 * float(ref2.abs().max())

"""leg.log_likelihood_batch(..., observed=mask): many LEG series with missing observations in one launch
(cgps_leg_loglik_batch_obs, leg_batch_kernel<.., OBS = true>) against the one-series pattern kernel
(cgps_leg_mahal_logdet_pair_obs), against one leg.log_likelihood(observed=) per series, against marginalisation (rows
deleted) on the golden series and against the dense Gaussian of the observed entries (tests/_missref.py) under
autograd; offsets, independence of neighbours, errors and graph replay."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import _missref as mr
import _util
from cyclic_gps import _hip, leg
import cyclic_gps.cyclic_reduction as cr

F64, F32 = torch.float64, torch.float32


# ---- recipes of tests/test_leg_batch.py and tests/test_leg_missing.py (copied, not imported) ------------------------
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


def _kernel_model(d, dtype, seed, P):
    """test_leg_missing._kernel_model: the diagonal of N from [0.8, 1.2], so that the symmetric part of G is not nearly
    singular; a table of P blocks whose entry 0 is zero (a row that observes nothing)."""
    gen = torch.Generator().manual_seed(seed)
    Nm = torch.tril(0.4 * torch.randn(d, d, generator=gen, dtype=F64), -1)
    Nm = Nm + torch.diag(0.8 + 0.4 * torch.rand(d, generator=gen, dtype=F64))
    Rm = torch.tril(0.3 * torch.randn(d, d, generator=gen, dtype=F64), -1)
    G = Nm @ Nm.T + Rm - Rm.T + 1e-5 * torch.eye(d, dtype=F64)
    Bs = torch.randn(P, d, 2, generator=gen, dtype=F64)
    table = 0.5 * Bs @ Bs.transpose(-1, -2)
    table[0] = 0
    return G.to(dtype).cuda(), table.to(dtype).cuda(), gen


def _golden_masks(n):
    """test_leg_missing._golden_masks: 30 % of the rows missing at random; the hole and the tail of the reference's CO2
    split plus the first row."""
    rand = torch.rand(n, generator=torch.Generator().manual_seed(1)) > 0.3
    gap = torch.ones(n, dtype=torch.bool)
    gap[262:n - 228] = False
    gap[-28:] = False
    gap[0] = False
    return {"rand30": rand, "gap": gap}


def _starts(lengths):
    s = [0]
    for n in lengths:
        s.append(s[-1] + n)
    return s


def _close(got, want, rtol):
    return abs(got - want) <= rtol * max(1.0, abs(want))


# ---- argument handling (no GPU) -------------------------------------------------------------------------------------
def test_observed_is_checked_before_anything_runs_dense_layout():
    m, _ = _model(2, 2, F64, 0, device="cpu")
    ts, xs = torch.zeros(3, 4, dtype=F64), torch.zeros(3, 4, 2, dtype=F64)
    for bad in (torch.ones(3, 4, 2, dtype=F64), torch.ones(3, 4, dtype=torch.uint8), [[True] * 4] * 3):
        with pytest.raises(ValueError, match="bool"):
            leg.log_likelihood_batch(m, ts, xs, observed=bad)
    for shape in ((3,), (12,), (12, 2), (3, 4, 2, 1), (3, 4, 1), (3, 4, 3), (3, 5), (3, 5, 2), (4, 4), (2, 4, 2)):
        with pytest.raises(ValueError, match="observed"):
            leg.log_likelihood_batch(m, ts, xs, observed=torch.ones(shape, dtype=torch.bool))
    with pytest.raises(ValueError, match="dense layout"):      # the layout's own errors come first, as without a mask
        leg.log_likelihood_batch(m, ts.reshape(-1), xs.reshape(-1, 2), observed=torch.ones(12, dtype=torch.bool))


def test_observed_is_checked_before_anything_runs_ragged_layout():
    m, _ = _model(2, 2, F64, 0, device="cpu")
    ts, xs = torch.zeros(10, dtype=F64), torch.zeros(10, 2, dtype=F64)
    for bad in (torch.ones(10, 2, dtype=F64), torch.ones(10, dtype=torch.int64)):
        with pytest.raises(ValueError, match="bool"):
            leg.log_likelihood_batch(m, ts, xs, [4, 6], observed=bad)
    for shape in ((), (9,), (11,), (9, 2), (10, 1), (10, 3), (10, 2, 1), (2, 5), (2, 5, 2)):
        with pytest.raises(ValueError, match="observed"):
            leg.log_likelihood_batch(m, ts, xs, [4, 6], observed=torch.ones(shape, dtype=torch.bool))
    with pytest.raises(ValueError, match="sum"):
        leg.log_likelihood_batch(m, ts, xs, [4, 5], observed=torch.ones(10, dtype=torch.bool))


def test_empty_batch_with_observed_returns_an_empty_tensor():
    m, _ = _model(3, 1, F64, 0, device="cpu")
    e = torch.zeros(0, dtype=F64)
    for obs in (torch.zeros(0, dtype=torch.bool), torch.zeros(0, 1, dtype=torch.bool)):
        out = leg.log_likelihood_batch(m, e, torch.zeros(0, 1, dtype=F64), [], observed=obs)
        assert out.shape == (0,) and out.dtype == F64
    for obs in (torch.zeros(0, 7, dtype=torch.bool), torch.zeros(0, 7, 1, dtype=torch.bool)):
        out = leg.log_likelihood_batch(m, torch.zeros(0, 7, dtype=F64), torch.zeros(0, 7, 1, dtype=F64), observed=obs)
        assert out.shape == (0,)


def test_c_entry_is_exported_and_checks_its_arguments_before_any_launch():
    assert "cgps_leg_loglik_batch_obs" in _hip.exported_symbols()
    lib = _hip.lib()
    fn = lib.cgps_leg_loglik_batch_obs
    assert lib.cgps_version() == 320
    fake = ctypes.c_void_p(256)
    call = lambda B, tab, P, pat, d=5, dt=_hip.F64: fn(fake, fake, B, fake, tab, P, pat, None, None, d, dt, 4096,   # noqa: E731
                                                       fake, fake, None)
    assert call(2, fake, 0, fake) == 1 and b"cgps_leg_loglik_batch_obs" in lib.cgps_last_error()
    assert call(2, fake, 257, fake) == 1 and call(2, fake, -1, fake) == 1
    assert call(2, None, 2, fake) == 1 and call(2, fake, 2, None) == 1
    assert call(-1, fake, 2, fake) == 1 and call(2 ** 31, fake, 2, fake) == 1
    assert fn(None, None, 2, None, fake, 2, fake, None, None, 5, _hip.F64, 4096, None, None, None) == 1
    # d = 8 and fp64 d = 6 are refused before any launch (the pointers are never touched)
    for d, dt in ((8, _hip.F64), (8, _hip.F32), (6, _hip.F64), (9, _hip.F64)):
        assert call(2, fake, 2, fake, d, dt) == 3
    # an empty batch is no work and no error, whatever the pointers
    assert fn(None, None, 0, None, None, 2, None, None, None, 5, _hip.F64, 4096, None, None, None) == 0
    assert call(0, fake, 256, fake, 7, _hip.F32) == 0


def test_plan_cache_keeps_the_most_recent_and_never_drops_what_a_capture_read(monkeypatch):
    """The cache's lifetime rule, on CPU plans: least recently USED goes first; a plan handed out during a stream
    capture stays for good (the captured kernels hold its device addresses); a capture cannot build a plan."""
    monkeypatch.setattr(leg, "_plans", {})
    monkeypatch.setattr(leg, "_captured_plans", {})
    capturing = [False]
    monkeypatch.setattr(leg, "_capturing", lambda device: capturing[0])
    size = leg.PLAN_CACHE_SIZE
    first = leg._cached_batch_plan([3, 4], "cpu")
    assert first.offsets.tolist() == [0, 3, 7] and leg._cached_batch_plan([3, 4], "cpu") is first
    for k in range(size - 1):
        leg._cached_batch_plan([1, 2 + k], "cpu")
    assert leg._cached_batch_plan([3, 4], "cpu") is first        # used again: now the most recent of a full cache
    leg._cached_batch_plan([9], "cpu")                           # drops [1, 2], the least recently used, not `first`
    assert leg._cached_batch_plan([3, 4], "cpu") is first and len(leg._plans) == size
    assert (1, 2) not in [k[0] for k in leg._plans]
    # a capture reads `first`; any number of other batches later it is still the same object, owned by the module
    capturing[0] = True
    assert leg._cached_batch_plan([3, 4], "cpu") is first
    with pytest.raises(RuntimeError, match="before the capture"):
        leg._cached_batch_plan([5, 5, 5], "cpu")
    capturing[0] = False
    for k in range(3 * size):
        leg._cached_batch_plan([2, 100 + k], "cpu")
    assert len(leg._plans) == size and leg._cached_batch_plan([3, 4], "cpu") is first
    assert leg._cached_batch_plan([5, 5, 5], "cpu").B == 3       # the refused build left nothing behind


# ---- the kernel -----------------------------------------------------------------------------------------------------
KERNEL_LENGTHS = [1, 2, 3, 255, 256, 257, 513, 129, 128]


def _batch_patterns(lengths, P, gen):
    """name -> uint8 [R]: random entries, every row the last entry, every row entry 0, and runs of entry 0 laid across
    every series boundary and across local rows 127/128 and 255/256 of the longer series (the lane-chunk boundaries of
    128 and 256 lanes at one, two and three rows per lane fall inside those runs or at the series' ends)."""
    st = _starts(lengths)
    R = st[-1]
    out = {"random": torch.randint(0, P, (R,), generator=gen).to(torch.uint8),
           "all": torch.full((R,), P - 1, dtype=torch.uint8), "none": torch.zeros(R, dtype=torch.uint8)}
    runs = torch.randint(1, P, (R,), generator=gen).to(torch.uint8)
    for s, n in zip(st[:-1], lengths):
        runs[max(0, s - 3):s + 2] = 0
        for k in (128, 256):
            if n > k:
                runs[s + k - 7:min(s + k + 9, s + n)] = 0
    runs[R - 3:] = 0
    out["runs"] = runs
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("d,dtype", [(1, F64), (2, F64), (3, F64), (4, F64), (5, F64), (7, F64), (2, F32), (4, F32),
                                     (5, F32), (6, F32), (7, F32)], ids=lambda p: str(p).replace("torch.", ""))
def test_batch_pattern_kernel_against_the_one_series_kernel(d, dtype):
    """One row, both sides of one row per lane against two (and, at 7 x 7 fp64 with its 128 lanes, of two against
    three), long and short series as neighbours; tables of 2 and 8 entries; a byte past a deliberately short table
    takes its last entry; the prior log-det is cgps_leg_loglik_batch's bit for bit."""
    rtol = 1e-9 if dtype == F64 else 3e-4
    for P in (2, 8):
        G, table, gen = _kernel_model(d, dtype, 300 + 10 * d + P, P)
        lengths = [KERNEL_LENGTHS[i] for i in torch.randperm(len(KERNEL_LENGTHS), generator=gen).tolist()]
        st = _starts(lengths)
        plan = leg._BatchPlan(lengths, "cuda")
        ts, _ = _ragged(lengths, 1, gen, dtype)
        v = torch.randn(st[-1], d, generator=gen, dtype=F64).to(dtype).cuda()
        q = torch.randn(st[-1], generator=gen, dtype=F64).to(dtype).cuda()
        prior = leg.leg_loglik_batch_reductions(ts, G, table[1].contiguous(), v, q, plan)[0][:, 2].clone()
        cases = [(name, pat.cuda(), table) for name, pat in _batch_patterns(lengths, P, gen).items()]
        wild = torch.randint(0, 256, (st[-1],), generator=gen).to(torch.uint8).cuda()
        wild[-1] = 255
        cases.append(("clamped", wild, table[:2].clone()))
        for name, pat, tab in cases:
            out, info = leg.leg_loglik_batch_reductions_obs(ts, G, tab, pat, v, q, plan)
            assert out.dtype == F64 and out.shape == (len(lengths), 4)
            assert int(info.abs().max()) == 0, (P, name, info.tolist())
            assert torch.equal(out[:, 2], prior), (P, name, out[:, 2].tolist(), prior.tolist())
            ref = torch.stack([torch.stack(leg.leg_loglik_reductions_obs(ts[s:e], G, tab, pat[s:e], v[s:e])).double()
                               for s, e in zip(st[:-1], st[1:])]).cpu()
            qs = torch.stack([q[s:e].double().sum() for s, e in zip(st[:-1], st[1:])]).cpu()
            got = out.cpu()
            for b, n in enumerate(lengths):
                what = (P, name, b, n)
                m1, l1, s1, q1 = got[b].tolist()
                m0, l0, s0 = ref[b].tolist()
                print("kernel", d, dtype, what, "mahal %.3e logdet %.3e prior %.3e" % (
                    abs(m1 - m0) / max(1.0, abs(m0)), abs(l1 - l0) / max(1.0, abs(l0)), abs(s1 - s0) / max(1.0, abs(s0))))
                assert _close(l1, l0, rtol), (what, l1, l0)
                assert _close(m1, m0, 10 * rtol), (what, m1, m0)
                assert _close(s1, s0, rtol), (what, s1, s0)
                assert _close(q1, float(qs[b]), 1e-12), (what, q1, float(qs[b]))


@pytest.mark.gpu
def test_a_series_above_batch_max_rows_takes_the_one_series_kernel_and_lands_in_its_slot():
    d, P = 3, 8
    G, table, gen = _kernel_model(d, F64, 41, P)
    lengths = [40, leg.BATCH_MAX_ROWS + 1, 7]
    st = _starts(lengths)
    plan = leg._BatchPlan(lengths, "cuda")
    assert plan.long == [1]
    ts, _ = _ragged(lengths, 1, gen, F64)
    v = torch.randn(st[-1], d, generator=gen, dtype=F64).cuda()
    q = torch.randn(st[-1], generator=gen, dtype=F64).cuda()
    pat = torch.randint(0, P, (st[-1],), generator=gen).to(torch.uint8).cuda()
    out, info = leg.leg_loglik_batch_reductions_obs(ts, G, table, pat, v, q, plan)
    assert int(info.abs().max()) == 0
    for b, (s, e) in enumerate(zip(st[:-1], st[1:])):
        m0, l0, s0 = (float(x) for x in leg.leg_loglik_reductions_obs(ts[s:e], G, table, pat[s:e], v[s:e]))
        m1, l1, s1, q1 = out[b].tolist()
        assert _close(l1, l0, 1e-9) and _close(s1, s0, 1e-9) and _close(m1, m0, 1e-8), (b, out[b].tolist(), (m0, l0, s0))
        assert _close(q1, float(q[s:e].sum()), 1e-12)
    # and through the public entry
    m, gen = _model(3, 2, F64, 43)
    ts, xs = _ragged(lengths, 2, gen, F64)
    obs = (torch.rand(st[-1], 2, generator=gen) < 0.6).cuda()
    got = leg.log_likelihood_batch(m, ts, xs, lengths, observed=obs)
    for b, (s, e) in enumerate(zip(st[:-1], st[1:])):
        want = float(leg.log_likelihood(m, ts[s:e], xs[s:e], observed=obs[s:e]))
        assert _close(float(got[b]), want, 1e-9), (b, float(got[b]), want)


@pytest.mark.gpu
def test_bit_identical_repeats_own_mask_per_series_and_independent_of_neighbours():
    """Every series has its own mask, so a kernel that indexed the pattern by the local row alone (without the series'
    offset) would give every series but the first another series' mask."""
    m, gen = _model(5, 2, F64, 3)
    lengths = [502, 33, 1, 700, 129]
    st = _starts(lengths)
    ts, xs = _ragged(lengths, 2, gen, F64)
    obs = (torch.rand(st[-1], 2, generator=gen) < 0.6).cuda()
    obs[st[2]] = True                                          # the one-row series observes something
    a = leg.log_likelihood_batch(m, ts, xs, lengths, observed=obs)
    b = leg.log_likelihood_batch(m, ts, xs, lengths, observed=obs)
    assert torch.equal(a, b)
    for i, (s, e) in enumerate(zip(st[:-1], st[1:])):
        want = float(leg.log_likelihood(m, ts[s:e], xs[s:e], observed=obs[s:e]))
        assert _close(float(a[i]), want, 1e-9), (i, float(a[i]), want)
    # reversed in order, behind a new neighbour with a mask and data of its own: every value the same
    order = list(reversed(range(len(lengths))))
    cat = lambda t, head: torch.cat([head] + [t[st[i]:st[i + 1]] for i in order])   # noqa: E731
    c = leg.log_likelihood_batch(m, cat(ts, ts[:50]), cat(xs, xs[:50] * 3.0), [50] + [lengths[i] for i in order],
                                 observed=cat(obs, ~obs[:50]))
    for k, i in enumerate(order):
        assert abs(float(c[k + 1]) - float(a[i])) <= 1e-12 * abs(float(a[i])), (i, float(c[k + 1]), float(a[i]))
    # a neighbour's mask and data change in place: the others do not move at all
    obs2, xs2 = obs.clone(), xs.clone()
    obs2[st[1]:st[2]] = ~obs2[st[1]:st[2]]
    xs2[st[1]:st[2]] *= -2.0
    e = leg.log_likelihood_batch(m, ts, xs2, lengths, observed=obs2)
    assert float(e[1]) != float(a[1])
    for i in (0, 2, 3, 4):
        assert abs(float(e[i]) - float(a[i])) <= 1e-12 * abs(float(a[i])), (i, float(e[i]), float(a[i]))


# ---- the public entry -----------------------------------------------------------------------------------------------
PUBLIC_LENGTHS = [7, 1, 300, 2, 65, 40]
UNOBSERVED, FULL = 4, 5                                         # the series of 65 rows sees nothing, that of 40 everything


def _public_model(d, obs_dim, dtype):
    """``_model`` under the first seed of 100 d + obs_dim, + 1000, + 2000, ... whose N N^T (the symmetric part of G) has
    no eigenvalue below 1e-2.  The recipe's diagonal of N, 0.8 + 0.4 randn, comes near zero for some seeds (smallest
    eigenvalue 7e-7 at 702, 3e-4 at 802); the blocks of such a G, rounded to fp32, lose the one-series fp32 call its
    digits against fp64 whatever kernel reduces them (test_leg_missing._kernel_model's note), and that call is the
    yardstick here.  The criterion looks at the model alone, never at a result."""
    seed = 100 * d + obs_dim
    while True:
        m, gen = _model(d, obs_dim, dtype, seed)
        N = m.N.double().cpu()
        if float(torch.linalg.eigvalsh(N @ N.T).min()) >= 1e-2:
            return m, gen
        seed += 1000


def _per_series_observed(m, ts, xs, obs, lengths):
    st = _starts(lengths)
    return [float(leg.log_likelihood(m, ts[s:e], xs[s:e], observed=obs[s:e])) for s, e in zip(st[:-1], st[1:])]


@pytest.mark.gpu
@pytest.mark.parametrize("d", range(1, 9))
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_against_one_masked_call_per_series_every_rank(d, dtype):
    """Ranks 1..8 in both dtypes (d = 8 and fp64 d = 6 take the per-series path), obs_dim 1 and 2, masks that keep
    ~60 % of the entries.  fp32 is compared with the fp64 per-series value of the same (fp32-rounded) inputs; the
    existing fp32 ``log_likelihood(observed=)`` must itself be within a quarter of that tolerance on these seeds."""
    rtol = 1e-9 if dtype == F64 else 1e-3
    lengths = PUBLIC_LENGTHS
    st = _starts(lengths)
    for obs_dim in (1, 2):
        m, gen = _public_model(d, obs_dim, dtype)
        # (fp32: gaps of at least 0.5, so that I - E^T E of the random 8 x 8 generators stays well conditioned)
        ts, xs = _ragged(lengths, obs_dim, gen, dtype, gap0=0.05 if dtype == F64 else 0.5)
        obs = (torch.rand(st[-1], obs_dim, generator=gen) < 0.6).cuda()
        obs[st[UNOBSERVED]:st[UNOBSERVED + 1]] = False
        obs[st[FULL]:st[FULL + 1]] = True
        out = leg.log_likelihood_batch(m, ts, xs, torch.tensor(lengths), observed=obs)
        assert out.dtype == dtype and out.shape == (len(lengths),)
        if dtype == F64:
            ref = _per_series_observed(m, ts, xs, obs, lengths)
        else:
            m64 = leg.LEGMatrices(*(t.double() for t in (m.N, m.R, m.B, m.Lambda)))
            ref = _per_series_observed(m64, ts.double(), xs.double(), obs, lengths)
            single = _per_series_observed(m, ts, xs, obs, lengths)
            worst = max(abs(a - r) / max(1.0, abs(r)) for a, r in zip(single, ref))
            print("public d=%d obs=%d f32: existing one-series call against fp64, worst %.3e" % (d, obs_dim, worst))
            assert worst <= 0.25 * rtol, (d, obs_dim, single, ref)
        got = out.tolist()
        print("public d=%d obs=%d %s: batched call against the reference, worst %.3e" % (
            d, obs_dim, dtype, max(abs(a - r) / max(1.0, abs(r)) for a, r in zip(got, ref))))
        for n, a, r in zip(lengths, got, ref):
            assert _close(a, r, rtol), (d, obs_dim, n, a, r)
        assert abs(got[UNOBSERVED]) <= 1e-9, got[UNOBSERVED]
        s, e = st[FULL], st[FULL + 1]
        full = float(leg.log_likelihood_batch(m, ts[s:e], xs[s:e], [lengths[FULL]])[0])
        assert _close(got[FULL], full, rtol), (got[FULL], full)
        # whatever the unobserved entries hold
        holed = torch.where(obs, xs, torch.full_like(xs, float("nan")))
        assert torch.equal(leg.log_likelihood_batch(m, ts, holed, lengths, observed=obs), out)
        if obs_dim == 1:                                        # whole-row flags are the same mask
            assert torch.equal(leg.log_likelihood_batch(m, ts, xs, lengths, observed=obs[:, 0]), out)
        # the dense layout with padded tails (time stamps go on increasing, data NaN, nothing observed)
        nmax = max(lengths)
        tsd = torch.empty(len(lengths), nmax, dtype=dtype, device="cuda")
        xsd = torch.full((len(lengths), nmax, obs_dim), float("nan"), dtype=dtype, device="cuda")
        obd = torch.zeros(len(lengths), nmax, obs_dim, dtype=torch.bool, device="cuda")
        for b, n in enumerate(lengths):
            tsd[b, :n], xsd[b, :n], obd[b, :n] = ts[st[b]:st[b + 1]], xs[st[b]:st[b + 1]], obs[st[b]:st[b + 1]]
            tsd[b, n:] = ts[st[b + 1] - 1] + torch.arange(1, nmax - n + 1, dtype=dtype, device="cuda")
        dense = leg.log_likelihood_batch(m, tsd, xsd, observed=obd).tolist()
        for n, a, r in zip(lengths, dense, got):
            assert _close(a, r, rtol), ("padded", d, obs_dim, n, a, r)
        assert abs(dense[UNOBSERVED]) <= 1e-9


@pytest.mark.gpu
def test_golden_series_eight_copies_with_rows_deleted():
    g, m, ts, xs = _load()
    n = ts.shape[0]
    masks = [mk.cuda() for mk in _golden_masks(n).values()]
    want = [float(leg.log_likelihood(m, ts[mk], xs[mk])) for mk in masks]
    obs = torch.stack([masks[b % 2] for b in range(8)])
    holed = torch.where(obs.unsqueeze(-1), xs.expand(8, -1, -1), torch.full((), float("nan"), dtype=F64, device="cuda"))
    for ob in (obs, obs.unsqueeze(-1)):
        out = leg.log_likelihood_batch(m, ts.expand(8, -1).contiguous(), holed.contiguous(), observed=ob)
        assert out.shape == (8,)
        for b, got in enumerate(out.tolist()):
            assert _close(got, want[b % 2], 1e-9), (b, got, want[b % 2])


# ---- gradients --------------------------------------------------------------------------------------------------------
LEG_PARAMS = ("N", "R", "B", "Lambda", "xs", "ts")
DENSE_CASES = {(3, 3, 37): (11, 111, 211), (5, 2, 64): (12, 112, 212)}
_dense = {}


def _dense_batch_ref(d, obs, n):
    """Three series (the data, times and mask of three seeds of _missref.leg_case under the model of the first), a
    random upstream weight per series, and the weighted sums of the dense reference's value and gradients."""
    key = (d, obs, n)
    if key not in _dense:
        seeds = DENSE_CASES[key]
        cases = [mr.leg_case(d, obs, n, s) for s in seeds]
        model = cases[0][0][:4]
        w = torch.randn(len(seeds), generator=torch.Generator().manual_seed(seeds[0]), dtype=F64)
        lls, gsum, gxs, gts = [], [torch.zeros_like(t) for t in model], [], []
        for wb, (case, mask) in zip(w.tolist(), cases):
            ll, grads = mr.leg_dense_value_and_grads(*model, case[5], case[4], mask)
            lls.append(ll)
            for acc, gpar in zip(gsum, grads[:4]):
                acc += wb * gpar
            gxs.append(wb * grads[4])
            gts.append(wb * grads[5])
        xs = torch.stack([c[0][4] for c in cases])
        ts = torch.stack([c[0][5] for c in cases])
        mask = torch.stack([c[1] for c in cases])
        _dense[key] = model, xs, ts, mask, w, torch.stack(lls), gsum + [torch.stack(gxs), torch.stack(gts)]
    return _dense[key]


def _check_grad(got, want, what):
    """test_leg_missing._check_grad, fp64"""
    want = want.detach().to("cpu", F64)
    assert got is not None, what + " is missing"
    got = got.detach().to("cpu", F64)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-7, atol=1e-10 * float(want.abs().max()), err_msg=what)


@pytest.mark.gpu
@pytest.mark.parametrize("frozen", [False, True], ids=["all", "NR_frozen"])
@pytest.mark.parametrize("d,obs,n", list(DENSE_CASES))
def test_gradients_against_the_dense_reference(d, obs, n, frozen):
    model, xs, ts, mask, w, lls, grads = _dense_batch_ref(d, obs, n)
    nan_xs = torch.where(mask, xs, torch.full_like(xs, float("nan")))
    train = [not (frozen and name in ("N", "R")) for name in LEG_PARAMS]
    p = [t.clone().cuda().requires_grad_(r) for t, r in zip(list(model) + [nan_xs, ts], train)]
    out = leg.log_likelihood_batch(leg.LEGMatrices(*p[:4]), p[5], p[4], observed=mask.cuda())
    for b in range(len(lls)):
        assert _close(float(out[b]), float(lls[b]), 1e-9), (b, float(out[b]), float(lls[b]))
    (out * w.cuda()).sum().backward()
    for name, leaf, want, r in zip(LEG_PARAMS, p, grads, train):
        if r:
            _check_grad(leaf.grad, want, "d ll / d %s" % name)
        else:
            assert leaf.grad is None, name
    assert float(p[4].grad[~mask.cuda()].abs().max()) == 0.0


# ---- errors, graph --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_repeated_time_stamp_in_a_masked_series_names_it():
    m, gen = _model(3, 1, F64, 5)
    lengths = [40, 300, 25, 60]
    ts, xs = _ragged(lengths, 1, gen, F64)
    obs = (torch.rand(sum(lengths), generator=gen) < 0.6).cuda()
    clean = leg.log_likelihood_batch(m, ts, xs, lengths, observed=obs)
    bad = ts.clone()
    bad[40 + 300 + 11] = bad[40 + 300 + 10]                  # series 2, local rows 10 / 11
    with pytest.raises(cr.NotPSDError, match="series 2"):
        leg.log_likelihood_batch(m, bad, xs, lengths, observed=obs)
    prev = cr.CHECK_POSITIVE_DEFINITE
    cr.CHECK_POSITIVE_DEFINITE = False
    try:
        out = leg.log_likelihood_batch(m, bad, xs, lengths, observed=obs)
    finally:
        cr.CHECK_POSITIVE_DEFINITE = prev
    assert math.isnan(float(out[2]))
    for b in (0, 1, 3):
        assert float(out[b]) == float(clean[b])


@pytest.mark.gpu
def test_masked_batch_replays_from_a_graph():
    g, m, ts, xs = _load()
    n = ts.shape[0]
    masks = _golden_masks(n)
    ts4, xs4 = ts.expand(4, -1).contiguous(), xs.expand(4, -1, -1).contiguous()
    first = torch.stack([masks["rand30"], masks["gap"], masks["rand30"], masks["gap"]]).cuda()
    obs = first.clone()
    graphed = leg.Graphed(leg.log_likelihood_batch, m, ts4, xs4, observed=obs)   # (turns the host check off itself)
    for _ in range(3):
        out = graphed().clone()
    ref = leg.log_likelihood_batch(m, ts4, xs4, observed=obs)
    assert float((out - ref).abs().max()) <= 1e-10 * float(ref.abs().max())
    obs.copy_(first.flip(0))                                     # new masks in place: the replay follows
    out2 = graphed().clone()
    ref2 = leg.log_likelihood_batch(m, ts4, xs4, observed=obs)
    assert float((out2 - ref2).abs().max()) <= 1e-10 * float(ref2.abs().max())
    assert float((out2 - out).abs().min()) > 1e-6
    # the capture owns its plan: more other batches than the cache holds, and the replay still reads its own offsets
    plan = leg._captured_plans[((n,) * 4, str(ts.device))]
    for k in range(leg.PLAN_CACHE_SIZE + 2):
        lengths = [3 + k, 5]
        leg.log_likelihood_batch(m, ts[:sum(lengths)], xs[:sum(lengths)], lengths, observed=first[0, :sum(lengths)])
    assert ((n,) * 4, str(ts.device)) not in leg._plans
    assert plan.offsets.tolist() == [0, n, 2 * n, 3 * n, 4 * n]
    assert float((graphed() - ref2).abs().max()) <= 1e-10 * float(ref2.abs().max())

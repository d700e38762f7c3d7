"""cgps_leg_intercast_seg (csrc/cgps_leg.h: leg_intercast_seg_kernel), the prediction kernel of a concatenated batch:
its argument checks without a GPU, and on the GPU its results against cgps_leg_intercast called series by series on the
slices -- bit for bit, since both kernels run the same device function -- with everything a lane must not read set to
NaN."""
import ctypes

import pytest
import torch

from cyclic_gps import _hip, leg, predict

LENGTHS = [1, 2, 3, 33, 64, 65, 257, 5]
F64 = torch.float64


def standard_targets(ts, b):
    """Targets of series b of the standard batch (ts: its own times, fp64, CPU), strictly increasing.  Between them the
    series cover: no target at all; a single target before the first row; a one-row series (before, at, after its
    row); and, for the longer ones, before the first row, exactly at it, interior points, an interior observation time
    itself, a point within 1e-8 + 1e-5 |t| of the last row, and after the last row."""
    n = ts.shape[0]
    if n == 1:
        return torch.stack([ts[0] - 0.7, ts[0], ts[0] + 0.5])
    if n == 2:
        return ts[:0]
    if n == 3:
        return ts[:1] - 0.5
    mid = 0.5 * (ts[:-1] + ts[1:])
    pick = mid[:: max(1, (n - 1) // 12)]
    last = ts[-1]
    near_last = last - 0.4e-5 * last.abs()                       # inside the closeness band, above every midpoint
    parts = [ts[:1] - 1.3, ts[:1], pick, ts[n // 2:n // 2 + 1], near_last[None], last[None] + 0.4]
    if b % 2:
        parts = parts[2:]                                        # (a series that starts in the interior)
    return torch.unique(torch.cat(parts))


def standard_batch(lengths, seed):
    """Per-series fp64 CPU times (series overlap and do not increase from one to the next) and their targets."""
    gen = torch.Generator().manual_seed(seed)
    ts = [1.5 * (b % 3) + torch.cumsum(0.2 + torch.rand(n, generator=gen, dtype=F64), 0) for b, n in enumerate(lengths)]
    return ts, [standard_targets(t, b) for b, t in enumerate(ts)]


def test_entry_is_exported_and_checks_its_arguments_before_any_launch():
    assert "cgps_leg_intercast_seg" in _hip.exported_symbols()
    lib = _hip.lib()
    fn = lib.cgps_leg_intercast_seg
    fake = ctypes.c_void_p(4096)                                 # never dereferenced: every call below returns first

    def call(B, P, d=3, dtype=_hip.F64, ptrs=None):
        p = ptrs if ptrs is not None else [fake] * 10
        return fn(p[0], p[1], p[2], p[3], B, P, p[4], d, dtype, p[5], p[6], p[7], p[8], p[9], None)

    assert call(-1, 4) == 1 and b"cgps_leg_intercast_seg" in lib.cgps_last_error()
    assert call(2, -1) == 1
    assert call(2, 4, ptrs=[None] * 10) == 1
    for hole in (0, 1, 2, 3, 4, 5, 6, 8, 9):                    # (7, the off-diagonal blocks, may be null: one one-row series)
        ptrs = [fake] * 10
        ptrs[hole] = None
        assert call(2, 4, ptrs=ptrs) == 1, hole
    assert call(0, 4, ptrs=[None] * 10) == 0                     # nothing to do: OK without touching the runtime
    assert call(2, 0, ptrs=[None] * 10) == 0
    assert call(0, 0, ptrs=[None] * 10) == 0
    assert call(2, 4, d=0) == 3 and call(2, 4, d=9) == 3
    assert call(2, 4, dtype=7) == 3
    assert lib.cgps_version() == 320


def _random_posterior(n, d, gen):
    A = torch.randn(n, d, d, generator=gen, dtype=F64) * 0.2
    Rs = A @ A.transpose(-1, -2) + 0.5 * torch.eye(d, dtype=F64)
    Os = torch.randn(max(n - 1, 0), d, d, generator=gen, dtype=F64) * 0.05
    return torch.randn(n, d, generator=gen, dtype=F64), Rs, Os


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("d", range(1, 9))
def test_segmented_intercast_equals_the_one_series_kernel_bit_for_bit(d, dtype, monkeypatch):
    """Every rank and both precisions.  The one-series results are first held to the torch form of the same glue (the
    tolerances of test_hip_intercast_against_torch_ops), so that the bit-equality below is equality with a right answer."""
    gen = torch.Generator().manual_seed(300 + d)
    Nm = torch.tril(torch.randn(d, d, generator=gen, dtype=F64)) * 0.4 + torch.eye(d, dtype=F64)
    Rm = torch.tril(torch.randn(d, d, generator=gen, dtype=F64), -1) * 0.3
    m = leg.LEGMatrices(Nm.to(dtype).cuda(), Rm.to(dtype).cuda(), torch.ones(1, d, dtype=dtype).cuda(),
                        torch.ones(1, 1, dtype=dtype).cuda())
    G = m.G
    ts, tts = standard_batch(LENGTHS, 40 + d)
    tlens = [int(t.shape[0]) for t in tts]
    assert 0 in tlens and 1 in tlens and sum(tlens) > 64         # more than one workgroup of targets
    post = [_random_posterior(n, d, gen) for n in LENGTHS]
    dev = lambda t: t.to(dtype).cuda()                           # noqa: E731
    want_m, want_c = [], []
    tol = dict(rtol=1e-9, atol=1e-11) if dtype == F64 else dict(rtol=2e-3, atol=2e-4)
    for (mu, Rs, Os), t, tt in zip(post, ts, tts):
        if tt.shape[0]:
            pm, pc = predict._intercast_hip(G, dev(mu), dev(Rs), dev(Os), dev(t), dev(tt))
            monkeypatch.setenv("CGPS_LEG_TORCH_INTERCAST", "1")
            rm, rc = predict.intercast(m, dev(mu), (dev(Rs), dev(Os)), dev(t), dev(tt))
            monkeypatch.delenv("CGPS_LEG_TORCH_INTERCAST")
            torch.testing.assert_close(pm, rm, **tol)
            torch.testing.assert_close(pc, rc, **tol)
            want_m.append(pm)
            want_c.append(pc)
    want_m, want_c = torch.cat(want_m), torch.cat(want_c)
    assert torch.isfinite(want_m).all() and torch.isfinite(want_c).all()

    plan = leg._cached_batch_plan(LENGTHS, G.device)
    tplan = leg._cached_batch_plan(tlens, G.device, make=predict._TargetPlan)
    mu = dev(torch.cat([p[0] for p in post]))
    Rs = dev(torch.cat([p[1] for p in post]))
    gap = torch.zeros(1, d, d, dtype=F64)
    Os = dev(torch.cat([x for p in post for x in (p[2], gap)][:-1]))
    tcat, ttcat = dev(torch.cat(ts)), dev(torch.cat(tts))
    got_m, got_c = predict._intercast_seg_hip(G, mu, Rs, Os, tcat, plan, ttcat, tplan)
    assert torch.equal(got_m, want_m) and torch.equal(got_c, want_c)

    # nothing is read across a series boundary: NaN in every cut gap's off-diagonal block changes nothing
    Os_nan = Os.clone()
    Os_nan[plan.boundary_rows()] = float("nan")
    got_m, got_c = predict._intercast_seg_hip(G, mu, Rs, Os_nan, tcat, plan, ttcat, tplan)
    assert torch.equal(got_m, want_m) and torch.equal(got_c, want_c)
    # ... and neither does NaN in the rows of the two neighbours that touch series 4 (its own targets looked at)
    b = 4
    lo, hi = plan.starts[b], plan.starts[b + 1]
    mu_n, Rs_n, ts_n = mu.clone(), Rs.clone(), tcat.clone()
    for r in (lo - 1, hi):
        mu_n[r], Rs_n[r], ts_n[r] = float("nan"), float("nan"), float("nan")
    Os_nan[lo - 2], Os_nan[hi] = float("nan"), float("nan")      # the neighbours' own last / first inner blocks
    got_m, got_c = predict._intercast_seg_hip(G, mu_n, Rs_n, Os_nan, ts_n, plan, ttcat, tplan)
    k0, k1 = tplan.starts[b], tplan.starts[b + 1]
    assert k1 - k0 > 4
    assert torch.equal(got_m[k0:k1], want_m[k0:k1]) and torch.equal(got_c[k0:k1], want_c[k0:k1])


@pytest.mark.gpu
def test_a_batch_of_one_row_series_has_no_off_diagonal_block_to_read():
    """One one-row series (R = 1: a null off-diagonal pointer) and several of them (every gap is a cut)."""
    d, dtype = 3, torch.float64
    gen = torch.Generator().manual_seed(9)
    m = leg.LEGMatrices(torch.eye(d, dtype=dtype).cuda(), torch.zeros(d, d, dtype=dtype).cuda(),
                        torch.ones(1, d, dtype=dtype).cuda(), torch.ones(1, 1, dtype=dtype).cuda())
    G = m.G
    for lengths in ([1], [1, 1, 1]):
        B = len(lengths)
        ts = torch.tensor([1.0, 0.5, 2.0][:B], dtype=dtype).cuda()
        tt = torch.stack([ts - 0.3, ts, ts + 0.6], 1).reshape(-1)
        mu, Rs, _ = _random_posterior(B, d, gen)
        mu, Rs = mu.cuda(), Rs.cuda()
        Os = torch.full((B - 1, d, d), float("nan"), dtype=dtype).cuda()
        plan = leg._cached_batch_plan(lengths, G.device)
        tplan = leg._cached_batch_plan([3] * B, G.device, make=predict._TargetPlan)
        got_m, got_c = predict._intercast_seg_hip(G, mu, Rs, Os, ts, plan, tt, tplan)
        for b in range(B):
            pm, pc = predict._intercast_hip(G, mu[b:b + 1], Rs[b:b + 1], Os[:0], ts[b:b + 1], tt[3 * b:3 * b + 3])
            assert torch.equal(got_m[3 * b:3 * b + 3], pm) and torch.equal(got_c[3 * b:3 * b + 3], pc)

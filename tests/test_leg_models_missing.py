"""leg.log_likelihood_models_observed(..., observed=): M LEG models over one batch of series with missing observations, in one
launch (cgps_leg_loglik_models_obs: the pattern bytes once for the batch, a table of diagonal terms per model).  Against
cgps_leg_loglik_batch_obs on every model's slices bit for bit, against a loop of leg.log_likelihood_batch(observed=)
over the models, and against the dense fp64 Gaussian of the observed entries (_missref, no shared code)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import _missref as mr
import _modelscase as mc
from cyclic_gps import _hip, leg
import cyclic_gps.cyclic_reduction as cr

F64, F32 = torch.float64, torch.float32
LENGTHS = mc.BOUNDARY_LENGTHS


# ---- argument handling and the C entry's checks (no GPU) -------------------------------------------------------------

def test_new_symbol_is_exported_and_declared():
    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert "cgps_leg_loglik_models_obs" in _hip.exported_symbols() and hasattr(lib, "cgps_leg_loglik_models_obs")
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cgps.h")
    assert "int cgps_leg_loglik_models_obs(" in open(header).read()
    assert _hip.lib().cgps_version() == 320


def test_c_entry_checks_its_arguments_before_any_launch():
    lib = _hip.lib()
    fn = lib.cgps_leg_loglik_models_obs
    fake = ctypes.c_void_p(256)
    # (ts, offsets, B, R, M, G, A_table, P, pattern, v, q, d, dtype, max_rows, out4, info2, stream)
    call = lambda B=2, R=10, M=3, P=4, d=5, dt=_hip.F64: fn(fake, fake, B, R, M, fake, fake, P, fake, None, None, d, dt,   # noqa: E731
                                                           4096, fake, fake, None)
    for M in (0, -1, 65536):
        assert call(M=M) == 1 and b"outside 1..65535" in lib.cgps_last_error()
    for P in (0, -1, 257):
        assert call(P=P) == 1 and b"outside 1..256" in lib.cgps_last_error()
    assert call(B=-1) == 1 and call(R=-1) == 1 and call(B=2 ** 31) == 1
    assert b"cgps_leg_loglik_models_obs" in lib.cgps_last_error()
    for k in (0, 1, 5, 6, 8, 14, 15):                  # every pointer but v and q (null: zeros), one at a time
        args = [fake, fake, 2, 10, 3, fake, fake, 4, fake, None, None, 5, _hip.F64, 4096, fake, fake, None]
        args[k] = None
        assert fn(*args) == 1 and b"cgps_leg_loglik_models_obs" in lib.cgps_last_error(), k
    for d, dt in ((8, _hip.F64), (8, _hip.F32), (6, _hip.F64)):
        assert call(d=d, dt=dt) == 3 and b"cgps_leg_loglik_models_obs" in lib.cgps_last_error()
    assert call(d=9) == 3
    # an empty batch is no work and no error, whatever the pointers
    assert fn(None, None, 0, 0, 3, None, None, 4, None, None, None, 5, _hip.F64, 4096, None, None, None) == 0
    assert call(B=0, P=256, d=7, dt=_hip.F32) == 0


def test_observed_is_checked_as_the_batch_checks_it():
    ms = [mc.model(2, 2, F64, s, device="cpu") for s in (0, 1)]
    ts, xs = torch.zeros(3, 4, dtype=F64), torch.zeros(3, 4, 2, dtype=F64)
    for bad in (torch.ones(3, 4, 2, dtype=F64), torch.ones(3, 4, dtype=torch.int64), [[True] * 4] * 3, 1):
        with pytest.raises(ValueError, match="bool"):
            leg.log_likelihood_models_observed(ms, ts, xs, observed=bad)
    for shape in ((3,), (12,), (12, 2), (3, 4, 1), (3, 4, 3), (3, 5), (2, 4, 2)):
        with pytest.raises(ValueError, match="observed"):
            leg.log_likelihood_models_observed(ms, ts, xs, observed=torch.ones(shape, dtype=torch.bool))
    ts, xs = torch.zeros(10, dtype=F64), torch.zeros(10, 2, dtype=F64)
    for shape in ((), (9,), (11,), (10, 1), (10, 3), (2, 5), (2, 5, 2)):
        with pytest.raises(ValueError, match="observed"):
            leg.log_likelihood_models_observed(ms, ts, xs, [4, 6], observed=torch.ones(shape, dtype=torch.bool))
    with pytest.raises(ValueError, match="sum"):                 # the layout's own errors, as without a mask
        leg.log_likelihood_models_observed(ms, ts, xs, [4, 5], observed=torch.ones(10, dtype=torch.bool))
    with pytest.raises(ValueError, match="model 1"):             # ... and the models'
        leg.log_likelihood_models_observed([ms[0], mc.model(3, 2, F64, 1, device="cpu")], ts, xs, [4, 6],
                                  observed=torch.ones(10, dtype=torch.bool))


def test_empty_batch_with_a_mask_gives_one_empty_row_per_model():
    ms = [mc.model(3, 1, F64, s, device="cpu") for s in (0, 1, 2)]
    e = torch.zeros(0, dtype=F64)
    for ob in (torch.zeros(0, dtype=torch.bool), torch.zeros(0, 1, dtype=torch.bool)):
        out = leg.log_likelihood_models_observed(ms, e, torch.zeros(0, 1, dtype=F64), [], observed=ob)
        assert out.shape == (3, 0) and out.dtype == F64
    out = leg.log_likelihood_models_observed(ms, torch.zeros(0, 7, dtype=F64), torch.zeros(0, 7, 1, dtype=F64),
                                    observed=torch.zeros(0, 7, dtype=torch.bool))
    assert out.shape == (3, 0)


def test_wrapper_refuses_wrong_operands_before_any_launch():
    plan = leg._BatchPlan([4, 6], "cpu")
    G, v, q = torch.zeros(2, 3, 3, dtype=F64), torch.zeros(2, 10, 3, dtype=F64), torch.zeros(2, 10, dtype=F64)
    ts = torch.zeros(10, dtype=F64)
    with pytest.raises(ValueError, match="pattern"):
        leg.leg_loglik_models_reductions_obs(ts, G, torch.zeros(2, 4, 3, 3, dtype=F64), torch.zeros(10, dtype=torch.uint8), v, q, plan)


# ---- the kernel ------------------------------------------------------------------------------------------------------

def _kernel_case(d, dtype, M, P, seed):
    """Hand-built operands: generators of M models, a table of P symmetric positive semi-definite blocks per model (entry
    0 zero: a row that observes nothing), bytes in 0..P-1 with runs of zeros across the series' ends, random v and q."""
    gen = torch.Generator().manual_seed(seed)
    G = torch.stack([mc.model(d, 1, dtype, seed + 17 * k).G for k in range(M)]).contiguous()
    Bs = torch.randn(M, P, d, 2, generator=gen, dtype=F64)
    A_table = 0.5 * Bs @ Bs.transpose(-1, -2)
    A_table[:, 0] = 0
    ts, _ = mc.ragged(LENGTHS, 1, gen, dtype)
    st = mc.starts(LENGTHS)
    R = st[-1]
    pattern = torch.randint(0, P, (R,), generator=gen).to(torch.uint8)
    pattern[st[mc.DEAD]:st[mc.DEAD + 1]] = 0
    pattern[st[mc.ENDS]] = 0
    pattern[st[mc.ENDS + 1] - 1] = 0
    v = torch.randn(M, R, d, generator=gen, dtype=F64).to(dtype).cuda()
    q = torch.randn(M, R, generator=gen, dtype=F64).to(dtype).cuda()
    return G, A_table.to(dtype).cuda().contiguous(), pattern.cuda(), ts, v, q, gen


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("d", [1, 3, 5, 7])
def test_kernel_is_the_batched_pattern_kernel_per_model_bit_for_bit(d, dtype):
    """out4[k], info2[k] are cgps_leg_loglik_batch_obs on model k's slices; P = 2, 4, 8 (obs_dim 1..3); the prior slot is
    the plain kernel's; a byte >= P reads entry P - 1."""
    M = 3
    plan = leg._BatchPlan(LENGTHS, "cuda")
    for P in (2, 4, 8):
        G, A_table, pattern, ts, v, q, gen = _kernel_case(d, dtype, M, P, 3000 + 10 * d + P)
        out, info = leg.leg_loglik_models_reductions_obs(ts, G, A_table, pattern, v, q, plan)
        assert out.shape == (M, len(LENGTHS), 4) and out.dtype == F64
        assert info.shape == (M, len(LENGTHS), 2) and info.dtype == torch.int32
        assert not bool(torch.isnan(out).any()) and int(info.abs().max()) == 0
        for k in range(M):
            o1, i1 = leg.leg_loglik_batch_reductions_obs(ts, G[k].contiguous(), A_table[k].contiguous(), pattern,
                                                         v[k].contiguous(), q[k].contiguous(), plan)
            assert torch.equal(out[k], o1), (P, k, (out[k] - o1).abs().max())
            assert torch.equal(info[k], i1), (P, k)
            plain, _ = leg.leg_loglik_batch_reductions(ts, G[k].contiguous(), A_table[k, P - 1].contiguous(), v[k].contiguous(),
                                                       q[k].contiguous(), plan)
            assert torch.equal(out[k, :, 2], plain[:, 2]), (P, k)
        # the clamp: bytes >= P are entry P - 1
        top = pattern == P - 1
        high = torch.where(top, torch.randint(P, 256, pattern.shape, generator=gen).to(torch.uint8).cuda(), pattern)
        assert int(top.sum()) > 0 and int(high.max()) >= P
        out2, info2 = leg.leg_loglik_models_reductions_obs(ts, G, A_table, high, v, q, plan)
        assert torch.equal(out2, out) and torch.equal(info2, info), P


# ---- the public call -------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("d", range(1, 9))
def test_against_one_masked_batched_call_per_model_every_rank(d, dtype):
    """Ranks 1..8 in both dtypes (d = 8 and fp64 d = 6 take the documented loop over the models); obs_dim 1..3; one series
    wholly unobserved, one without its first and last row, NaN in xs wherever it is not observed."""
    rtol = 1e-9 if dtype == F64 else 1e-3
    M = 3
    for obs in (1, 2, 3):
        ms = [mc.model(d, obs, dtype, 100 * d + obs + 7 * k) for k in range(M)]
        gen = torch.Generator().manual_seed(60 * d + obs)
        ts, xs = mc.ragged(LENGTHS, obs, gen, dtype)
        ob = mc.mask(LENGTHS, obs, gen, dead=mc.DEAD, ends=mc.ENDS)
        xs = mc.poisoned(xs, ob)
        out = leg.log_likelihood_models_observed(ms, ts, xs, torch.tensor(LENGTHS), observed=ob)
        assert out.shape == (M, len(LENGTHS)) and out.dtype == dtype
        ref = torch.stack([leg.log_likelihood_batch(m, ts, xs, LENGTHS, observed=ob) for m in ms])
        mc.assert_values(out, ref, rtol, "d=%d %s obs=%d" % (d, dtype, obs))
        assert float(out[:, mc.DEAD].abs().max()) <= rtol  # a series that observes nothing gives 0


@pytest.mark.gpu
def test_dense_padded_batch_with_a_tail_mask_is_the_ragged_call_on_the_true_lengths():
    ms = [mc.model(4, 2, F64, s) for s in (11, 12, 13)]
    true, n = [40, 17, 1, 33], 40
    gen = torch.Generator().manual_seed(5)
    ts, xs = mc.ragged([n] * len(true), 2, gen, F64)
    ob = mc.mask([n] * len(true), 2, gen)
    ts, xs, ob = ts.reshape(-1, n), xs.reshape(-1, n, 2), ob.reshape(-1, n, 2).clone()
    keep = [torch.arange(n) < t for t in true]
    for b, kp in enumerate(keep):
        ob[b, ~kp.cuda()] = False
    dense = leg.log_likelihood_models_observed(ms, ts, mc.poisoned(xs, ob), observed=ob)
    rag = leg.log_likelihood_models_observed(ms, torch.cat([ts[b, :t] for b, t in enumerate(true)]),
                                    torch.cat([xs[b, :t] for b, t in enumerate(true)]), true,
                                    observed=torch.cat([ob[b, :t] for b, t in enumerate(true)]))
    assert dense.shape == (3, 4)
    mc.assert_values(dense, rag, 1e-9, "dense padded against ragged")
    # whole-row flags [B, n] are the mask with every channel of the row
    rows = ob.all(-1)
    a = leg.log_likelihood_models_observed(ms, ts, xs, observed=rows)
    b = leg.log_likelihood_models_observed(ms, ts, xs, observed=rows.unsqueeze(-1).expand(-1, -1, 2))
    assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_everything_observed_is_the_call_without_a_mask(dtype):
    rtol = 1e-9 if dtype == F64 else 1e-3
    for obs in (1, 3):
        ms = [mc.model(5, obs, dtype, 20 + obs + k) for k in range(3)]
        gen = torch.Generator().manual_seed(7 + obs)
        ts, xs = mc.ragged(LENGTHS, obs, gen, dtype)
        a = leg.log_likelihood_models_observed(ms, ts, xs, LENGTHS, observed=torch.ones(xs.shape, dtype=torch.bool, device="cuda"))
        mc.assert_values(a, leg.log_likelihood_models(ms, ts, xs, LENGTHS), rtol, "all observed, obs=%d %s" % (obs, dtype))


DENSE_LENGTHS = [1, 5, 17, 40]


@functools.lru_cache(maxsize=None)
def _dense_reference(d, obs):
    """Three models, four series with _missref.leg_case's masks (first and last row missing, a run of four missing rows,
    the one-row series wholly unobserved), a random upstream gradient w[M, B]; the dense Gaussian of every (model,
    series), its gradients weighted and added up.  Computed once per (d, obs) and left unchanged."""
    M = 3
    models = [mr.leg_case(d, obs, 4, 900 + 10 * d + k)[0][:4] for k in range(M)]
    cases = [mr.leg_case(d, obs, n, 700 + 10 * d + n) for n in DENSE_LENGTHS]
    series = [(c[4], c[5], msk) for c, msk in cases]                   # (xs, ts, mask)
    w = torch.randn(M, len(DENSE_LENGTHS), generator=torch.Generator().manual_seed(d), dtype=F64)
    ll = torch.zeros(M, len(DENSE_LENGTHS), dtype=F64)
    gpar = [[torch.zeros_like(p) for p in mod] for mod in models]
    gxs = [torch.zeros_like(x) for x, _, _ in series]
    gts = [torch.zeros_like(t) for _, t, _ in series]
    for k, mod in enumerate(models):
        for b, (x, t, msk) in enumerate(series):
            if not bool(msk.any()):                     # no data: density 1, whatever the parameters (ll and gradients stay 0)
                continue
            val, grads = mr.leg_dense_value_and_grads(*mod, t, x, msk)
            ll[k, b] = val
            for acc, gp in zip(gpar[k], grads[:4]):
                acc += w[k, b] * gp
            gxs[b] += w[k, b] * grads[4]
            gts[b] += w[k, b] * grads[5]
    xs, ts = torch.cat([x for x, _, _ in series]), torch.cat([t for _, t, _ in series])
    return models, ts, xs, torch.cat([m for _, _, m in series]), w, ll, gpar, torch.cat(gxs), torch.cat(gts)


def test_dense_reference_cases_are_positive_definite_and_cover_the_masks():
    """(CPU) the reference's Cholesky went through at keep 0.6, the one-row series observes nothing and gives 0"""
    for d, obs in ((3, 2), (5, 1)):
        _, _, _, msk, _, ll, gpar, _, _ = _dense_reference(d, obs)
        assert bool(torch.isfinite(ll).all()) and float(ll[:, 0].abs().max()) == 0.0
        assert not bool(msk[0].any()) and 0.3 < float(msk.double().mean()) < 0.7
        assert all(bool(torch.isfinite(g).all()) for gp in gpar for g in gp)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["all", "NR_frozen", "model_1_only"])
@pytest.mark.parametrize("d,obs", [(3, 2), (5, 1)])
def test_values_and_gradients_against_the_dense_reference(d, obs, which):
    models, ts, xs, msk, w, ll, gpar, gxs, gts = _dense_reference(d, obs)
    train = []
    for k in range(len(models)):
        if which == "all":
            train.append((True, True, True, True))
        elif which == "NR_frozen":
            train.append((False, False, True, True))
        else:
            train.append((True, True, True, True) if k == 1 else (False, False, False, False))
    ms = [leg.LEGMatrices(*(p.clone().cuda().requires_grad_(r) for p, r in zip(mod, tr))) for mod, tr in zip(models, train)]
    ob = msk.cuda()
    t, x = ts.clone().cuda().requires_grad_(True), mc.poisoned(xs.cuda(), ob).requires_grad_(True)
    out = leg.log_likelihood_models_observed(ms, t, x, DENSE_LENGTHS, observed=ob)
    got = out.detach().cpu()
    mc.assert_values(got, ll, 1e-9, "values against the dense Gaussian")      # (every |ll| > 1 but the empty series' 0)
    (out * w.cuda()).sum().backward()
    for k, (m, tr) in enumerate(zip(ms, train)):
        for name, p, want, r in zip(("N", "R", "B", "Lambda"), (m.N, m.R, m.B, m.Lambda), gpar[k], tr):
            if r:
                mc.check_grad(p.grad, want, "d%s of model %d" % (name, k))
            else:
                assert p.grad is None, (name, k)
    mc.check_grad(x.grad, gxs, "dxs")                   # (with one model trainable xs and ts still see all three)
    mc.check_grad(t.grad, gts, "dts")


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [1, 2])
@pytest.mark.parametrize("obs", [1, 3])
def test_gradients_at_kernel_boundary_sizes_against_the_loop(obs, chunks, monkeypatch):
    """257 and 513 rows (rows per lane 1 -> 2 -> 3), two models at d = 5; then the same with the backward cut into two
    chunks of one model each.  rtol 1e-7, atol 1e-9.

    Gaps of at least 0.5, not 0.05: the bound is absolute, and at gaps from 0.05 it lies below the scatter of the
    reference itself.  Measured on an MI355X on these models and sizes with gaps from 0.05 (d/dts up to 29 .. 216 in
    size): one log_likelihood per series against the log_likelihood_batch loop -- both older than this call -- differ
    by 1.6e-9 .. 9.1e-9 in d/dts, the fully observed log_likelihood_models against its loop by 1.4e-9 .. 7.9e-9, and this
    call against the loop by 2.7e-9 .. 1.1e-8 (one chunk) and 1.5e-9 .. 7.5e-9 (two chunks); d/dN up to 7.9e-9 likewise.
    Every route factors a system of another size (one series, one model's batch, all models' batches), so the cyclic
    reduction pairs the rows differently; no route is closer to the others than they are to each other."""
    lengths = [257, 513]
    ms = [mc.model(5, obs, F64, s) for s in (41, 42)]
    gen = torch.Generator().manual_seed(43 + obs)
    ts, xs = mc.ragged(lengths, obs, gen, F64, gap0=0.5)
    ob = mc.mask(lengths, obs, gen, ends=1)
    w = torch.randn(2, 2, generator=gen, dtype=F64).cuda()
    if chunks == 2:
        monkeypatch.setattr(leg, "MODELS_BACKWARD_MAX_ROWS", sum(lengths))
    mc.compare_with_the_loop(ms, ts, mc.poisoned(xs, ob), lengths, w, ob)


@pytest.mark.gpu
def test_bit_identical_repeats_and_independent_of_other_models_series_and_unobserved_values():
    ms = [mc.model(5, 2, F64, s) for s in (3, 4)]
    lengths = [502, 33, 1, 129]
    gen = torch.Generator().manual_seed(6)
    ts, xs = mc.ragged(lengths, 2, gen, F64)
    ob = mc.mask(lengths, 2, gen, ends=0)
    a = leg.log_likelihood_models_observed(ms, ts, xs, lengths, observed=ob)
    assert torch.equal(a, leg.log_likelihood_models_observed(ms, ts, xs, lengths, observed=ob))
    # what the unobserved entries hold changes nothing
    assert torch.equal(a, leg.log_likelihood_models_observed(ms, ts, mc.poisoned(xs, ob), lengths, observed=ob))
    # other models before and after
    more = [mc.model(5, 2, F64, 8)] + ms + [mc.model(5, 2, F64, 9), mc.model(5, 2, F64, 10)]
    b = leg.log_likelihood_models_observed(more, ts, xs, lengths, observed=ob)
    assert torch.equal(b[1:3], a)
    # other series around them
    ts2, xs2 = mc.ragged([50, 700], 2, gen, F64)
    ob2 = mc.mask([50, 700], 2, gen)
    c = leg.log_likelihood_models_observed(ms, torch.cat([ts2[:50], ts, ts2[50:]]), torch.cat([xs2[:50], xs, xs2[50:]]),
                                  [50] + lengths + [700], observed=torch.cat([ob2[:50], ob, ob2[50:]]))
    assert torch.equal(c[:, 1:-1], a)
    # a model alone is its row
    assert torch.equal(leg.log_likelihood_models_observed(ms[1:], ts, xs, lengths, observed=ob)[0], a[1])


@pytest.mark.gpu
def test_repeated_time_stamp_names_its_model_and_series():
    ms = [mc.model(3, 2, F64, s) for s in (5, 6, 7)]
    lengths = [40, 300, 25, 60]
    gen = torch.Generator().manual_seed(8)
    ts, xs = mc.ragged(lengths, 2, gen, F64)
    ob = mc.mask(lengths, 2, gen)
    clean = leg.log_likelihood_models_observed(ms, ts, xs, lengths, observed=ob)
    bad = ts.clone()
    bad[40 + 300 + 11] = bad[40 + 300 + 10]                  # series 2, local rows 10 / 11: every model sees it
    with pytest.raises(cr.NotPSDError, match="model 0, series 2"):
        leg.log_likelihood_models_observed(ms, bad, xs, lengths, observed=ob)
    prev = cr.CHECK_POSITIVE_DEFINITE
    cr.CHECK_POSITIVE_DEFINITE = False
    try:
        out = leg.log_likelihood_models_observed(ms, bad, xs, lengths, observed=ob)
    finally:
        cr.CHECK_POSITIVE_DEFINITE = prev
    assert bool(torch.isnan(out[:, 2]).all())
    for b in (0, 1, 3):
        assert torch.equal(out[:, b], clean[:, b])


@pytest.mark.gpu
def test_a_series_above_batch_max_rows_takes_the_pair_kernel(monkeypatch):
    """BATCH_MAX_ROWS lowered to 64: the 301-row series goes through cgps_leg_mahal_logdet_pair_obs per model, the others
    through the one launch.  (Plans are cached by lengths: no other test uses these.)"""
    lengths = [31, 301, 47]
    ms = [mc.model(5, 2, F64, s) for s in (51, 52)]
    gen = torch.Generator().manual_seed(53)
    ts, xs = mc.ragged(lengths, 2, gen, F64)
    ob = mc.mask(lengths, 2, gen, ends=1)
    w = torch.randn(2, 3, generator=gen, dtype=F64).cuda()
    st = mc.starts(lengths)                               # (one series at a time: no plan of these lengths is made)
    ref = torch.stack([torch.stack([leg.log_likelihood(m, ts[a:e], xs[a:e], ob[a:e]) for a, e in zip(st[:-1], st[1:])])
                       for m in ms])
    monkeypatch.setattr(leg, "BATCH_MAX_ROWS", 64)
    plan = leg._cached_batch_plan(lengths, ts.device)
    assert plan.long == [1]
    out = leg.log_likelihood_models_observed(ms, ts, xs, lengths, observed=ob)
    mc.assert_values(out, ref, 1e-9, "pair kernel for the long series")
    mc.compare_with_the_loop(ms, ts, xs, lengths, w, ob)

"""leg.log_likelihood_models_observed(..., noise_var=): M LEG models over one batch of series with per-observation noise
variances (and missing observations), in one launch (cgps_leg_loglik_models_w: a basis and the rows' weights per
model).  Against cgps_leg_loglik_batch_w on every model's slices bit for bit, against a loop of
leg.log_likelihood_batch(observed=, noise_var=) over the models, and against the dense fp64 Gaussian of the observed
entries (_noiseref, no shared code)."""
import ctypes
import functools
import os

import pytest
import torch

import _modelscase as mc
import _noiseref as nr
from cyclic_gps import _hip, leg
import cyclic_gps.cyclic_reduction as cr

F64, F32 = torch.float64, torch.float32
LENGTHS = mc.BOUNDARY_LENGTHS


def _noise(lengths, obs, gen, dtype, per_row=False):
    """variances from [0, 2], [R, obs] or one per row [R]"""
    R = sum(lengths)
    return (2.0 * torch.rand((R,) if per_row else (R, obs), generator=gen, dtype=F64)).to(dtype).cuda()


# ---- argument handling and the C entry's checks (no GPU) -------------------------------------------------------------

def test_new_symbol_is_exported_and_declared():
    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert "cgps_leg_loglik_models_w" in _hip.exported_symbols() and hasattr(lib, "cgps_leg_loglik_models_w")
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cgps.h")
    assert "int cgps_leg_loglik_models_w(" in open(header).read()
    assert _hip.lib().cgps_version() == 320


def test_c_entry_checks_its_arguments_before_any_launch():
    lib = _hip.lib()
    fn = lib.cgps_leg_loglik_models_w
    fake = ctypes.c_void_p(256)
    # (ts, offsets, B, R, M, G, basis, Kb, weights, v, q, d, dtype, max_rows, out4, info2, stream)
    call = lambda B=2, R=10, M=3, Kb=3, d=5, dt=_hip.F64: fn(fake, fake, B, R, M, fake, fake, Kb, fake, None, None, d, dt,   # noqa: E731
                                                            4096, fake, fake, None)
    for M in (0, -1, 65536):
        assert call(M=M) == 1 and b"outside 1..65535" in lib.cgps_last_error()
    for Kb in (0, -1, 65):
        assert call(Kb=Kb) == 1 and b"outside 1..64" in lib.cgps_last_error()
    assert call(B=-1) == 1 and call(R=-1) == 1 and call(B=2 ** 31) == 1
    assert b"cgps_leg_loglik_models_w" in lib.cgps_last_error()
    for k in (0, 1, 5, 6, 8, 14, 15):                  # every pointer but v and q (null: zeros), one at a time
        args = [fake, fake, 2, 10, 3, fake, fake, 3, fake, None, None, 5, _hip.F64, 4096, fake, fake, None]
        args[k] = None
        assert fn(*args) == 1 and b"cgps_leg_loglik_models_w" in lib.cgps_last_error(), k
    for d, dt in ((8, _hip.F64), (8, _hip.F32), (6, _hip.F64)):
        assert call(d=d, dt=dt) == 3 and b"cgps_leg_loglik_models_w" in lib.cgps_last_error()
    assert call(d=9) == 3
    # an empty batch is no work and no error, whatever the pointers
    assert fn(None, None, 0, 0, 3, None, None, 3, None, None, None, 5, _hip.F64, 4096, None, None, None) == 0
    assert call(B=0, Kb=64, d=7, dt=_hip.F32) == 0


def test_noise_var_is_checked_as_the_batch_checks_it():
    ms = [mc.model(2, 2, F64, s, device="cpu") for s in (0, 1)]
    ts, xs = torch.zeros(3, 4, dtype=F64), torch.zeros(3, 4, 2, dtype=F64)
    for bad in (torch.ones(3, 4, 2, dtype=torch.int64), torch.ones(3, 4, dtype=torch.bool), [[0.5] * 4] * 3, 0.5):
        with pytest.raises(ValueError, match="floating"):
            leg.log_likelihood_models_observed(ms, ts, xs, noise_var=bad)
    for shape in ((3,), (12,), (12, 2), (3, 4, 2, 1), (3, 4, 1), (3, 4, 3), (3, 5), (3, 5, 2), (4, 4), (2, 4, 2)):
        with pytest.raises(ValueError, match="noise_var"):
            leg.log_likelihood_models_observed(ms, ts, xs, noise_var=torch.ones(shape, dtype=F64))
        with pytest.raises(ValueError, match="noise_var"):
            leg.log_likelihood_models_observed(ms, ts, xs, observed=torch.ones(3, 4, dtype=torch.bool),
                                      noise_var=torch.ones(shape, dtype=F64))
    with pytest.raises(ValueError, match="dense layout"):      # the layout's own errors come first, as without noise
        leg.log_likelihood_models_observed(ms, ts.reshape(-1), xs.reshape(-1, 2), noise_var=torch.ones(12, dtype=F64))
    ts, xs = torch.zeros(10, dtype=F64), torch.zeros(10, 2, dtype=F64)
    for shape in ((), (9,), (11,), (9, 2), (10, 1), (10, 3), (10, 2, 1), (2, 5), (2, 5, 2)):
        with pytest.raises(ValueError, match="noise_var"):
            leg.log_likelihood_models_observed(ms, ts, xs, [4, 6], noise_var=torch.ones(shape, dtype=F64))
    with pytest.raises(ValueError, match="sum"):
        leg.log_likelihood_models_observed(ms, ts, xs, [4, 5], noise_var=torch.ones(10, dtype=F64))


def test_empty_batch_with_noise_var_gives_one_empty_row_per_model():
    ms = [mc.model(3, 1, F64, s, device="cpu") for s in (0, 1, 2)]
    e = torch.zeros(0, dtype=F64)
    for s in (torch.zeros(0, dtype=F64), torch.zeros(0, 1, dtype=F64)):
        out = leg.log_likelihood_models_observed(ms, e, torch.zeros(0, 1, dtype=F64), [], noise_var=s)
        assert out.shape == (3, 0) and out.dtype == F64
        out = leg.log_likelihood_models_observed(ms, e, torch.zeros(0, 1, dtype=F64), [], observed=torch.zeros(0, dtype=torch.bool),
                                        noise_var=s)
        assert out.shape == (3, 0)
    out = leg.log_likelihood_models_observed(ms, torch.zeros(0, 7, dtype=F64), torch.zeros(0, 7, 1, dtype=F64),
                                    noise_var=torch.zeros(0, 7, dtype=F64))
    assert out.shape == (3, 0)


def test_wrapper_refuses_wrong_operands_before_any_launch():
    plan = leg._BatchPlan([4, 6], "cpu")
    G, v, q = torch.zeros(2, 3, 3, dtype=F64), torch.zeros(2, 10, 3, dtype=F64), torch.zeros(2, 10, dtype=F64)
    ts, basis = torch.zeros(10, dtype=F64), torch.zeros(2, 3, 3, 3, dtype=F64)
    with pytest.raises(ValueError, match="basis"):
        leg.leg_loglik_models_reductions_w(ts, G, torch.zeros(2, 65, 3, 3, dtype=F64), torch.zeros(2, 10, 65, dtype=F64), v, q, plan)
    with pytest.raises(ValueError, match="basis"):
        leg.leg_loglik_models_reductions_w(ts, G, basis[0], torch.zeros(2, 10, 3, dtype=F64), v, q, plan)
    with pytest.raises(ValueError, match="weights"):
        leg.leg_loglik_models_reductions_w(ts, G, basis, torch.zeros(10, 3, dtype=F64), v, q, plan)
    with pytest.raises(ValueError, match="dtype"):
        leg.leg_loglik_models_reductions_w(ts, G, basis.float(), torch.zeros(2, 10, 3, dtype=F32), v, q, plan)
    with pytest.raises(ValueError, match="device"):
        leg.leg_loglik_models_reductions_w(ts, G, basis, torch.zeros(2, 10, 3, dtype=F64), v, q, plan)


def test_rows_product_per_model_is_the_plain_product_on_both_sides_of_a_chunk():
    gen = torch.Generator().manual_seed(1)
    for R in (1, 7, 8, 9, 16, 21):
        a, b = torch.randn(3, R, 2, generator=gen, dtype=F64), torch.randn(3, R, 5, generator=gen, dtype=F64)
        want = torch.stack([a[k].T @ b[k] for k in range(3)])
        assert float((leg._rows_product_models(a, b, rows=8) - want).abs().max()) <= 1e-13


# ---- the kernel ------------------------------------------------------------------------------------------------------

def _kernel_case(d, dtype, M, Kb, seed):
    """Hand-built operands: generators of M models, Kb symmetric positive semi-definite basis blocks of rank 2 per model
    (non-negative weights keep K positive definite), weights from [0, 2] per model and row with all-zero rows where a
    series observes nothing or loses its ends, random v and q."""
    gen = torch.Generator().manual_seed(seed)
    G = torch.stack([mc.model(d, 1, dtype, seed + 17 * k).G for k in range(M)]).contiguous()
    Bs = torch.randn(M, Kb, d, 2, generator=gen, dtype=F64)
    basis = 0.5 * Bs @ Bs.transpose(-1, -2)
    ts, _ = mc.ragged(LENGTHS, 1, gen, dtype)
    st = mc.starts(LENGTHS)
    R = st[-1]
    weights = 2.0 * torch.rand(M, R, Kb, generator=gen, dtype=F64)
    weights[:, st[mc.DEAD]:st[mc.DEAD + 1]] = 0
    weights[:, st[mc.ENDS]] = 0
    weights[:, st[mc.ENDS + 1] - 1] = 0
    v = torch.randn(M, R, d, generator=gen, dtype=F64).to(dtype).cuda()
    q = torch.randn(M, R, generator=gen, dtype=F64).to(dtype).cuda()
    return G, basis.to(dtype).cuda().contiguous(), weights.to(dtype).cuda().contiguous(), ts, v, q


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("d", [1, 3, 5, 7])
def test_kernel_is_the_batched_weighted_kernel_per_model_bit_for_bit(d, dtype):
    """out4[k], info2[k] are cgps_leg_loglik_batch_w on model k's slices; Kb = 1, 3, 6 (obs_dim 1..3); the prior slot is
    the plain kernel's."""
    M = 3
    plan = leg._BatchPlan(LENGTHS, "cuda")
    for Kb in (1, 3, 6):
        G, basis, weights, ts, v, q = _kernel_case(d, dtype, M, Kb, 4000 + 10 * d + Kb)
        out, info = leg.leg_loglik_models_reductions_w(ts, G, basis, weights, v, q, plan)
        assert out.shape == (M, len(LENGTHS), 4) and out.dtype == F64
        assert info.shape == (M, len(LENGTHS), 2) and info.dtype == torch.int32
        assert not bool(torch.isnan(out).any()) and int(info.abs().max()) == 0
        for k in range(M):
            o1, i1 = leg.leg_loglik_batch_reductions_w(ts, G[k].contiguous(), basis[k].contiguous(), weights[k].contiguous(),
                                                       v[k].contiguous(), q[k].contiguous(), plan)
            assert torch.equal(out[k], o1), (Kb, k, (out[k] - o1).abs().max())
            assert torch.equal(info[k], i1), (Kb, k)
            plain, _ = leg.leg_loglik_batch_reductions(ts, G[k].contiguous(), basis[k, 0].contiguous(), v[k].contiguous(),
                                                       q[k].contiguous(), plan)
            assert torch.equal(out[k, :, 2], plain[:, 2]), (Kb, k)


# ---- the public call -------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("d", range(1, 9))
def test_against_one_noisy_batched_call_per_model_every_rank(d, dtype):
    """Ranks 1..8 in both dtypes (d = 8 and fp64 d = 6 take the documented loop over the models); obs_dim 1..3; with a
    mask (one series wholly unobserved, one without its first and last row, NaN in xs and noise_var wherever they are not
    observed) and, at obs_dim 2, without one and with one variance per row."""
    rtol = 1e-9 if dtype == F64 else 1e-3
    M = 3
    for obs in (1, 2, 3):
        ms = [mc.model(d, obs, dtype, 100 * d + obs + 7 * k) for k in range(M)]
        gen = torch.Generator().manual_seed(70 * d + obs)
        ts, xs = mc.ragged(LENGTHS, obs, gen, dtype)
        ob = mc.mask(LENGTHS, obs, gen, dead=mc.DEAD, ends=mc.ENDS)
        s = _noise(LENGTHS, obs, gen, dtype)
        cases = [("masked", mc.poisoned(xs, ob), ob, mc.poisoned(s, ob))]
        if obs == 2:
            cases += [("no mask", xs, None, s), ("per row", xs, None, _noise(LENGTHS, obs, gen, dtype, per_row=True))]
        for name, x, o, sv in cases:
            out = leg.log_likelihood_models_observed(ms, ts, x, torch.tensor(LENGTHS), observed=o, noise_var=sv)
            assert out.shape == (M, len(LENGTHS)) and out.dtype == dtype
            ref = torch.stack([leg.log_likelihood_batch(m, ts, x, LENGTHS, observed=o, noise_var=sv) for m in ms])
            mc.assert_values(out, ref, rtol, "d=%d %s obs=%d %s" % (d, dtype, obs, name))
            if o is not None:
                assert float(out[:, mc.DEAD].abs().max()) <= rtol      # a series that observes nothing gives 0


@pytest.mark.gpu
def test_dense_padded_batch_with_a_tail_mask_is_the_ragged_call_on_the_true_lengths():
    ms = [mc.model(4, 2, F64, s) for s in (11, 12, 13)]
    true, n = [40, 17, 1, 33], 40
    gen = torch.Generator().manual_seed(5)
    ts, xs = mc.ragged([n] * len(true), 2, gen, F64)
    ob = mc.mask([n] * len(true), 2, gen)
    s = _noise([n] * len(true), 2, gen, F64)
    ts, xs, s, ob = ts.reshape(-1, n), xs.reshape(-1, n, 2), s.reshape(-1, n, 2), ob.reshape(-1, n, 2).clone()
    for b, t in enumerate(true):
        ob[b, t:] = False
    dense = leg.log_likelihood_models_observed(ms, ts, mc.poisoned(xs, ob), observed=ob, noise_var=mc.poisoned(s, ob))
    cut = lambda a: torch.cat([a[b, :t] for b, t in enumerate(true)])   # noqa: E731
    rag = leg.log_likelihood_models_observed(ms, cut(ts), cut(xs), true, observed=cut(ob), noise_var=cut(s))
    assert dense.shape == (3, 4)
    mc.assert_values(dense, rag, 1e-9, "dense padded against ragged")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_zero_noise_and_everything_observed_is_the_call_without_either(dtype):
    rtol = 1e-9 if dtype == F64 else 1e-3
    for obs in (1, 3):
        ms = [mc.model(5, obs, dtype, 20 + obs + k) for k in range(3)]
        gen = torch.Generator().manual_seed(7 + obs)
        ts, xs = mc.ragged(LENGTHS, obs, gen, dtype)
        a = leg.log_likelihood_models_observed(ms, ts, xs, LENGTHS, observed=torch.ones(xs.shape, dtype=torch.bool, device="cuda"),
                                      noise_var=torch.zeros_like(xs))
        mc.assert_values(a, leg.log_likelihood_models(ms, ts, xs, LENGTHS), rtol, "no noise, obs=%d %s" % (obs, dtype))


DENSE_LENGTHS = [1, 5, 17, 40]


@functools.lru_cache(maxsize=None)
def _dense_reference(d, obs):
    """Three models, four series with _noiseref.leg_case's masks and variances (first and last row missing, a run of four
    missing rows, the one-row series wholly unobserved), a random upstream gradient w[M, B]; the dense Gaussian of every
    (model, series), its gradients weighted and added up.  Computed once per (d, obs) and left unchanged."""
    M = 3
    models = [nr.leg_case(d, obs, 4, 900 + 10 * d + k)[0][:4] for k in range(M)]
    series = [(c[4], c[5], c[6], msk) for c, msk in (nr.leg_case(d, obs, n, 700 + 10 * d + n) for n in DENSE_LENGTHS)]
    w = torch.randn(M, len(DENSE_LENGTHS), generator=torch.Generator().manual_seed(d), dtype=F64)
    ll = torch.zeros(M, len(DENSE_LENGTHS), dtype=F64)
    gpar = [[torch.zeros_like(p) for p in mod] for mod in models]
    gx = [[torch.zeros_like(a) for a in (x, t, s)] for x, t, s, _ in series]
    for k, mod in enumerate(models):
        for b, (x, t, s, msk) in enumerate(series):
            if not bool(msk.any()):                     # no data: density 1, whatever the parameters (ll and gradients stay 0)
                continue
            val, grads = nr.leg_dense_value_and_grads(*mod, t, x, s, msk)
            ll[k, b] = val
            for acc, gp in zip(gpar[k], grads[:4]):
                acc += w[k, b] * gp
            for acc, gp in zip(gx[b], grads[4:]):       # dxs, dts, ds
                acc += w[k, b] * gp
    cat = lambda i: torch.cat([sr[i] for sr in series])   # noqa: E731
    return (models, cat(1), cat(0), cat(2), cat(3), w, ll, gpar, torch.cat([g[0] for g in gx]),
            torch.cat([g[1] for g in gx]), torch.cat([g[2] for g in gx]))


def test_dense_reference_cases_are_positive_definite_and_cover_the_masks():
    """(CPU) the reference's Cholesky went through at keep 0.6, the one-row series observes nothing and gives 0"""
    for d, obs in ((3, 2), (5, 1)):
        _, _, _, _, msk, _, ll, gpar, _, _, gs = _dense_reference(d, obs)
        assert bool(torch.isfinite(ll).all()) and float(ll[:, 0].abs().max()) == 0.0
        assert not bool(msk[0].any()) and 0.3 < float(msk.double().mean()) < 0.7
        assert all(bool(torch.isfinite(g).all()) for gp in gpar for g in gp)
        assert float(gs[~msk].abs().max()) == 0.0 and float(gs[msk].abs().min()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["all", "NR_frozen", "model_1_only"])
@pytest.mark.parametrize("d,obs", [(3, 2), (5, 1)])
def test_values_and_gradients_against_the_dense_reference(d, obs, which):
    models, ts, xs, s, msk, w, ll, gpar, gxs, gts, gs = _dense_reference(d, obs)
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
    sv = mc.poisoned(s.cuda(), ob).requires_grad_(True)
    out = leg.log_likelihood_models_observed(ms, t, x, DENSE_LENGTHS, observed=ob, noise_var=sv)
    mc.assert_values(out.detach().cpu(), ll, 1e-9, "values against the dense Gaussian")   # (every |ll| > 1 but the empty series' 0)
    (out * w.cuda()).sum().backward()
    for k, (m, tr) in enumerate(zip(ms, train)):
        for name, p, want, r in zip(("N", "R", "B", "Lambda"), (m.N, m.R, m.B, m.Lambda), gpar[k], tr):
            if r:
                mc.check_grad(p.grad, want, "d%s of model %d" % (name, k))
            else:
                assert p.grad is None, (name, k)
    mc.check_grad(x.grad, gxs, "dxs")                   # (with one model trainable xs, ts and noise_var still see all three)
    mc.check_grad(t.grad, gts, "dts")
    mc.check_grad(sv.grad, gs, "dnoise_var")


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [1, 2])
@pytest.mark.parametrize("obs", [1, 3])
def test_gradients_at_kernel_boundary_sizes_against_the_loop(obs, chunks, monkeypatch):
    """257 and 513 rows (rows per lane 1 -> 2 -> 3), two models at d = 5, the gradient in noise_var included; then the same with the backward cut into two
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
    gen = torch.Generator().manual_seed(47 + obs)
    ts, xs = mc.ragged(lengths, obs, gen, F64, gap0=0.5)
    ob = mc.mask(lengths, obs, gen, ends=1)
    s = _noise(lengths, obs, gen, F64)
    w = torch.randn(2, 2, generator=gen, dtype=F64).cuda()
    if chunks == 2:
        monkeypatch.setattr(leg, "MODELS_BACKWARD_MAX_ROWS", sum(lengths))
    mc.compare_with_the_loop(ms, ts, mc.poisoned(xs, ob), lengths, w, ob, mc.poisoned(s, ob))


@pytest.mark.gpu
def test_bit_identical_repeats_and_independent_of_other_models_series_and_unobserved_values():
    ms = [mc.model(5, 2, F64, s) for s in (3, 4)]
    lengths = [502, 33, 1, 129]
    gen = torch.Generator().manual_seed(6)
    ts, xs = mc.ragged(lengths, 2, gen, F64)
    ob = mc.mask(lengths, 2, gen, ends=0)
    s = _noise(lengths, 2, gen, F64)
    a = leg.log_likelihood_models_observed(ms, ts, xs, lengths, observed=ob, noise_var=s)
    assert torch.equal(a, leg.log_likelihood_models_observed(ms, ts, xs, lengths, observed=ob, noise_var=s))
    # what the unobserved entries of xs and noise_var hold changes nothing
    assert torch.equal(a, leg.log_likelihood_models_observed(ms, ts, mc.poisoned(xs, ob), lengths, observed=ob,
                                                    noise_var=mc.poisoned(s, ob)))
    # other models before and after
    more = [mc.model(5, 2, F64, 8)] + ms + [mc.model(5, 2, F64, 9), mc.model(5, 2, F64, 10)]
    b = leg.log_likelihood_models_observed(more, ts, xs, lengths, observed=ob, noise_var=s)
    assert torch.equal(b[1:3], a)
    # other series around them
    ts2, xs2 = mc.ragged([50, 700], 2, gen, F64)
    ob2, s2 = mc.mask([50, 700], 2, gen), _noise([50, 700], 2, gen, F64)
    around = lambda u, w: torch.cat([w[:50], u, w[50:]])   # noqa: E731
    c = leg.log_likelihood_models_observed(ms, around(ts, ts2), around(xs, xs2), [50] + lengths + [700], observed=around(ob, ob2),
                                  noise_var=around(s, s2))
    assert torch.equal(c[:, 1:-1], a)
    # a model alone is its row
    assert torch.equal(leg.log_likelihood_models_observed(ms[1:], ts, xs, lengths, observed=ob, noise_var=s)[0], a[1])


@pytest.mark.gpu
def test_repeated_time_stamp_names_its_model_and_series():
    ms = [mc.model(3, 2, F64, s) for s in (5, 6, 7)]
    lengths = [40, 300, 25, 60]
    gen = torch.Generator().manual_seed(8)
    ts, xs = mc.ragged(lengths, 2, gen, F64)
    ob = mc.mask(lengths, 2, gen)
    s = _noise(lengths, 2, gen, F64)
    clean = leg.log_likelihood_models_observed(ms, ts, xs, lengths, observed=ob, noise_var=s)
    bad = ts.clone()
    bad[40 + 300 + 11] = bad[40 + 300 + 10]                  # series 2, local rows 10 / 11: every model sees it
    with pytest.raises(cr.NotPSDError, match="model 0, series 2"):
        leg.log_likelihood_models_observed(ms, bad, xs, lengths, observed=ob, noise_var=s)
    prev = cr.CHECK_POSITIVE_DEFINITE
    cr.CHECK_POSITIVE_DEFINITE = False
    try:
        out = leg.log_likelihood_models_observed(ms, bad, xs, lengths, observed=ob, noise_var=s)
    finally:
        cr.CHECK_POSITIVE_DEFINITE = prev
    assert bool(torch.isnan(out[:, 2]).all())
    for b in (0, 1, 3):
        assert torch.equal(out[:, b], clean[:, b])


@pytest.mark.gpu
def test_a_series_above_batch_max_rows_takes_the_pair_kernel(monkeypatch):
    """BATCH_MAX_ROWS lowered to 64: the 302-row series goes through cgps_leg_mahal_logdet_pair_w per model, the others
    through the one launch.  (Plans are cached by lengths: no other test uses these.)"""
    lengths = [31, 302, 47]
    ms = [mc.model(5, 2, F64, s) for s in (51, 52)]
    gen = torch.Generator().manual_seed(53)
    ts, xs = mc.ragged(lengths, 2, gen, F64)
    ob = mc.mask(lengths, 2, gen, ends=1)
    s = _noise(lengths, 2, gen, F64)
    w = torch.randn(2, 3, generator=gen, dtype=F64).cuda()
    st = mc.starts(lengths)                               # (one series at a time: no plan of these lengths is made)
    ref = torch.stack([torch.stack([leg.log_likelihood(m, ts[a:e], xs[a:e], ob[a:e], s[a:e]) for a, e in zip(st[:-1], st[1:])])
                       for m in ms])
    monkeypatch.setattr(leg, "BATCH_MAX_ROWS", 64)
    plan = leg._cached_batch_plan(lengths, ts.device)
    assert plan.long == [1]
    out = leg.log_likelihood_models_observed(ms, ts, xs, lengths, observed=ob, noise_var=s)
    mc.assert_values(out, ref, 1e-9, "pair kernel for the long series")
    mc.compare_with_the_loop(ms, ts, xs, lengths, w, ob, s)

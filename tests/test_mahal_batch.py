"""cr.mahal_and_det_batch: many block-tridiagonal systems in one launch (cgps_mahal_logdet_batch, csrc/cgps_tile_batch.h)
and its per-system adjoint (cgps_mahal_logdet_adjoint_seg, csrc/cgps_level.h).

CPU: argument checks of the Python entry and of the two C entries.  GPU: the reference's recorded values, every (d, dtype)
at the chunk boundaries of the kernel against the fp64 oracle, dense = ragged, independence of the systems, failures,
long systems, gradients against a dense fp64 reference, graph capture.  Tolerances are those of tests/test_hip_parity.py
(values) and tests/test_gradients.py (gradients) for the same inputs."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _gradref
import _util
from oracle import cr_oracle as O
import cyclic_gps.cyclic_reduction as cr
from cyclic_gps import _hip

F64, F32 = torch.float64, torch.float32
SIZES = [1, 2, 3, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1000]      # around NT = 128 / 256 lanes, C = 1 -> 2 -> 3 -> 4
TOL = {F64: dict(rtol=1e-9, atol=1e-10), F32: dict(rtol=3e-4, atol=3e-4)}


def _cat(systems, dtype=F64, device="cuda", cut=0.0):
    """Ragged operands of [(Rs, Os, b)]: concatenated Rs, Os (the entries between systems hold `cut`), x and the lengths."""
    Rs = torch.cat([s[0] for s in systems])
    x = torch.cat([s[2] for s in systems])
    d = Rs.shape[1]
    parts = []
    for i, s in enumerate(systems):
        parts.append(s[1])
        if i + 1 < len(systems):
            parts.append(torch.full((1, d, d), cut, dtype=s[1].dtype))
    Os = torch.cat(parts)
    return Rs.to(dtype).to(device), Os.to(dtype).to(device), x.to(dtype).to(device), [s[0].shape[0] for s in systems]


def _np(t):
    return t.detach().cpu().numpy()


# ---- CPU --------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_the_library_is_touched(monkeypatch):
    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_hip, "lib", no_lib)
    monkeypatch.setattr(cr, "_device", no_lib)
    d = 3
    R, Oo, x = torch.zeros(7, d, d, dtype=F64), torch.zeros(6, d, d, dtype=F64), torch.zeros(7, d, dtype=F64)
    with pytest.raises(ValueError, match="length -1"):
        cr.mahal_and_det_batch(R, Oo, x, lengths=[8, -1])
    with pytest.raises(ValueError, match="sum to 6"):
        cr.mahal_and_det_batch(R, Oo, x, lengths=[2, 4])
    with pytest.raises(ValueError):                                   # lengths of the wrong rank
        cr.mahal_and_det_batch(R, Oo, x, lengths=[[3, 4]])
    with pytest.raises(ValueError):
        cr.mahal_and_det_batch(R, Oo, x, lengths=torch.tensor([[3, 4]]))
    with pytest.raises(ValueError):
        cr.mahal_and_det_batch(R, Oo, x, lengths=torch.tensor([3.0, 4.0]))
    with pytest.raises(ValueError, match="ragged layout wants Rs"):   # operands of the wrong rank
        cr.mahal_and_det_batch(R.reshape(1, 7, d, d), Oo, x, lengths=[3, 4])
    with pytest.raises(ValueError, match="dense layout wants Rs"):
        cr.mahal_and_det_batch(R, Oo, x)
    with pytest.raises(ValueError, match="wants Os"):                 # one block per system missing: the dense Os
        cr.mahal_and_det_batch(R, Oo[:5], x, lengths=[3, 4])
    with pytest.raises(ValueError, match="wants Os"):
        cr.mahal_and_det_batch(R.reshape(1, 7, d, d), Oo.reshape(1, 6, d, d)[:, :5], x.reshape(1, 7, d))
    with pytest.raises(ValueError, match="wants x"):
        cr.mahal_and_det_batch(R, Oo, x[:6], lengths=[3, 4])
    with pytest.raises(TypeError, match="one dtype"):
        cr.mahal_and_det_batch(R, Oo.float(), x, lengths=[3, 4])
    with pytest.raises(TypeError, match="one dtype"):
        cr.mahal_and_det_batch(R, Oo, x.float(), lengths=[3, 4])
    with pytest.raises(TypeError):
        cr.mahal_and_det_batch(R.long(), Oo.long(), x.long(), lengths=[3, 4])
    with pytest.raises(ValueError, match="outside 1..8"):
        cr.mahal_and_det_batch(torch.zeros(2, 9, 9), torch.zeros(1, 9, 9), None, lengths=[2])


def _batch_call(lib, Rs=1, Os=1, x=1, offsets=1, B=1, packed=0, d=3, dtype=1, out=1, info=1):
    # fake non-null pointers: every case below returns before anything is dereferenced or launched
    p = lambda v: ctypes.c_void_p(4096 * v) if v else None   # noqa: E731
    return lib.cgps_mahal_logdet_batch(p(Rs), p(Os), p(x), p(offsets), B, packed, d, dtype, 4096, p(out), p(info), None)


def _adjoint_call(lib, Sd=1, So=1, w=1, seg=1, N=4, B=2, d=3, dtype=1, gm=1, gl=1):
    p = lambda v: ctypes.c_void_p(4096 * v) if v else None   # noqa: E731
    return lib.cgps_mahal_logdet_adjoint_seg(p(Sd), p(So), p(w), p(seg), N, B, d, dtype, p(gm), p(gl), None)


def test_c_entries_reject_null_pointers():
    lib = _hip.lib()
    for name in ("Rs", "Os", "offsets", "out", "info"):
        assert _batch_call(lib, **{name: 0}) == 1, name
        assert b"cgps_mahal_logdet_batch" in lib.cgps_last_error()
    assert _batch_call(lib, B=-1) == 1
    for name in ("Sd", "So", "w", "seg", "gm", "gl"):
        assert _adjoint_call(lib, **{name: 0}) == 1, name
        assert b"cgps_mahal_logdet_adjoint_seg" in lib.cgps_last_error()
    assert _adjoint_call(lib, N=0) == 1 and _adjoint_call(lib, B=0) == 1


def test_c_entries_reject_unsupported_sizes_and_types():
    lib = _hip.lib()
    assert _batch_call(lib, d=9) == 3 and _batch_call(lib, dtype=7) == 3
    assert _adjoint_call(lib, d=9) == 3 and _adjoint_call(lib, dtype=7) == 3
    # the block sizes the batched kernel is not built for: the caller reduces each system on its own
    assert _batch_call(lib, d=8, dtype=0) == 3 and _batch_call(lib, d=8, dtype=1) == 3 and _batch_call(lib, d=6, dtype=1) == 3


def test_c_entry_with_no_systems_is_ok():
    lib = _hip.lib()
    for d, dtype in ((1, 0), (3, 1), (5, 1), (6, 0), (7, 1)):
        assert _batch_call(lib, B=0, d=d, dtype=dtype) == 0
        assert _batch_call(lib, B=0, d=d, dtype=dtype, x=0) == 0


def test_symbols_are_declared():
    assert {"cgps_mahal_logdet_batch", "cgps_mahal_logdet_adjoint_seg"} <= set(_hip.exported_symbols())
    assert cr.BATCH_MAX_ROWS == 4096


# ---- GPU --------------------------------------------------------------------------------------------------------------
def _golden_batch(cases):
    gs = [_util.load_golden(p) for p in cases]
    systems = [tuple(torch.from_numpy(g[k]) for k in ("Rs", "Os", "v")) for g in gs]
    return systems, np.stack([g["mad"] for g in gs])


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["d3", "d1", "d5_twice"])
def test_reference_recorded_values(which):
    all_cases = _util.golden_cr_cases()
    if which == "d5_twice":
        paths = [p for d, n, p in all_cases if (d, n) == (5, 502)] * 2
        assert len(paths) == 2
    else:
        paths = [p for d, n, p in all_cases if d == int(which[1:])]
        assert len(paths) >= 2
    systems, mad = _golden_batch(paths)
    Rs, Os, x, lengths = _cat(systems)
    m, ld = cr.mahal_and_det_batch(Rs, Os, x, lengths=lengths)
    assert m.shape == (len(paths),) and ld.shape == (len(paths),) and m.dtype == F64 and m.is_cuda
    np.testing.assert_allclose(_np(m), mad[:, 0], rtol=1e-10, atol=1e-11)
    np.testing.assert_allclose(_np(ld), mad[:, 1], rtol=1e-10, atol=1e-11)


@functools.lru_cache(maxsize=None)
def _boundary_case(d, dtype, lead_one_row=False):
    """The systems of SIZES rounded to dtype (as fp64 CPU tensors), the oracle's fp64 values on those rounded inputs and
    the closed-form log-determinants.  Built once per (d, dtype) and left unchanged."""
    sizes = ([1] if lead_one_row else []) + SIZES
    systems, ref, logdets = [], [], []
    for i, n in enumerate(sizes):
        Rs, Os, b, _, logdet = _util.conditioned_system(n, d, seed=500 + 31 * n + d + i)
        sysr = tuple(t.to(dtype).to(F64) for t in (Rs, Os, b))
        m, ld = O.mahal_and_det(*sysr)
        systems.append(sysr)
        ref.append([float(m), float(ld)])
        logdets.append(logdet)
    return tuple(systems), np.array(ref), np.array(logdets)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_every_block_size_at_chunk_boundaries(d, dtype):
    """One ragged batch whose lengths straddle the lane counts and the rows-per-lane steps; d = 8 and fp64 d = 6 take the
    per-system fallback and are held to the same tolerances."""
    systems, ref, logdets = _boundary_case(d, dtype)
    Rs, Os, x, lengths = _cat(systems, dtype)
    m, ld = cr.mahal_and_det_batch(Rs, Os, x, lengths=lengths)
    assert m.dtype == dtype and ld.dtype == dtype and m.shape == (len(SIZES),)
    tol = TOL[dtype]
    np.testing.assert_allclose(_np(m).astype(np.float64), ref[:, 0], err_msg="mahal", **tol)
    np.testing.assert_allclose(_np(ld).astype(np.float64), ref[:, 1], err_msg="logdet against the oracle", **tol)
    np.testing.assert_allclose(_np(ld).astype(np.float64), logdets, err_msg="logdet against the closed form", **tol)


@pytest.mark.gpu
def test_odd_row_offsets():
    """The same batch behind a one-row system, 5 x 5 fp64 blocks: the other half of the systems now starts at an odd
    row, 8 bytes off a 16-byte boundary (the 1 000-row and the 511-row system among them)."""
    systems, ref, logdets = _boundary_case(5, F64, True)
    Rs, Os, x, lengths = _cat(systems)
    odd = [n for i, n in enumerate(lengths) if sum(lengths[:i]) % 2 == 1]
    assert lengths[0] == 1 and {1000, 511, 255, 127} <= set(odd)
    m, ld = cr.mahal_and_det_batch(Rs, Os, x, lengths=lengths)
    np.testing.assert_allclose(_np(m), ref[:, 0], **TOL[F64])
    np.testing.assert_allclose(_np(ld), ref[:, 1], **TOL[F64])
    np.testing.assert_allclose(_np(ld), logdets, **TOL[F64])


def _equal_systems(B, n, d, dtype, seed=0):
    return [tuple(t.to(dtype).to(F64) for t in _util.conditioned_system(n, d, seed=900 + seed + b)[:3]) for b in range(B)]


@pytest.mark.gpu
@pytest.mark.parametrize("d,dtype,n", [(5, F64, 37), (4, F32, 130), (3, F64, 1), (8, F64, 9)],
                         ids=["d5f64", "d4f32", "d3f64_one_row", "d8f64_fallback"])
def test_dense_equals_ragged_bitwise(d, dtype, n):
    B = 5
    systems = _equal_systems(B, n, d, dtype)
    Rs, Os, x, lengths = _cat(systems, dtype)
    Rd = torch.stack([s[0] for s in systems]).to(dtype).cuda()
    Od = torch.stack([s[1] for s in systems]).to(dtype).cuda()
    xd = torch.stack([s[2] for s in systems]).to(dtype).cuda()
    assert Od.shape == (B, n - 1, d, d)
    mr, lr = cr.mahal_and_det_batch(Rs, Os, x, lengths=lengths)
    md, ldd = cr.mahal_and_det_batch(Rd, Od, xd)
    assert torch.equal(mr, md) and torch.equal(lr, ldd)
    for args, kw in (((Rs, Os, None), dict(lengths=lengths)), ((Rd, Od, None), {})):
        m0, l0 = cr.mahal_and_det_batch(*args, **kw)
        assert torch.equal(l0, lr) and torch.equal(m0, torch.zeros_like(m0)) and m0.shape == (B,)
    # against the one-system entry point
    for b in range(B):
        m1, l1 = cr.mahal_and_det(Rd[b], Od[b], xd[b])
        np.testing.assert_allclose([float(mr[b]), float(lr[b])], [float(m1), float(l1)], **TOL[dtype])


@pytest.mark.gpu
def test_cpu_tensors_and_empty_systems():
    systems = _equal_systems(3, 6, 2, F64)
    Rs, Os, x, lengths = _cat(systems, device="cpu")
    m, ld = cr.mahal_and_det_batch(Rs, Os, x, lengths=lengths)
    assert m.device.type == "cpu" and ld.device.type == "cpu"
    mg, lg = cr.mahal_and_det_batch(Rs.cuda(), Os.cuda(), x.cuda(), lengths=torch.tensor(lengths))
    assert torch.equal(m, mg.cpu()) and torch.equal(ld, lg.cpu())
    # zero-length systems: (0, 0), the others unchanged
    lz = [0, lengths[0], 0, 0, lengths[1], lengths[2], 0]
    mz, lzd = cr.mahal_and_det_batch(Rs.cuda(), Os.cuda(), x.cuda(), lengths=lz)
    keep = [1, 4, 5]
    assert torch.equal(mz[keep], mg) and torch.equal(lzd[keep], lg)
    gone = [0, 2, 3, 6]
    assert float(mz[gone].abs().max()) == 0.0 and float(lzd[gone].abs().max()) == 0.0
    e = cr.mahal_and_det_batch(Rs[:0].cuda(), Os[:0].cuda(), x[:0].cuda(), lengths=[])
    assert e[0].shape == (0,) and e[1].shape == (0,)


@pytest.mark.gpu
@pytest.mark.parametrize("d,dtype", [(5, F64), (4, F64), (3, F32), (7, F64)], ids=["d5f64", "d4f64", "d3f32", "d7f64"])
def test_systems_are_independent(d, dtype):
    sizes = [3, 130, 1, 64, 257, 20]
    systems = [tuple(t.to(dtype).to(F64) for t in _util.conditioned_system(n, d, seed=40 + n)[:3]) for n in sizes]
    Rs, Os, x, lengths = _cat(systems, dtype)
    m, ld = cr.mahal_and_det_batch(Rs, Os, x, lengths=lengths)
    assert bool(torch.isfinite(m).all()) and bool(torch.isfinite(ld).all())
    # repeated calls
    m2, ld2 = cr.mahal_and_det_batch(Rs, Os, x, lengths=lengths)
    assert torch.equal(m, m2) and torch.equal(ld, ld2)
    # the entries of Os between systems are never read
    Rn, On, xn, _ = _cat(systems, dtype, cut=float("nan"))
    assert int(torch.isnan(On).flatten(1).any(1).sum()) == len(sizes) - 1
    mn, ldn = cr.mahal_and_det_batch(Rn, On, xn, lengths=lengths)
    assert torch.equal(m, mn) and torch.equal(ld, ldn)
    # a permutation of the batch permutes the results
    perm = [4, 2, 0, 5, 1, 3]
    Rp, Op, xp, lp = _cat([systems[i] for i in perm], dtype, cut=float("nan"))
    mp, ldp = cr.mahal_and_det_batch(Rp, Op, xp, lengths=lp)
    assert torch.equal(mp, m[perm]) and torch.equal(ldp, ld[perm])
    # one system alone, first, last and at an odd offset
    k, seen = 4, set()
    for order in ([k], [k, 0, 1], [0, 1, k], [2, k, 3], [0, 2, k, 5]):
        at = order.index(k)
        seen.add((at == 0, at == len(order) - 1, sum(sizes[i] for i in order[:at]) % 2))
        Ra, Oa, xa, la = _cat([systems[i] for i in order], dtype)
        ma, lda = cr.mahal_and_det_batch(Ra, Oa, xa, lengths=la)
        assert float(ma[at]) == float(m[k]) and float(lda[at]) == float(ld[k]), order
    assert {(True, True, 0), (True, False, 0), (False, True, 1), (False, False, 1), (False, False, 0)} <= seen


@pytest.mark.gpu
@pytest.mark.parametrize("d,dtype", [(5, F64), (4, F32), (8, F32)], ids=["d5f64", "d4f32", "d8f32_fallback"])
def test_an_indefinite_system_fails_alone(d, dtype, monkeypatch):
    sizes = [5, 300, 17, 129]
    systems = [tuple(t.to(dtype).to(F64) for t in _util.conditioned_system(n, d, seed=70 + n)[:3]) for n in sizes]
    bad, row = 2, 6
    broken = [tuple(t.clone() for t in s) for s in systems]
    broken[bad][0][row] = -broken[bad][0][row]
    Rs, Os, x, lengths = _cat(broken, dtype)
    with pytest.raises(cr.NotPSDError, match="system %d" % bad) as ei:
        cr.mahal_and_det_batch(Rs, Os, x, lengths=lengths)
    assert ei.value.system == bad and 0 <= ei.value.row < sizes[bad]
    monkeypatch.setattr(cr, "CHECK_POSITIVE_DEFINITE", False)
    m, ld = cr.mahal_and_det_batch(Rs, Os, x, lengths=lengths)
    assert bool(torch.isnan(m[bad])) and bool(torch.isnan(ld[bad]))
    good = [i for i in range(len(sizes)) if i != bad]
    Rg, Og, xg, lg = _cat([systems[i] for i in good], dtype)
    mg, ldg = cr.mahal_and_det_batch(Rg, Og, xg, lengths=lg)
    assert torch.equal(m[good], mg) and torch.equal(ld[good], ldg)


@pytest.mark.gpu
@pytest.mark.parametrize("d,dtype", [(5, F64), (3, F64), (4, F32)], ids=["d5f64", "d3f64", "d4f32"])
def test_long_systems_take_the_one_system_kernel(d, dtype, monkeypatch):
    monkeypatch.setattr(cr, "BATCH_MAX_ROWS", 64)
    sizes = [10, 65, 64, 200]                 # 65 and 200 are long; the last one starts at row 139, an odd one
    systems = [tuple(t.to(dtype).to(F64) for t in _util.conditioned_system(n, d, seed=300 + n)[:3]) for n in sizes]
    ref = np.array([[float(v) for v in O.mahal_and_det(*s)] for s in systems])
    Rs, Os, x, lengths = _cat(systems, dtype, cut=float("nan"))
    m, ld = cr.mahal_and_det_batch(Rs, Os, x, lengths=lengths)
    np.testing.assert_allclose(_np(m).astype(np.float64), ref[:, 0], **TOL[dtype])
    np.testing.assert_allclose(_np(ld).astype(np.float64), ref[:, 1], **TOL[dtype])
    m0, ld0 = cr.mahal_and_det_batch(Rs, Os, None, lengths=lengths)
    assert float(m0.abs().max()) == 0.0
    np.testing.assert_allclose(_np(ld0).astype(np.float64), ref[:, 1], **TOL[dtype])


# ---- gradients --------------------------------------------------------------------------------------------------------
GRAD_LENGTHS = [1, 2, 37, 257]
A_W = [0.7, 0.0, -1.1, 0.4]          # d loss / d mahal_b: distinct, system 1 takes no part in the loss
C_W = [-1.3, 0.0, 0.6, 2.1]          # d loss / d logdet_b


@functools.lru_cache(maxsize=None)
def _grad_case(d, dtype):
    """Systems rounded to dtype, and the fp64 dense reference of the loss's gradients (dR symmetrised), concatenated."""
    systems = [tuple(t.to(dtype).to(F64) for t in _util.conditioned_system(n, d, seed=1200 + 13 * n + d)[:3])
               for n in GRAD_LENGTHS]
    gR, gO, gx = [], [], []
    for b, (Rs, Os, y) in enumerate(systems):
        _, mR, mO, my = _gradref.dense_value_and_grads("mahal", Rs, Os, y)
        _, lR, lO, _ = _gradref.dense_value_and_grads("logdet", Rs, Os, y)
        gR.append(A_W[b] * mR + C_W[b] * lR)
        gO.append(A_W[b] * mO + C_W[b] * lO)
        gx.append(A_W[b] * my)
        if b + 1 < len(systems):
            gO.append(torch.zeros(1, d, d, dtype=F64))
    return tuple(systems), torch.cat(gR), torch.cat(gO), torch.cat(gx)


def _check(got, want, dtype, what):
    """tests/test_gradients.py::_check"""
    want = want.detach().to("cpu", F64)
    got = torch.zeros_like(want) if got is None else got.detach().to("cpu", F64)
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    scale = float(want.abs().max()) if want.numel() else 0.0
    if dtype == F64:
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-7, atol=1e-10 * scale, err_msg=what)
    else:
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=2e-5 * scale + 1e-30, err_msg=what)


def _loss(m, ld):
    a = torch.tensor(A_W, dtype=m.dtype, device=m.device)
    c = torch.tensor(C_W, dtype=m.dtype, device=m.device)
    return (a * m).sum() + (c * ld).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("d,dtype", [(3, F64), (5, F64), (4, F32), (8, F64)], ids=["d3f64", "d5f64", "d4f32", "d8f64"])
def test_gradients_against_dense_reference(d, dtype):
    systems, rR, rO, rx = _grad_case(d, dtype)
    Rs, Os, x, lengths = _cat(systems, dtype, cut=float("nan"))
    cuts = torch.isnan(Os).flatten(1).any(1)
    assert int(cuts.sum()) == len(lengths) - 1
    R, Oo, y = (t.clone().requires_grad_(True) for t in (Rs, Os, x))
    m, ld = cr.mahal_and_det_batch(R, Oo, y, lengths=lengths)
    gR, gO, gy = torch.autograd.grad(_loss(m, ld), (R, Oo, y))
    _check(_gradref.sym(gR), rR, dtype, "dR")
    _check(gO, rO, dtype, "dO")
    _check(gy, rx, dtype, "dx")
    assert float(gO[cuts].abs().max()) == 0.0                       # exactly zero, whatever the entry held
    s1 = slice(lengths[0], lengths[0] + lengths[1])                  # the system outside the loss
    assert float(gR[s1].abs().max()) == 0.0 and float(gy[s1].abs().max()) == 0.0
    # each input alone
    y1 = x.clone().requires_grad_(True)
    m, ld = cr.mahal_and_det_batch(Rs, Os, y1, lengths=lengths)
    (g1,) = torch.autograd.grad(_loss(m, ld), (y1,))
    _check(g1, rx, dtype, "dx alone")
    R1 = Rs.clone().requires_grad_(True)
    m, ld = cr.mahal_and_det_batch(R1, Os, x, lengths=lengths)
    (g2,) = torch.autograd.grad(_loss(m, ld), (R1,))
    _check(_gradref.sym(g2), rR, dtype, "dR alone")
    # the log-determinants alone
    R3, O3 = Rs.clone().requires_grad_(True), Os.clone().requires_grad_(True)
    m, ld = cr.mahal_and_det_batch(R3, O3, None, lengths=lengths)
    g3R, g3O = torch.autograd.grad((torch.tensor(C_W, dtype=dtype, device="cuda") * ld).sum(), (R3, O3))
    ldR, ldO = [], []
    for b, (Rb, Ob, yb) in enumerate(systems):
        _, lR, lO, _ = _gradref.dense_value_and_grads("logdet", Rb, Ob, yb)
        ldR.append(C_W[b] * lR)
        ldO.append(C_W[b] * lO)
        if b + 1 < len(systems):
            ldO.append(torch.zeros(1, d, d, dtype=F64))
    _check(_gradref.sym(g3R), torch.cat(ldR), dtype, "dR, x = None")
    _check(g3O, torch.cat(ldO), dtype, "dO, x = None")


@pytest.mark.gpu
def test_dense_layout_gradients_equal_the_ragged_ones():
    B, n, d = 4, 9, 3
    systems = _equal_systems(B, n, d, F64, seed=50)
    Rs, Os, x, lengths = _cat(systems, cut=5.0)
    w = torch.tensor([0.3, -0.8, 1.7, 0.5], dtype=F64, device="cuda")
    R, Oo, y = (t.clone().requires_grad_(True) for t in (Rs, Os, x))
    m, ld = cr.mahal_and_det_batch(R, Oo, y, lengths=lengths)
    gR, gO, gy = torch.autograd.grad((w * m).sum() - (w * ld).sum(), (R, Oo, y))
    Rd = torch.stack([s[0] for s in systems]).cuda().requires_grad_(True)
    Od = torch.stack([s[1] for s in systems]).cuda().requires_grad_(True)
    xd = torch.stack([s[2] for s in systems]).cuda().requires_grad_(True)
    m, ld = cr.mahal_and_det_batch(Rd, Od, xd)
    hR, hO, hy = torch.autograd.grad((w * m).sum() - (w * ld).sum(), (Rd, Od, xd))
    assert hR.shape == Rd.shape and hO.shape == Od.shape and hy.shape == xd.shape
    assert torch.equal(hR.reshape(B * n, d, d), gR) and torch.equal(hy.reshape(B * n, d), gy)
    keep = torch.ones(B * n - 1, dtype=torch.bool)
    keep[torch.arange(1, B) * n - 1] = False
    assert torch.equal(hO.reshape(-1, d, d), gO[keep.cuda()]) and float(gO[~keep.cuda()].abs().max()) == 0.0


# ---- graph capture ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_dense_forward_is_capturable_in_a_graph():
    B, n, d = 6, 130, 5
    systems = _equal_systems(B, n, d, F64, seed=20)
    Rd = torch.stack([s[0] for s in systems]).cuda()
    Od = torch.stack([s[1] for s in systems]).cuda()
    xd = torch.stack([s[2] for s in systems]).cuda()
    eager = cr.mahal_and_det_batch(Rd, Od, xd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cr.mahal_and_det_batch(Rd, Od, xd)            # (loads the code object before the capture)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = cr.mahal_and_det_batch(Rd, Od, xd)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
    # new values in the same buffers, replayed
    other = _equal_systems(B, n, d, F64, seed=21)
    Rd.copy_(torch.stack([s[0] for s in other]))
    Od.copy_(torch.stack([s[1] for s in other]))
    xd.copy_(torch.stack([s[2] for s in other]))
    g.replay()
    torch.cuda.synchronize()
    eager2 = cr.mahal_and_det_batch(Rd, Od, xd)
    assert torch.equal(out[0], eager2[0]) and torch.equal(out[1], eager2[1])
    assert not torch.equal(eager2[0], eager[0])

"""Drop-in for the reference's ``cyclic_gps/cyclic_reduction.py`` on MI355X.

Same names, argument names and return structures as the reference module
(reference file:line cited per function).  The path -- ``decompose_step``,
``decompose``, ``mahal_and_det``, ``halfsolve``, ``backhalfsolve``, ``solve``,
``det``, ``mahal``, ``inverse_blocks`` and their gradients -- runs in hand-written
HIP kernels for gfx950 reached through the C ABI of ``include/cgps.h``
(``_hip.py`` is the ctypes binding); PyTorch only owns the device memory and the
stream.  The six small banded-product helpers of the reference's surface
(``UU_T, Ux, U_Tx, SigU, UtV_diags, interleave``, :15-200) are NOT kernels of
this library: inside the path they are fused into the kernels above, and as
stand-alone names they are batched torch products on whatever device their
arguments live on.

* Inputs may live on the GPU (zero-copy) or on the CPU (they are staged to the
  current GPU and results are returned on the CPU, so the reference's own
  CPU-tensor tests run unchanged on a GPU box).  There is no CPU fallback: with
  no GPU or no ``libcgps.so`` the functions raise.
* ``decompose`` returns an indexable 4-tuple ``(ms, Ds, Fs, Gs)`` like the
  reference; the per-level tensors are views into three packed device buffers
  (``decomp.packed``) that the solve kernels use directly.
* ``ms`` stays a CPU int64 tensor (``np.array(ms)`` is used by callers,
  reference tests/test_cyclic_reduction.py:210).
"""
import ctypes

import numpy as np  # noqa: F401  (the reference's star-import exposes np and torch)
import torch

from . import _hip

JITTER = None  # reference :13 (passed to psd_safe_cholesky there; no jitter retry here)

try:  # raise the caller's own exception classes when gpytorch is installed
    from gpytorch.utils.errors import NanError, NotPSDError  # type: ignore
except Exception:  # pragma: no cover
    class NotPSDError(RuntimeError):
        """A diagonal block was not positive definite."""

    class NanError(RuntimeError):
        """The blocks handed in hold NaN (what psd_safe_cholesky raises in the reference, :227,306,429)."""

# Set to False to skip the device->host read of the `info` word after a
# factorisation (removes one stream synchronisation per call).  Nothing raises then:
# mahal_and_det returns NaN for both scalars on a block that is not positive definite, and a
# factor carries the NaNs of the failed square root.
CHECK_POSITIVE_DEFINITE = True


# ----------------------------------------------------------------------------
# plumbing
# ----------------------------------------------------------------------------
def _device():
    if not torch.cuda.is_available():
        raise _hip.CgpsError("no GPU visible: the cyclic-reduction kernels need an MI355X (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _stage(t, dtype=None):
    """Contiguous GPU tensor for t on a 16-byte boundary, which is what include/cgps.h asks of every array of blocks or
    vectors (copying from the CPU when needed; a contiguous view that starts off the boundary, such as Rs[1:] of odd-sized
    blocks, is copied to fresh memory, so that the Python surface keeps taking any view)."""
    if t.device.type != "cuda":
        t = t.to(_device())
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return _aligned16(t.contiguous())


def _aligned16(t):
    """t, or a copy of it when its first byte is not on a 16-byte boundary (a slice of odd-sized blocks at an odd row:
    the kernels read blocks and vectors 16 bytes at a time, and the library refuses such a pointer)."""
    return t.clone() if t.numel() and t.data_ptr() % 16 else t


def _back(t, like):
    return t if like.device.type == "cuda" else t.to(like.device)


def _check_blocks(Rs, Os):
    if Rs.dim() != 3 or Os.dim() != 3:
        raise TypeError("Rs and Os must be [num_blocks, block_dim, block_dim] tensors")
    if Rs.shape[1] != Rs.shape[2] or (Os.shape[0] > 0 and tuple(Os.shape[1:]) != tuple(Rs.shape[1:])):
        raise TypeError("block_dim mismatch between Rs %s and Os %s" % (tuple(Rs.shape), tuple(Os.shape)))
    assert Rs.shape[0] == Os.shape[0] + 1          # reference :223
    _hip.dtype_code(Rs.dtype)


def _raise_if_not_pd(info, *blocks):
    """The reference's error behaviour at its psd_safe_cholesky calls: NanError when the operands hold NaN,
    NotPSDError otherwise (its jitter-and-retry in between is not reproduced).  `blocks` are looked at only
    on the failure path."""
    if CHECK_POSITIVE_DEFINITE:
        bad = int(info.item())
        if bad != 0:
            for t in blocks:
                nan = int(torch.isnan(t).sum().item()) if t is not None and t.numel() else 0
                if nan:
                    raise NanError("%d of %d elements of the %s tensor are NaN." % (nan, t.numel(), tuple(t.shape)))
            err = NotPSDError("block row %d is not positive definite" % (bad - 1))
            err.row = bad - 1         # (for callers that name the row in terms of their own: leg.insample_posterior_batch)
            raise err


class CRDecomp(tuple):
    """(ms, Ds, Fs, Gs) exactly as the reference returns it (:309), plus the packed
    device buffers the per-level lists are views of."""

    def __new__(cls, ms, Ds, Fs, Gs, packed=None, like=None):
        self = super().__new__(cls, (ms, Ds, Fs, Gs))
        self.packed = packed      # (Dp, Fp, Gp) on the GPU, or None
        self.like = like          # tensor whose device the results should follow
        self.inputs = None        # (Rs, Os) when they require grad (set by decompose)
        return self


def _views(Dp, Fp, Gp, N):
    ms, offD, offF, offG = _hip.level_layout(N)
    L = len(ms)

    def cut(P, off, count):                      # one split call instead of one slice per level
        sizes = [off[i + 1] - off[i] for i in range(count)]
        return list(P[:off[count]].split(sizes)) if count else []
    return torch.tensor(ms, dtype=torch.int64), cut(Dp, offD, L), cut(Fp, offF, L - 1), cut(Gp, offG, L - 1)


def _packed(decomp):
    """(Dp, Fp, Gp, N, d, like) for any decomp: ours, or a plain tuple of lists."""
    if isinstance(decomp, CRDecomp) and decomp.packed is not None:
        Dp, Fp, Gp = decomp.packed
        return Dp, Fp, Gp, int(decomp[0][0]), Dp.shape[-1], decomp.like
    ms, Ds, Fs, Gs = decomp
    like = Ds[0]
    d = like.shape[-1]
    N = int(ms[0])
    dev = _device()
    Dp = torch.cat([_stage(t) for t in Ds], dim=0)
    pad = torch.zeros((1, d, d), dtype=like.dtype, device=dev)
    Fp = torch.cat([_stage(t) for t in Fs] + [pad], dim=0)
    Gp = torch.cat([_stage(t) for t in Gs] + [pad], dim=0)
    return Dp, Fp, Gp, N, d, like


# ----------------------------------------------------------------------------
# factorisation
# ----------------------------------------------------------------------------
def decompose_step(Rs, Os):
    """One reduction level -> (n, D, F, G), (Rs', Os')   (reference :203-259).  No autograd graph."""
    _check_blocks(Rs, Os)
    n, d = Rs.shape[0], Rs.shape[1]
    if n < 2:
        raise ValueError("decompose_step needs at least two diagonal blocks")
    R, O = _stage(Rs), _stage(Os)
    dev, dt = R.device, R.dtype
    new = lambda k: torch.empty((k, d, d), dtype=dt, device=dev)  # noqa: E731
    D, F, G, Rn, On = new((n + 1) // 2), new(n // 2), new((n - 1) // 2), new(n // 2), new(n // 2 - 1)
    info = torch.empty(1, dtype=torch.int32, device=dev)
    _hip.check(_hip.lib().cgps_decompose_step(
        _hip.ptr(R), _hip.ptr(O), n, d, _hip.dtype_code(dt), _hip.ptr(D), _hip.ptr(F), _hip.ptr(G),
        _hip.ptr(Rn), _hip.ptr(On), _hip.ptr(info), _hip.stream_ptr()))
    _raise_if_not_pd(info, R, O)
    b = lambda t: _back(t, Rs)  # noqa: E731
    return (n, b(D), b(F), b(G)), (b(Rn), b(On))


def _needs_grad(*ts):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def decompose(Rs, Os):
    """Full cyclic-reduction factorisation -> (ms, Ds, Fs, Gs)   (reference :287-309).

    The factor tensors themselves are plain (non-differentiable) device buffers; when Rs / Os
    require grad the returned decomp remembers them, and det(decomp) / solve(decomp, y) /
    mahal(decomp, y) differentiate with respect to them analytically (see _DetFn, _SolveFn).
    halfsolve, backhalfsolve and inverse_blocks of the factor build no autograd graph."""
    dec = _decompose_raw(Rs.detach(), Os.detach())
    if _needs_grad(Rs, Os):
        dec.inputs = (Rs, Os)
    return dec


def _decompose_raw(Rs, Os):
    _check_blocks(Rs, Os)
    N, d = Rs.shape[0], Rs.shape[1]
    R, O = _stage(Rs), _stage(Os)
    dev, dt = R.device, R.dtype
    Dp = torch.empty((N, d, d), dtype=dt, device=dev)
    Fp = torch.empty((N, d, d), dtype=dt, device=dev)
    Gp = torch.empty((N, d, d), dtype=dt, device=dev)
    info = torch.empty(1, dtype=torch.int32, device=dev)
    ws, nbytes = _hip.workspace(N, d, dt, _hip.OP_DECOMPOSE, dev)
    _hip.check(_hip.lib().cgps_decompose(
        _hip.ptr(R), _hip.ptr(O), N, d, _hip.dtype_code(dt), _hip.ptr(Dp), _hip.ptr(Fp), _hip.ptr(Gp),
        _hip.ptr(ws), nbytes, _hip.ptr(info), _hip.stream_ptr()))
    _raise_if_not_pd(info, R, O)
    ms, Ds, Fs, Gs = _views(Dp, Fp, Gp, N)
    if Rs.device.type != "cuda":
        Ds, Fs, Gs = ([_back(t, Rs) for t in lst] for lst in (Ds, Fs, Gs))
    return CRDecomp(ms, Ds, Fs, Gs, packed=(Dp, Fp, Gp), like=Rs)


def decompose_solve(Rs, Os, y):
    """(decompose(Rs, Os), solve(decomp, y)) in one call: what compute_insample_posterior does first
    (reference models.py:288-292: decompose, then solve), with the forward substitution of y riding along in the
    first pass of the factorisation -- the forward sweep never reads 7/8 of the factor (cgps_decompose_solve).
    An addition to the reference's surface (its callers that factor and solve together can switch to it);
    y: [N, d].  When Rs, Os or y require grad (and grad mode is on) it returns (decompose(Rs, Os), solve(decomp, y)),
    so x is differentiable in all three; otherwise one fused call that builds no autograd graph."""
    _check_blocks(Rs, Os)
    N, d = Rs.shape[0], Rs.shape[1]
    if _needs_grad(Rs, Os, y):
        dec = decompose(Rs, Os)
        return dec, solve(dec, y.reshape(N, d)).reshape(y.shape)
    R, O = _stage(Rs.detach()), _stage(Os.detach())
    dev, dt = R.device, R.dtype
    v = _stage(y.detach()).to(dt).reshape(N, d).contiguous()
    Dp, Fp, Gp = (torch.empty((N, d, d), dtype=dt, device=dev) for _ in range(3))
    xcrr = torch.empty((N, d), dtype=dt, device=dev)
    x = torch.empty((N, d), dtype=dt, device=dev)
    info = torch.empty(1, dtype=torch.int32, device=dev)
    ws, nbytes = _hip.workspace(N, d, dt, _hip.OP_DECOMPOSE_SOLVE, dev)
    _hip.check(_hip.lib().cgps_decompose_solve(
        _hip.ptr(R), _hip.ptr(O), _hip.ptr(v), N, d, _hip.dtype_code(dt), _hip.ptr(Dp), _hip.ptr(Fp), _hip.ptr(Gp),
        _hip.ptr(xcrr), _hip.ptr(x), _hip.ptr(ws), nbytes, _hip.ptr(info), _hip.stream_ptr()))
    _raise_if_not_pd(info, R, O)
    ms, Ds, Fs, Gs = _views(Dp, Fp, Gp, N)
    if Rs.device.type != "cuda":
        Ds, Fs, Gs = ([_back(t, Rs) for t in lst] for lst in (Ds, Fs, Gs))
    return CRDecomp(ms, Ds, Fs, Gs, packed=(Dp, Fp, Gp), like=Rs), _back(x.reshape(y.shape), y)


def mahal_and_det(Rs, Os, x):
    """(x^T J^-1 x, log|J|) in one fused sweep, factor not kept   (reference :380-438).
    Differentiable in Rs, Os and x (the reference trains through it, models.py:367-381)."""
    if _needs_grad(Rs, Os, x):
        return _MahalLogdetFn.apply(Rs, Os, x)
    return _mahal_and_det(Rs, Os, x, levelwise=False)


# ----------------------------------------------------------------------------
# analytic adjoints (checked against the reference's autograd in
# tests/test_oracle.py::test_oracle_gradients_match_reference_autograd).  With w = J^-1 x and
# Sig = J^-1:   m = x^T J^-1 x : dm/dx = 2w, dm/dR_i = -w_i w_i^T, dm/dO_i = -2 w_{i+1} w_i^T
#               l = log|J|     : dl/dR_i = Sig_ii, dl/dO_i = 2 Sig_{i+1,i}
#               s = u^T J^-1 y : with a = J^-1 u: ds/dy = a, ds/dR_i = -sym(a_i w_i^T),
#                                ds/dO_i = -(a_{i+1} w_i^T + w_{i+1} a_i^T)
# Every backward is solves and selected-inverse blocks on the same HIP kernels.
# ----------------------------------------------------------------------------
def _outer(a, b):
    return a.unsqueeze(-1) * b.unsqueeze(-2)


def _pair(a, b):
    """sum over the right-hand-side columns of a_c b_c^T per block row: [N, d] or [N, d, ...] -> [N, d, d]"""
    if a.dim() == 2:
        return _outer(a, b)
    m = a.shape[2:].numel()              # explicit: a -1 is ambiguous for zero rows (the off-diagonal terms at N = 1)
    return a.reshape(a.shape[0], a.shape[1], m) @ b.reshape(b.shape[0], b.shape[1], m).transpose(-1, -2)


class _MahalLogdetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Rs, Os, x):
        ctx.save_for_backward(Rs, Os, x)
        return _mahal_and_det(Rs.detach(), Os.detach(), x.detach(), levelwise=False)

    @staticmethod
    def backward(ctx, gm, gl):
        Rs, Os, x = ctx.saved_tensors
        need_blocks = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        gR = gO = None
        # factor and solve together: the forward substitution rides along in the factorisation (decompose_solve)
        dec, w = decompose_solve(Rs, Os, x.reshape(Rs.shape[0], Rs.shape[1]))
        if need_blocks:
            gR, gO = inverse_blocks(dec)
        if need_blocks:
            # gR = gl Sigma_diag - gm w w^T, gO = 2 (gl Sigma_off - gm w[1:] w[:-1]^T), written over
            # the blocks inverse_blocks just produced (one pass instead of ten element-wise kernels)
            if gR.is_cuda:
                N, d = gR.shape[0], gR.shape[1]
                wd = w.to(gR.dtype).contiguous()
                g2 = torch.stack([gm.reshape(()).to(gR.dtype), gl.reshape(()).to(gR.dtype)]).to(gR.device)
                _hip.check(_hip.lib().cgps_mahal_logdet_adjoint(
                    _hip.ptr(gR), _hip.ptr(gO), _hip.ptr(wd), N, d, _hip.dtype_code(gR.dtype),
                    _hip.ptr(g2[0:1]), _hip.ptr(g2[1:2]), _hip.stream_ptr()))
            else:       # blocks handed in as CPU tensors: the results were staged back to the host
                gR = gl * gR - gm * _outer(w, w)
                gO = 2 * (gl * gO - gm * _outer(w[1:], w[:-1]))
        return gR, gO, (2 * gm * w).reshape(x.shape)


class _DetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Rs, Os, dec):
        ctx.dec = dec
        return _det_raw(dec)

    @staticmethod
    def backward(ctx, g):
        Sd, So = inverse_blocks(ctx.dec)
        return g * Sd, 2 * g * So, None


class _SolveFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Rs, Os, y, dec):
        w = _solve_raw(dec, y.detach())
        ctx.dec = dec
        ctx.save_for_backward(w)
        return w

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        a = _solve_raw(ctx.dec, g.contiguous())
        gR = gO = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            aw = _pair(a, w)
            gR = -0.5 * (aw + aw.transpose(-1, -2))
            gO = -(_pair(a[1:], w[:-1]) + _pair(w[1:], a[:-1]))
        return gR, gO, a, None


def _mahal_and_det(Rs, Os, x, levelwise):
    _check_blocks(Rs, Os)
    N, d = Rs.shape[0], Rs.shape[1]
    R, O = _stage(Rs), _stage(Os)
    dev, dt = R.device, R.dtype
    v = _stage(x, dt).reshape(N, d)
    out = torch.empty(2, dtype=torch.float64, device=dev)
    info = torch.empty(1, dtype=torch.int32, device=dev)
    ws, nbytes = _hip.workspace(N, d, dt, _hip.OP_MAHAL_LOGDET, dev)
    fn = _hip.lib().cgps_mahal_logdet_levelwise if levelwise else _hip.lib().cgps_mahal_logdet
    _hip.check(fn(_hip.ptr(R), _hip.ptr(O), _hip.ptr(v), N, d, _hip.dtype_code(dt), _hip.ptr(ws), nbytes,
                  _hip.ptr(out), _hip.ptr(info), _hip.stream_ptr()))
    _raise_if_not_pd(info, R, O)
    res = _back(out.to(dt), Rs)
    return res[0], res[1]


# ----------------------------------------------------------------------------
# many independent systems at once (an addition to the reference's surface)
# ----------------------------------------------------------------------------
BATCH_MAX_ROWS = 4096
"""Systems longer than this are reduced by ``cgps_mahal_logdet`` (several workgroups per system) instead of the one
workgroup per system of ``cgps_mahal_logdet_batch``; their values go into their slots all the same."""


class _MahalBatchPlan:
    """What the lengths of a ragged batch fix on the host, as device tensors: row offsets, the system of every row and
    the coupling blocks that lie between two systems.  Cached by ``leg._cached_batch_plan`` (caches of its own)."""
    plans, captured = {}, {}

    def __init__(self, lengths, device):
        off = [0]
        for n in lengths:
            off.append(off[-1] + n)
        B, R = len(lengths), off[-1]
        self.offsets = torch.tensor(off, dtype=torch.int64).to(device, non_blocking=True)
        self.seg = torch.repeat_interleave(torch.arange(B, dtype=torch.int32),
                                           torch.tensor(lengths, dtype=torch.int64)).to(device, non_blocking=True)
        self.cuts = torch.tensor(sorted({s - 1 for s in off[1:-1] if 0 < s < R}), dtype=torch.int64).to(device, non_blocking=True)


class _BatchLayout:
    """The two input layouts of mahal_and_det_batch behind one face.  Dense: B systems of n rows, Os[B, n-1] (the
    kernel's os_packed = 1); offsets and row indices are made on the device, nothing is uploaded.  Ragged: the
    concatenated arrays and host-side lengths; the entries of Os between two systems belong to nobody."""

    def __init__(self, dense, lengths, d, dtype, shapes):
        self.dense, self.lengths, self.d, self.dtype, self.shapes = dense, lengths, d, dtype, shapes
        self.B, self.R = len(lengths), sum(lengths)
        self.n = lengths[0] if dense and lengths else 0
        self._plan = self._starts = None

    def plan(self, dev):
        if self._plan is None:
            from . import leg            # (leg imports this module: not at import time)
            self._plan = leg._cached_batch_plan(self.lengths, dev, make=_MahalBatchPlan)
        return self._plan

    def offsets(self, dev):
        if self.dense:
            return torch.arange(0, (self.B + 1) * self.n, self.n, dtype=torch.int64, device=dev)   # (n >= 1: R > 0)
        return self.plan(dev).offsets

    def seg(self, dev):
        """int32 [R]: the system of each row"""
        if self.dense:
            return torch.arange(self.R, dtype=torch.int32, device=dev).div(self.n, rounding_mode="floor")
        return self.plan(dev).seg

    def start(self, b):
        """(first row, first coupling block) of system b in the arrays handed to the kernel"""
        if self.dense:
            return b * self.n, b * (self.n - 1)
        if self._starts is None:
            self._starts = [0]
            for n in self.lengths:
                self._starts.append(self._starts[-1] + n)
        return self._starts[b], self._starts[b]

    def concatenated_Os(self, O):
        """Os [R-1, d, d] of the block-diagonal concatenation: the caller's coupling blocks, zero between systems."""
        d = self.d
        if self.dense:
            Oc = O.new_zeros(self.B, self.n, d, d)
            Oc[:, :self.n - 1] = O.reshape(self.B, self.n - 1, d, d)
            return Oc.reshape(self.R, d, d)[:self.R - 1]
        Oc = O.clone()
        cuts = self.plan(O.device).cuts
        if cuts.numel():
            Oc.index_fill_(0, cuts, 0)
        return Oc

    def caller_Os(self, So):
        """The other way round, for a gradient [R-1, d, d] that is zero between systems."""
        d = self.d
        if self.dense:
            pad = torch.cat([So, So.new_zeros(1, d, d)], dim=0).reshape(self.B, self.n, d, d)
            return pad[:, :self.n - 1].contiguous()
        return So


def _batch_layout(Rs, Os, x, lengths):
    """Checks the arguments of mahal_and_det_batch and describes them; raises before the library is touched."""
    for name, t in (("Rs", Rs), ("Os", Os)) + ((("x", x),) if x is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a tensor" % name)
    if Rs.dtype not in (torch.float32, torch.float64):
        raise TypeError("cyclic reduction supports float32 / float64 blocks, got %s" % Rs.dtype)
    if Os.dtype != Rs.dtype or (x is not None and x.dtype != Rs.dtype):
        raise TypeError("Rs, Os and x must share one dtype, got %s, %s and %s"
                        % (Rs.dtype, Os.dtype, None if x is None else x.dtype))
    if lengths is None:
        if Rs.dim() != 4 or Rs.shape[2] != Rs.shape[3]:
            raise ValueError("dense layout wants Rs[B, n, d, d], got %s (pass lengths for the ragged layout)" % (tuple(Rs.shape),))
        B, n, d = Rs.shape[0], Rs.shape[1], Rs.shape[2]
        if tuple(Os.shape) != (B, max(n - 1, 0), d, d):
            raise ValueError("dense layout wants Os[%d, %d, %d, %d], got %s" % (B, max(n - 1, 0), d, d, tuple(Os.shape)))
        if x is not None and tuple(x.shape) != (B, n, d):
            raise ValueError("dense layout wants x[%d, %d, %d], got %s" % (B, n, d, tuple(x.shape)))
        lens, dense = [int(n)] * B, True
    else:
        if isinstance(lengths, torch.Tensor):
            if lengths.is_cuda or lengths.dim() != 1 or lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
                raise ValueError("lengths must be host data: a sequence or a 1-d CPU integer tensor")
            lengths = lengths.tolist()
        try:
            lens = [int(n) for n in lengths]
        except TypeError:
            raise ValueError("lengths must be a flat sequence of integers")
        if any(int(a) != a for a in lengths):
            raise ValueError("lengths must be integers")
        if Rs.dim() != 3 or Rs.shape[1] != Rs.shape[2]:
            raise ValueError("ragged layout wants Rs[sum(lengths), d, d], got %s" % (tuple(Rs.shape),))
        R, d = Rs.shape[0], Rs.shape[1]
        bad = [b for b, n in enumerate(lens) if n < 0]
        if bad:
            raise ValueError("system %d has length %d" % (bad[0], lens[bad[0]]))
        if sum(lens) != R:
            raise ValueError("lengths sum to %d rows, Rs has %d" % (sum(lens), R))
        if tuple(Os.shape) != (max(R - 1, 0), d, d):
            raise ValueError("ragged layout wants Os[%d, %d, %d] (the concatenated system's), got %s"
                             % (max(R - 1, 0), d, d, tuple(Os.shape)))
        if x is not None and tuple(x.shape) != (R, d):
            raise ValueError("ragged layout wants x[%d, %d], got %s" % (R, d, tuple(x.shape)))
        dense = False
    if not 1 <= d <= 8:
        raise ValueError("block size d=%d outside 1..8" % d)
    return _BatchLayout(dense, lens, int(d), Rs.dtype, (tuple(Rs.shape), tuple(Os.shape), None if x is None else tuple(x.shape)))


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _mahal_batch_raw(R, O, v, lay):
    """([B, 2] fp64 {mahal, logdet}, [B] int32 info) of staged, flattened operands: R [R, d, d], O the caller's coupling
    blocks flattened to [., d, d], v [R, d] or None.  One launch of cgps_mahal_logdet_batch; systems it leaves out (longer
    than BATCH_MAX_ROWS; every system at d = 8 and fp64 d = 6) go through cgps_mahal_logdet on the same stream, each into
    its own slot.  Nothing is read on the host."""
    dev, dt, d, B = R.device, R.dtype, lay.d, lay.B
    out = torch.zeros(B, 2, dtype=torch.float64, device=dev)
    info = torch.zeros(B, dtype=torch.int32, device=dev)
    if lay.R == 0:
        return out, info
    dtc = _hip.dtype_code(dt)
    with torch.cuda.device(dev):
        rc = _hip.lib().cgps_mahal_logdet_batch(
            _hip.ptr(R), _hip.ptr(O if O.numel() else R),       # (one-row systems only: no coupling block is read)
            _hip.ptr(v), _hip.ptr(lay.offsets(dev)), B, 1 if lay.dense else 0, d, dtc, BATCH_MAX_ROWS,
            _hip.ptr(out), _hip.ptr(info), _hip.stream_ptr())
        if rc == 3:      # CGPS_ERR_UNSUPPORTED: a block size the batched kernel is not built for
            singles = [b for b, n in enumerate(lay.lengths) if n >= 1]
        else:
            _hip.check(rc)
            singles = [b for b, n in enumerate(lay.lengths) if n > BATCH_MAX_ROWS]
        for b in singles:
            n = lay.lengths[b]
            s, so = lay.start(b)
            Rb, Ob = _aligned16(R[s:s + n]), _aligned16(O[so:so + n - 1])
            vb = _aligned16(v[s:s + n]) if v is not None else torch.zeros(n, d, dtype=dt, device=dev)
            ws, nbytes = _hip.workspace(n, d, dt, _hip.OP_MAHAL_LOGDET, dev)
            _hip.check(_hip.lib().cgps_mahal_logdet(
                _hip.ptr(Rb), _hip.ptr(Ob), _hip.ptr(vb), n, d, dtc, _hip.ptr(ws), nbytes, _hip.ptr(out[b]),
                _hip.ptr(info[b:b + 1]), _hip.stream_ptr()))
    return out, info


def _mahal_and_det_batch(Rs, Os, x, lay):
    d = lay.d
    R = _stage(Rs).reshape(-1, d, d)
    O = _stage(Os).reshape(-1, d, d)
    v = None if x is None else _stage(x).reshape(-1, d)
    out, info = _mahal_batch_raw(R, O, v, lay)
    if CHECK_POSITIVE_DEFINITE and lay.B and not _capturing():     # (a capture cannot read info: NaN marks the slot)
        bad = info.cpu()
        rows = torch.nonzero(bad).flatten().tolist()
        if rows:
            b = rows[0]
            err = NotPSDError("batch: system %d: a block near its row %d is not positive definite" % (b, int(bad[b]) - 1))
            err.system, err.row = b, int(bad[b]) - 1
            raise err
    res = _back(out.to(lay.dtype), Rs)
    return res[:, 0].contiguous(), res[:, 1].contiguous()


class _BatchMahalLogdetFn(torch.autograd.Function):
    """Forward: the batched reduction (one launch).  Backward: the concatenated system of all systems, which is block
    diagonal (the coupling blocks at the cuts set to zero): decompose_solve + inverse_blocks once, then one launch of
    the per-system adjoint kernel with every system's own upstream gradients (cgps_mahal_logdet_adjoint_seg)."""

    @staticmethod
    def forward(ctx, Rs, Os, x, lay):
        ctx.lay = lay
        ctx.save_for_backward(Rs, Os, x)
        return _mahal_and_det_batch(Rs.detach(), Os.detach(), None if x is None else x.detach(), lay)

    @staticmethod
    def backward(ctx, gm, gl):
        Rs, Os, x = ctx.saved_tensors
        lay, d = ctx.lay, ctx.lay.d
        need_R, need_O, need_x = ctx.needs_input_grad[:3]
        need_x = need_x and x is not None
        if lay.R == 0:
            z = lambda t, need: torch.zeros_like(t) if need else None   # noqa: E731
            return z(Rs, need_R), z(Os, need_O), (z(x, need_x) if x is not None else None), None
        R = _stage(Rs.detach()).reshape(-1, d, d)
        dev, dt = R.device, R.dtype
        Oc = lay.concatenated_Os(_stage(Os.detach()).reshape(-1, d, d))
        g_m, g_l = _stage(gm.detach(), dt), _stage(gl.detach(), dt)
        gR = gO = gx = None
        with torch.cuda.device(dev):
            if x is None:
                dec, w = _decompose_raw(R, Oc), torch.zeros(lay.R, d, dtype=dt, device=dev)
            else:
                dec, w = decompose_solve(R, Oc, _stage(x.detach()).reshape(-1, d))
            seg = lay.seg(dev)
            if need_x:
                gx = _back((2 * torch.index_select(g_m, 0, seg).unsqueeze(-1) * w).reshape(x.shape), x)
            if need_R or need_O:
                Sd, So = inverse_blocks(dec)
                w = w.contiguous()
                _hip.check(_hip.lib().cgps_mahal_logdet_adjoint_seg(
                    _hip.ptr(Sd), _hip.ptr(So), _hip.ptr(w), _hip.ptr(seg), lay.R, lay.B, d, _hip.dtype_code(dt),
                    _hip.ptr(g_m), _hip.ptr(g_l), _hip.stream_ptr()))
                if need_R:
                    gR = _back(Sd.reshape(Rs.shape), Rs)
                if need_O:
                    gO = _back(lay.caller_Os(So).reshape(Os.shape), Os)
        return gR, gO, gx, None


def mahal_and_det_batch(Rs, Os, x, lengths=None):
    """``mahal_and_det`` of B independent systems in one launch -> (mahal [B], logdet [B]): what a Python loop of
    ``mahal_and_det`` calls returns, each system reduced by one workgroup (cgps_mahal_logdet_batch).  An addition to the
    reference's surface.

    Dense layout (``lengths=None``): Rs [B, n, d, d], Os [B, n-1, d, d], x [B, n, d].  Nothing is uploaded from the host,
    and the call can be captured in a HIP graph.  Ragged layout: the systems concatenated, Rs [R, d, d], Os [R-1, d, d],
    x [R, d], with ``lengths`` a sequence or CPU integer tensor that sums to R; the entries of Os between two systems are
    ignored whatever they hold, and a system of length 0 gives (0, 0).  The lengths' device tensors are built once and
    cached (``leg._cached_batch_plan``: a capture needs one ordinary call with the same lengths first).
    ``x=None`` gives the log-determinants alone; mahal is zeros.

    Systems longer than ``BATCH_MAX_ROWS``, and every system at d = 8 and fp64 d = 6 (block sizes the batched kernel is
    not built for), are reduced by ``cgps_mahal_logdet`` on the same stream into their own slots.  With
    ``CHECK_POSITIVE_DEFINITE`` a system that is not positive definite raises ``NotPSDError`` naming it (``err.system``)
    and its local row (``err.row``); without it (and inside a graph capture, which cannot read the info words) that
    system's two values are NaN and every other slot is untouched.  CPU tensors are staged to the device and the results
    returned on the CPU; there is no CPU fallback.  Differentiable in Rs, Os and x: the backward factors the concatenated
    system once and weights every row with its own system's upstream gradients; the gradient of an ignored entry of
    Os is exactly 0."""
    lay = _batch_layout(Rs, Os, x, lengths)
    if _needs_grad(Rs, Os, x):
        return _BatchMahalLogdetFn.apply(Rs, Os, x, lay)
    return _mahal_and_det_batch(Rs, Os, x, lay)


# ----------------------------------------------------------------------------
# operations on a stored factor
# ----------------------------------------------------------------------------
def _rhs(y, N, d, dt):
    """y [N, d] or [N, d, ...] (the reference's einsums carry a trailing "...", :52-57) as a contiguous
    [N, d, m] device tensor, plus m and the trailing shape to restore."""
    v = _stage(y, dt)
    tail = tuple(v.shape[2:])
    m = 1
    for s in tail:
        m *= s
    return v.reshape(N, d, m), m, tail


def halfsolve(decomp, y):
    """L^-1 (T y) as the per-level list ("CRR layout")   (reference :312-338).  y: [N, d] or [N, d, m].
    No autograd graph (neither in y nor in the factor's Rs / Os)."""
    xs, _ = _halfsolve(decomp, y, want_mahal=False)
    return xs


def _halfsolve(decomp, y, want_mahal):
    Dp, Fp, Gp, N, d, like = _packed(decomp)
    dev, dt = Dp.device, Dp.dtype
    v, m, tail = _rhs(y, N, d, dt)
    xcrr = torch.empty((N, d, m), dtype=dt, device=dev)
    mah = torch.empty(1, dtype=torch.float64, device=dev) if want_mahal else None
    ws, nbytes = _hip.workspace(N, d, dt, _hip.OP_HALFSOLVE, dev, nrhs=m)
    _hip.check(_hip.lib().cgps_halfsolve(
        _hip.ptr(Dp), _hip.ptr(Fp), _hip.ptr(Gp), N, d, _hip.dtype_code(dt), m, _hip.ptr(v), _hip.ptr(xcrr),
        _hip.ptr(ws), nbytes, _hip.ptr(mah), _hip.stream_ptr()))
    ms, offD, _, _ = _hip.level_layout(N)
    xcrr = xcrr.reshape((N, d) + tail)
    xs = [_back(xcrr[offD[i]:offD[i + 1]], y) for i in range(len(ms))]
    return xs, mah


def backhalfsolve(decomp, ycrr):
    """T^T L^-T applied to a per-level list -> natural order   (reference :341-377).  No autograd graph."""
    Dp, Fp, Gp, N, d, like = _packed(decomp)
    dev, dt = Dp.device, Dp.dtype
    src = ycrr[0]
    tail = tuple(src.shape[2:])
    b = torch.cat([_stage(t, dt).reshape(t.shape[0], d, -1) for t in ycrr], dim=0).contiguous()
    assert b.shape[0] == N
    m = b.shape[2]
    x = torch.empty((N, d, m), dtype=dt, device=dev)
    ws, nbytes = _hip.workspace(N, d, dt, _hip.OP_BACKSOLVE, dev, nrhs=m)
    _hip.check(_hip.lib().cgps_backsolve(
        _hip.ptr(Dp), _hip.ptr(Fp), _hip.ptr(Gp), N, d, _hip.dtype_code(dt), m, _hip.ptr(b), _hip.ptr(x),
        _hip.ptr(ws), nbytes, _hip.stream_ptr()))
    return _back(x.reshape((N, d) + tail), src)


def _decomp_inputs(decomp):
    inp = getattr(decomp, "inputs", None)
    return inp if inp is not None else (None, None)


def solve(decomp, y):
    """J^-1 y   (reference :441-444); y: [N, d] or [N, d, m] (up to eight columns share one read of the
    factor).  Differentiable in y and in the Rs / Os the factor came from."""
    Rs, Os = _decomp_inputs(decomp)
    if _needs_grad(Rs, Os, y):
        if Rs is None:       # only y carries grad: J^-1 is a constant symmetric operator
            like = _packed(decomp)[5]
            Rs = Os = torch.zeros(0, dtype=like.dtype, device=like.device)
        return _SolveFn.apply(Rs, Os, y, decomp)
    return _solve_raw(decomp, y)


def _solve_raw(decomp, y):
    Dp, Fp, Gp, N, d, like = _packed(decomp)
    dev, dt = Dp.device, Dp.dtype
    v, m, tail = _rhs(y, N, d, dt)
    x = torch.empty((N, d, m), dtype=dt, device=dev)
    ws, nbytes = _hip.workspace(N, d, dt, _hip.OP_SOLVE, dev, nrhs=m)
    _hip.check(_hip.lib().cgps_solve(
        _hip.ptr(Dp), _hip.ptr(Fp), _hip.ptr(Gp), N, d, _hip.dtype_code(dt), m, _hip.ptr(v), _hip.ptr(x),
        _hip.ptr(ws), nbytes, _hip.stream_ptr()))
    return _back(x.reshape((N, d) + tail), y)


def det(decomp):
    """log|J| from the factor (the reference's name; it is the log-determinant)   (reference :447-458).
    Differentiable in the Rs / Os the factor came from."""
    Rs, Os = _decomp_inputs(decomp)
    if _needs_grad(Rs, Os):
        return _DetFn.apply(Rs, Os, decomp)
    return _det_raw(decomp)


def _det_raw(decomp):
    Dp, Fp, Gp, N, d, like = _packed(decomp)
    dev, dt = Dp.device, Dp.dtype
    out = torch.empty(1, dtype=torch.float64, device=dev)
    ws, nbytes = _hip.workspace(N, d, dt, _hip.OP_LOGDET_FACTOR, dev)
    _hip.check(_hip.lib().cgps_logdet_factor(
        _hip.ptr(Dp), N, d, _hip.dtype_code(dt), _hip.ptr(ws), nbytes, _hip.ptr(out), _hip.stream_ptr()))
    return _back(out.to(dt), like)[0]


def mahal(decomp, y):
    """y^T J^-1 y = ||L^-1 T y||^2   (reference :461-467); y: [N, d] or [N, d, m] (summed over the columns).
    Differentiable in y and in the Rs / Os the factor came from: with a gradient wanted it is
    sum(y * solve(decomp, y)), accumulated in fp64, through _SolveFn; otherwise one halfsolve that reduces the norm."""
    Rs, Os = _decomp_inputs(decomp)
    if _needs_grad(Rs, Os, y):
        dt = _packed(decomp)[0].dtype
        w = solve(decomp, y)
        return (y.to(torch.float64) * w.to(torch.float64)).sum().to(dt)
    _, m = _halfsolve(decomp, y, want_mahal=True)
    return _back(m.to(_packed(decomp)[0].dtype), y)[0]


def inverse_blocks(decomp):
    """Diagonal and lower off-diagonal blocks of J^-1   (reference :470-503).  No autograd graph."""
    Dp, Fp, Gp, N, d, like = _packed(decomp)
    dev, dt = Dp.device, Dp.dtype
    Sd = torch.empty((N, d, d), dtype=dt, device=dev)
    So = torch.empty((N - 1, d, d), dtype=dt, device=dev)
    ws, nbytes = _hip.workspace(N, d, dt, _hip.OP_INVERSE_BLOCKS, dev)
    _hip.check(_hip.lib().cgps_inverse_blocks(
        _hip.ptr(Dp), _hip.ptr(Fp), _hip.ptr(Gp), N, d, _hip.dtype_code(dt), _hip.ptr(Sd), _hip.ptr(So),
        _hip.ptr(ws), nbytes, _hip.stream_ptr()))
    return _back(Sd, like), _back(So, like)


# ----------------------------------------------------------------------------
# sampling (an addition to the reference's surface; its LEGFamily.sample_from_prior, models.py:243-252, is a stub)
# ----------------------------------------------------------------------------
def standard_normal(rows, cols, seed, stream=0, dtype=torch.float64, device=None):
    """[rows, cols] standard normals, element (r, s) a pure function of (seed, stream, r, s): Philox4x32-10 and
    Box-Muller as csrc/cgps_rng.h specifies them (cgps_normal_fill).  The first c columns of a wider array are bitwise
    those of a c-column array; `stream` separates independent arrays drawn under one seed."""
    dev = _device() if device is None else torch.device(device)
    if dev.type != "cuda":
        raise _hip.CgpsError("standard_normal fills device memory: the generator is a HIP kernel (no CPU fallback)")
    rows, cols = int(rows), int(cols)
    out = torch.empty((rows, cols), dtype=dtype, device=dev)
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().cgps_normal_fill(_hip.ptr(out), rows, cols, _hip.dtype_code(dtype),
                                               int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream) & 0xFFFFFFFF, _hip.stream_ptr()))
    return out


def sample(decomp, num_samples, seed, mean=None, stream=0):
    """num_samples draws from N(mean, J^-1) off the factor of J: x[:, :, s] = mean + backhalfsolve(decomp, eps)[:, :, s]
    with eps = standard_normal(N d, num_samples, seed, stream) in CRR layout -- one call (cgps_sample) that makes the
    noise in registers inside the backward sweep and never writes it.  Returns [N, d, num_samples]; sample s depends on
    (seed, stream, s) only, not on num_samples.  mean: [N, d] or None (zero).  No autograd graph."""
    Dp, Fp, Gp, N, d, like = _packed(decomp)
    dev, dt = Dp.device, Dp.dtype
    S = int(num_samples)
    mu = None if mean is None else _stage(mean.detach(), dt).reshape(N, d).contiguous()
    x = torch.empty((N, d, S), dtype=dt, device=dev)
    ws, nbytes = _hip.sample_workspace(N, d, dt, S, dev)
    _hip.check(_hip.lib().cgps_sample(
        _hip.ptr(Dp), _hip.ptr(Fp), _hip.ptr(Gp), N, d, _hip.dtype_code(dt), S, _hip.ptr(mu),
        int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream) & 0xFFFFFFFF, _hip.ptr(x), _hip.ptr(ws), nbytes, _hip.stream_ptr()))
    return _back(x, like)


# ----------------------------------------------------------------------------
# banded products with the block upper-bidiagonal U (diagonal F, super-diagonal G).
# Thin device-side helpers of the reference surface (:15-200); they run as batched
# products wherever their inputs live and are not on the fused hot path.
# ----------------------------------------------------------------------------
def UU_T(diags, offdiags):
    """Block-tridiagonal part of U U^T -> (diagonal, lower off-diagonal)   (reference :15-37)."""
    nf, ng = diags.shape[0], offdiags.shape[0]
    dg = diags @ diags.transpose(-1, -2)
    dg[:ng] += offdiags @ offdiags.transpose(-1, -2)
    k = min(nf - 1, ng)
    return dg, diags[1:1 + k] @ offdiags[:k].transpose(-1, -2)


def Ux(diags, offdiags, x):
    """U @ x   (reference :40-60)."""
    nf, ng = diags.shape[0], offdiags.shape[0]
    out = torch.einsum("bij,bj...->bi...", diags, x[:nf])
    out[:ng] += torch.einsum("bij,bj...->bi...", offdiags, x[1:1 + ng])
    return out


def U_Tx(diags, offdiags, x):
    """U^T @ x   (reference :63-87)."""
    nf, ng = diags.shape[0], offdiags.shape[0]
    rows = nf + 1 if nf == ng else nf
    out = x.new_zeros((rows,) + tuple(x.shape[1:]))
    out[:nf] = torch.einsum("bji,bj...->bi...", diags, x)
    out[1:1 + ng] += torch.einsum("bji,bj...->bi...", offdiags, x[:ng])
    return out


def SigU(sig_dblocks, sig_offdblocks, u_dblocks, u_offdblocks):
    """Diagonal and upper-diagonal blocks of Sig @ U   (reference :90-136)."""
    nf, ng = u_dblocks.shape[0], u_offdblocks.shape[0]
    mid = sig_dblocks @ u_dblocks
    mid[1:] += sig_offdblocks @ u_offdblocks[:nf - 1]
    hi = sig_dblocks[:ng] @ u_offdblocks
    k = min(ng, nf - 1)
    hi[:k] += sig_offdblocks[:k].transpose(-1, -2) @ u_dblocks[1:1 + k]
    return mid, hi


def UtV_diags(u_dblocks, u_offdblocks, v_dblocks, v_offdblocks):
    """Diagonal blocks of U^T V   (reference :139-178)."""
    nf, ng = u_dblocks.shape[0], u_offdblocks.shape[0]
    rows = nf + 1 if nf == ng else nf
    out = u_dblocks.new_zeros((rows,) + tuple(u_dblocks.shape[1:]))
    out[:nf] = u_dblocks.transpose(-1, -2) @ v_dblocks
    out[1:1 + ng] += u_offdblocks.transpose(-1, -2) @ v_offdblocks
    return out


def interleave(a, b):
    """V[::2] = a; V[1::2] = b   (reference :181-200)."""
    n, m = a.shape[0], b.shape[0]
    k = min(n, m)
    out = a.new_empty((n + m,) + tuple(a.shape[1:]))
    out[0:2 * k:2] = a[:k]
    out[1:2 * k:2] = b[:k]
    out[2 * k:] = a[k:] if n > m else b[k:]
    return out

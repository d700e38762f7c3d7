"""Thin harness for BASELINE config 5: LEG marginal likelihood + in-sample posterior mean.

This is NOT a re-implementation of the reference's `LEGFamily` (models.py is out of scope,
SURVEY.md section 2); it is the minimum of the caller's math needed to FEED the cyclic-reduction
path with the operands the reference feeds it, restated in our own code:

    G            = N N^T + R - R^T + 1e-5 I                       (models.py:152-159)
    Sigma^-1     = PEG precision blocks from exp(-1/2 dt G)        (models.py:181-239)
    K            = Sigma^-1 + blockdiag(B^T (LL^T)^-1 B)           (models.py:254-268)
    v            = x (LL^T)^-1 B                                   (models.py:270-280)
    log p(x)     = -1/2 (mahal + logdet)                           (models.py:301-372)
    posterior    = solve(decompose(K), v), inverse_blocks(...)     (models.py:282-298)

The d x d assembly (matrix exponentials, two small solves per time gap) is embarrassingly
parallel batched device work done with torch ops; everything block-tridiagonal goes through
cyclic_gps.cyclic_reduction, i.e. the HIP kernels.  Tensors follow the device of `ts`.
"""
import collections
import contextlib
import functools
import math
import os

import torch

from . import _hip
from . import cyclic_reduction as cr


_eyes = {}


def _scaled_eye(n, scale, dtype, device):
    """scale * I, built once per (n, scale, dtype, device): N ~ 500 is launch-bound and this is two launches per use."""
    key = (n, scale, dtype, device)
    e = _eyes.get(key)
    if e is None:
        e = _eyes[key] = scale * torch.eye(n, dtype=dtype, device=device)
    return e


_llw = {}


def _ll_weights(n, dtype, device):
    """weights of (x (LL^T)^-1 x, log LL^T, k_mahal, k_det, log|Sigma^-1|) in the log-likelihood: -1/2 (quad - k_mahal + n log LLT
    + k_det - sig) (the n log 2 pi of the observation term is a host constant)"""
    key = (n, dtype, device)
    w = _llw.get(key)
    if w is None:
        w = _llw[key] = torch.tensor([-0.5, -0.5 * n, 0.5, -0.5, 0.5], dtype=dtype, device=device)
    return w


class LEGMatrices:
    """The four model matrices as the reference registers them (models.py:135-178):
    N [d,d] lower triangular, R [d,d] strictly lower (G uses R - R^T), B [obs,d],
    Lambda [obs,obs] lower triangular with softplus already applied."""

    def __init__(self, N, R, B, Lambda):
        self.N, self.R, self.B, self.Lambda = N, R, B, Lambda

    def to(self, device):
        return LEGMatrices(*(t.to(device) for t in (self.N, self.R, self.B, self.Lambda)))

    @property
    def G(self):
        d = self.N.shape[0]
        return torch.addmm(self.R - self.R.T + _scaled_eye(d, 1e-5, self.N.dtype, self.N.device), self.N, self.N.T)

    @property
    def LLT_inv(self):
        """(Lambda Lambda^T + 1e-9 I)^-1, obs_dim x obs_dim, used through plain matrix products
        (torch.linalg.solve's GPU backward faults on ROCm 7.0 for a 1x1 system with hundreds of
        right-hand sides; the inverse's backward is matmul only)."""
        return self.inv_of(self.LLT)

    @staticmethod
    def inv_of(LLT):
        if LLT.shape[0] == 1:                         # a single output: no factorisation call (and none inside a HIP graph)
            return 1.0 / LLT
        return torch.linalg.inv_ex(LLT)[0]            # inv_ex: no error check, hence no device->host synchronisation

    @property
    def LLT(self):
        o = self.Lambda.shape[0]
        return torch.addmm(_scaled_eye(o, 1e-9, self.Lambda.dtype, self.Lambda.device), self.Lambda, self.Lambda.T)


def _peg_precision_hip(ts, G):
    """The same blocks from one HIP kernel (cgps_peg_precision, csrc/cgps_leg.h): one lane per block
    row, matrix exponential and the two small solves in registers.  No autograd graph."""
    n, d = ts.shape[0], G.shape[0]
    ts = ts.to(G.dtype).contiguous()
    G = G.contiguous()
    Rs = torch.empty(n, d, d, dtype=G.dtype, device=G.device)
    Os = torch.empty(max(n - 1, 0), d, d, dtype=G.dtype, device=G.device)
    info = torch.zeros(1, dtype=torch.int32, device=G.device)
    _hip.check(_hip.lib().cgps_peg_precision(_hip.ptr(ts), _hip.ptr(G), n, d, _hip.dtype_code(G.dtype), _hip.ptr(Rs),
                                             _hip.ptr(Os), _hip.ptr(info), _hip.stream_ptr()))
    if cr.CHECK_POSITIVE_DEFINITE:
        bad = int(info.item())
        if bad:
            raise cr.NotPSDError("time gap next to row %d gives a singular PEG block (zero-length gap?)" % (bad - 1))
    return Rs, Os


class _PegPrecisionFn(torch.autograd.Function):
    """cgps_peg_precision with its analytic adjoint (cgps_peg_precision_adjoint, csrc/cgps_leg.h): a
    training step assembles its operands with the same kernel as an evaluation."""

    @staticmethod
    def forward(ctx, ts, G):
        ctx.save_for_backward(ts, G)
        Rs, Os = _peg_precision_hip(ts.detach(), G.detach())
        ctx.mark_non_differentiable()
        return Rs, Os

    @staticmethod
    def backward(ctx, gRs, gOs):
        ts, G = ctx.saved_tensors
        n, d = ts.shape[0], G.shape[0]
        if n < 2:
            return None, torch.zeros_like(G)
        tsd = ts.detach().to(G.dtype).contiguous()
        gRs = torch.zeros(n, d, d, dtype=G.dtype, device=G.device) if gRs is None else cr._aligned16(gRs.to(G.dtype).contiguous())
        gOs = torch.zeros(n - 1, d, d, dtype=G.dtype, device=G.device) if gOs is None else cr._aligned16(gOs.to(G.dtype).contiguous())
        nb = (n - 1 + 63) // 64
        part = torch.empty(nb, d, d, dtype=G.dtype, device=G.device)
        want_ts = ctx.needs_input_grad[0]
        gtau = torch.empty(n - 1, dtype=G.dtype, device=G.device) if want_ts else None
        _hip.check(_hip.lib().cgps_peg_precision_adjoint(
            _hip.ptr(tsd), _hip.ptr(G.detach().contiguous()), n, d, _hip.dtype_code(G.dtype), _hip.ptr(gRs), _hip.ptr(gOs),
            _hip.ptr(part), _hip.ptr(gtau), _hip.stream_ptr()))
        gts = None
        if want_ts:
            z = gtau.new_zeros(1)
            gts = (torch.cat([z, gtau]) - torch.cat([gtau, z])).to(ts.dtype)
        return gts, part.sum(0)


def peg_precision(ts, G):
    """Diagonal and lower off-diagonal blocks of the PEG prior precision (models.py:181-239).
    On the GPU one HIP kernel, differentiable in G and ts through its analytic adjoint (a second
    kernel); on CPU tensors batched torch ops."""
    d = G.shape[0]
    wants_grad = torch.is_grad_enabled() and (G.requires_grad or ts.requires_grad)
    if G.is_cuda and ts.is_cuda and 1 <= d <= 8 and G.dtype in (torch.float32, torch.float64):
        if wants_grad and os.environ.get("CGPS_LEG_TORCH_ASSEMBLY") != "1":
            return _PegPrecisionFn.apply(ts, G)
        if not wants_grad:
            return _peg_precision_hip(ts, G)
    eye = torch.eye(d, dtype=G.dtype, device=G.device)
    # F = E - I without cancellation, as the kernels take it (csrc/cgps_leg.h, mat_expm1): the top right block of
    # matrix_exp([[A, I], [0, 0]]) is phi_1(A) and F = A phi_1(A).  I - E^T E = -(F + F^T + F^T F) then keeps its
    # relative precision at gaps far below the length scale of G, where E E^T and I agree to many digits.
    Am = -0.5 * G.unsqueeze(0) * (ts[1:] - ts[:-1]).reshape(-1, 1, 1)
    aug = torch.cat([torch.cat([Am, eye.expand_as(Am)], -1), Am.new_zeros(Am.shape[0], d, 2 * d)], -2)
    X = torch.matrix_exp(aug)
    E, F = X[:, :d, :d], Am @ X[:, :d, d:]
    Et, Ft = E.transpose(-1, -2), F.transpose(-1, -2)
    a = torch.linalg.solve(-(F + Ft + Ft @ F), Et)    # (I - E^T E)^-1 E^T
    b = torch.linalg.solve(-(F + Ft + F @ Ft), E)     # (I - E E^T)^-1 E
    c1, c2 = E @ a, Et @ b
    Rs = eye.repeat(ts.shape[0], 1, 1)
    Rs[:-1] += c2
    Rs[1:] += c1
    return Rs.contiguous(), (-b).contiguous()


def fused_supported(ts, G):
    """The assembly-in-registers form (cgps_leg_mahal_logdet) exists for this case: GPU tensors, no gradient wanted, a
    block size whose first pass runs one lane per row.  Looks at ts and G only: ``log_likelihood`` also keeps the fused
    kernels off when B, Lambda or xs need a gradient."""
    d = G.shape[0]
    return (G.is_cuda and ts.is_cuda and G.dtype in (torch.float32, torch.float64) and 1 <= d <= 7 and
            not (d == 6 and G.dtype == torch.float64) and
            not (torch.is_grad_enabled() and (G.requires_grad or ts.requires_grad)) and
            os.environ.get("CGPS_LEG_UNFUSED") != "1")


def leg_mahal_and_det(ts, G, A=None, v=None):
    """(v^T J^-1 v, log|J|) of J = PEG precision(ts, G) + blockdiag(A) in ONE kernel launch that never writes the blocks
    of J to memory (cgps_leg_mahal_logdet, csrc/cgps_tile_leg.h): what `peg_precision` + `cr.mahal_and_det` compute
    (models.py:349-367).  A [d,d] or None; v [N,d] or None (zeros).  No autograd graph."""
    n, d, dt = ts.shape[0], G.shape[0], G.dtype
    ts = ts.to(dt).contiguous()
    G = G.contiguous()
    A = None if A is None else A.to(dt).contiguous()
    v = None if v is None else v.to(dt).contiguous()
    ws, ws_bytes = _hip.workspace(n, d, dt, _hip.OP_MAHAL_LOGDET, G.device)
    out = torch.empty(2, dtype=torch.float64, device=G.device)
    info = torch.zeros(1, dtype=torch.int32, device=G.device)
    _hip.check(_hip.lib().cgps_leg_mahal_logdet(_hip.ptr(ts), _hip.ptr(G), _hip.ptr(A), _hip.ptr(v), n, d, _hip.dtype_code(dt),
                                                _hip.ptr(ws), ws_bytes, _hip.ptr(out), _hip.ptr(info), _hip.stream_ptr()))
    if cr.CHECK_POSITIVE_DEFINITE:
        bad = int(info.item())
        if bad:
            raise cr.NotPSDError("LEG system: a block near row %d is not positive definite (or a time gap has zero length)" % (bad - 1))
    out = out.to(dt)
    return out[0], out[1]


def leg_loglik_reductions(ts, G, A, v):
    """The two reductions of a LEG log-likelihood in ONE launch (cgps_leg_mahal_logdet_pair): returns
    (v^T K^-1 v, log|K|, log|Sigma^-1|) with K = PEG precision(ts, G) + blockdiag(A), Sigma^-1 the PEG precision itself
    (models.py:349-367: decompose + det of Sigma^-1, mahal_and_det of K).  No autograd graph."""
    dt = G.dtype
    ts = ts.to(dt).contiguous()
    G, A, v = G.contiguous(), A.to(dt).contiguous(), v.to(dt).contiguous()
    return _leg_pair_checked(ts, G, _hip.ROWS_PLAIN, A, None, v)


# ---- many independent series at once ----------------------------------------------------------
BATCH_MAX_ROWS = 4096
"""Series longer than this are reduced by ``cgps_leg_mahal_logdet_pair`` (several workgroups per series) instead
of the one workgroup per series of ``cgps_leg_loglik_batch``; their values go into their slots all the same."""


def _batch_layout(ts, xs, lengths):
    """(ts [R], xs [R, obs], lengths as a list of ints) of either input layout; raises ValueError before
    anything is launched when the lengths do not describe the rows."""
    if lengths is None:
        if ts.dim() != 2 or xs.dim() != 3 or tuple(xs.shape[:2]) != tuple(ts.shape):
            raise ValueError("dense layout wants ts[B, n] and xs[B, n, obs_dim], got %s and %s"
                             % (tuple(ts.shape), tuple(xs.shape)))
        B, n = ts.shape
        if B > 0 and n < 1:
            raise ValueError("series of length 0")
        return ts.reshape(B * n), xs.reshape(B * n, xs.shape[-1]), [int(n)] * B
    if isinstance(lengths, torch.Tensor):
        if lengths.is_cuda or lengths.dim() != 1 or lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
            raise ValueError("lengths must be host data: a list or a 1-d CPU integer tensor")
        lengths = lengths.tolist()
    lengths = [int(n) for n in lengths]
    if ts.dim() != 1 or xs.dim() != 2:
        raise ValueError("ragged layout wants ts[sum(lengths)] and xs[sum(lengths), obs_dim], got %s and %s"
                         % (tuple(ts.shape), tuple(xs.shape)))
    bad = [b for b, n in enumerate(lengths) if n < 1]
    if bad:
        raise ValueError("series %d has length %d (every series needs at least one row)" % (bad[0], lengths[bad[0]]))
    total = sum(lengths)
    if total != ts.shape[0] or total != xs.shape[0]:
        raise ValueError("lengths sum to %d rows, ts has %d and xs %d" % (total, ts.shape[0], xs.shape[0]))
    return ts, xs, lengths


def batch_supported(ts, G):
    """The batched kernel (cgps_leg_loglik_batch) exists for this case: GPU tensors and the block sizes of
    ``fused_supported`` (d <= 7, not fp64 d = 6), with or without a gradient."""
    d = G.shape[0]
    return (G.is_cuda and ts.is_cuda and G.dtype in (torch.float32, torch.float64) and 1 <= d <= 7 and
            not (d == 6 and G.dtype == torch.float64))


class _BatchPlan:
    """What the lengths fix on the host: device offsets, per-row lengths for repeat_interleave, the series-cut mask
    of the concatenated assembly, and the series handed to the one-series kernel."""

    def __init__(self, lengths, device):
        self.lengths = lengths
        self.B, self.R = len(lengths), sum(lengths)
        off = [0]
        for n in lengths:
            off.append(off[-1] + n)
        self.starts = off
        self.offsets = torch.tensor(off, dtype=torch.int64).to(device, non_blocking=True)
        self.lens = torch.tensor(lengths, dtype=torch.int64).to(device, non_blocking=True)
        cut = torch.zeros(max(self.R - 1, 0), dtype=torch.uint8)
        if self.B > 1:
            cut[torch.tensor(off[1:-1]) - 1] = 1
        self.cut = cut.to(device, non_blocking=True)
        self.long = [b for b, n in enumerate(lengths) if n > BATCH_MAX_ROWS]

    def per_row(self, g):
        return g.repeat_interleave(self.lens, output_size=self.R)

    def boundary_rows(self, m=1):
        """Device int64 [m B - 1]: the entries of the off-diagonal array of m models' concatenated batches (m = 1: of the
        batch) that lie between two series or two models.  Computed on the device from the offsets (nothing copied from
        the host) at the first use and kept: a call that is to be captured builds it in its warm-up."""
        kept = self.__dict__.setdefault("_boundary_rows", {})
        idx = kept.get(m)
        if idx is None:
            ends = self.offsets[1:] - 1
            idx = kept[m] = (torch.arange(m, device=ends.device).unsqueeze(1) * self.R + ends).reshape(-1)[:-1].contiguous()
        return idx


PLAN_CACHE_SIZE = 8
_plans = {}                 # (lengths, device) -> plan, least recently used first
_captured_plans = {}        # plans that a stream capture has read: never dropped


def _capturing(device):
    return torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing()


def _cached_batch_plan(lengths, device, make=None):
    """The plan of these lengths, built once: a repeated call -- a training loop over one data set, a graph capture
    after its warm-up -- then copies nothing from the host.  The PLAN_CACHE_SIZE most recently used plans are kept.
    A plan handed out while the current stream is being captured is kept for as long as the process lives: the
    captured kernels hold the addresses of its device tensors and nothing else would own them, whoever made the
    capture and whatever they kept of its results.  A capture cannot build a plan (that is a copy from the host):
    RuntimeError unless an ordinary call with the same lengths came first, as ``Graphed``'s warm-up is.  ``make``
    (None: ``_BatchPlan``) is another plan class with caches of its own, ``make.plans`` and ``make.captured``
    (``predict._TargetPlan``): the kinds do not compete for slots."""
    key = (tuple(lengths), str(device))
    plans, captured = (_plans, _captured_plans) if make is None else (make.plans, make.captured)
    plan = captured.get(key)
    if plan is not None:
        return plan
    plan = plans.pop(key, None)                                  # (put back below, as the most recent)
    if _capturing(device):
        if plan is None:
            raise RuntimeError("a batched call inside a graph capture (log_likelihood_batch(observed= / noise_var=), the batched "
                               "posterior and predictions) needs one ordinary call with the same lengths before the capture "
                               "(leg.Graphed's warm-up is one)")
        captured[key] = plan
        return plan
    if plan is None:
        plan = (make or _BatchPlan)(lengths, device)
        while len(plans) >= PLAN_CACHE_SIZE:
            plans.pop(next(iter(plans)))
    plans[key] = plan
    return plan


def _leg_pair_raw(ts, G, source, term, rows, v):
    """The pair of reductions of one series, (out4 fp64, info2), nothing read on the host.  ``source`` names where a
    row's diagonal term comes from, as in ``_posterior_blocks_models``: _hip.ROWS_PLAIN (term [d, d], rows None:
    cgps_leg_mahal_logdet_pair), ROWS_TABLE (term [P, d, d], rows = pattern bytes [n]: cgps_leg_mahal_logdet_pair_obs) or
    ROWS_WEIGHTED (term = basis [Kb, d, d], rows = weights [n, Kb]: cgps_leg_mahal_logdet_pair_w)."""
    n, d, dt = ts.shape[0], G.shape[0], G.dtype
    ws, ws_bytes = _hip.pair_workspace(n, d, dt, G.device), _hip.pair_workspace_bytes(n, d, dt)
    out = torch.empty(4, dtype=torch.float64, device=G.device)
    info = torch.zeros(2, dtype=torch.int32, device=G.device)
    lib = _hip.lib()
    fn = (lib.cgps_leg_mahal_logdet_pair, lib.cgps_leg_mahal_logdet_pair_obs, lib.cgps_leg_mahal_logdet_pair_w)[source]
    per_row = () if source == _hip.ROWS_PLAIN else (term.shape[0], _hip.ptr(rows))
    _hip.check(fn(_hip.ptr(ts), _hip.ptr(G), _hip.ptr(term), *per_row, _hip.ptr(v), n, d, _hip.dtype_code(dt), _hip.ptr(ws),
                  ws_bytes, _hip.ptr(out), _hip.ptr(info), _hip.stream_ptr()))
    return out, info


def _leg_pair_checked(ts, G, source, term, rows, v):
    """``_leg_pair_raw`` as the one-series entry points hand it on: NotPSDError for a system that is not positive definite
    (under ``cr.CHECK_POSITIVE_DEFINITE``), then (v^T K^-1 v, log|K|, log|Sigma^-1|) in G's dtype."""
    out, info = _leg_pair_raw(ts, G, source, term, rows, v)
    if cr.CHECK_POSITIVE_DEFINITE:
        bad = info.tolist()
        if bad[0] or bad[1]:
            raise cr.NotPSDError("LEG system: a block near row %d is not positive definite (or a time gap has zero length)"
                                 % ((bad[0] or bad[1]) - 1))
    out = out.to(G.dtype)
    return out[0], out[1], out[3]


def _check_pattern(pattern, n):
    if pattern.dtype != torch.uint8 or pattern.shape != (n,) or not pattern.is_cuda:
        raise ValueError("pattern must be a uint8 device tensor of shape [%d], got %s %s"
                         % (n, pattern.dtype, tuple(pattern.shape)))


def _check_basis_weights(basis, weights, dt):
    if basis.dtype != dt or weights.dtype != dt:
        raise ValueError("basis and weights must have G's dtype %s, got %s and %s" % (dt, basis.dtype, weights.dtype))
    if not (basis.is_cuda and weights.is_cuda):
        raise ValueError("basis and weights must be device tensors")


def leg_loglik_reductions_obs(ts, G, A_table, pattern, v):
    """``leg_loglik_reductions`` of a series whose rows observe different channels, still ONE launch
    (cgps_leg_mahal_logdet_pair_obs): K = PEG precision(ts, G) + blockdiag(A_table[pattern[i]]).  A_table [P, d, d] with
    1 <= P <= 256, pattern uint8 [N] on the device (a byte >= P takes the last entry), v [N, d].  No autograd graph."""
    n, d, dt = ts.shape[0], G.shape[0], G.dtype
    _check_pattern(pattern, n)
    if A_table.dim() != 3 or tuple(A_table.shape[1:]) != (d, d):
        raise ValueError("A_table must be [P, %d, %d], got %s" % (d, d, tuple(A_table.shape)))
    ts = ts.to(dt).contiguous()
    G, A_table, pattern, v = G.contiguous(), A_table.to(dt).contiguous(), pattern.contiguous(), v.to(dt).contiguous()
    return _leg_pair_checked(ts, G, _hip.ROWS_TABLE, A_table, pattern, v)


def leg_loglik_reductions_w(ts, G, basis, weights, v):
    """``leg_loglik_reductions`` of a series whose rows each add a term of their own, still ONE launch
    (cgps_leg_mahal_logdet_pair_w): K = PEG precision(ts, G) + blockdiag(sum_k weights[i, k] basis[k]), the d x d terms
    formed in registers and never written.  basis [Kb, d, d] with 1 <= Kb <= 64 and weights [N, Kb], both device tensors
    of G's dtype (``observation_weights`` builds them); v [N, d].  No autograd graph."""
    n, d, dt = ts.shape[0], G.shape[0], G.dtype
    if basis.dim() != 3 or tuple(basis.shape[1:]) != (d, d) or not 1 <= basis.shape[0] <= 64:
        raise ValueError("basis must be [Kb, %d, %d] with 1 <= Kb <= 64, got %s" % (d, d, tuple(basis.shape)))
    if tuple(weights.shape) != (n, basis.shape[0]):
        raise ValueError("weights must be [%d, %d] (one row of Kb weights per time stamp), got %s"
                         % (n, basis.shape[0], tuple(weights.shape)))
    if tuple(v.shape) != (n, d):
        raise ValueError("v must be [%d, %d], got %s" % (n, d, tuple(v.shape)))
    _check_basis_weights(basis, weights, dt)
    ts = ts.to(dt).contiguous()
    G, basis, weights, v = G.contiguous(), basis.contiguous(), weights.contiguous(), v.to(dt).contiguous()
    return _leg_pair_checked(ts, G, _hip.ROWS_WEIGHTED, basis, weights, v)


def _leg_rows_reductions(ts, G, source, term, rows, v, q, plan):
    """The reductions of a batch for one model (G [d, d]: [B, 4] fp64 and [B, 2] info words) or for M models (G
    [M, d, d]: [M, B, 4] and [M, B, 2]) from one launch -- cgps_leg_loglik_batch / cgps_leg_loglik_models, with _obs or
    _w for the other sources -- and the series longer than BATCH_MAX_ROWS through ``_leg_pair_raw`` per model and series
    on the same stream.  (source, term, rows) as in ``_leg_pair_raw``; with M models term, v and q carry a leading model
    axis, and so do the weights (the pattern bytes describe the batch once).  Checked, contiguous operands."""
    models = G.dim() == 3
    d, dt = G.shape[-1], G.dtype
    lead, batch = ((G.shape[0],), (plan.R, G.shape[0])) if models else ((), ())
    out = torch.empty(*lead, plan.B, 4, dtype=torch.float64, device=G.device)
    info = torch.zeros(*lead, plan.B, 2, dtype=torch.int32, device=G.device)
    fn = getattr(_hip.lib(), "cgps_leg_loglik_" + ("models" if models else "batch") + ("", "_obs", "_w")[source])
    per_row = () if source == _hip.ROWS_PLAIN else (term.shape[-3], _hip.ptr(rows))
    _hip.check(fn(_hip.ptr(ts), _hip.ptr(plan.offsets), plan.B, *batch, _hip.ptr(G), _hip.ptr(term), *per_row, _hip.ptr(v),
                  _hip.ptr(q), d, _hip.dtype_code(dt), BATCH_MAX_ROWS, _hip.ptr(out), _hip.ptr(info), _hip.stream_ptr()))
    if plan.long:
        own_rows = source == _hip.ROWS_WEIGHTED               # a model's own weights; the pattern is every model's
        if not models:                                        # one model: views with a model axis of length 1
            G, term, v, q, out_m, info_m = (t.unsqueeze(0) for t in (G, term, v, q, out, info))
            rows = rows.unsqueeze(0) if own_rows else rows
        else:
            out_m, info_m = out, info
        for b in plan.long:
            s, e = plan.starts[b], plan.starts[b + 1]
            for k in range(G.shape[0]):
                rows_k = None if rows is None else rows[k, s:e] if own_rows else rows[s:e]
                o4, i2 = _leg_pair_raw(ts[s:e], G[k], source, term[k], rows_k, v[k, s:e])
                out_m[k, b, :3] = o4[[0, 1, 3]]
                out_m[k, b, 3] = q[k, s:e].to(torch.float64).sum()
                info_m[k, b] = i2
    return out, info


def leg_loglik_batch_reductions(ts, G, A, v, q, plan):
    """The per-series reductions of a batch, no autograd graph: [B, 4] fp64 rows (v^T K^-1 v, log|K|, log|Sigma^-1|,
    sum q) and [B, 2] info words (cgps_leg_loglik_batch; series longer than BATCH_MAX_ROWS through
    cgps_leg_mahal_logdet_pair on the same stream).  ts, A, v, q in G's dtype, contiguous."""
    return _leg_rows_reductions(ts, G, _hip.ROWS_PLAIN, A, None, v, q, plan)


def leg_loglik_batch_reductions_obs(ts, G, A_table, pattern, v, q, plan):
    """``leg_loglik_batch_reductions`` of series whose rows observe different channels, still ONE launch
    (cgps_leg_loglik_batch_obs): K_b = PEG precision(ts_b, G) + blockdiag(A_table[pattern[i]]) over the series' rows.
    A_table [P, d, d] with 1 <= P <= 256, pattern uint8 [R] on the device, one byte per row of the concatenated batch
    (a byte >= P takes the last entry); series longer than BATCH_MAX_ROWS through cgps_leg_mahal_logdet_pair_obs with
    their slice of the pattern.  ts, A_table, v, q in G's dtype, contiguous.  No autograd graph."""
    d = G.shape[0]
    _check_pattern(pattern, plan.R)
    if A_table.dim() != 3 or tuple(A_table.shape[1:]) != (d, d):
        raise ValueError("A_table must be [P, %d, %d], got %s" % (d, d, tuple(A_table.shape)))
    return _leg_rows_reductions(ts, G, _hip.ROWS_TABLE, A_table, pattern.contiguous(), v, q, plan)


def leg_loglik_batch_reductions_w(ts, G, basis, weights, v, q, plan):
    """``leg_loglik_batch_reductions`` of series whose rows each add a term of their own, still ONE launch
    (cgps_leg_loglik_batch_w): K_b = PEG precision(ts_b, G) + blockdiag(sum_k weights[i, k] basis[k]) over the series'
    rows, the d x d terms formed in registers and never written.  basis [Kb, d, d] with 1 <= Kb <= 64 and weights
    [R, Kb], one row per row of the concatenated batch, both device tensors of G's dtype (``observation_weights`` builds
    them); series longer than BATCH_MAX_ROWS through cgps_leg_mahal_logdet_pair_w with their slice of the weights.
    ts, v, q in G's dtype, contiguous.  No autograd graph."""
    d, dt = G.shape[0], G.dtype
    if basis.dim() != 3 or tuple(basis.shape[1:]) != (d, d) or not 1 <= basis.shape[0] <= 64:
        raise ValueError("basis must be [Kb, %d, %d] with 1 <= Kb <= 64, got %s" % (d, d, tuple(basis.shape)))
    if tuple(weights.shape) != (plan.R, basis.shape[0]):
        raise ValueError("weights must be [%d, %d] (one row of Kb weights per row of the batch), got %s"
                         % (plan.R, basis.shape[0], tuple(weights.shape)))
    _check_basis_weights(basis, weights, dt)
    return _leg_rows_reductions(ts, G, _hip.ROWS_WEIGHTED, basis.contiguous(), weights.contiguous(), v, q, plan)


# ---- one model or many: the drivers of the concatenated system ------------------------------------------------------
# Everything below that takes G follows ``_leg_rows_reductions``: G [d, d] means no model axis -- one model's batch, the
# _seg / _batch entry points, failures named "LEG batch: series b" -- and G [M, d, d] the system "model 0's batch, then
# model 1's batch, ...", the _models entry points, failures named "LEG models: model k, series b".  The other operands
# carry the same leading axis or none.
MODELS_BACKWARD_MAX_ROWS = 1 << 22
"""The backward of ``log_likelihood_models`` runs in chunks of whole models whose concatenated rows stay under this
(a chunk always holds at least one model): about ten [rows, d, d] arrays are live at once, 0.84 GB each for a full
chunk at d = 5 in fp64."""


def _model_chunks(G, R, max_rows):
    """The chunks of whole models of at most ``max_rows`` concatenated rows (one model at least) as (k0, k1, sel), ``sel``
    the slice that takes the chunk's models out of a stacked operand.  G [d, d]: the one chunk (0, 1, None), whose
    operands are taken as they are (``_take``)."""
    if G.dim() == 2:
        return [(0, 1, None)]
    M, per = G.shape[0], max(1, max_rows // R)
    return [(k0, min(M, k0 + per), slice(k0, min(M, k0 + per))) for k0 in range(0, M, per)]


def _take(t, sel):
    """The chunk's models of a stacked operand; without a model axis the operand itself (not even a view is made: a
    one-model call is bound by its launches)."""
    return t if sel is None else t[sel]


def _cat_chunks(parts):
    """The chunks' results along the model axis (the one chunk itself when there is no other: no copy)."""
    return parts[0] if len(parts) == 1 else torch.cat(parts)


def _locate_row(plan, row):
    """(model of the chunk, series, local row) of a row of the concatenated system of one or several models' batches."""
    import bisect
    k, row = divmod(row, plan.R)
    b = min(max(bisect.bisect_right(plan.starts, row) - 1, 0), plan.B - 1)
    return k, b, row - plan.starts[b]


_NOT_PD = "a block near its row %d is not positive definite"
_NOT_PD_OR_GAP = _NOT_PD + " (or a time gap has zero length)"
_GAP_BLOCK = "the time gap next to its row %d gives a singular PEG block (zero-length gap?)"
_GAP_NOISE = "the time gap next to its row %d is singular (zero-length gap?)"


def _not_pd_error(k, b, text):
    """The NotPSDError that names series b of one model's batch (k None) or of model k."""
    where = ("LEG batch: series %d" % b) if k is None else ("LEG models: model %d, series %d" % (k, b))
    return cr.NotPSDError("%s: %s" % (where, text))


def _row_error(plan, row, k0, text):
    """``_not_pd_error`` for a row of the concatenated system; ``k0`` is None without a model axis and otherwise the
    first model of the chunk.  ``text`` takes the local row."""
    k, b, r = _locate_row(plan, row)
    return _not_pd_error(None if k0 is None else k0 + k, b, text % r)


def _check_gaps(info, plan, k0, text):
    """Under ``cr.CHECK_POSITIVE_DEFINITE``: the info word of an assembly kernel read on the host, a singular gap named."""
    if cr.CHECK_POSITIVE_DEFINITE:
        bad = int(info.item())
        if bad:
            raise _row_error(plan, bad - 1, k0, text)


def _raise_not_pd(info):
    """The first failed system of the reductions' info words [B, 2] or [M, B, 2], named."""
    bad = info.cpu()
    hits = torch.nonzero(bad.amax(-1)).tolist()
    if hits:
        k, b = hits[0] if info.dim() == 3 else (None, hits[0][0])
        code = bad[tuple(hits[0])].tolist()
        raise _not_pd_error(k, b, _NOT_PD_OR_GAP % ((code[0] or code[1]) - 1))


def _peg_precision_models(ts, G, cut, info=None):
    """Blocks of the block-diagonal PEG precision of concatenated series (cgps_peg_precision_seg) or, with G [m, d, d], of
    the same rows model after model (cgps_peg_precision_models): Rs [m R, d, d], Os [m R - 1, d, d] with zero blocks
    between two models.  ``info``: an int32 word to receive the kernel's (1 + the row of a singular gap).  No autograd
    graph."""
    R, d, lib = ts.shape[0], G.shape[-1], _hip.lib()
    fn, count = (lib.cgps_peg_precision_models, (R, G.shape[0])) if G.dim() == 3 else (lib.cgps_peg_precision_seg, (R,))
    n = math.prod(count)
    Rs = torch.empty(n, d, d, dtype=G.dtype, device=G.device)
    Os = torch.empty(max(n - 1, 0), d, d, dtype=G.dtype, device=G.device)
    if info is None:
        info = torch.zeros(1, dtype=torch.int32, device=G.device)
    _hip.check(fn(_hip.ptr(ts), _hip.ptr(G), _hip.ptr(cut), *count, d, _hip.dtype_code(G.dtype), _hip.ptr(Rs), _hip.ptr(Os),
                  _hip.ptr(info), _hip.stream_ptr()))
    return Rs, Os


_peg_precision_seg = _peg_precision_models        # the same function: the name of its form without a model axis


def _peg_precision_adjoint_models(ts, G, cut, gRs, gOs, want_ts):
    """(d loss / d G, d loss / d ts [R] or None) through cgps_peg_precision_adjoint_seg or, with G [m, d, d],
    cgps_peg_precision_adjoint_models: every model's partial sums added per model, the models' gradients in ts added
    over the models."""
    R, d = ts.shape[0], G.shape[-1]
    if R < 2:
        return torch.zeros_like(G), (torch.zeros_like(ts) if want_ts else None)
    lead = tuple(G.shape[:-2])
    part = torch.empty(lead + ((R - 1 + 63) // 64, d, d), dtype=G.dtype, device=G.device)
    gtau = torch.empty(lead + (R - 1,), dtype=G.dtype, device=G.device) if want_ts else None
    lib = _hip.lib()
    fn, count = (lib.cgps_peg_precision_adjoint_models, (R,) + lead) if lead else (lib.cgps_peg_precision_adjoint_seg, (R,))
    _hip.check(fn(_hip.ptr(ts), _hip.ptr(G), _hip.ptr(cut), *count, d, _hip.dtype_code(G.dtype), _hip.ptr(cr._aligned16(gRs.contiguous())),
                  _hip.ptr(cr._aligned16(gOs.contiguous())), _hip.ptr(part), _hip.ptr(gtau), _hip.stream_ptr()))
    gts = None
    if want_ts:
        z = gtau.new_zeros(lead + (1,))
        gts = torch.cat([z, gtau], -1) - torch.cat([gtau, z], -1)
        if lead:
            gts = gts.sum(0)
    return part.sum(-3), gts


def _mm(a, b):
    """a b of two matrices or of two stacks of matrices, by the call that each case has always made: ``torch.matmul``
    reshapes a stack on its way to ``bmm``, which for an axis of length 1 can pick another kernel and another last bit."""
    return torch.bmm(a, b) if a.dim() == 3 else torch.mm(a, b)


def _rows_product_models(a, b, rows=4096):
    """a^T b of two tall matrices a [R, p] and b [R, q] (contiguous), or per model of a [m, R, p] and b [m, R, q], as
    batched products over chunks of ``rows`` rows, added up by one reduction in a fixed order, plus the product of the
    remainder.  One ``a.T @ b`` with R in the hundreds of thousands and p, q of a few dozen is a single GEMM tile's worth
    of output with all of R as its inner dimension: 55 ms at R = 514 048, p = 1, q = 25 on an MI355X."""
    R, p, q = a.shape[-2], a.shape[-1], b.shape[-1]
    C = R // rows
    out = _mm(a[..., C * rows:, :].transpose(-1, -2), b[..., C * rows:, :])
    if C:
        out = out + torch.bmm(a[..., :C * rows, :].reshape(-1, rows, p).transpose(1, 2),
                              b[..., :C * rows, :].reshape(-1, rows, q)).view(tuple(a.shape[:-2]) + (C, p, q)).sum(-3)
    return out


_rows_product = _rows_product_models        # the same function: the name of its form without a model axis


def _models_diag(source, G, term, rows, need_term, need_rows):
    """What the backward has to know about where the rows' diagonal terms come from, as a pair of functions over a chunk
    of models (``sel`` of ``_model_chunks``): diag_term(sel) is what K's diagonal adds to the chunk's Rs [.., R, d, d],
    and diag_grads(sel, gR) sends its block gradients gR [.., R, d, d] back as (d loss / d term, d loss / d rows) of the
    chunk, None where not wanted.  (source, term, rows) as in ``_leg_pair_raw``."""
    d, dd = G.shape[-1], G.shape[-1] * G.shape[-1]
    if source == _hip.ROWS_PLAIN:                                # a model's one block, broadcast over its rows
        return (lambda sel: _take(term, sel).unsqueeze(-3)), (lambda sel, gR: (gR.sum(-3), None))
    if source == _hip.ROWS_TABLE:
        # row i adds A_table[idx[i]]; the gradient of A_table is the per-pattern sum of the rows' block gradients, taken as
        # a matrix product with the one-hot matrix of the pattern, which all models share (no scatter: ``index_add_`` on
        # the GPU adds with atomics, in no fixed order)
        P = term.shape[-3]
        idx = rows.long().clamp(max=P - 1)                       # the kernel's clamp

        def table_grads(sel, gR):
            lead = tuple(gR.shape[:-3])
            codes = torch.arange(P, device=idx.device).unsqueeze(1)
            step = max(1024, (1 << 24) // P)                     # rows per product: the one-hot matrix stays small
            gA = torch.zeros(lead + (P, dd), dtype=G.dtype, device=G.device)
            for s in range(0, gR.shape[-3], step):               # (one product unless P * R > 2^24)
                onehot = (idx[s:s + step].unsqueeze(0) == codes).to(G.dtype)
                gA = gA + torch.matmul(onehot, gR[..., s:s + step, :, :].reshape(lead + (-1, dd)))
            return gA.view(lead + (P, d, d)), None
        return (lambda sel: _take(term, sel)[..., idx, :, :]), table_grads
    # row i adds sum_k weights[i, k] basis[k]; gR_i goes to the basis as sum_i weights[i, k] gR_i and to the weights as
    # <gR_i, basis[k]>, both plain matrix products (per model)
    Kb = term.shape[-3]

    def weighted_grads(sel, gR):
        lead = tuple(gR.shape[:-3])
        gR = gR.reshape(lead + (-1, dd))
        gb = _rows_product_models(_take(rows, sel), gR).view(lead + (Kb, d, d)) if need_term else None
        gw = _mm(gR, _take(term, sel).reshape(lead + (Kb, dd)).transpose(-1, -2)) if need_rows else None
        return gb, gw
    return (lambda sel: torch.einsum("...nk,...kij->...nij", _take(rows, sel), _take(term, sel))), weighted_grads


def _models_backward(needs, plan, source, ts, G, term, rows, v, gout):
    """The backward of ``_LegModelsFn`` on the concatenated system -- block-diagonal over series, and over models when there
    are several (zero coupling between them) -- in chunks of whole models (MODELS_BACKWARD_MAX_ROWS; without a model
    axis the one chunk is the operands themselves): series-aware assembly, decompose_solve + inverse_blocks of K (its
    diagonal Rs + the source's term, ``_models_diag``) and of Sigma^-1, block gradients weighted per row by the systems'
    upstream gradients, series-aware adjoint.  Returns (gts, gG, gterm, grows, gv, gq) for ``needs``, the six
    needs_input_grad of those inputs."""
    need_ts, need_G, need_term, need_rows, need_v, need_q = needs
    need_diag = need_term or need_rows
    d, R = G.shape[-1], plan.R
    gout = gout.to(G.dtype)
    diag_term, diag_grads = _models_diag(source, G, term, rows, need_term, need_rows)

    def spread(g, c):                                 # column c of [.., B, 4], spread over the rows of the chunk
        return g[..., c].repeat_interleave(plan.lens, dim=-1, output_size=R).reshape(-1)

    gq = spread(gout, 3).view(tuple(gout.shape[:-2]) + (R,)) if need_q else None
    gts, gG, gterm, grows, gv = None, [], [], [], []
    if need_ts or need_G or need_diag or need_v:
        for _, _, sel in _model_chunks(G, R, MODELS_BACKWARD_MAX_ROWS):
            g, Gc = _take(gout, sel), _take(G, sel)
            lead = tuple(Gc.shape[:-2])
            Rs, Os = _peg_precision_models(ts, Gc, plan.cut)
            gm, gl = spread(g, 0), spread(g, 1)
            dec, w = cr.decompose_solve((Rs.view(lead + (R, d, d)) + diag_term(sel)).view(-1, d, d), Os, _take(v, sel).reshape(-1, d))
            if need_v:
                gv.append((2 * gm.unsqueeze(-1) * w).view(lead + (R, d)))
            if need_ts or need_G or need_diag:
                Sd, So = cr.inverse_blocks(dec)
                gR = gl.view(-1, 1, 1) * Sd - gm.view(-1, 1, 1) * (w.unsqueeze(-1) * w.unsqueeze(-2))
                if need_diag:
                    gt, gr = diag_grads(sel, gR.view(lead + (R, d, d)))
                    gterm.append(gt)
                    grows.append(gr)
                if need_ts or need_G:
                    # (the entries of gO between two models hold whatever the zero coupling gives: never read)
                    gO = 2 * (gl[1:].view(-1, 1, 1) * So - gm[1:].view(-1, 1, 1) * (w[1:].unsqueeze(-1) * w[:-1].unsqueeze(-2)))
                    if Rs.shape[0] > 1:      # (one row: its block is I whatever G and ts are)
                        gs = spread(g, 2)
                        Sd0, So0 = cr.inverse_blocks(cr.decompose(Rs, Os))     # the prior precision's log-det
                        gR = gR + gs.view(-1, 1, 1) * Sd0
                        gO = gO + 2 * gs[1:].view(-1, 1, 1) * So0
                    gGc, gtsc = _peg_precision_adjoint_models(ts, Gc, plan.cut, gR, gO, need_ts)
                    if need_G:
                        gG.append(gGc)
                    if need_ts:
                        gts = gtsc if gts is None else gts + gtsc          # chunks in ascending order
    gG, gv = (_cat_chunks(p) if p else None for p in (gG, gv))
    gterm, grows = (_cat_chunks(p) if p and p[0] is not None else None for p in (gterm, grows))
    return gts, gG, gterm, grows, gv, gq


def _reductions_by_source(forms, ts, G, source, term, rows, v, q, plan):
    """The public reductions of this source (``forms``: the plain, _obs and _w function), so that an autograd forward
    checks its operands exactly as a direct call does."""
    if rows is None:
        return forms[source](ts, G, term, v, q, plan)
    return forms[source](ts, G, term, rows, v, q, plan)


class _LegModelsFn(torch.autograd.Function):
    """``apply(ts, G, term, rows, v, q, source, plan)``, with (source, term, rows) as in ``_leg_pair_raw`` and, for M
    models over the batch, a leading model axis on G, term, v, q and on the weights.  Forward: the batched reductions of
    that source, every (model, series) in one launch.  Backward: ``_models_backward``.  ``rows`` gets a gradient for the
    weighted source alone."""

    @staticmethod
    def forward(ctx, ts, G, term, rows, v, q, source, plan):
        ctx.plan, ctx.source = plan, source
        ctx.save_for_backward(ts, G, term, rows, v)
        forms = ((leg_loglik_models_reductions, leg_loglik_models_reductions_obs, leg_loglik_models_reductions_w)
                 if G.dim() == 3 else
                 (leg_loglik_batch_reductions, leg_loglik_batch_reductions_obs, leg_loglik_batch_reductions_w))
        out, info = _reductions_by_source(forms, ts.detach(), G.detach(), source, term.detach(),
                                          None if rows is None else rows.detach(), v.detach(), q.detach(), plan)
        if cr.CHECK_POSITIVE_DEFINITE:
            _raise_not_pd(info)
        return out.to(G.dtype)

    @staticmethod
    def backward(ctx, gout):
        ts, G, term, rows, v = ctx.saved_tensors
        return _models_backward(ctx.needs_input_grad[:6], ctx.plan, ctx.source, ts, G, term, rows, v, gout) + (None, None)


def _log_likelihood_per_series(m, ts, xs, lengths, observed=None, noise_var=None):
    """One ``log_likelihood`` per series: d = 8, fp64 d = 6 and CPU tensors (no batched kernel there)."""
    outs, s = [], 0
    for b, n in enumerate(lengths):
        try:
            outs.append(log_likelihood(m, ts[s:s + n], xs[s:s + n], None if observed is None else observed[s:s + n],
                                       None if noise_var is None else noise_var[s:s + n]))
        except cr.NotPSDError as e:
            raise cr.NotPSDError("LEG batch: series %d: %s" % (b, e)) from None
        s += n
    return torch.stack(outs)


_OBSERVED = ("observed", "a bool tensor", lambda dtype: dtype == torch.bool)
_NOISE_VAR = ("noise_var", "a floating-point tensor", lambda dtype: dtype.is_floating_point)


def _batch_like_xs(t, spec, xs_shape, dense):
    """``observed`` or ``noise_var`` (``spec``: its name, what it must be, and the test of its dtype) in the layout of the
    batch's xs, flattened to the rows of the concatenated batch ([R, obs] or [R]); raises ValueError before anything is
    launched."""
    name, what, dtype_ok = spec
    if not isinstance(t, torch.Tensor) or not dtype_ok(t.dtype):
        raise ValueError("%s must be %s" % (name, what))
    xs_shape = tuple(xs_shape)
    if dense:
        if tuple(t.shape) not in (xs_shape, xs_shape[:2]):
            raise ValueError("dense layout wants %s[B, n, obs_dim] or %s[B, n] like xs %s, got %s"
                             % (name, name, xs_shape, tuple(t.shape)))
        return t.reshape((xs_shape[0] * xs_shape[1],) + tuple(t.shape[2:]))
    if tuple(t.shape) not in (xs_shape, xs_shape[:1]):
        raise ValueError("ragged layout wants %s[sum(lengths), obs_dim] or %s[sum(lengths)] like xs %s, got %s"
                         % (name, name, xs_shape, tuple(t.shape)))
    return t


def _batch_args(obs, ts, xs, lengths, observed, noise_var, flat=False):
    """Everything a batched call on a model of ``obs`` channels checks before it launches anything: (ts [R], xs [R, obs],
    lengths, observed [R, obs] or None, noise_var [R, obs] / [R] or None, dense, (B, n) of the dense layout or None).
    ``flat``: a wrong channel count prints the shape of xs [R, obs] (the text of the many-model calls), not the caller's."""
    dense = lengths is None
    xs_shape = tuple(xs.shape)
    ts, xs, lengths = _batch_layout(ts, xs, lengths)
    if observed is not None:
        observed = _batch_like_xs(observed, _OBSERVED, xs_shape, dense)
    if noise_var is not None:
        noise_var = _batch_like_xs(noise_var, _NOISE_VAR, xs_shape, dense)
    if xs.shape[1] != obs:
        raise ValueError("xs must have %d channels, got %s" % (obs, tuple(xs.shape) if flat else xs_shape))
    if observed is not None:
        observed = _observed_2d(observed, obs)
    return ts, xs, lengths, observed, noise_var, dense, (xs_shape[:2] if dense else None)


def log_likelihood_batch(m, ts, xs, lengths=None, observed=None, noise_var=None):
    """log p(xs_b | ts_b) of the LEG model for B independent series (models.py:301-372 for each), as a [B] tensor of
    the model's dtype; ``out.sum()`` is what a training step over the batch minimises.

    ``lengths=None``: the dense layout of the reference's dataset, ts[B, n] and xs[B, n, obs_dim].  Otherwise the
    ragged layout: ts[sum(lengths)], xs[sum(lengths), obs_dim], series b being rows offsets[b]:offsets[b+1];
    ``lengths`` is host data (a list or a CPU integer tensor, every length >= 1).  The time stamps of different
    series are independent.  Differentiable in N, R, B, Lambda (through ``m``), xs and ts, for any upstream
    gradient and any subset of trainable parameters.  On the GPU one launch for every series up to
    BATCH_MAX_ROWS rows (cgps_leg_loglik_batch) and a backward through the concatenated, decoupled system;
    d = 8, fp64 d = 6 and CPU tensors take one ``log_likelihood`` per series.  With
    ``cr.CHECK_POSITIVE_DEFINITE`` a series that is not positive definite raises ``NotPSDError`` naming it; without
    it its slot is NaN and no other slot is affected.

    ``observed`` (bool, in the layout of xs: [B, n, obs_dim] or [B, n] for whole rows; ragged [sum(lengths), obs_dim]
    or [sum(lengths)]; None: everything, and exactly the calls above): every slot is the density of that series'
    observed entries alone, as ``log_likelihood(..., observed=)`` gives it.  Entries of xs that are not observed are
    ignored whatever they hold (NaN included); a row that observes nothing is marginalised out exactly, so a dense
    batch of series of unequal true length is the mask whose tail rows are False (the padded time stamps must still
    increase); a series that observes nothing at all has log-likelihood 0.  Still one launch
    (cgps_leg_loglik_batch_obs; ``observation_tables`` for the operands), the same gradients, the same fallbacks and
    errors, and nothing read on the host when ``cr.CHECK_POSITIVE_DEFINITE`` is off.

    ``noise_var`` (floating point, >= 0, in the layout of xs: [B, n, obs_dim] or [B, n] for one value per row; ragged
    [sum(lengths), obs_dim] or [sum(lengths)]; None: none, and exactly the calls above): per-point error bars, every
    slot being what ``log_likelihood(..., noise_var=)`` gives for that series -- the noise covariance of row i is
    Lambda Lambda^T + 1e-9 I + diag(noise_var[i]).  Combines with ``observed``; entries of noise_var that are not
    observed are ignored whatever they hold (NaN included).  Still one launch (cgps_leg_loglik_batch_w: every row's term
    is built in registers from obs_dim (obs_dim + 1) / 2 numbers; ``observation_weights`` for the operands),
    differentiable in noise_var as well, the same fallbacks and errors, and nothing read on the host when
    ``cr.CHECK_POSITIVE_DEFINITE`` is off."""
    if observed is None and noise_var is None:
        ts, xs, lengths = _batch_layout(ts, xs, lengths)
    else:
        ts, xs, lengths, observed, noise_var = _batch_args(m.B.shape[0], ts, xs, lengths, observed, noise_var)[:5]
    G = m.G
    dt = G.dtype
    if not lengths:
        return torch.empty(0, dtype=dt, device=ts.device)
    if not batch_supported(ts, G):
        return _log_likelihood_per_series(m, ts, xs, lengths, observed, noise_var)
    if noise_var is not None:
        plan = _cached_batch_plan(lengths, G.device)
        basis, weights, c_rows, xl, xz = _noise_operands(m, ts, xs, observed, noise_var)
        v = (xl @ m.B).to(dt).contiguous()
        q = ((xl * xz).sum(-1) + c_rows).to(dt).contiguous()             # the observation constant rides in sum q
        source, term, rows = _hip.ROWS_WEIGHTED, basis.to(dt).contiguous(), weights.to(dt).contiguous()
    elif observed is not None:
        plan = _cached_batch_plan(lengths, G.device)
        pattern, idx, A_table, c_table, xl, xz = _observed_operands(m, ts, xs, observed)
        v = (xl @ m.B).to(dt).contiguous()
        q = ((xl * xz).sum(-1) + c_table[idx]).to(dt).contiguous()       # the observation constant rides in sum q
        source, term, rows = _hip.ROWS_TABLE, A_table.to(dt).contiguous(), pattern
    else:
        plan = _BatchPlan(lengths, G.device)
        LLT = m.LLT
        Li = m.inv_of(LLT)
        xl = xs @ Li
        v = (xl @ m.B).to(dt).contiguous()
        q = (xl * xs).sum(-1).to(dt).contiguous()
        source, term, rows = _hip.ROWS_PLAIN, (m.B.T @ Li @ m.B).to(dt).contiguous(), None
    red = _LegModelsFn.apply(ts.to(dt).contiguous(), G.contiguous(), term, rows, v, q, source, plan)
    if source == _hip.ROWS_PLAIN:
        llt_det = torch.log(2 * math.pi * LLT[0, 0]) if LLT.shape[0] == 1 else torch.logdet(2 * math.pi * LLT)
        n = plan.lens.to(dt)
        return -0.5 * ((red[:, 3] - red[:, 0]) + (n * llt_det + red[:, 1] - red[:, 2]))
    return -0.5 * ((red[:, 3] - red[:, 0]) + (red[:, 1] - red[:, 2]))


# ---- many models over one batch ------------------------------------------------------------------------------------
# The other axis of the batch: M parameter sets (the starts of a fit, a population of chains, a grid of length scales,
# the components of a mixture) on the same B series.  Forward: grid (B, 2, M) of cgps_leg_loglik_models, one launch.
# Backward: the block-diagonal system "model 0's batch, then model 1's batch, ..." of M R rows, assembled by
# cgps_peg_precision_models from the one ts and the M generators, and its adjoint cgps_peg_precision_adjoint_models.
def _contract(a, b):
    """a [..., p, q] times b [..., q, r] for a small q, as q outer products added up in ascending order with plain
    elementwise multiplies and adds: every entry is rounded the same way whatever the other dimensions are, so a
    model's operands do not depend on how many models or rows stand next to them (a batched GEMM may pick another
    kernel, and another order of summation, for another batch size)."""
    out = a[..., :, 0, None] * b[..., 0, None, :]
    for j in range(1, a.shape[-1]):
        out = out + a[..., :, j, None] * b[..., j, None, :]
    return out


def _spd_inverse_logdet(S):
    """(S^-1, log|S|) of symmetric positive definite S [M, o, o] for a small o, by Gauss-Jordan elimination without
    pivoting in elementwise operations over the models: as ``_contract``, nothing a model gets depends on its
    neighbours (a batched factorisation may take another route for another batch size), and nothing is read on the
    host.  Differentiable."""
    M, o = S.shape[0], S.shape[1]
    aug = torch.cat([S, torch.eye(o, dtype=S.dtype, device=S.device).expand(M, o, o)], -1)
    logdet = None
    for j in range(o):
        piv = aug[:, j, j]
        logdet = torch.log(piv) if logdet is None else logdet + torch.log(piv)
        row = aug[:, j, :] / piv.unsqueeze(-1)
        aug = aug - aug[:, :, j, None] * row.unsqueeze(1)        # clears column j everywhere, row j included
        aug = torch.cat([aug[:, :j], row.unsqueeze(1), aug[:, j + 1:]], 1)
    return aug[:, :, o:], logdet


def _check_models_rhs(v, q, M, R, d):
    if tuple(v.shape) != (M, R, d) or tuple(q.shape) != (M, R):
        raise ValueError("v must be [%d, %d, %d] and q [%d, %d], got %s and %s"
                         % (M, R, d, M, R, tuple(v.shape), tuple(q.shape)))


def leg_loglik_models_reductions(ts, G, A, v, q, plan):
    """``leg_loglik_batch_reductions`` for M models over the same batch, no autograd graph: [M, B, 4] fp64 and [M, B, 2]
    info words from one launch (cgps_leg_loglik_models; series longer than BATCH_MAX_ROWS through
    cgps_leg_mahal_logdet_pair per model and series on the same stream).  ts [R]; G, A [M, d, d]; v [M, R, d];
    q [M, R]; all in G's dtype, contiguous."""
    return _leg_rows_reductions(ts, G, _hip.ROWS_PLAIN, A, None, v, q, plan)


def leg_loglik_models_reductions_obs(ts, G, A_table, pattern, v, q, plan):
    """``leg_loglik_models_reductions`` of series whose rows observe different channels, still ONE launch
    (cgps_leg_loglik_models_obs): the mask belongs to the data, so ``pattern`` (uint8 [R] on the device, a byte >= P takes
    the last entry) is shared by the models and every model brings a table of its own, A_table [M, P, d, d] with
    1 <= P <= 256.  ts [R]; G [M, d, d]; v [M, R, d]; q [M, R]; all in G's dtype, contiguous.  Series longer than
    BATCH_MAX_ROWS through cgps_leg_mahal_logdet_pair_obs per model and series.  No autograd graph."""
    M, d, dt = G.shape[0], G.shape[1], G.dtype
    _check_pattern(pattern, plan.R)
    if A_table.dim() != 4 or A_table.shape[0] != M or tuple(A_table.shape[2:]) != (d, d) or not 1 <= A_table.shape[1] <= 256:
        raise ValueError("A_table must be [%d, P, %d, %d] with 1 <= P <= 256, got %s" % (M, d, d, tuple(A_table.shape)))
    _check_models_rhs(v, q, M, plan.R, d)
    if A_table.dtype != dt or not A_table.is_cuda:
        raise ValueError("A_table must be a device tensor of G's dtype %s, got %s" % (dt, A_table.dtype))
    return _leg_rows_reductions(ts, G, _hip.ROWS_TABLE, A_table.contiguous(), pattern.contiguous(), v, q, plan)


def leg_loglik_models_reductions_w(ts, G, basis, weights, v, q, plan):
    """``leg_loglik_models_reductions`` of series whose rows each add a term of their own, still ONE launch
    (cgps_leg_loglik_models_w): K of (model k, series b) = PEG precision(ts_b, G[k]) + blockdiag(sum_j weights[k, i, j]
    basis[k, j]) over the series' rows.  basis [M, Kb, d, d] with 1 <= Kb <= 64 and weights [M, R, Kb] (the entries of
    each model's own inverse noise covariance), device tensors of G's dtype.  ts [R]; G [M, d, d]; v [M, R, d]; q [M, R];
    contiguous.  Series longer than BATCH_MAX_ROWS through cgps_leg_mahal_logdet_pair_w per model and series.  No
    autograd graph."""
    M, d, dt = G.shape[0], G.shape[1], G.dtype
    if basis.dim() != 4 or basis.shape[0] != M or tuple(basis.shape[2:]) != (d, d) or not 1 <= basis.shape[1] <= 64:
        raise ValueError("basis must be [%d, Kb, %d, %d] with 1 <= Kb <= 64, got %s" % (M, d, d, tuple(basis.shape)))
    Kb = basis.shape[1]
    if tuple(weights.shape) != (M, plan.R, Kb):
        raise ValueError("weights must be [%d, %d, %d] (Kb weights per model and row of the batch), got %s"
                         % (M, plan.R, Kb, tuple(weights.shape)))
    _check_models_rhs(v, q, M, plan.R, d)
    _check_basis_weights(basis, weights, dt)
    return _leg_rows_reductions(ts, G, _hip.ROWS_WEIGHTED, basis.contiguous(), weights.contiguous(), v, q, plan)


def _models_pattern_tables(Bm, LLT, o, dt):
    """``observation_tables`` for stacked models, elementwise over the models: (Li_table [M, P, o, o], A_table
    [M, P, d, d], c_table [M, P]) for the P = 2^obs patterns."""
    M = Bm.shape[0]
    Mt = _pattern_mask_table(o, dt, Bm.device)                           # [P, o]
    unobs = torch.diag_embed(1 - Mt)
    W = Mt.unsqueeze(2) * LLT.unsqueeze(1) * Mt.unsqueeze(1) + unobs     # [M, P, o, o]
    Wi, logdet_W = _spd_inverse_logdet(W.reshape(-1, o, o))
    Li_table = Wi.view(M, -1, o, o) - unobs
    A_table = _contract(_contract(Bm.transpose(1, 2).unsqueeze(1), Li_table), Bm.unsqueeze(1))
    c_table = Mt.sum(1) * math.log(2 * math.pi) + logdet_W.view(M, -1)
    return Li_table, A_table, c_table


def _models_noise_rows(Bm, LLT, o, dt, observed, noise_var):
    """``observation_weights`` for stacked models, elementwise over models and rows: (basis [M, Kb, d, d], weights
    [M, R, Kb], Li_rows [M, R, o, o], c_rows [M, R]).  observed bool [R, o] or None; noise_var [R, o] or [R]."""
    M = Bm.shape[0]
    if noise_var.dim() == 1:
        noise_var = noise_var.unsqueeze(-1).expand(-1, o)
    s = noise_var.to(dt)
    if observed is None:
        Mt = torch.ones((), dtype=dt, device=Bm.device).expand(s.shape)
    else:
        s = torch.where(observed, s, torch.zeros((), dtype=dt, device=s.device))
        Mt = observed.to(dt)
    unobs = torch.diag_embed(1 - Mt)                                     # [R, o, o]
    W = Mt.unsqueeze(2) * (LLT.unsqueeze(1) + torch.diag_embed(s)) * Mt.unsqueeze(1) + unobs     # [M, R, o, o]
    Wi, logdet_W = _spd_inverse_logdet(W.reshape(-1, o, o))
    Li_rows = Wi.view(M, -1, o, o) - unobs
    c_rows = Mt.sum(1) * math.log(2 * math.pi) + logdet_W.view(M, -1)
    ci, cj, same = _tril_pairs(o, Bm.device)
    outer = Bm[:, ci].unsqueeze(3) * Bm[:, cj].unsqueeze(2)              # b_c b_c'^T per model
    basis = torch.where(same, outer, outer + outer.transpose(2, 3))
    weights = Li_rows[:, :, ci, cj]
    return basis, weights, Li_rows, c_rows


def _models_operands(ms):
    """The models' matrices stacked: (N, R, B, Lambda) as [M, ...]; ValueError unless they share rank, obs_dim, dtype
    and device."""
    ms = list(ms)
    if not ms:
        raise ValueError("log_likelihood_models wants at least one model")
    for k, m in enumerate(ms):
        if not isinstance(m, LEGMatrices):
            raise ValueError("model %d is not a LEGMatrices" % k)
        for name in ("N", "R", "B", "Lambda"):
            a, b = getattr(m, name), getattr(ms[0], name)
            if tuple(a.shape) != tuple(b.shape) or a.dtype != b.dtype or a.device != b.device:
                raise ValueError("model %d: %s is %s %s on %s, model 0 has %s %s on %s (the models must share rank, obs_dim, "
                                 "dtype and device)" % (k, name, tuple(a.shape), a.dtype, a.device, tuple(b.shape), b.dtype,
                                                        b.device))
    m0 = ms[0]
    d, o = m0.N.shape[0], m0.B.shape[0]
    if (tuple(m0.N.shape) != (d, d) or tuple(m0.R.shape) != (d, d) or tuple(m0.B.shape) != (o, d)
            or tuple(m0.Lambda.shape) != (o, o)):
        raise ValueError("a model wants N [d, d], R [d, d], B [obs, d] and Lambda [obs, obs], got %s, %s, %s, %s"
                         % tuple(tuple(t.shape) for t in (m0.N, m0.R, m0.B, m0.Lambda)))
    if len({t.dtype for t in (m0.N, m0.R, m0.B, m0.Lambda)}) != 1 or len({t.device for t in (m0.N, m0.R, m0.B, m0.Lambda)}) != 1:
        raise ValueError("a model's four matrices must share dtype and device")
    return ms, tuple(torch.stack([getattr(m, name) for m in ms]) for name in ("N", "R", "B", "Lambda"))


def _models_args(ms, ts, xs, lengths, observed, noise_var):
    """``_batch_args`` of a call over many models: (ms, (N, R, B, Lambda) stacked), then its seven values."""
    ms, mats = _models_operands(ms)
    return (ms, mats) + _batch_args(mats[2].shape[1], ts, xs, lengths, observed, noise_var, flat=True)


def _models_setup(ms, ts, xs, lengths, observed=None, noise_var=None):
    """What ``log_likelihood_models`` and ``log_likelihood_models_observed`` do first: the stacked matrices, the layout and
    its checks, and the two ways a call ends early -- an empty batch, and the block sizes and devices without a batched
    kernel, which take one ``log_likelihood_batch`` per model.  Returns (result, None) then, and otherwise
    (None, (ts, xs, observed, noise_var, plan, Bm, G, LLT)) with xs [R, obs], observed [R, obs] or None, noise_var [R, obs],
    [R] or None, and the models' G [M, d, d] and LLT [M, obs, obs]."""
    ms, (Nm, Rm, Bm, Lm), ts, xs, lengths, observed, noise_var = _models_args(ms, ts, xs, lengths, observed, noise_var)[:7]
    M, d, o, dt = len(ms), Nm.shape[1], Bm.shape[1], Nm.dtype
    if not lengths:
        return torch.empty(M, 0, dtype=dt, device=ts.device), None
    if not batch_supported(ts, Nm[0]):
        outs = []
        for k, m in enumerate(ms):
            try:
                outs.append(log_likelihood_batch(m, ts, xs, lengths, observed, noise_var))
            except cr.NotPSDError as e:
                raise cr.NotPSDError("LEG models: model %d: %s" % (k, e)) from None
        return torch.stack(outs), None
    if (observed is not None or noise_var is not None) and o > MAX_PATTERN_OBS:
        raise ValueError("observation patterns are tabulated for obs_dim <= %d, got %d" % (MAX_PATTERN_OBS, o))
    plan = _cached_batch_plan(lengths, Nm.device)
    G = _contract(Nm, Nm.transpose(1, 2)) + (Rm - Rm.transpose(1, 2)) + _scaled_eye(d, 1e-5, dt, Nm.device)
    LLT = _contract(Lm, Lm.transpose(1, 2)) + _scaled_eye(o, 1e-9, dt, Nm.device)
    return None, (ts, xs, observed, noise_var, plan, Bm, G, LLT)


def log_likelihood_models(ms, ts, xs, lengths=None):
    """log p(xs_b | ts_b) of M LEG models for the same B series, as an [M, B] tensor of the models' dtype: entry (k, b)
    is ``log_likelihood(ms[k], series b)``.  What several starts of a fit, a population of chains, a grid of length
    scales or the responsibilities of a mixture of LEG processes evaluate.

    ``ms``: a non-empty sequence of ``LEGMatrices`` of one rank, obs_dim, dtype and device (ValueError otherwise, before
    anything is launched).  ``ts`` / ``xs`` / ``lengths``: the two layouts of ``log_likelihood_batch``.  An empty batch
    gives an [M, 0] tensor.  Differentiable in every model's N, R, B, Lambda, in xs and in ts, for any upstream
    gradient and any subset of trainable tensors.  On the GPU one launch for all models and all series up to
    BATCH_MAX_ROWS rows (cgps_leg_loglik_models), longer series per (model, series) through
    cgps_leg_mahal_logdet_pair, and a backward through the concatenated system of all models' batches in chunks of
    MODELS_BACKWARD_MAX_ROWS rows; a repeated call with the same lengths copies nothing from the host.  d = 8, fp64
    d = 6 and CPU tensors take one ``log_likelihood_batch`` per model.  With ``cr.CHECK_POSITIVE_DEFINITE`` a system
    that is not positive definite raises ``NotPSDError`` naming its model and series; without it that slot is NaN and
    no other slot is affected."""
    out, operands = _models_setup(ms, ts, xs, lengths)
    if operands is None:
        return out
    ts, xs, _, _, plan, Bm, G, LLT = operands
    o, dt = Bm.shape[1], Bm.dtype
    Li, llt_det = _spd_inverse_logdet(LLT)
    llt_det = llt_det + o * math.log(2 * math.pi)
    xl = _contract(xs.unsqueeze(0), Li)                   # [M, R, obs]
    v = _contract(xl, Bm).to(dt).contiguous()             # [M, R, d]
    q = xl[..., 0] * xs[:, 0]
    for c in range(1, o):
        q = q + xl[..., c] * xs[:, c]
    A = _contract(_contract(Bm.transpose(1, 2), Li), Bm).to(dt).contiguous()
    red = _LegModelsFn.apply(ts.to(dt).contiguous(), G.contiguous(), A, None, v, q.to(dt).contiguous(), _hip.ROWS_PLAIN, plan)
    n = plan.lens.to(dt)
    return -0.5 * ((red[..., 3] - red[..., 0]) + (n * llt_det.unsqueeze(1) + red[..., 1] - red[..., 2]))


def log_likelihood_models_observed(ms, ts, xs, lengths=None, observed=None, noise_var=None):
    """``log_likelihood_models`` for data with missing observations and per-point noise: the [M, B] tensor whose entry
    (k, b) is ``log_likelihood_batch(ms[k], ..., observed=, noise_var=)[b]``.  (An entry point of its own:
    ``log_likelihood_models`` keeps its four arguments, and refuses these two keywords, as its callers and tests know it.)

    ``ms``, ``ts`` / ``xs`` / ``lengths``: those of ``log_likelihood_models``.  ``observed`` and ``noise_var``: those of
    ``log_likelihood_batch``, in the layout of xs, with the same checks.  The mask and the variances belong to the data,
    so all models share them.  Unobserved entries of xs and noise_var are ignored whatever they hold (NaN included), a
    row that observes nothing is marginalised out, a series that observes nothing gives 0, and a dense padded batch is
    the mask whose tail rows are False.  Still one launch: with ``observed`` alone cgps_leg_loglik_models_obs (one
    pattern byte per row for the batch, a table of 2^obs_dim diagonal terms per model), with ``noise_var``
    cgps_leg_loglik_models_w (obs_dim (obs_dim + 1) / 2 weights per model and row).  Differentiable as
    ``log_likelihood_models`` is, and in ``noise_var`` as well; the same fallbacks (d = 8, fp64 d = 6 and CPU tensors
    take one ``log_likelihood_batch(observed=, noise_var=)`` per model) and errors; nothing read on the host when
    ``cr.CHECK_POSITIVE_DEFINITE`` is off.  With both None the call is ``log_likelihood_models(ms, ts, xs, lengths)``."""
    if observed is None and noise_var is None:
        return log_likelihood_models(ms, ts, xs, lengths)
    out, operands = _models_setup(ms, ts, xs, lengths, observed, noise_var)
    if operands is None:
        return out
    ts, xs, observed, noise_var, plan, Bm, G, LLT = operands
    o, dt = Bm.shape[1], Bm.dtype
    xz = xs if observed is None else torch.where(observed, xs, torch.zeros((), dtype=xs.dtype, device=xs.device))
    if noise_var is not None:
        basis, weights, Li_rows, c = _models_noise_rows(Bm, LLT, o, dt, observed, noise_var)
    else:
        weights_c = 1 << torch.arange(o, device=observed.device)
        pattern = (observed * weights_c).sum(1).to(torch.uint8)
        idx = pattern.long()
        Li_table, A_table, c_table = _models_pattern_tables(Bm, LLT, o, dt)
        Li_rows, c = Li_table[:, idx], c_table[:, idx]
    xl = _contract(xz.unsqueeze(0).unsqueeze(2), Li_rows).squeeze(2)        # x~^T Li per model and row: [M, R, obs]
    v = _contract(xl, Bm).to(dt).contiguous()
    q = xl[..., 0] * xz[:, 0]
    for ch in range(1, o):
        q = q + xl[..., ch] * xz[:, ch]
    q = (q + c).to(dt).contiguous()                       # the observation constant rides in sum q
    if noise_var is not None:
        source, term, rows = _hip.ROWS_WEIGHTED, basis.to(dt).contiguous(), weights.to(dt).contiguous()
    else:
        source, term, rows = _hip.ROWS_TABLE, A_table.to(dt).contiguous(), pattern
    red = _LegModelsFn.apply(ts.to(dt).contiguous(), G.contiguous(), term, rows, v, q, source, plan)
    return -0.5 * ((red[..., 3] - red[..., 0]) + (red[..., 1] - red[..., 2]))


# ---- missing observations ------------------------------------------------------------------------------------------
# A row that observes the channels S only contributes B^T Li B to its diagonal block of the posterior precision, with
# Li = (LLT[S, S])^-1 embedded in zeros (zero when S is empty); everything after the assembly -- factor, solve, selected
# inverse, sampler -- is unchanged.  All 2^obs patterns form one small batched table; a row names its entry by the
# code sum_c observed[i, c] 2^c, computed on the device: nothing here reads a device value on the host.
MAX_PATTERN_OBS = 8

_pattern_masks = {}


def _pattern_mask_table(obs, dtype, device):
    """[2^obs, obs]: row p holds the bits of p (bit c = channel c observed), built once per (obs, dtype, device)."""
    key = (obs, dtype, device)
    t = _pattern_masks.get(key)
    if t is None:
        codes = torch.arange(1 << obs, device=device)
        t = _pattern_masks[key] = ((codes.unsqueeze(1) >> torch.arange(obs, device=device)) & 1).to(dtype)
    return t


def _observed_2d(observed, obs):
    if not isinstance(observed, torch.Tensor) or observed.dtype != torch.bool:
        raise ValueError("observed must be a bool tensor")
    if observed.dim() == 1:
        return observed.unsqueeze(-1).expand(-1, obs)
    if observed.dim() != 2 or observed.shape[1] != obs:
        raise ValueError("observed must be [n] or [n, %d] (one flag per row or per observed channel), got %s"
                         % (obs, tuple(observed.shape)))
    return observed


def observation_tables(m, observed):
    """What rows with missing observations need, for every pattern at once: ``(pattern, A_table, Li_table, c_table)``.

    ``observed``: bool [n, obs_dim], or [n] for whole rows.  With M = diag(mask of pattern p), S its observed channels
    and LLT = Lambda Lambda^T + 1e-9 I:  W = M LLT M + (I - M),  Li_table[p] = W^-1 - (I - M)  (= (LLT[S, S])^-1 embedded
    in zeros),  A_table[p] = B^T Li_table[p] B,  c_table[p] = |S| log 2 pi + log|W|  (log|W| = log|LLT[S, S]|);
    pattern[i] = sum_c observed[i, c] 2^c as uint8.  P = 2^obs_dim entries, obs_dim <= 8.  Batched torch ops,
    differentiable in B and Lambda, nothing read on the host."""
    obs = m.B.shape[0]
    if obs > MAX_PATTERN_OBS:
        raise ValueError("observation patterns are tabulated for obs_dim <= %d, got %d" % (MAX_PATTERN_OBS, obs))
    observed = _observed_2d(observed, obs)
    dt, dev = m.B.dtype, m.B.device
    Mt = _pattern_mask_table(obs, dt, dev)
    LLT = m.LLT
    if obs == 1:                                        # a single output: no factorisation call, the scalar log
        W = Mt * LLT[0, 0] + (1 - Mt)                   # [2, 1]
        Li_table = (1.0 / W - (1 - Mt)).unsqueeze(-1)
        logdet_W = torch.log(W[:, 0])
    else:
        unobs = torch.diag_embed(1 - Mt)
        W = Mt.unsqueeze(2) * LLT * Mt.unsqueeze(1) + unobs
        Li_table = torch.linalg.inv_ex(W)[0] - unobs    # the inverse's backward is matmul only (see LLT_inv); no host check
        logdet_W = torch.logdet(W)
    A_table = m.B.T @ Li_table @ m.B
    c_table = Mt.sum(1) * math.log(2 * math.pi) + logdet_W
    weights = 1 << torch.arange(obs, device=observed.device)
    pattern = (observed * weights).sum(1).to(torch.uint8)
    return pattern, A_table, Li_table, c_table


def _observed_operands(m, ts, xs, observed):
    """(pattern, row index into the tables, A_table, c_table, x~ Li per row, x~) with x~ = xs where observed, 0 elsewhere
    (whatever the unobserved entries hold, NaN included)."""
    if xs.dim() != 2 or xs.shape[1] != m.B.shape[0]:
        raise ValueError("xs must be [n, %d], got %s" % (m.B.shape[0], tuple(xs.shape)))
    observed = _observed_2d(observed, xs.shape[1])
    if not (observed.shape[0] == xs.shape[0] == ts.shape[0]):
        raise ValueError("observed has %d rows, xs has %d, ts has %d" % (observed.shape[0], xs.shape[0], ts.shape[0]))
    pattern, A_table, Li_table, c_table = observation_tables(m, observed)
    xz = torch.where(observed, xs, torch.zeros((), dtype=xs.dtype, device=xs.device))
    idx = pattern.long()
    xl = (xz.unsqueeze(1) @ Li_table[idx]).squeeze(1)           # x~^T Li(m_i): Li is symmetric
    return pattern, idx, A_table, c_table, xl, xz


# ---- per-observation noise variances ---------------------------------------------------------------------------
# Entry c of row i carries extra independent noise of variance s_ic >= 0: the row's noise covariance is LLT + diag(s_i),
# so its Li has no finite table.  But A_i = B^T Li_i B is a weighted sum of obs (obs + 1) / 2 blocks shared by all rows
# (the symmetrised outer products of B's rows), weighted by the entries of Li_i: the fused kernel gets the basis once
# and Kb numbers per row.
_tril = {}


def _tril_pairs(obs, device):
    """(c, c') of the pairs c >= c' in row-major order over the lower triangle, built once per (obs, device)."""
    key = (obs, device)
    t = _tril.get(key)
    if t is None:
        ij = torch.tril_indices(obs, obs, device=device)
        t = _tril[key] = (ij[0], ij[1], (ij[0] == ij[1]).view(-1, 1, 1))
    return t


def observation_weights(m, observed, noise_var):
    """What rows with noise variances of their own need: ``(basis, weights, Li_rows, c_rows)``.

    ``noise_var``: [n, obs_dim] variances s_ic >= 0 of independent noise added to entry c of row i, or [n] for the same
    value in every channel of a row.  ``observed``: bool [n, obs_dim], [n] for whole rows, or None (everything).  With
    M_i = diag(observed_i), S_i its observed channels and C_i = Lambda Lambda^T + 1e-9 I + diag(s_i):
    W_i = M_i C_i M_i + (I - M_i),  Li_rows[i] = W_i^-1 - (I - M_i)  (= (C_i[S_i, S_i])^-1 embedded in zeros),
    c_rows[i] = |S_i| log 2 pi + log|W_i|.  The pairs c >= c' of channels, in row-major order over the lower triangle,
    index Kb = obs_dim (obs_dim + 1) / 2 entries:  basis[k] = b_c b_c^T (c = c') or b_c b_c'^T + b_c' b_c^T (c > c'), b_c
    row c of B, and weights[i, k] = Li_rows[i][c, c'], so that  sum_k weights[i, k] basis[k] = B^T Li_rows[i] B.
    ``noise_var`` at entries that are not observed is ignored whatever it holds (NaN included).  Values are not checked:
    a negative or non-finite variance at an observed entry surfaces as NotPSDError or NaN downstream, like a
    zero-length gap -- mark missing data with ``observed``, not with an infinite variance.  obs_dim <= 8.  Batched
    torch ops, differentiable in B, Lambda and noise_var, nothing read on the host."""
    obs = m.B.shape[0]
    if obs > MAX_PATTERN_OBS:
        raise ValueError("per-row observation terms are built for obs_dim <= %d, got %d" % (MAX_PATTERN_OBS, obs))
    if not isinstance(noise_var, torch.Tensor) or not noise_var.dtype.is_floating_point:
        raise ValueError("noise_var must be a floating-point tensor")
    if noise_var.dim() == 1:
        noise_var = noise_var.unsqueeze(-1).expand(-1, obs)
    if noise_var.dim() != 2 or noise_var.shape[1] != obs:
        raise ValueError("noise_var must be [n] or [n, %d] (one variance per row or per observed channel), got %s"
                         % (obs, tuple(noise_var.shape)))
    dt, dev = m.B.dtype, m.B.device
    s = noise_var.to(dt)
    if observed is None:
        Mt = torch.ones((), dtype=dt, device=dev).expand(s.shape)
    else:
        observed = _observed_2d(observed, obs)
        if observed.shape[0] != s.shape[0]:
            raise ValueError("observed has %d rows, noise_var has %d" % (observed.shape[0], s.shape[0]))
        s = torch.where(observed, s, torch.zeros((), dtype=dt, device=s.device))
        Mt = observed.to(dt)
    LLT = m.LLT
    if obs == 1:                                        # a single output: no factorisation call, the scalar log
        W = Mt * (LLT[0, 0] + s) + (1 - Mt)             # [n, 1]
        Li_rows = (1.0 / W - (1 - Mt)).unsqueeze(-1)
        logdet_W = torch.log(W[:, 0])
    else:
        unobs = torch.diag_embed(1 - Mt)
        W = Mt.unsqueeze(2) * (LLT + torch.diag_embed(s)) * Mt.unsqueeze(1) + unobs
        Li_rows = torch.linalg.inv_ex(W)[0] - unobs     # the inverse's backward is matmul only (see LLT_inv); no host check
        logdet_W = torch.logdet(W)
    c_rows = Mt.sum(1) * math.log(2 * math.pi) + logdet_W
    ci, cj, same = _tril_pairs(obs, dev)
    outer = m.B[ci].unsqueeze(2) * m.B[cj].unsqueeze(1)  # b_c b_c'^T
    basis = torch.where(same, outer, outer + outer.transpose(1, 2))
    weights = Li_rows[:, ci, cj]
    return basis, weights, Li_rows, c_rows


def _noise_operands(m, ts, xs, observed, noise_var):
    """(basis, weights, c_rows, x~ Li per row, x~) with x~ = xs where observed, 0 elsewhere."""
    if xs.dim() != 2 or xs.shape[1] != m.B.shape[0]:
        raise ValueError("xs must be [n, %d], got %s" % (m.B.shape[0], tuple(xs.shape)))
    if not isinstance(noise_var, torch.Tensor) or noise_var.dim() not in (1, 2):
        raise ValueError("noise_var must be a tensor of shape [n] or [n, %d]" % xs.shape[1])
    if not (noise_var.shape[0] == xs.shape[0] == ts.shape[0]):
        raise ValueError("noise_var has %d rows, xs has %d, ts has %d" % (noise_var.shape[0], xs.shape[0], ts.shape[0]))
    if observed is not None:
        observed = _observed_2d(observed, xs.shape[1])
        if observed.shape[0] != xs.shape[0]:
            raise ValueError("observed has %d rows, xs has %d" % (observed.shape[0], xs.shape[0]))
    basis, weights, Li_rows, c_rows = observation_weights(m, observed, noise_var)
    xz = xs if observed is None else torch.where(observed, xs, torch.zeros((), dtype=xs.dtype, device=xs.device))
    xl = (xz.unsqueeze(1) @ Li_rows).squeeze(1)                 # x~^T Li_i: Li is symmetric
    return basis, weights, c_rows, xl, xz


def _chol_forward(W, Y):
    """T^-1 Y [..., obs, k] for the lower Cholesky factor T of W [..., obs, obs], obs <= 8: the obs steps of the
    factorisation and of the forward substitution as batched elementwise ops -- no factorisation call, nothing read on
    the host (capturable).  A pivot that is not positive gives NaN, like the square root of a failed block elsewhere."""
    obs = W.shape[-1]
    L = torch.zeros_like(W)
    X = torch.empty_like(Y)
    for j in range(obs):
        lj = L[..., j, :j]
        ljj = torch.sqrt(W[..., j, j] - (lj * lj).sum(-1)).unsqueeze(-1)
        L[..., j, j:j + 1] = ljj
        if j + 1 < obs:
            L[..., j + 1:, j] = (W[..., j + 1:, j] - (L[..., j + 1:, :j] * lj.unsqueeze(-2)).sum(-1)) / ljj
        X[..., j, :] = (Y[..., j, :] - (lj.unsqueeze(-1) * X[..., :j, :]).sum(-2)) / ljj
    return X


def observation_noise_factors(m, observed=None, noise_var=None):
    """The factor H of a row's observation term, H H^T = B^T Li B, that perturb-and-solve sampling multiplies the row's
    observation noise with (``posterior_perturbation_batch``): H = B^T M T^-T [rank, obs_dim] with M = diag(observed),
    W = M (LLT + diag(s)) M + (I - M) -- exactly the W of ``observation_tables`` and ``observation_weights`` -- and T its
    lower Cholesky factor.  The column of an unobserved channel is exactly zero.  Neither argument: one block
    [rank, obs_dim].  ``observed`` alone (bool [n, obs_dim] or [n]): the table [2^obs_dim, rank, obs_dim] of all
    patterns, indexed by ``observation_tables``' pattern byte.  ``noise_var`` ([n, obs_dim] or [n]; with or without
    ``observed``): one block per row, [n, rank, obs_dim]; noise_var at unobserved entries is ignored, NaN included.
    obs_dim <= 8.  Batched torch ops, nothing read on the host, no factorisation call."""
    obs = m.B.shape[0]
    if obs > MAX_PATTERN_OBS:
        raise ValueError("observation noise factors are built for obs_dim <= %d, got %d" % (MAX_PATTERN_OBS, obs))
    dt, dev = m.B.dtype, m.B.device
    LLT = m.LLT
    if noise_var is None and observed is None:
        return _chol_forward(LLT, m.B).transpose(-1, -2).contiguous()
    if noise_var is None:
        _observed_2d(observed, obs)                                          # (its checks; every pattern is tabulated)
        Mt = _pattern_mask_table(obs, dt, dev)
        C = LLT
    else:
        if not isinstance(noise_var, torch.Tensor) or not noise_var.dtype.is_floating_point:
            raise ValueError("noise_var must be a floating-point tensor")
        s = noise_var.to(dt)
        if s.dim() == 1:
            s = s.unsqueeze(-1).expand(-1, obs)
        if s.dim() != 2 or s.shape[1] != obs:
            raise ValueError("noise_var must be [n] or [n, %d], got %s" % (obs, tuple(noise_var.shape)))
        if observed is None:
            Mt = torch.ones((), dtype=dt, device=dev).expand(s.shape)
        else:
            observed = _observed_2d(observed, obs)
            if observed.shape[0] != s.shape[0]:
                raise ValueError("observed has %d rows, noise_var has %d" % (observed.shape[0], s.shape[0]))
            s = torch.where(observed, s, torch.zeros((), dtype=dt, device=s.device))
            Mt = observed.to(dt)
        C = LLT + torch.diag_embed(s)
    W = Mt.unsqueeze(2) * C * Mt.unsqueeze(1) + torch.diag_embed(1 - Mt)
    return _chol_forward(W, Mt.unsqueeze(2) * m.B).transpose(-1, -2).contiguous()


def merge_targets(ts, xs, target_ts, check=True):
    """Insert the times ``target_ts`` [k] into the series as wholly unobserved rows: ``(ts_all [n + k], xs_all
    [n + k, obs], observed_all bool [n + k], target_index int64 [k])``, ts_all sorted (a stable sort on the device),
    target_index[j] the row of target j.  With ``observed=observed_all``, ``insample_posterior`` and
    ``sample_from_posterior`` then give posterior blocks, neighbouring cross-covariances and joint paths at times that
    have no data.  A target at an observation time makes a zero-length gap: ``check=True`` reads one flag on the host
    and raises ValueError; with ``check=False`` nothing is read (graph capture) and the singular gap surfaces as
    NotPSDError or NaN like any other."""
    n, k = ts.shape[0], target_ts.shape[0]
    ts_all, perm = torch.sort(torch.cat([ts, target_ts.to(dtype=ts.dtype, device=ts.device)]), stable=True)
    xs_all = torch.cat([xs, xs.new_zeros(k, xs.shape[1])])[perm]
    observed_all = perm < n
    where = torch.empty_like(perm)
    where[perm] = torch.arange(n + k, device=perm.device)
    if check and n + k > 1 and bool((ts_all[1:] == ts_all[:-1]).any()):
        raise ValueError("a target time coincides with another time of the series (zero-length gap)")
    return ts_all, xs_all, observed_all, where[n:]


def posterior_precision(m, ts):
    Rs, Os = peg_precision(ts, m.G)
    BtLB = m.B.T @ m.LLT_inv @ m.B
    return Rs + BtLB.unsqueeze(0), Os


def compute_v(m, xs):
    return (xs @ m.LLT_inv @ m.B).contiguous()


def _posterior_system(m, ts, xs, observed, noise_var=None):
    """(K_Rs, K_Os, v) of the posterior N(K^-1 v, K^-1); with ``observed``, row i adds A(m_i) and v_i = B^T Li(m_i) x~_i;
    with ``noise_var``, row i adds sum_k weights[i, k] basis[k] = B^T Li_i B and v_i = B^T Li_i x~_i."""
    if noise_var is not None:
        basis, weights, _, xl, _ = _noise_operands(m, ts, xs, observed, noise_var)
        Rs, Os = peg_precision(ts, m.G)
        return Rs + torch.einsum("nk,kij->nij", weights, basis), Os, (xl @ m.B).contiguous()
    if observed is None:
        return posterior_precision(m, ts) + (compute_v(m, xs),)
    _, idx, A_table, _, xl, _ = _observed_operands(m, ts, xs, observed)
    Rs, Os = peg_precision(ts, m.G)
    return Rs + A_table[idx], Os, (xl @ m.B).contiguous()


def _log_likelihood_observed(m, ts, xs, observed):
    """``log_likelihood`` with a per-row observation pattern:  -1/2 [sum q_i - v^T K^-1 v + sum c(m_i) + log|K| -
    log|Sigma^-1|],  K = PEG precision + blockdiag(A(m_i)),  v_i = B^T Li(m_i) x~_i,  q_i = x~_i^T Li(m_i) x~_i.

    fp32 with a gradient wanted: the observation-space terms (tables, x~ Li, v, q, c) are formed in fp64 and only the
    operands of the kernels are rounded to fp32.  sum q_i and v^T K^-1 v nearly cancel where the model explains the data,
    and so do their gradients in Lambda and B -- each about a hundred times their sum -- so the same terms in fp32 leave
    1e-4 .. 3e-4 of the largest entry in d ll / d Lambda whatever the kernels return; in fp64 they
    leave what the fp32 reductions themselves do, about 2e-5."""
    G = m.G
    dt = G.dtype
    wide = (dt == torch.float32 and torch.is_grad_enabled() and
            any(t.requires_grad for t in (m.N, m.R, m.B, m.Lambda, xs, ts)))
    if wide:
        m, xs = LEGMatrices(m.N, m.R, m.B.double(), m.Lambda.double()), xs.double()
    pattern, idx, A_table, c_table, xl, xz = _observed_operands(m, ts, xs, observed)
    v = (xl @ m.B).contiguous()
    obs_terms = (xl * xz).sum() + c_table[idx].sum()
    if wide:
        Rs, Os = peg_precision(ts, G)
        v32 = v.to(dt)
        _, sig_inv_det = cr.mahal_and_det(Rs, Os, torch.zeros_like(v32))
        k_mahal, k_det = cr.mahal_and_det(Rs=Rs + A_table[idx].to(dt), Os=Os, x=v32)
        return (-0.5 * ((obs_terms - k_mahal.double()) + (k_det.double() - sig_inv_det.double()))).to(dt)
    if fused_supported(ts, G) and not (torch.is_grad_enabled() and (A_table.requires_grad or v.requires_grad)):
        k_mahal, k_det, sig_inv_det = leg_loglik_reductions_obs(ts, G, A_table, pattern, v)
    else:
        Rs, Os = peg_precision(ts, G)
        _, sig_inv_det = cr.mahal_and_det(Rs, Os, torch.zeros_like(v))
        k_mahal, k_det = cr.mahal_and_det(Rs=Rs + A_table[idx], Os=Os, x=v)
    return -0.5 * ((obs_terms - k_mahal) + (k_det - sig_inv_det))


def _log_likelihood_noise(m, ts, xs, observed, noise_var):
    """``log_likelihood`` with per-observation noise variances:  -1/2 [sum q_i - v^T K^-1 v + sum c_i + log|K| -
    log|Sigma^-1|],  K = PEG precision + blockdiag(B^T Li_i B),  v_i = B^T Li_i x~_i,  q_i = x~_i^T Li_i x~_i."""
    basis, weights, c_rows, xl, xz = _noise_operands(m, ts, xs, observed, noise_var)
    v = (xl @ m.B).contiguous()
    G = m.G
    obs_terms = (xl * xz).sum() + c_rows.sum()
    if fused_supported(ts, G) and not (torch.is_grad_enabled() and
                                       (basis.requires_grad or weights.requires_grad or v.requires_grad)):
        k_mahal, k_det, sig_inv_det = leg_loglik_reductions_w(ts, G, basis.to(G.dtype), weights.to(G.dtype), v)
    else:
        Rs, Os = peg_precision(ts, G)
        _, sig_inv_det = cr.mahal_and_det(Rs, Os, torch.zeros_like(v))
        k_mahal, k_det = cr.mahal_and_det(Rs=Rs + torch.einsum("nk,kij->nij", weights, basis), Os=Os, x=v)
    return -0.5 * ((obs_terms - k_mahal) + (k_det - sig_inv_det))


def log_likelihood(m, ts, xs, observed=None, noise_var=None):
    """log p(xs | ts) of the LEG model (models.py:301-372).  Differentiable in N, R, B, Lambda (through ``m``), xs and
    ts, for any subset of trainable parameters.  The fused reductions (no autograd graph) are taken only when none of
    ts, G, B^T (LL^T)^-1 B and v needs a gradient; otherwise the blocks go through ``peg_precision`` and
    ``cr.mahal_and_det``.

    ``observed`` (bool [n, obs_dim], or [n] for whole rows; None: everything): the density of the observed entries
    alone.  Entries of xs that are not observed are ignored whatever they hold; a row that observes nothing is
    marginalised out, i.e. the result is that of the series without it (``observation_tables``).  The same fused /
    unfused choice (cgps_leg_mahal_logdet_pair_obs), the same gradients, and nothing read on the host.

    ``noise_var`` ([n, obs_dim] or [n], >= 0; None: none, and exactly the calls above): entry c of row i carries extra
    independent noise of variance noise_var[i, c] -- per-point error bars -- so the noise covariance of row i is
    Lambda Lambda^T + 1e-9 I + diag(noise_var[i]) (``observation_weights``).  Combines with ``observed``; entries of
    noise_var that are not observed are ignored whatever they hold.  The fused path (cgps_leg_mahal_logdet_pair_w) builds
    every row's term in registers from obs_dim (obs_dim + 1) / 2 numbers per row; with a gradient wanted the unfused
    path, differentiable in noise_var as well.  Nothing read on the host.  With target times: after ``merge_targets``
    the per-row noise of the merged series is ``noise_all = zeros(n + k, obs_dim); noise_all[observed_all] = noise_var``
    (the stable sort keeps the data rows in their order), passed with ``observed=observed_all``."""
    if noise_var is not None:
        return _log_likelihood_noise(m, ts, xs, observed, noise_var)
    if observed is not None:
        return _log_likelihood_observed(m, ts, xs, observed)
    LLT = m.LLT
    Li = m.inv_of(LLT)
    xl = xs @ Li
    v = (xl @ m.B).contiguous()
    A = m.B.T @ Li @ m.B
    G = m.G
    n = xs.shape[0]
    # fused_supported looks at ts and G only; B, Lambda and xs reach the reductions through A and v
    fused = fused_supported(ts, G) and not (torch.is_grad_enabled() and (A.requires_grad or v.requires_grad))
    if fused and LLT.shape[0] == 1:
        # the two reductions (prior precision: log-det only; posterior precision: mahal + log-det) never see their blocks
        # in memory, and run side by side in one launch: they share nothing but ts and G.  The scalar terms around them
        # are one product, one log and one weighted sum (N ~ 500 is launch-bound: every small launch is ~2.5 us)
        k_mahal, k_det, sig_inv_det = leg_loglik_reductions(ts, G, A, v)
        terms = torch.stack([torch.dot(xl.reshape(-1), xs.reshape(-1)), torch.log(LLT[0, 0]), k_mahal, k_det, sig_inv_det])
        return torch.dot(terms, _ll_weights(n, terms.dtype, terms.device)) - 0.5 * n * math.log(2 * math.pi)
    llt_mahal = (xl * xs).sum()
    llt_det = (torch.log(2 * math.pi * LLT[0, 0]) if LLT.shape[0] == 1 else torch.logdet(2 * math.pi * LLT)) * n
    if fused:
        k_mahal, k_det, sig_inv_det = leg_loglik_reductions(ts, G, A, v)
        return -0.5 * ((llt_mahal - k_mahal) + (llt_det + k_det - sig_inv_det))
    Rs, Os = peg_precision(ts, G)
    _, sig_inv_det = cr.mahal_and_det(Rs, Os, torch.zeros_like(v))       # = det(decompose(Rs, Os)), fused
    K_Rs = Rs + A.unsqueeze(0)
    k_mahal, k_det = cr.mahal_and_det(Rs=K_Rs, Os=Os, x=v)
    return -0.5 * ((llt_mahal - k_mahal) + (llt_det + k_det - sig_inv_det))


class Graphed:
    """``fn(*args, **kwargs)`` of this harness (``log_likelihood``, ``insample_posterior``,
    ``predict.make_predictions`` ...) captured once in a HIP graph and replayed: an evaluation loop over
    fixed shapes then costs one graph launch instead of the function's 25-60 kernel launches and the Python
    between them (N ~ 500 is launch-bound: BASELINE config 5).

    The graph reads its inputs from the tensors given here: change them IN PLACE (``copy_``) between
    replays.  Positive-definiteness is not checked inside the graph (the check reads a device word on the
    host); a non-PD system shows up as NaN / inf in the results.  No gradient.  ``fn`` must not read
    device values on the host (``predict.make_predictions(..., check_sorted=False)``)."""

    def __init__(self, fn, *args, warmup=2, **kwargs):
        dev = next(a.device for a in args if isinstance(a, torch.Tensor))
        prev = cr.CHECK_POSITIVE_DEFINITE
        cr.CHECK_POSITIVE_DEFINITE = False
        try:
            with torch.no_grad():
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):                   # workspaces and library handles exist before capture
                    for _ in range(warmup):
                        fn(*args, **kwargs)
                torch.cuda.current_stream(dev).wait_stream(side)
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph):
                    self.value = fn(*args, **kwargs)
        finally:
            cr.CHECK_POSITIVE_DEFINITE = prev

    def __call__(self):
        """Replay; returns what ``fn`` returned at capture (the same tensors every time)."""
        self.graph.replay()
        return self.value


class GraphedLogLikelihood(Graphed):
    """``log_likelihood(m, ts, xs)`` as a replayable HIP graph (see ``Graphed``); ``value`` is the 0-d result."""

    def __init__(self, m, ts, xs, warmup=2):
        super().__init__(log_likelihood, m, ts, xs, warmup=warmup)


class GraphedValueAndGrad:
    """One training evaluation -- ``ll = log_likelihood(m, ts, xs); ll.backward()`` -- captured in a HIP
    graph (forward through the fused kernels, backward through ``solve`` + ``inverse_blocks`` + the two
    analytic adjoints).  ``m``'s four matrices must be leaf tensors that require a gradient; the graph
    leaves d ll / d (N, R, B, Lambda) in their ``.grad`` (overwritten at every replay) and ll in ``value``.
    Update the matrices / data in place between replays (an optimiser's ``step()`` does).  As with
    ``GraphedLogLikelihood`` nothing is checked on the host inside the graph."""

    def __init__(self, m, ts, xs, warmup=3):
        self.params = [m.N, m.R, m.B, m.Lambda]
        if not all(p.is_leaf and p.requires_grad for p in self.params):
            raise ValueError("the four LEG matrices must be leaf tensors with requires_grad=True")
        prev = cr.CHECK_POSITIVE_DEFINITE
        cr.CHECK_POSITIVE_DEFINITE = False
        try:
            cur = torch.cuda.current_stream(ts.device)
            side = torch.cuda.Stream(device=ts.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                for _ in range(warmup):
                    for p in self.params:
                        p.grad = None
                    log_likelihood(m, ts, xs).backward()
            cur.wait_stream(side)
            for p in self.params:
                p.grad = None                               # the capture allocates the gradients in the graph's pool
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.value = log_likelihood(m, ts, xs)
                self.value.backward()
            self.grads = [p.grad for p in self.params]
        finally:
            cr.CHECK_POSITIVE_DEFINITE = prev

    def __call__(self):
        """Replay; returns (ll, [d ll / d N, d ll / d R, d ll / d B, d ll / d Lambda]) -- the same tensors every time."""
        self.graph.replay()
        return self.value, self.grads


def insample_posterior(m, ts, xs, observed=None, noise_var=None):
    """Posterior mean [N,d] and (diag, lower off-diag) covariance blocks (models.py:282-298).  The mean is
    differentiable; the covariance blocks (``cr.inverse_blocks``) carry no autograd graph.  ``observed`` as in
    ``log_likelihood``: the posterior is given at ALL rows, those that observe nothing included (``merge_targets``).
    ``noise_var`` as in ``log_likelihood``: per-observation noise variances (the mean is differentiable in them too)."""
    K_Rs, K_Os, v = _posterior_system(m, ts, xs, observed, noise_var)
    if K_Rs.is_cuda and not (torch.is_grad_enabled() and (K_Rs.requires_grad or K_Os.requires_grad or v.requires_grad)):
        dec, mean = cr.decompose_solve(K_Rs, K_Os, v)      # factor and solve together (cgps_decompose_solve)
    else:
        dec = cr.decompose(Rs=K_Rs, Os=K_Os)
        mean = cr.solve(dec, v)
    return mean, cr.inverse_blocks(dec)


# ---- the posterior of many series at once, under one model or many -------------------------------------------------
# The concatenated system of all series is block-diagonal, and so is the system "model 0's batch, then model 1's batch,
# ..." that the backward of ``log_likelihood_models`` already reduces: one factorisation and one selected inverse of it
# are the posterior of every (model, series).  cgps_leg_posterior_blocks_seg / _models assemble it with every model's own
# row terms, cgps_leg_intercast_seg / _models (predict.py) predict from it.
MODELS_POSTERIOR_MAX_ROWS = MODELS_BACKWARD_MAX_ROWS
"""``insample_posterior_models`` and the predictions built on it run in chunks of whole models whose concatenated rows
stay under this (a chunk always holds at least one model).  Live per row of a chunk: K's two block arrays [rows, d, d],
the factor's three packed arrays of about the same size together with the reduction's workspace, the two covariance
arrays [rows, d, d], and v and the mean [rows, d] -- about eight [rows, d, d] arrays, 0.84 GB each for a full chunk at
d = 5 in fp64; with ``noise_var`` the weights [rows, obs_dim (obs_dim + 1) / 2] of all models as well."""


def _posterior_batch_supported(ts, G):
    """The concatenated system runs on the general kernels: GPU tensors, every rank 1..8, both precisions."""
    return G.is_cuda and ts.is_cuda and G.dtype in (torch.float32, torch.float64) and 1 <= G.shape[0] <= 8


def _posterior_blocks_models(ts, G, cut, source, term, rows=None):
    """(K_Rs, Os, info) of concatenated series with every row's term added inside the assembly kernel
    (cgps_leg_posterior_blocks_seg): K's diagonal blocks are written once.  source: _hip.ROWS_PLAIN (term [d, d]),
    ROWS_TABLE (term [entries, d, d], rows = pattern bytes [R]) or ROWS_WEIGHTED (term = basis [Kb, d, d], rows = weights
    [R, Kb]); cut may be None (one series).  With G [m, d, d] the same rows under every model
    (cgps_leg_posterior_blocks_models): K_Rs [m R, d, d], Os [m R - 1, d, d] with zero blocks between two models, term and
    the weights with a leading model axis, the pattern bytes shared by the models.  Contiguous operands of G's dtype.
    No autograd graph."""
    R, d, lib = ts.shape[0], G.shape[-1], _hip.lib()
    fn, count = ((lib.cgps_leg_posterior_blocks_models, (R, G.shape[0])) if G.dim() == 3 else
                 (lib.cgps_leg_posterior_blocks_seg, (R,)))
    n = math.prod(count)
    entries = 0 if source == _hip.ROWS_PLAIN else term.shape[-3]
    K_Rs = torch.empty(n, d, d, dtype=G.dtype, device=G.device)
    Os = torch.empty(max(n - 1, 0), d, d, dtype=G.dtype, device=G.device)
    info = torch.zeros(1, dtype=torch.int32, device=G.device)
    term = cr._aligned16(term)                      # (an array of blocks: include/cgps.h wants it on a 16-byte boundary)
    _hip.check(fn(_hip.ptr(ts), _hip.ptr(G), _hip.ptr(cut), *count, d, _hip.dtype_code(G.dtype), source, _hip.ptr(term),
                  entries, _hip.ptr(rows), _hip.ptr(K_Rs), _hip.ptr(Os), _hip.ptr(info), _hip.stream_ptr()))
    return K_Rs, Os, info


_posterior_blocks_seg = _posterior_blocks_models        # the same function: the name of its form without a model axis


def _posterior_blocks_composed(ts, G, cut, source, term, rows=None):
    """What ``_posterior_blocks_models`` replaces for one model, for A/B timing (CGPS_LEG_BLOCKS_COMPOSED=1):
    cgps_peg_precision_seg, then the gather or einsum and the add as torch passes."""
    info = torch.zeros(1, dtype=torch.int32, device=G.device)
    Rs, Os = _peg_precision_models(ts, G, cut, info)
    if source == _hip.ROWS_WEIGHTED:
        return Rs.add_(torch.einsum("nk,kij->nij", rows, term)), Os, info
    if source == _hip.ROWS_TABLE:
        return Rs.add_(term[rows.long().clamp(max=term.shape[0] - 1)]), Os, info
    return Rs.add_(term.unsqueeze(0)), Os, info


def _posterior_system_rows(plan, ts, G, source, term, rows, k0):
    """(K_Rs, K_Os) of the concatenated posterior system of one model's batch or of a chunk of models: the series-aware
    assembly (zero coupling across a series boundary, the gap there never evaluated) with the rows' terms added inside it
    (``_posterior_blocks_models``).  With G [d, d], CGPS_LEG_BLOCKS_COMPOSED=1 takes the composition it replaces instead,
    for A/B timing.  With ``cr.CHECK_POSITIVE_DEFINITE`` a singular time gap raises NotPSDError naming its series (k0 as
    in ``_row_error``)."""
    composed = G.dim() == 2 and os.environ.get("CGPS_LEG_BLOCKS_COMPOSED") == "1"
    blocks = _posterior_blocks_composed if composed else _posterior_blocks_models
    K_Rs, K_Os, info = blocks(ts, G, plan.cut, source, term, rows)
    _check_gaps(info, plan, k0, _GAP_BLOCK)
    return K_Rs, K_Os


def _failed_model_series(plan, m, K_Rs, K_Os, row):
    """(model of the chunk, series, local row) of a factorisation that failed near ``row`` of the concatenated system.
    The factor's info word is the SMALLEST row whose pivot was not positive, and once a block has failed its NaN climbs the
    levels of the concatenated reduction through the zero couplings (0 * NaN) and fails pivots of earlier series and
    models too: the word can name a row in front of the one that broke.  So, on this path only, every (model, series) is
    reduced on its own (``cr.mahal_and_det_batch``: one workgroup per system, systems never meet) and the first that
    fails is named; if none does there, ``row`` is mapped through ``_locate_row``."""
    try:
        cr.mahal_and_det_batch(K_Rs, K_Os, None, lengths=list(plan.lengths) * m)
    except cr.NotPSDError as e:
        system = getattr(e, "system", None)
        if system is not None:
            return system // plan.B, system % plan.B, e.row
    return _locate_row(plan, row)


def _factor_error(e, plan, K_Rs, K_Os, k0):
    """The NotPSDError ``e`` of a factorisation of the concatenated system (k0 as in ``_row_error``) with its system
    named; ``e`` itself when it names no row."""
    row = getattr(e, "row", None)
    if row is None:
        return e
    if k0 is None:                       # (kept as it is: one model's batch maps the factor's word, many models re-reduce)
        return _row_error(plan, row, None, _NOT_PD)
    k, b, r = _failed_model_series(plan, K_Rs.shape[0] // plan.R, K_Rs, K_Os, row)
    return _not_pd_error(k0 + k, b, _NOT_PD % r)


def _posterior_models_chunks(plan, ts, G, source, term, rows, v):
    """The posterior of the batch under every model in chunks of whole models (MODELS_POSTERIOR_MAX_ROWS): yields (k0, k1,
    mean [m R, d], cov_diag [m R, d, d], cov_off [m R - 1, d, d]) of the models k0 .. k1 - 1, the entries of cov_off
    between two series or two models exactly zero.  One assembly launch, one ``cr.decompose_solve`` and one
    ``cr.inverse_blocks`` per chunk.  G [d, d]: the one chunk (0, 1, ...) of one model's batch, whose assembly
    CGPS_LEG_BLOCKS_COMPOSED=1 composes from torch passes.  With ``cr.CHECK_POSITIVE_DEFINITE`` a singular time gap or a
    block that is not positive definite raises NotPSDError naming its (model and) series."""
    named = G.dim() == 3
    for k0, k1, sel in _model_chunks(G, plan.R, MODELS_POSTERIOR_MAX_ROWS):
        K_Rs, K_Os = _posterior_system_rows(plan, ts, _take(G, sel), source, _take(term, sel),
                                            rows if source != _hip.ROWS_WEIGHTED else _take(rows, sel), k0 if named else None)
        try:
            dec, mean = cr.decompose_solve(K_Rs, K_Os, _take(v, sel).reshape(K_Rs.shape[0], -1))
        except cr.NotPSDError as e:
            raise _factor_error(e, plan, K_Rs, K_Os, k0 if named else None) from None
        if named:                        # many models: room for the inverse and for the next chunk.  One model's batch keeps
            del K_Rs, K_Os               # its blocks to the end: freed here, the allocator carves them up for the smaller
        Sd, So = cr.inverse_blocks(dec)  # tensors that follow, and the launch-bound B = 1 call measured 10-20 us slower
        if named:
            del dec
        if (k1 - k0) * plan.B > 1:
            So.index_fill_(0, plan.boundary_rows(k1 - k0), 0)      # (zero up to its sign or a failed system's NaN: exactly zero)
        yield k0, k1, mean, Sd, So


def _posterior_operands_batch(m, ts, xs, observed, noise_var):
    """(source, term, rows, v) of the concatenated posterior system: where the assembly takes a row's diagonal term from
    (``_posterior_blocks_models``) and the right-hand side v [R, d], contiguous and of G's dtype."""
    dt = m.N.dtype
    if noise_var is not None:
        basis, weights, _, xl, _ = _noise_operands(m, ts, xs, observed, noise_var)
        source, term, rows = _hip.ROWS_WEIGHTED, basis.to(dt).contiguous(), weights.to(dt).contiguous()
    elif observed is not None:
        pattern, _, A_table, _, xl, _ = _observed_operands(m, ts, xs, observed)
        source, term, rows = _hip.ROWS_TABLE, A_table.to(dt).contiguous(), pattern.contiguous()
    else:
        Li = m.LLT_inv
        xl = xs @ Li
        source, term, rows = _hip.ROWS_PLAIN, (m.B.T @ Li @ m.B).to(dt).contiguous(), None
    return source, term, rows, (xl @ m.B).to(dt).contiguous()


def _insample_posterior_per_series(m, ts, xs, lengths, observed, noise_var):
    """One ``insample_posterior`` per series (what inputs outside ``_posterior_batch_supported`` get: they behave as they
    do for one series), concatenated, the entry of cov_off at a series boundary zero."""
    means, Sds, Sos, s = [], [], [], 0
    d = m.N.shape[0]
    for b, n in enumerate(lengths):
        try:
            mean, (Sd, So) = insample_posterior(m, ts[s:s + n], xs[s:s + n], None if observed is None else observed[s:s + n],
                                                None if noise_var is None else noise_var[s:s + n])
        except cr.NotPSDError as e:
            raise cr.NotPSDError("LEG batch: series %d: %s" % (b, e)) from None
        means.append(mean)
        Sds.append(Sd)
        Sos.append(So)
        if b + 1 < len(lengths):
            Sos.append(So.new_zeros(1, d, d))
        s += n
    return torch.cat(means), torch.cat(Sds), torch.cat(Sos)


def _posterior_flat(m, ts, xs, lengths, observed, noise_var):
    """(mean, cov_diag, cov_off) of the concatenated batch by whichever path the inputs get."""
    if _posterior_batch_supported(ts, m.G):
        return _posterior_flat_hip(m, ts, xs, lengths, observed, noise_var)[:3]
    return _insample_posterior_per_series(m, ts, xs, lengths, observed, noise_var)


def _posterior_flat_hip(m, ts, xs, lengths, observed, noise_var):
    """(mean [R, d], cov_diag [R, d, d], cov_off [R-1, d, d], plan) of the concatenated batch (already validated): the one
    chunk of ``_posterior_models_chunks`` without a model axis."""
    plan = _cached_batch_plan(lengths, m.N.device)
    G = m.G
    source, term, rows, v = _posterior_operands_batch(m, ts, xs, observed, noise_var)
    (_, _, mean, Sd, So), = _posterior_models_chunks(plan, ts.to(G.dtype).contiguous(), G.contiguous(), source, term, rows, v)
    return mean, Sd, So, plan


def insample_posterior_batch(m, ts, xs, lengths=None, observed=None, noise_var=None):
    """``insample_posterior`` of B independent series in one call: posterior mean and (diagonal, lower off-diagonal)
    covariance blocks of every series (models.py:282-298 for each).  Inference only: the call runs under
    ``torch.no_grad`` and NOTHING it returns carries an autograd graph (the mean included, unlike
    ``insample_posterior``'s).

    Layouts, ``lengths``, ``observed`` and ``noise_var``: those of ``log_likelihood_batch``.  Dense (``lengths=None``):
    ts[B, n], xs[B, n, obs_dim] give mean [B, n, d], cov_diag [B, n, d, d], cov_off [B, n-1, d, d].  Ragged: ts[R],
    xs[R, obs_dim] and host ``lengths`` give mean [R, d], cov_diag [R, d, d], cov_off [R-1, d, d]; series b's
    off-diagonal blocks are rows starts[b] .. starts[b+1]-2 and the entry at a series boundary is exactly zero.  The
    posterior is given at ALL rows, those that observe nothing included; what xs (and noise_var) hold at unobserved
    entries is ignored, NaN included.  A padded dense batch is the mask whose tail rows are False.  noise_var values are
    not checked (``observation_weights``): a negative or non-finite variance at an observed entry surfaces as
    NotPSDError or NaN.  B = 0 returns empty tensors.  Every ValueError is raised before anything is launched.

    How: the concatenated system of all series is block-diagonal -- cgps_peg_precision_seg writes zero coupling across
    a series boundary -- and the inverse of a block-diagonal matrix is block-diagonal, so ONE ``cr.decompose_solve`` and
    ONE ``cr.inverse_blocks`` of the concatenated system are the posterior of every series: every rank 1..8, both
    precisions, no limit on a series' length.  A repeated call with the same lengths copies nothing
    from the host (``_cached_batch_plan``); with ``cr.CHECK_POSITIVE_DEFINITE`` off nothing is read on the host either,
    and the call can be captured (``Graphed``) after one ordinary call with the same lengths.

    Failures: with ``cr.CHECK_POSITIVE_DEFINITE`` a block that is not positive definite, or a zero-length gap, raises
    ``cr.NotPSDError`` naming the series and its local row.  With the check off the failed series' results are NaN, and
    the NaN CAN REACH OTHER SERIES: the concatenated reduction multiplies a neighbour's blocks by the zero coupling, and
    0 * NaN = NaN (unlike ``log_likelihood_batch``, whose series never meet).

    CPU tensors, or a rank or dtype outside the kernels', go through ``insample_posterior`` series by series and behave
    as that does (there is no CPU implementation)."""
    with torch.no_grad():
        ts, xs, lengths, observed, noise_var, dense, bn = _batch_args(m.B.shape[0], ts, xs, lengths, observed, noise_var)
        d, dt = m.N.shape[0], m.N.dtype
        if not lengths:
            e = lambda *shape: torch.empty(shape, dtype=dt, device=ts.device)      # noqa: E731
            if dense:
                return e(0, bn[1], d), (e(0, bn[1], d, d), e(0, max(bn[1] - 1, 0), d, d))
            return e(0, d), (e(0, d, d), e(0, d, d))
        mean, Sd, So = _posterior_flat(m, ts, xs, lengths, observed, noise_var)
        if dense:
            return _dense_posterior(mean, Sd, So, bn[0], bn[1])
        return mean, (Sd, So)


def _dense_posterior(mean, Sd, So, B, n):
    """The concatenated posterior of B series of n rows each as mean [B, n, d], (cov_diag [B, n, d, d], cov_off
    [B, n-1, d, d]): the boundary entries of cov_off are dropped."""
    d = mean.shape[-1]
    if n > 1:
        So = So.as_strided((B, n - 1, d, d), (n * d * d, d * d, d, 1), So.storage_offset()).contiguous()
    else:
        So = So.new_empty(B, 0, d, d)
    return mean.reshape(B, n, d), (Sd.reshape(B, n, d, d), So)


# ---- the posterior of many models over one batch: its checks and its stacked operands --------------------------------
def _models_posterior_args(ms, ts, xs, lengths, observed, noise_var):
    """Everything the posterior and prediction calls over many models check before they launch anything, with the
    ValueErrors of ``log_likelihood_models_observed``: (ms, (N, R, B, Lambda) stacked, ts [R], xs [R, obs], lengths,
    observed [R, obs] or None, noise_var [R, obs] / [R] or None, dense, (B, n) of the dense layout or None)."""
    args = _models_args(ms, ts, xs, lengths, observed, noise_var)
    mats, ts, lengths = args[1], args[2], args[4]
    o = mats[2].shape[1]
    if (lengths and _posterior_batch_supported(ts, mats[0][0]) and (observed is not None or noise_var is not None)
            and o > MAX_PATTERN_OBS):
        raise ValueError("observation patterns are tabulated for obs_dim <= %d, got %d" % (MAX_PATTERN_OBS, o))
    return args


def _models_posterior_operands(mats, xs, observed, noise_var):
    """The stacked operands of the posterior systems, built as ``log_likelihood_models`` and
    ``log_likelihood_models_observed`` build them (elementwise over the models: a model's operands do not depend on its
    neighbours): (G [M, d, d], source, term, rows, v [M, R, d]), contiguous and of the models' dtype."""
    Nm, Rm, Bm, Lm = mats
    d, o, dt = Nm.shape[1], Bm.shape[1], Nm.dtype
    G = _contract(Nm, Nm.transpose(1, 2)) + (Rm - Rm.transpose(1, 2)) + _scaled_eye(d, 1e-5, dt, Nm.device)
    LLT = _contract(Lm, Lm.transpose(1, 2)) + _scaled_eye(o, 1e-9, dt, Nm.device)
    if observed is None and noise_var is None:
        Li, _ = _spd_inverse_logdet(LLT)
        xl = _contract(xs.unsqueeze(0), Li)                                     # [M, R, obs]
        source, term, rows = _hip.ROWS_PLAIN, _contract(_contract(Bm.transpose(1, 2), Li), Bm).to(dt).contiguous(), None
    else:
        xz = xs if observed is None else torch.where(observed, xs, torch.zeros((), dtype=xs.dtype, device=xs.device))
        if noise_var is not None:
            basis, weights, Li_rows, _ = _models_noise_rows(Bm, LLT, o, dt, observed, noise_var)
            source, term, rows = _hip.ROWS_WEIGHTED, basis.to(dt).contiguous(), weights.to(dt).contiguous()
        else:
            pattern = (observed * (1 << torch.arange(o, device=observed.device))).sum(1).to(torch.uint8)
            Li_table, A_table, _ = _models_pattern_tables(Bm, LLT, o, dt)
            Li_rows = Li_table[:, pattern.long()]
            source, term, rows = _hip.ROWS_TABLE, A_table.to(dt).contiguous(), pattern
        xl = _contract(xz.unsqueeze(0).unsqueeze(2), Li_rows).squeeze(2)        # x~^T Li per model and row
    return G.contiguous(), source, term, rows, _contract(xl, Bm).to(dt).contiguous()


def _posterior_models_per_model(ms, each):
    """What inputs outside ``_posterior_batch_supported`` get: ``each(model)`` -- one batched call -- per model, a
    NotPSDError prefixed with the model."""
    outs = []
    for k, m in enumerate(ms):
        try:
            outs.append(each(m))
        except cr.NotPSDError as e:
            raise cr.NotPSDError("LEG models: model %d: %s" % (k, e)) from None
    return outs


def insample_posterior_models(ms, ts, xs, lengths=None, observed=None, noise_var=None):
    """``insample_posterior_batch`` of M LEG models for the same B series in one call: slot k of every result is
    ``insample_posterior_batch(ms[k], ...)``.  What the posterior under every chain of a population, under every start of
    a fit that survived, or under the components of a mixture needs.  Inference only: the call runs under
    ``torch.no_grad`` and nothing it returns carries an autograd graph.

    ``ms``, ``ts`` / ``xs`` / ``lengths``, ``observed`` and ``noise_var``: exactly those of
    ``log_likelihood_models_observed``, with its ValueErrors, raised before anything is launched; the mask and the
    variances belong to the data and are shared by all models.  Dense (``lengths=None``): mean [M, B, n, d], (cov_diag
    [M, B, n, d, d], cov_off [M, B, n-1, d, d]).  Ragged: mean [M, R, d], (cov_diag [M, R, d, d], cov_off [M, R-1, d, d]),
    the entry of cov_off at a series boundary exactly zero.  An empty batch gives empty tensors with leading dimension M.

    How: the stacked operands of ``log_likelihood_models*`` (elementwise over the models), ONE
    cgps_leg_posterior_blocks_models for the blocks of the system "model 0's batch, then model 1's batch, ..." with
    every model's own row terms, ONE ``cr.decompose_solve`` and ONE ``cr.inverse_blocks`` on its M R rows (DESIGN.md
    4.18); more than MODELS_POSTERIOR_MAX_ROWS rows go in chunks of whole models.  Every rank 1..8, both precisions.  A
    repeated call with the same lengths copies nothing from the host (``_cached_batch_plan``); with
    ``cr.CHECK_POSITIVE_DEFINITE`` off nothing is read on the host either.  Not capturable in a HIP graph.

    Failures: with ``cr.CHECK_POSITIVE_DEFINITE`` a block that is not positive definite, or a zero-length gap, raises
    ``cr.NotPSDError`` naming the model, the series and its local row.  With the check off the failed model's results are
    NaN, and the NaN CAN REACH NEIGHBOURING SERIES AND MODELS OF THE SAME CHUNK: the concatenated reduction multiplies a
    neighbour's blocks by the zero coupling, and 0 * NaN = NaN (as in ``insample_posterior_batch``).

    CPU tensors, or a rank or dtype outside the kernels', take one ``insample_posterior_batch`` per model; a
    NotPSDError from it is prefixed with the model."""
    with torch.no_grad():
        ms, mats, ts, xs, lengths, observed, noise_var, dense, bn = _models_posterior_args(ms, ts, xs, lengths, observed,
                                                                                          noise_var)
        M, d, dt = len(ms), mats[0].shape[1], mats[0].dtype
        if not lengths:
            e = lambda *shape: torch.empty(shape, dtype=dt, device=ts.device)      # noqa: E731
            if dense:
                return e(M, 0, bn[1], d), (e(M, 0, bn[1], d, d), e(M, 0, max(bn[1] - 1, 0), d, d))
            return e(M, 0, d), (e(M, 0, d, d), e(M, 0, d, d))
        R = sum(lengths)
        if not _posterior_batch_supported(ts, mats[0][0]):
            outs = _posterior_models_per_model(ms, lambda m: _posterior_flat(m, ts, xs, lengths, observed, noise_var))
            mean, Sd, So = (torch.stack([o[j] for o in outs]) for j in range(3))
            if dense:
                B, n = bn
                So = torch.stack([_dense_posterior(o[0], o[1], o[2], B, n)[1][1] for o in outs])
                return mean.reshape(M, B, n, d), (Sd.reshape(M, B, n, d, d), So)
            return mean, (Sd, So)
        plan = _cached_batch_plan(lengths, mats[0].device)
        G, source, term, rows, v = _models_posterior_operands(mats, xs, observed, noise_var)
        mean = torch.empty(M, R, d, dtype=dt, device=G.device)
        Sd = torch.empty(M, R, d, d, dtype=dt, device=G.device)
        # (a model's R - 1 entries; the one between two models is dropped.  Dense: the ones between two series as well)
        off_shape, off_strides = ((R - 1, d, d), (d * d, d, 1))
        if dense:
            B, n = bn
            off_shape, off_strides = ((B, n - 1, d, d), (n * d * d, d * d, d, 1))
        So = torch.empty((M,) + off_shape, dtype=dt, device=G.device)
        for k0, k1, mean_c, Sd_c, So_c in _posterior_models_chunks(plan, ts.to(dt).contiguous(), G, source, term, rows, v):
            mean[k0:k1] = mean_c.view(k1 - k0, R, d)
            Sd[k0:k1] = Sd_c.view(k1 - k0, R, d, d)
            if So.numel():
                So[k0:k1] = So_c.as_strided((k1 - k0,) + off_shape, (R * d * d,) + off_strides, So_c.storage_offset())
        if dense:
            return mean.view(M, B, n, d), (Sd.view(M, B, n, d, d), So)
        return mean, (Sd, So)


# ---- leave-one-out predictives -----------------------------------------------------------------------------------
# How well a fitted model explains the data it was fitted to, point by point: the distribution of every observation given
# all the others.  Nothing is refitted: with (mu_i, S_ii) the posterior of row i's latent, Li_i = M W_i^-1 M the row's
# noise precision on its observed channels (``observation_weights``) and x~ the data with zeros where nothing is
# observed,  g_i = Li_i M (x~_i - B mu_i)  and  P_i = Li_i - Li_i (B S_ii B^T) Li_i  are the row's block of P x and of P,
# P the precision of the marginal Gaussian of ALL observed entries (Woodbury), and a Gaussian's conditionals are read off
# its precision.  cgps_leg_loo evaluates that for every row of every series under every model.
LooPredictive = collections.namedtuple("LooPredictive", ["mean", "var", "logpdf", "score"])
_LEAVE = {"entry": 0, "row": 1}


def _loo_leave(leave, obs):
    if leave not in _LEAVE:
        raise ValueError("leave must be 'entry' or 'row', got %r" % (leave,))
    if obs > MAX_PATTERN_OBS:
        raise ValueError("observation patterns are tabulated for obs_dim <= %d, got %d" % (MAX_PATTERN_OBS, obs))
    return _LEAVE[leave]


def _loo_data(xs, observed, noise_var, dt):
    """The data as cgps_leg_loo reads it: (xs [R, obs] of the models' dtype, pattern bytes [R] or None, noise_var
    [R, obs] or None), contiguous."""
    obs = xs.shape[1]
    pattern = None
    if observed is not None:
        pattern = (observed * (1 << torch.arange(obs, device=observed.device))).sum(1).to(torch.uint8).contiguous()
    if noise_var is not None:
        noise_var = noise_var.to(dt)
        if noise_var.dim() == 1:
            noise_var = noise_var.unsqueeze(-1).expand(-1, obs)
        noise_var = noise_var.contiguous()
    return xs.to(dt).contiguous(), pattern, noise_var


def _loo_rows(xs, pattern, noise_var, offsets, Bm, LLT, mean, Sd, leave):
    """cgps_leg_loo on a given posterior: xs [R, obs], pattern uint8 [R] or None, noise_var [R, obs] or None, offsets
    device int64 [B + 1] (shared by the models), Bm [M, obs, d], LLT [M, obs, obs], mean [M R, d] and Sd [M R, d, d] (the
    rows of ``_posterior_models_chunks``; M = 1: those of one batch), leave 0 (entry) or 1 (row), all contiguous and of
    one dtype.  Returns (mean [M, R, obs], var [M, R, obs] or [M, R, obs, obs], logpdf [M, R, obs] or [M, R], score
    [M, B] fp64, info int32 [1]: 0 or 1 + the smallest failing row of the M R).  Nothing is read on the host."""
    if not (xs.is_cuda and mean.is_cuda and Sd.is_cuda and Bm.is_cuda):
        raise _hip.CgpsError("leave-one-out predictives run on the GPU (there is no CPU implementation)")
    M, obs, d = Bm.shape
    R, B, dt, dev = xs.shape[0], offsets.shape[0] - 1, mean.dtype, mean.device
    assert tuple(mean.shape) == (M * R, d) and tuple(Sd.shape) == (M * R, d, d) and tuple(LLT.shape) == (M, obs, obs)
    assert tuple(xs.shape) == (R, obs) and all(t.dtype == dt for t in (xs, Bm, LLT, Sd))
    assert pattern is None or (pattern.dtype == torch.uint8 and tuple(pattern.shape) == (R,))
    assert noise_var is None or (noise_var.dtype == dt and tuple(noise_var.shape) == (R, obs))
    assert offsets.dtype == torch.int64 and offsets.is_cuda
    row = leave == _LEAVE["row"]
    out_mean = torch.empty(M, R, obs, dtype=dt, device=dev)
    out_var = torch.empty((M, R, obs, obs) if row else (M, R, obs), dtype=dt, device=dev)
    out_lp = torch.empty((M, R) if row else (M, R, obs), dtype=dt, device=dev)
    score = torch.zeros(M, B, dtype=torch.float64, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    c = lambda t: None if t is None else t.contiguous()      # noqa: E731
    xs, pattern, noise_var, Bm, LLT, mean, Sd = (c(t) for t in (xs, pattern, noise_var, Bm, LLT, mean, Sd))
    _hip.check(_hip.lib().cgps_leg_loo(
        _hip.ptr(xs), _hip.ptr(pattern), _hip.ptr(noise_var), _hip.ptr(offsets), B, R, M, _hip.ptr(Bm), _hip.ptr(LLT), d, obs,
        _hip.dtype_code(dt), _hip.ptr(mean), _hip.ptr(Sd), leave, _hip.ptr(out_mean), _hip.ptr(out_var), _hip.ptr(out_lp),
        _hip.ptr(score), _hip.ptr(info), _hip.stream_ptr()))
    return out_mean, out_var, out_lp, score, info


_LOO_FAILED = ("its leave-one-out precision is not positive definite (the posterior failed, or the noise of the row is "
               "indefinite)")


def _loo_empty(lead, obs, leave, dt, device):
    """Empty results with the leading dimensions ``lead`` (the last of them the empty one) in front of the row axes."""
    e = lambda *shape: torch.empty(lead + shape, dtype=dt, device=device)      # noqa: E731
    return e(obs), (e(obs, obs) if leave else e(obs)), (e() if leave else e(obs))


def _single_series_args(obs, ts, xs, observed, noise_var):
    """What a call on one series of a model of ``obs`` channels checks before it launches anything; returns ``observed``
    as bool [n, obs] or None."""
    if ts.dim() != 1 or xs.dim() != 2 or xs.shape[0] != ts.shape[0] or xs.shape[1] != obs:
        raise ValueError("one series wants ts[n] and xs[n, %d], got %s and %s" % (obs, tuple(ts.shape), tuple(xs.shape)))
    n = ts.shape[0]
    if observed is not None:
        observed = _observed_2d(observed, obs)
        if observed.shape[0] != n:
            raise ValueError("observed has %d rows, xs has %d" % (observed.shape[0], n))
    if noise_var is not None:
        if not isinstance(noise_var, torch.Tensor) or not noise_var.dtype.is_floating_point:
            raise ValueError("noise_var must be a floating-point tensor")
        if noise_var.dim() not in (1, 2) or noise_var.shape[0] != n or (noise_var.dim() == 2 and noise_var.shape[1] != obs):
            raise ValueError("noise_var must be [n] or [n, %d], got %s" % (obs, tuple(noise_var.shape)))
    return observed


def loo_predictive(m, ts, xs, observed=None, noise_var=None, leave="entry"):
    """Leave-one-out predictives of one series under a fitted model: ``LooPredictive(mean, var, logpdf, score)``.

    ``leave="entry"``: for every observed entry (i, c), the Gaussian of x_ic given every OTHER observed entry of the
    series, the other channels of row i included: mean, var and logpdf (the log density of the value that was seen), each
    [n, obs_dim].  ``leave="row"``: for every row, the Gaussian of its observed channels given all other ROWS: mean
    [n, obs_dim], var the covariance [n, obs_dim, obs_dim], logpdf [n].  ``score`` = sum of logpdf, a 0-d fp64 tensor:
    the LOO-CV score of Rasmussen & Williams 5.4.2.  (x - mean) / sqrt(var) are the standardised residuals.  For
    obs_dim = 1 the two coincide.  An unobserved entry has mean = var = NaN (row mode: its row and column of var) and
    logpdf 0; a row that observes nothing has logpdf 0.  ``observed`` and ``noise_var`` as in ``log_likelihood``; what xs
    and noise_var hold at unobserved entries is ignored, NaN included.

    Nothing is refitted: all n obs_dim predictives follow from ONE ``insample_posterior`` and a few obs_dim x obs_dim
    operations per row (cgps_leg_loo).  An evaluation from the posterior loses the factor
    kappa = var_loo / (the entry's noise variance) in relative accuracy, which no formulation from (mu_i, S_ii) avoids.
    Inference only: runs under ``torch.no_grad``.  obs_dim <= 8.  With ``cr.CHECK_POSITIVE_DEFINITE`` a row whose
    predictive does not exist raises ``cr.NotPSDError`` naming it; with the check off its results are NaN.  CPU tensors
    behave as ``insample_posterior`` does (there is no CPU implementation)."""
    with torch.no_grad():
        obs = m.B.shape[0]
        lv = _loo_leave(leave, obs)
        observed = _single_series_args(obs, ts, xs, observed, noise_var)
        n, dt = ts.shape[0], m.N.dtype
        if n == 0:
            return LooPredictive(*_loo_empty((0,), obs, lv, dt, ts.device),
                                 torch.zeros((), dtype=torch.float64, device=ts.device))
        mean, (Sd, _) = insample_posterior(m, ts, xs, observed, noise_var)
        offsets = _cached_batch_plan([n], m.N.device).offsets
        xs_c, pattern, nv = _loo_data(xs, observed, noise_var, dt)
        om, ov, ol, score, info = _loo_rows(xs_c, pattern, nv, offsets, m.B.unsqueeze(0).contiguous(), m.LLT.unsqueeze(0),
                                            mean.contiguous(), Sd.contiguous(), lv)
        if cr.CHECK_POSITIVE_DEFINITE:
            bad = int(info.item())
            if bad:
                raise cr.NotPSDError("LEG leave-one-out: row %d: %s" % (bad - 1, _LOO_FAILED))
        return LooPredictive(om[0], ov[0], ol[0], score[0, 0])


def loo_predictive_batch(m, ts, xs, lengths=None, observed=None, noise_var=None, leave="entry"):
    """``loo_predictive`` of B independent series in one call: ``LooPredictive(mean, var, logpdf, score)`` with
    ``score`` [B] (fp64), the LOO-CV score of every series.

    Layouts, ``lengths``, ``observed`` and ``noise_var``: those of ``insample_posterior_batch``, with its checks and
    ValueErrors, raised before anything is launched.  Dense (``lengths=None``): mean and, for ``leave="entry"``, var and
    logpdf are [B, n, obs_dim]; for ``leave="row"`` var is [B, n, obs_dim, obs_dim] and logpdf [B, n].  Ragged: the same
    with the leading [R] of the concatenated rows.  B = 0 returns empty tensors.

    How: the posterior of the concatenated batch (``insample_posterior_batch``'s ONE ``cr.decompose_solve`` and ONE
    ``cr.inverse_blocks``), then ONE cgps_leg_loo: one lane per row, then one workgroup per series that adds the
    series' log densities in a fixed order, so that a series' score does not depend on its place in the batch.

    Failures: with ``cr.CHECK_POSITIVE_DEFINITE`` a failed posterior raises as ``insample_posterior_batch`` does, and a
    row whose predictive does not exist (its P not positive definite: indefinite noise, a negative ``noise_var``) raises
    ``cr.NotPSDError`` naming the series and its local row; with the check off the row's results and its series' score
    are NaN.  CPU tensors, or a rank or dtype outside the kernels', behave as ``insample_posterior_batch`` does (there is
    no CPU implementation)."""
    with torch.no_grad():
        obs = m.B.shape[0]
        lv = _loo_leave(leave, obs)
        ts, xs, lengths, observed, noise_var, dense, bn = _batch_args(m.B.shape[0], ts, xs, lengths, observed, noise_var)
        dt = m.N.dtype
        if not lengths:
            lead = (0, bn[1]) if dense else (0,)
            return LooPredictive(*_loo_empty(lead, obs, lv, dt, ts.device), torch.empty(0, dtype=torch.float64, device=ts.device))
        mean, Sd, _ = _posterior_flat(m, ts, xs, lengths, observed, noise_var)
        plan = _cached_batch_plan(lengths, m.N.device)
        xs_c, pattern, nv = _loo_data(xs, observed, noise_var, dt)
        om, ov, ol, score, info = _loo_rows(xs_c, pattern, nv, plan.offsets, m.B.unsqueeze(0).contiguous(), m.LLT.unsqueeze(0),
                                            mean.contiguous(), Sd.contiguous(), lv)
        if cr.CHECK_POSITIVE_DEFINITE:
            bad = int(info.item())
            if bad:
                _, b, r = _locate_row(plan, bad - 1)
                raise cr.NotPSDError("LEG leave-one-out: series %d: row %d: %s" % (b, r, _LOO_FAILED))
        om, ov, ol = om[0], ov[0], ol[0]
        if dense:
            om, ov, ol = (t.reshape(bn + tuple(t.shape[1:])) for t in (om, ov, ol))
        return LooPredictive(om, ov, ol, score[0])


def loo_predictive_models(ms, ts, xs, lengths=None, observed=None, noise_var=None, leave="entry"):
    """``loo_predictive_batch`` of M LEG models for the same B series in one call: slot k of every result is
    ``loo_predictive_batch(ms[k], ...)``, and ``score`` [M, B] (fp64) is the LOO-CV score of every model on every series
    -- the number that ranks restarts, chains, grid points or mixture components by held-out fit without holding
    anything out.

    ``ms``, ``ts`` / ``xs`` / ``lengths``, ``observed`` and ``noise_var``: exactly those of ``insample_posterior_models``,
    with its ValueErrors, raised before anything is launched; the mask and the variances belong to the data and are
    shared by all models.  Dense: [M, B, n, ...]; ragged: [M, R, ...]; an empty batch gives empty tensors with leading
    dimension M.

    How: ``insample_posterior_models``' chunks of whole models (MODELS_POSTERIOR_MAX_ROWS), each consumed by ONE
    cgps_leg_loo (grid over rows and models) as soon as it exists: only the LOO outputs are kept, the [M, R, d, d]
    covariance blocks of all models are never held at once.

    Failures: with ``cr.CHECK_POSITIVE_DEFINITE``, as ``insample_posterior_models`` for the posterior, and a row whose
    predictive does not exist raises ``cr.NotPSDError`` naming the model, the series and its local row.  CPU tensors, or a
    rank or dtype outside the kernels', take one ``loo_predictive_batch`` per model."""
    with torch.no_grad():
        ms, mats, ts, xs, lengths, observed, noise_var, dense, bn = _models_posterior_args(ms, ts, xs, lengths, observed,
                                                                                          noise_var)
        M, obs, dt = len(ms), mats[2].shape[1], mats[0].dtype
        lv = _loo_leave(leave, obs)
        if not lengths:
            lead = (M, 0, bn[1]) if dense else (M, 0)
            return LooPredictive(*_loo_empty(lead, obs, lv, dt, ts.device),
                                 torch.empty(M, 0, dtype=torch.float64, device=ts.device))
        if not _posterior_batch_supported(ts, mats[0][0]):
            outs = _posterior_models_per_model(
                ms, lambda m: loo_predictive_batch(m, ts, xs, lengths, observed, noise_var, leave))
            om, ov, ol, score = (torch.stack([o[j] for o in outs]) for j in range(4))
        else:
            plan = _cached_batch_plan(lengths, mats[0].device)
            G, source, term, rows, v = _models_posterior_operands(mats, xs, observed, noise_var)
            Bm = mats[2].contiguous()
            LLT = (_contract(mats[3], mats[3].transpose(1, 2)) + _scaled_eye(obs, 1e-9, dt, Bm.device)).contiguous()
            xs_c, pattern, nv = _loo_data(xs, observed, noise_var, dt)
            parts = []
            for k0, k1, mean_c, Sd_c, _ in _posterior_models_chunks(plan, ts.to(dt).contiguous(), G, source, term, rows, v):
                out = _loo_rows(xs_c, pattern, nv, plan.offsets, Bm[k0:k1], LLT[k0:k1], mean_c, Sd_c, lv)
                del mean_c, Sd_c
                if cr.CHECK_POSITIVE_DEFINITE:
                    bad = int(out[4].item())
                    if bad:
                        k, b, r = _locate_row(plan, bad - 1)
                        raise cr.NotPSDError("LEG leave-one-out: model %d, series %d: row %d: %s" % (k0 + k, b, r, _LOO_FAILED))
                parts.append(out[:4])
            om, ov, ol, score = (parts[0][j] if len(parts) == 1 else torch.cat([p[j] for p in parts]) for j in range(4))
        if dense:
            om, ov, ol = (t.reshape((M,) + bn + tuple(t.shape[2:])) for t in (om, ov, ol))
        return LooPredictive(om, ov, ol, score)


# ---- one-step-ahead predictives and filtered states ------------------------------------------------------------------
# The causal quantities of a series: the distribution of row i's observation given the rows BEFORE it, the log density
# of what was seen under it (the terms whose sum is the log-likelihood), and the state z_i given the rows up to and
# including i.  The smoother's kernels cannot supply them -- cyclic reduction eliminates rows in even / odd order, and the
# pivot that carries x_<=i exists only under forward elimination -- so cgps_leg_filter walks every series forward, one
# lane per (series, model), everything in registers.
FilterPredictive = collections.namedtuple("FilterPredictive", ["mean", "cov", "logpdf", "z_mean", "z_cov", "loglik", "state"])
FilterState = collections.namedtuple("FilterState", ["t", "mean", "cov"])

_FILTER_FAILED = ("its one-step-ahead predictive does not exist (the covariance of its observed channels is not positive "
                  "definite -- a negative noise_var? --, its gap is negative, or a result is not finite)")


# The time-parallel form (cgps_leg_filter_scan): what ``chunk_rows="auto"`` stands for -- the fastest pair
# measured for one series of 2^20 rows (rank 5, fp64) on one MI355X.
FILTER_CHUNK_ROWS = 128
FILTER_SCAN_FANOUT = 16


def _filter_chunking(chunk_rows):
    """``chunk_rows`` of the filter calls as None (the serial kernel) or (rows per chunk L >= 1, fan-out F >= 2) of the
    time-parallel form: an int L, a pair (L, F) or "auto"; ValueError for anything else."""
    if chunk_rows is None:
        return None
    if isinstance(chunk_rows, str) and chunk_rows == "auto":
        return FILTER_CHUNK_ROWS, FILTER_SCAN_FANOUT
    is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)      # noqa: E731
    if is_int(chunk_rows):
        chunk_rows = (chunk_rows, FILTER_SCAN_FANOUT)
    if not (isinstance(chunk_rows, (tuple, list)) and len(chunk_rows) == 2 and all(is_int(v) for v in chunk_rows)
            and chunk_rows[0] >= 1 and chunk_rows[1] >= 2):
        raise ValueError('chunk_rows must be None, "auto", an int L >= 1 or a pair (L, F) with L >= 1 rows per chunk and '
                         "fan-out F >= 2, got %r" % (chunk_rows,))
    return int(chunk_rows[0]), int(chunk_rows[1])


# The time-parallel backward: what ``backward_chunk_rows="auto"`` stands for, and how the chunks'
# transfer maps are measured -- d sequential probe calls of cgps_leg_filter_adjoint (False), or ONE call over d + 1 copies
# of the models (True: copy 0 carries the real cotangents, copies 1..d the probes) at d + 1 times the memory of the saved
# states and the cotangents.  Both MEASURED (tools/time_filter_grad_scan.py, one MI355X, fp64, rank 5): 128 rows is the
# fastest L or within 7 % of it at 2^14, 2^17 and 2^20 rows (256 wins at 2^20), and the replicated call is the faster
# at 2^20 rows (14.3 against 15.4 ms at obs_dim 1, 15.7 against 18.3 ms at obs_dim 3) and at every shorter length.
FILTER_BACKWARD_CHUNK_ROWS = 128
FILTER_LINK_REPLICATE = True


def _filter_backward_chunking(backward_chunk_rows):
    """``backward_chunk_rows`` of the filter calls as None (the serial reverse walk) or the rows per chunk L >= 1 of the
    time-parallel backward: an int L or "auto"; ValueError for anything else."""
    if backward_chunk_rows is None:
        return None
    if isinstance(backward_chunk_rows, str) and backward_chunk_rows == "auto":
        return FILTER_BACKWARD_CHUNK_ROWS
    if not (isinstance(backward_chunk_rows, int) and not isinstance(backward_chunk_rows, bool) and backward_chunk_rows >= 1):
        raise ValueError('backward_chunk_rows must be None, "auto" or an int L >= 1 rows per chunk, got %r'
                         % (backward_chunk_rows,))
    return int(backward_chunk_rows)


class _ChunkPlan:
    """The chunk layout of a batch for chunks of ``L`` rows (a subclass per L: ``_chunk_plan_kind``): ceil(n_b / L)
    chunks per series, restarting at every series' first row.  Device int64 tensors ``chunk_offsets`` [chunks + 1] (row
    offsets), ``chunk_series`` [chunks] and ``series_chunks`` [B + 1] (the first chunk of every series), planned on the
    host from the lengths and cached like the batch plans (``_cached_batch_plan``).  ``rounds``: ceil(log2(the most
    chunks of one series - 1)), the doubling rounds of ``_filter_link_scan``."""
    L = None

    def __init__(self, lengths, device):
        lens = torch.as_tensor(list(lengths), dtype=torch.int64)
        per = (lens + (self.L - 1)) // self.L
        self.rounds = max(int(per.max()) - 2, 0).bit_length() if len(lengths) else 0
        zero = torch.zeros(1, dtype=torch.int64)
        first = torch.cat([zero, torch.cumsum(per, 0)])
        rows = torch.cat([zero, torch.cumsum(lens, 0)])
        self.chunks = int(first[-1])
        ser = torch.repeat_interleave(torch.arange(len(lengths), dtype=torch.int64), per, output_size=self.chunks)
        local = torch.arange(self.chunks, dtype=torch.int64) - first[ser]
        off = torch.cat([rows[ser] + local * self.L, rows[-1:]])
        self.chunk_offsets, self.chunk_series, self.series_chunks = (t.to(device) for t in (off, ser, first))


@functools.lru_cache(maxsize=None)
def _chunk_plan_kind(L):
    return type("_ChunkPlan%d" % L, (_ChunkPlan,), {"L": L, "plans": {}, "captured": {}})


def _filter_state_kind(init):
    """``init`` (not None) checked as a ``FilterState``: a triple of tensors; ValueError otherwise."""
    if not (isinstance(init, tuple) and len(init) == 3 and all(isinstance(t, torch.Tensor) for t in init)):
        raise ValueError("init must be a FilterState (t, mean, cov) of tensors")


def _filter_state(init, want, wants):
    """``_filter_state_kind``, and the three shapes are ``want`` (an entry None: not looked at); ValueError otherwise,
    ``wants`` saying what the call takes."""
    _filter_state_kind(init)
    got = tuple(tuple(t.shape) for t in init)
    if any(w is not None and g != w for g, w in zip(got, want)):
        raise ValueError("%s, got %s, %s and %s" % ((wants,) + got))
    return init


def _filter_init(init, lead, d, ts, starts, dt):
    """``init`` checked against the batch: (t0 [B], m0 lead + [d], P0 lead + [d, d]) of dtype ``dt``, contiguous, or None.
    ``lead`` is (B,) or (M, B); ``starts`` the first row of every series.  ValueError for the wrong kind, shape or device
    and for a state later than the first row of its series."""
    if init is None:
        return None
    B = lead[-1]
    want = ((B,), tuple(lead) + (d,), tuple(lead) + (d, d))
    t0, m0, P0 = _filter_state(init, want, "init wants t %s, mean %s and cov %s" % want)
    if any(t.device != ts.device for t in (t0, m0, P0)) or not all(t.dtype.is_floating_point for t in (t0, m0, P0)):
        raise ValueError("init must hold floating-point tensors on the device of ts")
    t0 = t0.to(dt).contiguous()
    if B and bool((t0 > ts.to(dt)[torch.as_tensor(starts, device=ts.device)]).any()):
        raise ValueError("init.t lies after the first row of its series (the gap to the first row may be zero, not negative)")
    return t0, m0.to(dt).contiguous(), P0.to(dt).contiguous()


def _filter_rows(ts, xs, pattern, noise_var, offsets, G, Bm, LLT, init, scan=None):
    """cgps_leg_filter, or with ``scan`` = (a ``_ChunkPlan`` of the batch, fan-out) cgps_leg_filter_scan: ts [R], xs
    [R, obs], pattern uint8 [R] or None, noise_var [R, obs] or None, offsets device int64 [B + 1] (shared by the models), G [M, d, d], Bm [M, obs, d], LLT [M, obs, obs], init (t0 [B], m0 [M, B, d], P0
    [M, B, d, d]) or None, all contiguous and of one dtype.  Returns (mean [M, R, obs], cov [M, R, obs, obs], logpdf
    [M, R], z_mean [M, R, d], z_cov [M, R, d, d], loglik [M, B] fp64, m_end [M, B, d], P_end [M, B, d, d], info int32
    [1]: 0 or 1 + the smallest failing row of the M R).  Nothing is read on the host."""
    if not (ts.is_cuda and xs.is_cuda and G.is_cuda and Bm.is_cuda):
        raise _hip.CgpsError("one-step-ahead predictives run on the GPU (there is no CPU implementation)")
    M, obs, d = Bm.shape
    R, B, dt, dev = xs.shape[0], offsets.shape[0] - 1, G.dtype, G.device
    assert tuple(G.shape) == (M, d, d) and tuple(LLT.shape) == (M, obs, obs) and tuple(ts.shape) == (R,)
    assert tuple(xs.shape) == (R, obs) and all(t.dtype == dt for t in (ts, xs, Bm, LLT))
    assert pattern is None or (pattern.dtype == torch.uint8 and tuple(pattern.shape) == (R,))
    assert noise_var is None or (noise_var.dtype == dt and tuple(noise_var.shape) == (R, obs))
    assert offsets.dtype == torch.int64 and offsets.is_cuda
    t0, m0, P0 = init if init is not None else (None, None, None)
    assert init is None or (tuple(t0.shape) == (B,) and tuple(m0.shape) == (M, B, d) and tuple(P0.shape) == (M, B, d, d)
                            and all(t.dtype == dt and t.is_cuda for t in init))
    e = lambda *shape: torch.empty(shape, dtype=dt, device=dev)      # noqa: E731
    mean, cov, lp, zm, zc = e(M, R, obs), e(M, R, obs, obs), e(M, R), e(M, R, d), e(M, R, d, d)
    m_end, P_end = e(M, B, d), e(M, B, d, d)
    loglik = torch.zeros(M, B, dtype=torch.float64, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    c = lambda t: None if t is None else t.contiguous()      # noqa: E731
    ts, xs, pattern, noise_var, G, Bm, LLT, t0, m0, P0 = (c(t) for t in (ts, xs, pattern, noise_var, G, Bm, LLT, t0, m0, P0))
    data = (_hip.ptr(ts), _hip.ptr(xs), _hip.ptr(pattern), _hip.ptr(noise_var), _hip.ptr(offsets), B, R, M, _hip.ptr(G),
            _hip.ptr(Bm), _hip.ptr(LLT), d, obs, _hip.dtype_code(dt), _hip.ptr(t0), _hip.ptr(m0), _hip.ptr(P0))
    res = (_hip.ptr(mean), _hip.ptr(cov), _hip.ptr(lp), _hip.ptr(zm), _hip.ptr(zc), _hip.ptr(loglik), _hip.ptr(m_end),
           _hip.ptr(P_end), _hip.ptr(info), _hip.stream_ptr())
    if scan is None:
        _hip.check(_hip.lib().cgps_leg_filter(*data, *res))
    else:
        chunks, fanout = scan
        ws, nbytes = _hip.filter_scan_workspace(chunks.chunks, M, d, dt, fanout, dev)
        _hip.check(_hip.lib().cgps_leg_filter_scan(
            *data, _hip.ptr(chunks.chunk_offsets), _hip.ptr(chunks.chunk_series), _hip.ptr(chunks.series_chunks),
            chunks.chunks, chunks.L, fanout, _hip.ptr(ws), nbytes, *res))
    return mean, cov, lp, zm, zc, loglik, m_end, P_end, info


def _filter_adjoint_rows(xs, pattern, noise_var, offsets, G, Bm, LLT, gap, zm, zc, m0, P0, cots, out=None):
    """cgps_leg_filter_adjoint: the data and operands of ``_filter_rows``, gap [R] (the time before every row; 0 at a first
    row without a start state), the saved z_mean / z_cov, the start states or None, and ``cots`` = the cotangents of
    (mean, cov, logpdf, z_mean, z_cov), each [M, R, ...] or None.  Returns (x_bar [M, R, obs], s_bar [M, R, obs], B_bar
    [M, B, obs, d], LLT_bar [M, B, obs, obs], m0_bar [M, B, d], P0_bar [M, B, d, d], G_bar partial sums [M, blocks, d, d],
    gap_bar [M, R]).  ``out``: the eight of an earlier call with the same shapes, written again instead of fresh ones.
    ``offsets`` may be a chunk plan's ``chunk_offsets`` with the chunks' start states: the entry then walks every chunk
    as if it were a series.  Nothing is read on the host."""
    M, obs, d = Bm.shape
    R, B, dt, dev = xs.shape[0], offsets.shape[0] - 1, G.dtype, G.device
    c = lambda t: None if t is None else t.to(dt).contiguous()      # noqa: E731
    cots = [c(t) for t in cots]
    for t, tail in zip(cots, ((obs,), (obs, obs), (), (d,), (d, d))):
        assert t is None or tuple(t.shape) == (M, R) + tail
    e = lambda *shape: torch.empty(shape, dtype=dt, device=dev)      # noqa: E731
    blocks = (R + 63) // 64
    shapes = ((M, R, obs), (M, R, obs), (M, B, obs, d), (M, B, obs, obs), (M, B, d), (M, B, d, d), (M, blocks, d, d), (M, R))
    if out is None:
        out = tuple(e(*s) for s in shapes)
    assert all(tuple(t.shape) == s and t.dtype == dt and t.is_contiguous() for t, s in zip(out, shapes))
    gx, gs, gB, gL, gm0, gP0, gG, gg = out
    ws, nbytes = _hip.filter_adjoint_workspace(R, B, M, d, obs, dt, dev)
    xs, noise_var, G, Bm, LLT, gap, zm, zc, m0, P0 = (c(t) for t in (xs, noise_var, G, Bm, LLT, gap, zm, zc, m0, P0))
    _hip.check(_hip.lib().cgps_leg_filter_adjoint(
        _hip.ptr(xs), _hip.ptr(pattern), _hip.ptr(noise_var), _hip.ptr(offsets), B, R, M, _hip.ptr(G), _hip.ptr(Bm),
        _hip.ptr(LLT), d, obs, _hip.dtype_code(dt), _hip.ptr(gap), _hip.ptr(zm), _hip.ptr(zc), _hip.ptr(m0), _hip.ptr(P0),
        *(_hip.ptr(t) for t in cots), _hip.ptr(ws), nbytes, _hip.ptr(gx), _hip.ptr(gs), _hip.ptr(gB), _hip.ptr(gL),
        _hip.ptr(gm0), _hip.ptr(gP0), _hip.ptr(gG), _hip.ptr(gg), _hip.stream_ptr()))
    return gx, gs, gB, gL, gm0, gP0, gG, gg


# ---- the time-parallel backward --------------------------------------------------------------------------
# The reverse recursion is affine in the cotangent it receives.  Chunk c maps what its last row receives, (mb, Db), to
# what it hands the chunk before it:
#     mb_in = PhiT_c mb + cm_c ;    Db_in = PhiT_c Db PhiT_c^T + sum_j mb_j T_c[j] + cD_c          (T_c[j] symmetric)
# Db never feeds mb, Db -> Db is the congruence with the matrix that carries mb, and mb -> Db is linear.  Two chunks, 1
# the earlier rows, 2 the later ones (2 is applied first), compose to
#     PhiT_12 = PhiT_1 PhiT_2 ;    T_12[j] = PhiT_1 T_2[j] PhiT_1^T + sum_i (PhiT_2)_ij T_1[i]
#     cm_12 = PhiT_1 cm_2 + cm_1 ;    cD_12 = PhiT_1 cD_2 PhiT_1^T + sum_i (cm_2)_i T_1[i] + cD_1
def _filter_link_scan(PhiT, T, cm, cD, series_chunks, rounds=None):
    """What every chunk's last row receives from the later chunks of its series: (mb [M, C, d], Db [M, C, d, d]), the affine
    part of the composite of chunks c + 1 .. the series' last (zero for a series' last chunk).  ``PhiT`` [M, C, d, d],
    ``T`` [M, C, d, d, d] (T[m, c, j] symmetric), ``cm`` [M, C, d], ``cD`` [M, C, d, d]: the chunks' maps in the notation
    above; ``series_chunks`` int64 [B + 1]: the first chunk of every series.  A segmented suffix scan over the chunk axis
    by doubling: ``rounds`` rounds (None: ceil(log2(C - 1)), enough for any layout; a chunk receives at most the composite
    of the n - 1 chunks after it, n the most chunks of a series, and the caller that knows n passes ceil(log2(n - 1))).
    A composition across a series' boundary is never SELECTED, so nothing -- a failed series' NaN included -- passes from
    one series into another.  Pure torch on any device; nothing is read on the host."""
    M, C, d = cm.shape
    dev = cm.device
    if C == 0:
        return cm.clone(), cD.clone()
    B = series_chunks.shape[0] - 1
    per = series_chunks[1:] - series_chunks[:-1]
    ser = torch.repeat_interleave(torch.arange(B, device=dev), per, output_size=C)
    end = series_chunks[1:][ser]                                   # one past the last chunk of the chunk's series
    idx = torch.arange(C, device=dev)
    if rounds is None:
        rounds = max(C - 2, 0).bit_length()

    def later(step):
        nxt = idx + step
        return nxt < end, nxt.clamp_max(C - 1)

    def select(ok, new, old):
        return torch.where(ok.reshape((1, C) + (1,) * (old.dim() - 2)), new, old)

    step = 1
    for r in range(rounds):                                        # element c: the composite of c .. c + step - 1
        ok, j = later(step)
        Phi = PhiT.transpose(-1, -2)
        m2, D2 = cm[:, j], cD[:, j]
        new_m = (PhiT @ m2.unsqueeze(-1)).squeeze(-1) + cm
        new_D = PhiT @ D2 @ Phi + torch.einsum("mci,mciab->mcab", m2, T) + cD
        if r + 1 < rounds:                                         # (the last round's maps are used by nobody)
            P2, T2 = PhiT[:, j], T[:, j]
            new_T = PhiT.unsqueeze(2) @ T2 @ Phi.unsqueeze(2) + torch.einsum("mcij,mciab->mcjab", P2, T)
            PhiT, T = select(ok, PhiT @ P2, PhiT), select(ok, new_T, T)
        cm, cD = select(ok, new_m, cm), select(ok, new_D, cD)
        step *= 2
    ok, j = later(1)
    return select(ok, cm[:, j], torch.zeros_like(cm)), select(ok, cD[:, j], torch.zeros_like(cD))


def _filter_chunk_maps(run, M, R, d, dt, dev, last, cots, replicate):
    """The maps of ``_filter_link_scan`` for every (model, chunk), measured by cgps_leg_filter_adjoint itself: (PhiT, T,
    cm, cD, the eight output buffers to use again or None).  ``run(cots, out, copies)`` is the entry over the chunk view
    (``copies`` > 1: over that many copies of the models along the model axis), ``last`` the chunks' last rows.  (cm, cD)
    are the start-state adjoints under the real cotangents with nothing received; column j of PhiT and T[j] those under
    no cotangent but e_j on z_mean of every chunk's last row.  ``replicate``: one call over d + 1 copies of the models
    instead of d + 1 calls."""
    if not replicate:
        bufs = run(cots, None, 1)
        C = bufs[4].shape[1]
        cm, cD = bufs[4].clone(), bufs[5].clone()
        PhiT = torch.empty(M, C, d, d, dtype=dt, device=dev)
        T = torch.empty(M, C, d, d, d, dtype=dt, device=dev)
        probe = torch.zeros(M, R, d, dtype=dt, device=dev)
        for j in range(d):
            if j:
                probe[:, last, j - 1] = 0
            probe[:, last, j] = 1
            run([None, None, None, probe, None], bufs, 1)
            PhiT[..., j] = bufs[4]
            T[:, :, j] = bufs[5]
        return PhiT, T, cm, cD, bufs
    K = d + 1
    big = []
    for j, t in enumerate(cots):
        if t is None and j != 3:
            big.append(None)
            continue
        tail = (d,) if j == 3 else tuple(t.shape[2:])
        full = torch.zeros((K, M, R) + tail, dtype=dt, device=dev)
        if t is not None:
            full[0] = t
        big.append(full)
    for j in range(d):
        big[3][j + 1, :, last, j] = 1
    out = run([None if t is None else t.reshape((K * M,) + tuple(t.shape[2:])) for t in big], None, K)
    C = out[4].shape[1]
    gm0, gP0 = out[4].reshape(K, M, C, d), out[5].reshape(K, M, C, d, d)
    return gm0[1:].permute(1, 2, 3, 0), gP0[1:].permute(1, 2, 0, 3, 4), gm0[0], gP0[0], None


def _filter_chunk_states(chunks, zm, zc, m0, P0):
    """The chunk view of a batch: (the start state of every chunk -- mean [M, C, d] and cov [M, C, d, d]: the saved
    filtered state of the row before it, for a series' first chunk its (m0, P0), or (0, I) when there is none --, the
    chunks' last rows [C])."""
    M, R, d = zm.shape
    dt, dev, C = zm.dtype, zm.device, chunks.chunks
    coff, cser, first = chunks.chunk_offsets, chunks.chunk_series, chunks.series_chunks
    head = (torch.arange(C, device=dev) == first[:-1][cser]).reshape(1, C, 1)      # a series' first chunk
    prev = (coff[:-1] - 1).clamp_min(0)
    if m0 is not None:
        sm, sP = m0.to(dt)[:, cser], P0.to(dt)[:, cser]
    else:
        sm, sP = torch.zeros(1, 1, d, dtype=dt, device=dev), torch.eye(d, dtype=dt, device=dev).reshape(1, 1, d, d)
    return (torch.where(head, sm, zm[:, prev]).contiguous(), torch.where(head.unsqueeze(-1), sP, zc[:, prev]).contiguous(),
            coff[1:] - 1)


def _filter_adjoint_linked(xs, pattern, noise_var, G, Bm, LLT, gap, zm, zc, m0, P0, cots, chunks, replicate=None):
    """``_filter_adjoint_rows`` of the batch, parallel in time: the entry runs over the chunks of
    ``chunks`` (a ``_ChunkPlan`` of the batch) as if they were series -- ``_filter_chunk_states`` --, d + 1 times to
    measure every chunk's map, a scan over arrays with one element per chunk links them, and a last call with what every
    chunk receives on its last row gives the result.  Returns the eight of ``_filter_adjoint_rows`` with B_bar and LLT_bar
    per (model, CHUNK) and m0_bar, P0_bar per (model, series): those of the series' first chunk."""
    M, obs, d = Bm.shape
    R, dt, dev, C = xs.shape[0], G.dtype, G.device, chunks.chunks
    replicate = FILTER_LINK_REPLICATE if replicate is None else replicate
    coff, first = chunks.chunk_offsets, chunks.series_chunks
    B = first.shape[0] - 1
    cm0, cP0, last = _filter_chunk_states(chunks, zm, zc, m0, P0)
    cots = [None if t is None else t.to(dt) for t in cots]

    def run(cots_, out, copies):
        rep = lambda t: t if copies == 1 else t.repeat((copies,) + (1,) * (t.dim() - 1))      # noqa: E731
        return _filter_adjoint_rows(xs, pattern, noise_var, coff, rep(G), rep(Bm), rep(LLT), gap, rep(zm), rep(zc), rep(cm0),
                                    rep(cP0), cots_, out)

    PhiT, T, cm, cD, bufs = _filter_chunk_maps(run, M, R, d, dt, dev, last, cots, replicate)
    wide = lambda t: t.to(torch.float64)      # noqa: E731
    rm, rD = _filter_link_scan(wide(PhiT), wide(T), wide(cm), wide(cD), first, chunks.rounds)
    g_zm = torch.zeros(M, R, d, dtype=dt, device=dev) if cots[3] is None else cots[3].clone()
    g_zc = torch.zeros(M, R, d, d, dtype=dt, device=dev) if cots[4] is None else cots[4].clone()
    g_zm.index_add_(1, last, rm.to(dt))
    g_zc.index_add_(1, last, rD.to(dt))
    gx, gs, gB, gL, gm0, gP0, gG, gg = run(cots[:3] + [g_zm, g_zc], bufs, 1)
    has_rows = (first[1:] > first[:-1]).reshape(1, B, 1)
    at = first[:-1].clamp_max(C - 1)
    gm0 = torch.where(has_rows, gm0[:, at], torch.zeros((), dtype=dt, device=dev))
    gP0 = torch.where(has_rows.unsqueeze(-1), gP0[:, at], torch.zeros((), dtype=dt, device=dev))
    return gx, gs, gB, gL, gm0, gP0, gG, gg


class _FilterFn(torch.autograd.Function):
    """``_filter_rows`` with a backward: the forward is the same launch (serial or time-parallel) and
    keeps z_mean and z_cov; the backward is ONE cgps_leg_filter_adjoint -- gaps, the serial reverse walk, the Frechet pass
    -- and a few torch sums, or with ``bchunks`` (a ``_ChunkPlan`` of the batch in which a series has more than one chunk)
    ``_filter_adjoint_linked``, the same entry over chunks.  Inputs: G [M, d, d], Bm [M, obs, d], LLT
    [M, obs, obs], ts [R], xs [R, obs], noise_var [R, obs] or None, t0 [B], m0 [M, B, d], P0 [M, B, d, d] or three None;
    ``pattern``, ``offsets``, ``scan`` and ``bchunks`` carry no gradient.  Outputs: the nine of ``_filter_rows``; info is
    not differentiable."""

    @staticmethod
    def forward(ctx, G, Bm, LLT, ts, xs, noise_var, t0, m0, P0, pattern, offsets, scan, bchunks=None):
        ctx.set_materialize_grads(False)
        init = None if t0 is None else (t0, m0, P0)
        out = _filter_rows(ts, xs, pattern, noise_var, offsets, G, Bm, LLT, init, scan)
        ctx.save_for_backward(G, Bm, LLT, ts, xs, noise_var, t0, m0, P0, out[3], out[4])
        ctx.data = (pattern, offsets, bchunks)
        ctx.mark_non_differentiable(out[8])
        return out

    @staticmethod
    def backward(ctx, g_mean, g_cov, g_lp, g_zm, g_zc, g_ll, g_mend, g_Pend, _g_info):
        G, Bm, LLT, ts, xs, noise_var, t0, m0, P0, zm, zc = ctx.saved_tensors
        pattern, offsets, bchunks = ctx.data
        M, obs, d = Bm.shape
        R, B, dt, dev = xs.shape[0], offsets.shape[0] - 1, G.dtype, G.device
        lens = offsets[1:] - offsets[:-1]
        sid = torch.repeat_interleave(torch.arange(B, device=dev), lens, output_size=R)      # the series of every row
        is_first = torch.arange(R, device=dev) == offsets[:-1][sid]
        has_rows = lens > 0
        last = (offsets[1:] - 1).clamp_min(0)
        # loglik is the sum of the series' logpdf; the end state is the last row's filtered state (a series without rows:
        # the state it started from)
        if g_ll is not None:
            add = g_ll.to(dt)[:, sid]
            g_lp = add if g_lp is None else g_lp + add
        direct = [None, None]
        cots = [g_zm, g_zc]
        for j, (g_end, tail) in enumerate(((g_mend, (d,)), (g_Pend, (d, d)))):
            if g_end is not None:
                keep = has_rows.reshape((1, B) + (1,) * len(tail))
                acc = torch.zeros((M, R) + tail, dtype=dt, device=dev) if cots[j] is None else cots[j].to(dt).clone()
                cots[j] = acc.index_add_(1, last, g_end.to(dt) * keep)
                direct[j] = g_end.to(dt) * ~keep
        gap = ts - torch.roll(ts, 1)
        gap = torch.where(is_first, (ts - t0[sid]) if t0 is not None else torch.zeros_like(ts), gap)
        if bchunks is None:
            gx, gs, gB, gL, gm0, gP0, gG, gg = _filter_adjoint_rows(xs, pattern, noise_var, offsets, G, Bm, LLT, gap, zm, zc,
                                                                  m0, P0, [g_mean, g_cov, g_lp] + cots)
        else:
            gx, gs, gB, gL, gm0, gP0, gG, gg = _filter_adjoint_linked(xs, pattern, noise_var, G, Bm, LLT, gap, zm, zc, m0, P0,
                                                                    [g_mean, g_cov, g_lp] + cots, bchunks)
            # a failed (model, series): NaN in ALL its entries of x_bar and s_bar, as the serial walk stores them (the
            # linked one leaves the exact zeros of its unobserved entries)
            failed = ~torch.isfinite(zm[:, last].sum(-1) + zc[:, last].sum((-1, -2))) & has_rows
            nan = torch.full((), float("nan"), dtype=dt, device=dev)
            gx, gs = (torch.where(failed[:, sid].unsqueeze(-1), nan, t) for t in (gx, gs))
        gg = gg.sum(0)
        inner = torch.where(is_first, torch.zeros_like(gg), gg)      # gap i = ts[i] - ts[i - 1]
        g_ts = inner - torch.cat([inner[1:], inner.new_zeros(1)])
        g_t0 = None
        if t0 is not None:                                           # gap = ts[first row] - t0
            head = torch.where(is_first, gg, torch.zeros_like(gg))
            g_ts = g_ts + head
            g_t0 = -torch.zeros(B, dtype=dt, device=dev).index_add_(0, sid, head)
            gm0 = gm0 if direct[0] is None else gm0 + direct[0]
            gP0 = gP0 if direct[1] is None else gP0 + direct[1]
        else:
            gm0 = gP0 = None
        return (gG.sum(1), gB.sum(1), gL.sum(1), g_ts, gx.sum(0), gs.sum(0) if noise_var is not None else None, g_t0, gm0,
                gP0, None, None, None, None)


def _filter_empty(lead, obs, d, dt, device):
    """Empty per-row results with the leading dimensions ``lead`` (one of them the empty one) in front of the row axes."""
    e = lambda *shape: torch.empty(tuple(lead) + shape, dtype=dt, device=device)      # noqa: E731
    return e(obs), e(obs, obs), e(), e(d), e(d, d)


def _filter_models(mats, ts, xs, lengths, observed, noise_var, init, named, chunking=None, differentiable=False,
                   backward_rows=None):
    """The filter of the stacked models ``mats`` over a validated, non-empty batch: (the eight tensors of
    ``_filter_rows``, the times of the series' last rows [B]).  ``init`` has the models' axis.  ``named``: whether a
    failure's message names the model.  ``chunking``: None or the (L, F) of ``_filter_chunking``.  ``differentiable``:
    under grad mode and with an input that requires grad, the launch goes through ``_FilterFn`` and the results carry
    a graph (the caller must not be under ``torch.no_grad``).  ``backward_rows``: None or the L of
    ``_filter_backward_chunking``; the backward of that graph is then parallel in time wherever a series has more than one
    chunk of L rows."""
    Nm, Rm, Bm, Lm = mats
    M, obs, d, dt = Nm.shape[0], Bm.shape[1], Nm.shape[1], Nm.dtype
    if obs > MAX_PATTERN_OBS:
        raise ValueError("the filter's channel axis is built for obs_dim <= %d, got %d" % (MAX_PATTERN_OBS, obs))
    off = [0]
    for n in lengths:
        off.append(off[-1] + n)
    init = _filter_init(init, (M, len(lengths)), d, ts, off[:-1], dt)
    if not (ts.is_cuda and xs.is_cuda and Nm.is_cuda):
        raise _hip.CgpsError("one-step-ahead predictives run on the GPU (there is no CPU implementation)")
    plan = _cached_batch_plan(lengths, Nm.device)
    G = (_contract(Nm, Nm.transpose(1, 2)) + (Rm - Rm.transpose(1, 2)) + _scaled_eye(d, 1e-5, dt, Nm.device)).contiguous()
    LLT = (_contract(Lm, Lm.transpose(1, 2)) + _scaled_eye(obs, 1e-9, dt, Nm.device)).contiguous()
    xs_c, pattern, nv = _loo_data(xs, observed, noise_var, dt)
    ts_c = ts.to(dt).contiguous()
    scan = None if chunking is None else (_cached_batch_plan(lengths, Nm.device, _chunk_plan_kind(chunking[0])), chunking[1])
    t0, m0, P0 = init if init is not None else (None, None, None)
    inputs = (G, Bm.contiguous(), LLT, ts_c, xs_c, nv, t0, m0, P0)
    if differentiable and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in inputs):
        bchunks = None
        if backward_rows is not None and max(lengths) > backward_rows:
            bchunks = _cached_batch_plan(lengths, Nm.device, _chunk_plan_kind(backward_rows))
        out = _FilterFn.apply(*inputs, pattern, plan.offsets, scan, bchunks)
    else:
        with torch.no_grad():
            out = _filter_rows(ts_c, xs_c, pattern, nv, plan.offsets, G, Bm.contiguous(), LLT, init, scan)
    if cr.CHECK_POSITIVE_DEFINITE:
        bad = int(out[8].item())
        if bad:
            k, b, r = _locate_row(plan, bad - 1)
            where = ("model %d, series %d" % (k, b)) if named else ("series %d" % b)
            raise cr.NotPSDError("LEG filter: %s: row %d: %s" % (where, r, _FILTER_FAILED))
    return out[:8], ts_c[plan.offsets[1:] - 1]


def _filter_grad_mode(differentiable):
    """The context the filter calls run under: ``torch.no_grad`` unless ``differentiable``."""
    return contextlib.nullcontext() if differentiable else torch.no_grad()


def _stack1(m):
    return tuple(t.unsqueeze(0) for t in (m.N, m.R, m.B, m.Lambda))


def filter_predictive(m, ts, xs, observed=None, noise_var=None, init=None, chunk_rows=None, differentiable=False,
                      backward_chunk_rows=None):
    """One-step-ahead predictives and filtered states of one series: ``FilterPredictive(mean, cov, logpdf, z_mean, z_cov,
    loglik, state)``.

    For every row i: ``mean`` [n, obs_dim] and ``cov`` [n, obs_dim, obs_dim], the Gaussian of the row's observation (all
    channels) given the rows BEFORE it, p(x_i | x_<i); ``logpdf`` [n], the log density of the row's observed entries
    under it (0 for a row that observes nothing); ``z_mean`` [n, d] and ``z_cov`` [n, d, d], the state z_i given the rows
    up to and including i -- the only estimate available while the data are still arriving.  ``loglik`` (0-d fp64) is the
    sum of ``logpdf`` in row order: ``log_likelihood`` of the series.  T^-1 (x_o - mean_o) with cov[o, o] = T T^T are the
    standardised innovations.  ``observed`` and ``noise_var`` as in ``log_likelihood``; what xs and noise_var hold at
    unobserved entries is ignored, NaN included.

    ``state`` is the ``FilterState(t, mean, cov)`` after the last row.  Pass it as ``init=`` of a later call on the rows
    that FOLLOW to continue without refiltering; the gap from ``init.t`` to the first row may be zero but not negative
    (ValueError).  ``init=None``: the prior N(0, I) at the first row.

    ``chunk_rows=None``: the work is SERIAL in the series' rows (cgps_leg_filter, DESIGN.md 4.22: one lane per (series,
    model) walks its rows): one series of 2^20 rows is one lane's chain of 2^20 steps.  ``chunk_rows=`` an int L, a pair
    (L, F) or "auto" (``FILTER_CHUNK_ROWS``, ``FILTER_SCAN_FANOUT``): TIME-PARALLEL (cgps_leg_filter_scan, DESIGN.md
    4.23) -- the series is cut into chunks of L rows, a scan with fan-out F over the chunks' compositions gives every
    chunk the exact state it starts from, and the serial kernel runs over the chunks as if they were series: chains of
    about 2 L + F log_F(n / L) steps instead of n.  Same results, shapes and failures; rows [0, L) are the serial call's
    bit for bit, later rows agree with it to rounding (fp64: the bounds of the serial call against the dense truths;
    fp32: at most 4x the error of the recursion in torch), ``loglik`` is the sum of the chunks' sums.  Pass it for ONE
    long series or a few -- 2^20 rows, rank 5, fp64 on one MI355X: 2.03 s serially, 2.43 ms with "auto" (DESIGN.md 4.23);
    2^14 rows: 30.8 ms and 0.84 ms with (16, 16) -- and for batches as well, see ``filter_predictive_batch``.
    ``differentiable=False`` (the default): inference only, the call runs under ``torch.no_grad``.
    ``differentiable=True``: under grad mode and with an input that requires grad, ``mean``, ``cov``, ``logpdf``,
    ``z_mean``, ``z_cov``, ``loglik``, ``state.mean`` and ``state.cov`` carry a graph -- same forward launch, same bits --
    with gradients in the model's N, R, B, Lambda and in ``ts``, ``xs``, ``noise_var``, ``init.t``, ``init.mean``,
    ``init.cov`` (a mask has none; the gradient in xs and noise_var is exactly 0 at unobserved entries).  The backward
    is one cgps_leg_filter_adjoint: a reverse walk of the rows, one lane per series, from the saved
    ``z_mean`` / ``z_cov``.  ``backward_chunk_rows=None`` (the default): that walk is SERIAL whatever ``chunk_rows`` is --
    the backward of one long series is one lane's chain.  ``backward_chunk_rows=`` an int L >= 1 or "auto"
    (``FILTER_BACKWARD_CHUNK_ROWS`` = 128, chosen from the measurement below): the backward is TIME-PARALLEL (DESIGN.md
    4.25), independent of ``chunk_rows`` since it needs only the saved states -- the same entry walks chunks of L rows as if they were series,
    once over d + 1 copies of the model to measure every chunk's affine map of the cotangent it receives (d + 1 times the
    memory of the saved states; ``FILTER_LINK_REPLICATE = False``: d + 1 calls instead), a scan over arrays with one
    element per chunk links the chunks of a series, and one more call gives the gradients: chains of about 2 L steps
    ((d + 2) L with the sequential calls) and ceil(log2(n / L)) scan rounds instead of n.  Same gradients to rounding
    (fp64: rtol 1e-7 / atol 1e-10 against autograd of the recursion; fp32: at most 4x the error of the serial backward);
    a series that fits one chunk: the serial call, bit for bit.  Forward + backward of ``loglik.sum()``, one series, rank 5, fp64, obs_dim 1 on one MI355X with
    ``chunk_rows="auto"``: 2^20 rows 2.85 s with the serial backward (timed once), 14.3 ms with "auto" (13.5 ms with 256);
    2^17 rows 398 ms and 5.0 ms; 2^14 rows 45.3 ms and 4.3 ms.  Anything else is a ValueError; without
    ``differentiable=True`` or with nothing that requires grad it is checked and ignored.  No second derivatives.
    Ranks 1..8, obs_dim <= 8, both precisions.  With
    ``cr.CHECK_POSITIVE_DEFINITE`` a row whose predictive does not exist raises ``cr.NotPSDError`` naming it; with the
    check off that row, all later rows and ``loglik`` are NaN.  CPU tensors behave as ``insample_posterior`` does (there
    is no CPU implementation)."""
    with _filter_grad_mode(differentiable):
        chunking = _filter_chunking(chunk_rows)
        backward_rows = _filter_backward_chunking(backward_chunk_rows)
        obs, d, dt = m.B.shape[0], m.N.shape[0], m.N.dtype
        observed = _single_series_args(obs, ts, xs, observed, noise_var)
        n = ts.shape[0]
        if init is not None:
            _filter_state(init, ((), (d,), (d, d)), "one series wants init with t 0-d, mean [%d] and cov [%d, %d]" % (d, d, d))
            init = FilterState(init[0].reshape(1), init[1].reshape(1, 1, d), init[2].reshape(1, 1, d, d))
        if n == 0:
            state = FilterState(*(t.reshape(s).to(dt) for t, s in zip(init, ((), (d,), (d, d))))) if init is not None else None
            return FilterPredictive(*_filter_empty((0,), obs, d, dt, ts.device),
                                    torch.zeros((), dtype=torch.float64, device=ts.device), state)
        out, t_end = _filter_models(_stack1(m), ts, xs, [n], observed, noise_var, init, False, chunking, differentiable,
                                     backward_rows)
        return FilterPredictive(*(t[0] for t in out[:5]), out[5][0, 0], FilterState(t_end[0], out[6][0, 0], out[7][0, 0]))


def filter_predictive_batch(m, ts, xs, lengths=None, observed=None, noise_var=None, init=None, chunk_rows=None,
                            differentiable=False, backward_chunk_rows=None):
    """``filter_predictive`` of B independent series in one call: ``FilterPredictive(mean, cov, logpdf, z_mean, z_cov,
    loglik, state)`` with ``loglik`` [B] (fp64) and ``state = FilterState(t [B], mean [B, d], cov [B, d, d])``.

    Layouts, ``lengths``, ``observed`` and ``noise_var``: those of ``insample_posterior_batch``, with its checks and
    ValueErrors, raised before anything is launched.  Dense (``lengths=None``): the per-row results are [B, n, ...];
    ragged: [R, ...] over the concatenated rows.  B = 0 returns empty tensors (and ``state`` = ``init``).  ``init``: a
    ``FilterState`` of B states, as a previous call's ``state``, to continue every series on the rows that follow; a
    state later than its series' first row is a ValueError.

    How: ONE cgps_leg_filter, one lane per series, 64-lane workgroups, no workspace, nothing read on the host unless
    ``cr.CHECK_POSITIVE_DEFINITE``.  The work is SERIAL in a series' rows and parallel across series: 1 024 series of 502
    rows fill 16 CUs for 502 steps; one series of 2^20 rows is one lane's chain of 2^20 steps.  A series' results do
    not depend on its place in the batch, bit for bit.

    ``chunk_rows=`` (an int L, a pair (L, F), or "auto"): the time-parallel form of ``filter_predictive``, one
    cgps_leg_filter_scan over all series -- chunks of L rows that never straddle a series (ceil(n_b / L) per series,
    planned on the host from ``lengths`` and cached like the batch plan), one scan over all chunks in which a series'
    first chunk is a reset that is SELECTED, so nothing crosses from one series into the next, a failed one's NaN
    included.  A series' results then depend on its place in the batch through the grouping of the scan alone: within
    64 eps of any other place, not bit for bit.  When to pass it (one MI355X, fp64, rank 5, series of 502 rows): measured
    faster than the serial kernel from 64 series (1.62 -> 1.19 ms with "auto", 1.03 ms with (64, 32)) up to 1 024 series
    (1.68 -> 1.47 ms, 1.39 ms) -- no crossover inside that range; the longer the series the larger the gain.  Leave it
    None for the bit-for-bit guarantees above and for ``loglik`` as the sum of the rows in row order.

    ``differentiable=``: as in ``filter_predictive`` -- False (the default) is inference only under ``torch.no_grad``;
    True builds the graph for every result but ``state.t``, and the backward is one serial reverse walk per series
    (cgps_leg_filter_adjoint, one lane per series; with ``chunk_rows=`` too) unless ``backward_chunk_rows=`` (an int L
    or "auto") makes it parallel in time as in ``filter_predictive``: chunks of L rows that never straddle a series, a
    series' first chunk starting from its ``init``, nothing passing from one series into the next, a failed one's NaN
    included.  When to pass it (one MI355X, fp64, rank 5, series of 502 rows, forward + backward of
    ``loglik.sum()``): at 64 series 64 rows per chunk measured 3.24 ms against 3.42 ms serial at obs_dim 1 -- level in
    a second run -- (3.81 against 5.06 ms at obs_dim 3) and "auto" 3.46 ms (4.55 ms); at 1 024 series the serial walk
    WINS, 4.17 ms against 6.40 ms (6.11 against 7.60 ms) -- leave it None for wide batches of short series.  ``loglik.sum().backward()`` gives the
    gradients of ``log_likelihood_batch`` without the smoother's factorisation; per-row weights on ``logpdf``, losses on
    ``mean`` or ``z_mean`` and the gradient into ``init`` come from nowhere else.

    Failures: with ``cr.CHECK_POSITIVE_DEFINITE`` a row whose predictive does not exist raises ``cr.NotPSDError`` naming
    the series and its local row; with the check off that row, the later rows of THAT series, its ``loglik`` and its
    ``state`` are NaN and every other series is untouched (with ``differentiable=True`` the gradient in that series' rows
    of xs and noise_var, in its ``init`` and in the model's matrices is NaN; the other series' rows are untouched).  CPU tensors behave as ``insample_posterior_batch`` does
    (there is no CPU implementation)."""
    with _filter_grad_mode(differentiable):
        chunking = _filter_chunking(chunk_rows)
        backward_rows = _filter_backward_chunking(backward_chunk_rows)
        ts, xs, lengths, observed, noise_var, dense, bn = _batch_args(m.B.shape[0], ts, xs, lengths, observed, noise_var)
        obs, d, dt = m.B.shape[0], m.N.shape[0], m.N.dtype
        if init is not None:
            B = len(lengths)
            _filter_state(init, (None, (B, d), (B, d, d)), "a batch of %d series wants init with t [%d], mean [%d, %d] and "
                          "cov [%d, %d, %d]" % (B, B, B, d, B, d, d))
            init = FilterState(init[0], init[1].unsqueeze(0), init[2].unsqueeze(0))
        if not lengths:
            if init is not None and tuple(init[0].shape) != (0,):
                raise ValueError("init wants t [0] for an empty batch, got %s" % (tuple(init[0].shape),))
            lead = (0, bn[1]) if dense else (0,)
            state = FilterState(init[0], init[1][0], init[2][0]) if init is not None else None
            return FilterPredictive(*_filter_empty(lead, obs, d, dt, ts.device),
                                    torch.empty(0, dtype=torch.float64, device=ts.device), state)
        out, t_end = _filter_models(_stack1(m), ts, xs, lengths, observed, noise_var, init, False, chunking, differentiable,
                                     backward_rows)
        rows = [t[0] for t in out[:5]]
        if dense:
            rows = [t.reshape(bn + tuple(t.shape[1:])) for t in rows]
        return FilterPredictive(*rows, out[5][0], FilterState(t_end, out[6][0], out[7][0]))


def filter_predictive_models(ms, ts, xs, lengths=None, observed=None, noise_var=None, init=None, chunk_rows=None,
                             differentiable=False, backward_chunk_rows=None):
    """``filter_predictive_batch`` of M LEG models for the same B series in one call: slot k of every result is
    ``filter_predictive_batch(ms[k], ...)``, bit for bit; ``loglik`` is [M, B] (fp64) and ``state =
    FilterState(t [B], mean [M, B, d], cov [M, B, d, d])``.  ``logpdf`` [M, ...] holds the terms from which the running
    posterior weights of the M models over time follow (a cumulative sum along the rows and a softmax over the models):
    online model averaging.

    ``ms``, ``ts`` / ``xs`` / ``lengths``, ``observed`` and ``noise_var``: exactly those of ``insample_posterior_models``,
    with its ValueErrors, raised before anything is launched; the mask, the variances and ``init.t`` belong to the data
    and are shared by all models.  Dense: [M, B, n, ...]; ragged: [M, R, ...]; an empty batch gives empty tensors with
    leading dimension M.

    How: ONE cgps_leg_filter with grid (ceil(B / 64), M): one lane per (series, model).  The work is SERIAL in a
    series' rows: one series of 2^20 rows is one lane's chain of 2^20 steps under every model.  ``chunk_rows=`` (an int
    L, a pair (L, F), or "auto"): the time-parallel form of ``filter_predictive_batch`` with grid rows for the models
    (cgps_leg_filter_scan); slot k is still the call on ``ms[k]`` with the same ``chunk_rows``, bit for
    bit.  When to pass it: as for ``filter_predictive_batch`` (timed with one model only).  ``differentiable=``: as in
    ``filter_predictive_batch``, with gradients in every model's four matrices; the gradients in ``ts``, ``xs``,
    ``noise_var`` and ``init.t``, which the models share, are summed over the models.  ``backward_chunk_rows=``: the
    time-parallel backward of ``filter_predictive_batch`` with one chunk map per (model, chunk); None (the default) is the
    serial walk.

    Failures: with ``cr.CHECK_POSITIVE_DEFINITE`` a row whose predictive does not exist raises ``cr.NotPSDError`` naming
    the model, the series and its local row; with the check off that row and the later rows of that series under THAT
    model, its ``loglik`` and its ``state`` are NaN, and every other series and model is untouched.  CPU tensors raise
    as ``filter_predictive_batch`` does (there is no CPU implementation)."""
    with _filter_grad_mode(differentiable):
        chunking = _filter_chunking(chunk_rows)
        backward_rows = _filter_backward_chunking(backward_chunk_rows)
        ms, mats, ts, xs, lengths, observed, noise_var, dense, bn = _models_posterior_args(ms, ts, xs, lengths, observed,
                                                                                          noise_var)
        M, obs, d, dt = len(ms), mats[2].shape[1], mats[0].shape[1], mats[0].dtype
        if init is not None:
            _filter_state_kind(init)                               # (``_filter_init`` checks the shapes)
        if not lengths:
            if init is not None and (tuple(init[0].shape), tuple(init[1].shape), tuple(init[2].shape)) != ((0,), (M, 0, d), (M, 0, d, d)):
                raise ValueError("init wants t [0], mean [%d, 0, %d] and cov [%d, 0, %d, %d] for an empty batch" % (M, d, M, d, d))
            lead = (M, 0, bn[1]) if dense else (M, 0)
            return FilterPredictive(*_filter_empty(lead, obs, d, dt, ts.device),
                                    torch.empty(M, 0, dtype=torch.float64, device=ts.device),
                                    FilterState(*init) if init is not None else None)
        out, t_end = _filter_models(mats, ts, xs, lengths, observed, noise_var, init, True, chunking, differentiable,
                                     backward_rows)
        rows = list(out[:5])
        if dense:
            rows = [t.reshape((M,) + bn + tuple(t.shape[2:])) for t in rows]
        return FilterPredictive(*rows, out[5], FilterState(t_end, out[6], out[7]))


# ---- drawing from the process -----------------------------------------------------------------------
def sample_observations(m, z, seed, stream=1):
    """Observations of latent paths z [n, rank, S]: x = B z + Lambda eps' [n, obs, S], eps' =
    ``cr.standard_normal(n obs, S, seed, stream)`` (the observation model of models.py:254-280).  Its default noise
    stream is 1; the latent draws of ``cr.sample`` use stream 0 of the same seed."""
    n, S = z.shape[0], z.shape[2]
    obs = m.B.shape[0]
    eps = cr.standard_normal(n * obs, S, seed, stream=stream, dtype=z.dtype, device=z.device if z.is_cuda else None)
    eps = eps.to(z.device).reshape(n, obs, S)                # (CPU inputs: generated on the GPU, like every result)
    return torch.baddbmm(torch.matmul(m.Lambda.to(z.dtype), eps), m.B.to(z.dtype).expand(n, -1, -1), z)


def sample_from_prior(m, ts, num_samples, seed):
    """num_samples draws of the LEG process at times ts: (z [n, rank, S] latent paths, x [n, obs, S] observations).
    The finished form of the reference's LEGFamily.sample_from_prior stub (models.py:243-252): the prior precision
    (``peg_precision``), its factor, ``cr.sample`` for z, ``sample_observations`` for x.  No autograd graph."""
    with torch.no_grad():
        Rs, Os = peg_precision(ts, m.G)
        z = cr.sample(cr.decompose(Rs, Os), num_samples, seed)
        return z, sample_observations(m, z, seed)


def sample_from_posterior(m, ts, xs, num_samples, seed, observed=None, noise_var=None):
    """num_samples latent paths z [n, rank, S] from the posterior given xs at ts: factor and posterior mean together
    (``cr.decompose_solve``), then ``cr.sample`` with that mean -- two library calls.  No autograd graph.  ``observed``
    as in ``log_likelihood``: joint paths through every row, observed or not; ``noise_var`` as there too."""
    with torch.no_grad():
        K_Rs, K_Os, v = _posterior_system(m, ts, xs, observed, noise_var)
        dec, mean = cr.decompose_solve(K_Rs, K_Os, v)
        return cr.sample(dec, num_samples, seed, mean=mean)


# ---- drawing paths for many series at once: perturb and solve -------------------------------------
# x = K^-1 (v + w), w ~ N(0, K), is a draw from the posterior N(K^-1 v, K^-1).  K is a sum of local positive
# semi-definite pieces (the stationary start of a series, one transition per time gap, one observation per row), so w
# is a sum of local pieces of noise indexed by (series id, local row): cgps_leg_perturbation_seg makes v + w for all
# rows, series and samples in one launch, and the draw of a series does not depend on where it sits in the batch.
MAX_SERIES_ID = 1 << 24
SAMPLE_RHS_FACTOR = 4
"""``sample_from_posterior_batch`` solves the right-hand sides in chunks of columns: a multiple of eight (one solve
panel) that keeps a chunk at most this many times the size of K's own blocks (2 d^2 values a row), eight at the least."""


def _sample_column_chunk(d):
    return max(8, 2 * d * SAMPLE_RHS_FACTOR // 8 * 8)


def _series_ids_arg(series_ids, lengths, d, obs, device):
    """The ids as a device int64 [B] after the checks of the generator's index space (ValueError before any launch)."""
    B = len(lengths)
    if lengths and max(lengths) * max(d, obs) >= 1 << 40:
        raise ValueError("a series of %d rows does not fit the generator's 2^40 elements per series" % max(lengths))
    if series_ids is None:
        if B > MAX_SERIES_ID:
            raise ValueError("%d series: the default ids 0 .. B-1 must stay below 2^24" % B)
        return torch.arange(B, dtype=torch.int64, device=device)
    if isinstance(series_ids, torch.Tensor):
        if series_ids.dim() != 1 or series_ids.dtype.is_floating_point or series_ids.dtype == torch.bool:
            raise ValueError("series_ids must be a list or a 1-d integer tensor")
        series_ids = series_ids.tolist()
    ids = [int(k) for k in series_ids]
    if len(ids) != B:
        raise ValueError("series_ids names %d series, the batch has %d" % (len(ids), B))
    bad = [k for k in ids if not 0 <= k < MAX_SERIES_ID]
    if bad:
        raise ValueError("series id %d outside 0 .. 2^24 - 1" % bad[0])
    return torch.tensor(ids, dtype=torch.int64).to(device)


def _sample_count(num_samples):
    S = int(num_samples)
    if S < 1:
        raise ValueError("num_samples must be at least 1, got %d" % S)
    return S


def _perturbation_models(ts, G, plan, ids, hsource, hterm, pattern, v, S, seed, words, k0=0):
    """rhs [R, d, S] of cgps_leg_perturbation_seg under the stream word ``words`` (an int) or, with G [m, d, d], rhs
    [m R, d, S] of cgps_leg_perturbation_models for the models of one chunk (the first of them model k0 of the call):
    hterm [m, ...] by source, v [m, R, d] or None, ``words`` device int64 [m].  Contiguous operands of G's dtype on G's
    device.  With ``cr.CHECK_POSITIVE_DEFINITE`` a singular time gap raises NotPSDError naming (model,) series and row."""
    R, d, dt, lib = plan.R, G.shape[-1], G.dtype, _hip.lib()
    fn, count, words = ((lib.cgps_leg_perturbation_models, (R, G.shape[0]), _hip.ptr(words)) if G.dim() == 3 else
                        (lib.cgps_leg_perturbation_seg, (R,), int(words) & 0xFFFFFFFF))
    out = torch.empty(math.prod(count), d, S, dtype=dt, device=G.device)
    info = torch.zeros(1, dtype=torch.int32, device=G.device)
    entries = hterm.shape[-3] if hsource == _hip.H_TABLE else 0
    obs = hterm.shape[-1] if hsource != _hip.H_NONE else 0
    _hip.check(fn(_hip.ptr(ts), *count, _hip.ptr(G), d, _hip.dtype_code(dt), _hip.ptr(plan.offsets), _hip.ptr(ids), plan.B,
                  hsource, _hip.ptr(hterm), entries, obs, _hip.ptr(pattern), _hip.ptr(v), S, int(seed) & 0xFFFFFFFFFFFFFFFF,
                  words, _hip.ptr(out), _hip.ptr(info), _hip.stream_ptr()))
    _check_gaps(info, plan, k0 if G.dim() == 3 else None, _GAP_NOISE)
    return out


_perturbation_seg = _perturbation_models        # the same function: the name of its form without a model axis


def _solve_columns_models(K_Rs, K_Os, rhs, plan, k0):
    """K^-1 rhs [rows, d, S] on the concatenated system of one model's batch (k0 None) or of a chunk of models (the first
    of them model k0 of the call): one factorisation, a failure named as ``_posterior_models_chunks`` names it, the
    right-hand sides in column chunks (a column never depends on the chunking: the solve treats its columns
    independently)."""
    try:
        dec = cr.decompose(K_Rs, K_Os)
    except cr.NotPSDError as e:
        raise _factor_error(e, plan, K_Rs, K_Os, k0) from None
    return _solve_factor_columns(dec, rhs)


def _solve_factor_columns(dec, rhs):
    """``cr.solve`` of rhs [rows, d, S] on a given factor, in column chunks of ``_sample_column_chunk(d)`` columns."""
    S, chunk = rhs.shape[2], _sample_column_chunk(rhs.shape[1])
    if S <= chunk:
        return cr.solve(dec, rhs)
    x = torch.empty_like(rhs)
    for c in range(0, S, chunk):
        x[:, :, c:c + chunk] = cr.solve(dec, rhs[:, :, c:c + chunk])
    return x


def _noise_source(rows, observed, noise_var):
    """(hsource, pattern) of the perturbation kernels: where a row's observation-noise factor comes from, and the pattern
    bytes of the table source (``rows`` of the posterior operands: ``observation_tables``' byte)."""
    if noise_var is not None:
        return _hip.H_ROWS, None
    return (_hip.H_PLAIN, None) if observed is None else (_hip.H_TABLE, rows)


def _posterior_perturbation_flat(m, ts, xs, observed, noise_var, plan, ids, S, seed, stream):
    """(K_Rs, K_Os, rhs [R, d, S]) of the concatenated batch (already validated, on the GPU)."""
    G = m.G
    dt = G.dtype
    source, term, rows, v = _posterior_operands_batch(m, ts, xs, observed, noise_var)
    tsc, Gc = ts.to(dt).contiguous(), G.contiguous()
    K_Rs, K_Os = _posterior_system_rows(plan, tsc, Gc, source, term, rows, None)
    hsource, pattern = _noise_source(rows, observed, noise_var)
    hterm = observation_noise_factors(m, observed, noise_var).to(dt).contiguous()
    return K_Rs, K_Os, _perturbation_models(tsc, Gc, plan, ids, hsource, hterm, pattern, v, S, seed, stream)


def _on_gpu(m, *tensors):
    """The model and the tensors on the GPU the kernels run on (there is no CPU implementation)."""
    dev = m.N.device if m.N.is_cuda else cr._device()
    return (m if m.N.is_cuda else m.to(dev),) + tuple(None if t is None else t.to(dev) for t in tensors)


def _perturbation_call(m, ts, xs, num_samples, seed, lengths, observed, noise_var, series_ids, stream, solve):
    like = ts
    ts, xs, lengths, observed, noise_var, dense, bn = _batch_args(m.B.shape[0], ts, xs, lengths, observed, noise_var)
    S = _sample_count(num_samples)
    d, obs, dt = m.N.shape[0], m.B.shape[0], m.N.dtype
    if not 1 <= d <= 8 or dt not in (torch.float32, torch.float64) or obs > MAX_PATTERN_OBS:
        raise ValueError("batched sampling is built for rank 1..8, obs_dim <= 8, float32 / float64")
    if not lengths:
        _series_ids_arg(series_ids, lengths, d, obs, "cpu")
        return torch.empty(((0, bn[1], d, S) if dense else (0, d, S)), dtype=dt, device=like.device)
    m, ts, xs, observed, noise_var = _on_gpu(m, ts, xs, observed, noise_var)
    ids = _series_ids_arg(series_ids, lengths, d, obs, m.N.device)
    plan = _cached_batch_plan(lengths, m.N.device)
    K_Rs, K_Os, out = _posterior_perturbation_flat(m, ts, xs, observed, noise_var, plan, ids, S, seed, stream)
    if solve:
        out = _solve_columns_models(K_Rs, K_Os, out, plan, None)
    out = cr._back(out, like)
    return out.reshape(bn[0], bn[1], d, S) if dense else out


def posterior_perturbation_batch(m, ts, xs, num_samples, seed, lengths=None, observed=None, noise_var=None,
                                 series_ids=None, stream=0):
    """The right-hand sides of ``sample_from_posterior_batch``: rhs = v + w with w ~ N(0, K), K the concatenated
    posterior precision of the batch (``insample_posterior_batch``'s system) and v its right-hand side, so that
    K^-1 rhs[:, :, s] is a posterior draw.  One kernel (cgps_leg_perturbation_seg) makes every row of every series and
    sample; the noise is generated in registers.  Arguments as ``sample_from_posterior_batch``; returns [B, n, rank, S]
    (dense) or [R, rank, S] (ragged).  For a caller with a factor of K of their own.

    Series b's rows depend only on (seed, stream, series_ids[b], its own ts / xs / observed / noise_var, the column s)
    -- bitwise: not on the series' position in the batch, on the other series, on the layout or on num_samples."""
    with torch.no_grad():
        return _perturbation_call(m, ts, xs, num_samples, seed, lengths, observed, noise_var, series_ids, stream, False)


def sample_from_posterior_batch(m, ts, xs, num_samples, seed, lengths=None, observed=None, noise_var=None,
                                series_ids=None, stream=0):
    """num_samples latent paths from the posterior of each of B independent series, in one call: [B, n, rank, S]
    (dense) or [R, rank, S] (ragged).  Layouts, ``lengths``, ``observed`` and ``noise_var``: exactly those of
    ``insample_posterior_batch`` (paths run through every row, observed or not; what xs and noise_var hold at unobserved
    entries is ignored, NaN included).  ``series_ids``: B integers in 0 .. 2^24 - 1 (a list or an integer tensor; read
    on the host), default 0 .. B-1, that name the series to the noise generator -- give a series the id it has in the
    whole data set and its draws are the same in every batch it appears in; two series with one id share their noise.
    ``stream``: the generator's stream word; the latent noise uses ``stream``, the observation noise ``stream + 1``.
    A series of n rows needs n max(rank, obs_dim) < 2^40.  No autograd graph.  B = 0 returns an empty tensor.  Every
    ValueError is raised before anything is launched.

    What is guaranteed.  The DISTRIBUTION is that of ``sample_from_posterior`` series by series, N(K_b^-1 v_b,
    K_b^-1), independent across series with different ids.  The NUMBERS are not those of ``sample_from_posterior``:
    that draws mean + (factor)^T eps off the cyclic-reduction factor, this is another sampler, perturb and solve:
    x = K^-1 (v + w) with w ~ N(0, K) summed from local pieces of noise.  The draw of a series depends
    only on (seed, stream, its id, its data, s): not on its position in the batch, on the other series, on the layout
    or on num_samples -- bitwise on the right-hand side (``posterior_perturbation_batch``), to the accuracy of the solve
    on the draw itself.  There is no per-series fallback to ``sample_from_posterior``.

    How: ``_posterior_system_rows`` (one assembly launch), one cgps_leg_perturbation_seg launch for the right-hand
    sides, ONE ``cr.decompose`` and ``cr.solve`` on column chunks of at most ``_sample_column_chunk(rank)`` columns.  A
    repeated call with the same lengths and default ids copies nothing from the host.  With
    ``cr.CHECK_POSITIVE_DEFINITE`` a zero-length gap or a block that is not positive definite raises ``cr.NotPSDError``
    naming the series and its local row.  CPU tensors: the work still runs on the GPU (there is no CPU implementation)
    and the result comes back to the CPU."""
    with torch.no_grad():
        return _perturbation_call(m, ts, xs, num_samples, seed, lengths, observed, noise_var, series_ids, stream, True)


def sample_from_prior_batch(m, ts, num_samples, seed, lengths=None, series_ids=None, stream=0):
    """num_samples latent paths of the LEG process at each of B independent series' times: ts [B, n] -> [B, n, rank, S],
    or ts [R] with host ``lengths`` -> [R, rank, S].  ``sample_from_posterior_batch`` without data: K is the prior
    precision (cgps_peg_precision_seg), there is no v and no observation noise.  ``series_ids``, ``stream`` and the
    guarantee as there: the distribution is ``sample_from_prior``'s latent paths series by series, the numbers are not,
    and a series' draw depends only on (seed, stream, its id, its times, s).  No autograd graph."""
    with torch.no_grad():
        like = ts
        dense = lengths is None
        shape = tuple(ts.shape)
        ts, _, lengths = _batch_layout(ts, ts.new_zeros(shape + (1,)) if dense else ts.new_zeros(shape[0] if shape else 0, 1),
                                       lengths)
        S = _sample_count(num_samples)
        d, dt = m.N.shape[0], m.N.dtype
        if not 1 <= d <= 8 or dt not in (torch.float32, torch.float64):
            raise ValueError("batched sampling is built for rank 1..8, float32 / float64")
        if not lengths:
            _series_ids_arg(series_ids, lengths, d, 1, "cpu")
            return torch.empty(((0, shape[1], d, S) if dense else (0, d, S)), dtype=dt, device=like.device)
        m, ts = _on_gpu(m, ts)
        ids = _series_ids_arg(series_ids, lengths, d, 1, m.N.device)
        plan = _cached_batch_plan(lengths, m.N.device)
        tsc, G = ts.to(dt).contiguous(), m.G.contiguous()
        rhs = _perturbation_models(tsc, G, plan, ids, _hip.H_NONE, None, None, None, S, seed, stream)   # (names a singular gap)
        Rs, Os = _peg_precision_models(tsc, G, plan.cut)
        out = cr._back(_solve_columns_models(Rs, Os, rhs, plan, None), like)
        return out.reshape(shape + (d, S)) if dense else out


# ---- sample paths and replicated observations under many models -----------------------------------
# The models axis of perturb and solve: the right-hand sides of the system "model 0's batch, then model 1's batch, ..."
# come from ONE cgps_leg_perturbation_models launch, every model under a stream word of its own, and one factorisation
# of the concatenated system solves them all.  A model owns four consecutive words: w (latent noise), w + 1
# (observation noise of the perturbation), w + 2 (replicated observations, cgps_leg_observations), w + 3 (spare).
MAX_STREAM_WORD = (1 << 32) - 4
MODEL_STREAM_STRIDE = 4


def _model_stream_words(M, stream, model_streams):
    """The M stream words of a ``*_models`` sampler as a list of ints, each in 0 .. 2^32 - 4 (ValueError otherwise):
    ``model_streams`` (a list or a 1-d integer tensor of M words) or stream + 4 k."""
    if model_streams is None:
        words = [int(stream) + MODEL_STREAM_STRIDE * k for k in range(M)]
    else:
        if isinstance(model_streams, torch.Tensor):
            if model_streams.dim() != 1 or model_streams.dtype.is_floating_point or model_streams.dtype == torch.bool:
                raise ValueError("model_streams must be a list or a 1-d integer tensor")
            model_streams = model_streams.tolist()
        words = [int(w) for w in model_streams]
        if len(words) != M:
            raise ValueError("model_streams names %d words, there are %d models" % (len(words), M))
    bad = [(k, w) for k, w in enumerate(words) if not 0 <= w <= MAX_STREAM_WORD]
    if bad:
        raise ValueError("model %d: stream word %d outside 0 .. 2^32 - 4" % bad[0])
    return words


def _sampling_kernels_built(d, obs, dt):
    if not 1 <= d <= 8 or dt not in (torch.float32, torch.float64) or obs > MAX_PATTERN_OBS:
        raise ValueError("batched sampling is built for rank 1..8, obs_dim <= 8, float32 / float64")


def _models_on_gpu(ms, *tensors):
    """``_on_gpu`` for a list of models that share a device."""
    dev = ms[0].N.device if ms[0].N.is_cuda else cr._device()
    return [m if m.N.is_cuda else m.to(dev) for m in ms], tuple(None if t is None else t.to(dev) for t in tensors)


def _models_noise_factors(ms, observed=None, noise_var=None):
    """``observation_noise_factors`` of every model, stacked: [M, rank, obs] (neither argument), [M, 2^obs, rank, obs]
    (``observed``) or [M, n, rank, obs] (``noise_var``).  Model k's slice is ``observation_noise_factors(ms[k], ...)``
    itself, evaluated on that model alone -- see ``_models_sampling_operands``."""
    return torch.stack([observation_noise_factors(m, observed, noise_var) for m in ms]).contiguous()


def _models_sampling_operands(ms, ts, xs, observed, noise_var):
    """What the samplers over many models read, stacked: (G [M, d, d], source, term, rows, v [M, R, d], hsource, hterm,
    pattern) -- (source, term, rows) for ``_posterior_blocks_models``, (hsource, hterm, pattern) for
    ``_perturbation_models``.  Slot k of a ``*_models`` sampler is promised to be the one-model call's right-hand sides
    BIT FOR BIT, so every operand the perturbation kernel reads must carry the one-model path's own rounding: G, v and
    the H factors are evaluated by that path's functions (``LEGMatrices.G``, ``_posterior_operands_batch``,
    ``observation_noise_factors``), model by model on unchanged shapes, and stacked.  The elementwise stacked forms of
    ``_models_posterior_operands`` round differently from those GEMM-based ones: they agree to an
    ulp, not to the bit.  The cost is a few dozen small launches per model, independent of the batch."""
    dt = ms[0].N.dtype
    parts = [_posterior_operands_batch(m, ts, xs, observed, noise_var) for m in ms]
    source = parts[0][0]
    G = torch.stack([m.G for m in ms]).contiguous()
    term = torch.stack([p[1] for p in parts])
    v = torch.stack([p[3] for p in parts])
    rows = torch.stack([p[2] for p in parts]) if source == _hip.ROWS_WEIGHTED else parts[0][2]
    hsource, pattern = _noise_source(rows, observed, noise_var)
    return G, source, term, rows, v, hsource, _models_noise_factors(ms, observed, noise_var).to(dt), pattern


def _stack_model_chunks(parts, M, R):
    """[M, R, ...] from the chunks' [m R, ...] results (a view when there is one chunk)."""
    out = _cat_chunks(parts)
    return out.view((M, R) + tuple(out.shape[1:]))


def _perturbation_models_call(ms, ts, xs, num_samples, seed, lengths, observed, noise_var, series_ids, stream,
                              model_streams, solve):
    like = ts
    ms, mats, ts, xs, lengths, observed, noise_var, dense, bn = _models_posterior_args(ms, ts, xs, lengths, observed,
                                                                                      noise_var)
    S = _sample_count(num_samples)
    M, d, obs, dt = len(ms), mats[0].shape[1], mats[2].shape[1], mats[0].dtype
    _sampling_kernels_built(d, obs, dt)
    words = _model_stream_words(M, stream, model_streams)
    if not lengths:
        _series_ids_arg(series_ids, lengths, d, obs, "cpu")
        return torch.empty(((M, 0, bn[1], d, S) if dense else (M, 0, d, S)), dtype=dt, device=like.device)
    ms, (ts, xs, observed, noise_var) = _models_on_gpu(ms, ts, xs, observed, noise_var)
    dev = ms[0].N.device
    ids = _series_ids_arg(series_ids, lengths, d, obs, dev)
    plan = _cached_batch_plan(lengths, dev)
    R = plan.R
    G, source, term, rows, v, hsource, hterm, pattern = _models_sampling_operands(ms, ts, xs, observed, noise_var)
    tsc, wd = ts.to(dt).contiguous(), torch.tensor(words, dtype=torch.int64).to(dev)
    parts = []
    for k0, k1, sel in _model_chunks(G, R, MODELS_POSTERIOR_MAX_ROWS):
        rhs = _perturbation_models(tsc, G[sel], plan, ids, hsource, hterm[sel], pattern, v[sel], S, seed, wd[sel], k0)
        if solve:
            K_Rs, K_Os, info = _posterior_blocks_models(tsc, G[sel], plan.cut, source, term[sel],
                                                        rows if source != _hip.ROWS_WEIGHTED else rows[sel])
            # (a singular gap was named by the perturbation already: both kernels evaluate the gaps the same way)
            rhs = _solve_columns_models(K_Rs, K_Os, rhs, plan, k0)
            del K_Rs, K_Os
        parts.append(rhs)
    out = cr._back(_stack_model_chunks(parts, M, R), like)
    return out.reshape(M, bn[0], bn[1], d, S) if dense else out


def posterior_perturbation_models(ms, ts, xs, num_samples, seed, lengths=None, observed=None, noise_var=None,
                                  series_ids=None, stream=0, model_streams=None):
    """The right-hand sides of ``sample_from_posterior_models``: [M, B, n, rank, S] (dense) or [M, R, rank, S] (ragged),
    slot k ``posterior_perturbation_batch(ms[k], ..., stream=w_k)`` bit for bit, from ONE cgps_leg_perturbation_models
    launch per chunk of whole models.  Arguments as ``sample_from_posterior_models`` without ``observations``.  For a
    caller with a factor of the concatenated system of their own."""
    with torch.no_grad():
        return _perturbation_models_call(ms, ts, xs, num_samples, seed, lengths, observed, noise_var, series_ids, stream,
                                         model_streams, False)


def sample_from_posterior_models(ms, ts, xs, num_samples, seed, lengths=None, observed=None, noise_var=None,
                                 series_ids=None, stream=0, model_streams=None, observations=False):
    """``sample_from_posterior_batch`` of M LEG models for the same B series in one call: joint latent paths under
    every random start of a fit, every chain of a population, every point of a grid or every component of a mixture.
    Returns [M, B, n, rank, S] (dense) or [M, R, rank, S] (ragged); slot k is
    ``sample_from_posterior_batch(ms[k], ..., stream=w_k)`` -- bitwise on the right-hand sides
    (``posterior_perturbation_models``), to the accuracy of the solve on the draws.  No autograd graph.

    ``ms``, ``ts`` / ``xs`` / ``lengths``, ``observed`` and ``noise_var``: exactly those of ``insample_posterior_models``,
    with its ValueErrors; the mask and the variances belong to the data and are shared by the models.  ``series_ids``
    as in ``sample_from_posterior_batch``.  The stream words: ``model_streams`` (a list or an integer tensor of M words,
    each in 0 .. 2^32 - 4; read on the host) gives w_k; equal words give the models common random numbers (the same
    noise pushed through every model: what a comparison of models wants).  Otherwise w_k = ``stream`` + 4 k, a
    ValueError if that leaves the range: a model owns w_k (latent noise), w_k + 1 (observation noise) and w_k + 2
    (replicated observations), so models with the default words are independent.  Every ValueError is raised before
    anything is launched; B = 0 returns empty tensors with leading dimension M.

    ``observations=True`` returns (z, x) with x = ``sample_observations_models(ms, z, seed, ...)`` on the same words:
    one replicated data set per path, [M, B, n, obs_dim, S] or [M, R, obs_dim, S].

    How: every model's operands from the one-model path's own functions, stacked (``_models_sampling_operands``: that
    is what makes slot k bitwise); then per chunk of whole models (MODELS_POSTERIOR_MAX_ROWS) ONE
    cgps_leg_perturbation_models, ONE cgps_leg_posterior_blocks_models, ONE ``cr.decompose`` and ``cr.solve`` on column
    chunks.  Every rank 1..8, obs_dim <= 8, both precisions.  With ``cr.CHECK_POSITIVE_DEFINITE`` a
    zero-length gap or a block that is not positive definite raises ``cr.NotPSDError`` naming the model, the series and
    its local row (a zero-length gap belongs to the data: the first model of the call meets it).  CPU tensors: the work
    runs on the GPU and the result comes back to the CPU."""
    with torch.no_grad():
        ms = list(ms)
        z = _perturbation_models_call(ms, ts, xs, num_samples, seed, lengths, observed, noise_var, series_ids, stream,
                                      model_streams, True)
        if not observations:
            return z
        words = _model_stream_words(len(z), stream, model_streams)
        return z, sample_observations_models(ms, z, seed, lengths, observed, noise_var, series_ids, model_streams=words)


def sample_from_prior_models(ms, ts, num_samples, seed, lengths=None, series_ids=None, stream=0, model_streams=None):
    """``sample_from_prior_batch`` of M LEG models at the same B series' times in one call: ts [B, n] ->
    [M, B, n, rank, S], or ts [R] with host ``lengths`` -> [M, R, rank, S]; slot k is
    ``sample_from_prior_batch(ms[k], ..., stream=w_k)``, the stream words as in ``sample_from_posterior_models``.  K is
    the prior precision of every model (cgps_peg_precision_models where that kernel is built, otherwise
    cgps_leg_posterior_blocks_models with a zero plain term), there is no v and no observation noise.  No autograd
    graph."""
    with torch.no_grad():
        like = ts
        ms, mats = _models_operands(ms)
        dense = lengths is None
        shape = tuple(ts.shape)
        ts, _, lengths = _batch_layout(ts, ts.new_zeros(shape + (1,)) if dense else ts.new_zeros(shape[0] if shape else 0, 1),
                                       lengths)
        S = _sample_count(num_samples)
        M, d, dt = len(ms), mats[0].shape[1], mats[0].dtype
        _sampling_kernels_built(d, 1, dt)
        words = _model_stream_words(M, stream, model_streams)
        if not lengths:
            _series_ids_arg(series_ids, lengths, d, 1, "cpu")
            return torch.empty(((M, 0, shape[1], d, S) if dense else (M, 0, d, S)), dtype=dt, device=like.device)
        ms, (ts,) = _models_on_gpu(ms, ts)
        dev = ms[0].N.device
        ids = _series_ids_arg(series_ids, lengths, d, 1, dev)
        plan = _cached_batch_plan(lengths, dev)
        R = plan.R
        G = torch.stack([m.G for m in ms]).contiguous()
        tsc, wd = ts.to(dt).contiguous(), torch.tensor(words, dtype=torch.int64).to(dev)
        peg = batch_supported(tsc, G[0])                           # (cgps_peg_precision_models: d <= 7, not fp64 d = 6)
        parts = []
        for k0, k1, sel in _model_chunks(G, R, MODELS_POSTERIOR_MAX_ROWS):
            rhs = _perturbation_models(tsc, G[sel], plan, ids, _hip.H_NONE, None, None, None, S, seed, wd[sel], k0)
            if peg:
                Rs, Os = _peg_precision_models(tsc, G[sel], plan.cut)
            else:
                Rs, Os, _ = _posterior_blocks_models(tsc, G[sel], plan.cut, _hip.ROWS_PLAIN,
                                                     torch.zeros(k1 - k0, d, d, dtype=dt, device=dev))
            parts.append(_solve_columns_models(Rs, Os, rhs, plan, k0))
            del Rs, Os
        out = cr._back(_stack_model_chunks(parts, M, R), like)
        return out.reshape((M,) + shape + (d, S)) if dense else out


# Replicated observations: data sets drawn from the observation model given latent paths -- from the posterior
# predictive when the paths are posterior draws: what a posterior predictive check compares the data with.
def _observations_rows(z, pattern, noise_var, plan, ids, Bm, LLT, seed, words):
    """x [M R, obs, S] of cgps_leg_observations: z [M R, d, S], pattern uint8 [R] or None, noise_var [R, obs] or None,
    Bm [M, obs, d], LLT [M, obs, obs], words device int64 [M]; contiguous, of one dtype.  Returns (x, info)."""
    (M, obs, d), S, R, dt = Bm.shape, z.shape[2], plan.R, z.dtype
    x = torch.empty(M * R, obs, S, dtype=dt, device=z.device)
    info = torch.zeros(1, dtype=torch.int32, device=z.device)
    _hip.check(_hip.lib().cgps_leg_observations(
        _hip.ptr(z), _hip.ptr(pattern), _hip.ptr(noise_var), _hip.ptr(plan.offsets), _hip.ptr(ids), plan.B, R, M, _hip.ptr(Bm),
        _hip.ptr(LLT), d, obs, _hip.dtype_code(dt), S, int(seed) & 0xFFFFFFFFFFFFFFFF, _hip.ptr(words), _hip.ptr(x),
        _hip.ptr(info), _hip.stream_ptr()))
    return x, info


def _observations_call(ms, z, seed, lengths, observed, noise_var, series_ids, words, models):
    """``sample_observations_models`` (``models``: z has the leading model axis) and ``sample_observations_batch``."""
    like = z
    lead = 1 if models else 0
    ms, mats = _models_operands(ms)
    M, d, obs, dt = len(ms), mats[0].shape[1], mats[2].shape[1], mats[0].dtype
    _sampling_kernels_built(d, obs, dt)
    dense = lengths is None
    if not isinstance(z, torch.Tensor) or not z.dtype.is_floating_point or z.dim() != lead + (4 if dense else 3):
        raise ValueError("z must be a floating-point tensor %s[B, n, rank, S] (dense) or %s[sum(lengths), rank, S] (ragged)"
                         % (("[M]",) * 2 if models else ("",) * 2))
    if (models and z.shape[0] != M) or z.shape[-2] != d or z.shape[-1] < 1:
        raise ValueError("z %s does not fit %d models of rank %d with at least one sample" % (tuple(z.shape), M, d))
    S = z.shape[-1]
    rows_shape = tuple(z.shape[lead:-2])                           # (B, n) or (R,)
    xs_shape = rows_shape + (obs,)
    # (the layout checks of the other batched calls, on storage-free stand-ins for ts and xs of the right shapes)
    _, _, lengths, observed, noise_var = _batch_args(obs, torch.empty(rows_shape, device="meta"),
                                                     torch.empty(xs_shape, device="meta"), lengths, observed, noise_var)[:5]
    out_shape = tuple(z.shape[:-2]) + (obs, S)
    if not lengths:
        _series_ids_arg(series_ids, lengths, d, obs, "cpu")
        return torch.empty(out_shape, dtype=dt, device=like.device)
    ms, (z, observed, noise_var) = _models_on_gpu(ms, z, observed, noise_var)
    dev = ms[0].N.device
    ids = _series_ids_arg(series_ids, lengths, d, obs, dev)
    plan = _cached_batch_plan(lengths, dev)
    _, pattern, nv = _loo_data(z.new_zeros(0, obs), observed, noise_var, dt)
    Bm = mats[2].to(dev).contiguous()
    LLT = torch.stack([m.LLT for m in ms]).to(dt).contiguous()     # (each model's own LLT, as the one-model calls form it)
    wd = torch.tensor(words, dtype=torch.int64).to(dev)
    x, info = _observations_rows(z.to(dt).reshape(M * plan.R, d, S).contiguous(), pattern, nv, plan, ids, Bm, LLT, seed, wd)
    if cr.CHECK_POSITIVE_DEFINITE:
        bad = int(info.item())
        if bad:
            k, b, r = _locate_row(plan, bad - 1)
            raise cr.NotPSDError("LEG replicated observations: model %d, series %d: the noise covariance of its row %d is "
                                 "not positive definite (a negative noise_var?)" % (k, b, r))
    return cr._back(x, like).reshape(out_shape)


def sample_observations_batch(m, z, seed, lengths=None, observed=None, noise_var=None, series_ids=None, stream=0):
    """Replicated observations of latent paths of B series, in one launch: z [B, n, rank, S] (dense) or [R, rank, S]
    with host ``lengths`` (the samplers' layouts) -> x [B, n, obs_dim, S] or [R, obs_dim, S],
    x = B z + T eps'' with T T^T = Lambda Lambda^T + 1e-9 I + diag(s_row): the distribution of the data at EVERY row,
    observed or not, given the paths -- with z from ``sample_from_posterior_batch`` a draw from the posterior
    predictive, the replicated data sets of a posterior predictive check.  ``noise_var`` ([.., obs_dim] or one value
    per row) adds the row's own variances where ``observed`` (bool, same layouts; None: everywhere) says the entry was
    measured; at unobserved entries s is 0 and noise_var is not read (NaN included).  ``series_ids`` as in the
    samplers.  The noise is generated in registers (cgps_leg_observations) under stream word ``stream`` + 2: with the
    ``stream`` of the sampler that made z it is independent of the two words that draw used, and a series' replicate
    depends only on (seed, stream, its id, its rows, s) -- not on its place in the batch or on S, bitwise.  No autograd
    graph.  CPU tensors run on the GPU and come back."""
    with torch.no_grad():
        if not isinstance(m, LEGMatrices):
            raise ValueError("m is not a LEGMatrices")
        return _observations_call([m], z, seed, lengths, observed, noise_var, series_ids, _model_stream_words(1, stream, None),
                                  False)


def sample_observations_models(ms, z, seed, lengths=None, observed=None, noise_var=None, series_ids=None, stream=0,
                               model_streams=None):
    """``sample_observations_batch`` under M models in ONE launch: z [M, B, n, rank, S] or [M, R, rank, S] (what
    ``sample_from_posterior_models`` returns) -> x [M, B, n, obs_dim, S] or [M, R, obs_dim, S]; slot k is
    ``sample_observations_batch(ms[k], z[k], ..., stream=w_k)`` bit for bit, w_k from ``model_streams`` or
    ``stream`` + 4 k as in ``sample_from_posterior_models``.  The mask and the variances belong to the data and are
    shared by the models."""
    with torch.no_grad():
        ms = list(ms)
        return _observations_call(ms, z, seed, lengths, observed, noise_var, series_ids,
                                  _model_stream_words(len(ms), stream, model_streams), True)


# ---- observations that are not Gaussian: the Laplace approximation ----------------------------------
LaplacePosterior = collections.namedtuple("LaplacePosterior", ["mean", "cov", "log_evidence", "iterations", "converged"])

_FAMILIES = {"poisson": _hip.GLM_POISSON, "bernoulli": _hip.GLM_BERNOULLI, "gaussian": _hip.GLM_GAUSSIAN}
GLM_CANDIDATES = 12
"""Step lengths 1, 1/2, .., 2^-11 of the damped Newton step (cgps_leg_glm_step tries the same)."""
LAPLACE_TOL = {torch.float64: 1e-16, torch.float32: 1e-9}
"""``tol=None``: a series has converged once a step's gain is <= tol (1 + |psi|).  The gain of a Newton step is about
half its squared length in the metric of J, and the point it lands on is within about that squared length of the
mode: these leave the mode at rounding level in either precision.  They are also well above what rounding does to
the gain itself, about eps^2 |z|^2 |J| cond(J) (the step is then noise, and so is its gain): a smaller tolerance
would be met by chance or not at all."""
_LOG_EXPOSURE = ("log_exposure", "a floating-point tensor", lambda dtype: dtype.is_floating_point)


class _GlmOperands:
    """What every step of one call reads, contiguous and of the model's dtype: the prior blocks (written once), the
    data, the pattern bytes (None: everything observed), offset and extra (None: zeros), B, the plan."""

    def __init__(self, plan, Rs, Os, ys, observed, offset, extra, Bm, family, tol):
        self.plan, self.Rs, self.Os, self.ys, self.observed = plan, Rs, Os, ys, observed
        self.offset, self.extra, self.Bm, self.family, self.tol = offset, extra, Bm, family, float(tol)
        obs = ys.shape[1]
        self.pattern = None
        if observed is not None:
            self.pattern = (observed * (1 << torch.arange(obs, device=observed.device))).sum(1).to(torch.uint8).contiguous()


def _glm_step_hip(op, z, prop, state):
    """One launch of cgps_leg_glm_step: (z_out, J_Rs, rhs, state_out)."""
    R, d = z.shape
    dt, dev = z.dtype, z.device
    z_out = torch.empty(R, d, dtype=dt, device=dev)
    J_Rs = torch.empty(R, d, d, dtype=dt, device=dev)
    rhs = torch.empty(R, d, dtype=dt, device=dev)
    state_out = torch.empty(op.plan.B, _hip.GLM_STATE, dtype=torch.float64, device=dev)
    P = _hip.ptr
    _hip.check(_hip.lib().cgps_leg_glm_step(
        P(z), P(prop), P(op.Rs), P(op.Os), P(op.ys), P(op.pattern), P(op.offset), P(op.extra), P(op.Bm), P(op.plan.offsets),
        op.plan.B, R, d, op.ys.shape[1], _hip.dtype_code(dt), op.family, op.tol, P(state), P(z_out), P(J_Rs), P(rhs),
        P(state_out), _hip.stream_ptr()))
    return z_out, J_Rs, rhs, state_out


def _glm_point(family, y, eta, s):
    """(log density, its derivative g, the weight w = -l'', the factor of ``_glm_diff``, ``up``) at the linear predictor
    eta; ``up``: Bernoulli entries with eta > 0, whose line difference is taken on the mirror image (None elsewhere)"""
    if family == _hip.GLM_POISSON:
        e = torch.exp(eta)
        return y * eta - e, y - e, e, e, None
    if family == _hip.GLM_BERNOULLI:
        e = torch.exp(-eta.abs())
        r = 1.0 / (1.0 + e)
        sig = torch.where(eta >= 0, r, e * r)
        return y * eta - (eta.clamp(min=0) + torch.log1p(e)), y - sig, e * r * r, e * r, eta > 0
    inv, res = 1.0 / s, y - eta
    return -0.5 * res * res * inv - 0.5 * torch.log(2 * math.pi * s), res * inv, inv, inv, None


def _glm_diff(family, y, g, base, up, t):
    """l(eta + t) - l(eta) with nothing of the size of l cancelling: the arithmetic of ``glm_diff`` (csrc/cgps_leg_glm.h).
    Bernoulli: from the side on which sigma <= 1/2, i.e. on the mirror image (1 - y, -t) where eta > 0; base =
    sigma(-|eta|), so the argument of log1p stays at or above -1/2."""
    if family == _hip.GLM_POISSON:
        return y * t - base * torch.expm1(t)
    if family == _hip.GLM_BERNOULLI:
        ym, tm = torch.where(up, 1.0 - y, y), torch.where(up, -t, t)
        return ym * tm - torch.log1p(base * torch.expm1(tm))
    return t * (g - 0.5 * t * base)


def _glm_step_composed(op, z, prop, state):
    """The step of cgps_leg_glm_step as torch passes over [R, obs] and [R, d, d] arrays (CGPS_LEG_GLM_COMPOSED=1): the same
    arithmetic in the arrays' dtype, the sums per series in fp64 (``index_add_``: not in a fixed order).  For A/B timing,
    and the yardstick of the kernel's fp32 error."""
    plan, fam, dt = op.plan, op.family, z.dtype
    F64 = torch.float64
    B, R = plan.B, z.shape[0]
    seg = plan.per_row(torch.arange(B, device=z.device))
    mask = op.observed if op.observed is not None else torch.ones_like(op.ys, dtype=torch.bool)
    zero = z.new_zeros(())

    def ssum(x):
        return torch.zeros(B, dtype=F64, device=z.device).index_add_(0, seg, x.to(F64))

    def quad(u, v):
        q = (u * (op.Rs @ v.unsqueeze(-1)).squeeze(-1)).sum(-1).to(F64)
        if R > 1:
            Ov, Ou = (op.Os @ v[:-1].unsqueeze(-1)).squeeze(-1), (op.Os @ u[:-1].unsqueeze(-1)).squeeze(-1)
            c = torch.where(plan.cut == 0, ((u[1:] * Ov).sum(-1) + (v[1:] * Ou).sum(-1)).to(F64), zero.to(F64))
            q = q + torch.cat([c, c.new_zeros(1)])
        return ssum(q)

    def predictor(zz):
        bz = zz @ op.Bm.T
        eta = bz if op.offset is None else bz + op.offset
        if fam != _hip.GLM_GAUSSIAN and op.extra is not None:
            eta = eta + op.extra
        return bz, eta

    s = op.extra if fam == _hip.GLM_GAUSSIAN else None
    if prop is None:
        active = torch.zeros(B, dtype=torch.bool, device=z.device)
        delta = torch.zeros_like(z)
        iters = torch.zeros(B, dtype=F64, device=z.device)
    else:
        active = state[:, 2] == 0
        delta = torch.where(active[seg].unsqueeze(-1), prop - z, zero)
        iters = state[:, 1]
    qa, qb, qc = quad(z, z), quad(z, delta), quad(delta, delta)
    _, eta0 = predictor(z)
    de = delta @ op.Bm.T
    _, g0, _, base0, up0 = _glm_point(fam, op.ys, eta0, s)
    gd = ssum(torch.where(mask, g0 * de, zero).sum(-1))
    alpha = torch.zeros(B, dtype=F64, device=z.device)
    gain, found = torch.zeros_like(alpha), torch.zeros_like(active)
    for k in range(GLM_CANDIDATES):
        ak = 0.5 ** k
        gk = ssum(torch.where(mask, _glm_diff(fam, op.ys, g0, base0, up0, ak * de), zero).sum(-1)) - ak * qb - 0.5 * ak * ak * qc
        ok = active & ~found & (gk >= 0) & torch.isfinite(gk)
        alpha, gain, found = torch.where(ok, ak, alpha), torch.where(ok, gk, gain), found | ok
    a_row = alpha[seg].to(dt).unsqueeze(-1)
    z_out = z if prop is None else torch.where(a_row == 1, prop, torch.where(a_row == 0, z, z + a_row * (prop - z)))
    bz, eta = predictor(z_out)
    l, g, w, _, _ = _glm_point(fam, op.ys, eta, s)
    wm, u = torch.where(mask, w, zero), torch.where(mask, w * bz + g, zero)
    J_Rs = op.Rs + torch.einsum("rc,ca,cb->rab", wm, op.Bm, op.Bm)
    rhs = u @ op.Bm
    psi = ssum(torch.where(mask, l, zero).sum(-1)) - 0.5 * (qa + 2 * alpha * qb + alpha * alpha * qc)
    bound = op.tol * (1 + psi.abs())
    conv = torch.where(found, gain <= bound, (gd - qb).abs() <= bound)
    flags = torch.where(conv, float(_hip.GLM_CONVERGED), torch.where(found, 0.0, float(_hip.GLM_STALLED)))
    out = torch.stack([psi, iters + 1, flags.to(F64), alpha], 1)
    if prop is None:
        out[:, 1:] = 0
    else:
        out = torch.where(active.unsqueeze(-1), out, state)
    return z_out.contiguous(), J_Rs.contiguous(), rhs.contiguous(), out


def _glm_step(op, z, prop, state):
    if os.environ.get("CGPS_LEG_GLM_COMPOSED") == "1":
        return _glm_step_composed(op, z, prop, state)
    return _glm_step_hip(op, z, prop, state)


def _laplace_args(m, ts, ys, lengths, family, observed, offset, log_exposure, noise_var, init, max_iter, tol, on_gpu=True):
    """Everything the Laplace calls check, before anything is launched: (family code, ts [R], ys [R, obs], lengths,
    observed [R, obs] or None, offset [obs] or None, extra [R, obs] or None, init [R, d] or None, dense, (B, n), tol).
    ``on_gpu=False`` leaves the refusal of CPU tensors to a caller that has ValueErrors of its own to raise first."""
    if family not in _FAMILIES:
        raise ValueError("family must be one of %s, got %r" % (sorted(_FAMILIES), family))
    fam = _FAMILIES[family]
    d, obs, dt = m.N.shape[0], m.B.shape[0], m.N.dtype
    if obs > MAX_PATTERN_OBS:
        raise ValueError("the Laplace posterior is built for obs_dim <= %d, got %d" % (MAX_PATTERN_OBS, obs))
    if not 1 <= d <= 8 or dt not in (torch.float32, torch.float64):
        raise ValueError("the Laplace posterior is built for rank 1..8, float32 / float64")
    if not isinstance(ts, torch.Tensor) or not isinstance(ys, torch.Tensor):
        raise ValueError("ts and ys must be tensors")
    dense, ys_shape = lengths is None, tuple(ys.shape)
    if fam == _hip.GLM_GAUSSIAN and noise_var is None:
        raise ValueError("family 'gaussian' needs noise_var, the variance of every observed entry")
    if fam != _hip.GLM_GAUSSIAN and noise_var is not None:
        raise ValueError("noise_var belongs to family 'gaussian', got family %r" % family)
    if fam == _hip.GLM_GAUSSIAN and log_exposure is not None:
        raise ValueError("log_exposure belongs to the families 'poisson' and 'bernoulli'")
    ts, ys, lengths, observed, noise_var, dense, bn = _batch_args(obs, ts, ys, lengths, observed, noise_var)
    if log_exposure is not None:
        log_exposure = _batch_like_xs(log_exposure, _LOG_EXPOSURE, ys_shape, dense)
    extra = noise_var if fam == _hip.GLM_GAUSSIAN else log_exposure
    if extra is not None and extra.dim() == 1:
        extra = extra.unsqueeze(-1).expand(-1, obs)
    if offset is not None and (not isinstance(offset, torch.Tensor) or not offset.dtype.is_floating_point or
                               tuple(offset.shape) != (obs,)):
        raise ValueError("offset must be a floating-point tensor [%d]" % obs)
    if init is not None:
        want = (bn[0], bn[1], d) if dense else (ts.shape[0], d)
        if not isinstance(init, torch.Tensor) or not init.dtype.is_floating_point or tuple(init.shape) != want:
            raise ValueError("init must be a floating-point tensor %s, the shape of the mean" % (want,))
        init = init.reshape(-1, d)
    if int(max_iter) != max_iter or max_iter < 0:
        raise ValueError("max_iter must be a non-negative integer, got %r" % (max_iter,))
    if tol is None:
        tol = LAPLACE_TOL[dt]
    elif not tol >= 0:
        raise ValueError("tol must be >= 0, got %r" % (tol,))
    tensors = [t for t in (m.N, ts, ys, observed, offset, extra, init) if t is not None]
    if on_gpu and lengths and not all(t.is_cuda for t in tensors):
        raise _hip.CgpsError("the Laplace posterior runs on GPU tensors only (there is no CPU implementation)")
    return fam, ts, ys, lengths, observed, offset, extra, init, dense, bn, float(tol)


def _laplace_flat(m, fam, ts, ys, lengths, observed, offset, extra, init, max_iter, tol, saved=None):
    """The Newton loop on the concatenated batch: (mean [R, d], cov_diag, cov_off, log_evidence [B], iterations [B],
    converged [B]).  ``saved``: a dict that receives the operands of the evidence's backward (``_LaplaceEvidenceFn``)."""
    d, dt, dev = m.N.shape[0], m.N.dtype, m.N.device
    plan = _cached_batch_plan(lengths, dev)
    c = lambda t: None if t is None else t.to(dt).contiguous()       # noqa: E731
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    Rs, Os = _peg_precision_seg(ts.to(dt).contiguous(), m.G.contiguous(), plan.cut, info)     # once per call
    _check_gaps(info, plan, None, _GAP_BLOCK)
    ys = c(ys)
    op = _GlmOperands(plan, Rs, Os, ys, None if observed is None else observed.contiguous(), c(offset), c(extra), c(m.B), fam, tol)
    z = torch.zeros(plan.R, d, dtype=dt, device=dev) if init is None else cr._aligned16(c(init))
    z, J_Rs, rhs, state = _glm_step(op, z, None, None)
    for _ in range(int(max_iter)):
        _, prop = cr.decompose_solve(J_Rs, Os, rhs)
        z, J_Rs, rhs, state = _glm_step(op, z, prop, state)
        if bool((state[:, 2] != 0).all()):                           # one flag read on the host per iteration
            break
    dec = cr.decompose(J_Rs, Os)                                    # J at the mode: the step wrote it at z_out
    Sd, So = cr.inverse_blocks(dec)
    if plan.B > 1:
        So.index_fill_(0, plan.boundary_rows(1), 0)
    _, logdet_J = cr.mahal_and_det_batch(J_Rs, Os, None, lengths=lengths)
    _, logdet_K = cr.mahal_and_det_batch(Rs, Os, None, lengths=lengths)
    ev = state[:, 0] + 0.5 * (logdet_K.to(torch.float64) - logdet_J.to(torch.float64))
    if fam == _hip.GLM_POISSON:                                      # the term of log p that does not depend on eta
        lg = torch.lgamma(ys.to(torch.float64) + 1)
        if observed is not None:
            lg = torch.where(observed, lg, lg.new_zeros(()))
        ev = ev - torch.zeros_like(ev).index_add_(0, plan.per_row(torch.arange(plan.B, device=dev)), lg.sum(-1))
    conv = (state[:, 2].to(torch.int64) & _hip.GLM_CONVERGED) != 0
    if saved is not None:                                            # what the gradient of the evidence reads
        s_rhs = _glm_evidence_rhs(op, z, Sd)
        u = torch.zeros_like(s_rhs) if fam == _hip.GLM_GAUSSIAN else cr._solve_raw(dec, s_rhs)
        Pd, Po = cr.inverse_blocks(cr.decompose(Rs, Os))
        saved.update(op=op, z=z, u=u, Sd=Sd, So=So, Pd=Pd, Po=Po, conv=conv, ts=ts.to(dt).contiguous(), G=m.G.contiguous())
    return z, Sd, So, ev, state[:, 1].to(torch.int64), conv


# ---- the gradient of the Laplace evidence at the mode -------------------------------------------------
def _glm_composed():
    return os.environ.get("CGPS_LEG_GLM_COMPOSED") == "1"


def _glm_evidence_rhs_hip(op, z, Sd):
    """One launch of cgps_leg_glm_evidence_rhs: s [R, d] = dE / dz at the mode."""
    R, d = z.shape
    s = torch.empty(R, d, dtype=z.dtype, device=z.device)
    P = _hip.ptr
    _hip.check(_hip.lib().cgps_leg_glm_evidence_rhs(
        P(z), P(Sd), P(op.ys), P(op.pattern), P(op.offset), P(op.extra), P(op.Bm), R, d, op.ys.shape[1],
        _hip.dtype_code(z.dtype), op.family, P(s), _hip.stream_ptr()))
    return s


def _glm_evidence_adjoint_hip(op, z, u, Sd, So, Pd, Po, gE):
    """One call of cgps_leg_glm_evidence_adjoint: (gRs [R, d, d], gOs [R - 1, d, d], g_extra [R, obs], gB_part
    [B, obs, d], goffset_part [B, obs]), the last two fp64 and per series."""
    R, d = z.shape
    dt, dev, obs, B = z.dtype, z.device, op.ys.shape[1], op.plan.B
    gRs = torch.empty(R, d, d, dtype=dt, device=dev)
    gOs = torch.empty(R - 1, d, d, dtype=dt, device=dev)
    g_extra = torch.empty(R, obs, dtype=dt, device=dev)
    gB_part = torch.empty(B, obs, d, dtype=torch.float64, device=dev)
    goffset_part = torch.empty(B, obs, dtype=torch.float64, device=dev)
    P = _hip.ptr
    _hip.check(_hip.lib().cgps_leg_glm_evidence_adjoint(
        P(z), P(u), P(Sd), P(So), P(Pd), P(Po), P(op.ys), P(op.pattern), P(op.offset), P(op.extra), P(op.Bm),
        P(op.plan.offsets), P(gE), B, R, d, obs, _hip.dtype_code(dt), op.family, P(gRs), P(gOs), P(g_extra), P(gB_part),
        P(goffset_part), _hip.stream_ptr()))
    return gRs, gOs, g_extra, gB_part, goffset_part


def _glm_wprime(family, eta, w):
    """dw / d eta: the arithmetic of ``glm_wprime`` (csrc/cgps_leg_glm_grad.h)"""
    if family == _hip.GLM_POISSON:
        return w
    if family == _hip.GLM_BERNOULLI:
        e = torch.exp(-eta.abs())
        t = (1.0 - e) / (1.0 + e)
        return torch.where(eta >= 0, -w * t, w * t)
    return torch.zeros_like(w)


def _glm_evidence_entries(op, z, Sd):
    """(mask, g, w, w', v, S B^T [R, obs, d]) of every entry at z, as torch passes; g, w, w' are zero where nothing is
    observed (whatever ys and extra hold there)."""
    fam = op.family
    mask = op.observed if op.observed is not None else torch.ones_like(op.ys, dtype=torch.bool)
    zero = z.new_zeros(())
    eta = z @ op.Bm.T
    if op.offset is not None:
        eta = eta + op.offset
    if fam != _hip.GLM_GAUSSIAN and op.extra is not None:
        eta = eta + op.extra
    _, g, w, _, _ = _glm_point(fam, op.ys, eta, op.extra if fam == _hip.GLM_GAUSSIAN else None)
    wp = _glm_wprime(fam, eta, w)
    SB = torch.einsum("rak,ck->rca", Sd, op.Bm)
    v = (SB * op.Bm).sum(-1)
    return mask, torch.where(mask, g, zero), torch.where(mask, w, zero), torch.where(mask, wp, zero), v, SB


def _glm_evidence_rhs_composed(op, z, Sd):
    """cgps_leg_glm_evidence_rhs as torch passes (CGPS_LEG_GLM_COMPOSED=1): the same arithmetic in the arrays' dtype."""
    _, _, _, wp, v, _ = _glm_evidence_entries(op, z, Sd)
    return (-0.5 * (wp * v) @ op.Bm).contiguous()


def _glm_evidence_adjoint_composed(op, z, u, Sd, So, Pd, Po, gE):
    """cgps_leg_glm_evidence_adjoint as torch passes over [R, obs], [R, obs, d] and [R, d, d] arrays
    (CGPS_LEG_GLM_COMPOSED=1): the same arithmetic in the arrays' dtype, the sums per series in fp64 (``index_add_``: not
    in a fixed order).  For A/B timing, and the yardstick of the kernels' fp32 error."""
    plan, fam, dt = op.plan, op.family, z.dtype
    F64 = torch.float64
    B, R = plan.B, z.shape[0]
    obs, d = op.Bm.shape
    seg = plan.per_row(torch.arange(B, device=z.device))
    ge = gE[seg].to(dt)
    mask, g, w, wp, v, SB = _glm_evidence_entries(op, z, Sd)
    e = g - 0.5 * wp * v - w * (u @ op.Bm.T)
    if fam == _hip.GLM_GAUSSIAN:
        g_extra = torch.where(mask, 0.5 * (g * g - w + v * w * w), z.new_zeros(())) * ge[:, None]
    else:
        g_extra = e * ge[:, None]
    keep, keep_b = (ge != 0), (gE != 0)                              # a dropped series: selected, not multiplied, as the kernels do
    zero = z.new_zeros(())
    g_extra = torch.where(keep[:, None], g_extra, zero)
    outer = lambda a, b: a.unsqueeze(-1) * b.unsqueeze(-2)           # noqa: E731
    gRs = torch.where(keep[:, None, None], (0.5 * ge)[:, None, None] * (Pd - Sd - outer(z, z) - outer(u, z) - outer(z, u)), zero)
    gOs = z.new_zeros(max(R - 1, 0), d, d)
    if R > 1:
        inner = Po - So - outer(z[1:], z[:-1]) - outer(u[1:], z[:-1]) - outer(z[1:], u[:-1])
        gOs = torch.where(((plan.cut == 0) & keep[:-1])[:, None, None], ge[:-1, None, None] * inner, zero)
    rowB = e.unsqueeze(-1) * z.unsqueeze(1) + g.unsqueeze(-1) * u.unsqueeze(1) - w.unsqueeze(-1) * SB
    zero64 = gE.new_zeros(())
    gB_part = torch.zeros(B, obs, d, dtype=F64, device=z.device).index_add_(0, seg, rowB.to(F64)) * gE[:, None, None]
    goffset_part = torch.zeros(B, obs, dtype=F64, device=z.device).index_add_(0, seg, e.to(F64)) * gE[:, None]
    gB_part, goffset_part = torch.where(keep_b[:, None, None], gB_part, zero64), torch.where(keep_b[:, None], goffset_part, zero64)
    return gRs.contiguous(), gOs.contiguous(), g_extra.contiguous(), gB_part, goffset_part


def _glm_evidence_rhs(op, z, Sd):
    return _glm_evidence_rhs_composed(op, z, Sd) if _glm_composed() else _glm_evidence_rhs_hip(op, z, Sd)


def _glm_evidence_adjoint(op, z, u, Sd, So, Pd, Po, gE):
    fn = _glm_evidence_adjoint_composed if _glm_composed() else _glm_evidence_adjoint_hip
    return fn(op, z, u, Sd, So, Pd, Po, gE)


_LAPLACE_SAVED = ("z", "u", "Sd", "So", "Pd", "Po", "conv", "ts", "G")


def _laplace_saved(log_evidence):
    """What the backward of a differentiable ``log_evidence`` will read, as a dict: the operands ``op`` (_GlmOperands),
    the mode z, u = J^-1 dE/dz, the blocks of J^-1 (Sd, So) and of K^-1 (Pd, Po), ``conv``, and ts and G as the prior
    blocks were built from them.  For the tests and tools that call the two entries on their own."""
    node = log_evidence.grad_fn
    while node is not None and not hasattr(node, "op"):              # (a 0-d evidence is a select of the [1] tensor)
        node = node.next_functions[0][0] if node.next_functions else None
    return dict(zip(_LAPLACE_SAVED, node.saved_tensors), op=node.op)


class _LaplaceEvidenceFn(torch.autograd.Function):
    """log_evidence [B] as a function of (G, B, offset, extra, ts): the forward hands on the values the Newton loop
    computed, the backward is the closed-form gradient at the mode: cgps_leg_glm_evidence_adjoint, then
    cgps_peg_precision_adjoint_seg for G and ts, then the sums over the series.  ``extra`` and ``ts`` are the caller's
    tensors in the caller's layout; their gradients go back in that layout and dtype.  No second derivatives."""

    @staticmethod
    def forward(ctx, ev, G, Bm, offset, extra, ts, saved):
        ctx.op, ctx.extra_per_row = saved["op"], saved["extra_per_row"]
        ctx.save_for_backward(*(saved[k] for k in _LAPLACE_SAVED))   # freed with the graph: a second backward raises
        ctx.like = tuple(None if t is None else (tuple(t.shape), t.dtype) for t in (G, Bm, offset, extra, ts))
        return ev.clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gE):
        sv, needs, op = dict(zip(_LAPLACE_SAVED, ctx.saved_tensors)), ctx.needs_input_grad, ctx.op
        gE = torch.where(sv["conv"], gE.to(torch.float64), gE.new_zeros((), dtype=torch.float64)).contiguous()
        gRs, gOs, g_extra, gB_part, goffset_part = _glm_evidence_adjoint(op, sv["z"], sv["u"], sv["Sd"], sv["So"], sv["Pd"],
                                                                         sv["Po"], gE)
        out = [None] * 7
        if needs[1] or needs[5]:
            gG, gts = _peg_precision_adjoint_models(sv["ts"], sv["G"], op.plan.cut, gRs, gOs, needs[5])
            if needs[1]:
                out[1] = gG.to(ctx.like[0][1])
            if needs[5]:
                out[5] = gts.reshape(ctx.like[4][0]).to(ctx.like[4][1])
        if needs[2]:
            out[2] = gB_part.sum(0).to(ctx.like[1][1])
        if needs[3]:
            out[3] = goffset_part.sum(0).to(ctx.like[2][1])
        if needs[4]:
            shape, dtype = ctx.like[3]
            # (one value per row, a dimension less than ys: the cotangents of the row's entries add up)
            out[4] = (g_extra.sum(-1) if ctx.extra_per_row else g_extra).reshape(shape).to(dtype)
        return tuple(out)


def laplace_posterior_batch(m, ts, ys, lengths=None, family=None, observed=None, offset=None, log_exposure=None,
                            noise_var=None, init=None, max_iter=50, tol=None, differentiable=False,
                            allow_unconverged=False):
    """The Laplace approximation of the posterior of B independent series whose observations are counts, binary outcomes
    or Gaussian values: ``LaplacePosterior(mean, cov, log_evidence, iterations, converged)``.

    Model: z ~ the LEG prior of ``m`` (``m.Lambda`` is not used), and every observed entry (i, c) has the linear
    predictor eta_ic = B[c, :] z_i + offset[c] + log_exposure[i, c] (both optional, default 0) with
    ``family="poisson"``: log p = y eta - e^eta - lgamma(y + 1); ``"bernoulli"``: log p = y eta - softplus(eta);
    ``"gaussian"``: y ~ N(eta, noise_var[i, c]), for which the approximation is exact.

    Layouts, ``lengths`` and ``observed``: those of ``insample_posterior_batch`` (dense ts[B, n], ys[B, n, obs_dim], or
    ragged with host ``lengths``); ``log_exposure`` and ``noise_var`` in the layout of ys (or one value per row);
    ``offset`` [obs_dim]; ``init`` a starting point in the shape of the mean (default zeros).  ``mean`` is the posterior
    mode and ``cov`` = (diag, off) the blocks of the inverse of J = K + blockdiag(B^T W B) at the mode, in the shapes of
    ``insample_posterior_batch``; ``log_evidence`` [B] (fp64) = sum log p(y | eta) - z^T K z / 2 + log|K| / 2 - log|J| / 2
    at the mode; ``iterations`` [B] (int64) the Newton steps a series took part in; ``converged`` [B] (bool).  Rows that
    observe nothing take part, so target times go in through ``merge_targets``; a padded dense batch is the mask whose
    tail rows are False.  What ys, log_exposure and noise_var hold at unobserved entries is ignored, NaN included.
    Values of ys are not checked (as those of ``noise_var`` are not elsewhere).  B = 0 returns empty tensors.  Every
    ValueError is raised before anything is launched.  By default inference only: runs under ``torch.no_grad``.

    ``differentiable=True`` (the keyword of the filter calls): ``log_evidence`` carries an autograd graph to whichever of
    ``m.N, m.R, m.B, offset, log_exposure, noise_var, ts`` require grad; everything else in the result stays detached, and
    the values are those of the default call bit for bit (the loop is the same one).  The gradient is the closed form at
    the mode (the implicit function theorem, not a graph through the Newton loop): the forward also
    computes dE / dz (cgps_leg_glm_evidence_rhs), one more solve on the factor of J and the blocks of K^-1; the backward
    is cgps_leg_glm_evidence_adjoint, the adjoint of the prior blocks and the sums over the series.  Gradients come back
    in the dtype of their inputs; ``m.Lambda`` takes no part and gets none; there are no second derivatives.  The formula
    holds at the mode only: a series that has not converged raises ``CgpsError`` naming the first such series, unless
    ``allow_unconverged=True``, with which such a series keeps its value but is treated as a constant (its cotangent is
    dropped: it contributes zero to every gradient).

    How: Newton's method on the concatenated block-tridiagonal system.  cgps_peg_precision_seg writes
    the prior blocks once; every iteration is one ``cr.decompose_solve`` (the proposal J^-1 r) and one launch of
    cgps_leg_glm_step, one workgroup per series, which picks the largest of the step lengths 1, 1/2, .., 2^-11 whose
    objective is finite and not below the current one, applies it, and writes J and r at the new point.  A series has
    converged once a step's gain is <= tol (1 + |psi|) (``tol=None``: ``LAPLACE_TOL``), and is then frozen: its result does
    not depend on how long its neighbours take.  The loop reads ONE flag on the host per iteration (have all series
    finished?) and stops early when they have; a series that has not converged within ``max_iter`` steps does not raise,
    ``converged`` reports it.  Then one factorisation at the mode, ``cr.inverse_blocks``, and two
    ``cr.mahal_and_det_batch`` calls for log|J| and log|K| per series.  CGPS_LEG_GLM_COMPOSED=1 composes the step, and
    the two gradient entries, from torch passes instead (A/B timing).

    One workgroup per series makes this a call for batches: one series of 2^20 rows runs on one workgroup.  Every rank
    1..8, obs_dim <= 8, both precisions.  CPU tensors raise ``CgpsError``: there is no CPU implementation."""
    with torch.no_grad():
        like, user_offset, user_extra = ts, offset, (noise_var if noise_var is not None else log_exposure)
        if differentiable and isinstance(user_extra, torch.Tensor) and isinstance(ys, torch.Tensor):
            extra_per_row = user_extra.dim() == ys.dim() - 1        # (the caller's ys: [.., obs_dim])
        else:
            extra_per_row = False
        fam, ts, ys, lengths, observed, offset, extra, init, dense, bn, tol = _laplace_args(
            m, ts, ys, lengths, family, observed, offset, log_exposure, noise_var, init, max_iter, tol)
        d, dt = m.N.shape[0], m.N.dtype
        if not lengths:
            e = lambda *shape, dtype=dt: torch.empty(shape, dtype=dtype, device=like.device)      # noqa: E731
            n = bn[1] if dense else None
            mean, cov = ((e(0, n, d), (e(0, n, d, d), e(0, max(n - 1, 0), d, d))) if dense else
                         (e(0, d), (e(0, d, d), e(0, d, d))))
            return LaplacePosterior(mean, cov, e(0, dtype=torch.float64), e(0, dtype=torch.int64), e(0, dtype=torch.bool))
        saved = {"extra_per_row": extra_per_row} if differentiable else None
        mean, Sd, So, ev, iters, conv = _laplace_flat(m, fam, ts, ys, lengths, observed, offset, extra, init, max_iter, tol,
                                                      saved)
        if dense:
            mean, (Sd, So) = _dense_posterior(mean, Sd, So, bn[0], bn[1])
        if not differentiable:
            return LaplacePosterior(mean, (Sd, So), ev, iters, conv)
        if not allow_unconverged and not bool(conv.all()):
            b = int(torch.nonzero(~conv)[0])
            raise _hip.CgpsError("the Laplace posterior of series %d has not converged after %d steps: the gradient of the "
                                 "evidence holds at the mode only (raise max_iter, or pass allow_unconverged=True to treat "
                                 "such a series as a constant)" % (b, int(iters[b])))
    ev = _LaplaceEvidenceFn.apply(ev, m.G, m.B, user_offset, user_extra, like, saved)
    return LaplacePosterior(mean, (Sd, So), ev, iters, conv)


def laplace_posterior(m, ts, ys, family, observed=None, offset=None, log_exposure=None, noise_var=None, init=None,
                      max_iter=50, tol=None, differentiable=False, allow_unconverged=False):
    """``laplace_posterior_batch`` of one series ts[n], ys[n, obs_dim]: ``LaplacePosterior`` with mean [n, d], cov
    ([n, d, d], [n-1, d, d]) and 0-d ``log_evidence``, ``iterations`` and ``converged``.  The series runs on one
    workgroup: the call is meant for series of moderate length, many of them through the batch form.
    ``differentiable`` and ``allow_unconverged``: as there."""
    if not isinstance(ts, torch.Tensor) or not isinstance(ys, torch.Tensor) or ts.dim() != 1 or ys.dim() != 2:
        raise ValueError("one series wants ts[n] and ys[n, obs_dim]")
    if ts.shape[0] < 1:
        raise ValueError("series of length 0")
    r = laplace_posterior_batch(m, ts, ys, [ts.shape[0]], family, observed, offset, log_exposure, noise_var, init, max_iter, tol,
                                differentiable, allow_unconverged)
    return LaplacePosterior(r.mean, r.cov, r.log_evidence[0], r.iterations[0], r.converged[0])


# ---- predictions on the response scale from a latent Gaussian -----------------------------------------
GlmPredictive = collections.namedtuple("GlmPredictive", ["eta_mean", "eta_var", "mean", "var", "logpdf"])

GLM_PREDICT_NEWTON = 12
"""Clipped Newton steps from u = 0 to the centre of the quadrature rule (cgps_leg_glm_predict takes the same)."""
# the positive half of the 32 physicists' Gauss-Hermite nodes x_i, and c_i = log(w_i / sqrt(pi)) + x_i^2: the literals of
# csrc/cgps_leg_glm_predict.h
_GH_X = (0.19484074156939933, 0.58497876543593245, 0.97650046358968284, 1.3703764109528718,
         1.7676541094632016, 2.1694991836061122, 2.5772495377323175, 2.9924908250023742,
         3.4171674928185707, 3.8537554854714446, 4.3055479533511984, 4.7771645035025964,
         5.2755509865158801, 5.8122259495159138, 6.4094981492696604, 7.1258139098307276)
_GH_C = (-1.5145958763594943, -1.5122499826361202, -1.507502504881913, -1.5002376390668201,
         -1.4902698653576023, -1.4773274278750061, -1.4610256034209449, -1.4408237003057275,
         -1.4159543626976631, -1.3853025051344199, -1.3471855059889207, -1.298921160459867,
         -1.2358809264517319, -1.1490650649154518, -1.0171680130339496, -0.76526240024416115)


def _glm_predict_hip(family, zm, zc, ys, observed, offset, extra, Bm):
    """One launch of cgps_leg_glm_predict on zm [P, d], zc [P, d, d] (contiguous, of Bm's dtype): (eta_mean, eta_var, mean,
    var, logpdf or None), each [P, obs].  ``observed``: bool [P, obs] or None, packed into the pattern bytes here (or the
    pattern bytes themselves, uint8 [P])."""
    P_, d = zm.shape
    obs, dt, dev = Bm.shape[0], zm.dtype, zm.device
    pattern = None
    if observed is not None and observed.dtype == torch.uint8:
        pattern = observed
    elif observed is not None and ys is not None:
        pattern = (observed * (1 << torch.arange(obs, device=dev))).sum(1).to(torch.uint8).contiguous()
    outs = [torch.empty(P_, obs, dtype=dt, device=dev) for _ in range(5 if ys is not None else 4)]
    if ys is None:
        outs.append(None)
    P = _hip.ptr
    _hip.check(_hip.lib().cgps_leg_glm_predict(
        P(zm), P(cr._aligned16(zc)), P(ys), P(pattern), P(offset), P(extra), P(Bm), P_, d, obs, _hip.dtype_code(dt), family,
        *[P(t) for t in outs], _hip.stream_ptr()))
    return tuple(outs)


def _glm_predict_l(family, y, eta):
    """l(y, eta) without lgamma(y + 1): the arithmetic of ``glm_predict_l`` (csrc/cgps_leg_glm_predict.h)"""
    if family == _hip.GLM_POISSON:
        return y * eta - torch.exp(eta)
    return (y - (eta > 0).to(eta.dtype)) * eta - torch.log1p(torch.exp(-eta.abs()))


def _glm_predict_point(family, y, eta):
    """(l, g, w) at eta: the arithmetic of ``glm_predict_point``"""
    if family == _hip.GLM_POISSON:
        e = torch.exp(eta)
        return y * eta - e, y - e, e
    e = torch.exp(-eta.abs())
    r = 1.0 / (1.0 + e)
    m = e * r
    up = (eta > 0).to(eta.dtype)
    return (y - up) * eta - torch.log1p(e), (y - up) + torch.where(eta > 0, m, -m), m * r


def _glm_log_integral(family, y, mu, v):
    """log of the integral of exp(l(y, eta)) N(eta; mu, v) by the rule of ``glm_log_integral``, as fp64 torch passes over
    arrays of the entries' shape and, for the nodes, that shape x 16 (Poisson without its -lgamma(y + 1))"""
    sv = v.sqrt()
    cap = 1.0 / sv
    u = torch.zeros_like(mu)
    for _ in range(GLM_PREDICT_NEWTON):
        _, g, w = _glm_predict_point(family, y, mu + sv * u)
        step = (sv * g - u) / (1.0 + v * w)
        u = u + torch.where(step > cap, cap, step)
    l, _, w = _glm_predict_point(family, y, mu + sv * u)
    s = 1.0 / (1.0 + v * w).sqrt()
    x = torch.tensor(_GH_X, dtype=mu.dtype, device=mu.device)
    c = torch.tensor(_GH_C, dtype=mu.dtype, device=mu.device)
    e = lambda t: t.unsqueeze(-1)                                    # noqa: E731
    dl = math.sqrt(2.0) * e(s) * x
    lp = _glm_predict_l(family, e(y), e(mu) + e(sv) * (e(u) + dl))
    lm = _glm_predict_l(family, e(y), e(mu) + e(sv) * (e(u) - dl))
    total = (torch.exp(c + (lp - e(l)) - dl * (e(u) + 0.5 * dl)) + torch.exp(c + (lm - e(l)) + dl * (e(u) - 0.5 * dl))).sum(-1)
    return torch.log(s) + (l - 0.5 * u * u) + torch.log(total)


def _glm_predict_composed(family, zm, zc, ys, observed, offset, extra, Bm):
    """cgps_leg_glm_predict as torch passes (CGPS_LEG_GLM_COMPOSED=1): mu and v in the arrays' dtype, the moments and the
    rule in fp64, as the kernel takes them.  For A/B timing, the yardstick of the kernel's fp32 error, and -- it accepts
    CPU tensors -- the test of the rule without a GPU."""
    F64, dt = torch.float64, zm.dtype
    mu = zm @ Bm.T
    if offset is not None:
        mu = mu + offset
    if family != _hip.GLM_GAUSSIAN and extra is not None:
        mu = mu + extra
    vT = (torch.einsum("pab,cb->pca", zc, Bm) * Bm).sum(-1)
    vT = torch.where(vT < 0, torch.zeros_like(vT), vT)
    mu64, v = mu.to(F64), vT.to(F64)
    given = None
    if ys is not None:
        given = torch.ones_like(mu, dtype=torch.bool) if observed is None else observed
        y = torch.where(given, ys.to(F64), torch.zeros_like(mu64))
    lp = None
    if family == _hip.GLM_GAUSSIAN:
        tot = v + extra.to(F64)
        mean, var = mu64, tot
        if ys is not None:
            res = y - mu64
            lp = -0.5 * res * res / tot - 0.5 * torch.log(2 * math.pi * tot)
    elif family == _hip.GLM_POISSON:
        mean = torch.exp(mu64 + 0.5 * v)
        var = mean + mean * mean * torch.expm1(v)
        if ys is not None:
            lp = _glm_log_integral(family, y, mu64, v) - torch.lgamma(y + 1.0)
    else:
        L1 = _glm_log_integral(family, torch.ones_like(mu64), mu64, v)
        L0 = _glm_log_integral(family, torch.zeros_like(mu64), mu64, v)
        mean, var = torch.exp(L1), torch.exp(L1 + L0)
        if ys is not None:
            lp = torch.where(y == 1, L1, L0)
            other = (y != 1) & (y != 0)                              # (values of ys are not checked: the rule at y itself)
            if bool(other.any()):
                lp = torch.where(other, _glm_log_integral(family, y, mu64, v), lp)
    if lp is not None:
        lp = torch.where(given, lp, torch.zeros_like(lp)).to(dt)
    return mu.contiguous(), vT.contiguous(), mean.to(dt), var.to(dt), lp


def _glm_predict(family, zm, zc, ys, observed, offset, extra, Bm):
    fn = _glm_predict_composed if _glm_composed() else _glm_predict_hip
    return fn(family, zm, zc, ys, observed, offset, extra, Bm)


def _glm_predict_family(family, log_exposure, noise_var, what=""):
    """the family's code; raises the ValueErrors about which of log_exposure / noise_var belongs to which family
    (``what``: the prefix of the argument names in the caller's signature)"""
    if family not in _FAMILIES:
        raise ValueError("family must be one of %s, got %r" % (sorted(_FAMILIES), family))
    fam = _FAMILIES[family]
    if fam == _hip.GLM_GAUSSIAN and noise_var is None:
        raise ValueError("family 'gaussian' needs %snoise_var, the variance of every predicted entry" % what)
    if fam != _hip.GLM_GAUSSIAN and noise_var is not None:
        raise ValueError("%snoise_var belongs to family 'gaussian', got family %r" % (what, family))
    if fam == _hip.GLM_GAUSSIAN and log_exposure is not None:
        raise ValueError("%slog_exposure belongs to the families 'poisson' and 'bernoulli'" % what)
    return fam


def glm_predictive(m, z_mean, z_cov, family, offset=None, log_exposure=None, noise_var=None, ys=None, observed=None):
    """What a latent Gaussian says about an observation of the families of ``laplace_posterior_batch``:
    ``GlmPredictive(eta_mean, eta_var, mean, var, logpdf)``, each [..., obs_dim].

    ``z_mean`` [..., d] and ``z_cov`` [..., d, d] of any leading shape: the latent at target times
    (``predict.laplace_predictions_batch`` does that in one call), or ``LaplacePosterior.mean`` and ``cov[0]`` for
    in-sample posterior predictive checks.  Per entry the linear predictor eta = B[c, :] z + offset[c] + log_exposure is
    N(eta_mean, eta_var); ``mean`` and ``var`` are the moments of y on the response scale (a Poisson rate, a Bernoulli
    probability; Gaussian: eta_mean and eta_var + noise_var), and ``logpdf`` = log of the integral of p(ys | eta) over that
    Gaussian -- the log predictive density of held-out data -- or None without ``ys``.  ``observed`` (bool, like ys): the
    entries of ys that exist; elsewhere logpdf is exact zero and ys is ignored, NaN included.  ``log_exposure`` /
    ``noise_var`` ([..., obs_dim]) are used at EVERY entry.  ``offset`` [obs_dim].

    Gaussian in closed form; Poisson mean and variance in closed form; the Poisson logpdf and everything Bernoulli by
    adaptive Gauss-Hermite quadrature with 32 nodes in fp64 (cgps_leg_glm_predict, a lane per entry; DESIGN.md 4.28 for
    its accuracy: within the fp64 test bound up to eta_var = 2, about 2e-5 relative at eta_var = 4).  Inference only, GPU
    tensors only; CGPS_LEG_GLM_COMPOSED=1 composes it from torch passes instead.  Every ValueError is raised before
    anything is launched."""
    fam = _glm_predict_family(family, log_exposure, noise_var)
    obs, d = m.B.shape
    dt = m.B.dtype
    if not 1 <= d <= 8 or obs > MAX_PATTERN_OBS or dt not in (torch.float32, torch.float64):
        raise ValueError("glm_predictive is built for rank 1..8, obs_dim <= %d, float32 / float64" % MAX_PATTERN_OBS)
    if not isinstance(z_mean, torch.Tensor) or not isinstance(z_cov, torch.Tensor) or not z_mean.dtype.is_floating_point:
        raise ValueError("z_mean and z_cov must be floating-point tensors")
    lead = tuple(z_mean.shape[:-1])
    if z_mean.dim() < 1 or z_mean.shape[-1] != d or tuple(z_cov.shape) != lead + (d, d):
        raise ValueError("z_mean must be [..., %d] and z_cov [..., %d, %d], got %s and %s"
                         % (d, d, d, tuple(z_mean.shape), tuple(z_cov.shape)))
    extra = noise_var if fam == _hip.GLM_GAUSSIAN else log_exposure
    if observed is not None and ys is None:
        raise ValueError("observed says which entries of ys exist: it needs ys")
    for name, t, ok in (("ys", ys, lambda q: q.is_floating_point), ("observed", observed, lambda q: q == torch.bool),
                        ("noise_var" if fam == _hip.GLM_GAUSSIAN else "log_exposure", extra, lambda q: q.is_floating_point)):
        if t is not None and (not isinstance(t, torch.Tensor) or not ok(t.dtype) or tuple(t.shape) != lead + (obs,)):
            raise ValueError("%s must be a %s tensor %s" % (name, "bool" if name == "observed" else "floating-point", lead + (obs,)))
    if offset is not None and (not isinstance(offset, torch.Tensor) or not offset.dtype.is_floating_point or
                               tuple(offset.shape) != (obs,)):
        raise ValueError("offset must be a floating-point tensor [%d]" % obs)
    tensors = [t for t in (m.B, z_mean, z_cov, ys, observed, offset, extra) if t is not None]
    if not _glm_composed() and not all(t.is_cuda for t in tensors):
        raise _hip.CgpsError("glm_predictive runs on GPU tensors only (there is no CPU implementation)")
    with torch.no_grad():
        c = lambda t, shape: None if t is None else t.to(dt).reshape(shape).contiguous()      # noqa: E731
        out = _glm_predict(fam, c(z_mean, (-1, d)), c(z_cov, (-1, d, d)), c(ys, (-1, obs)),
                           None if observed is None else observed.reshape(-1, obs), c(offset, (obs,)), c(extra, (-1, obs)),
                           c(m.B, (obs, d)))
        return GlmPredictive(*[None if t is None else t.reshape(lead + (obs,)) for t in out])


# ---- the config-5 workload -----------------------------------------------------------------
def co2_like_series(rows=770, seed=0, dtype=torch.float64):
    """Mauna-Loa-shaped monthly series (decimal date, ppm): quadratic trend + annual and
    semi-annual cycles + small noise.  Stand-in for ../data/co2_mm_mlo.csv, which is not part of
    the reference repo (co2_data_experiments.py:17)."""
    g = torch.Generator().manual_seed(seed)
    t = 1958.2 + torch.arange(rows, dtype=dtype) / 12.0
    u = t - 1958.0
    x = 315.0 + 0.8 * u + 0.012 * u * u + 2.9 * torch.sin(2 * math.pi * t) + 0.8 * torch.sin(4 * math.pi * t + 0.6)
    x = x + 0.3 * torch.randn(rows, dtype=dtype, generator=g)
    return t, x.unsqueeze(-1)


def load_co2_csv(path, dtype=torch.float64):
    """The real file, when a user has it: columns as in co2_data_experiments.py:17-19."""
    import numpy as np
    rows = []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith("#") or line[0].isalpha():
                continue
            rows.append([float(tok) for tok in line.replace(",", " ").split()])
    a = np.array(rows)
    return torch.tensor(a[:, 2], dtype=dtype), torch.tensor(a[:, 3], dtype=dtype).unsqueeze(-1)


def co2_workload(path=None, dtype=torch.float64):
    """(all_ts, all_xs, train_ts, train_xs) standardised and masked as the reference does
    (co2_data_experiments.py:21-30, dataset_process_utils.py:9-25)."""
    if path is not None and os.path.exists(path):
        t, x = load_co2_csv(path, dtype)
    else:
        t, x = co2_like_series(dtype=dtype)
    ts = 12 * (t - t.min())
    xs = x - x.mean()
    xs = xs / xs.std()
    train_ts = torch.cat([ts[:262], ts[502:-28]])
    train_xs = torch.cat([xs[:262], xs[502:-28]])
    return ts, xs, train_ts, train_xs

"""Prediction glue of the LEG model, batched over the target times (the step right AFTER the
cyclic-reduction path).

The reference walks the targets in a Python loop (models.py:467-514): per target one
``searchsorted`` hit, one or two matrix exponentials through an eigendecomposition of G
(model_utils.py:12-29) and one ``gaussian_stitch`` (model_utils.py:64-107) of a 2d x 2d or 3d x 3d
Gaussian.  Here the same arithmetic runs for ALL targets at once as batched tensor ops on the
device the in-sample posterior lives on (``searchsorted`` once, one batched ``matrix_exp``, one
batched d x d / 2d x 2d solve per branch): nothing comes back to the host inside
``make_predictions``.

Same names and argument meaning as the reference (methods of ``LEGFamily`` there, functions of a
``LEGMatrices`` here):

    gaussian_stitch(joint_mean, joint_cov, marginal_mean, marginal_cov)      model_utils.py:64-107
    build_2x2_block, build_3x3_block                                          model_utils.py:31-60
    forecast(eG, ip_mean, ip_cov)                                             models.py:394-408
    interpolate(eG1, eG2, prev_ip_mean, ..., next_ip_cov_diag)                models.py:410-452
    intercast(m, ip_mean, ip_cov, ts, target_ts)                              models.py:455-514
    predictive_posterior(m, ts, xs, target_ts)                                models.py:516-528
    make_predictions(m, ts, xs, target_ts)                                    models.py:530-546

The in-sample posterior itself (``decompose`` / ``solve`` / ``inverse_blocks``) is the HIP path
(``leg.insample_posterior``).  Pinned by ``tests/golden/leg_*.npz`` (``pp_mean``, ``pp_cov``,
``pred_mean``, ``pred_cov`` recorded from the reference's own ``make_predictions``).
"""
import collections
import os

import torch

from . import leg


def build_2x2_block(a, b, c, d):
    """[[a, b], [c, d]], batched over leading dimensions   (reference model_utils.py:31-50)."""
    return torch.cat([torch.cat([a, b], dim=-1), torch.cat([c, d], dim=-1)], dim=-2)


def build_3x3_block(a, b, c, d, e, f, g, h, i):
    """3 x 3 block matrix, batched   (reference model_utils.py:52-60)."""
    return torch.cat([torch.cat([a, b, c], dim=-1), torch.cat([d, e, f], dim=-1), torch.cat([g, h, i], dim=-1)], dim=-2)


def gaussian_stitch(joint_mean, joint_cov, marginal_mean, marginal_cov):
    """E and Cov of y under q(x, y) = p2(x) p1(y | x), p1 = N(joint_mean, joint_cov) over (x, y),
    p2 = N(marginal_mean, marginal_cov) over x   (reference model_utils.py:64-107).  Batched over
    leading dimensions (the reference transposes with ``.T``, i.e. is un-batched)."""
    m = marginal_cov.shape[-1]
    Axx, Ayx = joint_cov[..., :m, :m], joint_cov[..., m:, :m]
    # mean_transformer = C_yx C_xx^-1
    # (solve_ex: no error check, hence no device->host synchronisation; Axx = [[I, E^T], [E, I]] with
    # E a contraction, or I: never singular)
    Mt = torch.linalg.solve_ex(Axx.transpose(-1, -2), Ayx.transpose(-1, -2))[0].transpose(-1, -2)
    mean = joint_mean[..., m:] + (Mt @ marginal_mean[..., None])[..., 0]
    cond = joint_cov[..., m:, m:] - Mt @ joint_cov[..., :m, m:]
    return mean, cond + Mt @ marginal_cov @ Mt.transpose(-1, -2)


def compute_eG(G, diffs):
    """exp(-1/2 d G) for every d in diffs [m] -> [m, rank, rank].  (The reference goes through a
    complex eigendecomposition of G, model_utils.py:12-29; the matrix exponential itself is the
    same quantity without the detour through complex arithmetic.)"""
    return torch.matrix_exp(-0.5 * diffs.reshape(-1, 1, 1) * G.unsqueeze(0))


def forecast(eG, ip_mean, ip_cov):
    """One step away from an in-sample point: latent at the target given the in-sample posterior
    N(ip_mean, ip_cov) of its neighbour   (reference models.py:394-408).  Batched."""
    rank = eG.shape[-1]
    I = torch.eye(rank, dtype=eG.dtype, device=eG.device).expand(eG.shape)
    joint_mean = torch.zeros(eG.shape[:-2] + (2 * rank,), dtype=eG.dtype, device=eG.device)
    joint_cov = build_2x2_block(I, eG.transpose(-1, -2), eG, I)
    return gaussian_stitch(joint_mean, joint_cov, ip_mean, ip_cov)


def interpolate(eG1, eG2, prev_ip_mean, prev_ip_cov_diag, prev_ip_cov_offdiag, next_ip_mean, next_ip_cov_diag):
    """Latent at a target between two in-sample points   (reference models.py:410-452): eG1 spans
    previous -> target, eG2 target -> next.  Batched."""
    rank = eG1.shape[-1]
    I = torch.eye(rank, dtype=eG1.dtype, device=eG1.device).expand(eG1.shape)
    T = lambda a: a.transpose(-1, -2)  # noqa: E731
    eG3 = eG1 @ eG2
    joint_latent_mean = torch.zeros(eG1.shape[:-2] + (3 * rank,), dtype=eG1.dtype, device=eG1.device)
    joint_latent_cov = build_3x3_block(I, T(eG3), T(eG1),
                                       eG3, I, eG2,
                                       eG1, T(eG2), I)
    joint_ip_mean = torch.cat([prev_ip_mean, next_ip_mean], dim=-1)
    joint_ip_cov = build_2x2_block(prev_ip_cov_diag, T(prev_ip_cov_offdiag), prev_ip_cov_offdiag, next_ip_cov_diag)
    return gaussian_stitch(joint_latent_mean, joint_latent_cov, joint_ip_mean, joint_ip_cov)


def _intercast_hip(G, ip_mean, Rs, Os, ts, target_ts):
    """All targets in one HIP kernel (cgps_leg_intercast, csrc/cgps_leg.h): one lane per target, the two
    matrix exponentials and the stitch in registers.  No autograd graph (prediction is inference)."""
    from . import _hip
    dt, dev = ip_mean.dtype, ip_mean.device
    n, d, p = ip_mean.shape[0], G.shape[0], target_ts.shape[0]
    c = lambda t: leg.cr._aligned16(t.detach().to(device=dev, dtype=dt).contiguous())   # noqa: E731
    ts_, tt_, G_, mu_, Rs_, Os_ = c(ts), c(target_ts), c(G), c(ip_mean), c(Rs), c(Os)
    means = torch.empty(p, d, dtype=dt, device=dev)
    covs = torch.empty(p, d, d, dtype=dt, device=dev)
    _hip.check(_hip.lib().cgps_leg_intercast(_hip.ptr(ts_), n, _hip.ptr(tt_), p, _hip.ptr(G_), d, _hip.dtype_code(dt),
                                             _hip.ptr(mu_), _hip.ptr(Rs_), _hip.ptr(Os_), _hip.ptr(means),
                                             _hip.ptr(covs), _hip.stream_ptr()))
    return means, covs


def intercast(m, ip_mean, ip_cov, ts, target_ts, thresh=1e-10, check_sorted=True):
    """Posterior of the latent at every target time from the in-sample posterior
    (reference models.py:455-514; ``thresh`` is accepted and unused there as well).

    ip_mean [n, rank]; ip_cov = {"Rs": [n, rank, rank], "Os": [n-1, rank, rank]} (or a pair);
    ts [n] sorted; target_ts [p] strictly increasing (asserted like the reference does, :471 -- the
    one device->host read in here; check_sorted=False skips it).  Returns (means [p, rank],
    covs [p, rank, rank]).  Branches per target, as the reference takes them: before the first
    observation (backward forecast), after the last (forward forecast), at the first / last
    observation (in-sample values), otherwise interpolation between the two neighbours.
    On the GPU: one HIP kernel, a lane per target (``_intercast_hip``).  On CPU tensors (or with a
    gradient wanted, or CGPS_LEG_TORCH_INTERCAST=1) batched torch ops: every branch is evaluated for
    every target with clamped (harmless) arguments and the results are selected with masks, so no
    branch decision leaves the device."""
    Rs, Os = (ip_cov["Rs"], ip_cov["Os"]) if isinstance(ip_cov, dict) else ip_cov
    G = m.G
    n, rank = ts.shape[0], G.shape[0]
    target_ts = target_ts.to(ts.dtype)
    if check_sorted:
        assert bool((target_ts[1:] - target_ts[:-1] > 0).all())      # reference :471
    p = target_ts.shape[0]
    if (ip_mean.is_cuda and 1 <= rank <= 8 and ip_mean.dtype in (torch.float32, torch.float64)
            and os.environ.get("CGPS_LEG_TORCH_INTERCAST") != "1"
            and not (torch.is_grad_enabled() and any(t.requires_grad for t in (ip_mean, Rs, Os, G, ts, target_ts)))):
        return _intercast_hip(G, ip_mean, Rs, Os, ts, target_ts)
    idx = torch.searchsorted(ts, target_ts)
    close = lambda a, b: (a - b).abs() <= 1e-8 + 1e-5 * b.abs()      # noqa: E731  torch.allclose(a, b) defaults
    at_first = (idx == 0) & close(target_ts, ts[0])
    at_last = (idx > 0) & close(target_ts, ts[-1])
    back = (idx == 0) & ~at_first
    fwd = (idx == n) & ~at_last
    zero = torch.zeros((), dtype=ts.dtype, device=ts.device)
    ex = lambda v, shape: v.expand(shape)                            # noqa: E731
    # forecasts from the first / last observation
    mb, cb = forecast(compute_eG(G, torch.maximum(ts[0] - target_ts, zero)).transpose(-1, -2),
                      ex(ip_mean[0], (p, rank)), ex(Rs[0], (p, rank, rank)))
    mf, cf = forecast(compute_eG(G, torch.maximum(target_ts - ts[-1], zero)),
                      ex(ip_mean[-1], (p, rank)), ex(Rs[-1], (p, rank, rank)))
    means = torch.where(back[:, None], mb, mf)
    covs = torch.where(back[:, None, None], cb, cf)
    if n > 1:                                                         # interpolation between neighbours
        j = idx.clamp(1, n - 1)
        mi, ci = interpolate(
            eG1=compute_eG(G, torch.maximum(target_ts - ts[j - 1], zero)),
            eG2=compute_eG(G, torch.maximum(ts[j] - target_ts, zero)),
            prev_ip_mean=ip_mean[j - 1], prev_ip_cov_diag=Rs[j - 1], prev_ip_cov_offdiag=Os[j - 1],
            next_ip_mean=ip_mean[j], next_ip_cov_diag=Rs[j])
        mid = ~(back | fwd)
        means = torch.where(mid[:, None], mi, means)
        covs = torch.where(mid[:, None, None], ci, covs)
    means = torch.where(at_first[:, None], ip_mean[0], torch.where(at_last[:, None], ip_mean[-1], means))
    covs = torch.where(at_first[:, None, None], Rs[0], torch.where(at_last[:, None, None], Rs[-1], covs))
    return means, covs


def predictive_posterior(m, ts, xs, target_ts, check_sorted=True):
    """E[z(t) | x] and Cov[z(t) | x] at every target   (reference models.py:516-528).  The in-sample
    posterior is decompose + solve + inverse_blocks on the HIP path."""
    mean, (cRs, cOs) = leg.insample_posterior(m, ts, xs)
    return intercast(m, mean, {"Rs": cRs, "Os": cOs}, ts, target_ts, check_sorted=check_sorted)


def make_predictions(m, ts, xs, target_ts, check_sorted=True):
    """Predicted observation mean [p, obs_dim] and covariance [p, obs_dim, obs_dim] at the targets
    (reference models.py:530-546: the latent's B-image; the observation noise is not added there).
    check_sorted=False skips the reference's assertion on the targets (:471), the one device->host read:
    the call is then capturable in a HIP graph (``leg.Graphed``)."""
    pm, pv = predictive_posterior(m, ts, xs, target_ts, check_sorted=check_sorted)
    return pm @ m.B.T, m.B.unsqueeze(0) @ pv @ m.B.T.unsqueeze(0)


# ---- many series at once ---------------------------------------------------------------------------------------
class _TargetPlan:
    """What the target lengths fix on the host: device offsets of every series' targets, and the mask of the pairs of
    neighbouring targets that belong to different series (the sortedness check skips them).  A series may have no
    target."""

    plans = {}          # (lengths, device) -> plan, least recently used first (leg._cached_batch_plan)
    captured = {}       # plans that a stream capture has read: never dropped

    def __init__(self, lengths, device):
        self.lengths = lengths
        self.B, self.P = len(lengths), sum(lengths)
        off = [0]
        for p in lengths:
            off.append(off[-1] + p)
        self.starts = off
        self.offsets = torch.tensor(off, dtype=torch.int64).to(device, non_blocking=True)
        across = torch.zeros(max(self.P - 1, 0), dtype=torch.bool)
        inner = [o - 1 for o in off[1:-1] if 0 < o < self.P]
        if inner:
            across[torch.tensor(inner)] = True
        self.across = across.to(device, non_blocking=True)


def _batch_targets(target_ts, target_lengths, lengths, dense):
    """(target_ts [P], target lengths as a list of ints, shape of the dense targets (B, p) or None); raises ValueError
    before anything is launched."""
    B = len(lengths)
    if not isinstance(target_ts, torch.Tensor) or not target_ts.dtype.is_floating_point:
        raise ValueError("target_ts must be a floating-point tensor")
    if dense:
        if target_lengths is not None:
            raise ValueError("target_lengths belongs to the ragged layout (give lengths as well)")
        if target_ts.dim() == 1:
            target_ts = target_ts.unsqueeze(0).expand(B, -1)
        if target_ts.dim() != 2 or target_ts.shape[0] != B:
            raise ValueError("dense layout wants target_ts[B, p] or target_ts[p] shared by all %d series, got %s"
                             % (B, tuple(target_ts.shape)))
        p = int(target_ts.shape[1])
        return target_ts.reshape(B * p), [p] * B, (B, p)
    if target_lengths is None:
        raise ValueError("ragged layout wants target_lengths: how many of target_ts belong to each series")
    if isinstance(target_lengths, torch.Tensor):
        if (target_lengths.is_cuda or target_lengths.dim() != 1 or target_lengths.dtype.is_floating_point
                or target_lengths.dtype == torch.bool):
            raise ValueError("target_lengths must be host data: a list or a 1-d CPU integer tensor")
        target_lengths = target_lengths.tolist()
    target_lengths = [int(p) for p in target_lengths]
    if target_ts.dim() != 1:
        raise ValueError("ragged layout wants target_ts[sum(target_lengths)], got %s" % (tuple(target_ts.shape),))
    if len(target_lengths) != B:
        raise ValueError("target_lengths names %d series, lengths %d" % (len(target_lengths), B))
    bad = [b for b, p in enumerate(target_lengths) if p < 0]
    if bad:
        raise ValueError("series %d has %d targets" % (bad[0], target_lengths[bad[0]]))
    if sum(target_lengths) != target_ts.shape[0]:
        raise ValueError("target_lengths sum to %d targets, target_ts has %d" % (sum(target_lengths), target_ts.shape[0]))
    return target_ts, target_lengths, None


def _intercast_models_hip(G, ip_mean, Rs, Os, ts, plan, target_ts, tplan, means=None, covs=None):
    """All targets of all series in one HIP kernel (cgps_leg_intercast_seg, csrc/cgps_leg.h): a lane per target finds
    its series and does what ``_intercast_hip`` does for that series alone.  With G [m, d, d] the same under every model
    (cgps_leg_intercast_models): grid (target blocks, m), model k on its slices of the concatenated posterior ip_mean
    [m R, d], Rs [m R, d, d], Os [m R - 1, d, d], its predictions in means[k] [m, P, d] and covs[k] [m, P, d, d].  ``means``
    and ``covs``: contiguous tensors to write into (None: new ones)."""
    from . import _hip
    dt, dev = ip_mean.dtype, ip_mean.device
    d, P, lead = G.shape[-1], tplan.P, tuple(G.shape[:-2])
    c = lambda t: leg.cr._aligned16(t.detach().to(device=dev, dtype=dt).contiguous())   # noqa: E731
    ts_, tt_, G_, mu_, Rs_, Os_ = c(ts), c(target_ts), c(G), c(ip_mean), c(Rs), c(Os)
    if means is None:
        means = torch.empty(lead + (P, d), dtype=dt, device=dev)
        covs = torch.empty(lead + (P, d, d), dtype=dt, device=dev)
    fn = _hip.lib().cgps_leg_intercast_models if lead else _hip.lib().cgps_leg_intercast_seg
    _hip.check(fn(_hip.ptr(ts_), _hip.ptr(plan.offsets), _hip.ptr(tt_), _hip.ptr(tplan.offsets), plan.B, P, *lead, _hip.ptr(G_), d,
                  _hip.dtype_code(dt), _hip.ptr(mu_), _hip.ptr(Rs_), _hip.ptr(Os_), _hip.ptr(means), _hip.ptr(covs),
                  _hip.stream_ptr()))
    return means, covs


_intercast_seg_hip = _intercast_models_hip        # the same function: the name of its form without a model axis


def _intercast_per_series(m, mean, Sd, So, ts, lengths, target_ts, target_lengths):
    """``intercast`` series by series (inputs outside the kernels' cover)."""
    means, covs, s, k = [], [], 0, 0
    for n, p in zip(lengths, target_lengths):
        pm, pv = intercast(m, mean[s:s + n], (Sd[s:s + n], So[s:s + n - 1]), ts[s:s + n], target_ts[k:k + p],
                           check_sorted=False)
        means.append(pm)
        covs.append(pv)
        s, k = s + n, k + p
    return torch.cat(means), torch.cat(covs)


def predictive_posterior_batch(m, ts, xs, target_ts, lengths=None, target_lengths=None, observed=None, noise_var=None,
                               check_sorted=True):
    """``predictive_posterior`` of B independent series in one call: E[z(t) | x_b] and Cov[z(t) | x_b] at every target
    of every series.  Inference only: runs under ``torch.no_grad``, the results carry no autograd graph.

    Dense layout (``lengths=None``): ts[B, n], xs[B, n, obs_dim], target_ts[B, p] or [p] shared by all series; returns
    (means [B, p, rank], covs [B, p, rank, rank]).  Ragged: ts[R], xs[R, obs_dim], host ``lengths``, target_ts[P] and
    host ``target_lengths`` (how many targets each series has; zero is allowed); returns ([P, rank], [P, rank, rank])
    in the order of target_ts.  ``observed`` and ``noise_var`` as in ``leg.insample_posterior_batch``; a series' end is
    its own last row, observed or not, so a padded dense batch (tail rows False) predicts exactly as a per-series call
    with the same mask would.

    How: ``leg.insample_posterior_batch``'s one factorisation of the concatenated system, then ONE launch of
    cgps_leg_intercast_seg -- a lane per target finds its series and interpolates or forecasts inside that series
    alone; it never reads across a series boundary.  ``check_sorted=True`` asserts every series' targets strictly
    increasing (as the reference does, models.py:471) with one device->host read for the whole batch; ``False`` reads
    nothing, and after one ordinary call with the same lengths the call can be captured (``leg.Graphed``).  A repeated
    call with the same lengths and target lengths copies nothing from the host.  Errors, NaN propagation with
    ``cr.CHECK_POSITIVE_DEFINITE`` off and unsupported inputs: ``leg.insample_posterior_batch``."""
    with torch.no_grad():
        ts_f, xs_f, lens, observed, noise_var, dense, bn = leg._batch_args(m.B.shape[0], ts, xs, lengths, observed, noise_var)
        tt, tlens, bp = _batch_targets(target_ts, target_lengths, lens, dense)
        d, dt = m.N.shape[0], m.N.dtype
        P = sum(tlens)
        if not lens or P == 0:
            shape = bp if dense else (0,)
            return (torch.empty(shape + (d,), dtype=dt, device=ts_f.device),
                    torch.empty(shape + (d, d), dtype=dt, device=ts_f.device))
        tt = tt.to(ts_f.dtype)
        G = m.G
        if leg._posterior_batch_supported(ts_f, G):
            tplan = leg._cached_batch_plan(tlens, G.device, make=_TargetPlan)
            if check_sorted and P > 1:
                assert bool(((tt[1:] - tt[:-1] > 0) | tplan.across).all())     # reference :471, per series
            mean, Sd, So, plan = leg._posterior_flat_hip(m, ts_f, xs_f, lens, observed, noise_var)
            pm, pv = _intercast_models_hip(G, mean, Sd, So, ts_f, plan, tt, tplan)
        else:
            if check_sorted and P > 1:
                across = _TargetPlan(tlens, tt.device).across
                assert bool(((tt[1:] - tt[:-1] > 0) | across).all())
            mean, Sd, So = leg._insample_posterior_per_series(m, ts_f, xs_f, lens, observed, noise_var)
            pm, pv = _intercast_per_series(m, mean, Sd, So, ts_f, lens, tt, tlens)
        if dense:
            return pm.reshape(bp + (d,)), pv.reshape(bp + (d, d))
        return pm, pv


def make_predictions_batch(m, ts, xs, target_ts, lengths=None, target_lengths=None, observed=None, noise_var=None,
                           check_sorted=True):
    """``make_predictions`` of B independent series in one call: predicted observation mean [..., obs_dim] and covariance
    [..., obs_dim, obs_dim] at every target of every series -- the B-image of the latent posterior, without observation
    noise, as ``make_predictions`` gives it.  Arguments, layouts ([B, p, ...] dense, [P, ...] ragged), inference-only
    results and errors: ``predictive_posterior_batch``."""
    with torch.no_grad():
        pm, pv = predictive_posterior_batch(m, ts, xs, target_ts, lengths, target_lengths, observed, noise_var, check_sorted)
        return pm @ m.B.T, m.B @ pv @ m.B.T


# ---- counts and binary outcomes: predictions from the Laplace posterior -------------------------------
GlmPredictions = collections.namedtuple("GlmPredictions", ["z_mean", "z_cov", "eta_mean", "eta_var", "mean", "var", "logpdf",
                                                           "converged"])
_TARGET_SPECS = {
    "target_ys": ("target_ys", "a floating-point tensor", lambda dtype: dtype.is_floating_point),
    "target_observed": ("target_observed", "a bool tensor", lambda dtype: dtype == torch.bool),
    "target_log_exposure": ("target_log_exposure", "a floating-point tensor", lambda dtype: dtype.is_floating_point),
    "target_noise_var": ("target_noise_var", "a floating-point tensor", lambda dtype: dtype.is_floating_point),
}


def _flat_posterior(posterior, dense, bn, R, d):
    """(mean [R, d], Sd [R, d, d], So [R - 1, d, d], converged [B]) of a ``LaplacePosterior`` in the layout of the call
    (the blocks of So between two series of a dense batch are zeros: nothing reads them); ValueError when its shapes are
    not those of the data."""
    try:
        mean, (Sd, So), conv = posterior.mean, posterior.cov, posterior.converged
    except (AttributeError, TypeError, ValueError):
        raise ValueError("posterior must be a LaplacePosterior, what leg.laplace_posterior_batch returns for the same data")
    B = bn[0] if dense else None
    want = ((B, bn[1], d), (B, bn[1], d, d), (B, bn[1] - 1, d, d)) if dense else ((R, d), (R, d, d), (max(R - 1, 0), d, d))
    got = tuple(tuple(t.shape) if isinstance(t, torch.Tensor) else None for t in (mean, Sd, So))
    if got != want:
        raise ValueError("posterior is not of this data: mean and cov of shapes %s, the data wants %s" % (got, want))
    if dense:
        So = torch.cat([So, So.new_zeros(B, 1, d, d)], 1).reshape(R, d, d)[:R - 1]
    return mean.reshape(R, d), Sd.reshape(R, d, d), So, conv


def laplace_predictions_batch(m, ts, ys, target_ts, lengths=None, target_lengths=None, family=None, observed=None,
                              offset=None, log_exposure=None, noise_var=None, target_log_exposure=None,
                              target_noise_var=None, target_ys=None, target_observed=None, posterior=None, init=None,
                              max_iter=50, tol=None, check_sorted=True):
    """Predictions at new times for B independent series of counts, binary outcomes or Gaussian values, from the Laplace
    posterior of ``leg.laplace_posterior_batch``: ``GlmPredictions(z_mean, z_cov, eta_mean, eta_var, mean, var, logpdf,
    converged)``.  Inference only, GPU tensors only.

    The data arguments (ts, ys, lengths, family, observed, offset, log_exposure, noise_var, init, max_iter, tol) are
    those of ``leg.laplace_posterior_batch``; targets, ``target_lengths`` and ``check_sorted`` those of
    ``predictive_posterior_batch`` (dense target_ts [B, p] or [p], ragged [P] with host ``target_lengths``; a series may
    have no target).  ``target_log_exposure`` / ``target_noise_var`` (the latter required by ``family="gaussian"``),
    ``target_ys`` (held-out values) and ``target_observed`` (which of them exist) are in the layout of the targets:
    [B, p, obs_dim] dense, [P, obs_dim] ragged.

    ``z_mean`` [.., d] and ``z_cov`` [.., d, d] are the latent Gaussian at every target; ``eta_mean``, ``eta_var``, ``mean``,
    ``var`` and ``logpdf`` [.., obs_dim] what ``leg.glm_predictive`` says of it (``logpdf`` is None without ``target_ys``);
    ``converged`` [B] is the Newton loop's report: a series that has not converged within ``max_iter`` steps still
    predicts, from the point the loop left it at.

    How: the Newton loop of ``leg.laplace_posterior_batch`` -- unless ``posterior=`` hands in the ``LaplacePosterior`` of
    the same data, in which case no Newton step runs --, then ONE launch of cgps_leg_intercast_seg (a lane per target,
    never across a series boundary) and ONE of cgps_leg_glm_predict (a lane per target and channel).  Every ValueError is
    raised before anything is launched."""
    with torch.no_grad():
        fam_t = leg._glm_predict_family(family, target_log_exposure, target_noise_var, "target_")
        for name, t in (("target_ys", target_ys), ("target_observed", target_observed)):
            if t is not None and not isinstance(t, torch.Tensor):
                raise ValueError("%s must be a tensor" % name)
        if target_observed is not None and target_ys is None:
            raise ValueError("target_observed says which entries of target_ys exist: it needs target_ys")
        fam, ts_f, ys_f, lens, observed, offset, extra, init, dense, bn, tol = leg._laplace_args(
            m, ts, ys, lengths, family, observed, offset, log_exposure, noise_var, init, max_iter, tol, on_gpu=False)
        tt, tlens, bp = _batch_targets(target_ts, target_lengths, lens, dense)
        obs, d = m.B.shape
        dt, dev = m.N.dtype, ts_f.device
        P, R = sum(tlens), sum(lens)
        like = (bp + (obs,)) if dense else (P, obs)
        flat = {}
        for name, t in (("target_ys", target_ys), ("target_observed", target_observed),
                        ("target_log_exposure", target_log_exposure), ("target_noise_var", target_noise_var)):
            if t is not None:
                t = leg._batch_like_xs(t, _TARGET_SPECS[name], like, dense)
                flat[name] = t.unsqueeze(-1).expand(-1, obs) if t.dim() == 1 else t
        if posterior is not None:
            post = _flat_posterior(posterior, dense, bn, R, d)
        tensors = [t for t in (m.N, ts_f, ys_f, observed, offset, extra, init, tt) if t is not None] + list(flat.values())
        if posterior is not None:
            tensors += list(post)
        if lens and not all(t.is_cuda for t in tensors):
            raise leg._hip.CgpsError("the Laplace predictions run on GPU tensors only (there is no CPU implementation)")
        shape = bp if dense else (P,)
        e = lambda *tail, dtype=dt: torch.empty(shape + tail, dtype=dtype, device=dev)      # noqa: E731
        if not lens:
            return GlmPredictions(e(d), e(d, d), e(obs), e(obs), e(obs), e(obs), None if target_ys is None else e(obs),
                                  torch.empty(0, dtype=torch.bool, device=dev))
        tt = tt.to(ts_f.dtype)
        tplan = leg._cached_batch_plan(tlens, dev, make=_TargetPlan)
        if check_sorted and P > 1:
            assert bool(((tt[1:] - tt[:-1] > 0) | tplan.across).all())         # reference :471, per series
        if posterior is None:
            mean, Sd, So, _, _, conv = leg._laplace_flat(m, fam, ts_f, ys_f, lens, observed, offset, extra, init, max_iter, tol)
        else:
            mean, Sd, So, conv = post
        if P == 0:
            return GlmPredictions(e(d), e(d, d), e(obs), e(obs), e(obs), e(obs), None if target_ys is None else e(obs), conv)
        plan = leg._cached_batch_plan(lens, dev)
        zm, zc = _intercast_models_hip(m.G, mean, Sd, So, ts_f, plan, tt, tplan)
        c = lambda t: None if t is None else t.to(dt).contiguous()             # noqa: E731
        t_extra = flat.get("target_noise_var") if fam_t == leg._hip.GLM_GAUSSIAN else flat.get("target_log_exposure")
        t_obs = flat.get("target_observed")
        out = leg._glm_predict(fam_t, zm, zc, c(flat.get("target_ys")), None if t_obs is None else t_obs.contiguous(),
                               c(offset), c(t_extra), c(m.B))
        r = lambda t, *tail: None if t is None else t.reshape(shape + tail)      # noqa: E731
        return GlmPredictions(r(zm, d), r(zc, d, d), *[r(t, obs) for t in out], conv)


def laplace_predictions(m, ts, ys, target_ts, family, observed=None, offset=None, log_exposure=None, noise_var=None,
                        target_log_exposure=None, target_noise_var=None, target_ys=None, target_observed=None,
                        posterior=None, init=None, max_iter=50, tol=None, check_sorted=True):
    """``laplace_predictions_batch`` of one series ts[n], ys[n, obs_dim] at target_ts[p]: ``GlmPredictions`` with z_mean
    [p, d], z_cov [p, d, d], the rest [p, obs_dim] and a 0-d ``converged``; the ``target_*`` arguments [p, obs_dim];
    ``posterior``: what ``leg.laplace_posterior`` returned for the same series."""
    if not isinstance(ts, torch.Tensor) or not isinstance(ys, torch.Tensor) or ts.dim() != 1 or ys.dim() != 2:
        raise ValueError("one series wants ts[n] and ys[n, obs_dim]")
    if ts.shape[0] < 1:
        raise ValueError("series of length 0")
    if not isinstance(target_ts, torch.Tensor) or target_ts.dim() != 1:
        raise ValueError("one series wants target_ts[p]")
    if posterior is not None:
        try:
            posterior = leg.LaplacePosterior(posterior.mean, posterior.cov, None, None, posterior.converged.reshape(1))
        except (AttributeError, TypeError):
            raise ValueError("posterior must be a LaplacePosterior, what leg.laplace_posterior returns for the same series")
    r = laplace_predictions_batch(m, ts, ys, target_ts, [ts.shape[0]], [target_ts.shape[0]], family, observed, offset,
                                  log_exposure, noise_var, target_log_exposure, target_noise_var, target_ys, target_observed,
                                  posterior, init, max_iter, tol, check_sorted)
    return r._replace(converged=r.converged[0])


# ---- many models over one batch --------------------------------------------------------------------------------
def _predictive_posterior_models_flat(ms, ts, xs, target_ts, lengths, target_lengths, observed, noise_var, check_sorted):
    """(means [M, P, rank], covs [M, P, rank, rank], B stacked [M, obs, rank], shape of the dense targets (B, p) or None)
    of the validated call: the predictions in the order of the flattened targets."""
    ms, mats, ts_f, xs_f, lens, observed, noise_var, dense, _ = leg._models_posterior_args(ms, ts, xs, lengths, observed,
                                                                                           noise_var)
    tt, tlens, bp = _batch_targets(target_ts, target_lengths, lens, dense)
    M, d, dt, dev = len(ms), mats[0].shape[1], mats[0].dtype, ts_f.device
    P = sum(tlens)
    if not lens or P == 0:
        return torch.empty(M, P, d, dtype=dt, device=dev), torch.empty(M, P, d, d, dtype=dt, device=dev), mats[2], bp
    tt = tt.to(ts_f.dtype)
    if not leg._posterior_batch_supported(ts_f, mats[0][0]):
        outs = leg._posterior_models_per_model(ms, lambda m: predictive_posterior_batch(
            m, ts_f, xs_f, tt, lens, tlens, observed, noise_var, check_sorted))
        return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs]), mats[2], bp
    tplan = leg._cached_batch_plan(tlens, mats[0].device, make=_TargetPlan)
    if check_sorted and P > 1:
        assert bool(((tt[1:] - tt[:-1] > 0) | tplan.across).all())             # reference :471, per series
    plan = leg._cached_batch_plan(lens, mats[0].device)
    G, source, term, rows, v = leg._models_posterior_operands(mats, xs_f, observed, noise_var)
    ts_c, tt_c = ts_f.to(dt).contiguous(), tt.to(dt).contiguous()
    pm = torch.empty(M, P, d, dtype=dt, device=G.device)
    pv = torch.empty(M, P, d, d, dtype=dt, device=G.device)
    for k0, k1, mean, Sd, So in leg._posterior_models_chunks(plan, ts_c, G, source, term, rows, v):
        _intercast_models_hip(G[k0:k1], mean, Sd, So, ts_c, plan, tt_c, tplan, pm[k0:k1], pv[k0:k1])
    return pm, pv, mats[2], bp


def predictive_posterior_models(ms, ts, xs, target_ts, lengths=None, target_lengths=None, observed=None, noise_var=None,
                                check_sorted=True):
    """``predictive_posterior_batch`` of M LEG models for the same B series and the same targets in one call: slot k is
    ``predictive_posterior_batch(ms[k], ...)``.  Inference only: runs under ``torch.no_grad``.

    ``ms``, the layouts, ``observed`` and ``noise_var``: those of ``leg.insample_posterior_models`` (all models share the
    data, the mask and the variances).  Targets, ``target_lengths`` and ``check_sorted``: those of
    ``predictive_posterior_batch``; the targets are shared by all models.  Dense returns (means [M, B, p, rank], covs
    [M, B, p, rank, rank]), ragged ([M, P, rank], [M, P, rank, rank]) in the order of target_ts.

    How: ``leg.insample_posterior_models``'s one factorisation of the concatenated system of all models' batches, then
    ONE launch of cgps_leg_intercast_models, grid (target blocks, M): model k's workgroups read its slices of the
    posterior and never a row of another model or series.  More than ``leg.MODELS_POSTERIOR_MAX_ROWS`` rows go in chunks
    of whole models, each with its own factorisation and launch.  A repeated call with the same lengths and target
    lengths copies nothing from the host.  Errors, NaN propagation with ``cr.CHECK_POSITIVE_DEFINITE`` off and
    unsupported inputs (one ``predictive_posterior_batch`` per model): ``leg.insample_posterior_models``."""
    with torch.no_grad():
        pm, pv, _, bp = _predictive_posterior_models_flat(ms, ts, xs, target_ts, lengths, target_lengths, observed, noise_var,
                                                          check_sorted)
        if bp is not None:
            M, d = pm.shape[0], pm.shape[-1]
            return pm.reshape((M,) + bp + (d,)), pv.reshape((M,) + bp + (d, d))
        return pm, pv


def make_predictions_models(ms, ts, xs, target_ts, lengths=None, target_lengths=None, observed=None, noise_var=None,
                            check_sorted=True):
    """``make_predictions_batch`` of M LEG models for the same B series and targets in one call: predicted observation
    mean [M, ..., obs_dim] and covariance [M, ..., obs_dim, obs_dim], every model's latent posterior mapped through its own
    B, without observation noise.  Arguments, layouts ([M, B, p, ...] dense, [M, P, ...] ragged), inference-only results
    and errors: ``predictive_posterior_models``.  ``combine_predictions`` turns the M predictions into one."""
    with torch.no_grad():
        pm, pv, Bm, bp = _predictive_posterior_models_flat(ms, ts, xs, target_ts, lengths, target_lengths, observed,
                                                           noise_var, check_sorted)
        # B C B^T without a product broadcast over the targets (M P tiny matrix products): C B^T as one product per model
        # over all its targets' rows, then the obs_dim x obs_dim result as rank sums of elementwise products
        (M, P, d), o = pm.shape, Bm.shape[1]
        Bt = Bm.transpose(1, 2).contiguous()
        om = torch.bmm(pm, Bt)
        half = torch.bmm(pv.reshape(M, P * d, d), Bt).view(M, P, 1, d, o)                # C B^T: [M, P, 1, d, obs]
        Bl = Bm.unsqueeze(1).unsqueeze(-1)                                               # [M, 1, obs, d, 1]
        ov = Bl[:, :, :, 0] * half[:, :, :, 0]
        for j in range(1, d):
            ov = ov + Bl[:, :, :, j] * half[:, :, :, j]
        if bp is not None:
            return om.reshape((M,) + bp + (o,)), ov.reshape((M,) + bp + (o, o))
        return om, ov


def combine_predictions(means, covs, weights):
    """The moment-matched mixture of M predictions: mean sum_k w_k mu_k and covariance sum_k w_k (C_k + mu_k mu_k^T) -
    mu mu^T, for means [M, ..., c] and covs [M, ..., c, c] as ``make_predictions_models`` and
    ``predictive_posterior_models`` return them.  ``weights``: [M] -- one weight per model -- or [M, B] matching the
    second dimension of means (one per model and series of the dense layout; per model and target of the ragged one):
    responsibilities, or softmaxed log-likelihoods from ``leg.log_likelihood_models``.  The weights are NOT normalised
    for the caller.  The sum over k runs in ascending order with plain multiplies and adds, so a slot does not depend on
    the other series.  Pure torch, any device; ValueError when the shapes do not agree."""
    for name, t in (("means", means), ("covs", covs), ("weights", weights)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s must be a tensor" % name)
    if means.dim() < 2 or means.shape[0] < 1:
        raise ValueError("means must be [M, ..., c] with M >= 1, got %s" % (tuple(means.shape),))
    if tuple(covs.shape) != tuple(means.shape) + (means.shape[-1],):
        raise ValueError("covs must be %s for means %s, got %s"
                         % (tuple(means.shape) + (means.shape[-1],), tuple(means.shape), tuple(covs.shape)))
    if weights.dim() not in (1, 2) or weights.dim() > means.dim() - 1 or tuple(weights.shape) != tuple(means.shape[:weights.dim()]):
        raise ValueError("weights must be [M] or [M, B] matching the leading dimensions of means %s, got %s"
                         % (tuple(means.shape), tuple(weights.shape)))
    w = weights.to(means.dtype).reshape(tuple(weights.shape) + (1,) * (means.dim() - weights.dim()))
    mu, second = None, None
    for k in range(means.shape[0]):
        mk, wk = means[k], w[k]
        sk = covs[k] + mk.unsqueeze(-1) * mk.unsqueeze(-2)
        mu = wk * mk if mu is None else mu + wk * mk
        second = wk.unsqueeze(-1) * sk if second is None else second + wk.unsqueeze(-1) * sk
    return mu, second - mu.unsqueeze(-1) * mu.unsqueeze(-2)

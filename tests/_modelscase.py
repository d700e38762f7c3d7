"""Cases shared by tests/test_leg_models_missing.py and tests/test_leg_models_noise.py: models, ragged batches at the
kernel's lane-count boundaries, masks and the comparison with a loop of ``leg.log_likelihood_batch`` over the models."""
import numpy as np
import torch

from cyclic_gps import leg

F64, F32 = torch.float64, torch.float32

# rows per lane 1 -> 2 -> 3 at 256 lanes and (7 x 7 fp64) at 128 lanes; one, two and three rows
BOUNDARY_LENGTHS = [1, 2, 3, 129, 255, 256, 257, 513]
DEAD, ENDS = 4, 6                       # series 4 (255 rows) observes nothing; series 6 (257 rows) loses its first and last row


def model(d, obs, dtype, seed, device="cuda"):
    """(the conditioning of test_leg_models._model)"""
    gen = torch.Generator().manual_seed(seed)
    N = torch.tril(0.4 * torch.randn(d, d, generator=gen, dtype=F64)) + 0.8 * torch.eye(d, dtype=F64)
    R = torch.tril(0.3 * torch.randn(d, d, generator=gen, dtype=F64), -1)
    B = 0.7 * torch.randn(obs, d, generator=gen, dtype=F64)
    L = torch.tril(0.2 * torch.randn(obs, obs, generator=gen, dtype=F64)) + 0.6 * torch.eye(obs, dtype=F64)
    return leg.LEGMatrices(*(t.to(dtype).to(device) for t in (N, R, B, L)))


def starts(lengths):
    s = [0]
    for n in lengths:
        s.append(s[-1] + n)
    return s


def ragged(lengths, obs, gen, dtype, device="cuda", gap0=None):
    """Concatenated series, every one on a clock of its own, with irregular gaps (fp32: gaps of at least 0.5, so that
    I - E^T E of the random generators stays well conditioned)."""
    if gap0 is None:
        gap0 = 0.05 if dtype == F64 else 0.5
    ts, xs = [], []
    for n in lengths:
        t0 = 50.0 * torch.rand((), generator=gen, dtype=F64) - 25.0
        ts.append(t0 + torch.cumsum(gap0 + 0.5 * torch.rand(n, generator=gen, dtype=F64), 0))
        xs.append(torch.randn(n, obs, generator=gen, dtype=F64))
    return torch.cat(ts).to(dtype).to(device), torch.cat(xs).to(dtype).to(device)


def mask(lengths, obs, gen, keep=0.6, dead=None, ends=None, device="cuda"):
    """bool [R, obs] that keeps ~60 % of the entries; series ``dead`` wholly unobserved, series ``ends`` without its first
    and its last row."""
    st = starts(lengths)
    m = torch.rand(st[-1], obs, generator=gen) < keep
    if dead is not None:
        m[st[dead]:st[dead + 1]] = False
    if ends is not None:
        m[st[ends]] = False
        m[st[ends + 1] - 1] = False
    return m.to(device)


def poisoned(x, observed):
    """x with NaN wherever it is not observed (observed [R, obs] or [R]; x [R, obs] or [R])."""
    o = observed if observed.dim() == x.dim() else (observed.unsqueeze(-1) if x.dim() == 2 else observed.all(-1))
    return torch.where(o, x, torch.full((), float("nan"), dtype=x.dtype, device=x.device))


def close(got, want, rtol):
    return abs(got - want) <= rtol * max(1.0, abs(want))


def assert_values(got, ref, rtol, what=""):
    """|got - ref| <= rtol max(1, |ref|) entry by entry, the figures printed first"""
    g, r = got.detach().flatten().tolist(), ref.detach().flatten().tolist()
    worst = max([abs(a - b) / max(1.0, abs(b)) for a, b in zip(g, r)] + [0.0])
    print("%s worst %.3e (bound %.1e)" % (what, worst, rtol))
    for i, (a, b) in enumerate(zip(g, r)):
        assert close(a, b, rtol), (what, i, a, b)


def values_and_grads(fn, ms, ts, xs, w, noise_var=None):
    """fn(models, ts, xs, noise_var) -> [M, B]; the values and the gradients of (out * w).sum() in every model's four
    matrices, xs, ts and (when given) noise_var, on fresh leaves."""
    mm = [leg.LEGMatrices(*(p.detach().clone().requires_grad_(True) for p in (m.N, m.R, m.B, m.Lambda))) for m in ms]
    t, x = ts.detach().clone().requires_grad_(True), xs.detach().clone().requires_grad_(True)
    s = None if noise_var is None else noise_var.detach().clone().requires_grad_(True)
    out = fn(mm, t, x, s)
    (out * w).sum().backward()
    grads = [p.grad for m in mm for p in (m.N, m.R, m.B, m.Lambda)] + [x.grad, t.grad] + ([] if s is None else [s.grad])
    return out.detach(), grads


def compare_with_the_loop(ms, ts, xs, lengths, w, observed, noise_var=None, value_rtol=1e-9):
    """values (value_rtol) and gradients (rtol 1e-7, atol 1e-9, as test_leg_models._compare_with_the_loop) of the one call
    against a loop of log_likelihood_batch over the models under autograd"""
    loop = lambda mm, t, x, s: torch.stack([leg.log_likelihood_batch(m, t, x, lengths, observed, s) for m in mm])  # noqa: E731
    one = lambda mm, t, x, s: leg.log_likelihood_models_observed(mm, t, x, lengths, observed, s)                             # noqa: E731
    v0, g0 = values_and_grads(loop, ms, ts, xs, w, noise_var)
    v1, g1 = values_and_grads(one, ms, ts, xs, w, noise_var)
    assert_values(v1, v0, value_rtol, "values against the loop")
    names = ["%s of model %d" % (n, k) for k in range(len(ms)) for n in ("N", "R", "B", "Lambda")] + ["xs", "ts", "noise_var"]
    for name, a, r in zip(names, g1, g0):
        assert a is not None and r is not None, name
        assert not bool(torch.isnan(a).any()), name
        np.testing.assert_allclose(a.cpu().numpy(), r.cpu().numpy(), rtol=1e-7, atol=1e-9, err_msg=name)


def check_grad(got, want, what):
    """test_leg_models._check_grad: rtol 1e-7, atol 1e-10 x the largest entry"""
    want = want.detach().to("cpu", F64)
    assert got is not None, what + " is missing"
    got = got.detach().to("cpu", F64)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-7, atol=1e-10 * float(want.abs().max()), err_msg=what)

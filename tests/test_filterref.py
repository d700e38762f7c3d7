"""The forward recursion of tests/_filterref.py (what cgps_leg_filter evaluates: DESIGN.md 4.22) in fp64 against the
dense truths of ``_noiseref``, which need no filtering algebra: the sum of the row terms is the log density of all
observed entries; the filtered state of row i is the dense posterior with the mask's rows > i switched off; the
one-step-ahead predictive is that posterior with rows >= i switched off, pushed through B plus the row's noise.
Bound: 1e-12 relative to 1 + |value|.  Also the argument checks of leg.filter_predictive*, which come before anything
is launched and so run on CPU tensors."""
import pytest
import torch

import _filterref
import _noiseref as nr
from cyclic_gps import _hip, leg
from test_leg_posterior_batch import _model

F64 = torch.float64
CASES = [(1, 1, 1), (1, 1, 2), (5, 1, 7), (5, 3, 7), (8, 8, 6), (3, 2, 65)]
BOUND = 1e-12


def _rel(got, want):
    return float(((got - want).abs() / (1 + want.abs())).max())


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("d,obs,n", CASES)
def test_recursion_matches_the_dense_truths(d, obs, n, seed):
    (Nm, Rm, Bm, Lm, xs, ts, s), mask = nr.leg_case(d, obs, n, seed)
    mats = (Nm, Rm, Bm, Lm)
    out = _filterref.filter_ref(mats, ts, xs, s, mask)
    ll = nr.leg_dense_loglik(Nm, Rm, Bm, Lm, ts, xs, s, mask)
    worst = {"loglik": _rel(out["loglik"], ll)}
    LLT = Lm @ Lm.T + 1e-9 * torch.eye(obs, dtype=F64)
    rows = torch.arange(n).unsqueeze(1)
    for i in range(n):
        upto = mask & (rows <= i)
        mean, cov = nr.leg_dense_posterior(Nm, Rm, Bm, Lm, ts, xs, s, upto)
        worst["z_mean"] = max(worst.get("z_mean", 0.0), _rel(out["z_mean"][i], mean[i]))
        worst["z_cov"] = max(worst.get("z_cov", 0.0), _rel(out["z_cov"][i], cov[i, :, i, :]))
        before = mask & (rows < i)
        mean, cov = nr.leg_dense_posterior(Nm, Rm, Bm, Lm, ts, xs, s, before)
        so = torch.where(mask[i], s[i], torch.zeros_like(s[i]))
        worst["mean"] = max(worst.get("mean", 0.0), _rel(out["mean"][i], Bm @ mean[i]))
        worst["cov"] = max(worst.get("cov", 0.0), _rel(out["cov"][i], Bm @ cov[i, :, i, :] @ Bm.T + LLT + torch.diag(so)))
    print("d %d obs %d n %d seed %d: worst errors relative to 1 + |value|: %s" % (d, obs, n, seed, worst))
    assert all(v <= BOUND for v in worst.values()), worst
    assert bool((out["logpdf"][~mask.any(1)] == 0).all())


def test_recursion_continues_from_a_state():
    (Nm, Rm, Bm, Lm, xs, ts, s), mask = nr.leg_case(3, 2, 9, 4)
    mats = (Nm, Rm, Bm, Lm)
    whole = _filterref.filter_ref(mats, ts, xs, s, mask)
    for h in (1, 4, 8):
        head = _filterref.filter_ref(mats, ts[:h], xs[:h], s[:h], mask[:h])
        tail = _filterref.filter_ref(mats, ts[h:], xs[h:], s[h:], mask[h:], init=head["state"])
        for key in ("mean", "cov", "logpdf", "z_mean", "z_cov"):
            assert _rel(tail[key], whole[key][h:]) <= BOUND, (h, key)
        assert _rel(head["loglik"] + tail["loglik"], whole["loglik"]) <= BOUND


# ---- leg.filter_predictive*: every ValueError before anything is launched -------------------------------------------
def _cpu_case(B=3, n=4, obs=2, d=3):
    m, _ = _model(d, obs, 5)
    ts = torch.cumsum(torch.ones(B, n, dtype=F64), 1)
    return m, ts, torch.zeros(B, n, obs, dtype=F64)


def _state(lead, d, t):
    eye = torch.eye(d, dtype=F64)
    return leg.FilterState(t, torch.zeros(tuple(lead) + (d,), dtype=F64), eye.expand(tuple(lead) + (d, d)).clone())


def test_validation_errors_come_before_anything_runs():
    m, ts, xs = _cpu_case()
    B, n, obs = xs.shape
    d = 3
    tsr, xsr, lens = ts.reshape(-1), xs.reshape(B * n, obs), [n] * B
    ms = [m, _model(3, obs, 6)[0]]
    one, bat = leg.filter_predictive, leg.filter_predictive_batch
    mod = lambda *a, **k: leg.filter_predictive_models(ms, *a, **k)      # noqa: E731
    first = ts[:, 0].clone()
    bad = [
        # layouts, channels, lengths, masks and variances: the checks of insample_posterior_batch / _models
        lambda: one(m, ts, xs),
        lambda: one(m, ts[0], xs[0, :, :1]),
        lambda: bat(m, ts, xsr),
        lambda: bat(m, ts, xs[..., :1]),
        lambda: bat(m, tsr, xsr, lengths=[n] * (B - 1)),
        lambda: bat(m, tsr, xsr, lengths=[n, n, n - 1, 1, 0]),
        lambda: mod(ts, xsr),
        lambda: mod(tsr, xsr, lengths=[n] * (B - 1)),
        lambda: leg.filter_predictive_models([], ts, xs),
        lambda: one(m, ts[0], xs[0], observed=torch.ones(n, obs)),
        lambda: one(m, ts[0], xs[0], noise_var=torch.ones(n, obs + 1, dtype=F64)),
        lambda: bat(m, ts, xs, observed=torch.ones(B, n + 1, dtype=torch.bool)),
        lambda: bat(m, ts, xs, noise_var=torch.ones(B, n, obs, dtype=torch.int64)),
        lambda: mod(ts, xs, observed=torch.ones(B, n, obs)),
        # an init of the wrong kind or shape
        lambda: one(m, ts[0], xs[0], init=(first[0], torch.zeros(d, dtype=F64))),
        lambda: one(m, ts[0], xs[0], init=_state((1,), d, first[:1])),
        lambda: one(m, ts[0], xs[0], init=_state((), d + 1, first[0])),
        lambda: bat(m, ts, xs, init=_state((), d, first[0])),
        lambda: bat(m, ts, xs, init=_state((B + 1,), d, first)),
        lambda: bat(m, ts, xs, init=_state((B,), d, first[:2])),
        lambda: bat(m, tsr, xsr, lengths=lens, init=_state((B,), d + 1, first)),
        lambda: mod(ts, xs, init=_state((B,), d, first)),                        # no models' axis
        lambda: mod(ts, xs, init=_state((3, B), d, first)),                      # three states for two models
        lambda: bat(m, ts, xs, init=leg.FilterState(first, torch.zeros(B, d, dtype=torch.int64),
                                                    torch.zeros(B, d, d, dtype=F64))),
        # a state later than the first row of its series
        lambda: one(m, ts[0], xs[0], init=_state((), d, first[0] + 0.5)),
        lambda: bat(m, ts, xs, init=_state((B,), d, first + torch.tensor([0.0, 1e-9, 0.0], dtype=F64))),
        lambda: bat(m, tsr, xsr, lengths=lens, init=_state((B,), d, first + 1.0)),
        lambda: mod(ts, xs, init=_state((2, B), d, first + torch.tensor([0.0, 0.0, 2.0], dtype=F64))),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d raised nothing" % k)


def test_valid_cpu_calls_have_no_cpu_implementation():
    """Valid arguments on CPU tensors get past every check (a zero gap to the first row included) and then fail as the
    other calls do without a GPU: there is no CPU implementation and no fall-back."""
    m, ts, xs = _cpu_case()
    B, d = ts.shape[0], 3
    ms = [m, _model(3, xs.shape[2], 6)[0]]
    for call in (lambda: leg.filter_predictive(m, ts[0], xs[0], init=_state((), d, ts[0, 0])),
                 lambda: leg.filter_predictive_batch(m, ts, xs, init=_state((B,), d, ts[:, 0] - 0.25)),
                 lambda: leg.filter_predictive_models(ms, ts, xs, init=_state((2, B), d, ts[:, 0].clone())),
                 lambda: leg.filter_predictive_batch(m, ts, xs)):
        with pytest.raises(_hip.CgpsError):
            call()


def test_empty_batches_give_empty_tensors():
    m, ts, xs = _cpu_case()
    n, obs, d = ts.shape[1], xs.shape[2], 3
    ms = [m, _model(3, obs, 6)[0]]
    r = leg.filter_predictive_batch(m, ts[:0], xs[:0])
    assert tuple(r.mean.shape) == (0, n, obs) and tuple(r.cov.shape) == (0, n, obs, obs) and tuple(r.logpdf.shape) == (0, n)
    assert tuple(r.z_mean.shape) == (0, n, d) and tuple(r.z_cov.shape) == (0, n, d, d)
    assert tuple(r.loglik.shape) == (0,) and r.loglik.dtype == F64 and r.state is None
    r = leg.filter_predictive_batch(m, ts.reshape(-1)[:0], xs.reshape(-1, obs)[:0], lengths=[])
    assert tuple(r.mean.shape) == (0, obs) and tuple(r.z_cov.shape) == (0, d, d) and tuple(r.loglik.shape) == (0,)
    r = leg.filter_predictive_models(ms, ts[:0], xs[:0])
    assert tuple(r.mean.shape) == (2, 0, n, obs) and tuple(r.z_mean.shape) == (2, 0, n, d) and tuple(r.loglik.shape) == (2, 0)
    r = leg.filter_predictive_models(ms, ts.reshape(-1)[:0], xs.reshape(-1, obs)[:0], lengths=[])
    assert tuple(r.cov.shape) == (2, 0, obs, obs) and tuple(r.logpdf.shape) == (2, 0)
    r = leg.filter_predictive(m, ts[0, :0], xs[0, :0])
    assert tuple(r.mean.shape) == (0, obs) and tuple(r.z_cov.shape) == (0, d, d)
    assert tuple(r.loglik.shape) == () and float(r.loglik) == 0.0 and r.loglik.dtype == F64

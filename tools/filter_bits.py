"""Record, for one build of libcgps.so, every output of the calls that go through the per-row LEG kernels
(leg.filter_predictive_models with and without chunk_rows, leg.loo_predictive_models, leg.sample_observations_models),
and compare two such records bit for bit: a refactor of those kernels must change nothing.

    CGPS_LIB=/path/to/libcgps.so python tools/filter_bits.py record out.pt     (one fresh process per build)
    python tools/filter_bits.py compare a.pt b.pt                              (exit status 1 on any difference)

Cases: rank 1..8 x obs_dim {1, 2, 3, 4, 5, 8} x {fp64, fp32}, two models, three ragged series of 1, 5 and 9 rows; with and
without ``observed`` (rows that observe nothing in the middle of a series and as a series' first row), ``noise_var`` and
``init`` (one series continues AT its first time stamp); chunk_rows in {None, (4, 2), (1, 2)}; one case with a repeated
time stamp and one with a negative variance under cr.CHECK_POSITIVE_DEFINITE = False."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cyclic-gps_amd")]

LENGTHS = [1, 5, 9]
R = sum(LENGTHS)
CHUNKINGS = [None, (4, 2), (1, 2)]
F64 = torch.float64


def model(d, obs, seed, dtype):
    from cyclic_gps import leg
    gen = torch.Generator().manual_seed(seed)
    N = torch.tril(0.4 * torch.randn(d, d, generator=gen, dtype=F64), -1) + torch.diag(0.7 + 0.3 * torch.rand(d, generator=gen, dtype=F64))
    Rm = torch.tril(0.3 * torch.randn(d, d, generator=gen, dtype=F64), -1)
    B = 0.7 * torch.randn(obs, d, generator=gen, dtype=F64)
    L = torch.tril(0.2 * torch.randn(obs, obs, generator=gen, dtype=F64)) + 0.6 * torch.eye(obs, dtype=F64)
    return leg.LEGMatrices(*(t.to(dtype).cuda() for t in (N, Rm, B, L)))


def data(d, obs, seed, dtype):
    from cyclic_gps import leg
    gen = torch.Generator().manual_seed(seed)
    ts = torch.cat([3.0 - 1.1 * b + torch.cumsum(0.2 + torch.rand(n, generator=gen, dtype=F64), 0) for b, n in enumerate(LENGTHS)])
    xs = torch.randn(R, obs, generator=gen, dtype=F64)
    mask = torch.rand(R, obs, generator=gen) < 0.7
    mask[4] = False                                        # the middle of the second series
    mask[6] = False                                        # the first row of the third
    mask[10] = False                                       # and its middle
    nv = torch.rand(R, obs, generator=gen, dtype=F64)
    starts = torch.tensor([0, 1, 6])
    t0 = ts[starts] - torch.tensor([0.3, 0.4, 0.0], dtype=F64)
    mean = torch.randn(2, 3, d, generator=gen, dtype=F64)
    W = torch.randn(2, 3, d, d, generator=gen, dtype=F64)
    cov = 0.5 * torch.eye(d, dtype=F64) + 0.1 * W @ W.transpose(2, 3)
    init = leg.FilterState(*(t.to(dtype).cuda() for t in (t0, mean, cov)))
    z = torch.randn(2, R, d, 5, generator=gen, dtype=F64)
    return tuple(t.to(dtype).cuda() for t in (ts, xs)) + (mask.cuda(), nv.to(dtype).cuda(), init, z.to(dtype).cuda())


def record(path):
    from cyclic_gps import _hip, leg
    out = {}

    def keep(key, tensors):
        for j, t in enumerate(tensors):
            out["%s/%d" % (key, j)] = t.cpu()

    def flat(f):
        return list(f[:6]) + list(f.state)

    for dtype in (F64, torch.float32):
        for d in range(1, 9):
            for obs in (1, 2, 3, 4, 5, 8):
                tag = "%s d%d obs%d" % ("f64" if dtype == F64 else "f32", d, obs)
                ms = [model(d, obs, 100 * d + obs + k, dtype) for k in range(2)]
                ts, xs, mask, nv, init, z = data(d, obs, 1000 + 10 * d + obs, dtype)
                for ob in (None, mask):
                    for s in (None, nv):
                        kw = dict(lengths=LENGTHS, observed=ob, noise_var=s)
                        sub = "%s ob%d nv%d" % (tag, ob is not None, s is not None)
                        for st in (None, init):
                            for ch in CHUNKINGS:
                                keep("filter %s init%d ch%s" % (sub, st is not None, ch),
                                     flat(leg.filter_predictive_models(ms, ts, xs, init=st, chunk_rows=ch, **kw)))
                        for leave in ("entry", "row"):
                            try:
                                keep("loo %s %s" % (sub, leave), leg.loo_predictive_models(ms, ts, xs, leave=leave, **kw))
                            except leg.cr.NotPSDError as e:            # (the smoother's, before the LOO kernel runs)
                                print("loo %s %s: %s" % (sub, leave, e))
                        keep("obs %s" % sub, [leg.sample_observations_models(ms, z, 7, **kw)])
                # a gap of zero length inside a series, and a negative variance (rows fail: NaN from there on)
                ts0 = ts.clone()
                ts0[9] = ts0[8]
                bad = nv.clone()
                bad[8] = -5.0
                leg.cr.CHECK_POSITIVE_DEFINITE = False
                try:
                    for ch in CHUNKINGS:
                        keep("filter %s zero gap ch%s" % (tag, ch),
                             flat(leg.filter_predictive_models(ms, ts0, xs, lengths=LENGTHS, observed=mask, noise_var=nv, chunk_rows=ch)))
                        keep("filter %s negative variance ch%s" % (tag, ch),
                             flat(leg.filter_predictive_models(ms, ts, xs, lengths=LENGTHS, noise_var=bad, chunk_rows=ch)))
                finally:
                    leg.cr.CHECK_POSITIVE_DEFINITE = True
    torch.save(out, path)
    nans = sum(int(torch.isnan(t).any()) for t in out.values() if t.is_floating_point())
    print("recorded %d tensors (%d with NaN) from %s" % (len(out), nans, _hip.LIB_PATH))


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    assert sorted(a) == sorted(b), "the two records hold different cases"
    bad = []
    for k in sorted(a):
        x, y = a[k], b[k]
        same = x.shape == y.shape and x.dtype == y.dtype and torch.equal(torch.isnan(x), torch.isnan(y)) and \
            torch.equal(x.nan_to_num(0.0), y.nan_to_num(0.0))
        if x.is_floating_point() and same:                 # the sign of a zero counts as a bit too
            same = torch.equal(torch.signbit(x), torch.signbit(y))
        if not same:
            bad.append(k)
    print("compared %d tensors: %s" % (len(a), "all equal" if not bad else "%d differ" % len(bad)))
    for k in bad[:40]:
        x, y = a[k].double(), b[k].double()
        if x.shape == y.shape:
            diff = (x - y).abs().nan_to_num(0.0)
            print("  differs: %s: %d of %d entries, by %.3e at most (values up to %.3e), NaN in %d / %d places"
                  % (k, int((diff > 0).sum()), x.numel(), float(diff.max()), float(x.abs().nan_to_num(0.0).max()),
                     int(torch.isnan(x).sum()), int(torch.isnan(y).sum())))
        else:
            print("  differs: %s: shapes %s and %s" % (k, tuple(x.shape), tuple(y.shape)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "record":
        record(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)

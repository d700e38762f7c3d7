"""Time cgps_sample against the unfused composition of existing calls (device events after warm-up, the versions
alternated in one process, all through the C ABI on preallocated buffers):

    fused     cgps_sample(factor, mean)                                      noise made in registers, mean added in the store
    unfused   cgps_normal_fill -> cgps_backsolve -> x += mean                the definition of the result (the tests' reference)
    randn     torch.randn -> cgps_backsolve -> x += mean                     other noise; what glue around torch would cost

Cases: N = 2^20, d = 4, fp64, S = 8 (conditioned_system of the tests); n = 502, rank 5, fp64, S = 1024 (the prior
precision of the model of tests/golden/leg_co2like.npz at 502 monthly time stamps).

    python tools/time_sample.py [--rounds 30] [--json out.json]
    python tools/time_sample.py --profile-only      (fused calls only, for rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cyclic-gps_amd"), os.path.join(ROOT, "tests")]
from cyclic_gps import _hip, leg  # noqa: E402
import cyclic_gps.cyclic_reduction as cr  # noqa: E402


def big_case():
    import _util
    n, d = 2 ** 20, 4
    Rs, Os, _, mean, _ = _util.conditioned_system(n, d, device="cuda")
    return "N=2^20 d=4 fp64 S=8", cr.decompose(Rs, Os), mean.contiguous(), 8


def leg_case():
    g = np.load(os.path.join(ROOT, "tests", "golden", "leg_co2like.npz"))
    m = leg.LEGMatrices(*(torch.from_numpy(g[k]).to(torch.float64).cuda() for k in ("N", "R", "B", "Lambda")))
    t, _ = leg.co2_like_series(rows=502, seed=0)
    Rs, Os = leg.peg_precision((12 * (t - t.min())).cuda(), m.G)
    return "n=502 rank=5 fp64 S=1024", cr.decompose(Rs, Os), torch.zeros(502, 5, dtype=torch.float64, device="cuda"), 1024


def versions(dec, mean, S, seed=7):
    Dp, Fp, Gp = dec.packed
    N, d, dt, dev = Dp.shape[0], Dp.shape[-1], Dp.dtype, Dp.device
    lib, code = _hip.lib(), _hip.dtype_code(Dp.dtype)
    x = torch.empty(N, d, S, dtype=dt, device=dev)
    y = torch.empty(N, d, S, dtype=dt, device=dev)
    eps = torch.empty(N * d, S, dtype=dt, device=dev)
    ws_s, nb_s = _hip.sample_workspace(N, d, dt, S, dev)
    ws_s = ws_s.clone()                                     # (the cached scratch tensor is shared between ops)
    ws_b, nb_b = _hip.workspace(N, d, dt, _hip.OP_BACKSOLVE, dev, nrhs=S)
    mu = mean.unsqueeze(-1)

    def fused():
        _hip.check(lib.cgps_sample(_hip.ptr(Dp), _hip.ptr(Fp), _hip.ptr(Gp), N, d, code, S, _hip.ptr(mean), seed, 0,
                                   _hip.ptr(x), _hip.ptr(ws_s), nb_s, _hip.stream_ptr()))

    def back():
        _hip.check(lib.cgps_backsolve(_hip.ptr(Dp), _hip.ptr(Fp), _hip.ptr(Gp), N, d, code, S, _hip.ptr(eps), _hip.ptr(y),
                                      _hip.ptr(ws_b), nb_b, _hip.stream_ptr()))
        y.add_(mu)

    def unfused():
        _hip.check(lib.cgps_normal_fill(_hip.ptr(eps), N * d, S, code, seed, 0, _hip.stream_ptr()))
        back()

    def randn():
        torch.randn(eps.shape, dtype=dt, device=dev, out=eps)
        back()

    return {"fused": fused, "unfused": unfused, "randn": randn}, x, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile-only", action="store_true")
    a = ap.parse_args()
    res = []
    for case in (big_case, leg_case):
        name, dec, mean, S = case()
        fns, x, y = versions(dec, mean, S)
        if a.profile_only:
            for _ in range(a.rounds):
                fns["fused"]()
            torch.cuda.synchronize()
            continue
        # the fused call agrees with its definition before anything is timed
        fns["fused"]()
        fns["unfused"]()
        err = float(((x - y).abs() / (1.0 + y.abs())).max())
        assert err < 1e-9, err
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        a_ev, b_ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():                       # alternated: every round times every version once
                a_ev.record()
                fn()
                b_ev.record()
                b_ev.synchronize()
                times[k].append(a_ev.elapsed_time(b_ev) * 1e3)
        row = {"case": name, "rounds": a.rounds, "max_err_fused_vs_unfused": err}
        for k, t in times.items():
            q = np.percentile(t, [25, 50, 75])
            row[k + "_us"], row[k + "_q25_us"], row[k + "_q75_us"], row[k + "_min_us"] = float(q[1]), float(q[0]), float(q[2]), float(min(t))
        print(json.dumps(row), flush=True)
        res.append(row)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

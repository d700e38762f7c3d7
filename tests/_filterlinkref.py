"""The linking law of the time-parallel backward of the LEG filter, in torch on the CPU.

The reverse walk (reference (b), ``_filtergradref.filter_adjoint_ref``) is affine in the cotangent that its last row
receives.  Run over a chunk of rows [lo, hi) with ``init`` = the saved state of row lo - 1, it maps (mb, Db) on row hi - 1
to the adjoint of that saved state:
    mb_in = PhiT mb + cm ;    Db_in = PhiT Db PhiT^T + sum_j mb_j T[j] + cD
``chunk_maps`` measures (PhiT, T, cm, cD) with d + 1 runs of (b) itself, ``serial_link`` hands every chunk what the later
ones give it, one chunk after the other, and ``linked_adjoint`` runs (b) once more per chunk with that on its last row:
the whole backward of leg._filter_adjoint_linked with (b) in the place of cgps_leg_filter_adjoint and a serial loop in
the place of leg._filter_link_scan.  ``serial_compose`` is that loop on arbitrary elements, the reference of the scan."""
import torch

import _filtergradref as fg

F64 = torch.float64


def chunk_bounds(n, L):
    return [(lo, min(lo + L, n)) for lo in range(0, n, L)]


def per_row_cotangents(cot, n, d):
    """``cot`` of ``filter_adjoint_ref`` with loglik folded into logpdf and the end state's into the last row's z_mean, z_cov"""
    out = {k: (None if cot.get(k) is None else cot[k].detach().to(F64).clone()) for k in fg.KEYS}
    if cot.get("loglik") is not None:
        out["logpdf"] = (out["logpdf"] if out["logpdf"] is not None else torch.zeros(n, dtype=F64)) + cot["loglik"]
    for key, row, tail in (("state_mean", "z_mean", (d,)), ("state_cov", "z_cov", (d, d))):
        if cot.get(key) is not None:
            if out[row] is None:
                out[row] = torch.zeros((n,) + tail, dtype=F64)
            out[row][n - 1] += cot[key]
    return out


def run_chunk(ops, data, init, z_mean, z_cov, rows, lo, hi, recv):
    """(b) over the rows [lo, hi) from the saved state before them; ``rows``: per-row cotangents of the whole series or
    None (a probe), ``recv`` = (mb, Db) on the last row, either None."""
    ts, xs, s, mask = data
    start = init if lo == 0 else (ts[lo - 1], z_mean[lo - 1], z_cov[lo - 1])
    cot = {} if rows is None else {k: v[lo:hi] for k, v in rows.items() if v is not None}
    if recv[0] is not None:
        cot["state_mean"] = recv[0]
    if recv[1] is not None:
        cot["state_cov"] = recv[1]
    cut = lambda t: None if t is None else t[lo:hi]      # noqa: E731
    return fg.filter_adjoint_ref(*ops, ts[lo:hi], xs[lo:hi], cut(s), cut(mask), start, z_mean[lo:hi], z_cov[lo:hi], cot)


def chunk_maps(ops, data, init, z_mean, z_cov, rows, lo, hi):
    """(PhiT [d, d], T [d, d, d], cm [d], cD [d, d]) of the chunk [lo, hi)"""
    d = ops[0].shape[0]
    aff = run_chunk(ops, data, init, z_mean, z_cov, rows, lo, hi, (None, None))
    PhiT, T = torch.zeros(d, d, dtype=F64), torch.zeros(d, d, d, dtype=F64)
    for j in range(d):
        e = torch.zeros(d, dtype=F64)
        e[j] = 1.0
        probe = run_chunk(ops, data, init, z_mean, z_cov, None, lo, hi, (e, None))
        PhiT[:, j], T[j] = probe["m0"], probe["P0"]
    return PhiT, T, aff["m0"], aff["P0"]


def apply_map(el, mb, Db):
    PhiT, T, cm, cD = el
    return PhiT @ mb + cm, PhiT @ Db @ PhiT.T + torch.einsum("j,jab->ab", mb, T) + cD


def serial_link(maps):
    """What every chunk's last row receives: zero for the last chunk, and chunk c - 1 receives chunk c's map of what c does"""
    d = maps[0][2].shape[0]
    recv = [None] * len(maps)
    cur = (torch.zeros(d, dtype=F64), torch.zeros(d, d, dtype=F64))
    for c in range(len(maps) - 1, -1, -1):
        recv[c] = cur
        cur = apply_map(maps[c], *cur)
    return recv


def linked_adjoint(G, Bm, LLT, ts, xs, s, mask, init, z_mean, z_cov, cot, L):
    """The result of ``filter_adjoint_ref`` on the whole series, from runs over chunks of L rows linked as above"""
    n, d = xs.shape[0], G.shape[0]
    ops, data = (G, Bm, LLT), (ts, xs, s, mask)
    rows = per_row_cotangents(cot, n, d)
    bounds = chunk_bounds(n, L)
    recv = serial_link([chunk_maps(ops, data, init, z_mean, z_cov, rows, lo, hi) for lo, hi in bounds])
    parts = [run_chunk(ops, data, init, z_mean, z_cov, rows, lo, hi, r) for (lo, hi), r in zip(bounds, recv)]
    out = {k: sum(p[k] for p in parts) for k in ("G", "B", "LLT")}
    out.update({k: torch.cat([p[k] for p in parts]) for k in ("xs", "s", "gap")})
    out["m0"], out["P0"] = parts[0]["m0"], parts[0]["P0"]
    return out


def serial_compose(PhiT, T, cm, cD, series_chunks):
    """The reference of leg._filter_link_scan: per model and series, ``serial_link`` over its chunks.  PhiT [M, C, d, d],
    T [M, C, d, d, d], cm [M, C, d], cD [M, C, d, d], series_chunks a list of B + 1 ints."""
    rm, rD = torch.zeros_like(cm), torch.zeros_like(cD)
    for k in range(cm.shape[0]):
        for lo, hi in zip(series_chunks[:-1], series_chunks[1:]):
            recv = serial_link([(PhiT[k, c], T[k, c], cm[k, c], cD[k, c]) for c in range(lo, hi)])
            for c, (mb, Db) in zip(range(lo, hi), recv):
                rm[k, c], rD[k, c] = mb, Db
    return rm, rD

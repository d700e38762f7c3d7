"""The time-parallel filter of LEG series in torch, for any dtype: the five phases of
cgps_leg_filter_scan, one torch operation per lane's step.  tests/test_scanref.py holds it to ``_filterref.filter_ref``.

The element of rows j+1..i is (A, b, C, eta, J):  z_i | z_j, x_{j+1:i} ~ N(A z_j + b, C)  and the likelihood of
x_{j+1:i} as a function of z_j is proportional to exp(eta^T z_j - 1/2 z_j^T J z_j).  ``combine`` composes an earlier
with a later element, ``compose_row`` an element with the single row that follows it (only the obs x obs Cholesky),
``row_element`` is the element of one row.  A reset element (0, m, P, 0, 0) starts a series; combining with a reset on
the right SELECTS the right operand."""
import torch

import _filterref

F64 = torch.float64


def expm1_matrix(A):
    """exp(A) - I without the cancellation: Taylor from the first-order term on a scaled A, then F(2A) = 2 F + F F."""
    d = A.shape[0]
    nrm = float(A.abs().sum(1).max())
    s = 0
    while nrm > 0.25:
        nrm, s = nrm / 2, s + 1
    As = A / (2.0 ** s)
    term, F = As.clone(), As.clone()
    for k in range(2, 20):
        term = term @ As / k
        F = F + term
    for _ in range(s):
        F = 2 * F + F @ F
    return F if d else A


def gap_pair(G, gap):
    """(E, Q) of a gap: E = I + F, Q = I - E E^T = -(F + F^T + F F^T) with F = expm1(-1/2 gap G)."""
    F = expm1_matrix(-0.5 * gap * G)
    return torch.eye(G.shape[0], dtype=G.dtype) + F, -(F + F.T + F @ F.T)


def identity_element(d, dtype):
    z, I = torch.zeros(d, dtype=dtype), torch.eye(d, dtype=dtype)
    return (I, z, torch.zeros(d, d, dtype=dtype), z.clone(), torch.zeros(d, d, dtype=dtype))


def reset_element(m, P):
    d = m.shape[0]
    return (torch.zeros(d, d, dtype=m.dtype), m, P, torch.zeros(d, dtype=m.dtype), torch.zeros(d, d, dtype=m.dtype))


def row_element(E, Q, H, Cn, x):
    """The element of one row with gap (E, Q) that observes x = H z + N(0, Cn) (H with no rows: nothing observed)."""
    d = E.shape[0]
    if H.shape[0] == 0:
        return (E, torch.zeros(d, dtype=E.dtype), Q, torch.zeros(d, dtype=E.dtype), torch.zeros(d, d, dtype=E.dtype))
    T = torch.linalg.cholesky(H @ Q @ H.T + Cn)
    W = torch.linalg.solve_triangular(T, H, upper=False)
    r = torch.linalg.solve_triangular(T, x[:, None], upper=False)[:, 0]
    WE, QWt = W @ E, Q @ W.T
    return (E - QWt @ WE, QWt @ r, Q - QWt @ QWt.T, WE.T @ r, WE.T @ WE)


def combine(e1, e2, reset2=False):
    """The element of e1's rows followed by e2's.  ``reset2``: e2 starts a series -- the result IS e2."""
    if reset2:
        return e2
    A1, b1, C1, h1, J1 = e1
    A2, b2, C2, h2, J2 = e2
    d = A1.shape[0]
    K = torch.eye(d, dtype=A1.dtype) + C1 @ J2
    X = torch.linalg.solve(K, torch.cat([A1, (b1 + C1 @ h2)[:, None], C1], 1))     # LU with partial pivoting
    XA, xv, XC = X[:, :d], X[:, d], X[:, d + 1:]
    C = A2 @ XC @ A2.T + C2
    J = A1.T @ J2 @ XA + J1
    return (A2 @ XA, A2 @ xv + b2, 0.5 * (C + C.T), XA.T @ (h2 - J2 @ b1) + h1, 0.5 * (J + J.T))


def compose_row(e1, E, Q, H, Cn, x):
    """combine(e1, row_element(E, Q, H, Cn, x)) through the obs x obs factor alone."""
    A1, b1, C1, h1, J1 = e1
    Am, bm, Cm = E @ A1, E @ b1, E @ C1 @ E.T + Q
    if H.shape[0] == 0:
        return (Am, bm, Cm, h1, J1)
    T = torch.linalg.cholesky(H @ Cm @ H.T + Cn)
    sol = torch.linalg.solve_triangular(T, torch.cat([H @ Cm, H @ Am, (x - H @ bm)[:, None]], 1), upper=False)
    d = E.shape[0]
    W, U, r = sol[:, :d], sol[:, d:2 * d], sol[:, 2 * d]
    C = Cm - W.T @ W
    J = J1 + U.T @ U
    return (Am - W.T @ U, bm + W.T @ r, 0.5 * (C + C.T), h1 + U.T @ r, 0.5 * (J + J.T))


def chunk_layout(lengths, L):
    """[(series, first row, one past the last row)] of every chunk: ceil(n_b / L) chunks per series, restarting at
    every series' first row (rows are local to the series)."""
    return [(b, r, min(r + L, n)) for b, n in enumerate(lengths) for r in range(0, n, L)]


def scan_states(G, Bm, LLT, series, L, F):
    """Phases 1 to 3 over a list of series (ts, xs, s, mask, init) already in the working dtype: the state
    (t, mean, cov) every chunk starts from (None: the prior at the chunk's first row)."""
    d, dtype = G.shape[0], G.dtype
    chunks = chunk_layout([sr[0].shape[0] for sr in series], L)
    # 1. chunk summaries
    elems, flags = [], []
    for b, r0, r1 in chunks:
        ts, xs, s, mask, init = series[b]
        if r0 == 0:
            e = reset_element(*((torch.zeros(d, dtype=dtype), torch.eye(d, dtype=dtype)) if init is None else init[1:]))
            tprev = None if init is None else init[0]
        else:
            e, tprev = identity_element(d, dtype), ts[r0 - 1]
        for i in range(r0, r1):
            E, Q = gap_pair(G, ts[i] - tprev) if tprev is not None else (torch.eye(d, dtype=dtype), torch.zeros(d, d, dtype=dtype))
            o = mask[i].nonzero().flatten()
            e = compose_row(e, E, Q, Bm[o], LLT[o][:, o] + torch.diag(s[i, o]), xs[i, o])
            tprev = ts[i]
        elems.append(e)
        flags.append(r0 == 0)
    # 2. up-sweep: inclusive local prefixes in groups of F, the last one of a group goes up
    levels = [(elems, flags)]
    while len(levels[-1][0]) > F:
        el, fl = levels[-1]
        up_e, up_f = [], []
        for g in range(0, len(el), F):
            for j in range(g + 1, min(g + F, len(el))):
                el[j], fl[j] = combine(el[j - 1], el[j], fl[j]), fl[j - 1] or fl[j]
            up_e.append(el[min(g + F, len(el)) - 1])
            up_f.append(fl[min(g + F, len(el)) - 1])
        levels.append((up_e, up_f))
    el, fl = levels[-1]
    for j in range(1, len(el)):
        el[j], fl[j] = combine(el[j - 1], el[j], fl[j]), fl[j - 1] or fl[j]
    # 3. down-sweep: the completed prefix of the group before, applied to every local prefix
    for lv in range(len(levels) - 2, -1, -1):
        el, fl = levels[lv]
        up = levels[lv + 1][0]
        for j in range(F, len(el)):
            el[j] = combine(up[j // F - 1], el[j], fl[j])
    starts = []
    for c, (b, r0, r1) in enumerate(chunks):
        ts, init = series[b][0], series[b][4]
        starts.append(init if r0 == 0 else (ts[r0 - 1], elems[c - 1][1], elems[c - 1][2]))
    return chunks, starts


def scan_filter_ref(mats, series, L, F, dtype=F64):
    """The five phases over a list of series (ts [n], xs [n, obs], s or None, mask or None, init or None), evaluated in
    ``dtype`` on the CPU: a list of dicts with the keys of ``_filterref.filter_ref`` (loglik: the chunks' fp64 sums added
    in chunk order)."""
    Nm, Rm, Bm, Lm = (t.detach().to("cpu", dtype) for t in mats)
    d, obs = Nm.shape[0], Bm.shape[0]
    G = Nm @ Nm.T + Rm - Rm.T + 1e-5 * torch.eye(d, dtype=dtype)
    LLT = Lm @ Lm.T + 1e-9 * torch.eye(obs, dtype=dtype)
    ser = []
    for ts, xs, s, mask, init in series:
        n = xs.shape[0]
        ser.append((ts.to("cpu", dtype), xs.to("cpu", dtype),
                    torch.zeros(n, obs, dtype=dtype) if s is None else s.to("cpu", dtype),
                    torch.ones(n, obs, dtype=torch.bool) if mask is None else mask.cpu(),
                    None if init is None else tuple(t.to("cpu", dtype) for t in init)))
    chunks, starts = scan_states(G, Bm, LLT, ser, L, F)
    outs = [None] * len(ser)
    for (b, r0, r1), st in zip(chunks, starts):
        ts, xs, s, mask, _ = ser[b]
        # 4. the serial recursion over the chunk, from its exact start state
        o = _filterref.filter_ref(mats, ts[r0:r1], xs[r0:r1], s[r0:r1], mask[r0:r1], init=st, dtype=dtype)
        if outs[b] is None:
            outs[b] = o
        else:                                                    # 5. per series: chunk order
            for k in ("mean", "cov", "logpdf", "z_mean", "z_cov", "pre_mean"):
                outs[b][k] = torch.cat([outs[b][k], o[k]])
            outs[b]["loglik"] = outs[b]["loglik"] + o["loglik"]
            outs[b]["state"] = o["state"]
    return outs

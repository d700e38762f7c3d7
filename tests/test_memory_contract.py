"""The three promises include/cgps.h makes about memory, held on the device:

* the library never allocates: a workspace of EXACTLY the bytes the size query returns is enough (nothing is written
  past it, nothing before it);
* the workspace's contents are arbitrary before a call: no result depends on what the workspace, or anything outside
  an operand, held;
* outputs are written where the header says, all of them, and nowhere else.

How: tests/_arena.py places operands, outputs and workspaces inside one tensor, each between 64 KiB guards, and fills
guards, workspaces and outputs with 0xFF (NaN in both precisions, -1 as an int), then again with 0x00.  Every case
runs three times on the same operands -- the ordinary call, then the two poisoned ones -- and the results must be
``torch.equal``: the library sums in fixed orders without floating-point atomics, so bit equality is the bound.  An
element that is never stored keeps its poison and differs from the ordinary result under at least one of the two
bytes; a read outside an operand or of a workspace slot that was never written sees two different values in the two
runs.  The shapes come from the plans (tests/plan_cases.cpp), one case per kernel family and precision at least.

Alignment (part D): the header asks for 16-byte aligned arrays of blocks and vectors and refuses anything else with
CGPS_ERR_ARG before a launch; the Python wrappers copy a view that starts off the boundary.  No test hands the
library an address that is not inside real memory of its own."""
import contextlib
import functools
import os
import pathlib
import subprocess
import tempfile

import pytest
import torch

import _util
from _arena import Arena, GUARD, capacity_for
from cyclic_gps import _hip, leg, sharded
import cyclic_gps.cyclic_reduction as cr
from test_plan import _host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "cyclic-gps_amd", "csrc")
F32, F64 = torch.float32, torch.float64
POISONS = (0xFF, 0x00)
NRHS = (1, 2, 3, 9)
SAMPLES = (1, 9)
ERR_ARG = 1

# ---- the cases: (N, d, dtype) ----------------------------------------------------------------------------------------
# A first list (N in {1, 2, 3, 129, 257, 1025, 2049, 4097, 32769, 65537, 131073}) cut down to what tests/plan_cases.cpp says
# each size is there for (test_the_cases_cover_every_pass_kind):
#   N = 1, 2, 3: no coupling block, one elimination, the first system with a right neighbour only;
#   N = 257, 1025: stage-1 chunks of 4 and of 8 rows (chunk:4, chunk:8); 1025 is also the first size with a fused pass
#                  of inverse_blocks (inv:Tile, from 1024 rows);
#   N = 2049: chunks of one row again and the first size with more than one stage-1 workgroup (nine);
#   N = 129 and 4097 take no kind that 257 and 2049 do not: dropped;
#   N = 65409 = 511 * 128 + 1, d = 4: the smallest system whose first factorisation pass is a bulk pass that carries the
#                  right-hand side (dec:BulkRhs, 512 tiles); its decompose takes dec:Bulk, which is why 32769 (the
#                  smallest with dec:Bulk) is not here; also inv:Level next to inv:Deep;
#   N = 131073, d = 8, fp64: the smallest with a level-per-launch factorisation pass (dec:Level);
#   N = 524289, d = 1: the smallest with full 16-row stage-1 chunks (chunk:16) and, for a block size that has the
#                  latency-bound sweeps, with a regular sweep pass next to them.
SMALL_N = (1, 2, 3, 257, 1025, 2049)
BLOCKS = (1, 3, 4, 5, 6, 8)
CASES = ([(N, d, dt) for dt in (F64, F32) for N in SMALL_N for d in BLOCKS] +
         [(65409, 4, F64), (65409, 4, F32), (524289, 1, F64), (524289, 1, F32), (131073, 8, F64)])


def _case_id(c):
    return "N%d-d%d-%s" % (c[0], c[1], "fp64" if c[2] == F64 else "fp32")


# ---- every entry point of include/cgps.h: where this file runs it, or why it does not ----------------------------------
COVERED = {
    # workspace (B) and outputs / operands (C) together, test_core_entries_keep_the_memory_contract
    "cgps_mahal_logdet": "core", "cgps_mahal_logdet_levelwise": "core", "cgps_decompose": "core",
    "cgps_decompose_solve": "core", "cgps_halfsolve": "core", "cgps_backsolve": "core", "cgps_solve": "core",
    "cgps_logdet_factor": "core", "cgps_inverse_blocks": "core", "cgps_sample": "core",
    "cgps_decompose_step": "core", "cgps_mahal_logdet_adjoint": "core", "cgps_normal_fill": "core",
    "cgps_leg_mahal_logdet": "leg_fused", "cgps_leg_mahal_logdet_pair": "leg_fused",
    "cgps_leg_mahal_logdet_pair_obs": "leg_fused", "cgps_leg_mahal_logdet_pair_w": "leg_fused",
    "cgps_peg_precision": "leg_fused",
    "cgps_shard_reduce": "sharded", "cgps_finish_records": "sharded",
    "cgps_mahal_logdet_batch": "batch", "cgps_mahal_logdet_adjoint_seg": "batch",
    # the per-row LEG entry points, test_per_row_leg_entries_keep_the_memory_contract
    "cgps_peg_precision_adjoint": "rows",
    "cgps_peg_precision_seg": "rows",
    "cgps_peg_precision_adjoint_seg": "rows",
    "cgps_peg_precision_models": "rows",
    "cgps_peg_precision_adjoint_models": "rows",
    "cgps_leg_posterior_blocks_seg": "rows",
    "cgps_leg_posterior_blocks_models": "rows",
    "cgps_leg_intercast": "rows",
    "cgps_leg_intercast_seg": "rows",
    "cgps_leg_intercast_models": "rows",
    "cgps_leg_perturbation_seg": "rows",
    "cgps_leg_perturbation_models": "rows",
    "cgps_leg_observations": "rows",
    "cgps_leg_loo": "rows",
    "cgps_leg_filter": "rows",
    "cgps_leg_filter_scan": "rows",
    "cgps_leg_filter_adjoint": "rows",
    "cgps_leg_loglik_batch": "rows",
    "cgps_leg_loglik_batch_obs": "rows",
    "cgps_leg_loglik_batch_w": "rows",
    "cgps_leg_loglik_models": "rows",
    "cgps_leg_loglik_models_obs": "rows",
    "cgps_leg_loglik_models_w": "rows",
}
EXCEPTIONS = {
    "cgps_version": "no memory", "cgps_last_error": "no device memory",
    "cgps_level_layout": "host arithmetic", "cgps_workspace_bytes": "host arithmetic",
    "cgps_solve_workspace_bytes": "host arithmetic", "cgps_sample_workspace_bytes": "host arithmetic",
    "cgps_leg_filter_scan_workspace_bytes": "host arithmetic", "cgps_leg_filter_adjoint_workspace_bytes": "host arithmetic",
    "cgps_record_elems": "host arithmetic", "cgps_profile_next_call": "host state only", "cgps_reset_counters": "library-owned counters",
    "cgps_boundary_solve": "boundary helper", "cgps_boundary_recursions": "boundary helper",
}


def test_every_entry_point_is_covered_or_named():
    have = set(_hip.exported_symbols())
    named = set(COVERED) | set(EXCEPTIONS)
    assert not (set(COVERED) & set(EXCEPTIONS))
    assert have - named == set(), "entry points without a memory-contract case: %s" % sorted(have - named)
    assert named - have == set(), "names that are no entry points: %s" % sorted(named - have)


# ---- CPU: the shapes come from the plan --------------------------------------------------------------------------------
def _build(tmp_path, source, compiler, flags=()):
    exe = str(tmp_path / os.path.splitext(source)[0])
    subprocess.run(compiler + ["-std=c++17", "-O1", "-I", CSRC, *flags, os.path.join(HERE, source), "-o", exe], check=True)
    return exe


def _kinds(line):
    head, _, toks = line.partition("|")
    return head.split(), set(toks.split())


def test_the_cases_cover_every_pass_kind(tmp_path):
    """tests/plan_cases.cpp (host-only, cgps_plan.h alone) prints the kinds each case takes and, per precision, every
    kind any (N, d, nrhs) takes.  The case list must take them all: a kind added to the header later fails here until
    a case runs it.  Printed: the coverage table of DESIGN.md 3.2."""
    exe = _build(tmp_path, "plan_cases.cpp", _host_compiler(), ["-Wall"])
    args = ["%d,%d,%d,%d" % (N, d, 8 if dt == F64 else 4, m) for N, d, dt in CASES for m in NRHS]
    out = subprocess.run([exe, "--reachable"] + args, capture_output=True, text=True, check=True, timeout=300).stdout
    reachable, taken, first = {}, {4: set(), 8: set()}, {4: {}, 8: {}}
    for line in out.splitlines():
        head, kinds = _kinds(line)
        if head[0] == "reachable":
            reachable[int(head[1])] = kinds
        else:
            N, d, s = int(head[1]), int(head[2]), int(head[3])
            taken[s] |= kinds
            for k in kinds:
                first[s].setdefault(k, (N, d))
    assert set(reachable) == {4, 8}
    for s in (4, 8):
        print("scalar size %d: %s" % (s, ", ".join("%s (N %d d %d)" % (k, *first[s][k]) for k in sorted(first[s]))))
        assert reachable[s] - taken[s] == set(), "scalar size %d: no case takes %s" % (s, sorted(reachable[s] - taken[s]))
        assert taken[s] - reachable[s] == set()
    # the header's enums, so that a new enumerator cannot hide behind an old name in plan_cases.cpp
    plan = open(os.path.join(CSRC, "cgps_plan.h")).read()
    assert "enum class DecKind { Level, Bulk, BulkRhs, Lds };" in plan and "enum class InvKind { Deep, Tile, Level };" in plan
    assert {"dec:Level", "dec:Bulk", "dec:BulkRhs", "dec:Lds", "inv:Deep", "inv:Tile", "inv:Level"} <= reachable[8]
    # every case is there for a kind: each large one is the only one of its precision with the kind it was chosen for
    for N, d, dt, kind in [(65409, 4, F64, "dec:BulkRhs"), (65409, 4, F32, "dec:BulkRhs"), (524289, 1, F64, "chunk:16"),
                           (524289, 1, F32, "chunk:16"), (131073, 8, F64, "dec:Level")]:
        assert first[8 if dt == F64 else 4][kind] == (N, d), (kind, first[8 if dt == F64 else 4][kind])


def test_the_alignment_helper_alone(tmp_path):
    """check_alignment / misaligned of csrc/cgps_host.h as a stand-alone program (tests/align_check.cpp): built with hipcc
    (the header includes the HIP runtime's), run without a GPU; it touches no device."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = _build(tmp_path, "align_check.cpp", [hipcc, "-x", "hip", "--offload-arch=gfx950"], ["-Wno-unused-value"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "align_check: 0 failed" in r.stdout, r.stdout + r.stderr


# ---- the three runs ----------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _recording_scratch():
    """the ordinary call, with the workspace sizes it asks for written down (the arena of the poisoned runs is sized
    from them); the cached, grow-only buffers are what it gets, as always"""
    sizes, real = [], _hip._scratch

    def scratch(cache, nbytes, device):
        sizes.append(int(nbytes))
        return real(cache, nbytes, device)
    _hip._scratch = scratch
    try:
        yield sizes
    finally:
        _hip._scratch = real


def _flat(v):
    if isinstance(v, torch.Tensor):
        return [v]
    out = []
    for t in v:
        out += _flat(t)
    return out


def _bits(x):
    return x.contiguous().reshape(-1).view(torch.uint8)


def _assert_same(ref, got, what):
    assert list(ref) == list(got), (list(ref), list(got))
    bad = []
    for name in ref:
        a, b = _flat(ref[name]), _flat(got[name])
        assert len(a) == len(b), (name, len(a), len(b))
        for i, (x, y) in enumerate(zip(a, b)):
            assert x.shape == y.shape and x.dtype == y.dtype, (name, i, x.shape, y.shape)
            if not torch.equal(x, y) and not torch.equal(_bits(x), _bits(y)):      # (the same NaN is the same result)
                diff = (_bits(x) != _bits(y)).reshape(x.numel(), -1).any(-1)
                idx = torch.nonzero(diff.reshape(-1)).flatten()
                bad.append("%s[%d]: %d of %d elements differ, first at flat index %d (%r against %r)"
                           % (name, i, idx.numel(), x.numel(), int(idx[0]), x.reshape(-1)[idx[0]].item(), y.reshape(-1)[idx[0]].item()))
    assert not bad, "%s: %s" % (what, "; ".join(bad[:6]))


def _still_poison(t, byte):
    """every byte of t (a view into an arena) is still the poison"""
    return t.numel() == 0 or bool((t.contiguous().view(torch.uint8) == byte).all())


def _three_runs(fn, inputs, out_bytes, what):
    """fn(inputs, arena or None) -> ({name: tensors}, [tensors that must NOT have been written]).  (i) the ordinary call;
    (ii), (iii): operands placed in an arena, outputs allocated there and workspaces of exactly the size asked for,
    everything that is not an operand poisoned 0xFF, then 0x00.  Results equal bit for bit, guards intact, the
    unwritten tensors still poison.  Returns the ordinary results."""
    with _recording_scratch() as sizes:
        ref, _ = fn(inputs, None)
    torch.cuda.synchronize()
    in_bytes = [v.numel() * v.element_size() for v in inputs.values() if v is not None]
    for byte in POISONS:
        arena = Arena(capacity_for(sizes + in_bytes) + int(out_bytes))
        arena.poison(byte)                                        # (no view yet: the whole arena)
        placed = {k: (None if v is None else arena.put(v, k)) for k, v in inputs.items()}
        with arena.exact_scratch(_hip), arena.route_allocations():
            got, untouched = fn(placed, arena)
        torch.cuda.synchronize()
        tag = "%s, poison 0x%02X" % (what, byte)
        assert [v.numel() for v in arena.scratch] == sizes, (tag, [v.numel() for v in arena.scratch], sizes)
        for k, v in inputs.items():                               # the operands are operands: never written
            if v is not None:
                assert torch.equal(placed[k], v), "%s: operand %s was written" % (tag, k)
        arena.assert_guards(byte)
        _assert_same(ref, got, tag)
        for i, t in enumerate(untouched):
            assert _still_poison(t, byte), "%s: tensor %d that the header leaves unwritten was written" % (tag, i)
        del arena, placed, got
    return ref


def _out_bytes(n_allocs, payload):
    """room for the wrappers' own allocations: `payload` bytes in `n_allocs` tensors, each between guards"""
    return int(payload) + n_allocs * (GUARD + 1024)


# ---- B + C: the factorisation, the solves, the inverse, sampling ------------------------------------------------------------
def _core_ops(t, arena):
    """every entry point that works on one system, through the wrappers of cyclic_reduction.py"""
    Rs, Os, x, ys, xc = t["Rs"], t["Os"], t["x"], [t["y%d" % m] for m in NRHS], t["xcrr"]
    N, d = Rs.shape[0], Rs.shape[1]
    _, offD, offF, offG = _hip.level_layout(N)
    out, untouched = {}, []

    def label(s):
        if arena is not None:
            arena.label = s

    def factor(dec):
        Dp, Fp, Gp = dec.packed
        untouched.extend([Fp[offF[-1]:], Gp[offG[-1]:]])          # "allocate N blocks for each": the tails belong to nobody
        return [Dp, Fp[:offF[-1]], Gp[:offG[-1]]]
    label("mahal_and_det")
    out["mahal_and_det"] = list(cr._mahal_and_det(Rs, Os, x, levelwise=False))
    label("mahal_and_det levelwise")
    out["levelwise"] = list(cr._mahal_and_det(Rs, Os, x, levelwise=True))
    label("decompose")
    dec = cr._decompose_raw(Rs, Os)
    out["decompose"] = factor(dec)
    label("decompose_solve")
    dec2, xs = cr.decompose_solve(Rs, Os, x)
    out["decompose_solve"] = factor(dec2) + [xs]
    if N >= 2:
        label("decompose_step")
        (_, D1, F1, G1), (Rn, On) = cr.decompose_step(Rs, Os)
        out["decompose_step"] = [D1, F1, G1, Rn, On]
    for m, y in zip(NRHS, ys):
        label("halfsolve nrhs %d" % m)
        out["halfsolve%d" % m] = cr.halfsolve(dec, y)
        label("backsolve nrhs %d" % m)
        out["backsolve%d" % m] = cr.backhalfsolve(dec, [xc[offD[i]:offD[i + 1]] for i in range(len(offD) - 1)]
                                                  if m == 1 else out["halfsolve%d" % m])
        label("solve nrhs %d" % m)
        out["solve%d" % m] = cr.solve(dec, y)
    label("mahal (halfsolve with its norm)")
    out["mahal"] = cr.mahal(dec, x)
    label("det")
    out["det"] = cr.det(dec)
    label("inverse_blocks")
    Sd, So = cr.inverse_blocks(dec)
    out["inverse_blocks"] = [Sd.clone(), So.clone()]
    label("mahal_logdet_adjoint")                                 # in place on Sd, So; no workspace
    g2 = t["g2"]
    _hip.check(_hip.lib().cgps_mahal_logdet_adjoint(_hip.ptr(Sd), _hip.ptr(So), _hip.ptr(x), N, d, _hip.dtype_code(Rs.dtype),
                                                    _hip.ptr(g2[0:1]), _hip.ptr(g2[1:2]), _hip.stream_ptr()))
    out["mahal_logdet_adjoint"] = [Sd, So]
    for S in SAMPLES:
        label("sample %d" % S)
        out["sample%d" % S] = cr.sample(dec, S, seed=20 + S, mean=x)
    label("normal_fill")
    out["normal_fill"] = cr.standard_normal(N * d, 3, seed=5, stream=2, dtype=Rs.dtype)
    return out, untouched


def _system(N, d, dt, seed=3):
    Rs, Os, b, _, _ = _util.conditioned_system(N, d, dtype=dt, seed=seed + N + d, device="cuda")
    return Rs.contiguous(), Os.contiguous(), b.contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_core_entries_keep_the_memory_contract(case):
    N, d, dt = case
    Rs, Os, x = _system(N, d, dt)
    gen = torch.Generator(device="cuda").manual_seed(N + d)
    inputs = {"Rs": Rs, "Os": Os, "x": x, "xcrr": torch.randn(N, d, dtype=dt, device="cuda", generator=gen),
              "g2": torch.tensor([0.7, -1.3], dtype=dt, device="cuda")}
    for m in NRHS:
        inputs["y%d" % m] = torch.randn((N, d) if m == 1 else (N, d, m), dtype=dt, device="cuda", generator=gen)
    es = 4 if dt == F32 else 8
    payload = (12 * N * d * d + (3 * sum(NRHS) + sum(SAMPLES) + 12) * N * d) * es
    _three_runs(_core_ops, inputs, _out_bytes(160, 1.1 * payload), _case_id(case))


# ---- B + C: the fused LEG reductions and the assembly they replace -------------------------------------------------------
def _leg_model(d, dt, seed, P=3, Kb=2):
    gen = torch.Generator().manual_seed(seed)
    Nm = torch.tril(0.4 * torch.randn(d, d, generator=gen, dtype=F64), -1) + torch.diag(0.8 + 0.4 * torch.rand(d, generator=gen, dtype=F64))
    Rm = torch.tril(0.3 * torch.randn(d, d, generator=gen, dtype=F64), -1)
    G = Nm @ Nm.T + Rm - Rm.T + 1e-5 * torch.eye(d, dtype=F64)
    Bs = torch.randn(P, d, 2, generator=gen, dtype=F64)
    table = 0.5 * Bs @ Bs.transpose(-1, -2)
    table[0] = 0
    Cs = torch.randn(Kb, d, 2, generator=gen, dtype=F64)
    basis = 0.5 * Cs @ Cs.transpose(-1, -2)
    return G.to(dt).cuda(), table.to(dt).cuda(), basis.to(dt).cuda(), gen


def _leg_ops(t, arena):
    ts, G, table, basis, pattern, weights, v = (t[k] for k in ("ts", "G", "table", "basis", "pattern", "weights", "v"))
    out = {}

    def label(s):
        if arena is not None:
            arena.label = s
    label("peg_precision")
    out["peg_precision"] = list(leg._peg_precision_hip(ts, G))
    label("leg_mahal_logdet")
    out["leg_mahal_logdet"] = list(leg.leg_mahal_and_det(ts, G, table[1], v))
    for name, args in (("pair", (_hip.ROWS_PLAIN, table[2], None)), ("pair_obs", (_hip.ROWS_TABLE, table, pattern)),
                       ("pair_w", (_hip.ROWS_WEIGHTED, basis, weights))):
        label(name)
        out[name] = list(leg._leg_pair_raw(ts, G, args[0], args[1], args[2], v))
    return out, []


LEG_CASES = [(N, d, dt) for N, d, dt in CASES if d <= 7 and not (d == 6 and dt == F64)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", LEG_CASES, ids=_case_id)
def test_fused_leg_reductions_keep_the_memory_contract(case):
    N, d, dt = case
    G, table, basis, gen = _leg_model(d, dt, 50 + d)
    ts = torch.cumsum(0.2 + torch.rand(N, generator=gen, dtype=F64), 0).to(dt).cuda()
    inputs = {"ts": ts, "G": G, "table": table, "basis": basis,
              "pattern": torch.randint(0, 3, (N,), generator=gen).to(torch.uint8).cuda(),
              "weights": torch.rand(N, 2, generator=gen, dtype=F64).to(dt).cuda(),
              "v": torch.randn(N, d, generator=gen, dtype=F64).to(dt).cuda()}
    es = 4 if dt == F32 else 8
    _three_runs(_leg_ops, inputs, _out_bytes(40, 2.2 * N * d * d * es), _case_id(case))


# ---- B + C: many systems in one launch ----------------------------------------------------------------------------------
RAGGED = [1, 2, 7, 0, 64, 65]


def _batch_ops(t, arena):
    Rs, Os, x, off, seg, gm, gl = (t[k] for k in ("Rs", "Os", "x", "offsets", "seg", "gm", "gl"))
    R, d, B, dtc = Rs.shape[0], Rs.shape[1], off.numel() - 1, _hip.dtype_code(Rs.dtype)
    out, untouched = {}, []
    for packed in (0, 1):
        # os_packed = 1 reads Os as [B][n - 1]: the same arrays as three systems of two rows each
        o = t["offsets_dense"] if packed else off
        nb = o.numel() - 1
        for max_rows, name in ((4096, "batch%d" % packed), (3, "batch%d_short" % packed)):
            res = torch.empty(nb, 2, dtype=F64, device=Rs.device)
            info = torch.empty(nb, dtype=torch.int32, device=Rs.device)
            _hip.check(_hip.lib().cgps_mahal_logdet_batch(_hip.ptr(Rs), _hip.ptr(Os), _hip.ptr(x), _hip.ptr(o), nb, packed, d, dtc,
                                                          max_rows, _hip.ptr(res), _hip.ptr(info), _hip.stream_ptr()))
            lens = (o[1:] - o[:-1]).tolist()
            keep = [b for b, n in enumerate(lens) if 1 <= n <= max_rows]
            skip = [b for b, n in enumerate(lens) if not 1 <= n <= max_rows]
            out[name] = [res[keep], info[keep]]
            if arena is not None:                                 # "nothing of its slot is written"
                untouched.extend([res[skip], info[skip]])
    Sd, So = t["Sd"].clone(), t["So"].clone()
    if arena is not None:
        Sd, So = arena.put(Sd, "Sd in place"), arena.put(So, "So in place")
    _hip.check(_hip.lib().cgps_mahal_logdet_adjoint_seg(_hip.ptr(Sd), _hip.ptr(So), _hip.ptr(x), _hip.ptr(seg), R, B, d, dtc,
                                                        _hip.ptr(gm), _hip.ptr(gl), _hip.stream_ptr()))
    out["adjoint_seg"] = [Sd, So]
    return out, untouched


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("d", [1, 3, 5, 7])
def test_batched_systems_keep_the_memory_contract(d, dt):
    """cgps_mahal_logdet_batch, both layouts of Os, with a series longer than max_rows and an empty one (their slots
    keep the poison), and cgps_mahal_logdet_adjoint_seg in place.  d = 8 and fp64 d = 6 are CGPS_ERR_UNSUPPORTED."""
    R = sum(RAGGED)
    Rs, Os, x = _system(R, d, dt)
    off = [0]
    for n in RAGGED:
        off.append(off[-1] + n)
    gen = torch.Generator(device="cuda").manual_seed(d)
    B = len(RAGGED)
    inputs = {"Rs": Rs, "Os": Os, "x": x, "offsets": torch.tensor(off, dtype=torch.int64).cuda(),
              "offsets_dense": torch.arange(0, 8, 2, dtype=torch.int64).cuda(),
              "seg": torch.repeat_interleave(torch.arange(B, dtype=torch.int32), torch.tensor(RAGGED)).cuda(),
              "gm": torch.randn(B, dtype=dt, device="cuda", generator=gen), "gl": torch.randn(B, dtype=dt, device="cuda", generator=gen),
              "Sd": torch.randn(R, d, d, dtype=dt, device="cuda", generator=gen),
              "So": torch.randn(R - 1, d, d, dtype=dt, device="cuda", generator=gen)}
    _three_runs(_batch_ops, inputs, _out_bytes(24, 4 * R * d * d * 8), "batch d %d" % d)


# ---- B: two ranks played on one GPU ------------------------------------------------------------------------------------------
def _shard_ops(t, arena):
    Rs, Os, x = t["Rs"], t["Os"], t["x"]
    n, d, parts = Rs.shape[0], Rs.shape[1], 2
    bounds = [sharded.shard_bounds(n, parts, r) for r in range(parts)]
    rec_bytes, msg_bytes = sharded.message_layout(d, Rs.dtype)
    recv = torch.zeros(parts * msg_bytes, dtype=torch.uint8, device=Rs.device)
    for r, (lo, hi) in enumerate(bounds):
        ops = sharded.HipShardOps(hi - lo, d, Rs.dtype, Rs.device)
        ops.shard_reduce(Rs[lo:hi], Os[lo:hi - 1], x[lo:hi], None if lo == 0 else Os[lo - 1], recv[r * msg_bytes:(r + 1) * msg_bytes],
                         rec_bytes)
    out = torch.empty(2, dtype=F64, device=Rs.device)
    ops.finish(recv, parts, rec_bytes, msg_bytes, bounds[0][1] - bounds[0][0], n, out)
    used = (3 * d * d + 2 * d) * Rs.element_size()                # (the rest of a record's stride is padding)
    return {"records": [recv[r * msg_bytes:r * msg_bytes + used] for r in range(parts)],
            "partials": [recv[r * msg_bytes + rec_bytes:r * msg_bytes + rec_bytes + 24] for r in range(parts)],
            "finish": [out, ops.info]}, []


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("n,d", [(300, 4), (5000, 3), (5000, 8)])
def test_shard_reduce_and_finish_keep_the_memory_contract(n, d, dt):
    Rs, Os, x = _system(n, d, dt)
    _three_runs(_shard_ops, {"Rs": Rs, "Os": Os, "x": x}, _out_bytes(12, 4096), "shards n %d d %d" % (n, d))


# ---- B: one byte short is an argument error and nothing is touched ------------------------------------------------------------
def _short_calls(a, N, d, dt, nrhs, S):
    """{entry: (bytes the header asks for, call(ws_bytes))} on operands and outputs inside the arena `a`"""
    lib, dtc, st = _hip.lib(), _hip.dtype_code(dt), _hip.stream_ptr()
    P = lambda t: _hip.ptr(t)                                     # noqa: E731
    Rs, Os, x = (a.put(t, n) for t, n in zip(_system(N, d, dt), ("Rs", "Os", "x")))
    fac = [a.put(torch.rand(N, d, d, dtype=dt, device="cuda") + 2 * torch.eye(d, dtype=dt, device="cuda"), "factor%d" % i) for i in range(3)]
    Y = a.put(torch.randn(N, d, nrhs, dtype=dt, device="cuda"), "Y")
    G, table, basis, gen = _leg_model(d, dt, 9)
    G, table, basis = a.put(G, "G"), a.put(table, "table"), a.put(basis, "basis")
    ts = a.put(torch.arange(N, dtype=dt, device="cuda"), "ts")
    pattern = a.put(torch.zeros(N, dtype=torch.uint8, device="cuda"), "pattern")
    weights = a.put(torch.ones(N, 2, dtype=dt, device="cuda"), "weights")
    o = {k: a.empty(shape, dt, k) for k, shape in (("Dp", (N, d, d)), ("Fp", (N, d, d)), ("Gp", (N, d, d)), ("xcrr", (N, d)),
                                                     ("xo", (N, d)), ("Xo", (N, d, nrhs)), ("Sd", (N, d, d)), ("So", (N - 1, d, d)),
                                                     ("xs", (N, d, S)), ("record", (cr_record_elems(d, dt),)))}
    out4, info2 = a.empty((4,), F64, "out4"), a.empty((2,), torch.int32, "info2")
    wsb = lambda op, m=1: _hip._workspace_bytes(N, d, dtc, op, m)       # noqa: E731
    pair = _hip.pair_workspace_bytes(N, d, dt)
    calls = {
        "cgps_mahal_logdet": (wsb(_hip.OP_MAHAL_LOGDET), lambda w, b: lib.cgps_mahal_logdet(P(Rs), P(Os), P(x), N, d, dtc, w, b, P(out4), P(info2), st)),
        "cgps_mahal_logdet_levelwise": (wsb(_hip.OP_MAHAL_LOGDET_LEVELWISE), lambda w, b: lib.cgps_mahal_logdet_levelwise(P(Rs), P(Os), P(x), N, d, dtc, w, b, P(out4), P(info2), st)),
        "cgps_decompose": (wsb(_hip.OP_DECOMPOSE), lambda w, b: lib.cgps_decompose(P(Rs), P(Os), N, d, dtc, P(o["Dp"]), P(o["Fp"]), P(o["Gp"]), w, b, P(info2), st)),
        "cgps_decompose_solve": (wsb(_hip.OP_DECOMPOSE_SOLVE), lambda w, b: lib.cgps_decompose_solve(P(Rs), P(Os), P(x), N, d, dtc, P(o["Dp"]), P(o["Fp"]), P(o["Gp"]), P(o["xcrr"]), P(o["xo"]), w, b, P(info2), st)),
        "cgps_logdet_factor": (wsb(_hip.OP_LOGDET_FACTOR), lambda w, b: lib.cgps_logdet_factor(P(fac[0]), N, d, dtc, w, b, P(out4), st)),
        "cgps_inverse_blocks": (wsb(_hip.OP_INVERSE_BLOCKS), lambda w, b: lib.cgps_inverse_blocks(P(fac[0]), P(fac[1]), P(fac[2]), N, d, dtc, P(o["Sd"]), P(o["So"]), w, b, st)),
        "cgps_sample": (_hip._sample_workspace_bytes(N, d, dtc, S), lambda w, b: lib.cgps_sample(P(fac[0]), P(fac[1]), P(fac[2]), N, d, dtc, S, P(x), 1, 0, P(o["xs"]), w, b, st)),
        "cgps_shard_reduce": (wsb(_hip.OP_MAHAL_LOGDET), lambda w, b: lib.cgps_shard_reduce(P(Rs), P(Os), P(x), None, N, d, dtc, w, b, P(o["record"]), P(out4), st)),
    }
    for m, y, xo in ((1, x, o["xo"]), (nrhs, Y, o["Xo"])):
        calls["cgps_halfsolve nrhs %d" % m] = (wsb(_hip.OP_HALFSOLVE, m), lambda w, b, m=m, y=y, xo=xo: lib.cgps_halfsolve(P(fac[0]), P(fac[1]), P(fac[2]), N, d, dtc, m, P(y), P(xo), w, b, P(out4), st))
        calls["cgps_backsolve nrhs %d" % m] = (wsb(_hip.OP_BACKSOLVE, m), lambda w, b, m=m, y=y, xo=xo: lib.cgps_backsolve(P(fac[0]), P(fac[1]), P(fac[2]), N, d, dtc, m, P(y), P(xo), w, b, st))
        calls["cgps_solve nrhs %d" % m] = (wsb(_hip.OP_SOLVE, m), lambda w, b, m=m, y=y, xo=xo: lib.cgps_solve(P(fac[0]), P(fac[1]), P(fac[2]), N, d, dtc, m, P(y), P(xo), w, b, st))
    if d <= 7 and not (d == 6 and dt == F64):
        calls.update({
            "cgps_leg_mahal_logdet": (wsb(_hip.OP_MAHAL_LOGDET), lambda w, b: lib.cgps_leg_mahal_logdet(P(ts), P(G), P(table), P(x), N, d, dtc, w, b, P(out4), P(info2), st)),
            "cgps_leg_mahal_logdet_pair": (pair, lambda w, b: lib.cgps_leg_mahal_logdet_pair(P(ts), P(G), P(table), P(x), N, d, dtc, w, b, P(out4), P(info2), st)),
            "cgps_leg_mahal_logdet_pair_obs": (pair, lambda w, b: lib.cgps_leg_mahal_logdet_pair_obs(P(ts), P(G), P(table), 3, P(pattern), P(x), N, d, dtc, w, b, P(out4), P(info2), st)),
            "cgps_leg_mahal_logdet_pair_w": (pair, lambda w, b: lib.cgps_leg_mahal_logdet_pair_w(P(ts), P(G), P(basis), 2, P(weights), P(x), N, d, dtc, w, b, P(out4), P(info2), st)),
        })
    return calls


def cr_record_elems(d, dt):
    return sharded.record_elems(d, dt)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("N,d", [(3, 1), (257, 3), (2049, 4), (257, 5), (1025, 6), (1025, 8)])
def test_a_workspace_one_byte_short_is_an_argument_error(N, d, dt):
    """ws_bytes = need - 1 on real memory (the workspace view itself has all `need` bytes): CGPS_ERR_ARG, and not one
    byte of the arena -- operands, 0xFF outputs, workspace, guards -- has changed.  `need` bytes are accepted."""
    a = Arena(64 << 20)
    a.poison(0xFF)
    calls = _short_calls(a, N, d, dt, nrhs=3, S=9)
    ws = {name: a.place(need, "ws " + name) for name, (need, _) in calls.items()}
    before = a.buf.clone()
    for name, (need, call) in calls.items():
        assert need > 0 and ws[name].numel() == need
        rc = call(_hip.ptr(ws[name]), need - 1)
        torch.cuda.synchronize()
        assert rc == ERR_ARG, (name, rc, need)
        assert b"workspace" in _hip.lib().cgps_last_error(), (name, _hip.lib().cgps_last_error())
        assert torch.equal(a.buf, before), "%s: memory changed although the call was refused" % name
    for name, (need, call) in calls.items():                    # the exact size is enough (guards: checked at the end)
        assert call(_hip.ptr(ws[name]), need) == 0, (name, _hip.lib().cgps_last_error())
    torch.cuda.synchronize()
    a.assert_guards(0xFF)


# ---- D: alignment ------------------------------------------------------------------------------------------------------------
def _off_boundary(*ts):
    return all(t.data_ptr() % 16 != 0 for t in ts)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("d", [1, 3, 5])
def test_views_off_the_16_byte_boundary_give_the_results_of_their_clones(d, dt):
    """Rs[1:], Os[1:], x[1:] of a 258-row system: contiguous, and one odd-sized row off the boundary the header asks for.
    The wrappers copy such a view; the results are those of the same calls on clones, bit for bit."""
    N = 257
    Rf, Of, xf = _system(N + 1, d, dt)
    Rv, Ov, xv = Rf[1:], Of[1:], xf[1:]
    assert Rv.is_contiguous() and Ov.is_contiguous() and xv.is_contiguous() and _off_boundary(Rv, Ov, xv)
    Rc, Oc, xc = Rv.clone(), Ov.clone(), xv.clone()
    assert not _off_boundary(Rc) and not _off_boundary(Oc) and not _off_boundary(xc)

    _, _, offF, offG = _hip.level_layout(N)

    def run(R, O, x):
        out = {"mahal_and_det": list(cr.mahal_and_det(R, O, x))}
        dec = cr.decompose(R, O)
        out["decompose"] = [dec.packed[0], dec.packed[1][:offF[-1]], dec.packed[2][:offG[-1]]]
        out["solve"] = cr.solve(dec, x)
        out["inverse_blocks"] = list(cr.inverse_blocks(dec))
        out["decompose_solve"] = cr.decompose_solve(R, O, x)[1]
        return out
    _assert_same(run(Rc, Oc, xc), run(Rv, Ov, xv), "views d %d" % d)
    # a factor handed in as plain lists of views (no packed buffers) and a right-hand side off the boundary
    dec = cr.decompose(Rc, Oc)
    Yf = torch.randn(N + 1, d, 3, dtype=dt, device="cuda")
    assert _off_boundary(Yf[1:])
    _assert_same({"solve": cr.solve(dec, Yf[1:].clone())}, {"solve": cr.solve(dec, Yf[1:])}, "right-hand side d %d" % d)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("d", [1, 3, 5])
def test_sub_shards_at_an_odd_split_equal_cloned_shards(d, dt):
    """ShardedMahalLogdet(sub_shards=2) on 258 rows cuts at row 129: the second sub-shard's views start off the boundary.
    Against two ranks that each own a clone of their rows (played one after the other through an injected gather)."""
    n = 258
    Rs, Os, x = _system(n, d, dt)
    one = sharded.ShardedMahalLogdet(Rs, Os, x, None, n, 0, 1, sub_shards=2)
    sub = one.subs[1]
    assert _off_boundary(sub["Rs"], sub["x"]) and sub["Rs"].shape[0] == 129
    got = one.run().clone()
    sends, plans = [], []
    for r in range(2):
        lo, hi = sharded.shard_bounds(n, 2, r)
        pl = sharded.ShardedMahalLogdet(Rs[lo:hi].clone(), Os[lo:hi - 1].clone(), x[lo:hi].clone(),
                                        None if r == 0 else Os[lo - 1].clone(), n, r, 2,
                                        gather=lambda send, recv: recv.copy_(torch.cat(sends)))
        pl.reduce_to_send()
        torch.cuda.synchronize()
        sends.append(pl.send.clone())
        plans.append(pl)
    assert torch.equal(one.send, torch.cat(sends)), "the records differ"
    for pl in plans:
        assert torch.equal(pl.run(), got)
    m, ld = cr.mahal_and_det(Rs, Os, x)
    want = torch.stack([m, ld]).to(F64)
    assert torch.allclose(got, want, rtol=1e-9 if dt == F64 else 2e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("d", [1, 3, 5])
def test_the_library_refuses_a_pointer_off_its_boundary(d, dt):
    """Direct C calls with a pointer one row into an arena buffer: real memory of this test, misaligned.  CGPS_ERR_ARG with
    the argument's name, before anything is launched: not one byte of the arena (0xFF outputs included) has changed."""
    N, lib, dtc, st = 257, _hip.lib(), _hip.dtype_code(dt), _hip.stream_ptr()
    a = Arena(16 << 20)
    a.poison(0xFF)
    Rf, Of, xf = (a.put(t, n) for t, n in zip(_system(N + 1, d, dt), ("Rs", "Os", "x")))
    fac = [a.put(torch.rand(N + 1, d, d, dtype=dt, device="cuda") + 2 * torch.eye(d, dtype=dt, device="cuda"), "factor%d" % i) for i in range(3)]
    o = {k: a.empty((N + 1, d, d), dt, k) for k in ("Dp", "Fp", "Gp", "Sd", "So")}
    xo, out2, info = a.empty((N + 1, d), dt, "xo"), a.empty((2,), F64, "out2"), a.empty((1,), torch.int32, "info")
    ws = a.place(4 << 20, "ws")
    P, Q = (lambda t: _hip.ptr(t)), (lambda t: _hip.ptr(t[1:]))           # noqa: E731  (Q: one row in)
    assert _off_boundary(Rf[1:], Of[1:], xf[1:], o["Dp"][1:], xo[1:])
    nb = ws.numel()
    calls = [
        ("Rs", lambda: lib.cgps_mahal_logdet(Q(Rf), P(Of), P(xf), N, d, dtc, P(ws), nb, P(out2), P(info), st)),
        ("Os", lambda: lib.cgps_mahal_logdet(P(Rf), Q(Of), P(xf), N, d, dtc, P(ws), nb, P(out2), P(info), st)),
        ("x", lambda: lib.cgps_mahal_logdet(P(Rf), P(Of), Q(xf), N, d, dtc, P(ws), nb, P(out2), P(info), st)),
        ("x", lambda: lib.cgps_mahal_logdet_levelwise(P(Rf), P(Of), Q(xf), N, d, dtc, P(ws), nb, P(out2), P(info), st)),
        ("ws", lambda: lib.cgps_mahal_logdet(P(Rf), P(Of), P(xf), N, d, dtc, P(ws[16:]), nb - 16, P(out2), P(info), st)),
        ("Rs", lambda: lib.cgps_decompose(Q(Rf), P(Of), N, d, dtc, P(o["Dp"]), P(o["Fp"]), P(o["Gp"]), P(ws), nb, P(info), st)),
        ("Dp", lambda: lib.cgps_decompose(P(Rf), P(Of), N, d, dtc, Q(o["Dp"]), P(o["Fp"]), P(o["Gp"]), P(ws), nb, P(info), st)),
        ("Gp", lambda: lib.cgps_decompose(P(Rf), P(Of), N, d, dtc, P(o["Dp"]), P(o["Fp"]), Q(o["Gp"]), P(ws), nb, P(info), st)),
        ("y", lambda: lib.cgps_decompose_solve(P(Rf), P(Of), Q(xf), N, d, dtc, P(o["Dp"]), P(o["Fp"]), P(o["Gp"]), P(o["Sd"]), P(xo), P(ws), nb, P(info), st)),
        ("Fp", lambda: lib.cgps_solve(P(fac[0]), Q(fac[1]), P(fac[2]), N, d, dtc, 1, P(xf), P(xo), P(ws), nb, st)),
        ("y", lambda: lib.cgps_solve(P(fac[0]), P(fac[1]), P(fac[2]), N, d, dtc, 1, Q(xf), P(xo), P(ws), nb, st)),
        ("x", lambda: lib.cgps_solve(P(fac[0]), P(fac[1]), P(fac[2]), N, d, dtc, 1, P(xf), Q(xo), P(ws), nb, st)),
        ("xcrr", lambda: lib.cgps_halfsolve(P(fac[0]), P(fac[1]), P(fac[2]), N, d, dtc, 1, P(xf), Q(xo), P(ws), nb, None, st)),
        ("ycrr", lambda: lib.cgps_backsolve(P(fac[0]), P(fac[1]), P(fac[2]), N, d, dtc, 1, Q(xf), P(xo), P(ws), nb, st)),
        ("Dp", lambda: lib.cgps_inverse_blocks(Q(fac[0]), P(fac[1]), P(fac[2]), N, d, dtc, P(o["Sd"]), P(o["So"]), P(ws), nb, st)),
        ("So", lambda: lib.cgps_inverse_blocks(P(fac[0]), P(fac[1]), P(fac[2]), N, d, dtc, P(o["Sd"]), Q(o["So"]), P(ws), nb, st)),
        ("Dp", lambda: lib.cgps_logdet_factor(Q(fac[0]), N, d, dtc, P(ws), nb, P(out2), st)),
        ("mean", lambda: lib.cgps_sample(P(fac[0]), P(fac[1]), P(fac[2]), N, d, dtc, 2, Q(xf), 1, 0, P(o["Sd"]), P(ws), nb, st)),
        ("Rs", lambda: lib.cgps_shard_reduce(Q(Rf), P(Of), P(xf), None, N, d, dtc, P(ws), nb, P(o["Sd"]), P(out2), st)),
        ("O_left", lambda: lib.cgps_shard_reduce(P(Rf), P(Of), P(xf), Q(Of), N, d, dtc, P(ws), nb, P(o["Sd"]), P(out2), st)),
        ("Sd", lambda: lib.cgps_mahal_logdet_adjoint(Q(o["Sd"]), P(o["So"]), P(xf), N, d, dtc, P(xf), P(xf), st)),
        ("Rs", lambda: lib.cgps_decompose_step(Q(Rf), P(Of), N, d, dtc, P(o["Dp"]), P(o["Fp"]), P(o["Gp"]), P(o["Sd"]), P(o["So"]), P(info), st)),
    ]
    before = a.buf.clone()
    for k, (arg, call) in enumerate(calls):
        rc = call()
        msg = lib.cgps_last_error()
        torch.cuda.synchronize()
        assert rc == ERR_ARG, (k, arg, rc, msg)
        assert (" %s = " % arg).encode() in msg and b"not aligned" in msg, (k, arg, msg)
        assert torch.equal(a.buf, before), "call %d (%s): memory changed although the call was refused" % (k, arg)
    # the same calls on the boundary are accepted (mahal_logdet: the one whose three operands were moved above)
    assert lib.cgps_mahal_logdet(P(Rf), P(Of), P(xf), N, d, dtc, P(ws), nb, P(out2), P(info), st) == 0
    torch.cuda.synchronize()
    a.assert_guards(0xFF)


# ---- C (and B for the two LEG entries with a workspace): the per-row LEG entry points ------------------------------------------
# Through the lowest wrappers of leg.py / predict.py, the ones that take contiguous operands and make the one call: the
# operands the kernels read are then the arena's own views.  Ragged batch [1, 2, 7, 64, 65] (a one-row series, a series
# that ends one row into the next 64-row workgroup), M = 1 and 2 models, d x obs in {1, 3, 5, 8} x {1, 3, 8}; and batches
# of ONE series of 1, 2, 3 and 257 rows (R = 1: no gap, `cut` and the off-diagonal arrays are empty; 257: one row into
# the fifth 64-row workgroup) at obs = 3.  The forms for one series (cgps_peg_precision_adjoint, cgps_leg_intercast) run on
# the last series of every batch: n = 1 (intercast), 2, 3, 65, 257.  No series is empty: include/cgps.h gives n_b = 0 a
# meaning for cgps_mahal_logdet_batch alone (test_batched_systems_keep_the_memory_contract runs it there), and the Python
# surface refuses a series of length 0 for every per-row entry.
LENGTHS = [1, 2, 7, 64, 65]
TARGETS = [2, 0, 3, 1, 4]                 # targets per series; a series may have none
BATCHES = {"ragged": (LENGTHS, TARGETS), "R1": ([1], [2]), "R2": ([2], [3]), "R3": ([3], [2]), "R257": ([257], [4])}
SHORT_ROWS = 64                           # max_rows of the second log-likelihood call: longer series are skipped
DRAWS = 3


def _spd(gen, lead, n, dt, scale=0.3):
    W = torch.randn(*lead, n, n, generator=gen, dtype=F64)
    return (torch.eye(n, dtype=F64) + scale * W @ W.transpose(-1, -2)).to(dt).cuda()


def _rows_inputs(d, obs, M, dt, lengths=LENGTHS, targets_per=TARGETS):
    gen = torch.Generator().manual_seed(1000 + 10 * d + obs)
    R, B = sum(lengths), len(lengths)
    off = [0]
    for n in lengths:
        off.append(off[-1] + n)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=F64).to(dt).cuda()       # noqa: E731
    ts64 = torch.cat([2.0 - 0.7 * b + torch.cumsum(0.2 + torch.rand(n, generator=gen, dtype=F64), 0) for b, n in enumerate(lengths)])
    cut = torch.zeros(R - 1, dtype=torch.uint8)
    if B > 1:
        cut[torch.tensor(off[1:-1]) - 1] = 1
    t0 = torch.stack([ts64[off[b]] - 0.3 - 0.1 * b for b in range(B)])
    gap = torch.cat([ts64[:1] * 0, ts64[1:] - ts64[:-1]])
    gap[torch.tensor(off[:-1])] = 0.3 + 0.1 * torch.arange(B, dtype=F64)
    targets, toff = [], [0]
    for b, p in enumerate(targets_per):       # before, inside, at and after the series' own rows; strictly increasing
        lo, hi = float(ts64[off[b]]), float(ts64[off[b + 1] - 1])
        targets.append(torch.linspace(lo - 0.5, hi + 0.7, p, dtype=F64) if p else torch.zeros(0, dtype=F64))
        toff.append(toff[-1] + p)
    t = {
        "ts": ts64.to(dt).cuda(), "cut": cut.cuda(), "offsets": torch.tensor(off, dtype=torch.int64).cuda(),
        "ids": torch.arange(B, dtype=torch.int64).cuda() + 3, "words": (10 * torch.arange(M, dtype=torch.int64)).cuda(),
        "G": torch.stack([_leg_model(d, dt, 60 + 7 * k + d)[0] for k in range(M)]),
        "Bm": r(M, obs, d), "LLT": _spd(gen, (M,), obs, dt),
        "xs": r(R, obs), "noise_var": (0.1 + torch.rand(R, obs, generator=gen, dtype=F64)).to(dt).cuda(),
        "pat_table": torch.randint(0, 3, (R,), generator=gen).to(torch.uint8).cuda(),
        "pat_bits": torch.randint(0, 2 ** obs, (R,), generator=gen).to(torch.uint8).cuda(),
        "term": _spd(gen, (M,), d, dt), "table": _spd(gen, (M, 3), d, dt), "basis": _spd(gen, (M, 2), d, dt),
        "weights": torch.rand(M, R, 2, generator=gen, dtype=F64).to(dt).cuda(),
        "h_plain": r(M, d, obs), "h_table": r(M, 3, d, obs), "h_rows": r(M, R, d, obs),
        "v": r(M, R, d), "q": r(M, R), "ip_mean": r(M * R, d), "Sd": _spd(gen, (M * R,), d, dt),
        "So": 0.1 * r(M * R - 1, d, d), "gRs": r(M * R, d, d), "gOs": r(M * R - 1, d, d), "z": r(M * R, d, DRAWS),
        "targets": torch.cat(targets).to(dt).cuda(), "target_offsets": torch.tensor(toff, dtype=torch.int64).cuda(),
        "t0": t0.to(dt).cuda(), "m0": r(M, B, d), "P0": _spd(gen, (M, B), d, dt), "gap": gap.to(dt).cuda(),
        "c_mean": r(M, R, obs), "c_cov": r(M, R, obs, obs), "c_lp": r(M, R), "c_zm": r(M, R, d), "c_zc": r(M, R, d, d),
    }
    return t


def _rows_ops(t, arena, lengths=LENGTHS, targets_per=TARGETS):
    import types
    from cyclic_gps import predict
    G, M = t["G"], t["G"].shape[0]
    d, dt, dev = G.shape[-1], G.dtype, G.device
    R, B, obs = t["ts"].shape[0], len(lengths), t["Bm"].shape[1]
    plan = types.SimpleNamespace(R=R, B=B, offsets=t["offsets"], long=[], starts=t["offsets"].tolist(), lengths=lengths)
    tplan = types.SimpleNamespace(P=sum(targets_per), B=B, offsets=t["target_offsets"])
    keep = [b for b, n in enumerate(lengths) if n <= SHORT_ROWS]
    skip = [b for b, n in enumerate(lengths) if n > SHORT_ROWS]
    models = M > 1                                  # M = 1: the forms without a model axis; M = 2: the models forms
    lead = (lambda a: a) if models else (lambda a: a[0])
    fused = d <= 7 and not (d == 6 and dt == F64)   # cgps_peg_precision_models and the loglik forms are built for these
    out, untouched = {}, []

    def label(s):
        if arena is not None:
            arena.label = s
    Gm = lead(G)
    if fused or not models:
        label("peg_precision seg / models")
        out["peg_precision"] = list(leg._peg_precision_models(t["ts"], Gm, t["cut"]))
        label("peg_precision_adjoint seg / models")
        out["peg_adjoint"] = list(leg._peg_precision_adjoint_models(t["ts"], Gm, t["cut"], t["gRs"], t["gOs"], True))
    if M == 1 and lengths[-1] >= 2:
        label("peg_precision_adjoint")
        n1 = lengths[-1]                               # the last series alone (ts is read by element: any row may come first)
        part = torch.empty((n1 - 1 + 63) // 64, d, d, dtype=dt, device=dev)
        gtau = torch.empty(n1 - 1, dtype=dt, device=dev)
        _hip.check(_hip.lib().cgps_peg_precision_adjoint(_hip.ptr(t["ts"][R - n1:]), _hip.ptr(Gm), n1, d, _hip.dtype_code(dt), _hip.ptr(t["gRs"]),
                                                         _hip.ptr(t["gOs"]), _hip.ptr(part), _hip.ptr(gtau), _hip.stream_ptr()))
        out["peg_adjoint_one"] = [part, gtau]
    for name, src, term, rows in (("plain", _hip.ROWS_PLAIN, t["term"], None), ("table", _hip.ROWS_TABLE, t["table"], t["pat_table"]),
                                  ("weighted", _hip.ROWS_WEIGHTED, t["basis"], t["weights"])):
        label("posterior_blocks " + name)
        rows_m = rows if (rows is None or src == _hip.ROWS_TABLE) else lead(rows)
        out["posterior_blocks_" + name] = list(leg._posterior_blocks_models(t["ts"], Gm, t["cut"], src, lead(term), rows_m))
        if fused:
            label("loglik " + name)
            vq = (lead(t["v"]), lead(t["q"]))
            out["loglik_" + name] = list(leg._leg_rows_reductions(t["ts"], Gm, src, lead(term), rows_m, *vq, plan))
            label("loglik %s, max_rows 64" % name)          # a longer series is skipped: nothing of its slot is written
            real, leg.BATCH_MAX_ROWS = leg.BATCH_MAX_ROWS, SHORT_ROWS
            try:
                o4, _ = leg._leg_rows_reductions(t["ts"], Gm, src, lead(term), rows_m, *vq, plan)
            finally:
                leg.BATCH_MAX_ROWS = real
            out["loglik_short_" + name] = [o4[..., keep, :]]
            if arena is not None:
                untouched.append(o4[..., skip, :])
    if M == 1:
        label("intercast")                             # the last series alone
        s, n1, k = R - lengths[-1], lengths[-1], sum(targets_per) - targets_per[-1]
        out["intercast"] = list(predict._intercast_hip(Gm, t["ip_mean"][s:], t["Sd"][s:], t["So"][s:], t["ts"][s:], t["targets"][k:]))
    label("intercast seg / models")
    out["intercast_seg"] = list(predict._intercast_models_hip(Gm, t["ip_mean"], t["Sd"], t["So"], t["ts"], plan, t["targets"], tplan))
    for name, hs, hterm, pat in (("none", _hip.H_NONE, None, None), ("plain", _hip.H_PLAIN, t["h_plain"], None),
                                 ("table", _hip.H_TABLE, t["h_table"], t["pat_table"]), ("rows", _hip.H_ROWS, t["h_rows"], None)):
        label("perturbation " + name)
        out["perturbation_" + name] = leg._perturbation_models(t["ts"], Gm, plan, t["ids"], hs, None if hterm is None else lead(hterm), pat,
                                                               lead(t["v"]), DRAWS, 11, t["words"] if models else 5)
    label("observations")
    out["observations"] = list(leg._observations_rows(t["z"], t["pat_bits"], t["noise_var"], plan, t["ids"], t["Bm"], t["LLT"], 12, t["words"]))
    for leave in (0, 1):
        label("loo leave %d" % leave)
        out["loo%d" % leave] = list(leg._loo_rows(t["xs"], t["pat_bits"], t["noise_var"], t["offsets"], t["Bm"], t["LLT"], t["ip_mean"],
                                                   t["Sd"], leave))
    init = (t["t0"], t["m0"], t["P0"])
    label("filter")
    fo = leg._filter_rows(t["ts"], t["xs"], t["pat_bits"], t["noise_var"], t["offsets"], G, t["Bm"], t["LLT"], init)
    out["filter"] = list(fo)
    label("filter_scan")
    chunks = leg._chunk_plan_kind(4)(lengths, dev)
    out["filter_scan"] = list(leg._filter_rows(t["ts"], t["xs"], t["pat_bits"], t["noise_var"], t["offsets"], G, t["Bm"], t["LLT"], init,
                                               scan=(chunks, 2)))
    out["filter_scan_prior"] = list(leg._filter_rows(t["ts"], t["xs"], None, None, t["offsets"], G, t["Bm"], t["LLT"], None, scan=(chunks, 2)))
    label("filter_adjoint")
    out["filter_adjoint"] = list(leg._filter_adjoint_rows(t["xs"], t["pat_bits"], t["noise_var"], t["offsets"], G, t["Bm"], t["LLT"], t["gap"],
                                                          fo[3], fo[4], t["m0"], t["P0"],
                                                          [t["c_mean"], t["c_cov"], t["c_lp"], t["c_zm"], t["c_zc"]]))
    return out, untouched


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("obs", [1, 3, 8])
@pytest.mark.parametrize("d", [1, 3, 5, 8])
def test_per_row_leg_entries_keep_the_memory_contract(d, obs, M, dt):
    _rows_case("ragged", d, obs, M, dt)


def _rows_case(batch, d, obs, M, dt):
    lengths, targets_per = BATCHES[batch]
    inputs = _rows_inputs(d, obs, M, dt, lengths, targets_per)
    R = sum(lengths)
    payload = M * R * (40 * d * d + 6 * obs * obs + 20 * (d + obs) + 4 * d * DRAWS) * 8
    _three_runs(functools.partial(_rows_ops, lengths=lengths, targets_per=targets_per), inputs, _out_bytes(220, 2 * payload),
                "rows %s d %d obs %d M %d" % (batch, d, obs, M))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("d", [1, 3, 5, 8])
@pytest.mark.parametrize("batch", ["R1", "R2", "R3", "R257"])
def test_per_row_leg_entries_on_one_series_of_1_2_3_and_257_rows(batch, d, M, dt):
    _rows_case(batch, d, 3, M, dt)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F64, F32], ids=["fp64", "fp32"])
def test_the_scan_of_one_long_series_keeps_the_memory_contract(dt):
    """cgps_leg_filter_scan with chunk_rows = (4, 2) on ONE series of 70 rows (18 chunks, five levels of elements), M = 2."""
    d, obs, M, n = 5, 3, 2, 70
    gen = torch.Generator().manual_seed(77)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=F64).to(dt).cuda()       # noqa: E731
    inputs = {"ts": torch.cumsum(0.2 + torch.rand(n, generator=gen, dtype=F64), 0).to(dt).cuda(), "xs": r(n, obs),
              "offsets": torch.tensor([0, n], dtype=torch.int64).cuda(),
              "G": torch.stack([_leg_model(d, dt, 90 + k)[0] for k in range(M)]), "Bm": r(M, obs, d), "LLT": _spd(gen, (M,), obs, dt)}

    def ops(t, arena):
        if arena is not None:
            arena.label = "filter_scan, one series"
        chunks = leg._chunk_plan_kind(4)([n], t["G"].device)
        return {"filter_scan": list(leg._filter_rows(t["ts"], t["xs"], None, None, t["offsets"], t["G"], t["Bm"], t["LLT"], None,
                                                     scan=(chunks, 2)))}, []
    _three_runs(ops, inputs, _out_bytes(16, 64 * 1024), "scan of one series")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("d,obs", [(5, 3), (1, 1), (8, 8)])
def test_a_leg_workspace_one_byte_short_is_an_argument_error(d, obs, dt):
    """The same for the two LEG entries with a workspace, cgps_leg_filter_scan (chunk_rows = (4, 2)) and
    cgps_leg_filter_adjoint, as direct C calls on the ragged batch with M = 2: operands, 0xFF outputs and workspaces of
    exactly the stated size inside one arena.  ``need - 1``: CGPS_ERR_ARG and not one byte changed; a workspace 16 bytes
    off its 256-byte boundary: the same; ``need``: accepted, guards intact (that every output element is then written is
    test_per_row_leg_entries_keep_the_memory_contract's business)."""
    M, L, fanout = 2, 4, 2
    lib, dtc, st = _hip.lib(), _hip.dtype_code(dt), _hip.stream_ptr()
    src = _rows_inputs(d, obs, M, dt)
    R, B = sum(LENGTHS), len(LENGTHS)
    a = Arena(32 << 20)
    a.poison(0xFF)
    t = {k: a.put(v, k) for k, v in src.items()}
    chunks = leg._chunk_plan_kind(L)(LENGTHS, "cuda")
    co, cs, sc = (a.put(v, n) for v, n in ((chunks.chunk_offsets, "chunk_offsets"), (chunks.chunk_series, "chunk_series"),
                                           (chunks.series_chunks, "series_chunks")))
    e = lambda name, *shape: a.empty(shape, dt, name)            # noqa: E731
    fwd = [e("mean", M, R, obs), e("cov", M, R, obs, obs), e("logpdf", M, R), e("z_mean", M, R, d), e("z_cov", M, R, d, d),
           a.empty((M, B), F64, "loglik"), e("m_end", M, B, d), e("P_end", M, B, d, d), a.empty((1,), torch.int32, "info")]
    bwd = [e("g_xs", M, R, obs), e("g_noise_var", M, R, obs), e("g_Bmat", M, B, obs, d), e("g_LLT", M, B, obs, obs), e("g_m0", M, B, d),
           e("g_P0", M, B, d, d), e("g_G_partial", M, (R + 63) // 64, d, d), e("g_gap", M, R)]
    zm, zc = a.put(torch.randn(M, R, d, dtype=dt, device="cuda"), "saved z_mean"), a.put(_spd(torch.Generator().manual_seed(3), (M, R), d, dt), "saved z_cov")
    P = _hip.ptr
    data = (P(t["ts"]), P(t["xs"]), P(t["pat_bits"]), P(t["noise_var"]), P(t["offsets"]), B, R, M, P(t["G"]), P(t["Bm"]), P(t["LLT"]), d, obs,
            dtc, P(t["t0"]), P(t["m0"]), P(t["P0"]))
    calls = {
        "cgps_leg_filter_scan": (_hip.filter_scan_workspace_bytes(chunks.chunks, M, d, dtc, fanout), lambda w, b: lib.cgps_leg_filter_scan(
            *data, P(co), P(cs), P(sc), chunks.chunks, L, fanout, w, b, *(P(x) for x in fwd), st)),
        "cgps_leg_filter_adjoint": (_hip.filter_adjoint_workspace_bytes(R, B, M, d, obs, dtc), lambda w, b: lib.cgps_leg_filter_adjoint(
            P(t["xs"]), P(t["pat_bits"]), P(t["noise_var"]), P(t["offsets"]), B, R, M, P(t["G"]), P(t["Bm"]), P(t["LLT"]), d, obs, dtc,
            P(t["gap"]), P(zm), P(zc), P(t["m0"]), P(t["P0"]), P(t["c_mean"]), P(t["c_cov"]), P(t["c_lp"]), P(t["c_zm"]), P(t["c_zc"]),
            w, b, *(P(x) for x in bwd), st)),
    }
    ws = {name: a.place(need + 256, "ws " + name) for name, (need, _) in calls.items()}      # (+ 256: room for the shifted call)
    before = a.buf.clone()
    for name, (need, call) in calls.items():
        assert need > 0 and need % 256 == 0
        for what, w, b, word in (("short", ws[name], need - 1, b"workspace"), ("shifted", ws[name][16:], need, b"not aligned")):
            rc = call(P(w), b)
            msg = lib.cgps_last_error()
            torch.cuda.synchronize()
            assert rc == ERR_ARG and word in msg, (name, what, rc, msg)
            assert torch.equal(a.buf, before), "%s (%s): memory changed although the call was refused" % (name, what)
    for name, (need, call) in calls.items():
        assert call(P(ws[name]), need) == 0, (name, lib.cgps_last_error())
    torch.cuda.synchronize()
    a.assert_guards(0xFF)


# ---- the kernels against the plan's model of their writes -------------------------------------------------------------------
# tests/plan_check.cpp checks that every pass's write extent (forward_write_bytes, backward_write_bytes, the write_bytes
# of DecPass / InvPass) lies inside the region the plan hands it -- the plan against the plan.  Here the kernels are held
# to that model: after a call on a poisoned workspace of exactly the stated size, every byte of the workspace OUTSIDE the
# modelled extents still holds the poison.  A pass that stores one row further than the host believes is seen although it
# stays inside the (generously sized) region and far from the guards.
@functools.lru_cache(maxsize=None)
def _extents():
    """{(N, d, scalar size, op): [(offset, bytes)]} for every case, from tests/plan_cases.cpp --extents with the CU count
    of this device (the sweeps take the latency-bound kernels for passes of at most one tile per CU)."""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    args = ["%d,%d,%d,1" % (N, d, 8 if dt == F64 else 4) for N, d, dt in CASES]
    with tempfile.TemporaryDirectory(prefix="plan_cases_") as tmp:        # (gone again when the table has been read)
        exe = _build(pathlib.Path(tmp), "plan_cases.cpp", _host_compiler())
        out = subprocess.run([exe, "--cus", str(cus), "--extents"] + args, capture_output=True, text=True, check=True, timeout=300).stdout
    table = {}
    for line in out.splitlines():
        f = line.split()
        assert f[0] == "extent" and len(f) == 7, line
        table.setdefault((int(f[1]), int(f[2]), int(f[3]), f[4]), []).append((int(f[5]), int(f[6])))
    return table


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_passes_write_only_where_the_plan_says(case):
    N, d, dt = case
    Rs, Os, x = _system(N, d, dt)
    dec = cr._decompose_raw(Rs, Os)
    xs = cr.halfsolve(dec, x)
    ops = {"halfsolve": lambda: cr.halfsolve(dec, x), "backsolve": lambda: cr.backhalfsolve(dec, xs),
           "decompose": lambda: cr._decompose_raw(Rs, Os), "inverse": lambda: cr.inverse_blocks(dec)}
    for op, call in ops.items():
        with _recording_scratch() as sizes:
            call()
        assert len(sizes) == 1
        for byte in POISONS:
            arena = Arena(capacity_for(sizes))
            arena.poison(byte)
            arena.label = op
            with arena.exact_scratch(_hip):
                call()
            torch.cuda.synchronize()
            arena.assert_guards(byte)
            ws = arena.scratch[0]
            nobody = torch.ones(ws.numel(), dtype=torch.bool, device=ws.device)
            for off, nbytes in _extents().get((N, d, 8 if dt == F64 else 4, op), []):      # (no line: nothing is written)
                assert off + nbytes <= ws.numel(), (op, off, nbytes, ws.numel())
                nobody[off:off + nbytes] = False
            changed = torch.nonzero(nobody & (ws != byte)).flatten()
            assert changed.numel() == 0, ("%s %s, poison 0x%02X: %d workspace bytes outside the plan's write extents were written, "
                                          "offsets %d .. %d of %d" % (_case_id(case), op, byte, changed.numel(), int(changed[0]),
                                                                      int(changed[-1]), ws.numel()))

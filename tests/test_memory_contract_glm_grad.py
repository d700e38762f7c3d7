"""cgps_leg_glm_evidence_rhs and cgps_leg_glm_evidence_adjoint (include/cgps_glm_grad.h) held to the memory contract of
tests/test_memory_contract.py, exactly as tests/test_memory_contract_glm.py holds the step: the ordinary
call, then operands and outputs between 64 KiB guards with everything that is not an operand poisoned 0xFF, then 0x00.
Outputs equal bit for bit (every sum runs in a fixed order), guards intact, operands unchanged: so every output element
is written, nothing is read outside an operand and nothing is written outside an output.  The entries take no
workspace.  A null or misaligned argument is CGPS_ERR_ARG with the argument's name, and not one byte changes."""
import ctypes

import pytest
import torch

from _arena import Arena
from cyclic_gps import _hip, leg
from test_memory_contract import _out_bytes, _three_runs
from test_memory_contract_glm import ERR_ARG, FAMILIES, LENGTHS, OBS_OF, _inputs, _plan

F32, F64 = torch.float32, torch.float64


def _grad_inputs(d, obs, dt):
    """the operands of the step's test, and blocks, a solve and cotangents of the right shapes (the entries ask nothing of
    their values)"""
    t = _inputs(d, obs, dt)
    gen = torch.Generator().manual_seed(900 + 10 * d + obs)
    R, B = sum(LENGTHS), len(LENGTHS)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=F64)       # noqa: E731

    def spd(n):
        a = 0.3 * r(n, d, d)
        return a @ a.transpose(-1, -2) + 0.5 * torch.eye(d, dtype=F64)
    t = {k: t[k] for k in ("z", "counts", "binary", "values", "pattern", "offset", "log_exposure", "noise_var", "Bm", "offsets")}
    t.update(u=(0.1 * r(R, d)).to(dt).cuda(), Sd=spd(R).to(dt).cuda(), So=(0.1 * r(R - 1, d, d)).to(dt).cuda(),
             Pd=spd(R).to(dt).cuda(), Po=(0.1 * r(R - 1, d, d)).to(dt).cuda(),
             gE=torch.tensor([1.5, -0.75, 0.0, 2.0], dtype=F64).cuda())
    return t


def _grad_ops(t, arena):
    """both entries for every family, with and without pattern, offset and log_exposure"""
    out = {}
    plan = _plan(t["offsets"], len(LENGTHS))
    for name, fam in FAMILIES:
        ys = t[{"poisson": "counts", "bernoulli": "binary", "gaussian": "values"}[name]]
        extra = t["noise_var"] if name == "gaussian" else t["log_exposure"]
        for full in (False, True):
            if arena is not None:
                arena.label = "%s full %d" % (name, full)
            op = leg._GlmOperands(plan, None, None, ys, None, None if full else t["offset"],
                                  None if (full and name != "gaussian") else extra, t["Bm"], fam, 1e-3)
            op.pattern = None if full else t["pattern"]
            out["%s %d rhs" % (name, full)] = [leg._glm_evidence_rhs_hip(op, t["z"], t["Sd"])]
            out["%s %d adjoint" % (name, full)] = list(leg._glm_evidence_adjoint_hip(op, t["z"], t["u"], t["Sd"], t["So"], t["Pd"],
                                                                                   t["Po"], t["gE"]))
    return out, []


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("d", [1, 5, 8])
def test_the_gradient_entries_keep_the_memory_contract(d, dt):
    obs = OBS_OF[d]
    inputs = _grad_inputs(d, obs, dt)
    R, B = sum(LENGTHS), len(LENGTHS)
    per_call = R * (2 * d * d + d + obs) * 8 + B * obs * (d + 1) * 8
    ref = _three_runs(_grad_ops, inputs, _out_bytes(6 * 6, 6 * per_call), "glm grad d %d obs %d" % (d, obs))
    # what the three runs compared is a gradient, not zeros; the series with gE = 0 wrote exact zeros
    off = inputs["offsets"].tolist()
    gRs, gOs, g_extra, gB, goff = ref["poisson 0 adjoint"]
    assert all(bool(torch.isfinite(x).all()) for x in ref["poisson 0 adjoint"])
    assert float(gRs[off[3]:].abs().min()) >= 0 and float(gRs[off[3]:].abs().max()) > 0 and float(gB[3].abs().max()) > 0
    assert bool((gRs[off[2]:off[3]] == 0).all()) and bool((gB[2] == 0).all()) and bool((goff[2] == 0).all())
    for k in off[1:-1]:
        assert bool((gOs[k - 1] == 0).all())
    assert float(ref["poisson 0 rhs"][0].abs().max()) > 0 and float(ref["gaussian 0 rhs"][0].abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("d", [1, 5])
def test_a_null_or_misaligned_argument_is_refused_by_name(d, dt):
    obs = OBS_OF[d]
    t = _grad_inputs(d, obs, dt)
    R, B = sum(LENGTHS), len(LENGTHS)
    a = Arena(8 << 20)
    a.poison(0xFF)
    p = {k: a.put(v, k) for k, v in t.items()}
    o = {"s": a.empty((R, d), dt, "s"), "gRs": a.empty((R, d, d), dt, "gRs"), "gOs": a.empty((R - 1, d, d), dt, "gOs"),
         "g_extra": a.empty((R, obs), dt, "g_extra"), "gB_part": a.empty((B, obs, d), F64, "gB_part"),
         "goffset_part": a.empty((B, obs), F64, "goffset_part")}
    lib, dtc, st = _hip.lib(), _hip.dtype_code(dt), _hip.stream_ptr()
    base = {"z": p["z"], "u": p["u"], "Sd": p["Sd"], "So": p["So"], "Pd": p["Pd"], "Po": p["Po"], "ys": p["counts"],
            "pattern": p["pattern"], "offset": p["offset"], "extra": p["log_exposure"], "Bmat": p["Bm"], "offsets": p["offsets"],
            "gE": p["gE"], **o}
    rhs_order = ["z", "Sd", "ys", "pattern", "offset", "extra", "Bmat"]
    adj_order = ["z", "u", "Sd", "So", "Pd", "Po", "ys", "pattern", "offset", "extra", "Bmat", "offsets", "gE"]
    adj_tail = ["gRs", "gOs", "g_extra", "gB_part", "goffset_part"]

    def rhs(family=_hip.GLM_POISSON, **swap):
        ptrs = {k: _hip.ptr(v) for k, v in base.items()}
        ptrs.update(swap)
        return lib.cgps_leg_glm_evidence_rhs(*[ptrs[k] for k in rhs_order], R, d, obs, dtc, family, ptrs["s"], st)

    def adjoint(family=_hip.GLM_POISSON, **swap):
        ptrs = {k: _hip.ptr(v) for k, v in base.items()}
        ptrs.update(swap)
        return lib.cgps_leg_glm_evidence_adjoint(*[ptrs[k] for k in adj_order], B, R, d, obs, dtc, family,
                                                 *[ptrs[k] for k in adj_tail], st)

    one_in = lambda k: ctypes.c_void_p(base[k].data_ptr() + base[k].element_size())      # noqa: E731  (inside the view)
    before = a.buf.clone()
    for call, nulls, vecs in ((rhs, ("z", "Sd", "ys", "Bmat", "s"), ("z", "Sd", "s")),
                              (adjoint, ("z", "u", "Sd", "So", "Pd", "Po", "ys", "Bmat", "offsets", "gE", "gRs", "gOs", "g_extra",
                                         "gB_part", "goffset_part"), ("z", "u", "Sd", "So", "Pd", "Po", "gRs", "gOs"))):
        refused = [(k, {k: None}, b"NULL") for k in nulls] + [(k, {k: one_in(k)}, b"not aligned") for k in vecs]
        for k, swap, word in refused:
            rc = call(**swap)
            msg = lib.cgps_last_error()
            torch.cuda.synchronize()
            assert rc == ERR_ARG, (k, rc, msg)
            assert (b" %s = " % k.encode()) in msg and word in msg, (k, msg)
            assert torch.equal(a.buf, before), "%s: memory changed although the call was refused" % k
        assert call(family=_hip.GLM_GAUSSIAN, extra=None) == ERR_ARG and b" extra = " in lib.cgps_last_error()
        assert call(family=7) == ERR_ARG
        torch.cuda.synchronize()
        assert torch.equal(a.buf, before)
    assert rhs() == 0, lib.cgps_last_error()                    # the same calls with every argument in place are accepted
    assert adjoint() == 0, lib.cgps_last_error()
    torch.cuda.synchronize()
    a.assert_guards(0xFF)

"""cgps_leg_glm_step (include/cgps_glm.h) held to the memory contract of tests/test_memory_contract.py,
with the same arena (tests/_arena.py) and the same three runs: the ordinary call, then operands and outputs between
64 KiB guards with everything that is not an operand poisoned 0xFF, then 0x00.  Outputs equal bit for bit (every sum of
the kernel runs in a fixed order), guards intact, operands unchanged: so every output element is written, nothing is
read outside an operand and nothing is written outside an output.  The entry takes no workspace.  A null or misaligned
argument is CGPS_ERR_ARG with the argument's name, and not one byte changes."""
import ctypes
import types

import pytest
import torch

from _arena import Arena
from cyclic_gps import _hip, leg
from test_memory_contract import _leg_model, _out_bytes, _three_runs

F32, F64 = torch.float32, torch.float64
LENGTHS = (1, 2, 65, 257)          # one row; one coupling block; one row into a second stride of the 64 lanes; five strides
OBS_OF = {1: 1, 5: 3, 8: 8}
ERR_ARG = 1
FAMILIES = (("poisson", _hip.GLM_POISSON), ("bernoulli", _hip.GLM_BERNOULLI), ("gaussian", _hip.GLM_GAUSSIAN))


def _plan(offsets, B):
    return types.SimpleNamespace(offsets=offsets, B=B)


def _inputs(d, obs, dt):
    gen = torch.Generator().manual_seed(300 + 10 * d + obs)
    B, R = len(LENGTHS), sum(LENGTHS)
    off = [0]
    for n in LENGTHS:
        off.append(off[-1] + n)
    G = _leg_model(d, dt, 70 + d)[0]
    ts = torch.cat([1.0 - 0.4 * b + torch.cumsum(0.3 + 0.5 * torch.rand(n, generator=gen, dtype=F64), 0)
                    for b, n in enumerate(LENGTHS)]).to(dt).cuda()
    cut = torch.zeros(R - 1, dtype=torch.uint8)
    cut[torch.tensor(off[1:-1]) - 1] = 1
    Rs, Os = leg._peg_precision_seg(ts, G.contiguous(), cut.cuda())
    r = lambda *s: torch.randn(*s, generator=gen, dtype=F64)       # noqa: E731
    z = 0.3 * r(R, d)
    state = torch.tensor([[-3.0, 1.0, 0.0, 1.0], [-7.5, 2.0, float(_hip.GLM_CONVERGED), 0.5],
                          [-40.0, 3.0, 0.0, 0.25], [-90.0, 4.0, float(_hip.GLM_STALLED), 0.0]], dtype=F64)
    return {
        "z": z.to(dt).cuda(), "prop": (z + 0.2 * r(R, d)).to(dt).cuda(), "Rs": Rs, "Os": Os,
        "counts": torch.poisson(torch.full((R, obs), 2.0, dtype=F64), generator=gen).to(dt).cuda(),
        "binary": (torch.rand(R, obs, generator=gen) < 0.5).to(dt).cuda(), "values": r(R, obs).to(dt).cuda(),
        "pattern": torch.randint(0, 1 << obs, (R,), generator=gen).to(torch.uint8).cuda(),
        "offset": (0.5 * r(obs)).to(dt).cuda(), "log_exposure": (0.2 * r(R, obs)).to(dt).cuda(),
        "noise_var": (0.1 + 1.9 * torch.rand(R, obs, generator=gen, dtype=F64)).to(dt).cuda(),
        "Bm": (0.5 * r(obs, d)).to(dt).cuda(), "offsets": torch.tensor(off, dtype=torch.int64).cuda(), "state": state.cuda(),
    }


def _glm_ops(t, arena):
    """the first call (no proposal, no state) and a step with two active and two frozen series, for every family: with
    and without pattern, offset and log_exposure"""
    out = {}
    plan = _plan(t["offsets"], len(LENGTHS))
    for name, fam in FAMILIES:
        ys = t[{"poisson": "counts", "bernoulli": "binary", "gaussian": "values"}[name]]
        extra = t["noise_var"] if name == "gaussian" else t["log_exposure"]
        for full in (False, True):
            if arena is not None:
                arena.label = "%s full %d" % (name, full)
            op = leg._GlmOperands(plan, t["Rs"], t["Os"], ys, None, None if full else t["offset"],
                                  None if (full and name != "gaussian") else extra, t["Bm"], fam, 1e-3)
            op.pattern = None if full else t["pattern"]
            out["%s %d first" % (name, full)] = list(leg._glm_step_hip(op, t["z"], None, None))
            out["%s %d step" % (name, full)] = list(leg._glm_step_hip(op, t["z"], t["prop"], t["state"]))
    return out, []


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("d", [1, 5, 8])
def test_the_glm_step_keeps_the_memory_contract(d, dt):
    obs = OBS_OF[d]
    inputs = _inputs(d, obs, dt)
    R, B = sum(LENGTHS), len(LENGTHS)
    per_call = R * (d * d + 2 * d) * 8 + B * _hip.GLM_STATE * 8
    ref = _three_runs(_glm_ops, inputs, _out_bytes(4 * 12, 12 * per_call), "glm step d %d obs %d" % (d, obs))
    # what the three runs compared is a step, not a no-op: the active series moved, the frozen ones did not
    z_out, _, _, state = ref["poisson 0 step"]
    off = inputs["offsets"].tolist()
    for b, frozen in enumerate((False, True, False, True)):
        same = torch.equal(z_out[off[b]:off[b + 1]], inputs["z"][off[b]:off[b + 1]])
        assert same == frozen or float(state[b, 3]) == 0.0, (b, frozen, state[b].tolist())
        if frozen:
            assert torch.equal(state[b], inputs["state"][b])
        else:
            assert float(state[b, 1]) == float(inputs["state"][b, 1]) + 1
    assert bool(torch.isfinite(state).all())
    first = ref["poisson 0 first"]
    assert torch.equal(first[0], inputs["z"]) and float(first[3][:, 1:].abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("d", [1, 5])
def test_a_null_or_misaligned_argument_is_refused_by_name(d, dt):
    obs = OBS_OF[d]
    t = _inputs(d, obs, dt)
    R, B = sum(LENGTHS), len(LENGTHS)
    a = Arena(8 << 20)
    a.poison(0xFF)
    p = {k: a.put(v, k) for k, v in t.items()}
    o = {"z_out": a.empty((R, d), dt, "z_out"), "J_Rs": a.empty((R, d, d), dt, "J_Rs"), "rhs": a.empty((R, d), dt, "rhs"),
         "state_out": a.empty((B, _hip.GLM_STATE), F64, "state_out")}
    lib, dtc, st = _hip.lib(), _hip.dtype_code(dt), _hip.stream_ptr()
    order = ["z", "prop", "Rs", "Os", "ys", "pattern", "offset", "extra", "Bmat", "offsets"]
    tail = ["state_in", "z_out", "J_Rs", "rhs", "state_out"]
    base = {"z": p["z"], "prop": p["prop"], "Rs": p["Rs"], "Os": p["Os"], "ys": p["counts"], "pattern": p["pattern"],
            "offset": p["offset"], "extra": p["log_exposure"], "Bmat": p["Bm"], "offsets": p["offsets"], "state_in": p["state"], **o}

    def call(family=_hip.GLM_POISSON, **swap):
        ptrs = {k: _hip.ptr(v) for k, v in base.items()}
        ptrs.update(swap)
        return lib.cgps_leg_glm_step(*[ptrs[k] for k in order], B, R, d, obs, dtc, family, 1e-3, *[ptrs[k] for k in tail], st)

    one_in = lambda k: ctypes.c_void_p(base[k].data_ptr() + base[k].element_size())      # noqa: E731  (inside the view)
    before = a.buf.clone()
    refused = [(k, {k: None}, b"NULL") for k in ("z", "Rs", "Os", "ys", "Bmat", "offsets", "state_in", "z_out", "J_Rs", "rhs",
                                                  "state_out")]
    refused += [(k, {k: one_in(k)}, b"not aligned") for k in ("z", "prop", "Rs", "Os", "z_out", "J_Rs", "rhs")]
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
    assert call() == 0, lib.cgps_last_error()                   # the same call with every argument in place is accepted
    torch.cuda.synchronize()
    a.assert_guards(0xFF)

"""cgps_leg_glm_predict (include/cgps_glm_predict.h) held to the memory contract of tests/test_memory_contract.py (DESIGN.md
3.2), exactly as tests/test_memory_contract_glm_grad.py holds the gradient entries: the ordinary call, then operands and
outputs between 64 KiB guards with everything that is not an operand poisoned 0xFF, then 0x00.  Outputs equal bit for bit
(a lane per entry, nothing shared), guards intact, operands unchanged: so every output element is written, nothing is
read outside an operand and nothing is written outside an output.  The entry takes no workspace.  A null or misaligned
argument is CGPS_ERR_ARG with the argument's name, and not one byte changes."""
import ctypes

import pytest
import torch

from _arena import Arena
from cyclic_gps import _hip, leg
from test_memory_contract import _out_bytes, _three_runs
from test_memory_contract_glm import ERR_ARG, FAMILIES, LENGTHS, OBS_OF
from test_memory_contract_glm_grad import _grad_inputs

F32, F64 = torch.float32, torch.float64
KEYS = ("z", "Sd", "counts", "binary", "values", "pattern", "offset", "log_exposure", "noise_var", "Bm")


def _predict_inputs(d, obs, dt):
    """the operands of the gradient entries' test that this entry reads: the mode for the latent means, the blocks of J^-1
    for the covariances"""
    t = _grad_inputs(d, obs, dt)
    return {k: t[k] for k in KEYS}


def _predict_ops(t, arena):
    """every family, with and without pattern, offset and log_exposure, with and without ys"""
    out = {}
    for name, fam in FAMILIES:
        ys = t[{"poisson": "counts", "bernoulli": "binary", "gaussian": "values"}[name]]
        extra = t["noise_var"] if name == "gaussian" else t["log_exposure"]
        for full in (False, True):
            for data in (True, False):
                if arena is not None:
                    arena.label = "%s full %d data %d" % (name, full, data)
                got = leg._glm_predict_hip(fam, t["z"], t["Sd"], ys if data else None, None if (full or not data) else t["pattern"],
                                           None if full else t["offset"], None if (full and name != "gaussian") else extra, t["Bm"])
                out["%s %d %d" % (name, full, data)] = [x for x in got if x is not None]
    return out, []


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("d", [1, 5, 8])
def test_the_prediction_entry_keeps_the_memory_contract(d, dt):
    obs = OBS_OF[d]
    inputs = _predict_inputs(d, obs, dt)
    R = sum(LENGTHS)
    ref = _three_runs(_predict_ops, inputs, _out_bytes(5 * 12, 12 * 5 * R * obs * 8), "glm predict d %d obs %d" % (d, obs))
    # what the three runs compared are predictions, not zeros; absent entries have a logpdf of exact zero
    eta_mean, eta_var, mean, var, logpdf = ref["poisson 0 1"]
    assert all(bool(torch.isfinite(x).all()) for x in ref["poisson 0 1"])
    assert float(eta_var.min()) > 0 and float(mean.min()) > 0 and float(var.min()) > 0
    bits = (inputs["pattern"].unsqueeze(-1) >> torch.arange(obs, device="cuda")) & 1
    assert bool((logpdf[bits == 0] == 0).all()) and bool((logpdf[bits == 1] < 0).all())
    assert len(ref["poisson 0 0"]) == 4 and all(torch.equal(a, b) for a, b in zip(ref["poisson 0 0"], ref["poisson 0 1"]))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("d", [1, 5])
def test_a_null_or_misaligned_argument_is_refused_by_name(d, dt):
    obs = OBS_OF[d]
    t = _predict_inputs(d, obs, dt)
    R = sum(LENGTHS)
    a = Arena(8 << 20)
    a.poison(0xFF)
    p = {k: a.put(v, k) for k, v in t.items()}
    outs = ["eta_mean", "eta_var", "mean", "var", "logpdf"]
    o = {k: a.empty((R, obs), dt, k) for k in outs}
    lib, dtc, st = _hip.lib(), _hip.dtype_code(dt), _hip.stream_ptr()
    base = {"zm": p["z"], "zc": p["Sd"], "ys": p["counts"], "pattern": p["pattern"], "offset": p["offset"],
            "extra": p["log_exposure"], "Bmat": p["Bm"], **o}
    order = ["zm", "zc", "ys", "pattern", "offset", "extra", "Bmat"]

    def call(family=_hip.GLM_POISSON, **swap):
        ptrs = {k: _hip.ptr(v) for k, v in base.items()}
        ptrs.update(swap)
        return lib.cgps_leg_glm_predict(*[ptrs[k] for k in order], R, d, obs, dtc, family, *[ptrs[k] for k in outs], st)

    one_in = lambda k: ctypes.c_void_p(base[k].data_ptr() + base[k].element_size())      # noqa: E731  (inside the view)
    odd = lambda k: ctypes.c_void_p(base[k].data_ptr() + 1)                                # noqa: E731  (off its element size)
    before = a.buf.clone()
    refused = [(k, {k: None}, b"NULL") for k in ("zm", "zc", "Bmat", "eta_mean", "eta_var", "mean", "var", "ys", "logpdf")]
    refused += [("zc", {"zc": one_in("zc")}, b"not aligned")]
    refused += [(k, {k: odd(k)}, b"not aligned") for k in ("zm", "ys", "offset", "extra", "Bmat") + tuple(outs)]
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
    assert call(ys=None, logpdf=None, pattern=None) == 0, lib.cgps_last_error()      # ... and so is the one without data
    torch.cuda.synchronize()
    a.assert_guards(0xFF)

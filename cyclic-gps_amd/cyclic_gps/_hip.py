"""ctypes binding of libcgps.so (C ABI: include/cgps.h, and include/cgps_glm.h, include/cgps_glm_grad.h and
include/cgps_glm_predict.h for the extension entry points).

The library is the product: if it is missing this module raises, it never falls
back to a CPU or torch implementation.
"""
import ctypes
import functools
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CGPS_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libcgps.so"))

F32, F64 = 0, 1
OP_MAHAL_LOGDET, OP_DECOMPOSE, OP_HALFSOLVE, OP_BACKSOLVE, OP_SOLVE, OP_LOGDET_FACTOR, OP_INVERSE_BLOCKS, \
    OP_MAHAL_LOGDET_LEVELWISE, OP_DECOMPOSE_SOLVE = range(9)
MAX_LEVELS = 64
ROWS_PLAIN, ROWS_TABLE, ROWS_WEIGHTED = range(3)
H_NONE, H_PLAIN, H_TABLE, H_ROWS = range(4)

_lib = None

_vp, _i64, _int, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
_SIGNATURES = {
    "cgps_version": (_int, []),
    "cgps_last_error": (ctypes.c_char_p, []),
    "cgps_profile_next_call": (_int, [_vp, _vp]),
    "cgps_reset_counters": (_int, [_vp]),
    "cgps_boundary_solve": (_int, [_vp, _sz, _i64, _int, _int, _vp, _vp, _vp]),
    "cgps_boundary_recursions": (_int, [_vp, _sz, _i64, _i64, _int, _int, _vp, _vp, _vp]),
    "cgps_level_layout": (_int, [_i64, ctypes.POINTER(_int)] + [ctypes.POINTER(_i64)] * 4),
    "cgps_workspace_bytes": (_int, [_i64, _int, _int, _int, ctypes.POINTER(_sz)]),
    "cgps_mahal_logdet": (_int, [_vp, _vp, _vp, _i64, _int, _int, _vp, _sz, _vp, _vp, _vp]),
    "cgps_mahal_logdet_levelwise": (_int, [_vp, _vp, _vp, _i64, _int, _int, _vp, _sz, _vp, _vp, _vp]),
    "cgps_decompose_step": (_int, [_vp, _vp, _i64, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cgps_decompose": (_int, [_vp, _vp, _i64, _int, _int, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "cgps_decompose_solve": (_int, [_vp, _vp, _vp, _i64, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "cgps_solve_workspace_bytes": (_int, [_i64, _int, _int, _int, _int, ctypes.POINTER(_sz)]),
    "cgps_halfsolve": (_int, [_vp, _vp, _vp, _i64, _int, _int, _int, _vp, _vp, _vp, _sz, _vp, _vp]),
    "cgps_backsolve": (_int, [_vp, _vp, _vp, _i64, _int, _int, _int, _vp, _vp, _vp, _sz, _vp]),
    "cgps_solve": (_int, [_vp, _vp, _vp, _i64, _int, _int, _int, _vp, _vp, _vp, _sz, _vp]),
    "cgps_normal_fill": (_int, [_vp, _i64, _i64, _int, ctypes.c_uint64, ctypes.c_uint32, _vp]),
    "cgps_sample_workspace_bytes": (_int, [_i64, _int, _int, _i64, ctypes.POINTER(_sz)]),
    "cgps_sample": (_int, [_vp, _vp, _vp, _i64, _int, _int, _i64, _vp, ctypes.c_uint64, ctypes.c_uint32, _vp, _vp, _sz, _vp]),
    "cgps_logdet_factor": (_int, [_vp, _i64, _int, _int, _vp, _sz, _vp, _vp]),
    "cgps_inverse_blocks": (_int, [_vp, _vp, _vp, _i64, _int, _int, _vp, _vp, _vp, _sz, _vp]),
    "cgps_mahal_logdet_adjoint": (_int, [_vp, _vp, _vp, _i64, _int, _int, _vp, _vp, _vp]),
    "cgps_mahal_logdet_batch": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _int, _int, _i64, _vp, _vp, _vp]),
    "cgps_mahal_logdet_adjoint_seg": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _int, _int, _vp, _vp, _vp]),
    "cgps_peg_precision": (_int, [_vp, _vp, _i64, _int, _int, _vp, _vp, _vp, _vp]),
    "cgps_leg_mahal_logdet": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _int, _vp, ctypes.c_size_t, _vp, _vp, _vp]),
    "cgps_leg_mahal_logdet_pair": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _int, _vp, ctypes.c_size_t, _vp, _vp, _vp]),
    "cgps_leg_mahal_logdet_pair_obs": (_int, [_vp, _vp, _vp, _int, _vp, _vp, _i64, _int, _int, _vp, ctypes.c_size_t, _vp, _vp, _vp]),
    "cgps_leg_mahal_logdet_pair_w": (_int, [_vp, _vp, _vp, _int, _vp, _vp, _i64, _int, _int, _vp, ctypes.c_size_t, _vp, _vp, _vp]),
    "cgps_peg_precision_adjoint": (_int, [_vp, _vp, _i64, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    "cgps_leg_loglik_batch": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _int, _int, _i64, _vp, _vp, _vp]),
    "cgps_leg_loglik_batch_obs": (_int, [_vp, _vp, _i64, _vp, _vp, _int, _vp, _vp, _vp, _int, _int, _i64, _vp, _vp, _vp]),
    "cgps_leg_loglik_batch_w": (_int, [_vp, _vp, _i64, _vp, _vp, _int, _vp, _vp, _vp, _int, _int, _i64, _vp, _vp, _vp]),
    "cgps_peg_precision_seg": (_int, [_vp, _vp, _vp, _i64, _int, _int, _vp, _vp, _vp, _vp]),
    "cgps_peg_precision_adjoint_seg": (_int, [_vp, _vp, _vp, _i64, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    "cgps_leg_loglik_models": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _int, _int, _i64, _vp, _vp, _vp]),
    "cgps_leg_loglik_models_obs": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _int, _vp, _vp, _vp, _int, _int, _i64, _vp, _vp, _vp]),
    "cgps_leg_loglik_models_w": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _int, _vp, _vp, _vp, _int, _int, _i64, _vp, _vp, _vp]),
    "cgps_peg_precision_models": (_int, [_vp, _vp, _vp, _i64, _i64, _int, _int, _vp, _vp, _vp, _vp]),
    "cgps_peg_precision_adjoint_models": (_int, [_vp, _vp, _vp, _i64, _i64, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    "cgps_leg_intercast": (_int, [_vp, _i64, _vp, _i64, _vp, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cgps_leg_intercast_seg": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cgps_leg_posterior_blocks_seg": (_int, [_vp, _vp, _vp, _i64, _int, _int, _int, _vp, _int, _vp, _vp, _vp, _vp, _vp]),
    "cgps_leg_posterior_blocks_models": (_int, [_vp, _vp, _vp, _i64, _i64, _int, _int, _int, _vp, _int, _vp, _vp, _vp, _vp, _vp]),
    "cgps_leg_intercast_models": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cgps_leg_perturbation_seg": (_int, [_vp, _i64, _vp, _int, _int, _vp, _vp, _i64, _int, _vp, _int, _int, _vp, _vp, _i64,
                                         ctypes.c_uint64, ctypes.c_uint32, _vp, _vp, _vp]),
    "cgps_leg_perturbation_models": (_int, [_vp, _i64, _i64, _vp, _int, _int, _vp, _vp, _i64, _int, _vp, _int, _int, _vp, _vp,
                                            _i64, ctypes.c_uint64, _vp, _vp, _vp, _vp]),
    "cgps_leg_observations": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _int, _int, _int, _i64,
                                     ctypes.c_uint64, _vp, _vp, _vp, _vp]),
    "cgps_leg_loo": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _int, _int, _int, _vp, _vp, _int, _vp, _vp, _vp,
                            _vp, _vp, _vp]),
    "cgps_leg_filter": (_int, [_vp] * 5 + [_i64] * 3 + [_vp] * 3 + [_int] * 3 + [_vp] * 13),
    "cgps_leg_filter_scan_workspace_bytes": (_int, [_i64, _i64, _int, _int, _i64, ctypes.POINTER(_sz)]),
    "cgps_leg_filter_scan": (_int, [_vp] * 5 + [_i64] * 3 + [_vp] * 3 + [_int] * 3 + [_vp] * 6 + [_i64] * 3 + [_vp, _sz]
                             + [_vp] * 10),
    "cgps_leg_filter_adjoint_workspace_bytes": (_int, [_i64, _i64, _i64, _int, _int, _int, ctypes.POINTER(_sz)]),
    "cgps_leg_filter_adjoint": (_int, [_vp] * 4 + [_i64] * 3 + [_vp] * 3 + [_int] * 3 + [_vp] * 11 + [_sz] + [_vp] * 9),
    "cgps_record_elems":(_int, [_int, _int, ctypes.POINTER(_i64)]),
    "cgps_shard_reduce": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _int, _vp, _sz, _vp, _vp, _vp]),
    "cgps_finish_records": (_int, [_vp, _sz, _vp, _sz, _i64, _i64, _i64, _int, _int, _vp, _vp, _vp]),
}

# Entry points declared in include/cgps_glm.h: the same library, a table of their own
_EXTENSION_SIGNATURES = {
    "cgps_leg_glm_step": (_int, [_vp] * 10 + [_i64] * 2 + [_int] * 4 + [ctypes.c_double] + [_vp] * 6),
}
# Entry points declared in include/cgps_glm_grad.h (the gradient of the Laplace evidence): a third table
_GLM_GRADIENT_SIGNATURES = {
    "cgps_leg_glm_evidence_rhs": (_int, [_vp] * 7 + [_i64] + [_int] * 4 + [_vp] * 2),
    "cgps_leg_glm_evidence_adjoint": (_int, [_vp] * 13 + [_i64] * 2 + [_int] * 4 + [_vp] * 6),
}
# The entry point declared in include/cgps_glm_predict.h (predictions on the response scale): a fourth table
_GLM_PREDICT_SIGNATURES = {
    "cgps_leg_glm_predict": (_int, [_vp] * 7 + [_i64] + [_int] * 4 + [_vp] * 6),
}
GLM_POISSON, GLM_BERNOULLI, GLM_GAUSSIAN = range(3)
GLM_CONVERGED, GLM_STALLED = 1, 2
GLM_STATE = 4


class CgpsError(RuntimeError):
    pass


def exported_symbols():
    return sorted(_SIGNATURES)


def extension_symbols():
    """the entry points of include/cgps_glm.h"""
    return sorted(_EXTENSION_SIGNATURES)


def glm_gradient_symbols():
    """the entry points of include/cgps_glm_grad.h"""
    return sorted(_GLM_GRADIENT_SIGNATURES)


def glm_predict_symbols():
    """the entry points of include/cgps_glm_predict.h"""
    return sorted(_GLM_PREDICT_SIGNATURES)


def lib():
    """Load libcgps.so once; raise loudly when it is not there."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CgpsError(
                "libcgps.so not found at %s -- build it with `python __graft_entry__.py` "
                "(there is no CPU fallback)" % LIB_PATH)
        # libcgps needs libamdhip64.so.7; torch ships its own copy under that soname and must be
        # the one runtime in the process (its streams/pointers are what we are handed), so make
        # sure it is resident before the loader resolves our dependency.
        rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if os.path.exists(rt):
            ctypes.CDLL(rt, mode=ctypes.RTLD_GLOBAL)
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in list(_SIGNATURES.items()) + list(_EXTENSION_SIGNATURES.items()) + list(
                _GLM_GRADIENT_SIGNATURES.items()) + list(_GLM_PREDICT_SIGNATURES.items()):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise CgpsError("libcgps error %d: %s" % (rc, lib().cgps_last_error().decode()))


def dtype_code(dt):
    if dt == torch.float32:
        return F32
    if dt == torch.float64:
        return F64
    raise TypeError("cyclic reduction supports float32 / float64 blocks, got %s" % dt)


def ptr(t):
    return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=512)
def _level_layout_cached(N):
    n = _int(0)
    arrs = [(ctypes.c_int64 * (MAX_LEVELS + 1))() for _ in range(4)]
    check(lib().cgps_level_layout(N, ctypes.byref(n), *arrs))
    L = n.value
    return (tuple(arrs[0][:L]), tuple(arrs[1][:L + 1]), tuple(arrs[2][:L + 1]), tuple(arrs[3][:L + 1]))


def level_layout(N):
    """(ms, offD, offF, offG) python lists; offsets have one extra entry (the total)."""
    return tuple(list(t) for t in _level_layout_cached(int(N)))


@functools.lru_cache(maxsize=2048)
def _workspace_bytes(N, d, dtc, op, nrhs=1):
    b = _sz(0)
    if nrhs == 1:
        check(lib().cgps_workspace_bytes(N, d, dtc, op, ctypes.byref(b)))
    else:
        check(lib().cgps_solve_workspace_bytes(N, d, dtc, op, nrhs, ctypes.byref(b)))
    return b.value


_ws_cache, _pair_ws_cache = {}, {}


def _scratch(cache, nbytes, device):
    key = (device, torch.cuda.current_stream().cuda_stream)
    cur = cache.get(key)
    if cur is None or cur.numel() < nbytes:
        cur = cache[key] = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
    return cur


def workspace(N, d, dt, op, device, nrhs=1):
    """A cached scratch tensor of the size the library asks for (torch owns the memory)."""
    nbytes = _workspace_bytes(int(N), int(d), dtype_code(dt), int(op), int(nrhs))
    return _scratch(_ws_cache, nbytes, device), nbytes


@functools.lru_cache(maxsize=512)
def _sample_workspace_bytes(N, d, dtc, nrhs):
    b = _sz(0)
    check(lib().cgps_sample_workspace_bytes(N, d, dtc, nrhs, ctypes.byref(b)))
    return b.value


def sample_workspace(N, d, dt, nrhs, device):
    """The same for cgps_sample (its own carve-up: sample_ws in csrc/cgps_plan.h)."""
    nbytes = _sample_workspace_bytes(int(N), int(d), dtype_code(dt), int(nrhs))
    return _scratch(_ws_cache, nbytes, device), nbytes


@functools.lru_cache(maxsize=512)
def filter_scan_workspace_bytes(n_chunks, M, d, dtc, fanout):
    """What cgps_leg_filter_scan asks for (filter_scan_ws in csrc/cgps_plan.h); host arithmetic, no GPU needed."""
    b = _sz(0)
    check(lib().cgps_leg_filter_scan_workspace_bytes(n_chunks, M, d, dtc, fanout, ctypes.byref(b)))
    return b.value


def filter_scan_workspace(n_chunks, M, d, dt, fanout, device):
    """A cached scratch tensor for cgps_leg_filter_scan and its byte count."""
    nbytes = filter_scan_workspace_bytes(int(n_chunks), int(M), int(d), dtype_code(dt), int(fanout))
    return _scratch(_ws_cache, nbytes, device), nbytes


@functools.lru_cache(maxsize=512)
def filter_adjoint_workspace_bytes(R, B, M, d, obs, dtc):
    """What cgps_leg_filter_adjoint asks for (filter_adjoint_ws_bytes in csrc/cgps_plan.h); host arithmetic."""
    b = _sz(0)
    check(lib().cgps_leg_filter_adjoint_workspace_bytes(R, B, M, d, obs, dtc, ctypes.byref(b)))
    return b.value


def filter_adjoint_workspace(R, B, M, d, obs, dt, device):
    """A cached scratch tensor for cgps_leg_filter_adjoint and its byte count."""
    nbytes = filter_adjoint_workspace_bytes(int(R), int(B), int(M), int(d), int(obs), dtype_code(dt))
    return _scratch(_ws_cache, nbytes, device), nbytes


def pair_workspace_bytes(N, d, dt):
    """What cgps_leg_mahal_logdet_pair asks for: two fused pipelines, each rounded up to 256 bytes (tile_pair_ws in
    csrc/cgps_plan.h is the layout run_tile_leg cuts up; include/cgps.h states the size)."""
    return 2 * ((_workspace_bytes(int(N), int(d), dtype_code(dt), OP_MAHAL_LOGDET) + 255) // 256 * 256)


def pair_workspace(N, d, dt, device):
    """A cached scratch tensor of at least pair_workspace_bytes(N, d, dt) bytes."""
    return _scratch(_pair_ws_cache, pair_workspace_bytes(N, d, dt), device)

"""Child process of tests/test_fold_register_stages.py: the one-launch solve + log-det through the C ABI on seeded
systems, results saved to the .npz named on the command line.  The library reads CGPS_FOLD_REG once per process, so the
test starts this script twice, once with CGPS_FOLD_REG=0 (record stages through the LDS tile)."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cyclic-gps_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import _util  # noqa: E402
from cyclic_gps import _hip, sharded  # noqa: E402

D = 4
ROWS = [2049, 4096, 4097, 8191, 8449, 65535, 65536, 2 ** 19 + 1, 2 ** 20]
SHARD_ROWS = 8449


def mahal_logdet(Rs, Os, b):
    """(out2, info) of cgps_mahal_logdet, nothing raised"""
    n = Rs.shape[0]
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws, nbytes = _hip.workspace(n, D, Rs.dtype, _hip.OP_MAHAL_LOGDET, Rs.device)
    _hip.check(_hip.lib().cgps_mahal_logdet(_hip.ptr(Rs), _hip.ptr(Os), _hip.ptr(b), n, D, _hip.dtype_code(Rs.dtype),
                                            _hip.ptr(ws), nbytes, _hip.ptr(out), _hip.ptr(info), _hip.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(info.item())


def indefinite_system(n, row):
    Rs, Os, b, _, _ = _util.conditioned_system(n, D, seed=300 + row, device="cuda")
    Rs[row] = -Rs[row]
    return Rs, Os, b


def shard_record(n):
    """record and partial result of one n-row shard with a left coupling (cgps_shard_reduce)"""
    Rs, Os, b, _, _ = _util.conditioned_system(n + 1, D, seed=77, device="cuda")
    rec_bytes, msg_bytes = sharded.message_layout(D, torch.float64)
    send = torch.zeros(msg_bytes, dtype=torch.uint8, device="cuda")
    ops = sharded.HipShardOps(n, D, torch.float64, "cuda")
    ops.shard_reduce(Rs[1:].contiguous(), Os[1:].contiguous(), b[1:].contiguous(), Os[0].contiguous(), send, rec_bytes)
    torch.cuda.synchronize()
    return send.view(torch.float64).cpu().numpy()


def main(path):
    res = {}
    for n in ROWS:
        Rs, Os, b, _, _ = _util.conditioned_system(n, D, seed=100 + n, device="cuda")
        res["out_%d" % n], res["info_%d" % n] = mahal_logdet(Rs, Os, b)
    for name, row in (("first", 100), ("last", 4096)):
        res["fail_out_" + name], res["fail_info_" + name] = mahal_logdet(*indefinite_system(4097, row))
    res["shard"] = shard_record(SHARD_ROWS)
    np.savez(path, **res)


if __name__ == "__main__":
    main(sys.argv[1])

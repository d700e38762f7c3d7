"""Child process of tests/test_wave_levels.py: the one-launch solve + log-det through the C ABI on seeded systems,
results saved to the .npz named on the command line.  The library reads CGPS_WAVE_LEVELS once per process, so the test
starts this script twice, once with CGPS_WAVE_LEVELS=0 (every tile staged in LDS before its first level)."""
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
import cyclic_gps.cyclic_reduction as cr  # noqa: E402

D = 4
RAGGED = [4096 + r for r in (1, 2, 7, 8, 9, 63, 64, 65, 255)]
ROWS = [1024, 2048, 2304] + RAGGED + [65536, 2 ** 19 + 1, 2 ** 20, 2 ** 21]
# (name, rows, row made indefinite): the kept row of lane 0 of a full tile at 4 and at 8 rows per lane, a row that
# lane streams through, and the kept row of lane 0 of the fourth of 65 full tiles (4 rows per lane)
FAILS = [("kept4", 1024, 3), ("streamed", 1024, 1), ("kept8", 2048, 7), ("tile3", 66560, 3 * 1024 + 3)]
SHARDS = [8449, 2 ** 21]
SHARD_LEFT_ROWS = 300            # rows of the shard on the left


def mahal_logdet(Rs, Os, b, ws=None):
    """(out2, info) of cgps_mahal_logdet, nothing raised; ws: (workspace, bytes) of at least this size"""
    n = Rs.shape[0]
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws, nbytes = ws if ws is not None else _hip.workspace(n, D, Rs.dtype, _hip.OP_MAHAL_LOGDET, Rs.device)
    _hip.check(_hip.lib().cgps_mahal_logdet(_hip.ptr(Rs), _hip.ptr(Os), _hip.ptr(b), n, D, _hip.dtype_code(Rs.dtype),
                                            _hip.ptr(ws), nbytes, _hip.ptr(out), _hip.ptr(info), _hip.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(info.item())


def system(n):
    return _util.conditioned_system(n, D, seed=100 + n, device="cuda")[:3]


def indefinite_system(n, row):
    Rs, Os, b, _, _ = _util.conditioned_system(n, D, seed=300 + row, device="cuda")
    Rs[row] = -Rs[row]
    return Rs, Os, b


def sharded_and_whole(n):
    """out2 of a system of SHARD_LEFT_ROWS + n rows reduced as two shards (cgps_shard_reduce on each, the second with
    its left coupling, then cgps_finish_records), and out2 of the same system in one call"""
    m = SHARD_LEFT_ROWS
    Rs, Os, b, _, _ = _util.conditioned_system(m + n, D, seed=77 + n, device="cuda")
    rec_bytes, msg_bytes = sharded.message_layout(D, torch.float64)
    msgs = torch.zeros(2 * msg_bytes, dtype=torch.uint8, device="cuda")
    left = sharded.HipShardOps(m, D, torch.float64, "cuda")
    left.shard_reduce(Rs[:m].contiguous(), Os[:m - 1].contiguous(), b[:m].contiguous(), None, msgs[:msg_bytes], rec_bytes)
    right = sharded.HipShardOps(n, D, torch.float64, "cuda")
    right.shard_reduce(Rs[m:].contiguous(), Os[m:].contiguous(), b[m:].contiguous(), Os[m - 1].contiguous(), msgs[msg_bytes:],
                       rec_bytes)
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    right.finish(msgs, 2, rec_bytes, msg_bytes, n, m + n, out)
    torch.cuda.synchronize()
    assert int(right.info.item()) == 0
    whole, info = mahal_logdet(Rs, Os, b)
    assert info == 0
    return out.cpu().numpy(), whole


def main(path):
    res = {}
    for n in ROWS:
        res["out_%d" % n], res["info_%d" % n] = mahal_logdet(*system(n))
    for name, n, row in FAILS:
        res["fail_out_" + name], res["fail_info_" + name] = mahal_logdet(*indefinite_system(n, row))
        try:
            cr.mahal_and_det(*indefinite_system(n, row))
            res["fail_raised_" + name] = np.array(0)
        except cr.NotPSDError:
            res["fail_raised_" + name] = np.array(1)
    for n in SHARDS:
        res["shard_%d" % n], res["whole_%d" % n] = sharded_and_whole(n)
    np.savez(path, **res)


if __name__ == "__main__":
    main(sys.argv[1])

"""numpy restatement of the generator specification (csrc/cgps_rng.h), written from the specification:
Philox4x32-10, key = (seed lo, seed hi), counter = (r lo, r hi, column group, stream), Box-Muller on 53-bit (fp64:
two columns per block) or 24-bit (fp32: four columns per block) uniforms.  Everything is evaluated in float64; for
fp32 that is the float64 evaluation of the same u1, u2 the fp32 code uses."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable), key: two python ints -> four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                      # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def _words(rows, groups, seed, stream, row0=0):
    r = (np.arange(rows, dtype=np.uint64) + np.uint64(row0))[:, None]
    g = np.arange(groups, dtype=np.uint64)[None, :]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10((r & MASK, r >> S32, g, np.uint64(int(stream) & 0xFFFFFFFF)), (seed & 0xFFFFFFFF, seed >> 32))


def _box_muller(u1, u2):
    rho = np.sqrt(-2.0 * np.log(u1))
    return rho * np.cos(2.0 * np.pi * u2), rho * np.sin(2.0 * np.pi * u2)


def standard_normal(rows, cols, seed, stream=0, dtype=np.float64, row0=0):
    """[rows, cols] float64: the normals of row-elements row0 .. row0 + rows - 1 as the dtype's generator defines them."""
    if np.dtype(dtype) == np.float64:
        groups = (cols + 1) // 2
        w = [x.astype(np.uint64) for x in _words(rows, groups, seed, stream, row0)]
        k1 = (w[0] >> np.uint64(6)) * np.uint64(1 << 27) + (w[1] >> np.uint64(5))
        k2 = (w[2] >> np.uint64(6)) * np.uint64(1 << 27) + (w[3] >> np.uint64(5))
        zc, zs = _box_muller((k1.astype(np.float64) + 1.0) * 2.0 ** -53, k2.astype(np.float64) * 2.0 ** -53)
        out = np.stack([zc, zs], axis=-1).reshape(rows, 2 * groups)
    else:
        groups = (cols + 3) // 4
        w = [x.astype(np.uint64) for x in _words(rows, groups, seed, stream, row0)]
        u = lambda a, one: ((a >> np.uint64(8)).astype(np.float64) + one) * 2.0 ** -24   # noqa: E731
        a0, a1 = _box_muller(u(w[0], 1.0), u(w[1], 0.0))
        a2, a3 = _box_muller(u(w[2], 1.0), u(w[3], 0.0))
        out = np.stack([a0, a1, a2, a3], axis=-1).reshape(rows, 4 * groups)
    return np.ascontiguousarray(out[:, :cols])


KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

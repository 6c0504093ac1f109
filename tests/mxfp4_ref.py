"""OCP MXFP4 weight quantisation, restated in numpy (the format of include/zoomearth.h, the arithmetic of k_quantize_mxfp4).

A bf16 matrix W [N, K], K % 32 == 0, is cut into blocks of 32 consecutive k of a row.  Per block: amax = max |w|,
e = floor(log2(amax)) - 2 clamped to [E_MIN, E_MAX] = [-125, 125] (every code * 2^e is then a normal bf16), e = 0 for an all-zero
block; the scale byte is e + 127.  An element is w / 2^e rounded to the nearest of CODE_VALUES, ties to the even code, magnitudes
above 6 saturate, the sign is kept (-0 is code 8).  q [N, K / 2] holds the even k in the low nibble, scale is [N, K / 32].

Everything here is exact: w / 2^e is a power-of-two scaling in float64, the tie points are compared exactly."""
import numpy as np

CODE_VALUES = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
E_MIN, E_MAX = -125, 125
# a magnitude v (in units of 2^e) goes up one code above each of TIES_ABOVE and at or above each of TIES_AT_OR_ABOVE: the tie points,
# each resolved towards the even code
TIES_ABOVE = (0.25, 1.25, 2.5, 5.0)
TIES_AT_OR_ABOVE = (0.75, 1.75, 3.5)


def bf16_round_trip(x):
    """float values -> nearest-even bf16 -> float32 (numpy only)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


def block_exponent(amax):
    """amax >= 0 (float64 array) -> e"""
    with np.errstate(divide="ignore"):
        fl = np.floor(np.log2(np.where(amax > 0, amax, 1.0)))
    # floor(log2) through frexp: exact for every float (log2 of a value just below a power of two may round up)
    m, ex = np.frexp(np.where(amax > 0, amax, 1.0))
    fl = ex - 1
    e = np.clip(fl - 2, E_MIN, E_MAX)
    return np.where(amax > 0, e, 0).astype(np.int64)


def quantize(w):
    """w: float array [N, K] of bf16-representable finite values -> (q u8 [N, K/2], scale u8 [N, K/32], dequantised f32 [N, K])"""
    w = np.asarray(w, dtype=np.float64)
    n, k = w.shape
    assert k % 32 == 0
    blocks = w.reshape(n, k // 32, 32)
    e = block_exponent(np.abs(blocks).max(axis=2))                       # [N, K/32]
    v = np.abs(blocks) * np.exp2(-e.astype(np.float64))[:, :, None]       # exact: a power-of-two scaling
    code = np.zeros(v.shape, dtype=np.int64)
    for t in TIES_ABOVE:
        code += v > t
    for t in TIES_AT_OR_ABOVE:
        code += v >= t
    sign = np.signbit(blocks)
    nib = (code | (sign.astype(np.int64) << 3)).reshape(n, k)
    q = (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8)
    scale = (e + 127).astype(np.uint8)
    return q, scale, dequantize(q, scale)


def dequantize(q, scale):
    """(q u8 [N, K/2], scale u8 [N, K/32]) -> f32 [N, K]: code * 2^e, sign kept (code 8 is -0)"""
    q = np.asarray(q, dtype=np.uint8)
    n = q.shape[0]
    nib = np.empty((n, q.shape[1] * 2), dtype=np.int64)
    nib[:, 0::2] = q & 15
    nib[:, 1::2] = q >> 4
    mag = CODE_VALUES[nib & 7]
    val = np.where(nib & 8, -mag, mag)
    e = np.asarray(scale, dtype=np.int64) - 127
    out = val.reshape(n, -1, 32) * np.exp2(e.astype(np.float64))[:, :, None]
    return out.reshape(n, -1).astype(np.float32)


def hand_blocks():
    """The hand-written blocks of the issue, one per row: (name, 32 values).  Every value is a bf16."""
    z = np.zeros(32)

    def blk(*head):
        b = z.copy()
        b[:len(head)] = head
        return b
    rows = [
        ("all zeros", z.copy()),
        ("amax an exact power of two", blk(4.0, -2.0, 1.0, 0.5, 0.25, 3.0, -4.0, 0.125)),
        # e = 0 (amax 4): every tie of the grid, both signs
        ("every tie", blk(4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5)),
        # amax 5 and 7.5: e = 0, amax / 2^e in [4, 8): 5 ties down to 4, (6, 8) saturates to 6
        ("tie at five", blk(5.0, -5.0, 4.5, 5.5, 6.0)),
        ("saturation", blk(7.5, -7.0, 6.5, 6.0, 5.0, -7.96875)),
        ("minus zero", blk(1.0, -0.0, 0.0, -0.125, -1.0)),
        # clamp ends: amax below 2^-123 takes e = -125; amax 2^127 * 1.5 wants e = 125 exactly; the largest bf16 saturates at 6 * 2^125
        ("low clamp", blk(2.0 ** -126, 2.0 ** -125 * 1.5, -(2.0 ** -127), 2.0 ** -133, 2.0 ** -124)),
        ("low clamp, subnormal amax", blk(2.0 ** -130, -(2.0 ** -133))),
        ("high clamp", blk(2.0 ** 127 * 1.9921875, -(2.0 ** 127), 2.0 ** 125, 2.0 ** 123, 2.0 ** 126 * 1.25)),
        ("small block scale", blk(0.01171875, -0.0078125, 0.00390625, 0.0087890625)),
    ]
    return rows

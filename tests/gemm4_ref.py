"""The fragment-major MXFP4 copy of the batched decode step, restated in numpy (the layout of include/zoomearth.h, the moves of
k_pack_fragments4 in ze_quant.hip).  The format itself -- codes, scales, the quantiser -- is tests/mxfp4_ref.py.

W [N, K], N % 16 == 0, K % 32 == 0, S = K / 32 slices, nb = row / 16, ks = k / 32:
  codes  u8 [N / 16][S][64][4]: lane = (k % 32) / 8 * 16 + row % 16 holds q[row][k / 2 .. + 3] for k = 32 ks + 8 (lane / 16), unchanged
         (the even k in the low nibble): the lane's 8 codes of one 16 x 32 MFMA fragment, 256 B per fragment;
  scales u8 [N / 16][S][16]: byte (nb, ks, r) = scale[row r of block nb][ks].
rope_dim = D > 0 (the qkv projection): block nb = head h = nb / (D / 16), group j = nb % (D / 16) holds rows h D + 8 j .. + 7 and
h D + D / 2 + 8 j .. + 7, as the bf16 and FP8 fragment copies do."""
import numpy as np


def block_rows(n, rope_dim=0):
    """[N / 16, 16]: the weight row that sits at position r of fragment block nb"""
    assert n % 16 == 0
    nb, r = np.meshgrid(np.arange(n // 16), np.arange(16), indexing="ij")
    if rope_dim <= 0:
        return nb * 16 + r
    assert n % rope_dim == 0 and rope_dim % 16 == 0
    bph = rope_dim // 16
    h, j = nb // bph, nb % bph
    return h * rope_dim + np.where(r < 8, 8 * j + r, rope_dim // 2 + 8 * j + (r - 8))


def pack(q, scale, rope_dim=0):
    """q [N, K / 2], scale [N, K / 32] (any integer dtype: the test packs position numbers too) -> (codes [N / 16, S, 64, 4],
    scales [N / 16, S, 16])"""
    q, scale = np.asarray(q), np.asarray(scale)
    n, s = scale.shape
    assert q.shape == (n, 16 * s)
    rows = block_rows(n, rope_dim)                                  # [nb, 16]
    codes = np.empty((n // 16, s, 64, 4), dtype=q.dtype)
    for fq in range(4):
        # lanes 16 fq .. + 15: bytes 16 ks + 4 fq .. + 3 of their rows
        piece = q.reshape(n, s, 4, 4)[:, :, fq, :][rows]            # [nb, 16, S, 4]
        codes[:, :, 16 * fq:16 * fq + 16, :] = piece.transpose(0, 2, 1, 3)
    scales = scale[rows, :].transpose(0, 2, 1).copy()               # [nb, S, 16]
    return codes, scales


def unpack(codes, scales, rope_dim=0):
    """The inverse of pack: (q [N, K / 2], scale [N, K / 32])"""
    codes, scales = np.asarray(codes), np.asarray(scales)
    nblk, s = scales.shape[:2]
    n = nblk * 16
    rows = block_rows(n, rope_dim)
    q = np.empty((n, s, 4, 4), dtype=codes.dtype)
    for fq in range(4):
        piece = np.empty((n, s, 4), dtype=codes.dtype)
        piece[rows] = codes[:, :, 16 * fq:16 * fq + 16, :].transpose(0, 2, 1, 3)
        q[:, :, fq, :] = piece
    scale = np.empty((n, s), dtype=scales.dtype)
    scale[rows, :] = scales.transpose(0, 2, 1)
    return q.reshape(n, 16 * s), scale


def fragment_bytes(n, k):
    """bytes of the copy of one [n, k] tensor: 4 bits + 1/32 byte per weight"""
    return n * k // 2 + n * k // 32

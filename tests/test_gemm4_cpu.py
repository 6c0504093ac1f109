"""CPU checks of the MXFP4 fragment stream of the batched decode step: the fragment-major layout restated in numpy
(tests/gemm4_ref.py) is a bijection that unpacks to the canonical q / scale, and the two new C entries are declared, bound and
exported."""
import os
import re

import numpy as np
import pytest

import gemm4_ref as G
import mxfp4_ref as R
from zoomearth_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(n, k) for k in (32, 160, 2048) for n in (16, 96)]


def operands(n, k, seed):
    rng = np.random.default_rng(seed)
    w = R.bf16_round_trip(rng.standard_normal((n, k)) * np.exp2(rng.integers(-6, 7, size=(n, 1))))
    q, scale, _ = R.quantize(w)
    return q, scale


@pytest.mark.parametrize("n,k", SHAPES)
def test_unpacking_the_packed_copy_gives_q_and_scale(n, k):
    q, scale = operands(n, k, 1000 * n + k)
    codes, scales = G.pack(q, scale)
    assert codes.dtype == np.uint8 and codes.shape == (n // 16, k // 32, 64, 4) and scales.shape == (n // 16, k // 32, 16)
    assert codes.size + scales.size == G.fragment_bytes(n, k)
    q2, s2 = G.unpack(codes, scales)
    assert np.array_equal(q2, q) and np.array_equal(s2, scale)
    # the layout in the header's words, element by element, on a sample: lane = (k % 32) / 8 * 16 + row % 16 holds q[row][k / 2 .. + 3]
    rng = np.random.default_rng(7)
    for _ in range(200):
        row, kk = int(rng.integers(n)), int(rng.integers(k // 8)) * 8
        lane = (kk % 32) // 8 * 16 + row % 16
        assert np.array_equal(codes[row // 16, kk // 32, lane], q[row, kk // 2:kk // 2 + 4])
        assert scales[row // 16, kk // 32, row % 16] == scale[row, kk // 32]


def test_the_qkv_copy_follows_the_row_permutation_of_the_other_fragment_copies():
    n, k, d = 256, 64, 128
    q, scale = operands(n, k, 5)
    codes, scales = G.pack(q, scale, rope_dim=d)
    rows = G.block_rows(n, d)
    assert sorted(rows.ravel().tolist()) == list(range(n))
    # block 9 = head 1, group 1: dims 8 .. 15 and 72 .. 79 of head 1
    assert rows[9].tolist() == [128 + 8 + i for i in range(8)] + [128 + 72 + i for i in range(8)]
    assert np.array_equal(codes[9, 1, 16 * 2 + 11], q[128 + 72 + 3, 16 + 8:16 + 12]) and scales[9, 1, 11] == scale[128 + 72 + 3, 1]
    q2, s2 = G.unpack(codes, scales, rope_dim=d)
    assert np.array_equal(q2, q) and np.array_equal(s2, scale)


@pytest.mark.parametrize("n,k", SHAPES)
def test_every_swap_in_the_layout_changes_the_unpacked_matrix(n, k):
    """Packing POSITION NUMBERS shows where every packed nibble and scale byte comes from: each source position appears exactly once
    (a bijection), so exchanging two packed nibbles / scale bytes exchanges two different positions of the unpacked matrix -- it
    changes whenever the two hold different values.  Checked on the maps for every pair at once, and on real operands for a sample
    of swaps (every neighbouring pair of the smallest shape)."""
    nib_id = np.arange(n * k, dtype=np.int64).reshape(n, k)            # nibble (row, k)
    # a byte of q holds nibbles (2 b, 2 b + 1): pack the byte numbers, then expand
    byte_id = np.arange(n * k // 2, dtype=np.int64).reshape(n, k // 2)
    sc_id = np.arange(n * k // 32, dtype=np.int64).reshape(n, k // 32)
    cid, sid = G.pack(byte_id, sc_id)
    assert sorted(cid.ravel().tolist()) == list(range(n * k // 2)) and sorted(sid.ravel().tolist()) == list(range(n * k // 32))
    assert nib_id.size == 2 * cid.size
    q, scale = operands(n, k, 31 * n + k)
    codes, scales = G.pack(q, scale)
    flat_n = np.stack([codes.ravel() & 15, codes.ravel() >> 4], axis=1).ravel()   # packed nibbles in memory order, low first
    rng = np.random.default_rng(n + k)
    pairs = [(i, i + 1) for i in range(flat_n.size - 1)] if n * k <= 512 else []
    pairs += [tuple(rng.integers(flat_n.size, size=2)) for _ in range(300)]
    tried = 0
    for i, j in pairs:
        if flat_n[i] == flat_n[j]:
            continue
        f = flat_n.copy()
        f[i], f[j] = f[j], f[i]
        c2 = (f[0::2] | (f[1::2] << 4)).astype(np.uint8).reshape(codes.shape)
        q2, _ = G.unpack(c2, scales)
        assert (q2 != q).sum() in (1, 2)                                # the one or two bytes that hold the exchanged nibbles
        tried += 1
    assert tried > 100
    fs = scales.ravel()
    tried = 0
    for i, j in [(i, i + 1) for i in range(min(fs.size - 1, 200))] + [tuple(rng.integers(fs.size, size=2)) for _ in range(200)]:
        if fs[i] == fs[j]:
            continue
        f = fs.copy()
        f[i], f[j] = f[j], f[i]
        _, s2 = G.unpack(codes, f.reshape(scales.shape))
        assert (s2 != scale).sum() == 2
        tried += 1
    assert tried > 50


def test_the_two_entries_are_exported_and_bound():
    """Fails on a tree without the feature: the symbols are neither declared, bound nor in the library."""
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "zoomearth.h")).read()
    for name, nargs in (("ze_op_gemm4", 16), ("ze_fragment_bytes", 2)):
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert len(fn.argtypes) == nargs
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", hdr, flags=re.M | re.S)
        assert m is not None and len(m.group(1).split(",")) == nargs
    assert len(lib.ze_op_gemm.argtypes) == 17                      # (ze_op_gemm's own signature did not change)
    assert lib.ze_op_gemm4(None, 5, 0, None, 0, None, None, None, None, 0, None, 0, 1, 16, 32, None) < 0   # refused on the host
    assert lib.ze_fragment_bytes(None, None) < 0
    assert lib.ze_tune(24, 0) == 0 and lib.ze_tune(25, 0) < 0       # the new knob is the last one

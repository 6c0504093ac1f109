"""CPU: the MXFP4 weight format (tests/mxfp4_ref.py, the numpy statement of include/zoomearth.h's) on hand-written blocks, and the
three new entries of the C ABI (exported by the built library, bound with the header's argument counts)."""
import os
import re

import numpy as np
import pytest

import mxfp4_ref as R
from conftest import ROOT

from zoomearth_amd import _lib

BLOCKS = dict(R.hand_blocks())


def quant_row(name):
    q, s, dq = R.quantize(BLOCKS[name][None, :])
    nib = np.empty(32, dtype=np.int64)
    nib[0::2], nib[1::2] = q[0] & 15, q[0] >> 4
    return nib, int(s[0, 0]), dq[0]


def test_hand_blocks_are_bf16_values():
    w = np.stack(list(BLOCKS.values()))
    assert np.array_equal(R.bf16_round_trip(w).astype(np.float64), w)


def test_all_zero_block_takes_e_zero():
    nib, s, dq = quant_row("all zeros")
    assert s == 127 and not nib.any() and not dq.any()


def test_power_of_two_amax():
    nib, s, dq = quant_row("amax an exact power of two")       # amax 4 = 2^2: e = 0, 4 is code 6
    assert s == 127
    assert nib[:8].tolist() == [6, 8 | 4, 2, 1, 0, 5, 8 | 6, 0]  # 0.25 and 0.125 go to 0 (0.25 is the tie below 0.5)
    assert dq[:8].tolist() == [4.0, -2.0, 1.0, 0.5, 0.0, 3.0, -4.0, 0.0]


def test_every_tie_goes_to_the_even_code():
    nib, s, dq = quant_row("every tie")
    assert s == 127
    #                       4   .25 .75 1.25 1.75 2.5 3.5
    assert dq[:7].tolist() == [4.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0]
    assert nib[:7].tolist() == [6, 0, 2, 2, 4, 4, 6]
    assert dq[7:13].tolist() == [-0.0, -1.0, -1.0, -2.0, -2.0, -4.0] and np.signbit(dq[7:13]).all()
    assert nib[7:13].tolist() == [8, 10, 10, 12, 12, 14]
    nib, s, dq = quant_row("tie at five")                       # 5 -> 4 (code 6, even), 4.5 -> 4, 5.5 -> 6
    assert s == 127 and dq[:5].tolist() == [4.0, -4.0, 4.0, 6.0, 6.0] and nib[:5].tolist() == [6, 14, 6, 7, 7]


def test_magnitudes_between_six_and_eight_saturate():
    nib, s, dq = quant_row("saturation")                        # amax 7.96875: floor(log2) = 2, e = 0, amax / 2^e in (6, 8)
    assert s == 127
    assert dq[:6].tolist() == [6.0, -6.0, 6.0, 6.0, 4.0, -6.0] and nib[:6].tolist() == [7, 15, 7, 7, 6, 15]


def test_minus_zero_is_code_eight():
    nib, s, dq = quant_row("minus zero")                        # amax 1: e = -2, so 1 is 4 units (code 6)
    assert s == 125
    assert nib[:5].tolist() == [6, 8, 0, 8 | 1, 14]              # (-0.125 is -0.5 units of 2^-2: code 9)
    assert dq[1] == 0 and np.signbit(dq[1]) and not np.signbit(dq[2])


def test_clamp_ends():
    nib, s, dq = quant_row("low clamp")                         # amax 1.5 * 2^-125 wants e = -127: clamped to -125
    assert s == 2
    # units of 2^-125: 0.5 -> 0.5; 1.5 -> 1.5; -0.25 -> -0 (tie); 2^-8 -> 0; 2 -> 2
    assert nib[:5].tolist() == [1, 3, 8, 0, 4]
    assert dq[0] == np.float32(2.0 ** -126) and dq[4] == np.float32(2.0 ** -124)
    nib, s, dq = quant_row("low clamp, subnormal amax")         # a subnormal amax: e = -125, everything rounds to (signed) zero
    assert s == 2 and nib[:2].tolist() == [0, 8] and not dq.any()
    nib, s, dq = quant_row("high clamp")                        # the largest bf16: e wants 125 (floor(log2) = 127), 7.97 units saturate
    assert s == 252
    assert nib[:5].tolist() == [7, 8 | 6, 2, 0, 4] and dq[0] == np.float32(6.0 * 2.0 ** 125)
    assert R.E_MIN == -125 and R.E_MAX == 125
    # the range keeps every code * 2^e a normal bf16
    for e in (R.E_MIN, R.E_MAX):
        v = R.CODE_VALUES[1:] * 2.0 ** e
        assert np.isfinite(v.astype(np.float32)).all() and (v >= 2.0 ** -126).all()
        assert np.array_equal(R.bf16_round_trip(v).astype(np.float64), v)


def test_dequantised_values_round_trip_through_bf16():
    rng = np.random.default_rng(5)
    w = R.bf16_round_trip(rng.normal(size=(40, 256)) * np.exp2(rng.integers(-30, 30, size=(40, 1)))).astype(np.float64)
    w = np.concatenate([w, np.pad(np.stack(list(BLOCKS.values())), ((0, 0), (0, 224)))])
    dq = R.quantize(w)[2]
    assert np.array_equal(R.bf16_round_trip(dq).view(np.uint32), dq.view(np.uint32))   # bit for bit, the sign of -0 included


def test_requantising_is_idempotent():
    rng = np.random.default_rng(6)
    w = R.bf16_round_trip(rng.normal(size=(40, 256)) * np.exp2(rng.integers(-30, 30, size=(40, 1)))).astype(np.float64)
    w = np.concatenate([w, np.pad(np.stack(list(BLOCKS.values())), ((0, 0), (0, 224)))])
    q, s, dq = R.quantize(w)
    q2, s2, dq2 = R.quantize(dq)
    assert np.array_equal(q, q2) and np.array_equal(dq.view(np.uint32), dq2.view(np.uint32))
    # (a block the low clamp flushed to zero entirely is an all-zero block the second time: e = 0 by the rule for amax == 0)
    live = np.abs(dq).reshape(len(dq), -1, 32).max(axis=2) > 0
    assert np.array_equal(s[live], s2[live]) and (s2[~live] == 127).all()
    assert (~live & (s != 127)).sum() == 1                      # ... and the hand-written subnormal block is the only such one here


def test_the_three_entries_are_exported_and_bound():
    """Fails on a tree without the feature: the symbols are neither declared, bound nor in the library."""
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "zoomearth.h")).read()
    for name, nargs in (("ze_weights_quantize_mxfp4", 2), ("ze_op_quantize_mxfp4", 7), ("ze_op_gemv4", 21)):
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert len(fn.argtypes) == nargs
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", hdr, flags=re.M | re.S)
        assert m is not None and len(m.group(1).split(",")) == nargs
    assert len(lib.ze_op_gemv.argtypes) == 23                   # (ze_op_gemv's own signature did not change)
    assert lib.ze_weights_quantize_mxfp4(None, None) < 0        # a null engine is refused on the host: no GPU is touched
    assert lib.ze_op_quantize_mxfp4(None, None, 1, 32, None, None, None) < 0

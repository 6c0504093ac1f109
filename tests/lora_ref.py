"""Tests only: the numpy float32 restatement of the LoRA merge (zoomearth_amd/csrc/ze_lora.hip, k_lora_merge).

Per element: acc = 0; for k ascending: acc = f32(acc + f32(B[row, k] * A[k, col])); out = bf16_rne(f32(f32(W) + f32(scale * acc))), written
to row map_row(row, mode, offset) of a destination with leading dimension ld.  No fused multiply-add anywhere: numpy rounds every
float32 product and sum on its own, so the kernel's bits are reproduced exactly."""
import numpy as np


def bf16_bits(x):
    """float32 -> bf16 bits (uint16), round to nearest even: the repo's rule (checkpoint.write_safetensors, f32_to_bf16)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def map_row(r, mode, offset):
    r = np.asarray(r)
    return offset + r if mode == 0 else (r >> 4) * 32 + (r & 15) + offset


def as_f32(x):
    """float32 / float16 array or a (uint16, 'bf16') pair -> float32, exactly (what ze_lora_add uploads)."""
    return bf16_to_f32(x[0]) if isinstance(x, tuple) else np.asarray(x).astype(np.float32)


def merged_bits(base_bits, A, B, scale):
    """bf16 bits [rows, cols] of the merged tensor; base_bits uint16 [rows, cols], A f32 [r, cols], B f32 [rows, r]."""
    A, B = np.asarray(A, dtype=np.float32), np.asarray(B, dtype=np.float32)
    r = A.shape[0]
    if r == 0:
        return np.array(base_bits, dtype=np.uint16)
    acc = np.zeros(base_bits.shape, dtype=np.float32)
    for k in range(r):
        acc = (acc + (B[:, k:k + 1] * A[k:k + 1, :]).astype(np.float32)).astype(np.float32)
    s = np.float32(scale)
    return bf16_bits((bf16_to_f32(base_bits) + (s * acc).astype(np.float32)).astype(np.float32))


def merge_into(dst_bits, base_bits, A, B, scale, ld, mode=0, offset=0):
    """The kernel's store: dst_bits is a flat uint16 buffer; only the mapped rows' first `cols` columns change."""
    rows, cols = base_bits.shape
    out = merged_bits(base_bits, A, B, scale)
    at = map_row(np.arange(rows), mode, offset)[:, None] * ld + np.arange(cols)[None, :]
    dst_bits[at] = out
    return dst_bits


def merge_state_dict(weights, adapter):
    """{name: float32 array} base weights (values exact in bf16 or not: they are rounded first, as ze_load_weight does) and
    {name: (A, B, r, scale)} -> the host-merged weights as float32 arrays whose values are the merged bf16 values."""
    out = dict(weights)
    for name, (A, B, _r, scale) in adapter.items():
        out[name] = bf16_to_f32(merged_bits(bf16_bits(weights[name]), as_f32(A), as_f32(B), scale))
    return out

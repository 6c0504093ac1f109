"""CPU: LoRA adapters without a GPU -- the PEFT adapter reader (checkpoint.read_adapter), the numpy restatement of the merge kernel
(tests/lora_ref.py) against float64, and the C ABI's new entries."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import lora_ref
from zoomearth_amd import _lib, checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q0 = "model.language_model.layers.0.self_attn.q_proj"
D1 = "model.layers.1.mlp.down_proj"


def write_adapter(path, tensors, bf16=False, **cfg):
    os.makedirs(path, exist_ok=True)
    base = dict(peft_type="LORA", lora_alpha=16, r=8, bias="none", use_dora=False, fan_in_fan_out=False, modules_to_save=None,
                use_rslora=False, base_model_name_or_path="base")
    base.update(cfg)
    with open(os.path.join(path, "adapter_config.json"), "w", encoding="utf-8") as f:
        json.dump(base, f)
    checkpoint.write_safetensors(os.path.join(path, "adapter_model.safetensors"), tensors, bf16=bf16)


def ab(seed, rows, cols, r):
    g = np.random.default_rng(seed)
    return g.standard_normal((r, cols)).astype(np.float32), g.standard_normal((rows, r)).astype(np.float32)


# ---------------------------------------------------------------- read_adapter
def test_both_key_spellings_and_per_tensor_rank(tmp_path):
    a0, b0 = ab(1, 24, 16, 8)
    a1, b1 = ab(2, 16, 40, 4)
    write_adapter(str(tmp_path), {f"base_model.model.{Q0}.lora_A.weight": a0, f"base_model.model.{Q0}.lora_B.weight": b0,
                                  f"base_model.model.{D1}.lora_A.default.weight": a1, f"base_model.model.{D1}.lora_B.default.weight": b1})
    cfg, t = checkpoint.read_adapter(str(tmp_path))
    assert cfg["peft_type"] == "LORA" and sorted(t) == sorted([Q0 + ".weight", D1 + ".weight"])
    A, B, r, scale = t[Q0 + ".weight"]
    assert r == 8 and scale == 16 / 8 and np.array_equal(A, a0) and np.array_equal(B, b0)
    A, B, r, scale = t[D1 + ".weight"]
    assert r == 4 and scale == 16 / 4 and np.array_equal(A, a1) and np.array_equal(B, b1)      # the rank is the tensor's own


def test_rslora_alpha_pattern_and_bf16(tmp_path):
    a0, b0 = ab(3, 24, 16, 16)
    a1, b1 = ab(4, 16, 40, 4)
    tensors = {f"base_model.model.{Q0}.lora_A.weight": a0, f"base_model.model.{Q0}.lora_B.weight": b0,
               f"base_model.model.{D1}.lora_A.weight": a1, f"base_model.model.{D1}.lora_B.weight": b1}
    write_adapter(str(tmp_path / "rs"), tensors, use_rslora=True, lora_alpha=32)
    _, t = checkpoint.read_adapter(str(tmp_path / "rs"))
    assert t[Q0 + ".weight"][3] == 32 / 4.0 and t[D1 + ".weight"][3] == 32 / 2.0               # alpha / sqrt(r)
    write_adapter(str(tmp_path / "ap"), tensors, alpha_pattern={"down_proj": 6, "layers.0.self_attn.q_proj": 64}, bf16=True)
    _, t = checkpoint.read_adapter(str(tmp_path / "ap"))
    assert t[Q0 + ".weight"][3] == 64 / 16 and t[D1 + ".weight"][3] == 6 / 4
    bits, tag = t[Q0 + ".weight"][0]                                                            # bf16 stays raw bits
    assert tag == "bf16" and np.array_equal(bits, lora_ref.bf16_bits(a0))
    write_adapter(str(tmp_path / "ap2"), tensors, alpha_pattern={"up_proj": 6})                 # a pattern that matches nothing
    assert checkpoint.read_adapter(str(tmp_path / "ap2"))[1][D1 + ".weight"][3] == 16 / 4


@pytest.mark.parametrize("field,value", [("use_dora", True), ("fan_in_fan_out", True), ("bias", "all"), ("bias", "lora_only"),
                                         ("modules_to_save", ["lm_head"]), ("peft_type", "IA3")])
def test_every_unsupported_field_is_refused_by_name(tmp_path, field, value):
    a0, b0 = ab(5, 24, 16, 8)
    write_adapter(str(tmp_path), {f"base_model.model.{Q0}.lora_A.weight": a0, f"base_model.model.{Q0}.lora_B.weight": b0}, **{field: value})
    with pytest.raises(ValueError, match=field):
        checkpoint.read_adapter(str(tmp_path))


def test_an_a_without_its_b_is_refused(tmp_path):
    a0, b0 = ab(6, 24, 16, 8)
    write_adapter(str(tmp_path / "a"), {f"base_model.model.{Q0}.lora_A.weight": a0})
    with pytest.raises(ValueError, match="lora_A without lora_B"):
        checkpoint.read_adapter(str(tmp_path / "a"))
    write_adapter(str(tmp_path / "b"), {f"base_model.model.{Q0}.lora_B.weight": b0})
    with pytest.raises(ValueError, match="lora_B without lora_A"):
        checkpoint.read_adapter(str(tmp_path / "b"))
    write_adapter(str(tmp_path / "r"), {f"base_model.model.{Q0}.lora_A.weight": a0, f"base_model.model.{Q0}.lora_B.weight": b0[:, :4]})
    with pytest.raises(ValueError, match="rank"):
        checkpoint.read_adapter(str(tmp_path / "r"))
    write_adapter(str(tmp_path / "k"), {"base_model.model.lm_head.weight": a0})
    with pytest.raises(ValueError, match="unexpected tensor"):
        checkpoint.read_adapter(str(tmp_path / "k"))


# ---------------------------------------------------------------- the reference against float64
@pytest.mark.parametrize("rows,cols,r,scale", [(17, 24, 1, 2.0), (48, 100, 8, 0.25), (33, 72, 128, 1.0 / 16), (16, 8, 64, -3.0)])
def test_lora_ref_is_within_half_an_ulp_of_float64_plus_the_fp32_accumulation_bound(rows, cols, r, scale):
    """|bf16 result - exact| <= half a bf16 ulp of the exact value + (r + 2) * 2^-24 * (|W| + |s| * sum |B||A|): r products, r sums (the
    first is exact), the scale product and the final sum each contribute at most 2^-24 relative to a partial result that the absolute
    sums bound; the rounding to bf16 then moves the fp32 value by at most half an ulp of a number within that distance of the exact
    one (ulp taken at the larger of the two magnitudes)."""
    g = np.random.default_rng(rows * 1000 + r)
    W = lora_ref.bf16_bits((g.standard_normal((rows, cols)) * 0.05).astype(np.float32))
    A = (g.standard_normal((r, cols)) * 0.3).astype(np.float32)
    B = (g.standard_normal((rows, r)) * 0.3).astype(np.float32)
    got = lora_ref.bf16_to_f32(lora_ref.merged_bits(W, A, B, scale)).astype(np.float64)
    w64 = lora_ref.bf16_to_f32(W).astype(np.float64)
    s64 = float(np.float32(scale))
    exact = w64 + s64 * (B.astype(np.float64) @ A.astype(np.float64))
    mag = np.abs(w64) + abs(s64) * (np.abs(B).astype(np.float64) @ np.abs(A).astype(np.float64))
    acc = (r + 2) * 2.0 ** -24 * mag
    big = np.maximum(np.abs(exact) + acc, np.abs(got))
    half_ulp = 2.0 ** (np.floor(np.log2(np.maximum(big, 2.0 ** -126))) - 7) / 2
    err = np.abs(got - exact)
    print(f"max err / bound = {(err / (half_ulp + acc)).max():.3f}")
    assert (err <= half_ulp + acc).all()
    assert (got != w64).mean() > 0.5                                                            # (the delta is no rounding noise)


def test_lora_ref_stores_through_the_row_map_and_r0_copies():
    g = np.random.default_rng(9)
    W = lora_ref.bf16_bits(g.standard_normal((20, 8)).astype(np.float32))
    W[0, 0] = 0x8000                                                                            # -0.0 survives a restore
    A, B = ab(10, 20, 8, 4)
    dst = np.full(64 * 12, 0x7FC1, np.uint16)
    lora_ref.merge_into(dst, W, A, B, 0.5, ld=12, mode=1, offset=16)
    d = dst.reshape(64, 12)
    want = lora_ref.merged_bits(W, A, B, 0.5)
    assert np.array_equal(d[16:32, :8], want[:16]) and np.array_equal(d[48:52, :8], want[16:])
    touched = np.zeros((64, 12), bool)
    touched[16:32, :8] = touched[48:52, :8] = True
    assert (d[~touched] == 0x7FC1).all()
    assert np.array_equal(lora_ref.merged_bits(W, np.zeros((0, 8), np.float32), np.zeros((20, 0), np.float32), 1.0), W)
    assert lora_ref.map_row(np.arange(34), 1, 0).tolist() == list(range(16)) + list(range(32, 48)) + [64, 65]


# ---------------------------------------------------------------- the C ABI
LORA_SYMBOLS = ("ze_lora_create", "ze_lora_add", "ze_lora_destroy", "ze_lora_activate", "ze_lora_info", "ze_op_lora_merge")


def test_the_lora_entries_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "zoomearth.h"), encoding="utf-8") as f:
        header = f.read()
    assert re.search(r"#define ZE_MAX_ADAPTERS 8\b", header) and re.search(r"#define ZE_LORA_MAX_RANK 128\b", header)
    assert re.search(r"int ze_lora_add\(ze_engine\* e, int adapter, const char\* name, int dtype, int r, float scale, const void\* host_A, "
                     r"const void\* host_B\);", header)
    assert re.search(r"int ze_lora_activate\(ze_engine\* e, int adapter, void\* stream\);", header)
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in LORA_SYMBOLS:
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert name in _lib.EXPORTS, name
        assert re.search(rf" T {name}$", syms, re.M), name
    assert getattr(_lib.lib(), "ze_lora_info") is not None
    for field in ("PeftModel.from_pretrained", "set_adapter", "disable_adapter", "grpo_trainer.py:679"):
        assert field in header, field

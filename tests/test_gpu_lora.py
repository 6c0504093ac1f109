"""GPU: LoRA adapters -- the merge kernel (zoomearth_amd/csrc/ze_lora.hip) against tests/lora_ref.py bit for bit, and the engine, model,
scheduler and rollout paths built on it against a model loaded with the HOST-merged weights.  Every comparison is an equality."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import lora_ref
from gpu_util import CHAIN_W
from oracle import prng
from oracle import qwen25vl as Q

pytestmark = pytest.mark.gpu

INVALID, NOMEM, NOTFOUND = -1, -3, -4
SENTINEL = 0x7FC1
ENGINE_KW = dict(max_seqs=4, max_ctx=2048, max_patches=8192, max_tile_side=2048, max_prefill_rows=8192)
DECODER = re.compile(r"language_model\.layers\.\d+\.(self_attn\.[qkvo]_proj|mlp\.(gate|up|down)_proj)\.weight$")
VISION = ("model.visual.blocks.1.attn.qkv.weight", "model.visual.blocks.1.mlp.down_proj.weight")


# ---------------------------------------------------------------- 1. the kernel
def run_merge(e, rows, cols, r, mode, offset, pad, shift, seed):
    g = np.random.default_rng(seed)
    base = lora_ref.bf16_bits((g.standard_normal((rows, cols)) * 0.08).astype(np.float32))
    A = (g.standard_normal((r, cols)) * 0.2).astype(np.float32)
    B = (g.standard_normal((rows, r)) * 0.2).astype(np.float32)
    scale, ld = 0.75, cols + pad
    n_rows = int(lora_ref.map_row(rows - 1, mode, offset)) + 3
    want = lora_ref.merge_into(np.full(n_rows * ld + 8, SENTINEL, np.uint16), base, A, B, scale, ld, mode, offset)
    buf = torch.full((n_rows * ld + 8 + 8,), SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    dst = buf[shift:shift + n_rows * ld + 8]                          # shift = 1: the base address is 2 bytes off the 16-byte grid
    tb = torch.from_numpy(base.view(np.int16)).cuda().view(torch.bfloat16)
    e.op_lora_merge(tb, torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), scale, dst, ld, mode, offset)
    torch.cuda.synchronize()
    got = dst.view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, want), (rows, cols, r, mode, offset, pad, shift, int((got != want).sum()))
    rest = buf.view(torch.int16).cpu().numpy().view(np.uint16)
    assert (rest[:shift] == SENTINEL).all() and (rest[shift + len(want):] == SENTINEL).all()


@pytest.fixture(scope="module")
def small_engine():
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.engine import Engine
    e = Engine(ModelConfig.tiny(), device=0, max_seqs=1, max_ctx=256, max_patches=1024, max_tile_side=1024)
    yield e
    e.close()


@pytest.mark.parametrize("cols", [8, 24, 100, 1176])
def test_merge_kernel_is_bit_equal_to_the_reference(small_engine, cols):
    """rows x r x (mode, offset) x ld x alignment for one column count; padding columns, rows outside the map and the bytes around the
    destination keep the sentinel (merge_into writes the mapped elements only)."""
    n = 0
    for rows in (1, 16, 17, 48):
        for r in (1, 8, 128):
            for mode, offset in ((0, 0), (1, 0), (1, 16)):
                for pad in (0, 24):
                    for shift in (0, 1):
                        run_merge(small_engine, rows, cols, r, mode, offset, pad, shift, seed=n)
                        n += 1
    assert n == 144


def test_merge_kernel_r0_copies_and_past_one_column_tile(small_engine):
    g = np.random.default_rng(5)
    base = lora_ref.bf16_bits(g.standard_normal((35, 4104)).astype(np.float32))       # three column tiles of 2048, the last one short
    base[0, :4] = [0x8000, 0x7FC5, 0xFF80, 0x0001]                                    # -0, a NaN payload, -inf, a subnormal: a copy keeps bits
    tb = torch.from_numpy(base.view(np.int16)).cuda().view(torch.bfloat16)
    dst = torch.full((35 * 4104,), SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    small_engine.op_lora_merge(tb, None, None, 1.0, dst, 4104)
    assert np.array_equal(dst.view(torch.int16).cpu().numpy().view(np.uint16).reshape(35, 4104), base)
    run_merge(small_engine, 35, 4104, 5, 0, 2, 8, 0, seed=77)
    # more work items than the grid's 2048 workgroups: 130 row tiles x 17 column tiles of the scalar form (ld off the 16-byte grid),
    # so some workgroups take a second item and stage its B rows over the first one's
    run_merge(small_engine, 2064, 4104, 2, 0, 0, 1, 0, seed=78)
    lib, h = small_engine.lib, small_engine.h
    p = C.c_void_p(dst.data_ptr())
    for bad in ((0, 8, 1, 8, 0, 0), (4, 8, 129, 8, 0, 0), (4, 8, -1, 8, 0, 0), (4, 8, 1, 4, 0, 0), (4, 8, 1, 8, 2, 0), (4, 8, 1, 8, 0, -1)):
        rows, cols, r, ld, mode, off = bad
        assert lib.ze_op_lora_merge(h, p, rows, cols, p, p, r, 1.0, p, ld, mode, off, None) == INVALID, bad


# ---------------------------------------------------------------- the models
def make_adapter(shapes, names, seed, ranks=(8, 3, 16)):
    g = np.random.default_rng(seed)
    out = {}
    for i, name in enumerate(names):
        rows, cols = shapes[name]
        r = ranks[i % len(ranks)]
        A = (g.standard_normal((r, cols)) * 0.1).astype(np.float32)
        B = (g.standard_normal((rows, r)) * 0.1).astype(np.float32)
        out[name] = (A, B, r, 16.0 / r)
    return out


@pytest.fixture(scope="module")
def world():
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.engine import Engine
    from zoomearth_amd.modeling import ZoomEarthForConditionalGeneration
    cfg = Q.tiny_config()
    w = Q.synthetic_weights(cfg, **CHAIN_W)
    shapes = Q.weight_shapes(cfg)
    names = [k for k in shapes if DECODER.search(k)] + list(VISION)
    assert len(names) == 7 * cfg.text.num_hidden_layers + 2
    X = make_adapter(shapes, names, 1)
    Y = make_adapter(shapes, [n for n in names if "q_proj" in n or "down_proj" in n], 2, ranks=(4,))
    merged = lora_ref.merge_state_dict(w, X)
    models = []
    for weights in (w, merged, w):
        e = Engine(ModelConfig.tiny(), device=0, **ENGINE_KW)
        e.load_state_dict(weights.items())
        models.append(ZoomEarthForConditionalGeneration(ModelConfig.tiny(), e))
    ma, mm, mb = models
    ma.load_adapter(X, "x")
    ma.load_adapter(Y, "y")
    yield dict(cfg=cfg, w=w, X=X, Y=Y, merged=merged, ma=ma, mm=mm, mb=mb)
    for m in models:
        m.engine.close()


def arena(e):
    torch.cuda.synchronize()
    return e.weights_arena().clone()


def image_run(e):
    """prefill logits, 12 greedy tokens and the per-token log-probabilities of one image prompt"""
    cfg = Q.tiny_config()
    tile = prng.synthetic_tile(5, 300, 400)
    view = e.crop_resize(torch.from_numpy(tile).cuda(), (0, 0, 400, 300), (200, 150))
    pv, grid = e.preprocess_image(view)
    n_img = grid[1] * grid[2] // 4
    ids = [11, 12, cfg.vision_start_token_id] + [cfg.image_token_id] * n_img + [cfg.vision_end_token_id, 13, 14, 15, 16, 17]
    emb = e.vit_forward(pv, [grid])
    pos, delta = e.rope_index(ids, [grid])
    e.seq_reset(0)
    logits = e.prefill(0, ids, emb, pos, delta).cpu().numpy()
    toks = e.generate(0, 12, ignore_eos=True)
    e.seq_reset(1)
    lp = e.score(1, ids, emb, pos, delta).cpu().numpy()
    e.seq_reset(0), e.seq_reset(1)
    return logits, list(toks), lp


# ---------------------------------------------------------------- 2. merged on the device == merged on the host
def test_an_activated_adapter_equals_the_host_merged_checkpoint(world):
    ma, mm = world["ma"], world["mm"]
    ma.set_adapter("x")
    assert ma.engine.lora_info()[:2] == (ma._adapters["x"], 2) and ma.engine.lora_info()[2] > 0
    assert torch.equal(arena(ma.engine), arena(mm.engine))
    got, want = image_run(ma.engine), image_run(mm.engine)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and np.array_equal(got[2], want[2])
    base = image_run(world["mb"].engine)
    assert not np.array_equal(base[0], want[0])                                        # (the adapter moves the logits)
    ma.set_adapter(None)


# ---------------------------------------------------------------- 3. switches
def test_switches_restore_the_base_bits_and_skip_what_is_active(world):
    ma, mb = world["ma"], world["mb"]
    e = ma.engine
    base = arena(mb.engine)
    ma.set_adapter("x")
    assert not torch.equal(arena(e), base)
    ma.set_adapter(None)
    assert torch.equal(arena(e), base) and e.lora_info()[0] is None
    ma.set_adapter("y")
    y_from_base = arena(e)
    ma.set_adapter("x")
    ma.set_adapter("y")                                                                # X then Y: the tensors only X touched are restored
    assert torch.equal(arena(e), y_from_base) and not torch.equal(y_from_base, base)
    gen = e.prefix_pool_info()[2]
    e.lora_activate(ma._adapters["y"])                                                 # already active: nothing moves
    assert e.prefix_pool_info()[2] == gen
    ma.set_adapter("x")
    assert e.prefix_pool_info()[2] != gen
    ma.set_adapter(None)
    assert torch.equal(arena(e), base)


# ---------------------------------------------------------------- 4. disable_adapter, scoring and rollouts under the base weights
def text_items(n=3):
    from zoomearth_amd.modeling import ScoreItem
    return [ScoreItem(prng.uniform_ints(300 + i, 40 + 7 * i, 10, 1990).tolist(), [], [], [], 5) for i in range(n)]


def test_the_drawn_adapter_moves_log_probabilities_by_more_than_bf16_noise(world):
    """CPU: the host-merged oracle against the base oracle, with the yardstick of tests/test_gpu_batch.py (the oracle's own
    bf16-vs-fp32 error) -- so `ref_logps != logps` below is a property of the adapter, not of rounding."""
    cfg, ids = world["cfg"], text_items(1)[0].ids
    ref32 = Q.Qwen25VLOracle(cfg, world["w"], "fp32").prefill(ids)
    yard = float(np.abs(Q.Qwen25VLOracle(cfg, world["w"], "bf16").prefill(ids) - ref32).max())
    moved = float(np.abs(Q.Qwen25VLOracle(cfg, world["merged"], "fp32").prefill(ids) - ref32).max())
    print(f"adapter moves the last-position logits by {moved:.4f}; oracle bf16-vs-fp32 = {yard:.4f}")
    assert moved > 2.0 * yard


def test_disable_adapter_restores_on_exit_and_on_exception(world):
    ma, mb = world["ma"], world["mb"]
    ma.set_adapter("x")
    with ma.disable_adapter():
        assert ma.active_adapter is None and torch.equal(arena(ma.engine), arena(mb.engine))
    assert ma.active_adapter == "x"
    with pytest.raises(KeyError):
        with ma.disable_adapter():
            raise KeyError("inside")
    assert ma.active_adapter == "x" and torch.equal(arena(ma.engine), arena(world["mm"].engine))
    items = text_items()
    want_base = [t.cpu() for t in mb.score_sequences(items)]
    want_x = [t.cpu() for t in world["mm"].score_sequences(items)]
    got_base = [t.cpu() for t in ma.score_sequences(items, adapter=None)]
    assert ma.active_adapter == "x"
    got_x = [t.cpu() for t in ma.score_sequences(items)]
    assert all(torch.equal(a, b) for a, b in zip(got_base, want_base)) and all(torch.equal(a, b) for a, b in zip(got_x, want_x))
    assert not any(torch.equal(a, b) for a, b in zip(got_base, got_x))
    ids = torch.tensor([items[0].ids])
    assert torch.equal(ma.per_token_logps(ids, score_from=5, adapter=None)[0, 5:], want_base[0])
    assert ma.active_adapter == "x"
    ma.set_adapter(None)


def test_rollout_ref_logps_are_the_base_models_scores(world):
    from test_gpu_infer_e2e import word
    from test_gpu_rollout import bbox_tokenizer
    from zoomearth_amd import hostloop as H
    from zoomearth_amd.image import DeviceImage
    from zoomearth_amd.modeling import ScoreItem
    from zoomearth_amd.processor import ZoomEarthProcessor
    from zoomearth_amd.rollout import rollout_two_stage
    ma, mb = world["ma"], world["mb"]
    proc = ZoomEarthProcessor(bbox_tokenizer(), min_pixels=3136, max_pixels=128 * 128 * 28 * 28)
    tile = prng.synthetic_tile(90, 700, 900)
    samples = []
    for i in range(2):
        q = " ".join(word(int(v)) for v in prng.uniform_ints(70 + i, 5, 0, 1999))
        samples.append(dict(prompt=H.stage1_prompt(q), image=DeviceImage.from_numpy(tile, ma.engine), bbox=[1, 2, 3, 4] if i == 0 else []))
    kw = dict(num_generations=2, temperature=0.9, max_new_tokens=8, seed=11)
    with pytest.raises(ValueError, match="active LoRA adapter"):
        rollout_two_stage(ma, proc, samples, ref_logps=True, **kw)
    ma.set_adapter("x")
    ros = rollout_two_stage(ma, proc, samples, ref_logps=True, **kw)
    assert ma.active_adapter == "x" and len(ros) == 4 and all(r.error is None for r in ros)
    for ro in ros:                                                                      # the same sequences on the base-only model
        prompt = ro.prompt2 if ro.prompt2 is not None else ro.prompt1
        tail = ro.completion2_ids if ro.prompt2 is not None else ro.completion1_ids
        inp = proc(text=[prompt], images=list(ro.images), return_tensors="pt")   # (the front-end reads no weights)
        ids = inp["input_ids"][0].tolist() + [int(t) for t in tail]
        grids = inp["image_grid_thw"].tolist()
        offs = np.concatenate([[0], np.cumsum([g[0] * g[1] * g[2] for g in grids])]).astype(int)
        feats = [mb._features(inp["pixel_values"][offs[i]:offs[i + 1]], grids[i], None) for i in range(len(grids))]
        want = mb.score_sequences([ScoreItem(ids, grids, feats, None, min(max(ro.n_prompt1 - 1, 0), len(ids) - 1))])[0].cpu()
        assert ro.ref_logps.shape == ro.logps.shape and torch.equal(ro.ref_logps, want)
        assert not torch.equal(ro.ref_logps, ro.logps)
    ma.set_adapter(None)


# ---------------------------------------------------------------- 5. from_pretrained on an adapter directory
def test_from_pretrained_on_an_adapter_directory(world, tmp_path):
    from zoomearth_amd import checkpoint
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.modeling import ZoomEarthForConditionalGeneration
    t, v = ModelConfig.tiny().text, ModelConfig.tiny().vision
    base, ad = tmp_path / "base", tmp_path / "adapter"
    base.mkdir(), ad.mkdir()
    c = ModelConfig.tiny()
    cfg = {"vision_config": dict(depth=v.depth, hidden_size=v.hidden_size, num_heads=v.num_heads, intermediate_size=v.intermediate_size,
                                 out_hidden_size=v.out_hidden_size, fullatt_block_indexes=list(v.fullatt_block_indexes)),
           "hidden_size": t.hidden_size, "num_hidden_layers": t.num_hidden_layers, "num_attention_heads": t.num_attention_heads,
           "num_key_value_heads": t.num_key_value_heads, "intermediate_size": t.intermediate_size, "vocab_size": t.vocab_size,
           "rms_norm_eps": t.rms_norm_eps, "rope_theta": t.rope_theta, "rope_scaling": {"type": "mrope", "mrope_section": list(t.mrope_section)},
           "tie_word_embeddings": True, "image_token_id": c.image_token_id, "vision_start_token_id": c.vision_start_token_id,
           "vision_end_token_id": c.vision_end_token_id, "eos_token_id": list(c.eos_token_ids), "pad_token_id": c.pad_token_id,
           "zoomearth_synthetic_weights": CHAIN_W}
    (base / "config.json").write_text(json.dumps(cfg))
    tensors = {}
    for name, (A, B, _r, _s) in world["X"].items():
        tensors[f"base_model.model.{name[:-len('.weight')]}.lora_A.weight"] = A
        tensors[f"base_model.model.{name[:-len('.weight')]}.lora_B.default.weight"] = B
    checkpoint.write_safetensors(str(ad / "adapter_model.safetensors"), tensors)
    # per-tensor ranks 8 / 3 / 16 with scale 16 / r: one alpha for all
    (ad / "adapter_config.json").write_text(json.dumps(dict(peft_type="LORA", lora_alpha=16, r=8, bias="none",
                                                            base_model_name_or_path=str(base))))
    kw = dict(max_seqs=2, max_ctx=512, max_patches=1024, max_tile_side=1024)
    one = ZoomEarthForConditionalGeneration.from_pretrained(str(ad), **kw)
    two = ZoomEarthForConditionalGeneration.from_pretrained(str(base), **kw)
    try:
        assert one.active_adapter == "default" and two.active_adapter is None
        two.set_adapter(two.load_adapter(str(ad)))
        assert torch.equal(arena(one.engine), arena(two.engine))
        with pytest.raises(ValueError, match="already loaded"):
            two.load_adapter(str(ad))
        two.delete_adapter("default")
        assert two.active_adapter is None and two.engine.lora_info()[:2] == (None, 0)
    finally:
        one.engine.close(), two.engine.close()


# ---------------------------------------------------------------- 6. the scheduler
def test_a_scheduler_under_an_adapter_equals_the_host_merged_model(world):
    from tiny_tok import make_tokenizer
    from zoomearth_amd.processor import ZoomEarthProcessor
    from zoomearth_amd.scheduler import ChainScheduler, Request
    ma, mm = world["ma"], world["mm"]
    proc = ZoomEarthProcessor(make_tokenizer(), min_pixels=3136, max_pixels=128 * 128 * 28 * 28)
    prompts = [" ".join(f"w{int(v)}" for v in prng.uniform_ints(500 + i, 20 + 5 * i, 10, 1990)) for i in range(4)]

    def run(model, **kw):
        sched = ChainScheduler(model, proc, do_sample=False, burst=4, ignore_eos=True, **kw)
        reqs = [Request(prompt=p, images=[], max_new_tokens=10) for p in prompts]
        for r in reqs:
            sched.submit(r)
        sched.run()
        return sched, [list(r.tokens) for r in reqs]

    assert ma.active_adapter is None
    sched, got = run(ma, adapter="x")
    assert ma.active_adapter == "x"
    _, want = run(mm)
    _, base = run(world["mb"])
    assert got == want and got != base and all(len(t) == 10 for t in got)
    sched.submit(Request(prompt=prompts[0], images=[], max_new_tokens=4))
    with pytest.raises(RuntimeError, match="cannot change"):
        sched.set_adapter(None)
    sched.run()
    with pytest.raises(ValueError, match="no adapter"):
        ChainScheduler(ma, proc, adapter="nope")
    _, again = run(ma, adapter=None)
    assert again == base and ma.active_adapter is None


# ---------------------------------------------------------------- base-weight writes under an adapter, through the model
def test_a_base_weight_write_under_an_adapter_is_seen_by_the_model(world):
    from zoomearth_amd._lib import ZoomEarthError
    from zoomearth_amd.rollout import rollout_two_stage
    ma, mm, mb = world["ma"], world["mm"], world["mb"]
    norm = "model.language_model.norm.weight"
    ma.set_adapter("x")
    store = ma.engine.lora_info()[2]
    with pytest.raises(ZoomEarthError):                                                # refused calls write nothing: the adapter stays
        ma.engine.load_weight("model.language_model.nope.weight", world["w"][norm])
    with pytest.raises(ZoomEarthError):
        ma.engine.load_weight(norm, world["w"][norm][:-1])
    assert ma.active_adapter == "x" and ma.engine.lora_info()[2] == store
    ma.engine.load_weight(norm, world["w"][norm])                                      # a write: the merged arena is the base now
    assert ma.active_adapter is None and ma.engine.lora_info() == (None, 2, 0)
    assert torch.equal(arena(ma.engine), arena(mm.engine))
    with pytest.raises(ValueError, match="active LoRA adapter"):                       # no reference policy that equals the policy
        rollout_two_stage(ma, None, [], ref_logps=True)
    with ma.disable_adapter():
        assert ma.active_adapter is None
    assert ma.active_adapter is None
    ma.set_adapter("x")                                                                # merges again, on the new base
    assert ma.active_adapter == "x" and not torch.equal(arena(ma.engine), arena(mm.engine))
    ma.engine.load_state_dict(world["w"].items())                                      # back to the base checkpoint for the tests below
    assert ma.active_adapter is None and torch.equal(arena(ma.engine), arena(mb.engine))
    ma.set_adapter("x")
    assert torch.equal(arena(ma.engine), arena(mm.engine))
    ma.set_adapter(None)


# ---------------------------------------------------------------- fp16 / bf16 uploads
def test_fp16_and_bf16_adapters_upload_exactly(world):
    """ze_lora_add converts fp16 / bf16 A and B to fp32 exactly (the half conversion is the library's own, subnormals included): an
    adapter given in either format merges to the bits of the same values given as float32 (lora_ref.as_f32)."""
    ma = world["ma"]
    e = ma.engine
    q0, d0 = "model.language_model.layers.0.self_attn.q_proj.weight", "model.language_model.layers.1.mlp.down_proj.weight"
    g = np.random.default_rng(21)

    def half(shape):
        x = (g.standard_normal(shape) * 0.1).astype(np.float16)
        flat = x.reshape(-1)
        flat[:8] = np.array([6e-8, -6e-8, 3.1e-5, -5.9e-5, 6.1e-5, 0.0, -0.0, 1.0], np.float16)   # subnormals, the smallest normal, zeros
        flat[8:12] = np.array([65504.0, -65504.0, 2.0 ** -14, 2.0 ** -24], np.float16) * np.float16(1.0)
        return x

    def bf(shape):
        return (lora_ref.bf16_bits((g.standard_normal(shape) * 0.1).astype(np.float32)), "bf16")

    def merged(tensors):
        a = e.lora_load(tensors)
        e.lora_activate(a)
        out = arena(e)
        e.lora_activate(None)
        e.lora_destroy(a)
        return out

    assert np.isfinite(half((4, 8)).astype(np.float32)).all() and (half((4, 8)).reshape(-1)[0] != 0)
    cases = {"fp16": {q0: (half((8, 512)), half((512, 8)), 8, 1e-3), d0: (half((4, 1376)), half((512, 4)), 4, 1e-3)},
             "bf16": {q0: (bf((8, 512)), bf((512, 8)), 8, 2.0), d0: (bf((4, 1376)), bf((512, 4)), 4, 4.0)},
             "mixed": {q0: (half((8, 512)), bf((512, 8)), 8, 1e-3), d0: (bf((4, 1376)), (g.standard_normal((512, 4)) * 0.1).astype(np.float32), 4, 4.0)}}
    base = arena(e)
    for tag, tensors in cases.items():
        as32 = {n: (lora_ref.as_f32(A), lora_ref.as_f32(B), r, s) for n, (A, B, r, s) in tensors.items()}
        got, want = merged(tensors), merged(as32)
        assert torch.equal(got, want) and not torch.equal(got, base), tag
    assert torch.equal(arena(e), base)


# ---------------------------------------------------------------- 7. errors
def test_refused_calls_return_their_codes(world):
    ma = world["ma"]
    e = ma.engine
    lib, h = e.lib, e.h
    before = arena(e)
    q0 = b"model.language_model.layers.0.self_attn.q_proj.weight"
    A = np.zeros((129, 512), np.float32)
    B = np.zeros((512, 129), np.float32)
    pa, pb = A.ctypes.data_as(C.c_void_p), B.ctypes.data_as(C.c_void_p)
    a = e.lora_create()
    assert lib.ze_lora_add(h, a, b"model.language_model.layers.9.self_attn.q_proj.weight", 0, 8, 1.0, pa, pb) == NOTFOUND
    for name in (b"lm_head.weight", b"model.language_model.embed_tokens.weight", b"model.language_model.norm.weight",
                 b"model.language_model.layers.0.input_layernorm.weight", b"model.language_model.layers.0.self_attn.q_proj.bias"):
        assert lib.ze_lora_add(h, a, name, 0, 8, 1.0, pa, pb) == INVALID, name
        assert b"projection matrices only" in lib.ze_last_error(h)
    assert lib.ze_lora_add(h, a, q0, 0, 0, 1.0, pa, pb) == INVALID and lib.ze_lora_add(h, a, q0, 0, 129, 1.0, pa, pb) == INVALID
    assert lib.ze_lora_add(h, a, q0, 7, 8, 1.0, pa, pb) == INVALID                     # dtype
    assert lib.ze_lora_add(h, 99, q0, 0, 8, 1.0, pa, pb) == NOTFOUND
    assert lib.ze_lora_add(h, a, q0, 0, 8, 1.0, pa, pb) == 0
    assert lib.ze_lora_add(h, a, q0, 0, 8, 1.0, pa, pb) == INVALID                     # the same tensor twice
    assert lib.ze_lora_add(h, a, b"model.layers.0.self_attn.q_proj.weight", 0, 8, 1.0, pa, pb) == INVALID   # ... under its other spelling
    with pytest.raises(ValueError, match="shape mismatch"):
        e.lora_add(a, "model.language_model.layers.0.self_attn.k_proj.weight", A[:8], B[:, :8], 1.0)
    assert lib.ze_lora_activate(h, a, e._stream()) == 0
    assert lib.ze_lora_destroy(h, a) == INVALID                                        # the active one
    assert lib.ze_lora_add(h, a, b"model.language_model.layers.0.self_attn.k_proj.weight", 0, 8, 1.0, pa, pb) == INVALID   # deactivate first
    assert lib.ze_lora_activate(h, 7, e._stream()) == NOTFOUND and lib.ze_lora_activate(h, -2, e._stream()) == NOTFOUND
    extra = []
    out = C.c_int()
    while lib.ze_lora_create(h, C.byref(out)) == 0:
        extra.append(out.value)
    assert len(extra) + 3 == 8 and lib.ze_lora_create(h, C.byref(out)) == NOMEM        # x, y, a and the rest: the ninth is refused
    for x in extra:
        assert lib.ze_lora_destroy(h, x) == 0
    assert lib.ze_lora_destroy(h, extra[0]) == NOTFOUND
    # a base-weight write under an active adapter: the arena is the base now, nothing is active, the adapters stay
    assert e.lora_info()[0] == a
    e.load_weight("model.language_model.norm.weight", world["w"]["model.language_model.norm.weight"])
    assert e.lora_info() == (None, 3, 0)
    assert lib.ze_lora_destroy(h, a) == 0
    assert torch.equal(arena(e), before)                                               # (the zero delta changed no bit)
    assert ma.active_adapter is None


# ---------------------------------------------------------------- 8. FP8
def test_fp8_quantises_again_after_a_switch(world):
    ma, mm = world["ma"], world["mm"]
    ids = text_items(1)[0].ids

    def logits(e):
        pos, delta = e.rope_index(ids, [])
        e.seq_reset(0)
        out = e.prefill(0, ids, None, pos, delta).cpu().numpy()
        toks = e.generate(0, 6, ignore_eos=True)
        e.seq_reset(0)
        return out, list(toks)

    # (quantising replaces the arena's bf16 values by the dequantised ones: the base store has to date from before it -- as in any
    #  session that activated an adapter once -- or the dequantised values would be the base)
    ma.set_adapter("x")
    ma.set_adapter(None)
    ma.engine.quantize_fp8()
    base8 = logits(ma.engine)
    ma.set_adapter("x")                                                                # drops the FP8 copy with everything derived
    ma.engine.quantize_fp8()
    mm.engine.quantize_fp8()
    got, want = logits(ma.engine), logits(mm.engine)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and not np.array_equal(got[0], base8[0])
    ma.set_adapter(None)

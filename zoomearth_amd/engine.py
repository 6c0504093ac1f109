"""Python handle on one ze_engine (one process per GPU).

torch tensors are used only as device-memory containers (allocation, H2D/D2H copies, stream handles);
every computation goes through the C ABI of libzoomearth_hip.so.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Iterable, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .config import ModelConfig

MAX_TOP_LOGPROBS = 20  # ZE_MAX_TOP_LOGPROBS (OpenAI's cap on top_logprobs)
MAX_LOGIT_BIAS = 512   # ZE_MAX_LOGIT_BIAS (pairs of one chain's bias list)
MAX_RULE_INTS, MAX_RULE_WORDS, MAX_RULE_LEN = 1024, 64, 16   # ZE_MAX_RULE_* (token rules: ints of a packed list, records, ids of a record)
MAX_GRAMMARS = 16      # ZE_MAX_GRAMMARS (grammars of one engine; zoomearth_amd/grammar.py holds the limits of one grammar)


def pack_records(records) -> np.ndarray:
    """Token-id sequences as the packed records of ze_seq_set_token_rules: len, id0 .. id(len-1), ..."""
    out = []
    for r in records:
        r = [int(t) for t in r]
        out.append(len(r))
        out.extend(r)
    return np.asarray(out, dtype=np.int32)
_NP2ZE = {np.dtype(np.float32): _lib.ZE_F32, np.dtype(np.float16): _lib.ZE_F16}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _i32(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.int32))
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


class ScoreDetail(NamedTuple):
    """What score_batch_detail returns per scored position, packed in chain order (chain i: [offsets[i], offsets[i + 1])); the
    members that were not asked for are None."""
    logps: torch.Tensor                    # f32 [count]
    entropy: Optional[torch.Tensor]        # f32 [count]
    rank: Optional[torch.Tensor]           # int32 [count], 0 = the arg-max
    top_ids: Optional[torch.Tensor]        # int32 [count, top_n]
    top_logprobs: Optional[torch.Tensor]   # f32 [count, top_n]
    offsets: list

    def chain(self, i: int) -> "ScoreDetail":
        """The entries of chain i alone."""
        a, b = self.offsets[i], self.offsets[i + 1]
        return ScoreDetail(*(None if x is None else x[a:b] for x in self[:5]), [0, b - a])


class Engine:
    def __init__(self, config: ModelConfig, device: int = 0, max_seqs: int = 4, max_ctx: int = 4096,
                 max_patches: int = 8192, max_tile_side: int = 8192, max_prefill_rows: int = 0):
        if not torch.cuda.is_available():
            raise RuntimeError("zoomearth_amd needs a ROCm GPU (MI355X); there is no CPU fallback")
        self.lib = _lib.lib()
        self.config = config
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        self.zcfg = self._make_zcfg(config, max_seqs, max_ctx, max_patches, max_tile_side)
        self.zcfg.max_prefill_rows = int(max_prefill_rows)
        self.max_prefill_rows = max(int(max_prefill_rows), int(max_ctx))
        h = C.c_void_p()
        _lib.check(self.lib.ze_engine_create(C.byref(self.zcfg), device, C.byref(h)))
        self.h = h
        self.max_seqs, self.max_ctx, self.max_patches = max_seqs, max_ctx, max_patches
        self.patch_dim = (config.vision.in_channels * config.vision.temporal_patch_size
                          * config.vision.patch_size ** 2)

    # ------------------------------------------------------------------ plumbing
    @staticmethod
    def _make_zcfg(c: ModelConfig, max_seqs, max_ctx, max_patches, max_tile_side) -> _lib.ZeConfig:
        z = _lib.ZeConfig()
        v, t = c.vision, c.text
        z.vit_depth, z.vit_hidden, z.vit_heads = v.depth, v.hidden_size, v.num_heads
        z.vit_intermediate, z.vit_out_hidden = v.intermediate_size, v.out_hidden_size
        z.patch_size, z.temporal_patch_size, z.spatial_merge_size = v.patch_size, v.temporal_patch_size, v.spatial_merge_size
        z.window_size, z.in_channels = v.window_size, v.in_channels
        z.n_fullatt = len(v.fullatt_block_indexes)
        for i, b in enumerate(v.fullatt_block_indexes):
            z.fullatt_block_indexes[i] = b
        z.hidden, z.layers, z.heads, z.kv_heads = t.hidden_size, t.num_hidden_layers, t.num_attention_heads, t.num_key_value_heads
        z.intermediate, z.vocab = t.intermediate_size, t.vocab_size
        z.rms_eps, z.rope_theta = t.rms_norm_eps, t.rope_theta
        for i in range(3):
            z.mrope_section[i] = t.mrope_section[i]
        z.tie_word_embeddings = int(t.tie_word_embeddings)
        z.image_token_id, z.vision_start_token_id = c.image_token_id, c.vision_start_token_id
        z.vision_end_token_id, z.pad_token_id = c.vision_end_token_id, c.pad_token_id
        z.n_eos = len(c.eos_token_ids)
        for i, e in enumerate(c.eos_token_ids):
            z.eos_token_ids[i] = e
        z.max_seqs, z.max_ctx, z.max_patches, z.max_tile_side = max_seqs, max_ctx, max_patches, max_tile_side
        return z

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _use(self, *tensors):
        """The kernels about to be enqueued on the CURRENT stream read these tensors.  A tensor allocated on another stream (a
        tile uploaded or a view resized on the caller's stream, then cropped / encoded on the scheduler's admission stream)
        goes back to ITS stream's pool when the last reference drops, and the caching allocator would hand the block out again
        -- e.g. to the next tile's upload -- while this stream's reads are still queued: record_stream keeps the block until
        they are over (a no-op for a tensor of this stream)."""
        st = torch.cuda.current_stream(self.device)
        for t in tensors:
            if t is not None and t.is_cuda:
                t.record_stream(st)

    def _check(self, code):
        return _lib.check(code, self.h)

    def close(self):
        if getattr(self, "h", None):
            self.lib.ze_engine_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._check(self.lib.ze_sync(self.h, self._stream()))

    # ------------------------------------------------------------------ weights
    def load_weight(self, name: str, array) -> None:
        """array: numpy float32/float16, or a (uint16 view, 'bf16') pair for raw bf16 bits."""
        if isinstance(array, tuple):
            arr, dt = np.ascontiguousarray(array[0]), _lib.ZE_BF16
        else:
            arr = np.ascontiguousarray(array)
            if arr.dtype not in _NP2ZE:
                arr = arr.astype(np.float32)
            dt = _NP2ZE[arr.dtype]
        shape = (C.c_int64 * arr.ndim)(*arr.shape)
        self._check(self.lib.ze_load_weight(self.h, name.encode(), dt, arr.ndim, shape,
                                            arr.ctypes.data_as(C.c_void_p)))

    def load_state_dict(self, items: Iterable) -> None:
        for name, arr in items:
            self.load_weight(name, arr)
        self.assert_ready()

    def fill_synthetic(self, seed: int = 0, std: float = 0.02, matrix_gain: float = 1.0, bias_std: float = 0.0,
                       norm_jitter: float = 0.0) -> None:
        self._check(self.lib.ze_weights_fill_synthetic(self.h, seed, std, matrix_gain, bias_std, norm_jitter))

    def assert_ready(self) -> None:
        n = self.lib.ze_weights_missing(self.h)
        if n != 0:
            raise RuntimeError(self.lib.ze_last_error(self.h).decode())

    def weights_arena(self) -> torch.Tensor:
        """uint8 view of the packed weight arena (no copy), e.g. for one torch.distributed.broadcast over RCCL.  Reading it
        has no side effect; whoever WRITES through it calls weights_invalidate() afterwards (accel.broadcast_engine_weights
        and Accelerator.broadcast_weights do): the fragment / FP8 copies and the captured decode graphs derive from it."""
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self.lib.ze_weights_arena(self.h, C.byref(p), C.byref(n)))

        class _Arena:
            __cuda_array_interface__ = {"shape": (n.value,), "typestr": "|u1", "data": (p.value, False), "version": 2}

        holder = _Arena()
        t = torch.as_tensor(holder, device=self.device)
        t._ze_keepalive = self  # the engine owns the memory
        return t

    def weights_invalidate(self) -> None:
        """After writing through weights_arena() (broadcast, weight refresh): derived copies and graphs are rebuilt."""
        self._check(self.lib.ze_weights_invalidate(self.h))

    # ------------------------------------------------------------------ LoRA adapters
    def lora_create(self) -> int:
        """A resident, inactive, empty adapter (ze_lora_create); at most 8 per engine."""
        a = C.c_int()
        self._check(self.lib.ze_lora_create(self.h, C.byref(a)))
        return int(a.value)

    def lora_add(self, adapter: int, name: str, A, B, scale: float) -> None:
        """The delta of one base tensor (ze_lora_add): `name` its HF key, A [r, cols] and B [rows, r] numpy float32 / float16 or
        (uint16, 'bf16') pairs of one dtype, W' = bf16(W + scale * B @ A).  The shapes are checked against the base tensor."""
        def raw(x):
            if isinstance(x, tuple):
                return np.ascontiguousarray(x[0], dtype=np.uint16), _lib.ZE_BF16
            x = np.ascontiguousarray(x)
            if x.dtype not in _NP2ZE:
                x = x.astype(np.float32)
            return x, _NP2ZE[x.dtype]

        def f32(x, dt):   # exact: bf16 bits are the upper half of the float32 word
            return (x.astype(np.uint32) << 16).view(np.float32) if dt == _lib.ZE_BF16 else x.astype(np.float32)
        (a, da), (b, db) = raw(A), raw(B)
        if da != db:      # (the call carries one dtype)
            a, b, da = f32(a, da), f32(b, db), _lib.ZE_F32
        if a.ndim != 2 or b.ndim != 2 or a.shape[0] != b.shape[1]:
            raise ValueError(f"LoRA shapes for {name}: A {a.shape} has to be [r, cols] and B {b.shape} [rows, r]")
        if name != "lm_head.weight":   # (tied: no tensor of its own; the engine refuses it by name)
            rows, cols, _kind = self.weight_shape(name)
            if b.shape[0] != rows or a.shape[1] != cols:
                raise ValueError(f"LoRA shape mismatch for {name}: B @ A is {b.shape[0]} x {a.shape[1]}, the tensor is {rows} x {cols}")
        self._check(self.lib.ze_lora_add(self.h, int(adapter), name.encode(), da, int(a.shape[0]), float(scale),
                                         a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)))

    def weight_shape(self, name: str):
        """(rows, cols, kind) of an HF tensor by its key in either layout (ze_weight_shape): kind 0 projection matrix, 1 norm weight,
        2 bias, 3 embedding table / lm_head.  A key the engine has no tensor for raises."""
        r, c, k = C.c_int(), C.c_int(), C.c_int()
        self._check(self.lib.ze_weight_shape(self.h, name.encode(), C.byref(r), C.byref(c), C.byref(k)))
        return int(r.value), int(c.value), int(k.value)

    def lora_load(self, tensors) -> int:
        """A new adapter from {base key: (A, B, r, scale)} (checkpoint.read_adapter's second result); returns its id.  On an error
        the half-built adapter is destroyed."""
        a = self.lora_create()
        try:
            for name, (A, B, _r, scale) in tensors.items():
                self.lora_add(a, name, A, B, scale)
        except Exception:
            self.lora_destroy(a)
            raise
        return a

    def lora_activate(self, adapter: Optional[int]) -> None:
        """Merges adapter `adapter` into the weight arena, None = the base weights (ze_lora_activate): one pass per tensor from the
        base store, then everything derived from the weights is dropped as after a weight load.  K/V rows and ViT features computed
        under the previous weights are the caller's to drop."""
        self._check(self.lib.ze_lora_activate(self.h, -1 if adapter is None else int(adapter), self._stream()))

    def lora_destroy(self, adapter: int) -> None:
        self._check(self.lib.ze_lora_destroy(self.h, int(adapter)))

    def lora_info(self):
        """(active adapter or None, resident adapters, bytes of the base store)."""
        a, n, b = C.c_int(), C.c_int(), C.c_size_t()
        self._check(self.lib.ze_lora_info(self.h, C.byref(a), C.byref(n), C.byref(b)))
        return (None if a.value < 0 else int(a.value)), int(n.value), int(b.value)

    def op_lora_merge(self, base: torch.Tensor, A: Optional[torch.Tensor], B: Optional[torch.Tensor], scale: float, dst: torch.Tensor,
                      ld: int, mode: int = 0, offset: int = 0) -> None:
        """The merge kernel alone (ze_op_lora_merge): base bf16 [rows, cols], A f32 [r, cols], B f32 [rows, r] (both None: r = 0, a
        copy), dst a bf16 buffer the mapped rows fit into, leading dimension ld."""
        rows, cols = int(base.shape[0]), int(base.shape[1])
        r = 0 if A is None else int(A.shape[0])
        assert base.dtype == torch.bfloat16 and dst.dtype == torch.bfloat16 and base.is_contiguous()
        assert r == 0 or (A.dtype == torch.float32 and B.dtype == torch.float32 and A.is_contiguous() and B.is_contiguous()
                          and tuple(A.shape) == (r, cols) and tuple(B.shape) == (rows, r))
        last = (offset + rows - 1) if mode == 0 else ((rows - 1) // 16 * 32 + (rows - 1) % 16 + offset)
        assert ld >= cols and offset >= 0 and last * ld + cols <= dst.numel(), "the mapped rows do not fit into dst"
        self._use(base, A, B, dst)
        self._check(self.lib.ze_op_lora_merge(self.h, _ptr(base), rows, cols, _ptr(A), _ptr(B), r, float(scale), _ptr(dst), int(ld),
                                              int(mode), int(offset), self._stream()))

    # ------------------------------------------------------------------ front-end
    def crop_resize(self, tile: torch.Tensor, box: Sequence[int], out_wh: Sequence[int]) -> torch.Tensor:
        """PIL `tile.crop(box).resize(out_wh, BICUBIC)` on a device u8 [H, W, 3] tensor."""
        assert tile.dtype == torch.uint8 and tile.is_cuda and tile.is_contiguous() and tile.shape[-1] == 3
        h, w = int(tile.shape[0]), int(tile.shape[1])
        ow, oh = int(out_wh[0]), int(out_wh[1])
        out = torch.empty((oh, ow, 3), dtype=torch.uint8, device=self.device)
        b = (C.c_int32 * 4)(*[int(v) for v in box])
        self._use(tile)
        self._check(self.lib.ze_op_crop_resize(self.h, _ptr(tile), h, w, b, _ptr(out), oh, ow, self._stream()))
        return out

    def smart_resize(self, h: int, w: int, min_pixels: int, max_pixels: int):
        f = self.config.vision.patch_size * self.config.vision.spatial_merge_size
        oh, ow = C.c_int(), C.c_int()
        _lib.check(self.lib.ze_smart_resize(h, w, f, min_pixels, max_pixels, C.byref(oh), C.byref(ow)))
        return oh.value, ow.value

    def patchify(self, img: torch.Tensor) -> torch.Tensor:
        h, w = int(img.shape[0]), int(img.shape[1])
        p = self.config.vision.patch_size
        out = torch.empty(((h // p) * (w // p), self.patch_dim), dtype=torch.float32, device=self.device)
        self._use(img)
        self._check(self.lib.ze_op_patchify(self.h, _ptr(img), h, w, _ptr(out), self._stream()))
        return out

    def preprocess_image(self, img: torch.Tensor, min_pixels: int = 3136, max_pixels: int = 128 * 128 * 28 * 28):
        """u8 [H, W, 3] device image -> (pixel_values f32 [N, 1176] device, (1, gh, gw))."""
        assert img.dtype == torch.uint8 and img.is_cuda and img.is_contiguous()
        h, w = int(img.shape[0]), int(img.shape[1])
        rh, rw = self.smart_resize(h, w, min_pixels, max_pixels)
        p = self.config.vision.patch_size
        rows = (rh // p) * (rw // p)
        out = torch.empty((rows, self.patch_dim), dtype=torch.float32, device=self.device)
        grid = (C.c_int32 * 3)()
        self._use(img)
        self._check(self.lib.ze_preprocess_image(self.h, _ptr(img), h, w, min_pixels, max_pixels, _ptr(out), rows,
                                                 grid, self._stream()))
        return out, (int(grid[0]), int(grid[1]), int(grid[2]))

    # ------------------------------------------------------------------ index helpers
    def window_index(self, grids):
        g, gp = _i32(np.asarray(grids).reshape(-1, 3))
        n = int((g[:, 0] * g[:, 1] * g[:, 2]).sum()) // (self.config.vision.spatial_merge_size ** 2)
        wi = np.zeros(n, dtype=np.int64)
        cu = np.zeros(n + 2, dtype=np.int32)
        ncu = C.c_int()
        _lib.check(self.lib.ze_vision_window_index(C.byref(self.zcfg), gp, len(g), wi.ctypes.data_as(C.POINTER(C.c_int64)),
                                                   cu.ctypes.data_as(C.POINTER(C.c_int32)), len(cu), C.byref(ncu)))
        return wi, cu[: ncu.value]

    def rope_index(self, input_ids, grids):
        ids, ip = _i32(input_ids)
        g, gp = _i32(np.asarray(grids).reshape(-1, 3)) if len(grids) else (np.zeros((0, 3), np.int32), None)
        pos = np.zeros((3, len(ids)), dtype=np.int32)
        delta = C.c_int32()
        _lib.check(self.lib.ze_rope_index(C.byref(self.zcfg), ip, len(ids), gp, len(g),
                                          pos.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(delta)))
        return pos, int(delta.value)

    # ------------------------------------------------------------------ model
    def vit_forward(self, pixel_values: torch.Tensor, grids) -> torch.Tensor:
        assert pixel_values.dtype == torch.float32 and pixel_values.is_cuda and pixel_values.is_contiguous()
        g, gp = _i32(np.asarray(grids).reshape(-1, 3))
        n = int((g[:, 0] * g[:, 1] * g[:, 2]).sum())
        assert pixel_values.shape[0] == n, (pixel_values.shape, n)
        mu = self.config.vision.spatial_merge_size ** 2
        out = torch.empty((n // mu, self.config.vision.out_hidden_size), dtype=torch.bfloat16, device=self.device)
        self._use(pixel_values)
        self._check(self.lib.ze_vit_forward(self.h, _ptr(pixel_values), gp, len(g), _ptr(out), self._stream()))
        return out

    def seq_reset(self, seq: int):
        self._check(self.lib.ze_seq_reset(self.h, seq, self._stream()))

    def seq_retire(self, seq: int, stream=None):
        """The chain in `seq` is over: chains that read their prompt prefix from its cache move to another holder of the same
        rows.  `stream`: the stream the decode steps run on (default: the current one)."""
        st = C.c_void_p(stream.cuda_stream) if stream is not None else self._stream()
        self._check(self.lib.ze_seq_retire(self.h, seq, st))

    def seq_set_prefix_hint(self, seq: int, src: int, rows: int):
        """Declares that the first `rows` cached tokens of `seq` equal those of chain `src` (rows = 0 clears)."""
        self._check(self.lib.ze_seq_set_prefix_hint(self.h, seq, src, rows, self._stream()))

    def seq_set_split(self, seq: int, rows: int):
        """Measurement / tests: declare the chain's split row by hand (prefilling an image block sets it by itself)."""
        self._check(self.lib.ze_seq_set_split(self.h, int(seq), int(rows), self._stream()))

    def seq_prefix_hint(self, seq: int):
        """(source chain, rows): the decode attention reads the first `rows` cached tokens of `seq` from the source's cache
        (the same bits; one copy per tile in flight); (seq, 0) when it reads its own."""
        h = int(self.lib.ze_seq_prefix_hint(self.h, seq))
        if h < 0:
            self._check(h)
        return (h >> 16, h & 0xffff) if h else (seq, 0)

    def set_sampling_filter(self, seq: int, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0):
        """Top-k / top-p / min-p of chain `seq` (HF's warpers in HF's order, applied on the device inside the sampled step;
        0 / 1.0 / 0.0 = off; None counts as off).  Sampled draws of the chain honour it until the slot is reset, truncated or
        copied into; greedy decoding ignores it.  Chains with different filters share bursts and graphs."""
        self._check(self.lib.ze_seq_set_sampling_filter(self.h, int(seq), int(top_k or 0), float(1.0 if top_p is None else top_p),
                                                        float(min_p or 0.0), self._stream()))

    def _apply_filter(self, seqs, top_k, top_p, min_p):
        if top_k is None and top_p is None and min_p is None:
            return  # (whatever set_sampling_filter left on the chains stays)
        for q in seqs:
            self.set_sampling_filter(int(q), top_k, top_p, min_p)

    def sample_filter(self, logits: torch.Tensor, temperature, top_k, top_p, min_p):
        """The selection kernel alone (ze_op_sample_filter): logits f32 [rows, vocab] (row stride >= vocab), one temperature /
        top_k / top_p / min_p per row (scalars broadcast).  Returns (cut f32 [rows], kept int32 [rows]): row r keeps the
        kept[r] tokens with logits[r] / temperature[r] >= cut[r]."""
        assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
        rows = int(logits.shape[0])
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(temperature, dtype=np.float32), (rows,)))
        k = np.ascontiguousarray(np.broadcast_to(np.asarray(top_k, dtype=np.int32), (rows,)))
        p = np.ascontiguousarray(np.broadcast_to(np.asarray(top_p, dtype=np.float32), (rows,)))
        m = np.ascontiguousarray(np.broadcast_to(np.asarray(min_p, dtype=np.float32), (rows,)))
        cut = torch.empty(rows, dtype=torch.float32, device=self.device)
        kept = torch.empty(rows, dtype=torch.int32, device=self.device)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        ld = int(logits.stride(0)) if rows > 1 else int(logits.shape[1])   # (the stride of a one-row tensor means nothing)
        self._check(self.lib.ze_op_sample_filter(self.h, _ptr(logits), rows, int(logits.shape[1]), ld,
                                                 t.ctypes.data_as(fp), k.ctypes.data_as(ip), p.ctypes.data_as(fp),
                                                 m.ctypes.data_as(fp), _ptr(cut), _ptr(kept), self._stream()))
        return cut, kept

    def set_entropy_filter(self, seq: int, typical_p: float = 1.0, epsilon_cutoff: float = 0.0, eta_cutoff: float = 0.0):
        """Typical-p / epsilon / eta cutoffs of chain `seq` (HF's warpers in HF's order, behind top-k / top-p / min-p, applied on
        the device inside the sampled step; 1.0 / 0.0 / 0.0 = off; None counts as off).  Honoured and cleared wherever the
        sampling filter is; greedy decoding ignores it; a speculating chain refuses it."""
        self._check(self.lib.ze_seq_set_entropy_filter(self.h, int(seq), float(1.0 if typical_p is None else typical_p),
                                                       float(epsilon_cutoff or 0.0), float(eta_cutoff or 0.0), self._stream()))

    def sample_band(self, logits: torch.Tensor, temperature, top_k=0, top_p=1.0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0,
                    eta_cutoff=0.0):
        """The selection of the whole warper chain alone (ze_op_sample_band): logits f32 [rows, vocab] (row stride >= vocab), the
        settings per row (scalars broadcast).  Returns (cut f32 [rows], ceil f32 [rows], kept int32 [rows]): row r keeps the
        kept[r] tokens with cut[r] <= logits[r] / temperature[r] <= ceil[r]."""
        assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
        rows = int(logits.shape[0])

        def per_row(v, dtype):
            return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (rows,)))
        f = [per_row(v, np.float32) for v in (temperature, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff)]
        k = per_row(top_k, np.int32)
        cut = torch.empty(rows, dtype=torch.float32, device=self.device)
        ceil = torch.empty(rows, dtype=torch.float32, device=self.device)
        kept = torch.empty(rows, dtype=torch.int32, device=self.device)
        fp = C.POINTER(C.c_float)
        ld = int(logits.stride(0)) if rows > 1 else int(logits.shape[1])   # (the stride of a one-row tensor means nothing)
        self._use(logits)
        self._check(self.lib.ze_op_sample_band(self.h, _ptr(logits), rows, int(logits.shape[1]), ld, f[0].ctypes.data_as(fp),
                                               k.ctypes.data_as(C.POINTER(C.c_int32)), *(a.ctypes.data_as(fp) for a in f[1:]),
                                               _ptr(cut), _ptr(ceil), _ptr(kept), self._stream()))
        return cut, ceil, kept

    def sample_rows_band(self, logits: torch.Tensor, temperature, cut, ceil, repetition_penalty=1.0, seed=0, sample_stream=0,
                         index=0, seen: Optional[torch.Tensor] = None) -> torch.Tensor:
        """sample_rows under a band per row (ze_op_sample_rows_band): a sampled row draws among the tokens with cut[r] <=
        score / temperature[r] <= ceil[r] (host values, scalars broadcast).  Returns the tokens, int32 [rows]."""
        assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
        rows, vocab = int(logits.shape[0]), int(logits.shape[1])
        if seen is not None:
            assert seen.dtype == torch.uint8 and seen.is_contiguous() and tuple(seen.shape) == (rows, vocab)
            self._use(seen)

        def per_row(v, dtype):
            return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (rows,)))
        t, pen = per_row(temperature, np.float32), per_row(repetition_penalty, np.float32)
        sd, strm, idx = per_row(seed, np.uint64), per_row(sample_stream, np.int32), per_row(index, np.int32)
        lo, hi = per_row(cut, np.float32), per_row(ceil, np.float32)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        out = torch.empty(rows, dtype=torch.int32, device=self.device)
        ld = int(logits.stride(0)) if rows > 1 else vocab   # (the stride of a one-row tensor means nothing)
        self._use(logits)
        self._check(self.lib.ze_op_sample_rows_band(
            self.h, _ptr(logits), rows, vocab, ld, _ptr(seen) if seen is not None else None, t.ctypes.data_as(fp),
            pen.ctypes.data_as(fp), sd.ctypes.data_as(C.POINTER(C.c_uint64)), strm.ctypes.data_as(ip), idx.ctypes.data_as(ip),
            lo.ctypes.data_as(fp), hi.ctypes.data_as(fp), _ptr(out), self._stream()))
        return out

    def _apply_entropy_filter(self, seqs, typical_p, epsilon_cutoff, eta_cutoff):
        if typical_p is None and epsilon_cutoff is None and eta_cutoff is None:
            return  # (whatever set_entropy_filter left on the chains stays)
        for q in seqs:
            self.set_entropy_filter(int(q), typical_p, epsilon_cutoff, eta_cutoff)

    def set_sampling(self, seq: int, do_sample: Optional[bool] = None, temperature: float = 1.0, seed: int = 0,
                     repetition_penalty: float = 1.0):
        """Sampling request of chain `seq` (ze_seq_set_sampling): do_sample False = greedy, True = temperature sampling with the
        chain's own temperature and seed, None = clear (the chain follows the call's gen_params again); repetition_penalty is
        the chain's own in both modes.  Replaces the do_sample / temperature / seed / repetition_penalty of the gen_params of
        every generate / chain_begin / decode_burst call the chain takes part in, until the slot is reset, truncated or copied
        into.  Chains with different requests share bursts and graphs; a chain's tokens are those of a call whose gen_params
        carry its values."""
        mode = -1 if do_sample is None else int(bool(do_sample))
        self._check(self.lib.ze_seq_set_sampling(self.h, int(seq), mode, float(temperature), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                 float(repetition_penalty), self._stream()))

    def sample_rows(self, logits: torch.Tensor, temperature, repetition_penalty=1.0, seed=0, sample_stream=0, index=0,
                    seen: Optional[torch.Tensor] = None, top_k=None, top_p=None, min_p=None) -> torch.Tensor:
        """One draw per row with values of its own (ze_op_sample_rows, the per-chain sampling kernels of the batched step): logits
        f32 [rows, vocab] (row stride >= vocab); temperature (0 = greedy), repetition_penalty, seed, sample_stream and index per
        row (scalars broadcast); seen uint8 [rows, vocab] (nonzero = penalised) or None; top_k / top_p / min_p per row, or all
        None.  Returns the tokens, int32 [rows]; marks nothing as seen."""
        assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
        rows, vocab = int(logits.shape[0]), int(logits.shape[1])
        if seen is not None:
            assert seen.dtype == torch.uint8 and seen.is_contiguous() and tuple(seen.shape) == (rows, vocab)
            self._use(seen)

        def per_row(v, dtype):
            return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (rows,)))
        t, pen = per_row(temperature, np.float32), per_row(repetition_penalty, np.float32)
        sd, strm, idx = per_row(seed, np.uint64), per_row(sample_stream, np.int32), per_row(index, np.int32)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        filt = (None, None, None)
        if top_k is not None or top_p is not None or min_p is not None:
            filt = (per_row(0 if top_k is None else top_k, np.int32), per_row(1.0 if top_p is None else top_p, np.float32),
                    per_row(0.0 if min_p is None else min_p, np.float32))
        out = torch.empty(rows, dtype=torch.int32, device=self.device)
        ld = int(logits.stride(0)) if rows > 1 else vocab   # (the stride of a one-row tensor means nothing)
        self._use(logits)
        self._check(self.lib.ze_op_sample_rows(
            self.h, _ptr(logits), rows, vocab, ld, _ptr(seen) if seen is not None else None, t.ctypes.data_as(fp),
            pen.ctypes.data_as(fp), sd.ctypes.data_as(C.POINTER(C.c_uint64)), strm.ctypes.data_as(ip), idx.ctypes.data_as(ip),
            filt[0].ctypes.data_as(ip) if filt[0] is not None else None, filt[1].ctypes.data_as(fp) if filt[1] is not None else None,
            filt[2].ctypes.data_as(fp) if filt[2] is not None else None, _ptr(out), self._stream()))
        return out

    def set_logprobs(self, seq: int, top_n: Optional[int] = 0):
        """Log-probabilities of the tokens chain `seq` generates from now on (ze_seq_set_logprobs): None / -1 = off, 0 = the chosen
        token only, 1 .. MAX_TOP_LOGPROBS = that many best alternatives too.  Computed on the device from the step's own fp32
        logits (before repetition penalty, temperature and filters); held until the slot is reset, truncated or copied into.
        Chains with and without a request share bursts and graphs."""
        self._check(self.lib.ze_seq_set_logprobs(self.h, int(seq), -1 if top_n is None else int(top_n), self._stream()))

    def chain_logprobs(self, seq: int, capacity: int = 0, stream=None):
        """The entries of the tokens chain_tokens(seq) returns: (logprobs f32 [n], top_ids int32 [n, N], top_logprobs f32 [n, N]),
        N the chain's own request; places a row could not fill are (-1, -inf).  Raises for a chain without a request."""
        cap = max(1, min(int(capacity) if capacity else self.max_ctx, self.max_ctx))
        lp = np.empty(cap, dtype=np.float32)
        ids = np.empty((cap, MAX_TOP_LOGPROBS), dtype=np.int32)
        tlp = np.empty((cap, MAX_TOP_LOGPROBS), dtype=np.float32)
        n, tn = C.c_int(), C.c_int()
        st = C.c_void_p(stream.cuda_stream) if stream is not None else self._stream()
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        self._check(self.lib.ze_chain_logprobs(self.h, int(seq), lp.ctypes.data_as(fp), ids.ctypes.data_as(ip),
                                               tlp.ctypes.data_as(fp), cap, C.byref(n), C.byref(tn), st))
        m, N = n.value, tn.value  # (the C arrays are [capacity, N] packed)
        return (lp[:m].copy(), ids.reshape(-1)[:m * N].reshape(m, N).copy(), tlp.reshape(-1)[:m * N].reshape(m, N).copy())

    def chain_logprobs_batch(self, seqs, top_n: int = 0, capacity: int = 0, stream=None):
        """chain_logprobs for several chains in one device -> host copy and one wait: a list of (logprobs [n_i], top_ids
        [n_i, top_n], top_logprobs [n_i, top_n]); places beyond a chain's own request are (-1, -inf)."""
        if not len(seqs):
            return []
        cap = max(1, min(int(capacity) if capacity else self.max_ctx, self.max_ctx))
        N = int(top_n)
        sq, sp = _i32(seqs)
        lp = np.empty((len(sq), cap), dtype=np.float32)
        ids = np.empty((len(sq), cap, max(N, 1)), dtype=np.int32)
        tlp = np.empty((len(sq), cap, max(N, 1)), dtype=np.float32)
        n = (C.c_int32 * len(sq))()
        st = C.c_void_p(stream.cuda_stream) if stream is not None else self._stream()
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        self._check(self.lib.ze_chain_logprobs_batch(self.h, sp, len(sq), lp.ctypes.data_as(fp),
                                                     ids.ctypes.data_as(ip) if N else None, tlp.ctypes.data_as(fp) if N else None,
                                                     cap, N, n, st))
        return [(lp[i, :n[i]].copy(), ids[i, :n[i], :N].copy(), tlp[i, :n[i], :N].copy()) for i in range(len(sq))]

    def op_token_logprobs(self, logits: torch.Tensor, targets: torch.Tensor, top_n: int = 0):
        """The kernel alone (ze_op_token_logprobs): logits f32 [rows, vocab] (row stride >= vocab), targets int32 [rows].  Returns
        (logprob f32 [rows], top_ids int32 [rows, top_n], top_logprobs f32 [rows, top_n]): log_softmax(logits)[target] and the
        top_n largest entries in (value descending, id ascending) order."""
        assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
        assert targets.dtype == torch.int32 and targets.is_contiguous()
        rows = int(logits.shape[0])
        out = torch.empty(rows, dtype=torch.float32, device=self.device)
        ids = torch.empty((rows, max(int(top_n), 0)), dtype=torch.int32, device=self.device)
        tlp = torch.empty((rows, max(int(top_n), 0)), dtype=torch.float32, device=self.device)
        ld = int(logits.stride(0)) if rows > 1 else int(logits.shape[1])   # (the stride of a one-row tensor means nothing)
        self._check(self.lib.ze_op_token_logprobs(self.h, _ptr(logits), rows, int(logits.shape[1]), ld, _ptr(targets),
                                                  int(top_n), _ptr(out), _ptr(ids) if top_n > 0 else None,
                                                  _ptr(tlp) if top_n > 0 else None, self._stream()))
        return out, ids, tlp

    def seq_set_logit_adjust(self, seq: int, presence_penalty: float = 0.0, frequency_penalty: float = 0.0,
                             min_new_tokens: int = 0, logit_bias=None):
        """Additive logit adjustments of chain `seq` (ze_seq_set_logit_adjust), applied on the device to every step's row before
        the repetition penalty, temperature, filters and the draw -- greedy decoding included: `logit_bias` {token id: bias} (or
        (id, bias) pairs; at most MAX_LOGIT_BIAS, -inf bans the token), OpenAI's presence / frequency penalties over the counts
        of the tokens the chain generates from now on, and the EOS ids banned until min_new_tokens were generated.  Set after the
        chain's prefill and before its first draw; all-off values clear the request; held until the slot is reset, truncated or
        copied into.  Chains with and without a request share bursts and graphs."""
        pairs = list(logit_bias.items()) if hasattr(logit_bias, "items") else list(logit_bias or ())
        ids = np.ascontiguousarray([int(k) for k, _ in pairs], dtype=np.int32)
        vals = np.ascontiguousarray([float(v) for _, v in pairs], dtype=np.float32)
        self._check(self.lib.ze_seq_set_logit_adjust(self.h, int(seq), float(presence_penalty or 0.0), float(frequency_penalty or 0.0),
                                                     int(min_new_tokens or 0), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     vals.ctypes.data_as(C.POINTER(C.c_float)), len(pairs), self._stream()))

    def op_logit_adjust(self, logits: torch.Tensor, counts=None, presence=0.0, frequency=0.0, eos_masked=0, bias=None,
                        out: Optional[torch.Tensor] = None):
        """The kernel alone (ze_op_logit_adjust): logits f32 [rows, vocab] (row stride >= vocab), counts uint16-valued [rows, vocab]
        (a torch.int16 tensor holding the bit patterns, or a numpy uint16 array) or None, presence / frequency / eos_masked per row
        (scalars broadcast), bias: per row a list of (id, value) pairs (or a dict), or None.  Returns the adjusted rows, f32 with the
        stride of `logits` (columns beyond vocab are not written)."""
        assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
        rows, vocab = int(logits.shape[0]), int(logits.shape[1])
        ld = int(logits.stride(0)) if rows > 1 else vocab   # (the stride of a one-row tensor means nothing)
        dev = self.device

        def per_row(x, dt):
            return torch.from_numpy(np.broadcast_to(np.asarray(x, dtype=dt), (rows,)).copy()).to(dev)

        pr, fr, em = per_row(presence, np.float32), per_row(frequency, np.float32), per_row(eos_masked, np.int32)
        lists = [list(b.items()) if hasattr(b, "items") else list(b or ()) for b in (bias if bias is not None else [None] * rows)]
        assert len(lists) == rows
        off = np.zeros(rows + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(b) for b in lists])
        ids = np.asarray([int(k) for b in lists for k, _ in b] + [0], dtype=np.int32)   # (+ one entry: never an empty tensor)
        vals = np.asarray([float(v) for b in lists for _, v in b] + [0.0], dtype=np.float32)
        off_d, ids_d, vals_d = (torch.from_numpy(x).to(dev) for x in (off, ids, vals))
        if counts is not None:
            if isinstance(counts, np.ndarray):
                counts = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.uint16).view(np.int16)).to(dev)
            assert counts.dtype == torch.int16 and counts.is_contiguous() and tuple(counts.shape) == (rows, vocab)
        if out is None:
            out = torch.empty_strided((rows, vocab), (ld, 1), dtype=torch.float32, device=dev)
        assert out.dtype == torch.float32 and out.stride(1) == 1 and (rows <= 1 or int(out.stride(0)) == ld)
        self._check(self.lib.ze_op_logit_adjust(self.h, _ptr(logits), rows, vocab, ld, _ptr(counts) if counts is not None else None,
                                                _ptr(pr), _ptr(fr), _ptr(em), _ptr(off_d), _ptr(ids_d), _ptr(vals_d), _ptr(out),
                                                self._stream()))
        self._keep = (pr, fr, em, off_d, ids_d, vals_d, counts)   # (the launch is asynchronous: alive until the next one)
        return out

    def set_token_rules(self, seq: int, no_repeat_ngram_size: int = 0, stop=(), bad_words=(), context=None):
        """Token rules of chain `seq` (ze_seq_set_token_rules), on the device inside every step: HF's `no_repeat_ngram_size` and
        `bad_words_ids` (lists of token ids) over `context` (normally the prompt ids) + the generated ids, and `stop`: token-id
        sequences that finish the chain, as an EOS does, when one ends the generated ids.  Set after the chain's prefill and before
        its first draw; all-off values clear the request; held until the slot is reset, truncated or copied into.  Chains with and
        without rules share bursts and graphs."""
        stop, bad = [list(r) for r in (stop or ())], [list(r) for r in (bad_words or ())]
        sp, bp = pack_records(stop), pack_records(bad)
        ctx = np.ascontiguousarray([] if context is None else context, dtype=np.int32).reshape(-1)
        i32 = C.POINTER(C.c_int32)
        self._check(self.lib.ze_seq_set_token_rules(self.h, int(seq), int(no_repeat_ngram_size or 0), sp.ctypes.data_as(i32), len(stop),
                                                    bp.ctypes.data_as(i32), len(bad), ctx.ctypes.data_as(i32), int(ctx.size),
                                                    self._stream()))

    def op_token_rules(self, logits: torch.Tensor, histories, n_context=0, no_repeat_ngram_size=0, bad_words=None, stop=None,
                       min_new=0, out: Optional[torch.Tensor] = None):
        """The kernels alone (ze_op_token_rules): logits f32 [rows, vocab] (row stride >= vocab), `histories` one id list per row
        whose first n_context ids are the context, no_repeat_ngram_size / n_context / min_new per row (scalars broadcast),
        bad_words / stop per row a list of id lists (or None).  Returns (rows with -inf at the banned ids, f32 with the stride of
        `logits`, columns beyond vocab not written; stop flags int32 [rows])."""
        assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
        rows, vocab = int(logits.shape[0]), int(logits.shape[1])
        ld = int(logits.stride(0)) if rows > 1 else vocab
        dev = self.device
        assert len(histories) == rows

        def per_row(x):
            return np.broadcast_to(np.asarray(x, dtype=np.int32), (rows,)).copy()

        def flat(lists):
            off = np.zeros(rows + 1, dtype=np.int32)
            off[1:] = np.cumsum([len(x) for x in lists])
            return np.concatenate([np.asarray(x, dtype=np.int32).reshape(-1) for x in lists] + [np.zeros(4, np.int32)]), off

        hist, hoff = flat(histories)
        ban, boff = flat([pack_records(b or ()) for b in (bad_words if bad_words is not None else [None] * rows)])
        stp, soff = flat([pack_records(b or ()) for b in (stop if stop is not None else [None] * rows)])
        host = (hist, hoff, per_row(n_context), per_row(no_repeat_ngram_size), ban, boff, stp, soff, per_row(min_new))
        d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in host]
        if out is None:
            out = torch.empty_strided((rows, vocab), (ld, 1), dtype=torch.float32, device=dev)
        assert out.dtype == torch.float32 and out.stride(1) == 1 and (rows <= 1 or int(out.stride(0)) == ld)
        hit = torch.zeros(rows, dtype=torch.int32, device=dev)
        self._check(self.lib.ze_op_token_rules(self.h, _ptr(logits), rows, vocab, ld, *[_ptr(x) for x in d], _ptr(out), _ptr(hit),
                                               self._stream()))
        self._keep = d   # (the launch is asynchronous: alive until the next one)
        return out, hit

    def grammar_create(self, automaton) -> int:
        """A grammar on the device (ze_grammar_create): `automaton` has token_class uint16 [vocab], trans int16 [n_states, n_classes]
        (-1 = not allowed) and accepting uint8 [n_states] -- what zoomearth_amd.grammar.compile_regex / compile_choice return.
        Returns its id; at most MAX_GRAMMARS live at once.  Off the step path: it waits for the current stream."""
        tc = np.ascontiguousarray(automaton.token_class, dtype=np.uint16).reshape(-1)
        tr = np.ascontiguousarray(automaton.trans, dtype=np.int16)
        ac = np.ascontiguousarray(automaton.accepting, dtype=np.uint8).reshape(-1)
        if tr.ndim != 2 or ac.size != tr.shape[0] or tc.size != self.config.text.vocab_size:
            raise ValueError("automaton: token_class [vocab], trans [n_states, n_classes], accepting [n_states]")
        out = C.c_int(-1)
        self._check(self.lib.ze_grammar_create(self.h, tc.ctypes.data_as(C.POINTER(C.c_uint16)), int(tr.shape[1]),
                                               tr.ctypes.data_as(C.POINTER(C.c_int16)), int(tr.shape[0]),
                                               ac.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(out), self._stream()))
        return out.value

    def grammar_destroy(self, grammar: int):
        """Frees the grammar's id (ze_grammar_destroy); refused while a chain still uses it."""
        self._check(self.lib.ze_grammar_destroy(self.h, int(grammar)))

    def set_grammar(self, seq: int, grammar: Optional[int], state: int = 0):
        """Chain `seq` is held to `grammar` from `state` on (ze_seq_set_grammar), on the device inside every step: before each draw
        every token the automaton does not allow in the chain's state is -inf, after it the state moves on.  None / -1 clears.  Set
        after the chain's prefill and before its first draw; held until the slot is reset, truncated or copied into.  Chains of
        different grammars, states and none share bursts and graphs."""
        self._check(self.lib.ze_seq_set_grammar(self.h, int(seq), -1 if grammar is None else int(grammar), int(state), self._stream()))

    def chain_grammar_state(self, seq: int):
        """(state, violated) of chain `seq` (ze_chain_grammar_state); state -1: the chain has no grammar.  Waits for the stream."""
        st, vi = C.c_int(-1), C.c_int(0)
        self._check(self.lib.ze_chain_grammar_state(self.h, int(seq), C.byref(st), C.byref(vi), self._stream()))
        return st.value, vi.value

    def op_grammar_mask(self, grammar: int, logits: torch.Tensor, states, out: Optional[torch.Tensor] = None):
        """The mask kernel alone (ze_op_grammar_mask): logits f32 [rows, vocab] (row stride >= vocab, vocab <= the engine's), states
        per row (-1: a row without a grammar).  Returns the rows with -inf at every id the row's state does not allow, f32 with the
        stride of `logits` (columns beyond vocab are not written)."""
        assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
        rows, vocab = int(logits.shape[0]), int(logits.shape[1])
        ld = int(logits.stride(0)) if rows > 1 else vocab
        st = torch.from_numpy(np.broadcast_to(np.asarray(states, dtype=np.int32), (rows,)).copy()).to(self.device)
        if out is None:
            out = torch.empty_strided((rows, vocab), (ld, 1), dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.stride(1) == 1 and (rows <= 1 or int(out.stride(0)) == ld)
        self._check(self.lib.ze_op_grammar_mask(self.h, int(grammar), _ptr(logits), rows, vocab, ld, _ptr(st), _ptr(out), self._stream()))
        self._keep = (st,)   # (the launch is asynchronous: alive until the next one)
        return out

    def op_grammar_advance(self, grammar: int, states, tokens) -> torch.Tensor:
        """The advance kernel alone (ze_op_grammar_advance): int32 [rows] next states, -1 where the token is not allowed."""
        st = torch.from_numpy(np.ascontiguousarray(states, dtype=np.int32).reshape(-1)).to(self.device)
        tk = torch.from_numpy(np.ascontiguousarray(tokens, dtype=np.int32).reshape(-1)).to(self.device)
        assert st.numel() == tk.numel()
        out = torch.empty(max(st.numel(), 1), dtype=torch.int32, device=self.device)
        self._check(self.lib.ze_op_grammar_advance(self.h, int(grammar), _ptr(st), _ptr(tk), int(st.numel()), _ptr(out), self._stream()))
        self._keep = (st, tk)
        return out[:st.numel()]

    def seq_truncate(self, seq: int, keep: int):
        self._check(self.lib.ze_seq_truncate(self.h, seq, keep, self._stream()))

    def seq_copy_prefix(self, dst: int, src: int, n_tokens: int):
        """Chain `dst` becomes the first n_tokens cached tokens of chain `src` (shared prompt prefix: K/V rows copied)."""
        self._check(self.lib.ze_seq_copy_prefix(self.h, dst, src, n_tokens, self._stream()))

    def seq_fork(self, src: int, dsts):
        """Every chain of `dsts` becomes the prefilled chain `src` -- K/V rows, last-position logits and repetition-penalty marks, in
        one launch -- exactly as if it had prefilled the whole prompt itself: `chain_begin` can follow at once, after the chain's
        own requests are installed (the fork clears the slot's previous ones).  `src` must not have drawn a token since its prefill."""
        a, p = _i32(list(dsts))
        self._check(self.lib.ze_seq_fork(self.h, int(src), p, len(a), self._stream()))

    # -- beam search (csrc/ze_beam.hip)
    EARLY_STOPPING = {False: 0, True: 1, "never": 2}

    def _beam_params(self, num_beams, num_return_sequences, max_new_tokens, length_penalty, early_stopping, repetition_penalty,
                     use_graph=True, sync_every=8):
        if early_stopping not in self.EARLY_STOPPING:
            raise ValueError(f"early_stopping must be False, True or 'never', not {early_stopping!r}")
        return _lib.ZeBeamParams(int(num_beams), int(num_return_sequences), int(max_new_tokens), float(length_penalty),
                                 self.EARLY_STOPPING[early_stopping], float(repetition_penalty), int(bool(use_graph)), int(sync_every))

    def beam_search(self, seqs, groups: int, num_beams: int, max_new_tokens: int, num_return_sequences: int = 1,
                    length_penalty: float = 1.0, early_stopping=False, repetition_penalty: float = 1.0, use_graph: bool = True,
                    sync_every: int = 8):
        """Beam search over `groups` prompts (ze_beam_search): seqs[g * num_beams] is the prefilled, unstepped chain of group g, the
        other slots of the group are taken by the call.  Returns (tokens, scores, beam_indices): per group a list of
        num_return_sequences id lists, best first; HF's sequences_scores [groups, n]; and the beam indices per returned sequence."""
        sq, sp = _i32(list(seqs))
        if len(sq) != groups * num_beams:
            raise ValueError("seqs must name groups * num_beams slots")
        p = self._beam_params(num_beams, num_return_sequences, max_new_tokens, length_penalty, early_stopping, repetition_penalty,
                              use_graph, sync_every)
        n = groups * num_return_sequences
        tok = np.zeros((max(n, 1), max(max_new_tokens, 1)), np.int32)
        bix = np.zeros_like(tok)
        ln = np.zeros(max(n, 1), np.int32)
        sc = np.zeros(max(n, 1), np.float32)
        self._check(self.lib.ze_beam_search(self.h, sp, int(groups), C.byref(p), tok.ctypes.data_as(C.POINTER(C.c_int32)),
                                            ln.ctypes.data_as(C.POINTER(C.c_int32)), sc.ctypes.data_as(C.POINTER(C.c_float)),
                                            bix.ctypes.data_as(C.POINTER(C.c_int32)), self._stream()))
        R = num_return_sequences
        tokens = [[tok[g * R + r, :ln[g * R + r]].tolist() for r in range(R)] for g in range(groups)]
        indices = [[bix[g * R + r, :ln[g * R + r]].tolist() for r in range(R)] for g in range(groups)]
        return tokens, sc[:n].reshape(groups, R).copy(), indices

    def op_beam_step(self, seqs, groups: int, logits: torch.Tensor, begin: bool, num_beams: int, max_new_tokens: int,
                     length_penalty: float = 1.0, early_stopping=False, repetition_penalty: float = 1.0, vocab: Optional[int] = None):
        """One beam step on the caller's logits rows [groups * num_beams, ld] (ze_op_beam_step); returns a dict of host arrays:
        parent, token, score, rank per row and done per group."""
        sq, sp = _i32(list(seqs))
        assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 and logits.shape[0] == len(sq)
        p = self._beam_params(num_beams, 1, max_new_tokens, length_penalty, early_stopping, repetition_penalty)
        n = len(sq)
        par, tok, rank = (np.zeros(n, np.int32) for _ in range(3))
        sc = np.zeros(n, np.float32)
        done = np.zeros(groups, np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self.lib.ze_op_beam_step(self.h, sp, int(groups), C.byref(p), int(bool(begin)), _ptr(logits),
                                             int(vocab if vocab is not None else logits.shape[1]), int(logits.stride(0)), ip(par), ip(tok),
                                             sc.ctypes.data_as(C.POINTER(C.c_float)), ip(rank), ip(done), self._stream()))
        return dict(parent=par, token=tok, score=sc, rank=rank, done=done)

    def op_beam_finished(self, groups: int, num_beams: int, max_new_tokens: int):
        """The finished pools of the last beam call, by rank: dict of tokens (lists), scores, beam_indices (lists), finished."""
        n = groups * num_beams
        tok = np.zeros((n, max_new_tokens), np.int32)
        bix = np.zeros_like(tok)
        ln, fin = np.zeros(n, np.int32), np.zeros(n, np.int32)
        sc = np.zeros(n, np.float32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self.lib.ze_op_beam_finished(self.h, int(groups), ip(tok), ip(ln), sc.ctypes.data_as(C.POINTER(C.c_float)), ip(bix),
                                                 ip(fin), self._stream()))
        return dict(tokens=[tok[i, :ln[i]].tolist() for i in range(n)], scores=sc, beam_indices=[bix[i, :ln[i]].tolist() for i in range(n)],
                    finished=fin)

    def op_kv_reorder(self, pairs, row0: int, rows: int):
        """Cached rows [row0, row0 + rows) of every layer: chain dst takes chain src's, for every (src, dst) of `pairs` (ze_op_kv_reorder)."""
        src, sp = _i32([a for a, _ in pairs])
        dst, dp = _i32([b for _, b in pairs])
        self._check(self.lib.ze_op_kv_reorder(self.h, sp, dp, len(src), int(row0), int(rows), self._stream()))

    # -- prefix cache: the engine's pool of K/V blocks (zoomearth_amd/prefix_cache.py decides what is in them)
    def prefix_pool_create(self, n_blocks: int, block_rows: int) -> None:
        self._check(self.lib.ze_prefix_pool_create(self.h, int(n_blocks), int(block_rows)))

    def prefix_pool_destroy(self) -> None:
        self._check(self.lib.ze_prefix_pool_destroy(self.h))

    def prefix_pool_info(self):
        """(n_blocks, block_rows, generation): the pool's sizes (0, 0 without one) and the engine's weight generation."""
        nb, br, gen = C.c_int(), C.c_int(), C.c_uint()
        self._check(self.lib.ze_prefix_pool_info(self.h, C.byref(nb), C.byref(br), C.byref(gen)))
        return nb.value, br.value, gen.value

    def prefix_save(self, seq: int, row0: int, blocks, stream=None) -> None:
        """Rows [row0, row0 + len(blocks) * block_rows) of chain `seq` into the pool blocks `blocks`."""
        a, p = _i32(list(blocks))
        st = C.c_void_p(stream.cuda_stream) if stream is not None else self._stream()
        self._check(self.lib.ze_prefix_save(self.h, int(seq), int(row0), p, len(a), st))

    def prefix_load(self, blocks, n_rows: int, split_row: int, dsts) -> None:
        """The first n_rows rows held by `blocks` become the chains `dsts`: the first as if it had prefilled them, the others as if
        they had copied them from it (`seq_copy_prefix`); the tail's prefill follows."""
        a, p = _i32(list(blocks))
        d, dp = _i32(list(dsts))
        self._check(self.lib.ze_prefix_load(self.h, p, len(a), int(n_rows), int(split_row), dp, len(d), self._stream()))

    def seq_len(self, seq: int) -> int:
        return self._check(self.lib.ze_seq_len(self.h, seq))

    def mark_seen(self, seq: int, ids):
        a, p = _i32(ids)
        self._check(self.lib.ze_seq_mark_seen(self.h, seq, p, len(a), self._stream()))

    def mark_seen_batch(self, seqs, ids_list):
        """mark_seen for the chains of a prefill pass at once (one copy, one launch)."""
        if not len(seqs):
            return
        sq, sp = _i32(seqs)
        cnt, cp = _i32([len(x) for x in ids_list])
        flat, fp = _i32(np.concatenate([np.asarray(x, dtype=np.int32) for x in ids_list]) if len(ids_list) else [])
        self._check(self.lib.ze_seq_mark_seen_batch(self.h, sp, cp, len(sq), fp, self._stream()))

    def prefill(self, seq: int, new_ids, image_embeds, position_ids, rope_delta: int, want_logits: bool = True):
        """Appends `new_ids` to chain `seq`. position_ids: int32 [3, len(new_ids)]."""
        ids, ip = _i32(new_ids)
        pos, pp = _i32(position_ids)
        assert pos.shape == (3, len(ids))
        n_img = 0 if image_embeds is None else int(image_embeds.shape[0])
        if image_embeds is not None:
            assert image_embeds.dtype == torch.bfloat16 and image_embeds.is_contiguous()
        logits = torch.empty(self.config.text.vocab_size, dtype=torch.float32, device=self.device) if want_logits else None
        self._use(image_embeds)
        self._check(self.lib.ze_prefill(self.h, seq, ip, len(ids), _ptr(image_embeds), n_img, pp, rope_delta,
                                        _ptr(logits), self._stream()))
        return logits

    def score(self, seq: int, new_ids, image_embeds, position_ids, rope_delta: int):
        """prefill() plus the log-probability of every next id: returns f32 [len(new_ids) - 1] with
        out[t] = log_softmax(logits[t])[new_ids[t + 1]] (ze_score; replaces _get_per_token_logps of the reference's
        GRPO trainer)."""
        ids, ip = _i32(new_ids)
        pos, pp = _i32(position_ids)
        assert pos.shape == (3, len(ids))
        n_img = 0 if image_embeds is None else int(image_embeds.shape[0])
        if image_embeds is not None:
            assert image_embeds.dtype == torch.bfloat16 and image_embeds.is_contiguous()
        out = torch.empty(max(len(ids) - 1, 0), dtype=torch.float32, device=self.device)
        self._check(self.lib.ze_score(self.h, seq, ip, len(ids), _ptr(image_embeds), n_img, pp, rope_delta,
                                      _ptr(out) if len(ids) > 1 else _ptr(torch.empty(1, dtype=torch.float32, device=self.device)),
                                      self._stream()))
        return out

    def op_token_logprob(self, logits: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        """log_softmax(logits, -1).gather(targets) in fp32 for bf16 logits [rows, vocab] (row stride % 8 == 0)."""
        assert logits.dtype == torch.bfloat16 and logits.dim() == 2 and logits.stride(1) == 1
        assert targets.dtype == torch.int32 and targets.is_contiguous()
        out = torch.empty(logits.shape[0], dtype=torch.float32, device=self.device)
        self._check(self.lib.ze_op_token_logprob(self.h, _ptr(logits), logits.shape[0], logits.shape[1],
                                                 logits.stride(0), _ptr(targets), _ptr(out), self._stream()))
        return out

    def op_score_detail(self, logits: torch.Tensor, targets: torch.Tensor, top_n: int = 0) -> "ScoreDetail":
        """The kernel of score_batch_detail alone (ze_op_score_detail) on bf16 logits [rows, vocab] (row stride % 8 == 0): per row
        the log-probability of its target (the bits of op_token_logprob), the entropy, the target's rank and, for top_n > 0, the
        top_n first ids of (value descending, id ascending) with their log-probabilities."""
        assert logits.dtype == torch.bfloat16 and logits.dim() == 2 and logits.stride(1) == 1
        assert targets.dtype == torch.int32 and targets.is_contiguous()
        rows, n = int(logits.shape[0]), int(top_n)
        lp = torch.empty(rows, dtype=torch.float32, device=self.device)
        ent = torch.empty(rows, dtype=torch.float32, device=self.device)
        rank = torch.empty(rows, dtype=torch.int32, device=self.device)
        ids = torch.empty((rows, n), dtype=torch.int32, device=self.device) if n > 0 else None
        tlp = torch.empty((rows, n), dtype=torch.float32, device=self.device) if n > 0 else None
        self._check(self.lib.ze_op_score_detail(self.h, _ptr(logits), rows, int(logits.shape[1]), int(logits.stride(0)), _ptr(targets),
                                                n, _ptr(lp), _ptr(ent), _ptr(rank), _ptr(ids), _ptr(tlp), self._stream()))
        return ScoreDetail(lp, ent, rank, ids, tlp, [0, rows])

    def _batch_args(self, seqs, ids_list, embeds_list, pos_list, deltas):
        """The arguments ze_prefill_batch and ze_score_batch share, from per-chain lists: (n, seqs, lens, ids, embeds, image rows,
        positions, deltas) as the C ABI takes them, and the arrays the pointers point into (alive while the caller holds them)."""
        sq, sp = _i32(seqs)
        lens, lp = _i32([len(x) for x in ids_list])
        ids, ip = _i32(np.concatenate([np.asarray(x, dtype=np.int32) for x in ids_list]))
        pos = np.concatenate([np.asarray(p, dtype=np.int32).reshape(3, -1) for p in pos_list], axis=1)
        pos, pp = _i32(np.ascontiguousarray(pos))
        embs = [x for x in embeds_list if x is not None and x.shape[0] > 0]
        nrows, nrp = _i32([0 if x is None else int(x.shape[0]) for x in embeds_list])
        emb = (torch.cat(embs) if len(embs) > 1 else embs[0]).contiguous() if embs else None
        if emb is not None:
            assert emb.dtype == torch.bfloat16
        dl, dp = _i32(deltas)
        self._use(emb, *embs)
        return (len(sq), sp, lp, ip, emb, nrp, pp, dp), (sq, lens, ids, pos, nrows, dl)

    def prefill_batch(self, seqs, ids_list, embeds_list, pos_list, deltas):
        """One prefill pass for several chains (rows of all chains share every GEMM).  Per chain i: ids_list[i] (new
        token ids), embeds_list[i] (bf16 [rows, hidden] or None), pos_list[i] (int32 [3, len]), deltas[i].  Each
        chain's result is bit-identical to prefill() of that chain alone."""
        (n, sp, lp, ip, emb, nrp, pp, dp), _alive = self._batch_args(seqs, ids_list, embeds_list, pos_list, deltas)
        self._check(self.lib.ze_prefill_batch(self.h, sp, n, lp, ip, _ptr(emb), nrp, pp, dp, self._stream()))

    def score_batch(self, seqs, ids_list, embeds_list, pos_list, deltas, score_from=None):
        """prefill_batch() plus, for chain i, the log-probability of the next id at its new positions score_from[i] ..
        len(ids_list[i]) - 2 (ze_score_batch; score_from None: every position, as score()).  Returns (f32 [sum of the chains'
        counts] on the device, packed in chain order; offsets: n + 1 ints, chain i's values are out[offsets[i]:offsets[i + 1]]).
        A chain's values are the bits score() of that chain alone gives at those positions."""
        (n, sp, lp, ip, emb, nrp, pp, dp), alive = self._batch_args(seqs, ids_list, embeds_list, pos_list, deltas)
        lens = alive[1]
        sf = np.zeros(n, dtype=np.int32) if score_from is None else np.asarray(score_from, dtype=np.int32).reshape(-1)
        if len(sf) != n:
            raise ValueError(f"score_from has {len(sf)} entries for {n} chains")
        sf, sfp = _i32(sf)
        # (an out-of-range value is the library's error; the buffer is sized without trusting it)
        counts = np.clip(lens.astype(np.int64) - 1 - np.clip(sf, 0, None), 0, None)
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        out = torch.empty(max(int(offsets[-1]), 1), dtype=torch.float32, device=self.device)
        self._check(self.lib.ze_score_batch(self.h, sp, n, lp, ip, _ptr(emb), nrp, pp, dp, sfp, _ptr(out), self._stream()))
        return out[:int(offsets[-1])], offsets.tolist()

    def score_batch_detail(self, seqs, ids_list, embeds_list, pos_list, deltas, score_from=None, top_n: int = 0,
                           entropy: bool = False, rank: bool = False) -> "ScoreDetail":
        """score_batch() with more per scored position (ze_score_batch_detail): `logps` as score_batch gives them, bit for bit, and,
        where asked, `entropy` (f32), `rank` of the next id (int32, 0 = the arg-max) and the `top_n` (<= MAX_TOP_LOGPROBS) best ids
        with their log-probabilities (`top_ids` int32 / `top_logprobs` f32, [count, top_n], (value descending, id ascending), places
        a row cannot fill (-1, -inf)).  All on the device, packed as `logps`; what was not asked for is None.  Nothing asked: the
        launches of score_batch."""
        (n, sp, lp, ip, emb, nrp, pp, dp), alive = self._batch_args(seqs, ids_list, embeds_list, pos_list, deltas)
        lens = alive[1]
        sf = np.zeros(n, dtype=np.int32) if score_from is None else np.asarray(score_from, dtype=np.int32).reshape(-1)
        if len(sf) != n:
            raise ValueError(f"score_from has {len(sf)} entries for {n} chains")
        sf, sfp = _i32(sf)
        counts = np.clip(lens.astype(np.int64) - 1 - np.clip(sf, 0, None), 0, None)
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        total, tn = int(offsets[-1]), int(top_n)
        want_top = 0 < tn <= MAX_TOP_LOGPROBS   # (a value outside the range is the library's error)

        def buf(dtype, *shape):
            return torch.empty((max(total, 1),) + shape, dtype=dtype, device=self.device)
        out = buf(torch.float32)
        ent = buf(torch.float32) if entropy else None
        rk = buf(torch.int32) if rank else None
        ids = buf(torch.int32, tn) if want_top else None
        tlp = buf(torch.float32, tn) if want_top else None
        self._check(self.lib.ze_score_batch_detail(self.h, sp, n, lp, ip, _ptr(emb), nrp, pp, dp, sfp, tn, _ptr(out), _ptr(ent), _ptr(rk),
                                                   _ptr(ids), _ptr(tlp), self._stream()))
        cut = lambda x: None if x is None else x[:total]
        return ScoreDetail(cut(out), cut(ent), cut(rk), cut(ids), cut(tlp), offsets.tolist())

    def decode_step(self, seq: int, token: int = -1, want_logits: bool = True):
        logits = torch.empty(self.config.text.vocab_size, dtype=torch.float32, device=self.device) if want_logits else None
        self._check(self.lib.ze_decode_step(self.h, seq, token, _ptr(logits), self._stream()))
        return logits

    @staticmethod
    def _gen_params(max_new_tokens, repetition_penalty, ignore_eos, use_graph, sync_every, do_sample, temperature, seed):
        if do_sample and not (temperature and temperature > 0):
            raise ValueError("`temperature` has to be a strictly positive float when sampling")  # as HF raises
        if os.environ.get("ZE_NO_GRAPH") == "1":  # debugging aid: every decode step launched eagerly
            use_graph = False
        return _lib.ZeGenParams(max_new_tokens, repetition_penalty, int(ignore_eos), int(use_graph), sync_every,
                                int(bool(do_sample)), float(temperature or 0.0), int(seed) & (2 ** 64 - 1))

    def generate(self, seq: int, max_new_tokens: int, repetition_penalty: float = 1.0, ignore_eos: bool = False,
                 use_graph: bool = True, sync_every: int = 16, do_sample: bool = False, temperature: float = 1.0,
                 seed: int = 0, top_k=None, top_p=None, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
        p = self._gen_params(max_new_tokens, repetition_penalty, ignore_eos, use_graph, sync_every, do_sample,
                             temperature, seed)
        self._apply_filter([seq], top_k, top_p, min_p)
        self._apply_entropy_filter([seq], typical_p, epsilon_cutoff, eta_cutoff)
        out = (C.c_int32 * max(max_new_tokens, 1))()
        n = C.c_int()
        self._check(self.lib.ze_generate(self.h, seq, C.byref(p), out, C.byref(n), self._stream()))
        return [int(out[i]) for i in range(n.value)]

    def set_speculation(self, seq: int, k: int, prompt_ids=(), ngram_min: int = 1, ngram_max: int = 3, sampled: bool = False):
        """Speculative decoding by prompt lookup for chain `seq` (ze_seq_set_speculation; HF's prompt_lookup_num_tokens, vLLM's
        ngram method): up to `k` draft ids per step, looked up in prompt_ids + the generated ids by the most recent earlier
        occurrence of the last ngram_max .. ngram_min ids, verified in the same family-0 step.  Lossless and greedy only; k = 0
        clears.  Set after the chain's prefill; held until the slot is reset, truncated or copied into.
        sampled=True (ze_seq_set_speculation_mode, mode 1): the chain may sample -- temperature, seed, penalty, top-k / top-p /
        min-p, its own or the call's; every row draws the token a plain step at its position draws, so the answer is still bit for
        bit the plain one."""
        ids, ip = _i32(list(prompt_ids) if k else [])
        if sampled:
            self._check(self.lib.ze_seq_set_speculation_mode(self.h, int(seq), int(k), int(ngram_min), int(ngram_max), ip, len(ids), 1,
                                                             self._stream()))
            return
        self._check(self.lib.ze_seq_set_speculation(self.h, int(seq), int(k), int(ngram_min), int(ngram_max), ip, len(ids), self._stream()))

    def generate_speculative(self, seqs, max_new_tokens: int, repetition_penalty: float = 1.0, ignore_eos: bool = False,
                             use_graph: bool = True, burst: int = 8, do_sample: bool = False, temperature: float = 1.0, seed: int = 0,
                             sample_streams=None):
        """Generation for prefilled chains through family-0 bursts (chain_begin + decode_burst), the path chains with
        set_speculation take: a step emits up to k + 1 tokens per speculating chain.  Returns one id list per chain, trimmed to
        max_new_tokens -- bit for bit what the same bursts give without speculation.  do_sample / temperature / seed: the call's
        sampling (chains that speculate then need set_speculation(sampled=True)); sample_streams: the random stream per chain
        (default: its position in `seqs`)."""
        seqs = [int(s) for s in seqs]
        p = self.gen_params(repetition_penalty=repetition_penalty, ignore_eos=ignore_eos, use_graph=use_graph, do_sample=do_sample,
                            temperature=temperature, seed=seed)
        for i, s in enumerate(seqs):
            self.chain_begin(s, p, i if sample_streams is None else int(sample_streams[i]))
        n_gen, fin, live = {s: 1 for s in seqs}, {s: False for s in seqs}, list(seqs)
        while live:
            live = [s for s in live if n_gen[s] < max_new_tokens and not fin[s] and self.seq_len(s) < self.max_ctx]
            if not live:
                break
            left = max_new_tokens - min(n_gen[s] for s in live)
            ran, ng, f = self.decode_burst(live, max(1, min(int(burst), left)), p)
            if ran <= 0 or all(a == n_gen[s] for a, s in zip(ng, live)):
                break
            for s, a, b in zip(live, ng, f):
                n_gen[s], fin[s] = a, b
        return [self.chain_tokens(s, max_new_tokens) for s in seqs]

    def spec_stats(self, seq: int):
        """(speculative steps, draft ids proposed, draft ids accepted) of chain `seq` since set_speculation."""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._check(self.lib.ze_chain_spec_stats(self.h, int(seq), C.byref(a), C.byref(b), C.byref(c), self._stream()))
        return a.value, b.value, c.value

    def op_spec_draft(self, histories, k: int, ngram_min: int = 1, ngram_max: int = 3):
        """The drafter alone (ze_op_spec_draft) on a list of id histories; returns one draft (list of ids) per history."""
        rows = len(histories)
        ld = max(1, max((len(h) for h in histories), default=1))
        hist = np.zeros((rows, ld), dtype=np.int32)
        for r, h in enumerate(histories):
            hist[r, :len(h)] = h
        hd = torch.from_numpy(hist).to(self.device)
        ln = torch.tensor([len(h) for h in histories], dtype=torch.int32, device=self.device)
        out = torch.empty((rows, int(k)), dtype=torch.int32, device=self.device)
        on = torch.empty(rows, dtype=torch.int32, device=self.device)
        self._check(self.lib.ze_op_spec_draft(self.h, _ptr(hd), _ptr(ln), rows, ld, int(k), int(ngram_min), int(ngram_max), _ptr(out), _ptr(on),
                                              self._stream()))
        o, n = out.cpu().numpy(), on.cpu().numpy()
        return [[int(t) for t in o[r, :n[r]]] for r in range(rows)]

    def op_spec_accept(self, logits: torch.Tensor, drafts, k: int, seen: Optional[torch.Tensor] = None, repetition_penalty=1.0, room=None,
                       ignore_eos: bool = False):
        """The accept pass alone (ze_op_spec_accept): logits f32 [n * (k + 1), vocab] device, drafts a list of n id lists (<= k each),
        seen uint8 [n, vocab] device (updated in place) or None.  Returns (emitted ids per chain, finished flags)."""
        n, k = len(drafts), int(k)
        assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.shape[0] == n * (k + 1)
        d = np.full((n, k), -1, dtype=np.int32)
        for c, dr in enumerate(drafts):
            d[c, :len(dr)] = dr
        dd = torch.from_numpy(d).to(self.device)
        dl = torch.tensor([len(dr) for dr in drafts], dtype=torch.int32, device=self.device)
        pen = torch.tensor(np.broadcast_to(np.asarray(repetition_penalty, dtype=np.float32), (n,)).copy(), device=self.device)
        rm = torch.tensor(np.broadcast_to(np.asarray(k + 1 if room is None else room, dtype=np.int32), (n,)).copy(), device=self.device)
        out = torch.empty((n, k + 1), dtype=torch.int32, device=self.device)
        cnt = torch.empty(n, dtype=torch.int32, device=self.device)
        fin = torch.empty(n, dtype=torch.int32, device=self.device)
        self._check(self.lib.ze_op_spec_accept(self.h, _ptr(logits), n, int(logits.shape[1]), int(logits.stride(0)), k, _ptr(dd), _ptr(dl),
                                               _ptr(seen), _ptr(pen), _ptr(rm), int(bool(ignore_eos)), _ptr(out), _ptr(cnt), _ptr(fin),
                                               self._stream()))
        o, m, f = out.cpu().numpy(), cnt.cpu().numpy(), fin.cpu().numpy()
        return [[int(t) for t in o[c, :m[c]]] for c in range(n)], [bool(x) for x in f]

    def op_spec_accept_sampled(self, logits: torch.Tensor, drafts, k: int, temperature, seed=0, sample_stream=0, index0=0,
                               seen: Optional[torch.Tensor] = None, repetition_penalty=1.0, room=None, ignore_eos: bool = False,
                               top_k=None, top_p=None, min_p=None):
        """The accept pass of the sampled mode alone (ze_op_spec_accept_sampled): op_spec_accept's arguments (logits f32
        [n * (k + 1), vocab], row stride >= vocab) plus, per chain (scalars broadcast), temperature (0 = greedy), seed,
        sample_stream, index0 (the draw index of row 0) and top_k / top_p / min_p (or all None).  Returns (emitted ids per chain,
        finished flags); seen is updated in place."""
        n, k = len(drafts), int(k)
        assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 and logits.shape[0] == n * (k + 1)
        vocab = int(logits.shape[1])
        if seen is not None:
            assert seen.dtype == torch.uint8 and seen.is_contiguous() and tuple(seen.shape) == (n, vocab)
        d = np.full((n, k), -1, dtype=np.int32)
        for c, dr in enumerate(drafts):
            d[c, :len(dr)] = dr
        dd = torch.from_numpy(d).to(self.device)
        dl = torch.tensor([len(dr) for dr in drafts], dtype=torch.int32, device=self.device)

        def per_chain(v, dtype):
            return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (n,)))
        pen = torch.tensor(per_chain(repetition_penalty, np.float32).copy(), device=self.device)
        rm = torch.tensor(per_chain(k + 1 if room is None else room, np.int32).copy(), device=self.device)
        t, sd = per_chain(temperature, np.float32), per_chain(seed, np.uint64)
        strm, idx = per_chain(sample_stream, np.int32), per_chain(index0, np.int32)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        filt = (None, None, None)
        if top_k is not None or top_p is not None or min_p is not None:
            filt = (per_chain(0 if top_k is None else top_k, np.int32), per_chain(1.0 if top_p is None else top_p, np.float32),
                    per_chain(0.0 if min_p is None else min_p, np.float32))
        out = torch.empty((n, k + 1), dtype=torch.int32, device=self.device)
        cnt = torch.empty(n, dtype=torch.int32, device=self.device)
        fin = torch.empty(n, dtype=torch.int32, device=self.device)
        self._use(logits)
        self._check(self.lib.ze_op_spec_accept_sampled(
            self.h, _ptr(logits), n, vocab, int(logits.stride(0)), k, _ptr(dd), _ptr(dl), _ptr(seen) if seen is not None else None,
            _ptr(pen), _ptr(rm), int(bool(ignore_eos)), t.ctypes.data_as(fp), sd.ctypes.data_as(C.POINTER(C.c_uint64)),
            strm.ctypes.data_as(ip), idx.ctypes.data_as(ip), filt[0].ctypes.data_as(ip) if filt[0] is not None else None,
            filt[1].ctypes.data_as(fp) if filt[1] is not None else None, filt[2].ctypes.data_as(fp) if filt[2] is not None else None,
            _ptr(out), _ptr(cnt), _ptr(fin), self._stream()))
        o, m, f = out.cpu().numpy(), cnt.cpu().numpy(), fin.cpu().numpy()
        return [[int(t) for t in o[c, :m[c]]] for c in range(n)], [bool(x) for x in f]

    def decode_rows(self, seq: int, tokens):
        """Chain `seq` fed `tokens` at consecutive positions in one family-0 step (ze_op_decode_rows); logits f32 [len, vocab]."""
        tk, tp = _i32(tokens)
        logits = torch.empty((len(tk), self.config.text.vocab_size), dtype=torch.float32, device=self.device)
        self._check(self.lib.ze_op_decode_rows(self.h, int(seq), tp, len(tk), _ptr(logits), self._stream()))
        return logits

    def set_decode_regime(self, regime: int = -1) -> int:
        """Kernel family of the batched decode step: 0 fragment kernels (<= 64 chains per step), 1 row streaming (any
        count), -1 by capacity (max_seqs > 64 -> 1).  Returns the family in force."""
        return self._check(self.lib.ze_set_decode_regime(self.h, int(regime)))

    def decode_batch(self, seqs, tokens=None, want_logits: bool = True):
        sq, sp = _i32(seqs)
        tk, tp = _i32(tokens) if tokens is not None else (None, None)
        logits = torch.empty((len(sq), self.config.text.vocab_size), dtype=torch.float32, device=self.device) if want_logits else None
        self._check(self.lib.ze_decode_batch(self.h, sp, len(sq), tp, _ptr(logits), self._stream()))
        return logits

    def generate_batch(self, seqs, max_new_tokens: int, repetition_penalty: float = 1.0, ignore_eos: bool = False,
                       sync_every: int = 16, use_graph: bool = True, do_sample: bool = False, temperature: float = 1.0,
                       seed: int = 0, top_k=None, top_p=None, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
        """Generation for several prefilled chains at once; returns one token list per chain.  top_k / top_p / min_p, when
        given, are set on every chain of the call (set_sampling_filter beforehand for a filter per chain)."""
        sq, sp = _i32(seqs)
        self._apply_filter(sq, top_k, top_p, min_p)
        self._apply_entropy_filter(sq, typical_p, epsilon_cutoff, eta_cutoff)
        p = self._gen_params(max_new_tokens, repetition_penalty, ignore_eos, use_graph, sync_every, do_sample,
                             temperature, seed)
        out = (C.c_int32 * (len(sq) * max_new_tokens))()
        n_out = (C.c_int32 * len(sq))()
        self._check(self.lib.ze_generate_batch(self.h, sp, len(sq), C.byref(p), out, n_out, self._stream()))
        return [[int(out[i * max_new_tokens + t]) for t in range(n_out[i])] for i in range(len(sq))]

    # ------------------------------------------------------------------ continuous batching
    def chain_begin(self, seq: int, params, sample_stream: int = 0):
        """First token of a prefilled chain (from the logits its prefill left); `params` from gen_params()."""
        self._check(self.lib.ze_chain_begin(self.h, seq, C.byref(params), int(sample_stream), self._stream()))

    def gen_params(self, repetition_penalty: float = 1.0, ignore_eos: bool = False, use_graph: bool = True,
                   do_sample: bool = False, temperature: float = 1.0, seed: int = 0):
        return self._gen_params(0, repetition_penalty, ignore_eos, use_graph, 1, do_sample, temperature, seed)

    def decode_burst(self, seqs, steps: int, params):
        """`steps` sampled decode steps for the live chains `seqs`; returns (steps run, n_generated[], finished[])."""
        sq, sp = _i32(seqs)
        ng = (C.c_int32 * len(sq))()
        fin = (C.c_int32 * len(sq))()
        ran = self._check(self.lib.ze_decode_burst(self.h, sp, len(sq), int(steps), C.byref(params), ng, fin,
                                                   self._stream()))
        return ran, list(ng), [bool(f) for f in fin]

    def decode_burst_begin(self, seqs, steps: int, params):
        """First half of decode_burst: enqueues the steps on the current stream and returns at once (steps enqueued).  The
        caller may now enqueue a ViT / prefill round for OTHER chains on another stream; decode_burst_end collects."""
        sq, sp = _i32(seqs)
        return self._check(self.lib.ze_decode_burst_begin(self.h, sp, len(sq), int(steps), C.byref(params), self._stream()))

    def decode_burst_end(self, seqs):
        """Waits for the burst begun on the current stream; returns (n_generated[], finished[])."""
        sq, sp = _i32(seqs)
        ng = (C.c_int32 * len(sq))()
        fin = (C.c_int32 * len(sq))()
        self._check(self.lib.ze_decode_burst_end(self.h, sp, len(sq), ng, fin, self._stream()))
        return list(ng), [bool(f) for f in fin]

    def chain_tokens(self, seq: int, capacity: int = 0, stream=None):
        """The tokens chain `seq` has generated.  `stream`: the stream its decode steps ran on (default: the current one) --
        the call copies on it and waits for it, so a scheduler inside its admission stream's context names the decode stream
        (waiting for the admission stream would serialise the next burst behind the prefill pass in flight)."""
        cap = int(capacity) if capacity else self.max_ctx
        out = (C.c_int32 * max(cap, 1))()
        n = C.c_int()
        st = C.c_void_p(stream.cuda_stream) if stream is not None else self._stream()
        self._check(self.lib.ze_chain_tokens(self.h, seq, out, cap, C.byref(n), st))
        return [int(out[i]) for i in range(n.value)]

    def chain_tokens_batch(self, seqs, capacity: int = 0, stream=None):
        """chain_tokens for several chains in one device -> host copy and one wait; returns a list of id lists."""
        if not len(seqs):
            return []
        cap = max(1, min(int(capacity) if capacity else self.max_ctx, self.max_ctx))
        sq, sp = _i32(seqs)
        out = np.empty((len(sq), cap), dtype=np.int32)
        n = (C.c_int32 * len(sq))()
        st = C.c_void_p(stream.cuda_stream) if stream is not None else self._stream()
        self._check(self.lib.ze_chain_tokens_batch(self.h, sp, len(sq), out.ctypes.data_as(C.POINTER(C.c_int32)), cap, n, st))
        return [out[i, :n[i]].tolist() for i in range(len(sq))]

    def tile_upload(self, host_rgb) -> torch.Tensor:
        """Decoded RGB u8 [H, W, 3] host array / tensor (ideally pinned) -> device tensor (ze_tile_upload)."""
        t = host_rgb if isinstance(host_rgb, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(host_rgb, dtype=np.uint8))
        assert t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3 and t.is_contiguous()
        out = torch.empty(t.shape, dtype=torch.uint8, device=self.device)
        self._check(self.lib.ze_tile_upload(self.h, C.c_void_p(t.data_ptr()), int(t.shape[0]), int(t.shape[1]), _ptr(out),
                                            self._stream()))
        out._ze_host_keepalive = t  # the async copy reads the host buffer until the stream reaches it
        return out

    def tile_upload_tiff(self, plan, host_bytes: torch.Tensor):
        """ze_tile_upload_tiff: the compressed chunks of `plan` (zoomearth_amd.image.TiffPlan), read into the flat u8 tensor host_bytes
        (pinned for an asynchronous copy), go to the device and are decoded there on the current stream.  Returns (tile u8 [H, W, 3],
        status i32 [n_chunks]), both device tensors: the tile is valid when every status word is 0, which the caller checks where it
        waits for the upload."""
        assert host_bytes.dtype == torch.uint8 and host_bytes.is_contiguous() and host_bytes.numel() >= plan.n_bytes and not host_bytes.is_cuda
        table = np.ascontiguousarray(plan.table, dtype=np.int32)
        out = torch.empty((plan.height, plan.width, 3), dtype=torch.uint8, device=self.device)
        status = torch.empty(plan.n_chunks, dtype=torch.int32, device=self.device)
        self._check(self.lib.ze_tile_upload_tiff(self.h, C.c_void_p(host_bytes.data_ptr()), plan.n_bytes, C.c_void_p(table.ctypes.data),
                                                 plan.n_chunks, plan.height, plan.width, plan.compression, plan.predictor, int(plan.tiled),
                                                 plan.chunk_w, plan.chunk_h, _ptr(out), _ptr(status), self._stream()))
        out._ze_host_keepalive = host_bytes  # the async copy reads the host buffer until the stream reaches it
        return out, status

    def upload_tiff(self, path_or_plan) -> torch.Tensor:
        """`Image.open(path).convert("RGB")` on the device for an LZW / PackBits RGB TIFF: its compressed chunks are read into pinned memory
        and decoded by the engine.  Takes a path or a TiffPlan; returns the u8 [H, W, 3] device tensor.  ValueError for a file without a plan
        (zoomearth_amd.image.tiff_plan says which files have one), TiffChunkError when a chunk is defective -- decode_rgb is the way then."""
        from .image import TiffChunkError, TiffPlan, tiff_plan
        plan = path_or_plan if isinstance(path_or_plan, TiffPlan) else tiff_plan(path_or_plan)
        if plan is None:
            raise ValueError(f"{path_or_plan}: not a TIFF the device decodes (see zoomearth_amd.image.tiff_plan)")
        buf = torch.empty(plan.n_bytes, dtype=torch.uint8).pin_memory()
        if not plan.read_into(buf.numpy()):
            raise TiffChunkError(f"{plan.path}: a chunk is old-style (pre-6.0) LZW, which the device does not decode")
        out, status = self.tile_upload_tiff(plan, buf)
        st = status.cpu().numpy()
        if st.any():
            i = int(np.flatnonzero(st)[0])
            raise TiffChunkError(f"{plan.path}: chunk {i} is defective (status {int(st[i])})")
        return out

    def tiff_decode(self, dev_bytes: torch.Tensor, dev_table: torch.Tensor, h: int, w: int, compression: int, predictor: int, tiled: bool,
                    chunk_w: int, chunk_h: int, out: torch.Tensor, status: torch.Tensor) -> None:
        """ze_op_tiff_decode: the decode kernels alone on device operands -- dev_bytes u8 (16-byte aligned, a multiple of 16 long), dev_table
        i32 [n_chunks, 8], out u8 [h, w, 3] (or a larger buffer that starts with it), status i32 [n_chunks]."""
        assert dev_bytes.dtype == torch.uint8 and dev_table.dtype == torch.int32 and status.dtype == torch.int32 and out.dtype == torch.uint8
        assert dev_bytes.is_cuda and dev_table.is_cuda and out.is_cuda and status.is_cuda and dev_table.is_contiguous() and out.is_contiguous()
        n = int(dev_table.shape[0])
        assert status.numel() >= n and out.numel() >= h * w * 3
        self._use(dev_bytes), self._use(dev_table)
        self._check(self.lib.ze_op_tiff_decode(self.h, _ptr(dev_bytes), int(dev_bytes.numel()), _ptr(dev_table), n, int(h), int(w), int(compression),
                                               int(predictor), int(bool(tiled)), int(chunk_w), int(chunk_h), _ptr(out), _ptr(status), self._stream()))

    def sample_greedy(self, seq: int, logits: torch.Tensor, repetition_penalty: float = 1.0) -> int:
        tok = C.c_int32()
        self._check(self.lib.ze_op_sample_greedy(self.h, seq, _ptr(logits), repetition_penalty, C.byref(tok),
                                                 self._stream()))
        return int(tok.value)

    def sample_temperature(self, seq: int, logits: torch.Tensor, temperature: float, seed: int, index: int = 0,
                           repetition_penalty: float = 1.0) -> int:
        tok = C.c_int32()
        self._check(self.lib.ze_op_sample_temperature(self.h, seq, _ptr(logits), repetition_penalty, temperature,
                                                      int(seed) & (2 ** 64 - 1), index, C.byref(tok), self._stream()))
        return int(tok.value)

    def quantize_fp8(self):
        """Switch the decoder's linear layers to FP8 (E4M3, per-row power-of-two scales): see ze_weights_quantize_fp8."""
        self._check(self.lib.ze_weights_quantize_fp8(self.h, self._stream()))

    def quantize_mxfp4(self):
        """Switch the decoder's linear layers to MXFP4 (E2M1 codes, one E8M0 scale per 32 weights; reduced precision, opt-in): the
        batch-1 decode reads the 4-bit stream, the 2 .. 64-chain step of decode family 0 the 4-bit fragment copies (bit-identical to the
        dequantised form), every other path the dequantised bf16 values.  See ze_weights_quantize_mxfp4."""
        self._check(self.lib.ze_weights_quantize_mxfp4(self.h, self._stream()))

    WEIGHT_FORMATS = ("bf16", "fp8", "mxfp4")

    @property
    def weight_format(self) -> str:
        """The weight stream the batch-1 decode reads now: "bf16", "fp8" or "mxfp4" (the engine's state: a weight write or an
        adapter switch returns it to "bf16")."""
        return self.WEIGHT_FORMATS[self._check(self.lib.ze_weight_format(self.h))]

    def fragment_bytes(self) -> int:
        """Device bytes the fragment-major weight copies of the 2 .. 64-chain decode step hold now (ze_fragment_bytes): 0 before the
        first batched step; on an MXFP4 engine the 4-bit copies, 4.25 bits per quantised weight."""
        b = C.c_size_t()
        self._check(self.lib.ze_fragment_bytes(self.h, C.byref(b)))
        return int(b.value)

    def set_weight_format(self, fmt) -> None:
        """Quantise the loaded weights to `fmt` ("fp8" / "mxfp4"; None or "bf16": leave them).  The formats exclude each other."""
        if fmt in (None, "bf16"):
            return
        if fmt not in self.WEIGHT_FORMATS:
            raise ValueError(f"weight_format {fmt!r}: one of {self.WEIGHT_FORMATS}")
        self.quantize_fp8() if fmt == "fp8" else self.quantize_mxfp4()

    def set_fp8_activations(self, on: bool = True):
        """FP8 x FP8 batched decode (qkv and gate/up inputs quantised per row): see ze_set_fp8_activations.  Needs
        quantize_fp8() first; a weight change switches it off again."""
        self._check(self.lib.ze_set_fp8_activations(self.h, 1 if on else 0))

    def op_linear_mx(self, a8: torch.Tensor, sa: torch.Tensor, w8: torch.Tensor, sw: torch.Tensor, bias=None, swiglu: bool = False):
        """(a8 * sa[:, None]) @ (w8 * sw[:, None]).T on the block-scaled FP8 MFMA: a8 u8 [M, K], w8 u8 [N, K] (E4M3 bytes),
        sa / sw f32 powers of two per row (what op_quantize_fp8 returns) -> bf16 [M, N] ([M, N / 2] with swiglu)."""
        m, k = a8.shape
        n = w8.shape[0]
        out = torch.empty((m, n // 2 if swiglu else n), dtype=torch.bfloat16, device=self.device)
        self._check(self.lib.ze_op_linear_mx(self.h, _ptr(a8), _ptr(sa), _ptr(w8), _ptr(sw), _ptr(bias), _ptr(out), m, n, k,
                                             1 if swiglu else 0, self._stream()))
        return out

    def op_quantize_fp8(self, w: torch.Tensor):
        """w bf16 [rows, cols] on the device (overwritten with the dequantised values) -> (u8 bits, f32 scales)."""
        rows, cols = w.shape
        q = torch.empty((rows, cols), dtype=torch.uint8, device=self.device)
        sc = torch.empty(rows, dtype=torch.float32, device=self.device)
        self._check(self.lib.ze_op_quantize_fp8(self.h, _ptr(w), rows, cols, _ptr(q), _ptr(sc), self._stream()))
        return q, sc

    def op_quantize_mxfp4(self, w: torch.Tensor):
        """w bf16 [rows, cols] on the device (overwritten with the dequantised values) -> (u8 codes [rows, cols / 2], low nibble =
        even k; u8 E8M0 scales [rows, cols / 32]).  cols % 32 == 0."""
        rows, cols = w.shape
        q = torch.empty((rows, cols // 2), dtype=torch.uint8, device=self.device)
        sc = torch.empty((rows, cols // 32), dtype=torch.uint8, device=self.device)
        self._check(self.lib.ze_op_quantize_mxfp4(self.h, _ptr(w), rows, cols, _ptr(q), _ptr(sc), self._stream()))
        return q, sc

    # ------------------------------------------------------------------ unit ops (parity tests)
    def op_window_gather(self, pixel_values: torch.Tensor, grids) -> torch.Tensor:
        g, gp = _i32(np.asarray(grids).reshape(-1, 3))
        out = torch.empty(pixel_values.shape, dtype=torch.bfloat16, device=self.device)
        self._check(self.lib.ze_op_window_gather(self.h, _ptr(pixel_values), gp, len(g), _ptr(out), self._stream()))
        return out

    def op_window_scatter(self, x: torch.Tensor, grids) -> torch.Tensor:
        g, gp = _i32(np.asarray(grids).reshape(-1, 3))
        out = torch.empty_like(x)
        self._check(self.lib.ze_op_window_scatter(self.h, _ptr(x), x.shape[1], gp, len(g), _ptr(out), self._stream()))
        return out

    def op_vision_rope(self, qkv: torch.Tensor, grids, window_order: bool = True) -> torch.Tensor:
        """In place on qkv bf16 [n, 3 * heads * 80]; returns it."""
        g, gp = _i32(np.asarray(grids).reshape(-1, 3))
        self._check(self.lib.ze_op_vision_rope(self.h, _ptr(qkv), gp, len(g), int(window_order), self._stream()))
        return qkv

    def op_embed_scatter(self, input_ids, image_embeds=None) -> torch.Tensor:
        ids, ip = _i32(input_ids)
        out = torch.empty((len(ids), self.config.text.hidden_size), dtype=torch.bfloat16, device=self.device)
        n_img = 0 if image_embeds is None else int(image_embeds.shape[0])
        self._check(self.lib.ze_op_embed_scatter(self.h, ip, len(ids), _ptr(image_embeds), n_img, _ptr(out), self._stream()))
        return out

    def op_mrope_kv(self, seq: int, layer: int, qkv: torch.Tensor, position_ids, past: int) -> torch.Tensor:
        """In place on qkv bf16 [T, (heads + 2 kv_heads) * 128] (q roped); K / V rows appended to the cache at `past`."""
        pos, pp = _i32(position_ids)
        assert pos.shape == (3, qkv.shape[0])
        self._check(self.lib.ze_op_mrope_kv(self.h, seq, layer, _ptr(qkv), qkv.shape[0], pp, int(past), self._stream()))
        return qkv

    def op_rope_kv_decode(self, seqs, layer: int, qkv: torch.Tensor) -> torch.Tensor:
        sq, sp = _i32(seqs)
        assert qkv.shape[0] == len(sq)
        self._check(self.lib.ze_op_rope_kv_decode(self.h, sp, len(sq), layer, _ptr(qkv), self._stream()))
        return qkv

    def op_attn_decode(self, seqs, layer: int, qkv: torch.Tensor) -> torch.Tensor:
        """the attention of one batched decode step, alone: qkv as op_rope_kv_decode left it -> [n, heads x 128]"""
        sq, sp = _i32(seqs)
        t = self.config.text
        assert qkv.shape[0] == len(sq) and qkv.dtype == torch.bfloat16 and qkv.is_contiguous()
        out = torch.empty((len(sq), t.hidden_size), dtype=torch.bfloat16, device=self.device)
        self._check(self.lib.ze_op_attn_decode(self.h, sp, len(sq), layer, _ptr(qkv), _ptr(out), self._stream()))
        return out

    def op_attn_decode_single(self, seq: int, layer: int, qkv: torch.Tensor) -> torch.Tensor:
        """the attention of the single-chain decode step, alone: one chain's qkv row [(heads + 2 kv_heads) x 128] -> [heads x 128]"""
        t = self.config.text
        assert qkv.dtype == torch.bfloat16 and qkv.is_contiguous() and qkv.numel() == (t.num_attention_heads + 2 * t.num_key_value_heads) * 128
        out = torch.empty((t.hidden_size,), dtype=torch.bfloat16, device=self.device)
        self._check(self.lib.ze_op_attn_decode_single(self.h, int(seq), int(layer), _ptr(qkv), _ptr(out), self._stream()))
        return out

    def op_kv_read(self, seq: int, layer: int, start: int, n: int):
        t = self.config.text
        shape = (t.num_key_value_heads, n, t.hidden_size // t.num_attention_heads)
        k = torch.empty(shape, dtype=torch.bfloat16, device=self.device)
        v = torch.empty(shape, dtype=torch.bfloat16, device=self.device)
        self._check(self.lib.ze_op_kv_read(self.h, seq, layer, start, n, _ptr(k), _ptr(v), self._stream()))
        return k, v

    GV_QKV_ROPE, GV_RESIDUAL, GV_SWIGLU, GV_LOGITS, GV_PLAIN = 0, 1, 2, 3, 4   # epilogues of op_gemv

    def op_gemv(self, epi: int, x, w=None, w8=None, scale8=None, norm_w=None, eps: float = 1e-6, bias=None, act8: bool = False, out=None,
                argmax: bool = False, seen=None, penalty: float = 1.0, seq: int = 0, layer: int = 0, embed=None, token: int = -1,
                embed_out=None):
        """One launch of the single-chain decode GEMV family (ze_op_gemv): w bf16 [N, K] or (w8 u8 [N, K], scale8 f32 [N]); x bf16
        [K] (or row `token` of embed [V, K], copied to embed_out [K]).  `out` (allocated when None; RESIDUAL: the hidden row, updated
        in place): bf16 [N] (PLAIN, RESIDUAL), bf16 [N / 2] (SWIGLU), f32 [N] (LOGITS), bf16 [heads x 128] (QKV_ROPE: k / v go to row
        ctx of `layer`'s cache of chain `seq`).  Returns out, or (out, token) with argmax (LOGITS: the folded greedy arg-max, `seen`
        u8 [N] and `penalty` as the sampler's)."""
        mat = w8 if w8 is not None else w
        n, k = mat.shape
        if out is None:
            t = self.config.text
            shape, dt = {self.GV_SWIGLU: (n // 2, torch.bfloat16), self.GV_LOGITS: (n, torch.float32),
                         self.GV_QKV_ROPE: (t.hidden_size, torch.bfloat16)}.get(epi, (n, torch.bfloat16))
            out = torch.empty(shape, dtype=dt, device=self.device)
        tok = C.c_int32(-1)
        f32 = epi == self.GV_LOGITS
        self._check(self.lib.ze_op_gemv(self.h, epi, _ptr(w), _ptr(w8), _ptr(scale8), _ptr(x), _ptr(norm_w), eps, _ptr(bias), int(act8),
                                        n, k, None if f32 else _ptr(out), _ptr(out) if f32 else None, _ptr(seen), penalty,
                                        C.byref(tok) if argmax else None, seq, layer, _ptr(embed), int(token), _ptr(embed_out),
                                        self._stream()))
        return (out, int(tok.value)) if argmax else out

    def op_gemv4(self, epi: int, x, q4, scale4, norm_w=None, eps: float = 1e-6, bias=None, out=None, argmax: bool = False, seen=None,
                 penalty: float = 1.0, seq: int = 0, layer: int = 0, embed=None, token: int = -1, embed_out=None):
        """op_gemv with the MXFP4 stream as W (ze_op_gemv4): q4 u8 [N, K / 2], scale4 u8 [N, K / 32] as op_quantize_mxfp4 returns."""
        n, k = q4.shape[0], q4.shape[1] * 2
        if out is None:
            t = self.config.text
            shape, dt = {self.GV_SWIGLU: (n // 2, torch.bfloat16), self.GV_LOGITS: (n, torch.float32),
                         self.GV_QKV_ROPE: (t.hidden_size, torch.bfloat16)}.get(epi, (n, torch.bfloat16))
            out = torch.empty(shape, dtype=dt, device=self.device)
        tok = C.c_int32(-1)
        f32 = epi == self.GV_LOGITS
        self._check(self.lib.ze_op_gemv4(self.h, epi, _ptr(q4), _ptr(scale4), _ptr(x), _ptr(norm_w), eps, _ptr(bias), n, k,
                                         None if f32 else _ptr(out), _ptr(out) if f32 else None, _ptr(seen), penalty,
                                         C.byref(tok) if argmax else None, seq, layer, _ptr(embed), int(token), _ptr(embed_out),
                                         self._stream()))
        return (out, int(tok.value)) if argmax else out

    def op_logits_rows(self, x: torch.Tensor, w: torch.Tensor, norm_w: torch.Tensor, eps: float = 1e-6, out=None) -> torch.Tensor:
        """fp32 logits [n, N] of n hidden rows x bf16 [n, K] through the prefill paths' lm_head pass (ze_op_logits_rows)."""
        rows, k = x.shape
        n = w.shape[0]
        if out is None:
            out = torch.empty((rows, n), dtype=torch.float32, device=self.device)
        self._check(self.lib.ze_op_logits_rows(self.h, _ptr(w), _ptr(norm_w), eps, _ptr(x), _ptr(out), rows, n, k, self._stream()))
        return out

    def op_numeric_helpers(self, x: torch.Tensor, y: torch.Tensor):
        """(bf16(x) | bf16(bf16(silu(x)) * y) << 16, pack_bf16x2(x, y)) as two int32 tensors (u32 bit patterns): x, y f32 on the device."""
        n = x.numel()
        out = torch.empty(n, dtype=torch.int32, device=self.device)
        out2 = torch.empty(n, dtype=torch.int32, device=self.device)
        self._check(self.lib.ze_op_numeric_helpers(self.h, _ptr(x), _ptr(y), _ptr(out), _ptr(out2), n, self._stream()))
        return out, out2

    def op_linear(self, a, w, bias=None, act: int = 0):
        m, k = a.shape
        n = w.shape[0]
        if act == 10:  # fp32 logits of the row-streaming regime's lm_head
            out = torch.empty((m, n), dtype=torch.float32, device=self.device)
            self._check(self.lib.ze_op_linear(self.h, _ptr(a), _ptr(w), None, _ptr(out), m, n, k, act, self._stream()))
            return out
        out = torch.empty((m, n // 2 if act in (4, 7, 9) else n), dtype=torch.bfloat16, device=self.device)
        self._check(self.lib.ze_op_linear(self.h, _ptr(a), _ptr(w), _ptr(bias), _ptr(out), m, n, k, act, self._stream()))
        return out

    def op_gemm(self, launcher: int, epi: int, a, lda: int, w, ldw: int, bias, r, ldr: int, c, ldc: int, c_rows, m: int, n: int,
                k: int) -> int:
        """ze_op_gemm on device tensors the caller allocated (padding and sentinels are the caller's): c is written in place.
        Returns the status code without raising, so that a test can see ZE_ERR_INVALID (-1)."""
        return int(self.lib.ze_op_gemm(self.h, launcher, epi, _ptr(a), lda, _ptr(w), ldw, _ptr(bias), _ptr(r), ldr, _ptr(c), ldc,
                                       _ptr(c_rows), m, n, k, self._stream()))

    def op_gemm4(self, launcher: int, epi: int, a, lda: int, q4, scale4, bias, r, ldr: int, c, ldc: int, m: int, n: int, k: int) -> int:
        """ze_op_gemm4: op_gemm's fragment launchers (5 skinny, 6 one-shot) with the MXFP4 stream as W -- q4 u8 [N, K / 2], scale4 u8
        [N, K / 32] as op_quantize_mxfp4 returns them.  Returns the status code without raising (ZE_ERR_INVALID is -1)."""
        return int(self.lib.ze_op_gemm4(self.h, launcher, epi, _ptr(a), lda, _ptr(q4), _ptr(scale4), _ptr(bias), _ptr(r), ldr, _ptr(c), ldc,
                                        m, n, k, self._stream()))

    def op_rmsnorm(self, x, w, eps: float):
        out = torch.empty_like(x)
        self._check(self.lib.ze_op_rmsnorm(self.h, _ptr(x), _ptr(w), _ptr(out), x.shape[0], x.shape[1], eps,
                                           self._stream()))
        return out

    def op_attention(self, q, k, v, cu_seqlens, causal: bool):
        t, heads, d = q.shape
        kvh = k.shape[1]
        out = torch.empty_like(q)
        cu, cp = _i32(cu_seqlens)
        self._check(self.lib.ze_op_attention(self.h, _ptr(q), _ptr(k), _ptr(v), _ptr(out), t, heads, kvh, d, cp,
                                             len(cu) - 1, int(causal), self._stream()))
        return out

    # ------------------------------------------------------------------ measurement
    def profile_decode_kernel(self, which: int, iters: int = 72):
        us, by = C.c_float(), C.c_double()
        self._check(self.lib.ze_profile_decode_kernel(self.h, which, iters, C.byref(us), C.byref(by), self._stream()))
        return float(us.value), float(by.value)

    def profile_batch_kernel(self, which: int, n: int, iters: int = 72):
        us, by = C.c_float(), C.c_double()
        self._check(self.lib.ze_profile_batch_kernel(self.h, which, n, iters, C.byref(us), C.byref(by), self._stream()))
        return float(us.value), float(by.value)

    def profile_prefill_kernel(self, which: int, rows: int, iters: int = 12):
        """(avg us, FLOP) of one projection of a prefill pass (0 qkv, 1 o, 2 gate/up, 3 down) at `rows` rows, on the operands the
        last pass left in the workspace and the layers' own weights."""
        us, fl = C.c_float(), C.c_double()
        self._check(self.lib.ze_profile_prefill_kernel(self.h, which, rows, iters, C.byref(us), C.byref(fl), self._stream()))
        return float(us.value), float(fl.value)

    def profile_prefill_layer(self, rows: int, layers_run: int = 36):
        """{projection: (avg us, FLOP)} of a prefill layer's four projections issued in pass order at `rows` rows."""
        us, fl = (C.c_float * 4)(), (C.c_double * 4)()
        self._check(self.lib.ze_profile_prefill_layer(self.h, rows, layers_run, us, fl, self._stream()))
        return {k: (float(us[i]), float(fl[i])) for i, k in enumerate(("qkv", "o", "gate_up", "down"))}

    def phase_timers(self, enable: bool = True, reset: bool = False):
        out = (C.c_float * 5)()
        self._check(self.lib.ze_phase_timers(self.h, int(enable), int(reset), out))
        return dict(zip(("frontend", "vit", "prefill", "decode", "sample"), [float(x) for x in out]))

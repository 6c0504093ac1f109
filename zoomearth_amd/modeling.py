"""ZoomEarthForConditionalGeneration: the `Qwen2_5_VLForConditionalGeneration` call surface used by the
reference entry points, on top of the HIP engine.

replaces: `Qwen2_5_VLForConditionalGeneration.from_pretrained(model_name, torch_dtype=torch.float16)`, `.eval()`,
`.device`, `.generation_config.{temperature,top_p,top_k}` and
`model.generate(**inputs, max_new_tokens=1024, do_sample=..., num_beams=1[, temperature])`
(/root/reference/src/eval/infer.py:109-115,147-151,160-162; src/demo.py:14-19,128).

Documented deviations: arithmetic is bf16 (the reference runs fp16 weights under a bf16 autocast
wrapper); `do_sample=True, temperature=T` draws from softmax(logits / T) with the engine's counter-based
random stream (`seed=` kwarg or `generation_config.seed`); `top_k` / `top_p` / `min_p` (kwargs, then
`generation_config`) are HF's warpers in HF's order, applied per chain on the device (`Engine.set_sampling_filter`;
None, `top_k=0`, `top_p=1.0` mean off, `top_k=1` is greedy, out-of-range values raise ValueError as HF does);
`typical_p` / `epsilon_cutoff` / `eta_cutoff` (kwargs, then `generation_config`) follow them on the device
(`Engine.set_entropy_filter`; None, 1.0 / 0.0 / 0.0 mean off, values outside (0, 1) raise HF's ValueError);
`num_beams` must be 1.
"""
from __future__ import annotations

import json
import os
from collections import OrderedDict
from dataclasses import dataclass
from types import SimpleNamespace
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import processor as _processor
from .chain_request import ChainRequest
from .checkpoint import iter_checkpoint, read_adapter
from .config import ModelConfig
from .scheduler import KEEP_ADAPTER
from .score_plan import PlanItem, plan_score_passes, score_columns
from .engine import MAX_LOGIT_BIAS, MAX_RULE_INTS, MAX_RULE_LEN, MAX_RULE_WORDS, MAX_TOP_LOGPROBS, Engine


@dataclass
class GenerateOutput:
    """What generate(logprobs=N) returns.  sequences: the id tensor generate returns without it; logprobs f32 [rows, new]: the
    log-probability of every generated token (0 past a row's end); top_ids int32 / top_logprobs f32 [rows, new, N]: the step's N
    best tokens, best first (-1 / -inf past a row's end and where a step had fewer finite logits)."""
    sequences: torch.Tensor
    logprobs: torch.Tensor
    top_ids: torch.Tensor
    top_logprobs: torch.Tensor


@dataclass
class BeamSearchOutput:
    """What beam_search(return_dict_in_generate=True) returns, HF's GenerateBeamDecoderOnlyOutput in the fields this path fills:
    sequences [rows * num_return_sequences, prompt + new]; sequences_scores f32 (None without output_scores); beam_indices int32
    [.., new]: per generated token the running beam it extended, the row's offset row * num_beams included, -1 behind a row's end."""
    sequences: torch.Tensor
    sequences_scores: Optional[torch.Tensor]
    beam_indices: torch.Tensor


class ScoreItem(NamedTuple):
    """One sequence of `score_sequences`: its ids; its images in order -- grids (t, h, w), ViT features bf16 [merged rows,
    hidden] and identity keys (None: never shared); and the first position whose next-token log-probability is wanted."""
    ids: list
    grids: list
    feats: list
    keys: Optional[list] = None
    score_from: int = 0


class _Rows(NamedTuple):
    """The rows of one generate() call as the row loop reads them: ids and mask on the host, the images' grids, keys and patch-row
    offsets in prompt order, and the caller's tensors."""
    ids_cpu: np.ndarray
    mask: np.ndarray
    grids: list
    keys: list
    offs: np.ndarray
    pixel_values: Optional[torch.Tensor]
    input_ids: torch.Tensor


class adapter_scope:
    """`with adapter_scope(model, name_or_None):` runs the block under that adapter (None = the base weights) and puts the previously
    active one back on exit, also on an exception.  KEEP_ADAPTER: nothing is switched.  A switch that changes nothing launches
    nothing (ze_lora_activate).  Not for a model whose ChainScheduler has live chains: their K/V rows belong to the weights that made
    them (the scheduler's own `set_adapter` refuses then; this does not know of it)."""

    def __init__(self, model, adapter):
        self.model, self.adapter = model, adapter

    def __enter__(self):
        if self.adapter is not KEEP_ADAPTER:
            self.before = self.model.active_adapter
            self.model.set_adapter(self.adapter)
        return self.model

    def __exit__(self, *exc):
        if self.adapter is not KEEP_ADAPTER:
            self.model.set_adapter(self.before)
        return False


class ZoomEarthForConditionalGeneration:
    def __init__(self, config: ModelConfig, engine: Engine, generation_config=None):
        self.config = config
        self.engine = engine
        self.generation_config = generation_config or SimpleNamespace(
            temperature=None, top_p=None, top_k=None, repetition_penalty=1.0, do_sample=False,
            eos_token_id=list(config.eos_token_ids), pad_token_id=config.pad_token_id)
        self._vit_cache = OrderedDict()   # image key -> bf16 features
        self._chains = OrderedDict()      # slot -> (prompt ids tuple, image keys tuple)
        self._next_slot = 0
        self.reuse_prefix = True
        self._adapters = {}               # adapter name -> engine adapter id (which one is active is the ENGINE's state)
        _processor.set_default_engine(engine)

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_pretrained(cls, path: str, torch_dtype=None, device=None, max_seqs: int = 4, max_ctx: int = 4096,
                        max_patches: int = 8192, max_tile_side: int = 8192, max_prefill_rows: int = 0, broadcast=False, **kw):
        """broadcast=True under WORLD_SIZE > 1 (one rank per GPU): only rank 0 reads the safetensors, the other ranks
        receive the packed weight arena in ONE collective (accel.broadcast_engine_weights: RCCL over xGMI) -- where the
        reference has every rank read the checkpoint itself (/root/reference/src/eval/infer.py:147-151).  The seconds the
        collective took are left in `model.weight_broadcast_s`.
        A PEFT adapter directory (adapter_config.json, no config.json): the base model named by its `base_model_name_or_path` -- or
        by the `base=` keyword -- is loaded as above, then the adapter is loaded and activated (`load_adapter`, `set_adapter`); under
        broadcast every rank applies it itself after the base broadcast (A / B are a few MB).
        weight_format="fp8" / "mxfp4" (reduced precision, opt-in; default bf16): the decoder's linear layers are quantised once the
        weights -- with the adapter merged, if the path is one -- are in place (Engine.set_weight_format); `set_adapter` quantises
        again after every switch, since a switch returns the engine to bf16."""
        base = kw.pop("base", None)
        weight_format = kw.pop("weight_format", None)
        if os.path.exists(os.path.join(path, "adapter_config.json")) and not os.path.exists(os.path.join(path, "config.json")):
            if base is None:
                with open(os.path.join(path, "adapter_config.json"), encoding="utf-8") as f:
                    base = json.load(f).get("base_model_name_or_path")
            if not base:
                raise ValueError(f"{path}: adapter_config.json names no base_model_name_or_path (pass base=)")
            model = cls.from_pretrained(base, torch_dtype=torch_dtype, device=device, max_seqs=max_seqs, max_ctx=max_ctx,
                                        max_patches=max_patches, max_tile_side=max_tile_side, max_prefill_rows=max_prefill_rows,
                                        broadcast=broadcast, **kw)
            try:
                model.load_adapter(path)
                model.weight_format = weight_format
                model.set_adapter("default")
            except Exception:
                model.engine.close()
                raise
            return model
        config = ModelConfig.from_pretrained(path)
        dev = 0 if device is None else (device.index or 0 if isinstance(device, torch.device) else int(device))
        if device is None and "LOCAL_RANK" in os.environ:  # (more local ranks than GPUs: ranks share GPUs, accel.Accelerator)
            dev = int(os.environ["LOCAL_RANK"]) % max(1, torch.cuda.device_count())
        engine = Engine(config, device=dev, max_seqs=max_seqs, max_ctx=max_ctx, max_patches=max_patches,
                        max_tile_side=max_tile_side, max_prefill_rows=max_prefill_rows)
        rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
        broadcast = bool(broadcast) and world > 1
        bcast_s = 0.0
        try:
            if not broadcast or rank == 0:
                synth = None
                with open(os.path.join(path, "config.json"), encoding="utf-8") as f:
                    synth = json.load(f).get("zoomearth_synthetic_weights")
                if synth is not None:
                    # a checkpoint directory WITHOUT weight files whose config.json asks for the repo's synthetic weights
                    # (tools/bench_infer_e2e.py: the 3B shape end to end through src/infer.py with no 7.5-GB file on disk)
                    engine.fill_synthetic(**synth)
                    engine.assert_ready()
                else:
                    engine.load_state_dict(iter_checkpoint(path))
            if broadcast:
                from .accel import broadcast_engine_weights
                bcast_s = broadcast_engine_weights(engine, rank, world, src=0)
                engine.assert_ready()
        except Exception:
            engine.close()
            raise
        gen = SimpleNamespace(temperature=None, top_p=None, top_k=None, repetition_penalty=1.0, do_sample=False,
                              eos_token_id=list(config.eos_token_ids), pad_token_id=config.pad_token_id)
        gp = os.path.join(path, "generation_config.json")
        if os.path.exists(gp):
            with open(gp, encoding="utf-8") as f:
                for k, v in json.load(f).items():
                    setattr(gen, k, v)
        model = cls(config, engine, gen)
        model.weight_broadcast_s = bcast_s
        try:
            engine.set_weight_format(weight_format)
        except Exception:
            engine.close()
            raise
        model.weight_format = weight_format
        return model

    @classmethod
    def from_synthetic(cls, config: ModelConfig, seed: int = 0, std: float = 0.02, matrix_gain: float = 1.0,
                       bias_std: float = 0.0, norm_jitter: float = 0.0, device: int = 0, **engine_kw):
        engine = Engine(config, device=device, **engine_kw)
        engine.fill_synthetic(seed, std, matrix_gain, bias_std, norm_jitter)
        return cls(config, engine)

    def eval(self):
        return self

    def clone_lane(self, **engine_kw):
        """A second engine on the same GPU with a copy of this model's weights (device-to-device), for a further LANE of
        question chains: its own KV cache, workspaces, scheduler thread and HIP stream, so that the prefill / ViT rounds of
        one lane overlap the decode bursts of the other (src/eval/infer.py --lanes; bench.py --lanes).
        A lane cloned while a LoRA adapter is active takes the MERGED weights as its base: it has no adapters of its own, and
        nothing can take the delta out of it again."""
        e = self.engine
        kw = dict(device=e.device.index or 0, max_seqs=e.max_seqs, max_ctx=e.max_ctx, max_patches=e.max_patches,
                  max_tile_side=int(e.zcfg.max_tile_side), max_prefill_rows=int(e.zcfg.max_prefill_rows))
        kw.update(engine_kw)
        e2 = Engine(self.config, **kw)
        try:
            e2.weights_arena().copy_(e.weights_arena())
            torch.cuda.synchronize(e.device)
            e2.weights_invalidate()
            e2.assert_ready()
        except Exception:
            e2.close()
            raise
        gen = SimpleNamespace(**vars(self.generation_config))
        lane = ZoomEarthForConditionalGeneration.__new__(ZoomEarthForConditionalGeneration)
        lane.config, lane.engine, lane.generation_config = self.config, e2, gen
        lane._vit_cache, lane._chains, lane._next_slot, lane.reuse_prefix = OrderedDict(), OrderedDict(), 0, True
        lane.weight_broadcast_s = 0.0
        lane._adapters = {}
        return lane

    # ------------------------------------------------------------------ LoRA adapters
    def load_adapter(self, path_or_tensors, adapter_name: str = "default"):
        """replaces: PeftModel.from_pretrained / load_adapter.  A PEFT LoRA directory (checkpoint.read_adapter) or its tensors
        {base key: (A, B, r, scale)}: resident on the device under `adapter_name`, not active until `set_adapter`."""
        if adapter_name in self._adapters:
            raise ValueError(f"adapter {adapter_name!r} is already loaded")
        tensors = read_adapter(path_or_tensors)[1] if isinstance(path_or_tensors, (str, os.PathLike)) else path_or_tensors
        self._adapters[adapter_name] = self.engine.lora_load(tensors)
        return adapter_name

    @property
    def active_adapter(self):
        """The name of the adapter merged into the engine's weights, None for the base weights.  Read from the engine: a base-weight
        write (load_state_dict, fill_synthetic, weights_invalidate, a broadcast) under an active adapter leaves none active."""
        adapters = getattr(self, "_adapters", None)
        if not adapters:
            return None
        active = self.engine.lora_info()[0]
        return next((name for name, a in adapters.items() if a == active), None)

    def set_adapter(self, name) -> None:
        """replaces: PeftModel.set_adapter; None = the base weights.  Cached ViT features and chains belong to the weights that made
        them: every switch forgets them.  The chains of a running ChainScheduler on this model are not known here: switch through
        the scheduler (`ChainScheduler(adapter=)`, `set_adapter`), which refuses while chains are live, never under it."""
        if name is not None and name not in self._adapters:
            raise ValueError(f"no adapter {name!r} (loaded: {sorted(self._adapters)})")
        if name == self.active_adapter:
            return
        self.engine.lora_activate(None if name is None else self._adapters[name])
        self.engine.set_weight_format(getattr(self, "weight_format", None))   # (the switch dropped the quantised stream)
        self._vit_cache.clear()
        self._chains.clear()

    def disable_adapter(self):
        """replaces: `with model.disable_adapter():` (the reference policy of the GRPO step, grpo_trainer.py:679)."""
        return adapter_scope(self, None)

    def delete_adapter(self, name) -> None:
        if name not in self._adapters:
            raise ValueError(f"no adapter {name!r}")
        if name == self.active_adapter:
            self.set_adapter(None)
        self.engine.lora_destroy(self._adapters.pop(name))

    @property
    def device(self):
        return self.engine.device

    # ------------------------------------------------------------------ helpers
    def _features(self, pv_rows, grid, key):
        """ViT features of one image, cached by image identity (bit-identical to recomputation)."""
        if key is not None and key in self._vit_cache:
            self._vit_cache.move_to_end(key)
            return self._vit_cache[key]
        f = self.engine.vit_forward(pv_rows.contiguous(), [grid])
        if key is not None:
            self._vit_cache[key] = f
            while len(self._vit_cache) > 8:
                self._vit_cache.popitem(last=False)
        return f

    def _pick_slot(self, ids, keys):
        """Returns (slot, reusable prefix length).  A cached chain is reusable when its prefilled prompt is a
        strict prefix of `ids` and the images inside that prefix are the same objects."""
        if self.reuse_prefix and all(k is not None for k in keys):
            for slot, (pids, pkeys) in self._chains.items():
                n = len(pids)
                if 0 < n < len(ids) and tuple(ids[:n]) == pids and tuple(keys[: len(pkeys)]) == pkeys \
                        and ids[n] != self.config.image_token_id:
                    return slot, n
        slot = self._next_slot
        self._next_slot = (self._next_slot + 1) % self.engine.max_seqs
        return slot, 0

    # ------------------------------------------------------------------ rollout scoring
    @torch.no_grad()
    def per_token_logps(self, input_ids, attention_mask=None, pixel_values=None, image_grid_thw=None,
                        image_keys=None, score_from: Optional[int] = None, share_prefix: bool = True, min_shared: int = 64,
                        adapter=KEEP_ADAPTER, **kw):
        """Log-probability of every token given its prefix: f32 [B, L - 1], column t = log p(input_ids[:, t + 1]).
        adapter: a loaded adapter's name or None (the base weights, the GRPO step's reference policy) to score under; the previously
        active one is back afterwards.
        Same result layout as `_get_per_token_logps(model, input_ids, attention_mask, pixel_values=...,
        image_grid_thw=...)` of the reference's GRPO trainer (src/train/RL/src/open-r1-multimodal/src/open_r1/
        trainer/grpo_trainer.py:494-504), which it calls without gradients for the old policy and the reference
        model (:660-683).  Padded positions (attention_mask 0) are skipped, their columns are 0.
        score_from = k: columns t < k are not computed and stay 0 (the trainer keeps `[:, prompt_length - 1:]` only, so
        k = prompt_length - 1 skips the final norm, the lm_head and the log-softmax of every prompt position); shape, layout
        and padding rules are unchanged.  The rows run together through `score_sequences`."""
        e = self.engine
        with adapter_scope(self, adapter):   # (the ViT features of _score_items belong to the adapter too)
            items, where, shape = self._score_items(input_ids, attention_mask, pixel_values, image_grid_thw, image_keys, score_from)
            out = torch.zeros(shape, dtype=torch.float32, device=e.device)
            for (b, cols), lp in zip(where, self.score_sequences(items, share_prefix=share_prefix, min_shared=min_shared)):
                out[b, torch.as_tensor(cols, device=e.device)] = lp
        return out.to(input_ids.device) if input_ids.device.type != "cpu" else out.cpu()

    def _score_items(self, input_ids, attention_mask, pixel_values, image_grid_thw, image_keys, score_from):
        """The ScoreItems of a padded batch, where each lands ((row, columns) per item) and the result shape (B, L - 1)."""
        cfg = self.config
        ids_cpu = input_ids.cpu().numpy()
        mask = attention_mask.cpu().numpy().astype(bool) if attention_mask is not None else np.ones_like(ids_cpu, bool)
        grids = image_grid_thw.cpu().numpy().tolist() if image_grid_thw is not None else []
        keys = list(image_keys) if image_keys is not None else [None] * len(grids)
        rows_per = [g[0] * g[1] * g[2] for g in grids]
        offs = np.concatenate([[0], np.cumsum(rows_per)]).astype(int)
        gi = 0
        items, where = [], []
        for b in range(ids_cpu.shape[0]):
            valid = np.nonzero(mask[b])[0]
            ids = ids_cpu[b][valid].astype(np.int64).tolist()
            is_img = np.asarray(ids) == cfg.image_token_id
            n_img = int((is_img & ~np.concatenate([[False], is_img[:-1]])).sum())
            my = list(range(gi, gi + n_img))
            gi += n_img
            if gi > len(grids):
                raise ValueError("Image features and image tokens do not match")
            if len(ids) < 2:
                continue
            first, cols = score_columns(valid, score_from)
            if not cols:
                continue
            feats = [self._features(pixel_values[offs[i]:offs[i + 1]], grids[i], keys[i]) for i in my]
            items.append(ScoreItem(ids, [grids[i] for i in my], feats, [keys[i] for i in my], first))
            where.append((b, cols))
        return items, where, (ids_cpu.shape[0], max(ids_cpu.shape[1] - 1, 0))

    @torch.no_grad()
    def per_token_details(self, input_ids, attention_mask=None, pixel_values=None, image_grid_thw=None, image_keys=None,
                          score_from: Optional[int] = None, top_n: int = 0, entropy: bool = True, rank: bool = False,
                          share_prefix: bool = True, min_shared: int = 64, **kw):
        """per_token_logps with more per position, from the same passes (`score_sequences` with a request): a dict with `logps`
        f32 [B, L - 1] (the bits of per_token_logps) and, where asked, `entropy` f32 [B, L - 1] (the policy's per-token entropy a GRPO
        trainer logs and masks on), `rank` int32 [B, L - 1] and `top_ids` int32 / `top_logprobs` f32 [B, L - 1, top_n].  The padding
        rules are those of per_token_logps: columns of padded positions and columns before score_from hold 0 (rank -1, top ids -1,
        top log-probabilities -inf)."""
        e = self.engine
        items, where, shape = self._score_items(input_ids, attention_mask, pixel_values, image_grid_thw, image_keys, score_from)
        out = dict(logps=torch.zeros(shape, dtype=torch.float32, device=e.device))
        if entropy:
            out["entropy"] = torch.zeros(shape, dtype=torch.float32, device=e.device)
        if rank:
            out["rank"] = torch.full(shape, -1, dtype=torch.int32, device=e.device)
        if top_n:
            out["top_ids"] = torch.full(shape + (top_n,), -1, dtype=torch.int32, device=e.device)
            out["top_logprobs"] = torch.full(shape + (top_n,), float("-inf"), dtype=torch.float32, device=e.device)
        res = self.score_sequences(items, share_prefix=share_prefix, min_shared=min_shared, top_n=top_n, entropy=entropy, rank=rank)
        for (b, cols), d in zip(where, res):
            c = torch.as_tensor(cols, device=e.device)
            for name in out:
                out[name][b, c] = getattr(d, name)
        return {k: (v.to(input_ids.device) if input_ids.device.type != "cpu" else v.cpu()) for k, v in out.items()}

    @torch.no_grad()
    def score_sequences(self, items, share_prefix: bool = True, min_shared: int = 64, top_n: int = 0, entropy: bool = False,
                        rank: bool = False, adapter=KEEP_ADAPTER):
        """`_score_sequences` under `adapter` (a loaded adapter's name, or None for the base weights); the previously active adapter is
        back afterwards.  The items' ViT features are the caller's: for an adapter that touches the vision tower they have to come
        from the same weights."""
        with adapter_scope(self, adapter):
            return self._score_sequences(items, share_prefix, min_shared, top_n, entropy, rank)

    def _score_sequences(self, items, share_prefix: bool = True, min_shared: int = 64, top_n: int = 0, entropy: bool = False,
                         rank: bool = False):
        """Scores many sequences in as few passes as the engine's limits allow: one f32 tensor per ScoreItem, on the device,
        with the log-probability of the next id at positions item.score_from .. len(ids) - 2 -- the bits `Engine.score` of
        the sequence alone gives there.  The plan (score_plan.plan_score_passes) packs the sequences into `score_batch`
        passes of at most max_prefill_rows rows and max_seqs chains; with share_prefix, sequences with a common prompt (the G
        generations of a sample) prefill it once: one of them whole, in an earlier pass, the others copy its K/V rows
        (`seq_copy_prefix`, bit-identical) and prefill their tails.  The chain slots are scratch: cached chains of generate()
        are forgotten.  `last_score_stats` tells what the call did.
        top_n / entropy / rank: with any of them the passes go through `score_batch_detail` and every item gets a ScoreDetail
        (`logps` the same bits; the members not asked for None) instead of the tensor; with none, nothing changes."""
        e, cfg = self.engine, self.config
        detail = bool(top_n) or entropy or rank
        plan = plan_score_passes([PlanItem(it.ids, list(it.keys) if it.keys is not None else [None] * len(it.grids), it.score_from)
                                  for it in items], e.max_prefill_rows, e.max_seqs, cfg.image_token_id, share_prefix, min_shared)
        self._chains.clear()
        self._next_slot = 0
        out = [torch.zeros(0, dtype=torch.float32, device=e.device) for _ in items]
        stats = dict(passes=len(plan), rows_per_pass=[], shared_rows=0, scored_rows=0)
        for entries in plan:
            slots, ids_l, emb_l, pos_l, dl, sf = [], [], [], [], [], []
            for en in entries:
                it = items[en.item]
                pos, delta = e.rope_index(it.ids, it.grids)
                e.seq_reset(en.slot)
                if en.copy_from is not None:
                    e.seq_copy_prefix(en.slot, en.copy_from, en.start)
                    stats["shared_rows"] += en.start
                feats = list(it.feats[en.n_images:])
                slots.append(en.slot)
                ids_l.append(it.ids[en.start:])
                emb_l.append((torch.cat(feats) if len(feats) > 1 else feats[0]) if feats else None)
                pos_l.append(pos[:, en.start:])
                dl.append(delta)
                sf.append(it.score_from - en.start)
            if detail:
                det = e.score_batch_detail(slots, ids_l, emb_l, pos_l, dl, sf, top_n=top_n, entropy=entropy, rank=rank)
                off = det.offsets
            else:
                flat, off = e.score_batch(slots, ids_l, emb_l, pos_l, dl, sf)
            stats["rows_per_pass"].append(sum(len(x) for x in ids_l))
            stats["scored_rows"] += off[-1]
            for k, en in enumerate(entries):
                out[en.item] = det.chain(k) if detail else flat[off[k]:off[k + 1]]
        self.last_score_stats = stats
        return out

    # ------------------------------------------------------------------ generate
    @staticmethod
    def _logit_adjust_request(kw):
        """(presence_penalty, frequency_penalty, min_new_tokens, {id: bias}) from generate's keyword arguments, all-off values when
        nothing is asked for.  HF's `min_new_tokens`, `sequence_bias` (single-token keys) and `suppress_tokens`
        with HF's ValueErrors (MinNewTokensLengthLogitsProcessor, SequenceBiasLogitsProcessor, SuppressTokensLogitsProcessor);
        `presence_penalty`, `frequency_penalty` and `logit_bias` {id: bias} as the OpenAI API names them."""
        min_new = kw.get("min_new_tokens")
        if min_new is not None and (isinstance(min_new, bool) or not isinstance(min_new, (int, np.integer)) or min_new < 0):
            raise ValueError(f"`min_new_tokens` has to be a positive integer, but is {min_new}")
        bias = {}
        lb = kw.get("logit_bias")
        if lb is not None:
            if not isinstance(lb, dict):
                raise ValueError(f"`logit_bias` has to be a dictionary of token id -> bias, but is {lb}")
            for k, v in lb.items():
                if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                    raise ValueError(f"`logit_bias` has to be a dict with floats as values, but is {lb}")
                bias[int(k)] = float(v)
        sb = kw.get("sequence_bias")
        if sb is not None:
            if (not isinstance(sb, (dict, list))) or len(sb) == 0:
                raise ValueError(f"`sequence_bias` has to be a non-empty dictionary, or non-empty list of lists but is {sb}.")
            items = list(sb.items()) if isinstance(sb, dict) else [(tuple(x[0]) if isinstance(x, (list, tuple)) and len(x) == 2
                                                                      and isinstance(x[0], (list, tuple)) else None, x[1] if
                                                                     isinstance(x, (list, tuple)) and len(x) == 2 else None) for x in sb]
            if any(not isinstance(k, tuple) for k, _ in items):
                raise ValueError(f"`sequence_bias` has to be a dict with tuples as keys, but is {sb}.")
            if any(len(k) == 0 or any(isinstance(t, bool) or not isinstance(t, (int, np.integer)) or t < 0 for t in k) for k, _ in items):
                raise ValueError(f"Each key in `sequence_bias` has to be a non-empty tuple of positive integers, but is {sb}.")
            if any(isinstance(v, bool) or not isinstance(v, (float, np.floating)) for _, v in items):
                raise ValueError(f"`sequence_bias` has to be a dict with floats as values, but is {sb}.")
            for k, v in items:
                if len(k) != 1:
                    raise ValueError(f"`sequence_bias` keys are limited to a single token here (multi-token sequences are not "
                                     f"supported), but {k} has {len(k)}")
                bias[int(k[0])] = bias.get(int(k[0]), 0.0) + float(v)
        st = kw.get("suppress_tokens")
        if st is not None:
            for t in list(st):
                if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or t < 0:
                    raise ValueError(f"`suppress_tokens` has to be a list of positive integers, but is {st}")
                bias[int(t)] = float("-inf")
        pens = []
        for name in ("presence_penalty", "frequency_penalty"):
            v = kw.get(name)
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v)):
                raise ValueError(f"`{name}` has to be a finite float, but is {v}")
            pens.append(float(v or 0.0))
        bias = {k: v for k, v in bias.items() if v != 0.0}
        if len(bias) > MAX_LOGIT_BIAS:
            raise ValueError(f"at most {MAX_LOGIT_BIAS} tokens can carry a bias, but {len(bias)} do")
        return pens[0], pens[1], int(min_new or 0), bias

    @staticmethod
    def _token_rules_request(kw):
        """(no_repeat_ngram_size, stop records, bad-word records, stop strings) from generate's keyword arguments, all-off values
        when nothing is asked for.  HF's `no_repeat_ngram_size`, `bad_words_ids` and `stop_strings` (with
        `tokenizer=`) with HF's ValueErrors (NoRepeatNGramLogitsProcessor, NoBadWordsLogitsProcessor, GenerationMixin); vLLM's
        `stop_token_ids`."""
        def is_int(t):
            return not isinstance(t, bool) and isinstance(t, (int, np.integer))

        ngram = kw.get("no_repeat_ngram_size")
        if ngram is not None and ngram != 0 and (not is_int(ngram) or ngram <= 0):
            raise ValueError(f"`ngram_size` has to be a strictly positive integer, but is {ngram}")
        if ngram and ngram > MAX_RULE_LEN:
            raise ValueError(f"`no_repeat_ngram_size` is limited to {MAX_RULE_LEN} here, but is {ngram}")
        bad = kw.get("bad_words_ids")
        if bad is not None:
            if not isinstance(bad, list) or len(bad) == 0:
                raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bad}.")
            if any(not isinstance(b, list) for b in bad):
                raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bad}.")
            if any(len(b) == 0 or any(not is_int(t) or t < 0 for t in b) for b in bad):
                raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {bad}.")
        bad = [[int(t) for t in b] for b in (bad or [])]
        stop_ids = kw.get("stop_token_ids")
        if stop_ids is not None and (not isinstance(stop_ids, (list, tuple)) or any(not is_int(t) or t < 0 for t in stop_ids)):
            raise ValueError(f"`stop_token_ids` has to be a list of positive integers, but is {stop_ids}")
        stop = [[int(t)] for t in (stop_ids or [])]
        strings, tokenizer = kw.get("stop_strings"), kw.get("tokenizer")
        if isinstance(strings, str):
            strings = [strings]
        strings = list(strings or [])
        if strings:
            if tokenizer is None:
                raise ValueError("There are one or more stop strings, either in the arguments to `generate` or in the model's generation "
                                 "config, but we could not locate a tokenizer. When generating with stop strings, you must pass the "
                                 "model's tokenizer to the `tokenizer` argument of `generate`.")
            if any(not isinstance(x, str) for x in strings):
                raise ValueError(f"`stop_strings` has to be a string or a list of strings, but is {kw.get('stop_strings')}")
            from .hostloop import stop_string_records
            stop += [r for r in stop_string_records(tokenizer, strings) if len(r) <= MAX_RULE_LEN and r not in stop]
        for name, recs in (("stop sequences", stop), ("bad_words_ids", bad)):
            if len(recs) > MAX_RULE_WORDS or sum(1 + len(r) for r in recs) > MAX_RULE_INTS or any(len(r) > MAX_RULE_LEN for r in recs):
                raise ValueError(f"{name}: at most {MAX_RULE_WORDS} sequences of at most {MAX_RULE_LEN} tokens, {MAX_RULE_INTS} ints packed")
        return int(ngram or 0), stop, bad, strings

    @staticmethod
    def _entropy_filter_request(kw, gc) -> dict:
        """generate's `typical_p` / `epsilon_cutoff` / `eta_cutoff` (kwargs, then generation_config) as Engine.generate takes them: only
        the ones that are on (HF's off values: None or 1.0 / 0.0 / 0.0); HF's errors for anything else outside (0, 1)."""
        out = {}
        for name, off in (("typical_p", 1.0), ("epsilon_cutoff", 0.0), ("eta_cutoff", 0.0)):
            v = kw.get(name) if kw.get(name) is not None else getattr(gc, name, None)
            if v is None:
                continue
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError(f"`{name}` has to be a float > 0 and < 1, but is {v}")
            v = float(v)
            if v == off:
                continue
            if not (0.0 < v < 1.0):
                raise ValueError(f"`{name}` has to be a float > 0 and < 1, but is {v}")
            out[name] = v
        return out

    @staticmethod
    def _speculation_request(kw, do_sample, num_return_sequences=1):
        """(k, largest n-gram) from generate's `prompt_lookup_num_tokens` / `max_matching_ngram_size`; (0, 3) when not asked for."""
        k, g = kw.get("prompt_lookup_num_tokens"), kw.get("max_matching_ngram_size")
        if k is None:
            if g is not None:
                raise ValueError("`max_matching_ngram_size` needs `prompt_lookup_num_tokens`")
            return 0, 3
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not (1 <= k <= 8):
            raise ValueError(f"`prompt_lookup_num_tokens` has to be an integer in [1, 8], but is {k!r}")
        g = 3 if g is None else g
        if isinstance(g, bool) or not isinstance(g, (int, np.integer)) or not (1 <= g <= 8):
            raise ValueError(f"`max_matching_ngram_size` has to be an integer in [1, 8], but is {g!r}")
        if kw.get("prompt_lookup_sampling"):   # the sampled mode (Engine.set_speculation(sampled=True)): opt-in, rows budgeted by the caller
            return int(k), int(g)
        if do_sample or num_return_sequences != 1:
            raise ValueError("`prompt_lookup_num_tokens` is greedy speculative decoding here: it is not supported with "
                             "`do_sample=True` or `num_return_sequences` > 1.")
        return int(k), int(g)

    def compile_grammar(self, guided_regex=None, guided_choice=None, tokenizer=None):
        """The token automaton (zoomearth_amd.grammar.TokenAutomaton) of vLLM's `guided_regex` (a pattern) or `guided_choice` (a list
        of strings) against `tokenizer`'s vocabulary, padded to the model's; compiled once per pattern and tokenizer (a small memo on
        the host).  ValueError for both at once, a wrong type, a tokenizer that is no byte-level BPE or a pattern that does not
        compile."""
        from . import grammar
        if guided_regex is not None and guided_choice is not None:
            raise ValueError("`guided_regex` and `guided_choice` exclude each other")
        if guided_regex is not None and not isinstance(guided_regex, str):
            raise ValueError(f"`guided_regex` has to be a string, but is {guided_regex!r}")
        if guided_regex is None and (not isinstance(guided_choice, (list, tuple)) or not guided_choice or
                                     any(not isinstance(c, str) or not c for c in guided_choice)):
            raise ValueError(f"`guided_choice` has to be a non-empty list of non-empty strings, but is {guided_choice!r}")
        tokenizer = tokenizer if tokenizer is not None else getattr(self, "tokenizer", None)
        if tokenizer is None:
            raise ValueError("guided decoding compiles the pattern against the vocabulary: pass the model's tokenizer to the "
                             "`tokenizer` argument of `generate`.")
        memo = self.__dict__.setdefault("_automata", OrderedDict())
        key = (id(tokenizer), "regex", guided_regex) if guided_regex is not None else (id(tokenizer), "choice", tuple(guided_choice))
        if key in memo:
            memo.move_to_end(key)
            return memo[key][1]
        vkey = (id(tokenizer), "vocab")
        if vkey not in memo:
            memo[vkey] = (tokenizer, grammar.token_bytes(tokenizer, self.config.text.vocab_size)[:self.config.text.vocab_size])
        vocab = memo[vkey][1]
        memo.move_to_end(vkey)
        auto = grammar.compile_regex(guided_regex, vocab) if guided_regex is not None else grammar.compile_choice(guided_choice, vocab)
        memo[key] = (tokenizer, auto)   # (the tokenizer is kept alive: its id is the key)
        while len(memo) > 33:
            memo.popitem(last=False)
        return auto

    @torch.no_grad()
    def generate(self, input_ids=None, attention_mask=None, pixel_values=None, image_grid_thw=None,
                 mm_token_type_ids=None, image_keys=None, max_new_tokens: int = 20, do_sample: bool = False,
                 num_beams: int = 1, temperature=None, top_p=None, top_k=None, repetition_penalty=None,
                 ignore_eos: bool = False, logprobs: Optional[int] = None, num_return_sequences: int = 1, **kw):
        """`num_return_sequences` = k > 1 (sampling only, as in HF): k completions per input row, returned batch-major as HF lays them
        out -- rows (b0 r0, b0 r1, ..., b1 r0, ...) of a [batch * k, len] result, log-probabilities likewise.  Each input row is
        prefilled once and forked on the device (`Engine.seq_fork`); the completions are bit for bit those of a call on
        `input_ids.repeat_interleave(k, 0)`: row b * k + r draws on stream b * k + r.
        `logprobs`: None returns the id tensor; an int in 0 .. 20 returns a GenerateOutput with the log-probability of every
        generated token under the model's own distribution (the step's fp32 logits, before repetition penalty, temperature
        and filters) and that many best alternatives per step, computed on the device inside the decode step.
        `guided_regex` / `guided_choice` (vLLM's; with `tokenizer=`): every row is held to the pattern by a token automaton on the
        device (zoomearth_amd/grammar.py), set after each chain's prefill where the token rules are set.
        `prompt_lookup_num_tokens` = k (HF's; 1 .. 8) with `max_matching_ngram_size` (default 3, as HF's is 2 .. here up to 8):
        speculative decoding by prompt lookup on the device (Engine.set_speculation), greedy only.  The call goes through the
        family-0 bursts (Engine.generate_speculative) and returns bit for bit what those bursts return without it -- the batched
        family's sequence, which agrees with the single-chain path's within bf16 rounding.
        `prompt_lookup_sampling=True` with it: the sampled mode -- `do_sample=True` with temperature, seed and top-k / top-p / min-p
        (and `num_return_sequences` > 1 while two rows per completion fit a step's 64) speculate too; every row draws the token the
        plain family-0 bursts draw with the same seed, so the result is still theirs bit for bit."""
        if num_beams != 1:
            raise NotImplementedError("beam search is not part of the ZoomEarth path (num_beams=1 everywhere)")
        k = num_return_sequences
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError(f"`num_return_sequences` has to be a strictly positive integer, but is {k}")
        if k > 1 and not do_sample:
            raise ValueError(f"Greedy methods without beam search do not support `num_return_sequences` different than 1 (got {k}).")
        if logprobs is not None:
            if isinstance(logprobs, bool) or not isinstance(logprobs, (int, np.integer)) or not (0 <= logprobs <= MAX_TOP_LOGPROBS):
                raise ValueError(f"`logprobs` has to be None or an integer in [0, {MAX_TOP_LOGPROBS}], but is {logprobs}")
            logprobs = int(logprobs)
        e, cfg = self.engine, self.config
        ids_cpu = input_ids.cpu().numpy()
        mask = attention_mask.cpu().numpy().astype(bool) if attention_mask is not None else np.ones_like(ids_cpu, bool)
        grids = image_grid_thw.cpu().numpy().tolist() if image_grid_thw is not None else []
        keys = list(image_keys) if image_keys is not None else [None] * len(grids)
        rows_per = [g[0] * g[1] * g[2] for g in grids]
        offs = np.concatenate([[0], np.cumsum(rows_per)]).astype(int)
        pen = repetition_penalty if repetition_penalty is not None else getattr(self.generation_config, "repetition_penalty", 1.0) or 1.0
        gc = self.generation_config
        top_k = top_k if top_k is not None else getattr(gc, "top_k", None)
        top_p = top_p if top_p is not None else getattr(gc, "top_p", None)
        temperature = temperature if temperature is not None else getattr(gc, "temperature", None)
        if do_sample and top_k == 1 and k == 1:
            do_sample = False  # a one-token nucleus is the arg-max
        min_p = kw.get("min_p") if kw.get("min_p") is not None else getattr(gc, "min_p", None)
        filt_kw = {}
        if do_sample:  # HF's warpers in HF's order, on the device (Engine.set_sampling_filter); HF's "off" values and HF's errors
            if top_k not in (None, 0) and (not isinstance(top_k, (int, np.integer)) or top_k < 0):
                raise ValueError(f"`top_k` has to be a strictly positive integer, but is {top_k}")
            if top_p is not None and not (0.0 <= float(top_p) <= 1.0):
                raise ValueError(f"`top_p` has to be a float > 0 and < 1, but is {top_p}")
            if min_p is not None and not (0.0 <= float(min_p) <= 1.0):
                raise ValueError(f"`min_p` has to be a float in the [0, 1] interval, but is {min_p}")
            # (top_p = 0 keeps HF's min_tokens_to_keep = 1, the arg-max: the smallest positive value does the same)
            filt_kw = dict(top_k=int(top_k or 0), top_p=1.0 if top_p is None else max(float(top_p), 1e-37),
                           min_p=float(min_p or 0.0))
        ent_kw = self._entropy_filter_request(kw, gc)
        if ent_kw and kw.get("prompt_lookup_num_tokens") is not None:
            raise ValueError("`prompt_lookup_num_tokens` is greedy speculative decoding and cannot be combined with "
                             "`typical_p`, `epsilon_cutoff` or `eta_cutoff`")
        if do_sample:   # (without do_sample they are ignored, as HF ignores its warpers)
            filt_kw.update(ent_kw)
        presence, frequency, min_new, bias = self._logit_adjust_request(kw)
        ngram, stop, bad, stop_strings = self._token_rules_request(kw)
        spec_k, spec_g = self._speculation_request(kw, do_sample, k)
        spec_sampling = bool(spec_k and kw.get("prompt_lookup_sampling"))
        if spec_sampling and k > 1 and ids_cpu.shape[0] * k * 2 > 64:   # (1 + k_eff rows per completion, k_eff >= 1: generate_speculative's budget)
            raise ValueError("`prompt_lookup_num_tokens` is greedy speculative decoding here: it is not supported with "
                             "`do_sample=True` or `num_return_sequences` > 1.")
        # generate's sampling goes through gen_params and Engine.generate(**sample_kw): the chain carries none of its own, no filter
        chain = ChainRequest(speculative_tokens=spec_k, ngram_max=spec_g, ngram_min=1, speculative_sampling=spec_sampling, effective_penalty=float(pen), logprobs=logprobs, presence_penalty=presence, frequency_penalty=frequency,
                             min_new_tokens=min_new, logit_bias=bias, no_repeat_ngram_size=ngram, stop_ids=stop, bad_words_ids=bad)
        guided = None
        if kw.get("guided_regex") is not None or kw.get("guided_choice") is not None:
            guided = self.compile_grammar(kw.get("guided_regex"), kw.get("guided_choice"), kw.get("tokenizer"))
        if spec_k:
            what = chain.speculation_conflict(grammar=guided is not None)
            if what is not None:
                raise ValueError(f"`prompt_lookup_num_tokens` is greedy speculative decoding and cannot be combined with {what}")
        if do_sample and temperature is None:
            temperature = 1.0
        sample_kw = dict(do_sample=bool(do_sample), temperature=float(temperature or 1.0),
                         seed=int(kw.get("seed", getattr(gc, "seed", 0) or 0)), **filt_kw)
        gid = self.engine.grammar_create(guided) if guided is not None else None
        try:
            return self._generate_rows(_Rows(ids_cpu, mask, grids, keys, offs, pixel_values, input_ids), chain, gid, max_new_tokens,
                                       ignore_eos, sample_kw, stop_strings, kw.get("tokenizer"), int(k))
        finally:
            if gid is not None:   # the grammar lives for the call: off the chains, then off the engine
                for slot in range(self.engine.max_seqs):
                    if self.engine.chain_grammar_state(slot)[0] >= 0:
                        self.engine.set_grammar(slot, None)
                self.engine.grammar_destroy(gid)

    @torch.no_grad()
    def beam_search(self, input_ids=None, attention_mask=None, pixel_values=None, image_grid_thw=None, mm_token_type_ids=None,
                    image_keys=None, num_beams: int = 2, max_new_tokens: int = 20, length_penalty: float = 1.0, early_stopping=False,
                    num_return_sequences: int = 1, repetition_penalty=None, return_dict_in_generate: bool = False,
                    output_scores: bool = False, **kw):
        """Beam search on the device (Engine.beam_search; HF's `generate(num_beams=B, do_sample=False)`, which `generate` itself keeps
        refusing).  Takes the inputs of `generate` and returns what it returns: prompt + ids, right-padded, rows (b0 r0, b0 r1, ...,
        b1 r0, ...) for `num_return_sequences` = r per input row -- or, with `return_dict_in_generate`, a BeamSearchOutput with
        `sequences`, `sequences_scores` (with `output_scores`) and `beam_indices`.  Beside the beam parameters only
        `repetition_penalty` and the config's EOS ids apply; any other generation keyword is an error."""
        B, R = num_beams, num_return_sequences
        if isinstance(B, bool) or not isinstance(B, (int, np.integer)) or B < 2:
            raise ValueError(f"`num_beams` has to be an integer strictly greater than 1 for beam search, but is {B}")
        if isinstance(R, bool) or not isinstance(R, (int, np.integer)) or R < 1:
            raise ValueError(f"`num_return_sequences` has to be a strictly positive integer, but is {R}")
        if R > B:
            raise ValueError(f"`num_return_sequences` ({R}) has to be smaller or equal to `num_beams` ({B}).")
        if B > 16:
            raise ValueError(f"`num_beams` is at most 16 on the device, but is {B}")
        if kw.get("do_sample"):
            raise ValueError("beam search is greedy here: `do_sample` with beams is not supported")
        extra = sorted(k for k, v in kw.items() if k != "do_sample" and v is not None)
        if extra:
            raise ValueError(f"beam search takes the beam parameters and `repetition_penalty` only, not {extra}")
        e, cfg = self.engine, self.config
        ids_cpu = input_ids.cpu().numpy()
        mask = attention_mask.cpu().numpy().astype(bool) if attention_mask is not None else np.ones_like(ids_cpu, bool)
        grids = image_grid_thw.cpu().numpy().tolist() if image_grid_thw is not None else []
        keys = list(image_keys) if image_keys is not None else [None] * len(grids)
        offs = np.concatenate([[0], np.cumsum([g[0] * g[1] * g[2] for g in grids])]).astype(int)
        pen = repetition_penalty if repetition_penalty is not None else getattr(self.generation_config, "repetition_penalty", 1.0) or 1.0
        nrows = ids_cpu.shape[0]
        if nrows * B > e.max_seqs:
            raise ValueError(f"{nrows} rows of {B} beams need max_seqs >= {nrows * B} (engine has {e.max_seqs})")
        self._chains.clear()   # every group takes B slots from slot b * B on
        self._next_slot = 0
        # (the decode family stays as it is -- a scheduler may have pinned it, and a change moves the weight generation; an engine
        #  pinned to family 0 refuses more than 64 rows)
        gi, pending = 0, []
        for b in range(nrows):
            ids = ids_cpu[b][mask[b]].astype(np.int64).tolist()
            is_img = np.asarray(ids) == cfg.image_token_id
            n_img = int((is_img & ~np.concatenate([[False], is_img[:-1]])).sum())
            my = list(range(gi, gi + n_img))
            gi += n_img
            if gi > len(grids):
                raise ValueError("Image features and image tokens do not match")
            feats = [self._features(pixel_values[offs[i]:offs[i + 1]], grids[i], keys[i]) for i in my]
            emb = (torch.cat(feats) if len(feats) > 1 else feats[0]) if feats else None
            pos, delta = e.rope_index(ids, [grids[i] for i in my])
            for j in range(B):
                e.seq_reset(b * B + j)
            pending.append((b * B, ids, emb, pos, delta))
        group, rows = [], 0
        for item in pending + [None]:
            if group and (item is None or rows + len(item[1]) > e.max_prefill_rows):
                e.prefill_batch([g[0] for g in group], [g[1] for g in group], [g[2] for g in group], [g[3] for g in group],
                                [g[4] for g in group])
                group, rows = [], 0
            if item is not None:
                group.append(item)
                rows += len(item[1])
        if pen != 1.0:   # (HF's RepetitionPenaltyLogitsProcessor sees the prompt's ids; the marks travel with the fork)
            for slot, ids, _, _, _ in pending:
                e.mark_seen(slot, ids)
        tokens, scores, indices = e.beam_search(list(range(nrows * B)), nrows, B, max_new_tokens, num_return_sequences=R,
                                                length_penalty=length_penalty, early_stopping=early_stopping, repetition_penalty=float(pen))
        outs = [t for g in tokens for t in g]
        width = max(len(t) for t in outs)
        rep = np.repeat(ids_cpu, R, axis=0)
        res = torch.full((rep.shape[0], rep.shape[1] + width), cfg.pad_token_id, dtype=torch.long)
        res[:, : rep.shape[1]] = torch.from_numpy(rep)
        bix = torch.full((rep.shape[0], width), -1, dtype=torch.int32)
        for i, (t, x) in enumerate(zip(outs, (x for g in indices for x in g))):
            res[i, rep.shape[1]: rep.shape[1] + len(t)] = torch.tensor(t, dtype=torch.long)
            bix[i, : len(x)] = torch.tensor(x, dtype=torch.int32)
        if not return_dict_in_generate:
            return res.to(input_ids.device)
        return BeamSearchOutput(sequences=res.to(input_ids.device),
                                sequences_scores=torch.from_numpy(scores.reshape(-1).copy()) if output_scores else None, beam_indices=bix)

    @staticmethod
    def _speculative_sampling_kw(e, slots, chain: ChainRequest, sample_kw) -> dict:
        """What generate_speculative gets of the call's sampling: nothing in greedy mode (today's call); in sampled mode the call's
        do_sample / temperature / seed, behind its top-k / top-p / min-p written to the slots as generate_batch writes them."""
        if not (chain.speculative_sampling and sample_kw.get("do_sample")):
            return {}
        e._apply_filter(slots, sample_kw.get("top_k"), sample_kw.get("top_p"), sample_kw.get("min_p"))
        return dict(do_sample=True, temperature=sample_kw["temperature"], seed=sample_kw["seed"])

    def _generate_rows(self, rows: _Rows, chain: ChainRequest, gid, max_new_tokens, ignore_eos, sample_kw, stop_strings, tokenizer,
                       k: int = 1):
        e, cfg = self.engine, self.config
        ids_cpu, mask, grids, keys, offs, pixel_values, input_ids = rows
        pen, logprobs = chain.effective_penalty, chain.logprobs
        gi = 0
        outs = []
        nrows = ids_cpu.shape[0]
        # k completions per row (num_return_sequences): always the batched path; input row b is prefilled into slot b * k and forked
        # into the k - 1 slots behind it, so the chains sit in the slots -- and draw on the streams -- of the repeated batch
        batched = nrows > 1 or k > 1
        if batched and nrows * k > e.max_seqs:
            raise ValueError(f"batch of {nrows * k} rows needs max_seqs >= {nrows * k} (engine has {e.max_seqs})")
        if batched:  # every row gets its own chain slot; the decode steps then run as one batch
            self._chains.clear()
            self._next_slot = 0
            e.set_decode_regime(-1)  # (a scheduler may have pinned the family to its own capacity)
        spec = chain.speculative_tokens > 0
        if spec:   # the family-0 bursts carry the speculative steps (the row-streaming family has no multi-row kernels)
            if nrows * k > 64:
                raise ValueError("`prompt_lookup_num_tokens` runs on the fragment kernels: at most 64 rows per call")
            e.set_decode_regime(0)
        slots = []
        pending = []
        lps = []
        for b in range(nrows):
            ids = ids_cpu[b][mask[b]].astype(np.int64).tolist()
            is_img = np.asarray(ids) == cfg.image_token_id
            starts = is_img & ~np.concatenate([[False], is_img[:-1]])
            n_img = int(starts.sum())
            my = list(range(gi, gi + n_img))
            gi += n_img
            if gi > len(grids):
                raise ValueError("Image features and image tokens do not match")
            my_grids = [grids[i] for i in my]
            my_keys = [keys[i] for i in my]
            slot, reuse = (b * k, 0) if batched else self._pick_slot(ids, my_keys)
            pre = np.asarray(ids[:reuse]) == cfg.image_token_id
            n_img_reused = int((pre & ~np.concatenate([[False], pre[:-1]])).sum()) if reuse else 0
            feats = [self._features(pixel_values[offs[i]:offs[i + 1]], grids[i], keys[i]) for i in my[n_img_reused:]]
            emb = (torch.cat(feats) if len(feats) > 1 else feats[0]) if feats else None
            pos, delta = e.rope_index(ids, my_grids)
            if not batched:
                self._chains.pop(slot, None)  # re-registered only after its prefill succeeded
            if reuse:
                e.seq_truncate(slot, reuse)  # also clears the chain's seen-set
            else:
                e.seq_reset(slot)
            if batched:  # rows of several chains share every GEMM of the prefill (engine.prefill_batch)
                pending.append((slot, ids[reuse:], emb, pos[:, reuse:], delta, ids))
            else:
                e.prefill(slot, ids[reuse:], emb, pos[:, reuse:], delta, want_logits=False)
                if pen != 1.0:
                    e.mark_seen(slot, ids)
            if not batched:
                self._chains[slot] = (tuple(ids), tuple(my_keys))
                self._chains.move_to_end(slot)
                chain.install(e, slot, ids, gid)  # (the reset / truncate above cleared the slot's previous request)
                if spec:
                    outs.append(e.generate_speculative([slot], max_new_tokens, repetition_penalty=pen, ignore_eos=ignore_eos,
                                                       **self._speculative_sampling_kw(e, [slot], chain, sample_kw))[0])
                else:
                    outs.append(e.generate(slot, max_new_tokens, repetition_penalty=pen, ignore_eos=ignore_eos, **sample_kw))
                if logprobs is not None:
                    lps.append(e.chain_logprobs(slot, max_new_tokens))
            slots.append(slot)
        if batched:
            group, rows = [], 0
            for item in pending + [None]:
                if group and (item is None or rows + len(item[1]) > e.max_prefill_rows):
                    e.prefill_batch([g[0] for g in group], [g[1] for g in group], [g[2] for g in group],
                                    [g[3] for g in group], [g[4] for g in group])
                    group, rows = [], 0
                if item is not None:
                    group.append(item)
                    rows += len(item[1])
            if pen != 1.0:
                for slot, _, _, _, _, ids in pending:
                    e.mark_seen(slot, ids)
            if k > 1:   # the marks travel with the fork; every sibling gets its own request installed, like a row of its own
                for slot, _, _, _, _, ids in list(pending):
                    e.seq_fork(slot, list(range(slot + 1, slot + k)))
                    pending += [(slot + r, None, None, None, None, ids) for r in range(1, k)]
                pending.sort(key=lambda item: item[0])
                slots = [item[0] for item in pending]
            for slot, _, _, _, _, ids in pending:
                chain.install(e, slot, ids, gid)
            if spec:   # rows are budgeted as the engine counts them: 1 + k per chain, 64 in a step
                k_eff = min(chain.speculative_tokens, 64 // len(slots) - 1)
                if k_eff < chain.speculative_tokens:
                    for slot, _, _, _, _, ids in pending:
                        e.set_speculation(slot, k_eff, ids, chain.ngram_min, chain.ngram_max, **(dict(sampled=True) if chain.speculative_sampling else {}))
                outs = e.generate_speculative(slots, max_new_tokens, repetition_penalty=pen, ignore_eos=ignore_eos,
                                              **self._speculative_sampling_kw(e, slots, chain, sample_kw))
            else:
                outs = e.generate_batch(slots, max_new_tokens, repetition_penalty=pen, ignore_eos=ignore_eos, **sample_kw)
            if logprobs is not None:
                lps = e.chain_logprobs_batch(slots, logprobs, max_new_tokens)
        if chain.stop_ids or stop_strings:
            # what follows a stop is pad (HF's finished rows): the ids behind a matched stop sequence are the device's own pads;
            # a stop string is exact at text level, whatever tokenization carried it (hostloop.first_stop_cut)
            from .hostloop import first_stop_cut, first_stop_hit
            min_new = chain.min_new_tokens
            for b, t in enumerate(outs):
                cuts = [first_stop_hit(t, chain.stop_ids, min_new)]
                hit = first_stop_cut(tokenizer, t, stop_strings, min_new) if stop_strings else None
                cuts.append(hit[0] if hit else None)
                cuts = [n for n in cuts if n is not None]
                if cuts:
                    outs[b] = list(t[:min(cuts)])
        width = max(len(t) for t in outs)
        pad = cfg.pad_token_id
        if k > 1:   # (HF's expand_inputs_for_generation: every input row k times, in place)
            ids_cpu, nrows = np.repeat(ids_cpu, k, axis=0), nrows * k
        res = torch.full((ids_cpu.shape[0], ids_cpu.shape[1] + width), pad, dtype=torch.long)
        res[:, : ids_cpu.shape[1]] = torch.from_numpy(ids_cpu)
        for b, t in enumerate(outs):
            res[b, ids_cpu.shape[1]: ids_cpu.shape[1] + len(t)] = torch.tensor(t, dtype=torch.long)
        if logprobs is None:
            return res.to(input_ids.device)
        out = GenerateOutput(sequences=res.to(input_ids.device), logprobs=torch.zeros((nrows, width), dtype=torch.float32),
                             top_ids=torch.full((nrows, width, logprobs), -1, dtype=torch.int32),
                             top_logprobs=torch.full((nrows, width, logprobs), float("-inf"), dtype=torch.float32))
        for b, (lp, ids, tlp) in enumerate(lps):
            n = min(len(outs[b]), len(lp))
            out.logprobs[b, :n] = torch.from_numpy(lp[:n])
            out.top_ids[b, :n] = torch.from_numpy(ids[:n, :logprobs])
            out.top_logprobs[b, :n] = torch.from_numpy(tlp[:n, :logprobs])
        return out

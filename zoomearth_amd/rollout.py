"""Two-stage rollout driver: the generation half of one GRPO step of the reference, on the continuous-batching scheduler.

replaces: the rollout section of `Qwen2VLGRPOTrainer._generate_and_score_completions`
(/root/reference/src/train/RL/src/open-r1-multimodal/src/open_r1/trainer/grpo_trainer.py:561-683): the trainer's sampler
repeats every prompt G = num_generations times; stage 1 is one sampled `generate` over that batch; then, ONE SAMPLE AT A
TIME (`customized_funcs.chat`, :617), the first box of the completion (the whole view when none parses, :604-607) is
scaled by `max(max(w, h) / 512, 1)` to tile pixels, cut (>= 512 px window) and resized to <= 512 px, and stage 2
generates on `stage_1_prompt + completion.split("<answer>")[0] + <vision block>` with [view, crop]; samples whose
`bbox` field is empty skip stage 2 (:634-640).  The old-policy / reference-model log-probabilities are then computed on
the final prompt + completion ids from the stage-1 prompt length on (`_get_per_token_logps(...)[:, prompt_length - 1:]`,
:660-683).

Here all G x len(samples) chains advance together (sampled decoding at a temperature, one random stream per chain:
`seed`, stream = sample * G + g for stage 1 and the same + G * len(samples) for stage 2; the G generations of a sample are one
`Request(n=G)`: one prefill, forked on the device), stage 2 continues on the chain
slot of stage 1 with the cached stage-1 prompt reused, and scoring runs through `ze_score_batch` (`model.score_sequences`: all
rollouts in one planned call, scored from the stage-1 prompt's end, the generations of a sample sharing its rows).
The gradient side of the step is out of scope.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

from . import hostloop as H
from .scheduler import ChainScheduler, Request


@dataclass
class Rollout:
    sample: int                      # index into `samples`
    generation: int                  # 0 .. G-1
    prompt1: str
    completion1: str = ""
    completion1_ids: List[int] = field(default_factory=list)
    prompt2: Optional[str] = None    # None: the sample has no box to zoom into (stage 2 skipped)
    completion2: str = ""
    completion2_ids: List[int] = field(default_factory=list)
    bbox: Optional[list] = None      # box in tile pixels actually cut (None when stage 2 was skipped)
    scale: float = 1.0
    n_prompt1: int = 0               # stage-1 prompt length in tokens
    images: list = field(default_factory=list)   # images of the FINAL prompt, in order
    logps: Optional[object] = None   # f32 tensor: log p of every token of the final sequence from position n_prompt1 on
    entropies: Optional[object] = None   # f32 tensor aligned with logps: the policy's entropy at those positions (entropies=True)
    ref_logps: Optional[object] = None   # f32 tensor aligned with logps: the same positions under the base weights (ref_logps=True)
    # sampled_logps: the decode-time log-probability of every sampled id of the stage (the policy's own `old_per_token_logps` of
    # the completion positions, grpo_trainer.py:660-683), from the step that drew it -- no extra pass
    completion1_logps: List[float] = field(default_factory=list)
    completion2_logps: List[float] = field(default_factory=list)
    error: Optional[str] = None


def rollout_two_stage(model, processor, samples, num_generations: int = 4, temperature: float = 0.7,
                      max_new_tokens: int = 800, seed: int = 0, max_view: int = 512, with_logps: bool = True,
                      burst: int = 8, top_k: Optional[int] = None, top_p: Optional[float] = None,
                      min_p: Optional[float] = None, sampled_logps: bool = False, entropies: bool = False,
                      prefix_cache=None, ref_logps: bool = False, typical_p: Optional[float] = None,
                      epsilon_cutoff: Optional[float] = None, eta_cutoff: Optional[float] = None) -> List[Rollout]:
    """samples: dicts with `prompt` (the stage-1 prompt text, one `<|vision_start|><|image_pad|><|vision_end|>` block),
    `image` (the tile: DeviceImage or PIL) and `bbox` (the dataset's reference box; empty = non-cropping question).
    top_k / top_p / min_p: the sampling filters of the reference's generation step (GRPOConfig top_k / top_p / min_p,
    open_r1/trainer/grpo_config.py:62-70), applied to every chain of both stages; None = off.
    typical_p / epsilon_cutoff / eta_cutoff: HF's entropy-adaptive cutoffs of a generation_config, behind the three above on every
    chain of both stages; None (or 1.0 / 0.0 / 0.0) = off.
    sampled_logps: fill completion1_logps / completion2_logps with the log-probabilities the decode steps computed for their own
    samples (the model's distribution, before temperature and filters); independent of with_logps, which scores the final
    sequences with batched passes of their own.
    entropies: with with_logps, fill Rollout.entropies from the same planned scoring call (no further pass).
    prefix_cache: a PrefixCache of the model's engine (zoomearth_amd/prefix_cache.py) that the caller keeps between calls: the rows
    of the chains of one call stay in its pool, and the next call on the same samples prefills only what it does not hold (the
    trainer's `enable_prefix_caching=True`); a weight refresh between the calls empties it.
    ref_logps: with with_logps and a LoRA adapter active, one more planned scoring call runs under `model.disable_adapter()` and
    fills Rollout.ref_logps -- the reference-policy log-probabilities of the KL term, which the reference's trainer gets from the
    same model with the adapter disabled (grpo_trainer.py:672-684).  With no adapter active it raises: the reference policy would
    be the policy itself.
    Returns len(samples) * num_generations rollouts, sample-major."""
    if ref_logps and model.active_adapter is None:
        raise ValueError("ref_logps=True needs an active LoRA adapter: without one the reference policy is the policy itself")
    if ref_logps and not with_logps:
        raise ValueError("ref_logps=True needs with_logps=True")
    sched = ChainScheduler(model, processor, do_sample=True, temperature=temperature, seed=seed, burst=burst,
                           top_k=top_k, top_p=top_p, min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff,
                           eta_cutoff=eta_cutoff, logprobs=0 if sampled_logps else None,
                           **({} if prefix_cache is None else {"prefix_cache": prefix_cache}))
    n, G = len(samples), int(num_generations)
    out = [Rollout(sample=i, generation=g, prompt1=samples[i]["prompt"]) for i in range(n) for g in range(G)]
    views = {}
    for i, s in enumerate(samples):
        img = s["image"]
        view = H.resize_image_demo(img, max_view)             # customized_funcs.resize_image: <= 512 px, image only
        views[i] = (img, view, max(max(img.width, img.height) / max_view, 1))

    def fail(ro):
        def on_error(req, ex):
            ro.error = f"{type(ex).__name__}: {ex}"
        return on_error

    def stage1_done(ro):
        def done(req, tokens, text):
            ro.completion1, ro.completion1_ids, ro.n_prompt1 = text, list(tokens), req.n_prompt
            ro.completion1_logps = list(req.token_logprobs)
            img, view, scale = views[ro.sample]
            ro.images = [view]
            if not samples[ro.sample].get("bbox"):             # non-cropping question: the chain ends here
                return None
            boxes = H.extract_bbox(text, 1)
            # no parsable box -> the whole view (:604-607); a box that is not four numbers (which crashes the reference in
            # cut_image) is treated the same way
            box = boxes[0] if boxes and len(boxes[0]) == 4 else [0, 0, view.width, view.height]
            ro.scale = scale
            ro.bbox = [p * scale for p in box]
            crop = H.resize_image_demo(H.cut_image(img, ro.bbox), max_view)
            ro.prompt2 = H.stage2_prompt(ro.prompt1, text)
            ro.images = [view, crop]

            def done2(req2, tokens2, text2):
                ro.completion2, ro.completion2_ids = text2, list(tokens2)
                ro.completion2_logps = list(req2.token_logprobs)
                return None
            return Request(prompt=ro.prompt2, images=[view, crop], max_new_tokens=max_new_tokens,
                           stream_id=n * G + ro.sample * G + ro.generation, on_done=done2, on_error=fail(ro))
        return done

    # stage 1: ONE request per sample with n = G completions (Request.n): the prompt is prefilled once and forked on the device,
    # completion g draws on stream sample * G + g.  (More generations than the engine has chain slots go in several such requests.)
    cap = sched.engine.max_seqs
    for i in range(n):
        for g0 in range(0, G, cap):
            group = out[i * G + g0: i * G + min(g0 + cap, G)]

            def done(req, tokens, text, group=group):
                return stage1_done(group[req.index])(req, tokens, text)

            def failed(req, ex, group=group):
                fail(group[req.index])(req, ex)
            sched.submit(Request(prompt=samples[i]["prompt"], images=[views[i][1]], max_new_tokens=max_new_tokens,
                                 stream_id=i * G + g0, n=len(group), on_done=done, on_error=failed))
    sched.run()

    if with_logps:
        from .modeling import ScoreItem
        scored, items, pixel_rows = [], [], []
        for ro in out:
            if ro.error:
                continue
            # the final sequence as the trainer scores it: prompt ids re-tokenised from the final prompt text, then the
            # generated ids of the last stage
            prompt = ro.prompt2 if ro.prompt2 is not None else ro.prompt1
            tail = ro.completion2_ids if ro.prompt2 is not None else ro.completion1_ids
            inp = processor(text=[prompt], images=list(ro.images), return_tensors="pt")
            ids = inp["input_ids"][0].tolist() + [int(t) for t in tail]
            grids = inp["image_grid_thw"].tolist()
            keys = list(inp.get("image_keys") or [None] * len(grids))
            offs = [0]
            for g in grids:
                offs.append(offs[-1] + g[0] * g[1] * g[2])
            feats = [model._features(inp["pixel_values"][offs[i]:offs[i + 1]], grids[i], keys[i]) for i in range(len(grids))]
            if ref_logps:
                pixel_rows.append([inp["pixel_values"][offs[i]:offs[i + 1]] for i in range(len(grids))])
            scored.append(ro)
            items.append(ScoreItem(ids, grids, feats, keys, min(max(ro.n_prompt1 - 1, 0), max(len(ids) - 1, 0))))
        # ONE planned call for all rollouts: many sequences per pass, the G generations of a sample share their stage-1 prompt's
        # rows, and only the positions from the stage-1 prompt's end on go through the lm_head (model.score_sequences)
        if entropies:
            for ro, d in zip(scored, model.score_sequences(items, entropy=True)):
                ro.logps, ro.entropies = d.logps.cpu(), d.entropy.cpu()
        else:
            for ro, lp in zip(scored, model.score_sequences(items)):
                ro.logps = lp.cpu()
        if ref_logps:
            with model.disable_adapter():
                # (the items' ViT features come from the adapter's vision tower: recomputed under the base weights)
                base_items = [it._replace(feats=[model._features(pv, g, k) for pv, g, k in zip(pvs, it.grids, it.keys)])
                              for it, pvs in zip(items, pixel_rows)]
                for ro, lp in zip(scored, model.score_sequences(base_items)):
                    ro.ref_logps = lp.cpu()
    return out

"""OpenAI-compatible chat-completions shim over the engine, so the reference's `src/eval/infer_vllm.py` client
(`OpenAI(base_url="http://localhost:8000/v1").chat.completions.create(model=..., messages=[...])`,
/root/reference/src/eval/infer_vllm.py:19-24,153-156,218-221) can target this engine instead of `vllm serve`
(SURVEY.md 8f rank 3).

Request: the subset that client sends -- `messages` with `role` in {system, user, assistant} and `content` either a
string or a list of `{"type": "text", "text": ...}` / `{"type": "image_url", "image_url": {"url": "data:image/...;
base64,..."}}` items, plus `max_tokens`, `temperature`, `seed`, `top_p` and the vLLM extensions `top_k` (-1 / 0 = off) and
`min_p` (`stream` is not offered); the three filters apply to sampled requests, each request its own.  So do HF's `typical_p`,
`epsilon_cutoff` and `eta_cutoff` (in (0, 1); 1.0 / 0.0 / 0.0 = off; anything else is a 400), behind the three on the device.
`n` in [1, 16]: that many completions of the prompt, sampled requests only (n > 1 at temperature 0 / absent is a 400, vLLM's rule).
vLLM's `use_beam_search: true`: beam search on the device (`model.beam_search`) with `n` (2 .. 16) as the beam width AND the number
of choices, best first, and `length_penalty` (default 1.0); `repetition_penalty` applies; together with `temperature > 0`,
`logprobs` / `prompt_logprobs`, the guided fields or any logit adjustment / stop field it is a 400.  It runs while no other request's
chain is alive (it takes the engine's first n slots); requests that arrive behind it wait for it.
The prompt is prefilled once and forked on the device (`ze_seq_fork`); the response carries `n` choices with `index` 0 .. n-1, each
with its own `finish_reason`, `logprobs` and stop-string cut; choice i draws from random stream i of the request's `seed` (choice 0
is what n = 1 returns); `usage.completion_tokens` sums the choices, `prompt_tokens` counts once, `prompt_logprobs` appears once.
vLLM's `repetition_penalty` (finite, > 0; absent = the checkpoint's generation_config) is per request too.
`presence_penalty` / `frequency_penalty` ([-2, 2]), `logit_bias` (at most 300 `"id": bias` entries in [-100, 100]) and vLLM's
`min_tokens` adjust every step's logits on the device, each request its own values, greedy requests included.
`stop` (a string or up to 4 strings), vLLM's `stop_token_ids` and `no_repeat_ngram_size` are token rules on the device: the chain
ends in the step that completes a stop sequence (`finish_reason: "stop"`); the text is cut before a stop string, a stop token id
is kept as an EOS is.
vLLM's top-level `guided_regex` (a pattern) and `guided_choice` (a list of strings; not both) hold the reply to a format: a token
automaton on the device masks every step (`zoomearth_amd/grammar.py`); a pattern that does not compile is a 400.
`logprobs: true` (with `top_logprobs: 0..20`) adds `choices[0].logprobs.content`, one entry per completion token, from the
decode step's own logits (the model's distribution, before repetition penalty, temperature and filters).
vLLM's top-level `prompt_logprobs: 0..20` adds a top-level `prompt_logprobs` list: null for the first prompt token, then per token
`{id: {logprob, rank, decoded_token}}` for the token itself and that many best alternatives, from the request's own prefill pass
(`ze_score_batch_detail`).
Prompt: the Qwen2.5-VL chat template (`<|im_start|>role\\n ... <|im_end|>\\n`, an image item becomes
`<|vision_start|><|image_pad|><|vision_end|>`, a default system turn when the conversation has none, then the
generation prompt `<|im_start|>assistant\\n`).  temperature 0 / absent -> greedy, else temperature sampling.
Concurrent requests (infer_vllm.py keeps up to 100 in flight, :244-271) share the GPU through continuous batching
(`zoomearth_amd/scheduler.py`): a dispatcher thread admits every request, greedy or sampled, into the RUNNING batch between
bursts of decode steps -- newcomers are prefilled together and join the next burst, a finished request frees its KV slot and
its response returns at once.  Temperature, seed and repetition penalty are per chain on the device (`Engine.set_sampling`), so
a request's tokens do not depend on which other requests share its steps.  Images are decoded on the host and uploaded.

    python -m zoomearth_amd.serve --model_name /ckpt/ZoomEarth-3B --port 8000
"""

import base64
import io
import math
import threading
import time
import uuid
from dataclasses import dataclass, field
from typing import Any, Optional

DEFAULT_SYSTEM = "You are a helpful assistant."
MAX_N = 16   # completions per request (`n`)
IMAGE_PLACEHOLDER = "<|vision_start|><|image_pad|><|vision_end|>"


class BadRequest(ValueError):
    pass


def decode_data_url(url: str):
    """data:image/...;base64,<payload> -> PIL RGB image (what infer_vllm.py's encode_pil_image_to_data_url produces)."""
    from PIL import Image

    if not isinstance(url, str) or not url.startswith("data:") or ";base64," not in url:
        raise BadRequest("only base64 data URLs are accepted for image_url (no network access from the server)")
    try:
        raw = base64.b64decode(url.split(";base64,", 1)[1], validate=False)
        Image.MAX_IMAGE_PIXELS = None
        return Image.open(io.BytesIO(raw)).convert("RGB")
    except Exception as ex:
        raise BadRequest(f"cannot decode image: {ex}") from ex


def build_prompt(messages):
    """Qwen2.5-VL chat template over OpenAI messages -> (prompt string, [PIL images in prompt order])."""
    if not isinstance(messages, list) or not messages:
        raise BadRequest("messages must be a non-empty list")
    parts, images = [], []
    if messages[0].get("role") != "system":
        parts.append(f"<|im_start|>system\n{DEFAULT_SYSTEM}<|im_end|>\n")
    for m in messages:
        role = m.get("role")
        if role not in ("system", "user", "assistant"):
            raise BadRequest(f"unsupported role {role!r}")
        content = m.get("content")
        body = []
        if isinstance(content, str):
            body.append(content)
        elif isinstance(content, list):
            for item in content:
                kind = item.get("type") if isinstance(item, dict) else None
                if kind == "text":
                    body.append(str(item.get("text", "")))
                elif kind == "image_url":
                    iu = item.get("image_url")
                    images.append(decode_data_url(iu.get("url") if isinstance(iu, dict) else iu))
                    body.append(IMAGE_PLACEHOLDER)
                else:
                    raise BadRequest(f"unsupported content item type {kind!r}")
        else:
            raise BadRequest("message content must be a string or a list of items")
        parts.append(f"<|im_start|>{role}\n{''.join(body)}<|im_end|>\n")
    parts.append("<|im_start|>assistant\n")
    return "".join(parts), images


@dataclass
class _Parsed:
    """One validated request: OpenAI's / vLLM's fields under their own names, off values where the request names none."""
    req: dict
    prompt: str = ""
    pil_images: list = field(default_factory=list)
    max_tokens: int = 1024
    sample: bool = False
    temperature: Optional[float] = None
    seed: int = 0
    repetition_penalty: Optional[float] = None
    top_k: int = 0
    top_p: float = 1.0
    min_p: float = 0.0
    typical_p: float = 1.0
    epsilon_cutoff: float = 0.0
    eta_cutoff: float = 0.0
    logprobs: Optional[int] = None
    prompt_logprobs: Optional[int] = None
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    logit_bias: dict = field(default_factory=dict)
    min_tokens: int = 0
    stop: list = field(default_factory=list)
    stop_token_ids: list = field(default_factory=list)
    no_repeat_ngram_size: int = 0
    guided_regex: Optional[str] = None
    guided_choice: Optional[list] = None
    n: int = 1
    use_beam_search: bool = False
    length_penalty: float = 1.0
    future: Any = None

    def guided(self) -> bool:
        return self.guided_regex is not None or self.guided_choice is not None

    def rules(self) -> bool:
        return bool(self.stop or self.stop_token_ids or self.no_repeat_ngram_size)

    def entropy_kw(self) -> dict:
        """typical_p / epsilon_cutoff / eta_cutoff for generate() or a scheduler Request: the ones that are on."""
        return {k: v for k, v, off in (("typical_p", self.typical_p, 1.0), ("epsilon_cutoff", self.epsilon_cutoff, 0.0),
                                       ("eta_cutoff", self.eta_cutoff, 0.0)) if v != off}

    def adjusts(self) -> bool:
        """The request carries values generate() gives every row of a call alike: it runs alone, or through the dispatcher."""
        return bool(self.presence_penalty or self.frequency_penalty or self.logit_bias or self.min_tokens) or self.rules() or self.guided()

    def adjust_kw(self, tokenizer=None) -> dict:
        """generate()'s keyword arguments of the request's logit adjustments and token rules (none when they are all off)."""
        kw = dict(presence_penalty=self.presence_penalty, frequency_penalty=self.frequency_penalty, logit_bias=self.logit_bias,
                  min_new_tokens=self.min_tokens) if self.adjusts() else {}
        if self.guided():
            kw.update(guided_regex=self.guided_regex, guided_choice=self.guided_choice, tokenizer=tokenizer)
        if self.rules():
            kw.update(stop_strings=list(self.stop) or None, tokenizer=tokenizer, stop_token_ids=list(self.stop_token_ids) or None,
                      no_repeat_ngram_size=self.no_repeat_ngram_size or None)
        return kw

    def stop_records(self, tokenizer) -> list:
        """What the device finishes the chain on: the stop token ids, and the tokenizer's own encoding of every stop string."""
        from .engine import MAX_RULE_LEN
        from .hostloop import stop_string_records
        return [[t] for t in self.stop_token_ids] + [r for r in stop_string_records(tokenizer, self.stop) if len(r) <= MAX_RULE_LEN]


class ChatServer:
    """Holds the model / processor pair; turns OpenAI request dicts into response dicts, one at a time
    (`complete`), as an explicit batch (`complete_many`) or through the batching dispatcher (`submit`)."""

    def __init__(self, model, processor, model_id: str = "ZoomEarth", batch_window_s: float = 0.01, max_batch=None,
                 prefix_cache_rows: int = 0, speculative_ngram: int = 0, speculative_sampling: bool = False):
        self.model, self.processor, self.model_id = model, processor, model_id
        # --speculative-ngram K: greedy requests without log-probabilities, adjustments, rules or a grammar draft up to K ids per
        # step by prompt lookup (vLLM's ngram method; ChainScheduler(speculative_tokens=)); lossless.  0: off, today's steps.
        self.speculative_ngram = int(speculative_ngram or 0)
        # --speculative-sampling: sampled requests (temperature, seed, top_p) speculate too, in the sampled mode
        # (ChainScheduler(speculative_sampling=True)): every row draws what a plain step draws.  Off: they ride with one row.
        self.speculative_sampling = bool(speculative_sampling)
        # --prefix-cache-rows N: the K/V rows of finished requests stay in a pool of N rows (zoomearth_amd/prefix_cache.py), and a
        # later request whose prompt starts with them -- stage 2 of a question, the next question of a tile -- prefills only its
        # tail; `usage.prompt_tokens_details.cached_tokens` reports the rows it did not compute.  0: no pool, today's responses.
        self.prefix_cache_rows, self.prefix_cache = int(prefix_cache_rows), None
        self._lock = threading.Lock()  # the engine is single-stream
        self.batch_window_s = batch_window_s
        self.max_batch = int(max_batch or getattr(model.engine, "max_seqs", 1))
        self._queue = []
        self._cv = threading.Condition()
        self._worker = None
        self._stop = False
        self.scheduler = None  # the dispatcher's ChainScheduler (stats for tests / monitoring)

    # ------------------------------------------------------------------ request -> response pieces
    def _parse(self, req: dict) -> _Parsed:
        if req.get("stream"):
            raise BadRequest("stream=true is not offered")
        n = req.get("n")
        if n is not None and (isinstance(n, bool) or not isinstance(n, int)):
            raise BadRequest(f"n must be an integer, got {n!r}")
        if n is not None and not (1 <= n <= MAX_N):
            raise BadRequest(f"n must be in [1, {MAX_N}], got {n}")
        p = _Parsed(req)
        p.n = int(n or 1)
        p.prompt, p.pil_images = build_prompt(req.get("messages"))
        p.max_tokens = int(req.get("max_tokens") or req.get("max_completion_tokens") or 1024)
        t = req.get("temperature")
        p.sample = t is not None and float(t) > 0.0
        p.temperature = float(t) if p.sample else None
        if p.n > self.max_batch:
            raise BadRequest(f"n = {p.n} exceeds the engine's {self.max_batch} chain slots")
        # vLLM's `use_beam_search`: `n` is the beam width AND the number of choices, `length_penalty` HF's; greedy only
        ub = req.get("use_beam_search")
        if ub is not None and not isinstance(ub, bool):
            raise BadRequest(f"use_beam_search must be a boolean, got {ub!r}")
        p.use_beam_search = bool(ub)
        if p.use_beam_search:
            if p.sample:
                raise BadRequest("use_beam_search is greedy: it cannot be combined with temperature > 0")
            if p.n < 2:
                raise BadRequest("use_beam_search needs n >= 2: n is the beam width and the number of choices")
            lpen = req.get("length_penalty")
            if lpen is not None and (isinstance(lpen, bool) or not isinstance(lpen, (int, float)) or not math.isfinite(float(lpen))):
                raise BadRequest(f"length_penalty must be a finite number, got {lpen!r}")
            p.length_penalty = 1.0 if lpen is None else float(lpen)
        elif req.get("length_penalty") is not None:
            raise BadRequest("length_penalty needs use_beam_search = true")
        if p.n > 1 and not p.sample and not p.use_beam_search:
            raise BadRequest(f"n = {p.n} needs temperature > 0: greedy completions would all be the same")
        p.seed = int(req.get("seed") or 0)
        # vLLM's `repetition_penalty`: None = the model's own (generation_config)
        rp = req.get("repetition_penalty")
        if rp is not None:
            if isinstance(rp, bool) or not isinstance(rp, (int, float)):
                raise BadRequest(f"repetition_penalty must be a number, got {rp!r}")
            rp = float(rp)
            if not (math.isfinite(rp) and rp > 0.0):
                raise BadRequest(f"repetition_penalty must be finite and > 0, got {rp}")
        p.repetition_penalty = rp
        # sampling filters (OpenAI `top_p`; vLLM's `top_k`, -1 = off, and `min_p`): 0 / 1.0 / 0.0 = off
        try:
            p.top_p = 1.0 if req.get("top_p") is None else float(req["top_p"])
            p.top_k = 0 if req.get("top_k") is None else int(req["top_k"])
            p.min_p = 0.0 if req.get("min_p") is None else float(req["min_p"])
        except (TypeError, ValueError) as ex:
            raise BadRequest(f"top_p / top_k / min_p must be numbers: {ex}") from ex
        if not (0.0 < p.top_p <= 1.0):
            raise BadRequest(f"top_p must be in (0, 1], got {p.top_p}")
        if p.top_k < -1:
            raise BadRequest(f"top_k must be -1 (off) or >= 0, got {p.top_k}")
        if not (0.0 <= p.min_p <= 1.0):
            raise BadRequest(f"min_p must be in [0, 1], got {p.min_p}")
        p.top_k = max(p.top_k, 0)
        # HF's entropy-adaptive cutoffs under HF's names (vLLM's `typical_p` too): 1.0 / 0.0 / 0.0 = off
        for name, off in (("typical_p", 1.0), ("epsilon_cutoff", 0.0), ("eta_cutoff", 0.0)):
            v = req.get(name)
            if v is None:
                continue
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise BadRequest(f"{name} must be a number, got {v!r}")
            if float(v) != off and not (0.0 < float(v) < 1.0):
                raise BadRequest(f"{name} must be in (0, 1) or {off} (off), got {v}")
            setattr(p, name, float(v))
        # OpenAI's `logprobs` (bool) and `top_logprobs` (0 .. 20, only with logprobs): None = no block in the response
        lp, top = req.get("logprobs"), req.get("top_logprobs")
        if lp is not None and not isinstance(lp, bool):
            raise BadRequest(f"logprobs must be a boolean, got {lp!r}")
        if top is not None:
            if isinstance(top, bool) or not isinstance(top, int):
                raise BadRequest(f"top_logprobs must be an integer, got {top!r}")
            if not lp:
                raise BadRequest("top_logprobs needs logprobs = true")
            if not (0 <= top <= 20):
                raise BadRequest(f"top_logprobs must be in [0, 20], got {top}")
        p.logprobs = (int(top or 0) if lp else None)
        # vLLM's `prompt_logprobs` (0 .. 20): None = no list in the response
        plp = req.get("prompt_logprobs")
        if plp is not None:
            if isinstance(plp, bool) or not isinstance(plp, int):
                raise BadRequest(f"prompt_logprobs must be an integer, got {plp!r}")
            if not (0 <= plp <= 20):
                raise BadRequest(f"prompt_logprobs must be in [0, 20], got {plp}")
            p.prompt_logprobs = int(plp)
        # OpenAI's `presence_penalty` / `frequency_penalty` ([-2, 2]) and `logit_bias` ({"id": bias in [-100, 100]}, at most 300
        # entries), vLLM's `min_tokens`: applied on the device to every step's logits, greedy requests included
        for name in ("presence_penalty", "frequency_penalty"):
            v = req.get(name)
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float))):
                raise BadRequest(f"{name} must be a number, got {v!r}")
            v = 0.0 if v is None else float(v)
            if not (-2.0 <= v <= 2.0):
                raise BadRequest(f"{name} must be in [-2, 2], got {v}")
            setattr(p, name, v)
        lb = req.get("logit_bias")
        p.logit_bias = {}
        if lb is not None:
            if not isinstance(lb, dict):
                raise BadRequest(f"logit_bias must be an object of token id -> bias, got {lb!r}")
            if len(lb) > 300:
                raise BadRequest(f"logit_bias must have at most 300 entries, got {len(lb)}")
            vocab = int(self.model.config.text.vocab_size)
            for k, v in lb.items():
                try:
                    tid = int(k)
                except (TypeError, ValueError) as ex:
                    raise BadRequest(f"logit_bias keys must be token ids, got {k!r}") from ex
                if not (0 <= tid < vocab):
                    raise BadRequest(f"logit_bias token id must be in [0, {vocab}), got {tid}")
                if isinstance(v, bool) or not isinstance(v, (int, float)):
                    raise BadRequest(f"logit_bias values must be numbers, got {v!r}")
                if not (-100.0 <= float(v) <= 100.0):
                    raise BadRequest(f"logit_bias values must be in [-100, 100], got {v}")
                if tid in p.logit_bias:
                    raise BadRequest(f"logit_bias names token id {tid} twice")
                p.logit_bias[tid] = float(v)
        mt = req.get("min_tokens")
        if mt is not None and (isinstance(mt, bool) or not isinstance(mt, int)):
            raise BadRequest(f"min_tokens must be an integer, got {mt!r}")
        if mt is not None and mt < 0:
            raise BadRequest(f"min_tokens must be >= 0, got {mt}")
        p.min_tokens = int(mt or 0)
        # OpenAI's `stop` (a string or up to 4 strings), vLLM's `stop_token_ids`, HF's `no_repeat_ngram_size`: token rules on the device
        st = req.get("stop")
        if st is None:
            st = []
        elif isinstance(st, str):
            st = [st]
        if not isinstance(st, list) or any(not isinstance(x, str) for x in st):
            raise BadRequest(f"stop must be a string or a list of strings, got {req.get('stop')!r}")
        if len(st) > 4:
            raise BadRequest(f"stop must have at most 4 strings, got {len(st)}")
        if any(x == "" for x in st):
            raise BadRequest("stop strings must not be empty")
        p.stop = st
        sti = req.get("stop_token_ids")
        if sti is None:
            sti = []
        if not isinstance(sti, list) or any(isinstance(t, bool) or not isinstance(t, int) for t in sti):
            raise BadRequest(f"stop_token_ids must be a list of integers, got {req.get('stop_token_ids')!r}")
        if sti:
            vocab = int(self.model.config.text.vocab_size)
            if any(not (0 <= t < vocab) for t in sti):
                raise BadRequest(f"stop_token_ids must be in [0, {vocab}), got {sti}")
        if len(sti) > 32:
            raise BadRequest(f"stop_token_ids must have at most 32 entries, got {len(sti)}")
        p.stop_token_ids = [int(t) for t in sti]
        ng = req.get("no_repeat_ngram_size")
        if ng is not None and (isinstance(ng, bool) or not isinstance(ng, int)):
            raise BadRequest(f"no_repeat_ngram_size must be an integer, got {ng!r}")
        if ng is not None and not (0 <= ng <= 16):
            raise BadRequest(f"no_repeat_ngram_size must be in [0, 16], got {ng}")
        p.no_repeat_ngram_size = int(ng or 0)
        # vLLM's `guided_regex` (a pattern) / `guided_choice` (a list of strings): a token automaton on the device holds the chain to
        # it (zoomearth_amd/grammar.py).  Compiled here, so that a pattern that does not compile is a 400 before anything is queued.
        gr, gc = req.get("guided_regex"), req.get("guided_choice")
        if gr is not None and gc is not None:
            raise BadRequest("guided_regex and guided_choice exclude each other")
        if gr is not None and not isinstance(gr, str):
            raise BadRequest(f"guided_regex must be a string, got {gr!r}")
        if gc is not None and (not isinstance(gc, list) or not gc or any(not isinstance(x, str) or not x for x in gc)):
            raise BadRequest(f"guided_choice must be a non-empty list of non-empty strings, got {gc!r}")
        if gr is not None or gc is not None:
            try:
                self.model.compile_grammar(guided_regex=gr, guided_choice=gc, tokenizer=self.processor.tokenizer)
            except ValueError as ex:
                raise BadRequest(f"guided decoding: {ex}") from ex
        p.guided_regex, p.guided_choice = gr, gc
        if p.use_beam_search:   # the beam step serves the repetition penalty and the EOS ids only (ze_beam_search refuses the rest)
            if p.logprobs is not None or p.prompt_logprobs is not None:
                raise BadRequest("use_beam_search cannot be combined with logprobs / prompt_logprobs")
            if p.guided():
                raise BadRequest("use_beam_search cannot be combined with guided_regex / guided_choice")
            if p.adjusts():
                raise BadRequest("use_beam_search cannot be combined with presence_penalty / frequency_penalty / logit_bias / min_tokens / "
                                 "stop / stop_token_ids / no_repeat_ngram_size")
        return p

    def _logprobs_block(self, p: _Parsed, ids, lp) -> dict:
        """OpenAI's `choices[0].logprobs`: lp = (log-probability per token, [(id, logprob), ...] best first per token)."""
        tok = self.processor.tokenizer

        def entry(i, v):
            s = tok.decode([int(i)], skip_special_tokens=False)
            return {"token": s, "logprob": float(v), "bytes": list(s.encode("utf-8"))}

        content = []
        for t, i in enumerate(ids):
            item = entry(i, lp[0][t])
            item["top_logprobs"] = [entry(j, v) for j, v in lp[1][t][: p.logprobs]]
            content.append(item)
        return {"content": content}

    def _prompt_logprobs_list(self, p: _Parsed, ids, plp) -> list:
        """vLLM's `prompt_logprobs`: null for the first prompt token (and wherever the position was not scored), then per token
        {id: {logprob, rank (1-based), decoded_token}} for the token itself and the N best alternatives at its place.
        plp = (log-probability, 0-based rank, [(id, logprob), ...] best first) per prompt position."""
        tok = self.processor.tokenizer

        def entry(i, v, rank):
            return {"logprob": float(v), "rank": int(rank), "decoded_token": tok.decode([int(i)], skip_special_tokens=False)}

        out = []
        for t, i in enumerate(ids):
            if t >= len(plp[0]) or plp[0][t] is None:
                out.append(None)
                continue
            item = {str(int(i)): entry(i, plp[0][t], plp[1][t] + 1)}
            for place, (j, v) in enumerate((plp[2][t] or [])[: p.prompt_logprobs]):
                item.setdefault(str(int(j)), entry(j, v, place + 1))
            out.append(item)
        return out

    def _response(self, p: _Parsed, out, n_in: int, lp=None, prompt=None) -> dict:
        eos = set(self.model.config.eos_token_ids)
        pad = self.model.config.pad_token_id
        out = out[: p.max_tokens]
        stop = next((i for i, t in enumerate(out) if t in eos), None)
        ids = out if stop is None else out[: stop + 1]
        while stop is None and ids and ids[-1] == pad:
            ids = ids[:-1]
        text = None
        if p.stop_token_ids or p.stop:
            # the device ended the chain at the step that completed a stop sequence (pad follows); the text is cut here, exactly at
            # text level, whatever tokenization carried a stop string (hostloop.first_stop_cut).  A stop token id is kept, as an EOS is.
            from .hostloop import first_stop_cut, first_stop_hit
            n_id = first_stop_hit(ids, [[t] for t in p.stop_token_ids], p.min_tokens)
            cut = first_stop_cut(self.processor.tokenizer, ids, p.stop, p.min_tokens) if p.stop else None
            if cut is not None and (n_id is None or cut[0] <= n_id):
                ids, text, stop = ids[: cut[0]], cut[1].strip(), cut[0]
            elif n_id is not None:
                ids, stop = ids[:n_id], n_id
        if text is None:
            text = self.processor.tokenizer.decode(ids, skip_special_tokens=True).strip()
        res = {
            "id": "chatcmpl-" + uuid.uuid4().hex[:24], "object": "chat.completion", "created": int(time.time()),
            "model": p.req.get("model") or self.model_id,
            "choices": [{"index": 0, "message": {"role": "assistant", "content": text},
                         "finish_reason": "stop" if stop is not None else "length"}],
            "usage": {"prompt_tokens": n_in, "completion_tokens": len(ids), "total_tokens": n_in + len(ids)},
        }
        if p.logprobs is not None and lp is not None:  # (between message and finish_reason, where OpenAI has it)
            c = res["choices"][0]
            res["choices"][0] = {"index": c["index"], "message": c["message"], "logprobs": self._logprobs_block(p, ids, lp),
                                 "finish_reason": c["finish_reason"]}
        if p.prompt_logprobs is not None and prompt is not None:
            res["prompt_logprobs"] = self._prompt_logprobs_list(p, prompt[0], prompt[1:])
        return res

    @staticmethod
    def _merge_choices(parts, n_in: int) -> dict:
        """The one-choice responses of a request's n completions, in index order, as one response: n indexed choices, the usage
        summed over them with the prompt counted once; id, created and the top-level prompt_logprobs are the first one's."""
        res = parts[0]
        for i, r in enumerate(parts[1:], 1):
            res["choices"].append({**r["choices"][0], "index": i})
        done = sum(r["usage"]["completion_tokens"] for r in parts)
        details = parts[0]["usage"].get("prompt_tokens_details")
        res["usage"] = {"prompt_tokens": n_in, "completion_tokens": done, "total_tokens": n_in + done}
        if details is not None:
            res["usage"]["prompt_tokens_details"] = details
        return res

    def _run(self, batch):
        """One processor + generate call for the parsed requests of `batch` (all greedy without logit adjustments, or a single
        request: generate() gives every row of a call the same sampling settings and adjustments)."""
        from .image import DeviceImage

        with self._lock:
            images = [[DeviceImage.from_pil(im, self.model.engine) for im in p.pil_images] for p in batch]
            flat = [im for row in images for im in row]  # consumed in prompt order, row after row
            inputs = self.processor(text=[p.prompt for p in batch], images=flat or None, return_tensors="pt",
                                    padding="longest").to(self.model.device)
            width = int(inputs["input_ids"].shape[1])
            n_in = inputs["attention_mask"].sum(dim=1).tolist()
            p0 = batch[0]
            kw = dict(max_new_tokens=max(p.max_tokens for p in batch), num_beams=1, do_sample=p0.sample)
            if p0.sample:
                kw.update(temperature=p0.temperature, top_k=p0.top_k, top_p=p0.top_p, min_p=p0.min_p, seed=p0.seed)
                kw.update(p0.entropy_kw())
            if p0.repetition_penalty is not None:
                kw.update(repetition_penalty=p0.repetition_penalty)
            kw.update(p0.adjust_kw(self.processor.tokenizer))
            want = [p.logprobs for p in batch if p.logprobs is not None]
            if not want:
                out = self.model.generate(**inputs, **kw)[:, width:].tolist()
                return [self._response(p, row, int(n)) for p, row, n in zip(batch, out, n_in)]
            g = self.model.generate(**inputs, logprobs=max(want), **kw)
            out = g.sequences[:, width:].tolist()
            lps = [(g.logprobs[b].tolist(),
                    [[(i, v) for i, v in zip(ids, vals) if i >= 0] for ids, vals in zip(g.top_ids[b].tolist(), g.top_logprobs[b].tolist())])
                   for b in range(len(batch))]
        return [self._response(p, row, int(n), lp) for p, row, n, lp in zip(batch, out, n_in, lps)]

    def _run_beam(self, p: _Parsed) -> dict:
        """A `use_beam_search` request through model.beam_search: n beams, the n best finished hypotheses as n indexed choices, best
        first.  The call takes the engine's first n slots, so the caller runs it while no scheduler chain is alive, under the lock."""
        from .image import DeviceImage

        images = [DeviceImage.from_pil(im, self.model.engine) for im in p.pil_images]
        inputs = self.processor(text=[p.prompt], images=images or None, return_tensors="pt").to(self.model.device)
        width, n_in = int(inputs["input_ids"].shape[1]), int(inputs["attention_mask"].sum())
        kw = dict(num_beams=p.n, num_return_sequences=p.n, max_new_tokens=max(1, min(p.max_tokens, self.model.engine.max_ctx)),
                  length_penalty=p.length_penalty)
        if p.repetition_penalty is not None:
            kw.update(repetition_penalty=p.repetition_penalty)
        try:
            out = self.model.beam_search(**inputs, **kw)[:, width:].tolist()
        finally:
            for slot in range(p.n):   # the slots go back empty
                self.model.engine.seq_reset(slot)
        return self._merge_choices([self._response(p, row, n_in) for row in out], n_in)

    # ------------------------------------------------------------------ entry points
    def complete(self, req: dict) -> dict:
        p = self._parse(req)
        if p.use_beam_search:
            if self._worker is not None:   # a dispatcher owns the chain slots: it runs the request while none of its chains is alive
                return self.submit(req).result()
            with self._lock:
                return self._run_beam(p)
        if p.prompt_logprobs is not None or p.n > 1:   # the scheduler's work: the scoring prefill pass, the fork of n completions
            return self.submit(req).result()
        return self._run([p])[0]

    def complete_many(self, reqs) -> list:
        """The requests as ONE batch (all must be greedy with the model's own repetition penalty; at most max_seqs of them)."""
        batch = [self._parse(r) for r in reqs]
        if any(p.repetition_penalty is not None for p in batch) and len(batch) > 1:
            raise BadRequest("requests with a repetition_penalty of their own are not batched")
        if any(p.sample for p in batch) and len(batch) > 1:
            raise BadRequest("sampled requests are not batched")
        if any(p.adjusts() for p in batch) and len(batch) > 1:
            raise BadRequest("requests with presence_penalty / frequency_penalty / logit_bias / min_tokens / stop / stop_token_ids / "
                             "no_repeat_ngram_size / guided_regex / guided_choice are not batched")
        if len(batch) > self.max_batch:
            raise BadRequest(f"batch of {len(batch)} exceeds max_seqs = {self.max_batch}")
        if any(p.prompt_logprobs is not None or p.n > 1 or p.use_beam_search for p in batch):
            raise BadRequest("requests with prompt_logprobs or n > 1 go through submit() / complete()")   # (use_beam_search has n > 1)
        return self._run(batch)

    def submit(self, req: dict):
        """Queues the request for the batching dispatcher; returns a concurrent.futures.Future of the response.
        Malformed requests raise BadRequest here, before anything is queued."""
        from concurrent.futures import Future

        p = self._parse(req)
        p.future = Future()
        with self._cv:
            if self._worker is None:
                self._worker = threading.Thread(target=self._dispatch, name="ze-batcher", daemon=True)
                self._worker.start()
            self._queue.append(p)
            self._cv.notify()
        return p.future

    def close(self):
        with self._cv:
            self._stop = True
            self._cv.notify()
        if self.prefix_cache is not None:   # the dispatcher ends first (it may be in the middle of a step), then the pool goes
            worker = self._worker
            if worker is not None and worker is not threading.current_thread():
                worker.join()
            with self._lock:
                self.prefix_cache.close()
                self.prefix_cache = None

    def _request(self, p: _Parsed):
        """The scheduler's Request of a parsed one: its fields under the scheduler's names, the budget clamped to the KV capacity
        (per request: never fails its batch), its future resolved by the callbacks.  A sampled request carries its own temperature
        and seed, and random stream 0: what it would draw running alone.  With n > 1 the scheduler calls `done` once per completion
        (stream `index`); the future resolves with the n-th."""
        from .image import DeviceImage
        from .scheduler import Request

        parts = [None] * p.n

        def done(req, tokens, text):
            prompt = None
            if p.prompt_logprobs is not None and req.index == 0:
                prompt = (req._prompt_ids, req.prompt_token_logprobs, req.prompt_ranks, req.prompt_top_logprobs)
            parts[req.index] = self._response(p, tokens, req.n_prompt, (req.token_logprobs, req.top_logprobs), prompt)
            if self.prefix_cache is not None:   # OpenAI's field: the prompt rows this request did not compute
                parts[req.index]["usage"]["prompt_tokens_details"] = {"cached_tokens": int(getattr(req, "cached_tokens", 0))}
            if all(r is not None for r in parts) and not p.future.done():
                p.future.set_result(parts[0] if p.n == 1 else self._merge_choices(parts, req.n_prompt))
            return None

        def failed(req, ex):
            if not p.future.done():
                p.future.set_exception(ex)

        own = dict(do_sample=True, temperature=p.temperature, seed=p.seed, stream_id=0, top_k=p.top_k, top_p=p.top_p,
                   min_p=p.min_p, **p.entropy_kw()) if p.sample else {}
        if p.repetition_penalty is not None:
            own["repetition_penalty"] = p.repetition_penalty
        return Request(prompt=p.prompt, images=[DeviceImage.from_pil(im, self.model.engine) for im in p.pil_images],
                       max_new_tokens=max(1, min(p.max_tokens, self.model.engine.max_ctx)), on_done=done, on_error=failed,
                       logprobs=p.logprobs, prompt_logprobs=p.prompt_logprobs, presence_penalty=p.presence_penalty, frequency_penalty=p.frequency_penalty,
                       logit_bias=p.logit_bias, min_new_tokens=p.min_tokens, stop_ids=p.stop_records(self.processor.tokenizer),
                       no_repeat_ngram_size=p.no_repeat_ngram_size, guided_regex=p.guided_regex, guided_choice=p.guided_choice, n=p.n, **own)

    def _dispatch(self):
        """Running-batch admission (the concurrency model of the reference's src/eval/infer_vllm.py:244-271, where the
        client keeps up to 100 requests in flight): every request goes to ONE `ChainScheduler` -- a request that arrives
        while others are decoding is prefilled and joins their next burst, one that finishes frees its KV slot at once --
        and each future resolves as soon as ITS chain ends.  Wait, collect, submit, step."""
        from .scheduler import ChainScheduler

        sched = None
        beams, held = [], []   # beam requests wait for the running chains to end; what arrives behind them waits for the beams
        while True:
            with self._cv:
                # (a beam request that waits for the running chains to end is work too, and so is what waits behind it: neither
                #  the wait nor the stop may pass them by)
                while not self._queue and not self._stop and not beams and not (sched is not None and sched.busy()):
                    self._cv.wait()
                if self._stop and not self._queue and not beams and not (sched is not None and sched.busy()):
                    return
                if not beams and (sched is None or not sched.busy()):  # idle: give concurrent arrivals a moment to share the first prefill
                    deadline = time.monotonic() + self.batch_window_s
                    while len(self._queue) < self.max_batch and not self._stop:
                        left = deadline - time.monotonic()
                        if left <= 0:
                            break
                        self._cv.wait(left)
                new, self._queue = self._queue, []
            with self._lock:
                if sched is None:
                    kw = {}
                    if self.prefix_cache_rows > 0:   # (the cache outlives a scheduler that had to be replaced)
                        if self.prefix_cache is None:
                            from .prefix_cache import PrefixCache
                            self.prefix_cache = PrefixCache(self.model.engine, self.prefix_cache_rows)
                        kw["prefix_cache"] = self.prefix_cache
                    if self.speculative_ngram > 0:
                        kw["speculative_tokens"] = self.speculative_ngram
                        if self.speculative_sampling:
                            kw["speculative_sampling"] = True
                    sched = ChainScheduler(self.model, self.processor, do_sample=False, max_batch=self.max_batch, burst=8, **kw)
                    self.scheduler = sched
                def admit(reqs):
                    for p in reqs:
                        try:
                            sched.submit(self._request(p))
                        except Exception as ex:
                            if not p.future.done():
                                p.future.set_exception(ex)

                ahead = []   # arrivals in front of the first waiting beam request go to the scheduler as ever
                for p in new:
                    (beams if p.use_beam_search else held if beams else ahead).append(p)
                admit(ahead)
                if beams and not sched.busy():   # model.beam_search takes the first n slots: only while no chain is alive
                    for p in beams:
                        try:
                            p.future.set_result(self._run_beam(p))
                        except Exception as ex:
                            p.future.set_exception(ex)
                    waiting, beams, held = held, [], []
                    admit(waiting)
                if sched.busy():
                    try:
                        sched.step()
                    except Exception as ex:  # an engine failure: every request of the running batch gets the error
                        for r in sched.pending_requests():
                            if r.on_error:
                                r.on_error(r, ex)
                        sched = None


def create_app(server: ChatServer):
    from fastapi import FastAPI, Request
    from fastapi.responses import JSONResponse

    app = FastAPI(title="zoomearth-mi355x")

    @app.get("/health")
    def health():
        return {"status": "ok"}

    @app.get("/v1/models")
    def models():
        card = {"id": server.model_id, "object": "model", "owned_by": "zoomearth-mi355x"}
        adapter = getattr(server.model, "active_adapter", None)
        if adapter is not None:
            card["adapter"] = adapter
        engine = getattr(server.model, "engine", None)
        if engine is not None and hasattr(engine, "weight_format"):
            card["weight_format"] = engine.weight_format   # "bf16", or the reduced-precision decode stream: "fp8" / "mxfp4"
        if getattr(server, "speculative_ngram", 0) > 0:
            card["speculative_ngram"] = server.speculative_ngram   # draft ids per step by prompt lookup (lossless)
            card["speculative_sampling"] = bool(getattr(server, "speculative_sampling", False))   # sampled requests speculate too
        return {"object": "list", "data": [card]}

    @app.post("/v1/chat/completions")
    async def chat(request: Request):
        import asyncio

        try:
            body = await request.json()
            return JSONResponse(await asyncio.wrap_future(server.submit(body)))
        except BadRequest as ex:
            return JSONResponse({"error": {"message": str(ex), "type": "invalid_request_error"}}, status_code=400)
        except Exception as ex:  # engine errors surface as a 500 with the engine's message
            return JSONResponse({"error": {"message": str(ex), "type": "server_error"}}, status_code=500)

    return app


def main():  # pragma: no cover
    import argparse
    import os

    import uvicorn

    from .modeling import ZoomEarthForConditionalGeneration
    from .processor import ZoomEarthProcessor

    ap = argparse.ArgumentParser(description="OpenAI-compatible server on the MI355X engine")
    ap.add_argument("--model_name", required=True)
    ap.add_argument("--served_model_name", default="ZoomEarth")
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--port", type=int, default=8000)
    ap.add_argument("--prefix-cache-rows", type=int, default=0,
                    help="keep the K/V rows of finished requests in a pool of this many rows (0 = off); later requests that start "
                         "with them prefill only their tail and report usage.prompt_tokens_details.cached_tokens")
    ap.add_argument("--speculative-ngram", type=int, default=0,
                    help="speculative decoding by prompt lookup: up to K draft ids per step for greedy requests (vLLM's ngram method; "
                         "lossless; 0 = off; needs at most 64 chain slots; reported by /v1/models)")
    ap.add_argument("--speculative-sampling", action="store_true",
                    help="with --speculative-ngram: sampled requests (temperature / seed / top_p) speculate too, each row drawing "
                         "what a plain step draws (lossless; reported by /v1/models)")
    ap.add_argument("--lora", default=None, help="a PEFT LoRA adapter directory: loaded and activated at start (listed by /v1/models)")
    ap.add_argument("--weight-format", default="bf16", choices=["bf16", "fp8", "mxfp4"],
                    help="decode weight stream: fp8 / mxfp4 quantise the decoder's linear layers (reduced precision, opt-in; "
                         "reported by /v1/models)")
    args = ap.parse_args()
    model = ZoomEarthForConditionalGeneration.from_pretrained(args.model_name, weight_format=args.weight_format)
    if args.lora:
        model.set_adapter(model.load_adapter(args.lora, os.path.basename(os.path.normpath(args.lora)) or "default"))
    processor = ZoomEarthProcessor.from_pretrained(args.model_name, trust_remote_code=True, max_pixels=128 * 128 * 28 * 28)
    processor.tokenizer.padding_side = "left"
    uvicorn.run(create_app(ChatServer(model, processor, args.served_model_name, prefix_cache_rows=args.prefix_cache_rows,
                                     speculative_ngram=args.speculative_ngram, speculative_sampling=args.speculative_sampling)),
                host=args.host, port=args.port)


if __name__ == "__main__":  # pragma: no cover
    main()

"""Continuous batching of question chains on one GPU.

replaces: the one-sample-at-a-time loop of the reference (`BATCH_SIZE = 1`, /root/reference/src/eval/infer.py:27,
173-249) and the 100 requests its "fast" path keeps in flight against a serving back-end
(/root/reference/src/eval/infer_vllm.py:244-271).  Up to `max_seqs` chains share every decode step -- the weights are
streamed once per step for all of them (`ze_decode_burst`) -- and chains join and leave BETWEEN bursts: a request that
finishes (EOS or its token budget) hands its KV slot to the next waiting request, or keeps it for a follow-up that
extends its own prompt (stage 2 of the zoom chain: the cached stage-1 prompt is reused, only the appended tokens are
prefilled, `ze_seq_truncate`).  Newcomers of one round are prefilled together (`ze_prefill_batch`) after ONE
multi-resolution ViT call over all their images.

A chain's tokens do not depend on which chains share its bursts (the batched kernels accumulate every output element in
an order that is a function of the layer shape alone -- tests/test_gpu_batch.py), and its sampling stream is the
request's own `stream_id`.  The decode step has one kernel family per engine (`Engine.decode_regime`: the fragment kernels
of an engine with at most 64 chain slots, the row-streaming kernels of a larger one), chosen by the engine's CAPACITY and
never by how many chains happen to be live, so results are the same for any `max_batch` of one engine, including 1, and
for every engine of one regime; engines of different regimes agree within bf16 rounding (tests/test_gpu_3b_shape.py).
"""
from __future__ import annotations

import contextlib
import copy
import os
import time
from collections import OrderedDict, deque
import dataclasses
from dataclasses import InitVar, dataclass, field
from typing import Any, Callable, List, Optional

import numpy as np
import torch

from .chain_request import ChainRequest

# the default of every `adapter=` argument, here and in modeling.py (which imports this module, so the sentinel lives on this side):
# leave the model's LoRA adapter as it is
KEEP_ADAPTER = object()


@dataclass
class Request:
    prompt: str
    images: list                       # flat, in prompt order (DeviceImage / PIL / ndarray)
    max_new_tokens: int = 1024
    stream_id: int = 0                 # random stream of the request when sampling (e.g. the question number)
    on_done: Optional[Callable[["Request", List[int], str], Optional["Request"]]] = None
    on_error: Optional[Callable[["Request", Exception], None]] = None
    tag: Any = None
    # sampling filters of this request (None = the scheduler's default; 0 / 1.0 / 0.0 = off); used by a sampling scheduler only
    top_k: Optional[int] = None
    top_p: Optional[float] = None
    min_p: Optional[float] = None
    # log-probabilities of the generated tokens (None = the scheduler's default, which is off; 0 = the chosen token only; 1..20 =
    # that many best alternatives as well)
    logprobs: Optional[int] = None
    # logit adjustments of this request (None = the scheduler's default, which is off): OpenAI's presence / frequency penalties
    # over the tokens the request generates, `logit_bias` {token id: bias} (-inf bans the token), and the EOS ids banned until
    # min_new_tokens were generated; greedy schedulers honour them too
    presence_penalty: Optional[float] = None
    frequency_penalty: Optional[float] = None
    logit_bias: Optional[dict] = None
    min_new_tokens: Optional[int] = None
    # token rules of this request, on the device: `stop_ids` token-id sequences that end the chain as an EOS does (the request
    # is retired in the burst that matched, its slot goes to a waiting one), HF's `bad_words_ids` and `no_repeat_ngram_size` over
    # prompt + generated ids
    stop_ids: Optional[list] = None
    bad_words_ids: Optional[list] = None
    no_repeat_ngram_size: Optional[int] = None
    # guided decoding of this request (vLLM's `guided_regex`, a pattern, or `guided_choice`, a list of strings; not both): the chain
    # is held to it by a token automaton on the device (zoomearth_amd/grammar.py); requests of different grammars and none share bursts
    guided_regex: Optional[str] = None
    guided_choice: Optional[list] = None
    # sampling of this request (None = the scheduler's own value): greedy or sampled, temperature, seed and repetition penalty.
    # A request that names one carries its values into the engine's per-slot table, so requests with different values share the
    # same bursts; its draws are those of a scheduler whose own values are these (same stream_id)
    do_sample: Optional[bool] = None
    temperature: Optional[float] = None
    seed: Optional[int] = None
    repetition_penalty: Optional[float] = None
    # vLLM's `prompt_logprobs=N` (None = off; 0 = the prompt's own tokens only; 1..20 = that many best alternatives as well): the
    # request's prefill pass scores its prompt positions (ze_score_batch_detail).  An init-only argument kept as a plain attribute,
    # like its three result lists below: `dataclasses.fields(Request)` stays the list of what every request carries into its decode
    # steps, and a request that does not ask is the object it was
    prompt_logprobs: InitVar[Optional[int]] = None
    # parallel sampling (vLLM's `n`, HF's `num_return_sequences`): that many completions of the prompt, a sampled request only.  The
    # prompt is prefilled once and forked on the device (ze_seq_fork); completion i draws on stream `stream_id + i`, and on_done /
    # on_error run once per completion with a request object of its own that carries `.index` = i and `.parent` = this request (a
    # follow-up returned for it continues on that completion's slot).  Init-only like prompt_logprobs, and for the same reason
    n: InitVar[int] = 1
    # speculative decoding by prompt lookup (None = the scheduler's default; 0 = off; 1 .. 8 draft ids per step): greedy only -- a
    # request that names it together with sampling, log-probabilities, logit adjustments, token rules or a grammar is refused.
    # Init-only like prompt_logprobs, and for the same reason
    speculative_tokens: InitVar[Optional[int]] = None
    # the sampled mode of speculation for this request (None = the scheduler's default): a sampled request, with its top-k / top-p /
    # min-p, speculates too -- every row draws what a plain step draws (Engine.set_speculation(sampled=True)).  Init-only likewise
    speculative_sampling: InitVar[Optional[bool]] = None
    # HF's typical_p / epsilon_cutoff / eta_cutoff of this request (None = the scheduler's default; 1.0 / 0.0 / 0.0 = off), resolved
    # like min_p and written with the sampling filter.  Init-only like prompt_logprobs, and for the same reason
    typical_p: InitVar[Optional[float]] = None
    epsilon_cutoff: InitVar[Optional[float]] = None
    eta_cutoff: InitVar[Optional[float]] = None
    # filled by the scheduler
    slot: int = -1
    n_prompt: int = 0
    tokens: List[int] = field(default_factory=list)
    text: str = ""
    # with `logprobs`: one entry per token of `tokens`, there before on_done runs -- the log-probability of the token under the
    # model's own distribution at its step, and the step's best alternatives as (id, logprob), best first
    token_logprobs: List[float] = field(default_factory=list)
    top_logprobs: List[list] = field(default_factory=list)
    # with `prompt_logprobs`: one entry per prompt token, there before on_done runs -- the token's log-probability given the ids in
    # front of it, its 0-based rank, and the best alternatives at its place as (id, logprob), best first.  None at position 0 and
    # wherever the predicting row was not computed by the request's own pass (a cached prefix of its slot)
    def __post_init__(self, prompt_logprobs, n=1, speculative_tokens=None, speculative_sampling=None, typical_p=None, epsilon_cutoff=None,
                      eta_cutoff=None):
        self.typical_p, self.epsilon_cutoff, self.eta_cutoff = typical_p, epsilon_cutoff, eta_cutoff
        self.prompt_logprobs = prompt_logprobs
        self.speculative_tokens = speculative_tokens
        self.speculative_sampling = speculative_sampling
        self.n, self.index, self.parent = n, 0, None
        self.prompt_token_logprobs, self.prompt_ranks, self.prompt_top_logprobs = [], [], []


class GrammarCache:
    """The compiled grammars of one engine, least recently used first: at most `capacity` (ZE_MAX_GRAMMARS) live on the device,
    keyed by their pattern.  `acquire` returns the device id of the key's grammar -- compiling and creating it on first use, and
    evicting the least recently used grammar no live chain uses when the engine is full -- and counts the chain as a user;
    `release` gives the use back.  With every grammar in use, `acquire` raises: that request fails, nothing waits."""

    def __init__(self, engine, compile_fn, capacity: int = 16):
        self.engine, self.compile, self.capacity = engine, compile_fn, int(capacity)
        self.ids = OrderedDict()   # key -> device id, least recently used first
        self.users = {}            # key -> live chains

    def acquire(self, key) -> int:
        if key not in self.ids:
            automaton = self.compile(key)   # (first: a pattern that does not compile evicts nothing)
            if len(self.ids) >= self.capacity:
                idle = next((k for k in self.ids if self.users.get(k, 0) == 0), None)
                if idle is None:
                    raise RuntimeError(f"all {self.capacity} grammars of the engine are in use by live chains")
                self.engine.grammar_destroy(self.ids.pop(idle))
                self.users.pop(idle, None)
            self.ids[key] = self.engine.grammar_create(automaton)
        self.ids.move_to_end(key)
        self.users[key] = self.users.get(key, 0) + 1
        return self.ids[key]

    def release(self, key) -> None:
        if self.users.get(key, 0) > 0:
            self.users[key] -= 1


def shared_prefix_len(a, b, image_token_id) -> int:
    """Longest common prefix of two id lists that leaves both a non-empty tail and does not end inside a run of image
    tokens (a run is fed by one image's feature rows: it is shared whole or not at all).  The rule of every planner that
    shares K/V rows between chains (ChainScheduler._plan_sharing, score_plan.plan_score_passes)."""
    n = min(len(a), len(b)) - 1
    i = 0
    while i < n and a[i] == b[i]:
        i += 1
    return cut_at_image_run(a, i, image_token_id)


def cut_at_image_run(ids, i, image_token_id) -> int:
    """The largest cut <= i of `ids` that does not fall inside a run of image tokens."""
    while 0 < i < len(ids) and ids[i - 1] == image_token_id and ids[i] == image_token_id:
        i -= 1
    return i


def images_in(ids, n, image_token_id) -> int:
    """Image runs that begin in the first n ids."""
    return sum(1 for t in range(n) if ids[t] == image_token_id and (t == 0 or ids[t - 1] != image_token_id))


class _Live:
    __slots__ = ("req", "ids", "keys", "produced")

    def __init__(self, req, ids, keys):
        self.req, self.ids, self.keys, self.produced = req, ids, keys, 1


_PER_CHAIN = os.environ.get("ZE_PER_CHAIN_XFER") == "1"   # measurement only: the per-chain mark_seen / chain_tokens calls (A/B runs)


class ChainScheduler:
    def __init__(self, model, processor, do_sample: bool = False, temperature=None, repetition_penalty=None, seed: int = 0,
                 burst: int = 8, max_batch: Optional[int] = None, ignore_eos: bool = False, use_graph: Optional[bool] = None,
                 feature_cache: int = 64, min_admit: int = 1, max_wait_bursts: int = 2, share_prefix: bool = True,
                 min_shared: int = 64, reuse_generated: bool = True, overlap: Optional[bool] = None, hold_below: int = 0,
                 admit_chunk_rows: int = 0, top_k: Optional[int] = None, top_p: Optional[float] = None,
                 min_p: Optional[float] = None, logprobs: Optional[int] = None, presence_penalty: Optional[float] = None,
                 frequency_penalty: Optional[float] = None, logit_bias: Optional[dict] = None, min_new_tokens: Optional[int] = None,
                 prefix_cache_rows: int = 0, prefix_cache_block_rows: int = 32, prefix_cache=None, adapter=KEEP_ADAPTER,
                 speculative_tokens: int = 0, ngram_min: int = 1, ngram_max: int = 3, typical_p: Optional[float] = None,
                 epsilon_cutoff: Optional[float] = None, eta_cutoff: Optional[float] = None, speculative_sampling: bool = False):
        self.model, self.processor, self.engine = model, processor, model.engine
        # the sampled mode of speculation, the default of requests that name none: off -- a sampled request then rides with one row
        self.speculative_sampling = bool(speculative_sampling)
        self.typical_p, self.epsilon_cutoff, self.eta_cutoff = typical_p, epsilon_cutoff, eta_cutoff
        # Speculative decoding by prompt lookup: the default of requests that name none (0 = off).  A step of the fragment family
        # holds 64 rows, one per chain and one more per draft id: a chain's k is lowered when it joins so that the live chains' rows,
        # and one row for every slot still free, fit (_spec_budget).  Requests that cannot speculate (sampled, log-probabilities,
        # adjustments, rules, a grammar) ride the same bursts with one row.
        self.speculative_tokens, self.ngram_min, self.ngram_max = int(speculative_tokens or 0), int(ngram_min), int(ngram_max)
        if not (0 <= self.speculative_tokens <= 8) or not (1 <= self.ngram_min <= self.ngram_max <= 8):
            raise ValueError("speculative_tokens has to be in [0, 8] and 1 <= ngram_min <= ngram_max <= 8")
        if self.speculative_tokens and min(int(max_batch or self.engine.max_seqs), self.engine.max_seqs) > 64:
            raise ValueError("speculative decoding runs on the fragment kernels: max_batch <= 64")
        # Logit adjustments: the defaults of requests that name none (None = off).  Written into the slot's rows of the engine's
        # tables next to the filter, with zero counts, for fresh slots and for follow-ups on a parked slot alike; requests with and
        # without them share the same bursts.
        self.presence_penalty, self.frequency_penalty = presence_penalty, frequency_penalty
        self.logit_bias, self.min_new_tokens = logit_bias, min_new_tokens
        # Log-probabilities of generated tokens: the default of requests that name none (None = off).  Written into the slot's row
        # of the engine's table next to the filter; requests with and without them share the same bursts.
        self.logprobs = logprobs
        # Sampling filters (top-k / top-p / min-p): the defaults of requests that name none; settable between requests.  A request's
        # filter is written into its slot's row of the engine's table right before its first draw, so requests with different
        # filters share the same bursts.  Written for a request whose effective mode is sampled (its own `do_sample`, else the
        # scheduler's): a greedy scheduler without such requests never touches the table.
        self.do_sample = bool(do_sample)
        self.top_k, self.top_p, self.min_p = top_k, top_p, min_p
        gc = model.generation_config
        pen = repetition_penalty if repetition_penalty is not None else (getattr(gc, "repetition_penalty", 1.0) or 1.0)
        if do_sample and temperature is None:
            temperature = getattr(gc, "temperature", None) or 1.0
        self.penalty = float(pen)
        self.temperature, self.seed = float(temperature or 1.0), int(seed)
        # Captured hipGraphs for the decode steps: yes in the fragment regime (at most 64 chains: a step of ~3.4 ms is ~330
        # launches), no in the row-streaming regime -- its steps take 6-25 ms, the host runs far ahead of the GPU, and a graph
        # is keyed by (live chains, attention grid), i.e. captured anew at almost every burst (stream: 72.1 / 72.0 questions/s
        # with graphs, 72.7 / 72.7 without)
        if use_graph is None:
            use_graph = min(int(max_batch or self.engine.max_seqs), self.engine.max_seqs) <= 64
        self.use_graph = bool(use_graph)
        self.params = self.engine.gen_params(repetition_penalty=self.penalty, ignore_eos=ignore_eos, use_graph=use_graph,
                                             do_sample=bool(do_sample), temperature=float(temperature or 1.0), seed=seed)
        # Admission hysteresis: while chains are decoding, newcomers wait until `min_admit` of them can share one ViT call
        # and one prefill pass (a 520-row prefill alone runs its GEMMs at a third of the rate of a 4000-row pass), but
        # never longer than `max_wait_bursts` bursts; with nothing decoding they are admitted at once.
        self.min_admit = max(1, int(min_admit))
        self.max_wait_bursts = max(0, int(max_wait_bursts))
        self._waited = 0
        # Hold: while an admission round still has prefill passes to run and fewer than `hold_below` chains are live, the live
        # chains do not decode -- a step costs almost the same at 60 chains as at 400, so the early members of a round wait
        # for the later ones instead of stepping alone beside the passes.  0: never hold (a server's latency setting).
        self.hold_below = max(0, int(hold_below))
        # Admission in CHUNKS (round 6): with a long queue -- the start of a run: hundreds of prompts at once -- tokenising and planning
        # every waiting request before the first pass is enqueued leaves the GPU idle for the whole of it (0.4 s for 640 prompts).  With
        # `admit_chunk_rows` > 0 one call of _admit takes requests off the queue only until that many new rows are planned (a pass's
        # worth) and the NEXT request is about another first image (the questions of a tile stay together: their shared prefix is
        # planned within one call), enqueues that pass, and prepares the next chunk while the GPU runs it.  Under `hold_below` the
        # requests still admissible count as "round in progress": the early chunks' chains wait for the later ones as before.
        self.admit_chunk_rows = max(0, int(admit_chunk_rows))
        # Shared prompt prefixes: the questions about one tile start with the same system turn and the same view's image
        # tokens (347 of the 802 tokens of a stage-1 prompt).  A fresh chain whose prompt starts like that of a chain that
        # already holds those K/V rows copies them (ze_seq_copy_prefix) and prefills only its own tail; when a round brings
        # several such chains and none exists yet, the first one's prefix is prefilled alone (pass A), copied to the
        # others, and all tails go through one pass (pass B).  Bit-identical to prefilling every prompt in full.
        self.share_prefix = bool(share_prefix)
        self.min_shared = max(1, int(min_shared))
        # Follow-ups keep the K/V rows of the tokens their predecessor generated while the new prompt repeats those ids
        # (exact in real arithmetic; in bf16 the rows come from the decode kernels instead of the prefill kernels, both
        # held to the same tolerance against the oracle).  False: only the predecessor's PROMPT rows are kept, which is
        # bit-identical to prefilling the new prompt in full.
        self.reuse_generated = bool(reuse_generated)
        self.burst = max(1, int(burst))
        self.max_batch = min(int(max_batch or self.engine.max_seqs), self.engine.max_seqs)
        # the decode step's kernel family follows the scheduler's CAPACITY, never the live count (see the module docstring)
        if hasattr(self.engine, "set_decode_regime"):
            self.engine.set_decode_regime(1 if self.max_batch > 64 else 0)
        self.waiting = deque()
        self.live = OrderedDict()          # slot -> _Live
        self.parked = {}                   # slot -> (prompt ids, image keys, generated ids with K/V rows): finished chains whose slot waits for a follow-up
        self.free = list(range(self.max_batch))[::-1]
        self._features = OrderedDict()     # image key -> ViT features (LRU)
        self._feature_cap = feature_cache
        self.stats = dict(bursts=0, steps=0, chain_steps=0, prefill_rows=0, admitted=0, vit_calls=0, shared_rows=0,
                          reused_generated_rows=0, overlapped_passes=0, forked_chains=0, forked_rows=0)
        # Prefix cache (zoomearth_amd/prefix_cache.py): K/V rows that outlive their chains.  The sharing above needs a donor that is
        # alive or parked; with a cache, a chain that retires leaves the full blocks of its rows in the engine's pool, and a later
        # fresh chain whose prompt starts with them loads them (ze_prefix_load) and prefills only its tail -- the second HTTP request
        # of a question, the next question of a tile sent after the first has finished, the next rollout of the same samples.
        # `prefix_cache_rows` = 0 (the default): no pool, no call, today's path.  `prefix_cache`: a PrefixCache of this engine that
        # outlives the scheduler (rollout_two_stage hands the same one to every call).
        self.prefix_cache, self._owns_prefix_cache = prefix_cache, False
        if prefix_cache is None and int(prefix_cache_rows) > 0:
            from .prefix_cache import PrefixCache
            self.prefix_cache = PrefixCache(self.engine, int(prefix_cache_rows), int(prefix_cache_block_rows))
            self._owns_prefix_cache = True   # (close() gives the pool back; a cache handed in is its owner's)
        if self.prefix_cache is not None:
            self.prefix_cache.unpin_all()   # (loads a previous scheduler of this engine planned and never ran)
            self.stats.update(prefix_cache_hit_rows=0, prefix_cache_saved_rows=0, prefix_cache_evicted_blocks=0,
                              prefix_cache_save_errors=0)
            self.prefix_cache_last_error = None
        # Overlap of the two kinds of work on one GPU: while a burst of decode steps runs on the caller's stream
        # (ze_decode_burst_begin: enqueued, not awaited), ONE prefill pass of the admission round -- its ViT call included --
        # is enqueued on a side stream; the burst is collected afterwards (ze_decode_burst_end) and the chains whose pass
        # has completed join the next burst.  The batched decode step has activation buffers of its own and the chains of
        # a pass are not in the burst, so the two streams share no state; the matrix-bound pass fills what the bandwidth-
        # and latency-bound decode steps leave idle, and the host work of admission (tokeniser, index builders, callbacks)
        # hides behind the burst.  Results are unchanged: the same kernels on the same operands.
        if overlap is None:
            overlap = hasattr(self.engine, "decode_burst_begin") and os.environ.get("ZE_OVERLAP", "1") != "0"
        self.overlap = bool(overlap)
        self._side = torch.cuda.Stream(device=self.engine.device) if (self.overlap and torch.cuda.is_available()) else None
        self._carry = []                   # (admit_chunk_rows) planned items of a partial pass, waiting for the next chunk's
        self._groups = deque()             # prefill passes of the admission round in progress, one per step
        self._round = None                 # (todo, needed) of that round: images still to encode / features to keep
        self._ready = []                   # prefilled requests waiting to join the live set
        self._pass_done = []               # (overlap) per entry of _ready: the event behind its prefill pass
        self._trace_ev = None
        if os.environ.get("ZE_SCHED_TRACE") and torch.cuda.is_available():   # measurement only: when the first passes really START on the GPU
            self._trace_ev = dict(base=torch.cuda.Event(enable_timing=True), t0=time.perf_counter(), passes=[])
            self._trace_ev["base"].record(torch.cuda.current_stream(self.engine.device))
        model._chains.clear()              # the scheduler owns every chain slot while it runs
        # LoRA adapter: a loaded adapter's name, None for the base weights, or (the default) whatever the model has active.  Set here,
        # before any chain exists, and fixed for the scheduler's life: the K/V rows of every chain belong to it.
        if adapter is not KEEP_ADAPTER:
            self.set_adapter(adapter)

    def set_adapter(self, adapter) -> None:
        """Switches the model's LoRA adapter for this scheduler.  Refused while chains are live or being admitted; a switch drops the
        ViT feature LRU and the parked chains, whose rows came from the other weights (a prefix cache is flushed by the engine's
        generation)."""
        if adapter == self.model.active_adapter:
            return
        if self.live or self._ready or self._groups or self._carry or self.waiting:
            raise RuntimeError("the LoRA adapter cannot change while chains are live or waiting")
        self.model.set_adapter(adapter)
        self._features.clear()
        self.parked.clear()   # (a parked slot belongs to a waiting follow-up: there is none)

    def close(self) -> None:
        """Gives back what the scheduler created on the engine: the prefix pool of `prefix_cache_rows` (a `prefix_cache` object
        handed in stays its owner's).  A scheduler without a cache has nothing to close."""
        if self._owns_prefix_cache and self.prefix_cache is not None:
            self.prefix_cache.close()
        self.prefix_cache, self._owns_prefix_cache = None, False

    # ------------------------------------------------------------------ queue
    def submit(self, req: Request) -> None:
        n = getattr(req, "n", 1)
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not (1 <= n <= self.engine.max_seqs):
            raise ValueError(f"`n` has to be an integer in [1, {self.engine.max_seqs}] (the engine's chain slots), but is {n!r}")
        if n > 1:
            sampled = self.do_sample if req.do_sample is None else bool(req.do_sample)
            temperature = self.temperature if req.temperature is None else float(req.temperature)
            if not (sampled and temperature > 0.0):
                raise ValueError(f"n = {n} completions need a sampled request (do_sample with a temperature > 0): greedy ones are all the same")
        self.waiting.append(req)

    # -- parallel sampling: one request, n completions
    @staticmethod
    def _completion(req: Request, i: int) -> Request:
        """The request object of completion i of `req`: its fields, `index`, `parent`, the stream `stream_id + i`, results of its own."""
        c = copy.copy(req)
        c.n, c.index, c.parent, c.stream_id, c.slot = 1, i, req, req.stream_id + i, -1
        c.tokens, c.text, c.token_logprobs, c.top_logprobs = [], "", [], []
        return c

    @staticmethod
    def _take_forks(req):
        """The siblings `req` (an anchor) still has to fork, each with its pinned slot; they are nobody's afterwards."""
        forks = getattr(req, "_forks", None) or []
        if forks:
            req._forks = []
        return forks

    def _fork(self, req, ids, keys) -> None:
        """Behind the anchor's pass, on its stream: its pinned siblings become the chain it is (ze_seq_fork: K/V rows, logits, marks)
        and wait with it for their first draw.  A failure is the siblings' alone -- slots back, on_error each; the anchor goes on."""
        forks = self._take_forks(req)
        if not forks:
            return
        try:
            self.engine.seq_fork(req.slot, [k.slot for k in forks])
        except Exception as ex:
            self._fail_all(forks, ex)
            return
        for k in forks:
            k._chain, k.n_prompt = req._chain, req.n_prompt
            if req._chain.wants_prompt_logprobs:   # computed once, by the anchor's pass: shared by reference
                k._prompt_ids = req._prompt_ids
                k.prompt_token_logprobs, k.prompt_ranks, k.prompt_top_logprobs = (req.prompt_token_logprobs, req.prompt_ranks,
                                                                                  req.prompt_top_logprobs)
            self._ready.append((k, ids, keys))
        self.stats["forked_chains"] += len(forks)
        self.stats["forked_rows"] += len(forks) * len(ids)

    def pending_requests(self):
        """Every request the scheduler holds, whatever its state (a caller that gives up on the engine fails them all)."""
        reqs = [l.req for l in self.live.values()] + list(self.waiting) + [r for r, _, _ in self._ready]
        reqs += [it["req"] for g in list(self._groups) + [self._carry] for it in g if it.get("final", True)]
        reqs += [k for r in list(reqs) for k in (getattr(r, "_forks", None) or [])]   # (siblings that wait for their anchor's pass)
        return reqs

    def busy(self) -> bool:
        return bool(self.waiting or self.live or self._groups or self._ready or self._carry)

    def run(self) -> None:
        while self.busy():
            self.step()
        tr = self._trace_ev
        if tr is not None and tr["passes"]:
            torch.cuda.synchronize()
            with open(os.environ["ZE_SCHED_TRACE"], "a") as f:
                for host_s, a, b in tr["passes"]:
                    f.write(f"{id(self) % 100000} {tr['t0']:.4f} G {host_s:.4f} {tr['base'].elapsed_time(a) / 1e3:.4f} {tr['base'].elapsed_time(b) / 1e3:.4f}\n")

    # ------------------------------------------------------------------ one scheduling round
    def step(self) -> None:
        tp = time.perf_counter
        t0 = tp()
        if self._side is not None:
            # what the caller put on ITS stream before submitting (the tile upload, the view's resize) is read by the
            # admission work on the side stream: order the two here, while the caller's stream holds nothing else
            self._side.wait_stream(torch.cuda.current_stream(self.engine.device))
        hold = self._round_in_progress() and len(self.live) < self.hold_below
        handle = self._burst_begin() if (self.live and self.overlap and not hold) else None
        t1 = tp()
        with self._side_stream():
            if not self._groups:
                self._admit()
            t2 = tp()
            if self._groups:
                self._run_group(self._groups.popleft())
                if handle is not None:
                    self.stats["overlapped_passes"] += 1
        t3 = tp()
        if handle is not None:
            self._burst_end(handle)
        t4 = tp()
        more = bool(self._carry or (self.admit_chunk_rows and self.waiting and self.waiting[0].slot < 0 and self.free))
        self._join_ready(wait=hold and not self._groups and not more)   # (held with nothing left to enqueue: wait for the oldest pass)
        if handle is None:   # (nothing was decoding beside the pass: the round may just have begun, or been completed)
            hold = self._round_in_progress() and len(self.live) < self.hold_below
            if self.live and not hold:
                self._burst()
        if hold:
            self.stats["held_steps"] = self.stats.get("held_steps", 0) + 1
        t5 = tp()
        st = self.stats   # host seconds of the scheduling round by part (burst_end = waiting for the GPU + retiring + the callbacks)
        for k, v in (("host_s_burst_begin", t1 - t0), ("host_s_admit", t2 - t1), ("host_s_pass", t3 - t2), ("host_s_burst_end", t4 - t3),
                     ("host_s_join", t5 - t4)):
            st[k] = st.get(k, 0.0) + v

    @staticmethod
    def _first_image_key(req):
        """What tells two requests about the same view apart from two about different ones, before anything is tokenised: the
        first image object itself (the entry points hand every question of a tile the same view object), by value where it has one."""
        if not req.images:
            return None
        im = req.images[0]
        return im if isinstance(im, (str, int, tuple)) else id(im)

    def _round_in_progress(self) -> bool:
        """Passes still to run, prefilled chains still to join -- or, when admitting in chunks, requests the next call of _admit can take."""
        if self._groups or self._ready or self._carry:
            return True
        # (FRESH requests only: a follow-up that waits for its pass is the steady state of a running stream, not a round being admitted)
        return bool(self.admit_chunk_rows and self.waiting and self.waiting[0].slot < 0 and self.free)

    def _side_stream(self):
        """Admission work (front-end, ViT, prefill, the callbacks' crops) runs on the side stream when overlapping."""
        return torch.cuda.stream(self._side) if self._side is not None else contextlib.nullcontext()

    # -- admission: waiting requests take free slots (a follow-up keeps the slot its predecessor parked)
    def _admit(self) -> None:
        e = self.engine
        # (admitting in chunks: the rest of a queue whose first chunks are already in is not "a few newcomers" -- no waiting for more)
        chunking = bool(self._carry or (self.admit_chunk_rows and self.waiting and self.waiting[0].slot < 0 and self.free))
        if self.live and self.min_admit > 1 and not chunking:
            ready = sum(1 for r in self.waiting if r.slot >= 0) + min(len(self.free), sum(1 for r in self.waiting if r.slot < 0))
            if 0 < ready < self.min_admit and self._waited < self.max_wait_bursts:
                self._waited += 1
                return
        self._waited = 0
        # tokenise / preprocess each newcomer as it leaves the queue; collect the images whose features are not cached
        prepared, todo, needed = [], OrderedDict(), set()
        if self._carry and self._round is not None:   # (items held back from the last chunk keep their images' entries)
            todo, needed = OrderedDict(self._round[0]), set(self._round[1])
        rows_planned, last_img = 0, None
        while self.waiting:
            req = self.waiting[0]
            if self.admit_chunk_rows and rows_planned >= self.admit_chunk_rows and prepared:
                first = self._first_image_key(req)
                if first is None or first != last_img:
                    break                                      # a pass's worth is planned and the next request is about another tile
            if req.slot < 0:
                if not self.free:
                    break
                req.slot = self.free.pop()
            self.waiting.popleft()
            last_img = self._first_image_key(req)
            if getattr(req, "n", 1) > 1:
                # n completions: completion 0 is the anchor -- it takes the slot and goes through the round like any request --
                # and carries the others until its pass has run (below: slots; _prefill: the fork)
                kids = [self._completion(req, i) for i in range(req.n)]
                kids[0].slot, kids[0]._forks = req.slot, kids[1:]
                req = kids[0]
            try:
                req._chain = self._resolve(req)   # once per request: every later stage of the chain's life reads it
                inp = self.processor(text=[req.prompt], images=list(req.images) or None, return_tensors="pt")
                ids = inp["input_ids"][0].tolist()
                grids = inp["image_grid_thw"].tolist() if req.images else []
                keys = list(inp.get("image_keys", []))
                mu = self.model.config.vision.spatial_merge_size ** 2
                n_img_tok = sum(g[0] * g[1] * g[2] // mu for g in grids)
                if ids.count(self.model.config.image_token_id) != n_img_tok:
                    raise ValueError("Image features and image tokens do not match")
                if len(ids) + 1 > e.max_ctx:
                    raise ValueError(f"prompt of {len(ids)} tokens exceeds max_ctx = {e.max_ctx}")
                rows = np.concatenate([[0], np.cumsum([g[0] * g[1] * g[2] for g in grids])]).astype(int)
                if len(grids) and int(np.diff(rows).max()) > e.max_patches:
                    raise ValueError(f"image of {int(np.diff(rows).max())} patches exceeds max_patches = {e.max_patches}")
                reuse, n_reused = self._reusable(req.slot, ids, keys)
                for i in range(n_reused, len(grids)):
                    if keys[i] in self._features:
                        self._features.move_to_end(keys[i])   # needed this round: not an eviction candidate
                    elif keys[i] not in todo:
                        todo[keys[i]] = (inp["pixel_values"][rows[i]:rows[i + 1]], grids[i])
                    needed.add(keys[i])
                prepared.append(dict(req=req, ids=ids, grids=grids, keys=keys, reuse=reuse, n_reused=n_reused, copy_from=None,
                                     upto=len(ids), final=True))
                rows_planned += len(ids) - reuse
                if getattr(req, "_forks", None):
                    # The siblings' slots leave `free` NOW and are in nobody's reach until the fork takes them: a slot that is
                    # only remembered while it sits in `free` is handed to the next newcomer (free.pop() is LIFO; items carried
                    # over chunks of admit_chunk_rows live across several calls).  Siblings without a slot become ordinary
                    # requests of the same prompt and stream at the head of the queue: the shared-prefix path brings them in
                    # later, with the same bits.
                    forks, overflow = [], []
                    for k in req._forks:
                        if self.free:
                            k.slot = self.free.pop()
                            forks.append(k)
                        else:
                            overflow.append(k)
                    req._forks = forks
                    self.waiting.extendleft(reversed(overflow))
            except Exception as ex:  # a malformed request must not take the batch down
                self._fail(req, ex)
        if not prepared and not self._carry:
            return
        # The round's prefill passes: rows of several chains share every GEMM, up to max_prefill_rows per pass; pass A (the
        # prefixes that other newcomers of this round will copy) goes first.  One pass runs per step (beside the decode burst
        # when overlapping); each encodes the images it needs that are not cached yet -- ONE multi-resolution ViT call.
        try:
            anchors = self._plan_sharing(prepared) if self.share_prefix else []
        except Exception as ex:
            self._fail_all([p["req"] for p in prepared if p["req"].slot >= 0], ex)
            return
        self._round = (todo, needed)
        carried, self._carry = self._carry, []
        for which, items in (("A", anchors), ("B", carried + prepared)):
            group, rows = [], 0
            for item in items + [None]:
                if group and (item is None or rows + item["upto"] - item["reuse"] > e.max_prefill_rows):
                    # admitting in chunks: the last, partial pass of a chunk waits for the next chunk's items (passes stay full)
                    if (item is None and which == "B" and self.admit_chunk_rows and rows < 0.85 * e.max_prefill_rows
                            and self.waiting and (self.waiting[0].slot >= 0 or self.free)):
                        self._carry = group
                    else:
                        self._groups.append(group)
                    group, rows = [], 0
                if item is not None:
                    group.append(item)
                    rows += item["upto"] - item["reuse"]
        if not self.overlap:  # everything at once: one ViT call per round, then the passes back to back
            while self._groups:
                self._run_group(self._groups.popleft())

    def _run_group(self, group) -> None:
        """One prefill pass of the round, behind the ViT call for its uncached images.  A failure (the ViT call, the pass)
        must not orphan a request that already left `waiting`: whatever escapes fails every request of the pass -- slots
        freed, on_error called."""
        todo, needed = self._round
        try:
            if self.overlap:
                want = OrderedDict()
                for it in group:
                    for k in it["keys"]:
                        if k in todo and k not in want:
                            want[k] = todo.pop(k)
                self._encode(want, needed)
            elif todo:
                self._encode(OrderedDict(todo), needed)
                todo.clear()
            n0 = len(self._ready)
            tr = self._trace_ev
            if tr is not None and len(tr["passes"]) < 4 and self._side is not None:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(self._side)
                self._prefill(group)
                b.record(self._side)
                tr["passes"].append((time.perf_counter() - tr["t0"], a, b))
            else:
                self._prefill(group)
            if self._side is not None and len(self._ready) > n0:
                # the pass's own event: its chains may join the live set as soon as THIS pass is over, whatever else the
                # admission stream has been given since
                ev = torch.cuda.Event()
                ev.record(self._side)
                self._pass_done.extend([ev] * (len(self._ready) - n0))
        except Exception as ex:
            for it in group:
                self._unpin(it)
            self._fail_all([it["req"] for it in group if it["req"].slot >= 0 and it["req"].slot not in self.live
                            and not any(r is it["req"] for r, _, _ in self._ready)], ex)

    # -- shared prompt prefixes
    def _prefix_len(self, a, b) -> int:
        return shared_prefix_len(a, b, self.model.config.image_token_id)

    def _images_in(self, ids, n) -> int:
        return images_in(ids, n, self.model.config.image_token_id)

    def _plan_sharing(self, prepared):
        """Decides, for every fresh chain of the round, where its leading K/V rows come from; returns the pass-A items."""
        # (a chain that asked for prompt log-probabilities computes every row itself: it takes no prefix and, within its round, is
        # no anchor either -- an anchor's prefix goes through a pass of its own; alive or parked it donates like any other chain)
        fresh = [p for p in prepared if p["reuse"] == 0 and p["keys"] and all(k is not None for k in p["keys"])
                 and not p["req"]._chain.wants_prompt_logprobs]
        cache = self.prefix_cache
        if cache is not None:
            # what the pool holds of every fresh chain's prompt (text-only prompts too: the pool needs no image to group by)
            for p in prepared:
                if p["reuse"] == 0 and not p["req"]._chain.wants_prompt_logprobs:
                    p["cache"] = cache.match(p["ids"], p["keys"])
        if not fresh:
            if cache is not None:
                self._plan_cache(prepared)
            return []
        donors = {}   # first image key -> [(slot, ids, keys)]: chains that hold their prompt's K/V rows right now
        taken = {p["req"].slot for p in prepared}
        for slot, l in self.live.items():
            if l.keys and slot not in taken:
                donors.setdefault(l.keys[0], []).append((slot, l.ids, l.keys))
        for slot, (pids, pkeys, _gen) in self.parked.items():
            if pkeys:
                donors.setdefault(pkeys[0], []).append((slot, pids, pkeys))
        groups = OrderedDict()
        for p in fresh:
            groups.setdefault(p["keys"][0], []).append(p)
        anchors = []
        for k0, members in groups.items():
            rest = members
            for slot, dids, dkeys in donors.get(k0, []):   # an existing chain: every member that matches it copies from it
                for p in list(rest):
                    n = self._prefix_len(p["ids"], dids)
                    ni = self._images_in(p["ids"], n)
                    if n >= self.min_shared and tuple(p["keys"][:ni]) == tuple(dkeys[:ni]):
                        p.update(copy_from=slot, reuse=n, n_reused=ni)
                        rest = [q for q in rest if q is not p]
                if not rest:
                    break
            if cache is not None:
                # a live holder first (the decode attention shares it), then the round's own anchor; the pool where it covers more
                # rows than the donor does, or as many as the anchor's pass would compute
                n = self._anchor_prefix(rest)[0]
                for p in members:
                    self._plan_cache([p], floor=n if any(q is p for q in rest) else None)
                rest = [p for p in rest if not p.get("cached")]
            n, ni = self._anchor_prefix(rest)
            if not n:
                continue
            ref = rest[0]                                   # no donor yet: the first member's prefix is prefilled alone
            anchors.append(dict(ref, upto=n, final=False))
            ref.update(reuse=n, n_reused=ni, copy_from=-1)   # -1: the rows are already in its own slot after pass A
            for p in rest[1:]:
                p.update(copy_from=ref["req"].slot, reuse=n, n_reused=ni)
        if cache is not None:
            self._plan_cache([p for p in prepared if not any(q is p for q in fresh)])
        return anchors

    def _anchor_prefix(self, rest):
        """(rows, images) of the prefix the first of `rest` would prefill alone for the others to copy; (0, 0): no such prefix."""
        if len(rest) < 2:
            return 0, 0
        ref = rest[0]
        n = min(self._prefix_len(ref["ids"], p["ids"]) for p in rest[1:])
        ni = self._images_in(ref["ids"], n)
        if n < self.min_shared or any(tuple(p["keys"][:ni]) != tuple(ref["keys"][:ni]) for p in rest[1:]):
            return 0, 0
        return n, ni

    def _plan_cache(self, items, floor=None) -> None:
        """The items whose prompt the pool covers for more rows than their planned source does (and for `floor` rows at least) take
        them from the pool; the match stays pinned until its load is enqueued (or the request fails)."""
        for p in items:
            m = p.get("cache")
            if m and not p.get("cached") and m.rows > p["reuse"] and m.rows >= (floor or 0):
                self.prefix_cache.pin(m)
                p.update(copy_from=None, reuse=m.rows, n_reused=m.images, cached=m)

    def _reusable(self, slot, ids, keys):
        """(cached prefix length, images inside it) when the slot's parked chain is a strict prefix of `ids`.  With
        `reuse_generated` the prefix extends over the tokens the parked chain GENERATED for as long as the new prompt
        repeats them id for id (stage 2 re-inserts the stage-1 output: src/eval/infer.py:222): their K/V rows were written
        by the decode steps and are kept instead of being prefilled again."""
        rec = self.parked.pop(slot, None)
        if rec is None:
            return 0, 0
        pids, pkeys, gen = rec
        n = len(pids)
        cfg = self.model.config
        if 0 < n < len(ids) and tuple(ids[:n]) == pids and tuple(keys[: len(pkeys)]) == pkeys \
                and ids[n] != cfg.image_token_id and all(k is not None for k in pkeys):
            special = (cfg.image_token_id, getattr(cfg, "vision_start_token_id", None), getattr(cfg, "vision_end_token_id", None))
            m = 0
            while m < len(gen) and n + m < len(ids) - 1 and ids[n + m] == gen[m] and gen[m] not in special:
                m += 1
            self.stats["reused_generated_rows"] += m
            self.stats["generated_rows_offered"] = self.stats.get("generated_rows_offered", 0) + max(0, min(len(gen), len(ids) - 1 - n))
            return n + m, len(pkeys)
        return 0, 0

    def _encode(self, todo, needed=()) -> None:
        """ONE multi-resolution ViT call (per max_patches worth of images) for the uncached images of this round."""
        e = self.engine
        items = list(todo.items())
        i = 0
        while i < len(items):
            j, n = i, 0
            while j < len(items) and (j == i or n + items[j][1][0].shape[0] <= e.max_patches):
                n += items[j][1][0].shape[0]
                j += 1
            pvs = [it[1][0] for it in items[i:j]]
            grids = [it[1][1] for it in items[i:j]]
            feats = e.vit_forward((torch.cat(pvs) if len(pvs) > 1 else pvs[0]).contiguous(), grids)
            self.stats["vit_calls"] += 1
            self.stats["vit_images"] = self.stats.get("vit_images", 0) + len(grids)
            self.stats["vit_patches"] = self.stats.get("vit_patches", 0) + int(n)
            off = 0
            mu = self.model.config.vision.spatial_merge_size ** 2
            for (key, (_, g)) in items[i:j]:
                k = g[0] * g[1] * g[2] // mu
                self._features[key] = feats[off:off + k]
                off += k
            i = j
        # LRU eviction, never of a feature this round's prefills are about to read
        for key in list(self._features.keys()):
            if len(self._features) <= max(self._feature_cap, len(needed)):
                break
            if key not in needed:
                del self._features[key]

    def _prefill(self, group) -> None:
        e = self.engine
        slots, ids_l, emb_l, pos_l, dl = [], [], [], [], []
        ok = []
        # members of the pass with the same match in the prefix cache: ONE ze_prefix_load for all of them, at the first one's turn
        loads = {}
        for it in group:
            if it.get("cached") and it["req"].slot >= 0:
                loads.setdefault((it["cached"].blocks, it["cached"].rows), dict(items=[], state=None))["items"].append(it)
        for it in group:
            req, ids, grids, keys, reuse, n_reused, upto = (it["req"], it["ids"], it["grids"], it["keys"], it["reuse"],
                                                           it["n_reused"], it["upto"])
            if req.slot < 0:
                self._unpin(it)
                continue                                       # failed earlier in this round (pass A)
            if it["copy_from"] is not None and e.seq_len(it["copy_from"] if it["copy_from"] >= 0 else req.slot) < reuse:
                # the donor's rows are gone (its pass failed; _fail resets the slot, so a stale context of the slot's
                # previous occupant cannot pass for them): prefill in full
                it["copy_from"], reuse, n_reused = None, 0, 0
                it.update(reuse=0, n_reused=0)
            try:
                pos, delta = e.rope_index(ids, grids)
                n_upto = len(keys) if upto == len(ids) else self._images_in(ids, upto)   # pass A stops after the prefix
                feats = [self._features[k] for k in keys[n_reused:n_upto]]
                for k in keys[n_reused:n_upto]:
                    self._features.move_to_end(k)
                emb = (torch.cat(feats) if len(feats) > 1 else feats[0]) if feats else None
                if it.get("cached"):
                    self._load_cached(loads[(it["cached"].blocks, it["cached"].rows)], it)
                elif it["copy_from"] is None:
                    if reuse:
                        e.seq_truncate(req.slot, reuse)       # a follow-up on its own slot: keep the cached prompt
                    else:
                        e.seq_reset(req.slot)
                elif it["copy_from"] >= 0:                     # shared prefix: the rows of another chain
                    e.seq_reset(req.slot)
                    e.seq_copy_prefix(req.slot, it["copy_from"], reuse)
                    self.stats["shared_rows"] += reuse
                # (copy_from == -1: pass A left the prefix in this slot)
                slots.append(req.slot)
                ids_l.append(ids[reuse:upto])
                emb_l.append(emb)
                pos_l.append(pos[:, reuse:upto])
                dl.append(delta)
                ok.append(it)
            except Exception as ex:
                self._unpin(it)
                self._fail(req, ex)
        if not ok:
            return
        final = [it for it in ok if it["final"]]                # (pass A: the chain is completed by pass B)
        try:
            # (a request with a repetition penalty of its own is marked by ITS value: 1.0 reads no set)
            marked = [it for it in final if it["req"]._chain.effective_penalty != 1.0]
            if marked:
                # the prompts' ids into the repetition-penalty sets (cleared by the reset / truncate above): one copy and one
                # launch for the pass, IN FRONT of it -- behind it, the next call would find its staging buffer busy until the
                # whole pass has run
                if hasattr(e, "mark_seen_batch") and not _PER_CHAIN:
                    e.mark_seen_batch([it["req"].slot for it in marked], [it["ids"] for it in marked])
                else:
                    for it in marked:
                        e.mark_seen(it["req"].slot, it["ids"])
            asking = [k for k, it in enumerate(ok) if it["final"] and it["req"]._chain.wants_prompt_logprobs]
            if asking:
                # the scoring form of the pass: the askers from their first new row on, everybody else from the last row, which
                # contributes nothing -- their tokens and state are those of prefill_batch
                sf = [0 if k in asking else len(ids_l[k]) - 1 for k in range(len(ok))]
                top = max(ok[k]["req"]._chain.prompt_logprobs for k in asking)
                det = e.score_batch_detail(slots, ids_l, emb_l, pos_l, dl, score_from=sf, top_n=top, rank=True)
                for k in asking:
                    self._attach_prompt_logprobs(ok[k]["req"], ok[k]["ids"], ok[k]["reuse"], det.chain(k))
            else:
                e.prefill_batch(slots, ids_l, emb_l, pos_l, dl)
        except Exception as ex:
            self._fail_all([it["req"] for it in ok], ex)
            return
        self.stats["prefill_rows"] += sum(len(x) for x in ids_l)
        if os.environ.get("ZE_SCHED_TRACE"):   # measurement only
            with open(os.environ["ZE_SCHED_TRACE"], "a") as f:
                f.write(f"{id(self) % 100000} {time.perf_counter():.4f} P {len(slots)} {sum(len(x) for x in ids_l)}\n")
        for it in final:
            req, ids, keys = it["req"], it["ids"], it["keys"]
            req.n_prompt = len(ids)
            req.cached_tokens = it["reuse"]                     # rows the request did not compute: a donor's, the pool's, its own slot's
            self._ready.append((req, tuple(ids), tuple(keys)))
            self._fork(req, tuple(ids), tuple(keys))

    # -- prefix cache
    def _unpin(self, it) -> None:
        m = it.pop("cached", None)
        if m:
            self.prefix_cache.unpin(m)

    def _load_cached(self, load, it) -> None:
        """The pool's rows into the slots of every member of the pass that shares `it`'s match: enqueued once, at the turn of the
        first member to get this far, on the admission stream in front of the tails' pass; a failure is every member's."""
        if load["state"] is None:
            m, cfg = it["cached"], self.model.config
            end = getattr(cfg, "vision_end_token_id", None)
            # (the split row a prefill of these tokens notes: the row behind their first image block)
            split = next((t + 1 for t in range(m.rows) if it["ids"][t] == end), 0) if end is not None and end >= 0 else 0
            slots = [it["req"].slot] + [q["req"].slot for q in load["items"] if q is not it and q["req"].slot >= 0]
            try:
                self.prefix_cache.load(m, slots, split if split < 65536 else 0)
                load["state"] = True
                self.stats["prefix_cache_hit_rows"] += m.rows * len(slots)
            except Exception as ex:
                load["state"] = ex
        self._unpin(it)
        if load["state"] is not True:
            raise load["state"]

    def _save_to_cache(self, slot: int, ids, keys, n_rows: int) -> None:
        """A chain leaves its slot: the full blocks of its first n_rows rows that the pool does not hold yet are copied there, before
        the slot is retired or reset.  The decode steps that wrote the rows are over (the burst was collected), so the copy runs on
        the admission stream, ahead of whatever that stream writes into the slot next."""
        cache = self.prefix_cache
        if cache is None or n_rows < cache.block_rows:
            return
        try:
            evicted = cache.stats["evicted_blocks"]
            saved = cache.save(slot, ids, keys, n_rows, stream=self._side)
            self.stats["prefix_cache_saved_rows"] += saved
            self.stats["prefix_cache_evicted_blocks"] += cache.stats["evicted_blocks"] - evicted
        except Exception as ex:
            # the cache is an optimisation -- a chain that cannot be saved is recomputed next time and no request fails for it -- but
            # the failure is counted and kept, not lost
            self.stats["prefix_cache_save_errors"] += 1
            self.prefix_cache_last_error = ex

    def _resolve(self, req) -> ChainRequest:
        """The request's optional fields merged with the scheduler's defaults: its own value, else the scheduler's, else off.  A
        request that names none of the four sampling values carries none (it never reaches `set_sampling` and follows the
        scheduler's gen_params); the filter counts only for an effective sampled mode; the token rules have no defaults."""
        def pick(name, mine=None):   # (`mine`: the scheduler's attribute where its name differs)
            v = getattr(req, name, None)
            return getattr(self, mine or name) if v is None else v
        own = any(getattr(req, k, None) is not None for k in ("do_sample", "temperature", "seed", "repetition_penalty"))
        sampled, penalty = bool(pick("do_sample")), float(pick("repetition_penalty", "penalty"))
        top_p, logprobs = pick("top_p"), pick("logprobs")
        typical_p, epsilon_cutoff, eta_cutoff = pick("typical_p"), pick("epsilon_cutoff"), pick("eta_cutoff")
        for name, v, ok in (("typical_p", typical_p, lambda x: 0.0 < x <= 1.0), ("epsilon_cutoff", epsilon_cutoff, lambda x: 0.0 <= x < 1.0),
                            ("eta_cutoff", eta_cutoff, lambda x: 0.0 <= x < 1.0)):
            if v is not None and not ok(float(v)):
                raise ValueError(f"`{name}` has to be a float > 0 and < 1, but is {v}")
        chain = ChainRequest(
            sampling=(sampled, float(pick("temperature")), int(pick("seed")), penalty) if own else None,
            sampled=sampled, effective_penalty=penalty,
            top_k=int(pick("top_k") or 0), top_p=float(1.0 if top_p is None else top_p), min_p=float(pick("min_p") or 0.0),
            typical_p=float(1.0 if typical_p is None else typical_p), epsilon_cutoff=float(epsilon_cutoff or 0.0), eta_cutoff=float(eta_cutoff or 0.0),
            logprobs=None if logprobs is None else int(logprobs),
            prompt_logprobs=None if getattr(req, "prompt_logprobs", None) is None else int(req.prompt_logprobs),
            presence_penalty=float(pick("presence_penalty") or 0.0), frequency_penalty=float(pick("frequency_penalty") or 0.0),
            min_new_tokens=int(pick("min_new_tokens") or 0), logit_bias=pick("logit_bias") or {},
            no_repeat_ngram_size=int(getattr(req, "no_repeat_ngram_size", None) or 0),
            stop_ids=list(getattr(req, "stop_ids", None) or ()), bad_words_ids=list(getattr(req, "bad_words_ids", None) or ()))
        return self._with_speculation(req, chain)

    def _with_speculation(self, req, chain: ChainRequest) -> ChainRequest:
        """The request's speculative_tokens, else the scheduler's -- which yields to whatever of the request excludes it, while a
        request that names both is refused."""
        own = getattr(req, "speculative_tokens", None)
        k = self.speculative_tokens if own is None else own
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not (0 <= k <= 8):
            raise ValueError(f"`speculative_tokens` has to be an integer in [0, 8], but is {k!r}")
        if not k:
            return chain
        sampling = getattr(req, "speculative_sampling", None)
        sampling = self.speculative_sampling if sampling is None else bool(sampling)
        chain = dataclasses.replace(chain, speculative_sampling=sampling)
        what = chain.speculation_conflict(grammar=self._grammar_key(req) is not None)
        if what is not None:
            if own is None:
                return chain
            raise ValueError(f"`speculative_tokens` is greedy speculative decoding and cannot be combined with {what}")
        if self.max_batch > 64:
            raise ValueError("speculative decoding runs on the fragment kernels: max_batch <= 64")
        return dataclasses.replace(chain, speculative_tokens=int(k), ngram_min=self.ngram_min, ngram_max=self.ngram_max)

    def _spec_budget(self, k: int) -> int:
        """The k a joining chain gets: the rows of a step, sum of 1 + k over the live chains, stay <= 64 with one row left for every
        slot that may still fill."""
        used = sum(1 + l.req._chain.speculative_tokens for l in self.live.values())
        return max(0, min(int(k), 64 - used - 1 - (self.max_batch - len(self.live) - 1)))

    @staticmethod
    def _grammar_key(req):
        regex, choice = getattr(req, "guided_regex", None), getattr(req, "guided_choice", None)
        if regex is None and choice is None:
            return None
        if regex is not None and choice is not None:
            raise ValueError("`guided_regex` and `guided_choice` exclude each other")
        return ("regex", regex) if regex is not None else ("choice", tuple(choice) if isinstance(choice, (list, tuple)) else choice)

    def _set_grammar(self, req) -> None:
        """The request's grammar into its slot (cleared, like the filter, by the slot's reset / truncate / prefix copy), before its
        first draw; without one nothing is launched.  Raises when the pattern does not compile or every grammar is in use."""
        key = self._grammar_key(req)
        if key is None:
            return
        if getattr(self, "grammars", None) is None:
            def compile_key(k):
                kw = {"guided_regex": k[1]} if k[0] == "regex" else {"guided_choice": list(k[1]) if isinstance(k[1], tuple) else k[1]}
                return self.model.compile_grammar(tokenizer=self.processor.tokenizer, **kw)
            from .engine import MAX_GRAMMARS
            self.grammars = GrammarCache(self.engine, compile_key, MAX_GRAMMARS)
        gid = self.grammars.acquire(key)
        req._grammar_key = key
        self.engine.set_grammar(req.slot, gid)

    def _drop_grammar(self, req) -> None:
        """The chain is over: its slot lets go of the grammar, which may be evicted from now on."""
        key = getattr(req, "_grammar_key", None)
        if key is not None:
            req._grammar_key = None
            self.grammars.release(key)
            try:
                self.engine.set_grammar(req.slot, None)
            except Exception:
                pass

    @staticmethod
    def _attach_prompt_logprobs(req, ids, reuse: int, det) -> None:
        """The scored positions of the request's pass into its prompt lists: new row j predicts prompt token reuse + j + 1."""
        n, N = len(ids), req._chain.prompt_logprobs
        req._prompt_ids = list(ids)
        lps, ranks = det.logps.cpu().tolist(), det.rank.cpu().tolist()
        tids = det.top_ids.cpu().tolist() if det.top_ids is not None else None
        tlps = det.top_logprobs.cpu().tolist() if det.top_logprobs is not None else None
        req.prompt_token_logprobs, req.prompt_ranks, req.prompt_top_logprobs = [None] * n, [None] * n, [None] * n
        for j, (lp, rk) in enumerate(zip(lps, ranks)):
            t = reuse + j + 1
            req.prompt_token_logprobs[t], req.prompt_ranks[t] = float(lp), int(rk)
            req.prompt_top_logprobs[t] = [(int(i), float(v)) for i, v in zip(tids[j][:N], tlps[j][:N]) if int(i) >= 0] if N and tids else []

    @staticmethod
    def _attach_logprobs(req, lp, n: int) -> None:
        logps, ids, tlps = lp
        m = len(req.tokens)
        req.token_logprobs = [float(x) for x in logps[:m]]
        req.top_logprobs = [[(int(i), float(v)) for i, v in zip(ids[t][:n], tlps[t][:n]) if int(i) >= 0] for t in range(m)]

    def _join_ready(self, wait: bool = False) -> None:
        """The prefilled newcomers draw their first token (from the logits their pass left) and join the live set.  When
        overlapping, a pass that is still running does not hold the live chains up: they go into their next burst, the
        newcomers join behind a later one (with nothing live, the call waits for the oldest pass)."""
        if not self._ready:
            return
        keep_from = len(self._ready)
        if self._side is not None:
            if len(self._pass_done) != len(self._ready):   # (entries without an event: wait for everything, as before)
                self._side.synchronize()
                self._pass_done = [None] * len(self._ready)
            for i, ev in enumerate(self._pass_done):
                if ev is not None and not ev.query():
                    if i == 0 and (wait or not self.live):
                        ev.synchronize()                    # nothing to decode meanwhile
                        continue
                    keep_from = i
                    break
        for req, ids, keys in self._ready[:keep_from]:
            if req._chain.speculative_tokens:   # the step's 64 rows: this chain's k as the live set leaves room for it
                req._chain = dataclasses.replace(req._chain, speculative_tokens=self._spec_budget(req._chain.speculative_tokens))
            req._chain.install(self.engine, req.slot, ids)
            if self.prefix_cache is not None:
                req._prefilled = (ids, keys)   # (_release: the rows of a chain that got this far are worth keeping)
            try:
                self._set_grammar(req)
            except Exception as ex:   # no grammar to be had (a bad pattern, or all in use): this request fails, the round goes on
                self._fail(req, ex)
                continue
            self.engine.chain_begin(req.slot, self.params, req.stream_id)
            self.live[req.slot] = _Live(req, ids, keys)
            self.stats["admitted"] += 1
        if keep_from < len(self._ready):
            self.stats["deferred_joins"] = self.stats.get("deferred_joins", 0) + 1
        self._ready = self._ready[keep_from:]
        self._pass_done = self._pass_done[keep_from:]

    # histogram of the decode steps by their live-chain count (the row count of the step's GEMMs picks their tiles: which
    # buckets the stream spends its steps in says which tile is worth work); keys `steps_le_<bound>`
    _ROW_BOUNDS = (64, 128, 192, 256, 320, 384, 416, 448, 512, 640, 768)

    def _tally_step_rows(self, ran: int, n: int) -> None:
        if ran <= 0:
            return
        if os.environ.get("ZE_SCHED_TRACE"):   # measurement only: one line per burst (tools/sched_trace.py draws the occupancy)
            with open(os.environ["ZE_SCHED_TRACE"], "a") as f:
                f.write(f"{id(self) % 100000} {time.perf_counter():.4f} B {n} {ran} {len(self.waiting)} {len(self._groups)} {len(self._ready)}\n")
        b = next((x for x in self._ROW_BOUNDS if n <= x), None)
        k = f"steps_le_{b}" if b is not None else "steps_gt_768"
        self.stats[k] = self.stats.get(k, 0) + ran

    # -- one burst of decode steps for every live chain, then retire the finished ones
    def _burst(self) -> None:
        e = self.engine
        slots = list(self.live.keys())
        steps = self._burst_steps()
        ran, n_gen, fin = e.decode_burst(slots, steps, self.params)
        self.stats["bursts"] += 1
        self.stats["steps"] += ran
        self.stats["chain_steps"] += ran * len(slots)
        self._tally_step_rows(ran, len(slots))
        self._retire_finished(slots, n_gen, fin)

    def _retire_finished(self, slots, n_gen, fin) -> None:
        """The chains the burst finished leave the live set: their ids come over in ONE copy (chain_tokens_batch), then the
        callbacks run."""
        e = self.engine
        out = []
        for slot, ng, f in zip(slots, n_gen, fin):
            l = self.live[slot]
            l.produced = ng
            if f or ng >= min(l.req.max_new_tokens, e.max_ctx - l.req.n_prompt + 1):
                out.append(slot)
        toks = None
        if len(out) > 1 and hasattr(e, "chain_tokens_batch") and not _PER_CHAIN:
            ds = getattr(self, "_decode_stream", None)
            cap = max(self.live[s].req.max_new_tokens for s in out)
            toks = e.chain_tokens_batch(out, cap, stream=ds) if ds is not None else e.chain_tokens_batch(out, cap)
        lps = {}
        want = [s for s in out if self.live[s].req._chain.wants_logprobs]
        if len(want) > 1 and hasattr(e, "chain_logprobs_batch") and not _PER_CHAIN:   # the same for their log-probabilities
            ds = getattr(self, "_decode_stream", None)
            cap = max(self.live[s].req.max_new_tokens for s in want)
            top = max(self.live[s].req._chain.logprobs for s in want)
            lps = dict(zip(want, e.chain_logprobs_batch(want, top, cap, stream=ds) if ds is not None
                           else e.chain_logprobs_batch(want, top, cap)))
        for i, slot in enumerate(out):
            self._retire(slot, None if toks is None else toks[i][:self.live[slot].req.max_new_tokens], lps.get(slot))

    def _burst_steps(self) -> int:
        """Steps of the next burst: never past the chain with the fewest tokens left.  (Letting chains overrun their budget by
        up to burst - 1 steps, as a chain that ends with an EOS does, makes the bursts of a ragged stream 8 steps long instead
        of 1-3 -- and was no faster: 80.4 / 81.7 against 81.9 / 83.3 questions/s at bursts of 8, 84.1 / 83.4 at bursts of 4;
        the waits between bursts are not what the stream spends its time on.)"""
        e = self.engine
        budget = min(min(l.req.max_new_tokens, e.max_ctx - l.req.n_prompt + 1) - l.produced for l in self.live.values())
        return max(0, min(self.burst, budget))

    def _burst_begin(self):
        e = self.engine
        slots = list(self.live.keys())
        steps = self._burst_steps()
        ran = e.decode_burst_begin(slots, steps, self.params)
        return slots, ran

    def _burst_end(self, handle) -> None:
        e = self.engine
        slots, ran = handle
        self._decode_stream = torch.cuda.current_stream(e.device) if self._side is not None else None
        t0 = time.perf_counter()
        n_gen, fin = e.decode_burst_end(slots)
        self.stats["host_s_burst_wait"] = self.stats.get("host_s_burst_wait", 0.0) + time.perf_counter() - t0
        self.stats["bursts"] += 1
        self.stats["steps"] += ran
        self.stats["chain_steps"] += ran * len(slots)
        self._tally_step_rows(ran, len(slots))
        with self._side_stream():   # (the callbacks of finished chains crop / resize on the front-end's stream)
            self._retire_finished(slots, n_gen, fin)

    def _retire(self, slot: int, tokens=None, logprobs=None) -> None:
        l = self.live.pop(slot)
        req = l.req
        ds = getattr(self, "_decode_stream", None)
        if tokens is not None:
            req.tokens = tokens
        else:
            req.tokens = (self.engine.chain_tokens(slot, req.max_new_tokens, stream=ds) if ds is not None
                          else self.engine.chain_tokens(slot, req.max_new_tokens))
        chain = req._chain
        if chain.stop_ids:   # the ids behind a stop sequence are the pads of a finished chain
            from .hostloop import first_stop_hit
            n = first_stop_hit(req.tokens, chain.stop_ids, chain.min_new_tokens)
            if n is not None:
                req.tokens = list(req.tokens[:n])
        req.text = self.processor.tokenizer.decode(req.tokens, skip_special_tokens=True).strip()
        self._drop_grammar(req)
        if chain.wants_logprobs:
            if logprobs is None:
                logprobs = (self.engine.chain_logprobs(slot, req.max_new_tokens, stream=ds) if ds is not None
                            else self.engine.chain_logprobs(slot, req.max_new_tokens))
            self._attach_logprobs(req, logprobs, chain.logprobs)
        follow = None
        try:
            follow = req.on_done(req, req.tokens, req.text) if req.on_done else None
        except Exception as ex:
            if req.on_error:
                req.on_error(req, ex)
            else:
                raise
        if follow is not None:  # continues on this slot; its cached prompt is reusable
            follow.slot = slot
            # ... and so are the rows of the generated tokens that went through the model (all but the last one sampled)
            cached = min(self.engine.seq_len(slot) - len(l.ids), len(req.tokens) - 1) if self.reuse_generated else 0
            self.parked[slot] = (l.ids, l.keys, tuple(req.tokens[:max(0, cached)]))
            self.waiting.appendleft(follow)
        else:
            if self.prefix_cache is not None:
                # the prompt's rows and, under reuse_generated, those of the generated tokens that went through the model (all but
                # the last one sampled; up to the first id that could open or close an image block): what `parked` keeps
                gen, cfg = [], self.model.config
                if self.reuse_generated:
                    special = (cfg.image_token_id, getattr(cfg, "vision_start_token_id", None), getattr(cfg, "vision_end_token_id", None))
                    for t in req.tokens[:max(0, min(self.engine.seq_len(slot) - len(l.ids), len(req.tokens) - 1))]:
                        if t in special:
                            break
                        gen.append(int(t))
                req._prefilled = None
                self._save_to_cache(slot, list(l.ids) + gen, l.keys, len(l.ids) + len(gen))
            self._retire_slot(slot)
            self.free.append(slot)

    def _retire_slot(self, slot: int) -> None:
        """The slot's rows may be overwritten from now on: the chains that read their prompt prefix from it (the decode
        attention streams ONE copy of a tile's image prefix) are moved to another holder -- on the stream the decode steps run
        on, i.e. before the next burst, whatever stream the admission work uses."""
        retire = getattr(self.engine, "seq_retire", None)
        if retire is not None:
            retire(slot, stream=getattr(self, "_decode_stream", None))

    def _release(self, req: Request) -> None:
        if req.slot >= 0:
            self._drop_grammar(req)
            self.parked.pop(req.slot, None)
            done = getattr(req, "_prefilled", None)
            if self.prefix_cache is not None and done is not None:   # a chain that ran: its prompt's rows are good
                req._prefilled = None
                self._save_to_cache(req.slot, done[0], done[1], min(len(done[0]), self.engine.seq_len(req.slot)))
            try:
                self._retire_slot(req.slot)
                self.engine.seq_reset(req.slot)   # nothing may copy a prefix from what the slot held before
            except Exception:
                pass
            self.free.append(req.slot)
            req.slot = -1

    def _fail(self, req: Request, ex: Exception) -> None:
        forks = self._take_forks(req)
        if forks:   # an anchor takes the siblings it still carries with it: one error per completion
            return self._fail_all([req] + forks, ex)
        self._release(req)
        if req.on_error:
            req.on_error(req, ex)
        else:
            raise ex

    def _fail_all(self, reqs, ex: Exception) -> None:
        """Every request of `reqs` gets the error; the ones without an `on_error` re-raise it once all slots are back."""
        unhandled = False
        reqs = [r for req in reqs for r in [req] + self._take_forks(req)]
        for req in reqs:
            self._release(req)
            if req.on_error:
                req.on_error(req, ex)
            else:
                unhandled = True
        if unhandled:
            raise ex


def run_requests(model, processor, requests, **kw) -> None:
    """Convenience: every request through one scheduler, to completion."""
    s = ChainScheduler(model, processor, **kw)
    try:
        for r in requests:
            s.submit(r)
        s.run()
    finally:
        s.close()

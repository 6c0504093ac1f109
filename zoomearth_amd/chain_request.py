"""The resolved request of one chain: what the engine's per-slot tables get before the chain's first draw.

Every front-end (ChainScheduler, generate(), the server through the scheduler) validates and merges its own way -- HF's wording,
OpenAI's wording, the scheduler's defaults -- and ends in one ChainRequest.  The values here are final: no None-means-default, no
validation.  The "is this kind off" rules live in `install` and nowhere else; a chain with everything off makes no engine call.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional, Sequence, Tuple


@dataclass(frozen=True)
class ChainRequest:
    # (do_sample, temperature, seed, repetition_penalty) when the chain carries values of its own; None: it follows the gen_params
    # of the call that decodes it
    sampling: Optional[Tuple[bool, float, int, float]] = None
    # the chain's effective mode and repetition penalty, its own or its caller's: the filter is written for a sampled chain only, a
    # penalty other than 1.0 has the prompt's ids marked as seen
    sampled: bool = False
    effective_penalty: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    min_p: float = 0.0
    # HF's typical_p / epsilon_cutoff / eta_cutoff (1.0 / 0.0 / 0.0 = off), behind the three above and written with them
    typical_p: float = 1.0
    epsilon_cutoff: float = 0.0
    eta_cutoff: float = 0.0
    logprobs: Optional[int] = None
    # vLLM's prompt_logprobs: the chain's prefill pass scores its prompt positions (None: a plain prefill); nothing to install
    prompt_logprobs: Optional[int] = None
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    min_new_tokens: int = 0
    logit_bias: dict = field(default_factory=dict)
    no_repeat_ngram_size: int = 0
    stop_ids: Sequence = ()
    bad_words_ids: Sequence = ()
    # speculative decoding by prompt lookup (HF's prompt_lookup_num_tokens / max_matching_ngram_size, vLLM's ngram method): up to
    # that many draft ids per step, looked up in prompt + generated ids by their last ngram_max .. ngram_min ids; 0 = off.  Greedy
    # only: the front-ends refuse it together with a sampled mode, a filter, log-probabilities, logit adjustments, token rules or a
    # grammar, as the engine does
    speculative_tokens: int = 0
    ngram_min: int = 1
    ngram_max: int = 3
    # the sampled mode of speculation (Engine.set_speculation(sampled=True)): the chain may sample and carry a top-k / top-p / min-p
    # filter; every row draws what a plain step would, so it stays lossless.  Opt-in: without it the rule above holds
    speculative_sampling: bool = False

    @property
    def wants_logprobs(self) -> bool:
        return self.logprobs is not None

    @property
    def wants_prompt_logprobs(self) -> bool:
        return self.prompt_logprobs is not None

    def speculation_conflict(self, grammar: bool = False) -> Optional[str]:
        """What of this request speculation excludes (the engine's rule, ze_seq_set_speculation), or None."""
        if self.sampled and not self.speculative_sampling:
            return "sampling"
        if self.sampled and (self.typical_p < 1.0 or self.epsilon_cutoff > 0.0 or self.eta_cutoff > 0.0):
            return "entropy filters"
        if self.logprobs is not None:
            return "logprobs"
        if self.presence_penalty != 0.0 or self.frequency_penalty != 0.0 or self.logit_bias or self.min_new_tokens > 0:
            return "logit adjustments"
        if self.stop_ids or self.bad_words_ids or self.no_repeat_ngram_size > 0:
            return "token rules"
        return "guided decoding" if grammar else None

    def install(self, engine, slot: int, prompt_ids, grammar: Optional[int] = None) -> None:
        """The request into `slot`, whose reset / truncate / prefix copy cleared the previous chain's, before the first draw.  The
        prompt ids are the context of the bans (bad words, n-grams); `grammar` is the device id the caller acquired, if any."""
        if self.sampling is not None:
            do_sample, temperature, seed, penalty = self.sampling
            engine.set_sampling(slot, do_sample=do_sample, temperature=temperature, seed=seed, repetition_penalty=penalty)
        if self.sampled and (self.top_k > 0 or self.top_p < 1.0 or self.min_p > 0.0):
            engine.set_sampling_filter(slot, self.top_k, self.top_p, self.min_p)
        if self.sampled and (self.typical_p < 1.0 or self.epsilon_cutoff > 0.0 or self.eta_cutoff > 0.0):
            engine.set_entropy_filter(slot, self.typical_p, self.epsilon_cutoff, self.eta_cutoff)
        if self.logprobs is not None:
            engine.set_logprobs(slot, self.logprobs)
        if self.presence_penalty != 0.0 or self.frequency_penalty != 0.0 or self.logit_bias or self.min_new_tokens > 0:
            engine.seq_set_logit_adjust(slot, self.presence_penalty, self.frequency_penalty, self.min_new_tokens, self.logit_bias)
        bans = bool(self.bad_words_ids) or self.no_repeat_ngram_size > 0
        if self.stop_ids or bans:
            engine.set_token_rules(slot, self.no_repeat_ngram_size, list(self.stop_ids), list(self.bad_words_ids),
                                   context=list(prompt_ids) if bans else None)
        if grammar is not None:
            engine.set_grammar(slot, grammar)
        if self.speculative_tokens > 0:   # (last: the engine checks the slot's other requests)
            if self.speculative_sampling:
                engine.set_speculation(slot, self.speculative_tokens, list(prompt_ids), self.ngram_min, self.ngram_max, sampled=True)
            else:
                engine.set_speculation(slot, self.speculative_tokens, list(prompt_ids), self.ngram_min, self.ngram_max)

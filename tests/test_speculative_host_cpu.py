"""CPU: speculative decoding through the host layers -- ChainRequest.install, generate()'s HF keyword arguments, the scheduler's
row budget and the server's flag -- on recording stub engines whose speculative steps are the numpy restatement
(tests/spec_ref.py)."""
import numpy as np
import pytest
import torch

import spec_ref as S
from test_chain_request_cpu import Calls, GenStubEngine
from test_sampling_filters_cpu import wrapper
from test_scheduler_cpu import EOS, PAD, Proc, StubEngine, make_model
from zoomearth_amd.chain_request import ChainRequest
from zoomearth_amd.scheduler import ChainScheduler, Request

PROMPT = [11, 12, 13]


# ---------------------------------------------------------------- ChainRequest
def test_install_sets_speculation_last_and_untouched_defaults_call_nothing():
    engine = Calls()
    ChainRequest().install(engine, 2, tuple(PROMPT))
    assert engine.log == []
    ChainRequest(sampling=(False, 1.0, 0, 1.3), effective_penalty=1.3, speculative_tokens=4, ngram_min=2, ngram_max=5).install(engine, 2, tuple(PROMPT))
    assert engine.log == [("set_sampling", (2,), dict(do_sample=False, temperature=1.0, seed=0, repetition_penalty=1.3)),
                          ("set_speculation", (2, 4, PROMPT, 2, 5), {})]


@pytest.mark.parametrize("kw,what", [(dict(sampled=True), "sampling"), (dict(logprobs=0), "logprobs"), (dict(presence_penalty=0.5), "logit adjustments"),
                                     (dict(min_new_tokens=2), "logit adjustments"), (dict(logit_bias={3: 1.0}), "logit adjustments"),
                                     (dict(stop_ids=[[5]]), "token rules"), (dict(no_repeat_ngram_size=2), "token rules"),
                                     (dict(bad_words_ids=[[4]]), "token rules")])
def test_the_mutual_exclusions(kw, what):
    assert ChainRequest(speculative_tokens=4, **kw).speculation_conflict() == what
    assert ChainRequest(speculative_tokens=4, effective_penalty=1.3).speculation_conflict() is None
    assert ChainRequest(speculative_tokens=4).speculation_conflict(grammar=True) == "guided decoding"


# ---------------------------------------------------------------- generate()
class SpecGenStub(GenStubEngine):
    max_ctx = 256

    def set_speculation(self, slot, k, prompt_ids=(), ngram_min=1, ngram_max=3):
        self.log.append(("speculation", slot, k, list(prompt_ids), ngram_min, ngram_max))

    def generate_speculative(self, slots, max_new_tokens, **kw):
        self.log.append(("generate_speculative", list(slots), max_new_tokens, kw))
        return [[100] * max_new_tokens for _ in slots]

    def generate(self, slot, max_new_tokens, **kw):
        self.log.append(("generate", slot))
        return super().generate(slot, max_new_tokens, **kw)


def gen(rows, **kw):
    m = wrapper()
    m.engine = SpecGenStub(max_seqs=2)
    out = m.generate(input_ids=torch.tensor(rows), max_new_tokens=3, **kw)
    return m.engine.log, out


def names(log):
    return [c[0] for c in log if c[0] in ("speculation", "generate_speculative", "generate")]


def test_generate_takes_hfs_names_and_routes_through_the_bursts():
    log, out = gen([[11, 50, 51]], prompt_lookup_num_tokens=4, max_matching_ngram_size=2, repetition_penalty=1.2)
    assert [c for c in log if c[0] == "speculation"] == [("speculation", 0, 4, [11, 50, 51], 1, 2)]
    assert names(log) == ["speculation", "generate_speculative"]
    (call,) = [c for c in log if c[0] == "generate_speculative"]
    assert call[1:3] == ([0], 3) and call[3]["repetition_penalty"] == 1.2
    assert out.shape == (1, 6)
    log, _ = gen([[11, 50, 51], [12, 50, 52]], prompt_lookup_num_tokens=4)
    assert names(log) == ["speculation", "speculation", "generate_speculative"]
    log, _ = gen([[11, 50, 51]])                                  # untouched defaults: no call, today's path
    assert names(log) == ["generate"]


@pytest.mark.parametrize("kw", [dict(prompt_lookup_num_tokens=4, do_sample=True), dict(prompt_lookup_num_tokens=4, logprobs=0),
                                dict(prompt_lookup_num_tokens=4, no_repeat_ngram_size=2), dict(prompt_lookup_num_tokens=4, presence_penalty=0.5),
                                dict(prompt_lookup_num_tokens=4, stop_token_ids=[5]), dict(prompt_lookup_num_tokens=0),
                                dict(prompt_lookup_num_tokens=9), dict(prompt_lookup_num_tokens=True), dict(max_matching_ngram_size=2),
                                dict(prompt_lookup_num_tokens=4, max_matching_ngram_size=9),
                                dict(prompt_lookup_num_tokens=4, do_sample=True, num_return_sequences=2)])
def test_generate_refuses(kw):
    with pytest.raises(ValueError):
        gen([[11, 50, 51]], **kw)


def test_num_beams_stays_refused():
    with pytest.raises(NotImplementedError):
        gen([[11, 50, 51]], prompt_lookup_num_tokens=4, num_beams=2)


# ---------------------------------------------------------------- the scheduler against a stub whose steps are the restatement
class SpecStub(StubEngine):
    """StubEngine whose speculating chains take the restatement's steps: draft from prompt + generated ids, then accept against
    the ids the stub would have produced one by one."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.spec, self.stats, self.rows_seen = {}, {}, []

    def seq_reset(self, slot):
        super().seq_reset(slot)
        self.spec.pop(slot, None)

    def set_speculation(self, slot, k, prompt_ids=(), ngram_min=1, ngram_max=3):
        self.log.append(("speculation", slot, k))
        if k:
            self.spec[slot], self.stats[slot] = (k, list(prompt_ids), ngram_min, ngram_max), [0, 0, 0]
        else:
            self.spec.pop(slot, None)

    def spec_stats(self, slot):
        return tuple(self.stats.get(slot, (0, 0, 0)))

    def decode_burst(self, slots, steps, params):
        if not any(s in self.spec for s in slots):
            return super().decode_burst(slots, steps, params)
        rows = sum(1 + (self.spec[s][0] if s in self.spec else 0) for s in slots)
        self.rows_seen.append(rows)
        assert rows <= 64, "more than 64 rows in a step"
        self.log.append(("burst", len(slots), steps))
        for _ in range(steps):
            for s in slots:
                c = self.chains[s]
                if s not in self.spec or c["fin"]:
                    self._next(c)
                    continue
                k, prompt, gmin, gmax = self.spec[s]
                d = S.draft(prompt + c["out"], k, gmin, gmax, cap=self.max_ctx - len(c["ids"]) - len(c["out"]))
                a = 0
                while True:   # the stub's next id is the model's answer for the row
                    self._next(c)
                    if a == len(d) or c["out"][-1] != d[a] or c["fin"]:
                        break
                    a += 1
                st = self.stats[s]
                st[0], st[1], st[2] = st[0] + 1, st[1] + len(d), st[2] + a
        return steps, [len(self.chains[s]["out"]) for s in slots], [self.chains[s]["fin"] for s in slots]


def run_sched(n, k, max_seqs=16, **req_kw):
    model = make_model(max_seqs=max_seqs)
    model.engine = SpecStub(max_seqs=max_seqs)
    sched = ChainScheduler(model, Proc(), burst=4, share_prefix=False, speculative_tokens=k)
    done = {}
    for i in range(n):
        sched.submit(Request(prompt=f"{2 * i + 11} 60 61", images=[], max_new_tokens=12, tag=i,
                             on_done=lambda r, toks, text: done.__setitem__(r.tag, list(toks)), **req_kw))
    sched.run()
    return model.engine, done


def test_the_scheduler_budgets_a_steps_rows_and_lowers_k():
    plain, want = run_sched(10, 0, max_seqs=10)
    assert not [c for c in plain.log if c[0] == "speculation"]            # off: no call
    eng, got = run_sched(10, 8, max_seqs=10)
    # a joining chain gets what the live chains' rows leave, one row kept for every slot still free: 64 - 9 i - 1 - (9 - i) for chain i
    assert [c[2] for c in eng.log if c[0] == "speculation"] == [8, 8, 8, 8, 8, 8, 6]     # (k = 0: no call, the chain rides with one row)
    assert eng.rows_seen and max(eng.rows_seen) == 6 * 9 + 7 + 3 == 64
    assert got == want and len(got) == 10                                  # lossless, and trimmed to each request's budget
    assert all(len(t) == 12 for t in got.values())
    full, got16 = run_sched(16, 3)                                         # 16 x (1 + 3) rows fit: nobody is lowered
    assert [c[2] for c in full.log if c[0] == "speculation"] == [3] * 16 and max(full.rows_seen) == 64
    few, got4 = run_sched(4, 8)
    assert [c[2] for c in few.log if c[0] == "speculation"] == [8, 8, 8, 8]
    assert got4 == {i: got16[i] for i in range(4)} == {i: want[i] for i in range(4)}
    assert sum(few.spec_stats(s)[2] for s in range(4)) > 0                 # (the stub's ids cycle with period 7: drafts hit)


def test_requests_that_cannot_speculate_ride_along_and_naming_both_is_refused():
    model = make_model()
    model.engine = SpecStub(max_seqs=4)
    sched = ChainScheduler(model, Proc(), burst=4, share_prefix=False, speculative_tokens=4)
    assert sched._resolve(Request(prompt="1 2", images=[], stop_ids=[[5]])).speculative_tokens == 0
    assert sched._resolve(Request(prompt="1 2", images=[], do_sample=True, temperature=0.5)).speculative_tokens == 0
    assert sched._resolve(Request(prompt="1 2", images=[])).speculative_tokens == 4
    assert sched._resolve(Request(prompt="1 2", images=[], speculative_tokens=0)).speculative_tokens == 0
    assert sched._resolve(Request(prompt="1 2", images=[], speculative_tokens=2, repetition_penalty=1.3)).speculative_tokens == 2
    for kw in (dict(stop_ids=[[5]]), dict(do_sample=True), dict(guided_choice=["a"]), dict()):
        with pytest.raises(ValueError):
            sched._resolve(Request(prompt="1 2", images=[], speculative_tokens=9 if not kw else 4, **kw))
    with pytest.raises(ValueError):
        ChainScheduler(model, Proc(), speculative_tokens=9)


def test_the_server_reports_the_flag():
    from zoomearth_amd import serve
    srv = serve.ChatServer(make_model(), Proc(), "stub", speculative_ngram=4)
    assert srv.speculative_ngram == 4 and serve.ChatServer(make_model(), Proc(), "stub").speculative_ngram == 0

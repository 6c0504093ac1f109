"""CPU: the resolved request of one chain (zoomearth_amd/chain_request.py) -- `install` issues exactly the engine calls of what is
not off, in one order and one argument form, and the three front-ends (ChainScheduler._resolve, generate(), the server's
dispatcher) end in the same calls, on recording stub engines."""
import dataclasses

import numpy as np
import pytest
import torch

from test_chain_sampling_cpu import GatedStub
from test_logit_adjust_cpu import la_model
from test_sampling_filters_cpu import Proc, wrapper
from test_scheduler_cpu import Proc as WordProc
from test_scheduler_cpu import make_model
from test_token_rules_cpu import RulesStubEngine
from zoomearth_amd.chain_request import ChainRequest
from zoomearth_amd.scheduler import ChainScheduler, Request

NINF = float("-inf")


# ---------------------------------------------------------------- install: the exact calls, in order
class Calls:
    """Records every method call as (name, positional arguments, keyword arguments)."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        return lambda *a, **kw: self.log.append((name, a, kw))


PROMPT = [11, 12, 13]
SAMPLING = ("set_sampling", (2,), dict(do_sample=True, temperature=0.7, seed=9, repetition_penalty=1.2))
EVERYTHING = ChainRequest(sampling=(True, 0.7, 9, 1.2), sampled=True, effective_penalty=1.2, top_k=40, top_p=0.9, min_p=0.05, logprobs=3,
                          presence_penalty=0.5, frequency_penalty=-0.25, min_new_tokens=2, logit_bias={9: NINF}, no_repeat_ngram_size=3,
                          stop_ids=[[5, 6], [9]], bad_words_ids=[[4, 8]])
INSTALL_TABLE = [
    ("all off", ChainRequest(), None, []),
    ("all off, the caller's mode and penalty", ChainRequest(sampled=True, effective_penalty=1.3), None, []),
    ("sampling alone", ChainRequest(sampling=(True, 0.7, 9, 1.2), sampled=True, effective_penalty=1.2), None, [SAMPLING]),
    ("a greedy chain's own penalty", ChainRequest(sampling=(False, 1.0, 0, 1.5), effective_penalty=1.5), None,
     [("set_sampling", (2,), dict(do_sample=False, temperature=1.0, seed=0, repetition_penalty=1.5))]),
    ("filter alone", ChainRequest(sampled=True, top_k=40), None, [("set_sampling_filter", (2, 40, 1.0, 0.0), {})]),
    ("filter by top_p / min_p", ChainRequest(sampled=True, top_p=0.9, min_p=0.05), None, [("set_sampling_filter", (2, 0, 0.9, 0.05), {})]),
    ("greedy with a filter", ChainRequest(sampled=False, top_k=40, top_p=0.9, min_p=0.05), None, []),
    ("logprobs alone, the chosen token only", ChainRequest(logprobs=0), None, [("set_logprobs", (2, 0), {})]),
    ("presence penalty alone", ChainRequest(presence_penalty=-0.5), None, [("seq_set_logit_adjust", (2, -0.5, 0.0, 0, {}), {})]),
    ("min_new_tokens alone", ChainRequest(min_new_tokens=4), None, [("seq_set_logit_adjust", (2, 0.0, 0.0, 4, {}), {})]),
    ("bias alone", ChainRequest(logit_bias={7: 1.5}), None, [("seq_set_logit_adjust", (2, 0.0, 0.0, 0, {7: 1.5}), {})]),
    ("stop ids only", ChainRequest(stop_ids=[[5, 6], [9]]), None, [("set_token_rules", (2, 0, [[5, 6], [9]], []), dict(context=None))]),
    ("bad words", ChainRequest(bad_words_ids=[[4, 8]]), None, [("set_token_rules", (2, 0, [], [[4, 8]]), dict(context=PROMPT))]),
    ("an n-gram size", ChainRequest(no_repeat_ngram_size=2), None, [("set_token_rules", (2, 2, [], []), dict(context=PROMPT))]),
    ("grammar alone", ChainRequest(), 5, [("set_grammar", (2, 5), {})]),
    ("everything on", EVERYTHING, 0,                      # (grammar id 0 is a grammar)
     [SAMPLING, ("set_sampling_filter", (2, 40, 0.9, 0.05), {}), ("set_logprobs", (2, 3), {}),
      ("seq_set_logit_adjust", (2, 0.5, -0.25, 2, {9: NINF}), {}),
      ("set_token_rules", (2, 3, [[5, 6], [9]], [[4, 8]]), dict(context=PROMPT)), ("set_grammar", (2, 0), {})]),
]


@pytest.mark.parametrize("what,chain,grammar,want", INSTALL_TABLE, ids=[row[0] for row in INSTALL_TABLE])
def test_install_issues_exactly_the_calls_of_what_is_not_off(what, chain, grammar, want):
    engine = Calls()
    chain.install(engine, 2, tuple(PROMPT), grammar)
    assert engine.log == want
    assert chain.wants_logprobs == (chain.logprobs is not None)


def test_a_chain_request_holds_final_values():
    assert ChainRequest() == ChainRequest(sampling=None, sampled=False, effective_penalty=1.0, top_k=0, top_p=1.0, min_p=0.0, logprobs=None,
                                          presence_penalty=0.0, frequency_penalty=0.0, min_new_tokens=0, logit_bias={},
                                          no_repeat_ngram_size=0, stop_ids=(), bad_words_ids=())
    with pytest.raises(dataclasses.FrozenInstanceError):
        ChainRequest().top_k = 3


# ---------------------------------------------------------------- the scheduler: a mixed queue against the parent commit's log
class FullStubEngine(RulesStubEngine):
    """Every per-chain setter, recorded in the log of test_sampling_filters_cpu's stub (reset / truncate / copy / begin)."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.grammars = []

    def mark_seen(self, slot, ids):
        self.log.append(("seen", slot, list(ids)))

    def set_sampling(self, slot, do_sample=None, temperature=1.0, seed=0, repetition_penalty=1.0):
        self.log.append(("sampling", slot, do_sample, temperature, seed, repetition_penalty))

    def set_logprobs(self, slot, top_n=0):
        self.log.append(("logprobs", slot, top_n))

    def chain_logprobs(self, slot, cap=0):
        m = len(self.chains[slot]["out"][: cap or None])
        return np.full(m, -0.5, np.float32), np.zeros((m, 20), np.int32), np.zeros((m, 20), np.float32)

    def grammar_create(self, automaton):
        self.grammars.append(automaton)
        return len(self.grammars) - 1

    def grammar_destroy(self, gid):
        pass

    def chain_grammar_state(self, slot):
        return -1, 0

    def set_grammar(self, slot, gid, state=0):
        if gid is not None:
            self.log.append(("grammar", slot, gid))


def installs(log):
    """In chain_begin order: (first prompt id, what emptied the slot, the calls on the slot since, without the slot number)."""
    out = []
    for i, ev in enumerate(log):
        if ev[0] == "begin":
            j = max(k for k in range(i) if log[k][0] in ("reset", "truncate", "copy") and log[k][1] == ev[1])
            out.append((ev[2], log[j][0], [(x[0],) + tuple(x[2:]) for x in log[j + 1:i] if x[1] == ev[1]]))
    return out


def scheduler_log():
    """Six requests -- fields named by the request, by the scheduler, by neither -- and one follow-up on a parked slot, through a
    sampling scheduler with defaults of its own."""
    model = la_model(max_seqs=3)
    model.engine = FullStubEngine(max_seqs=3)
    model.compile_grammar = lambda tokenizer=None, **kw: kw
    sched = ChainScheduler(model, Proc(), do_sample=True, temperature=0.9, seed=7, repetition_penalty=1.1, top_k=20, logprobs=2,
                           frequency_penalty=0.25, min_new_tokens=1, burst=2, share_prefix=False)

    def follow(req, tokens, text):
        return Request(prompt=req.prompt + " 100 100 60", images=[], max_new_tokens=2, guided_regex="x+", logprobs=5, do_sample=False)

    for r in (Request(prompt="11 50 51", images=[], max_new_tokens=3),
              Request(prompt="12 50 51", images=[], max_new_tokens=3, do_sample=False, top_k=40, logprobs=0, frequency_penalty=0.0,
                      min_new_tokens=0),
              Request(prompt="13 50 51", images=[], max_new_tokens=3, temperature=0.5, seed=3, top_p=0.8, min_p=0.1, presence_penalty=-0.5,
                      logit_bias={9: -100.0}, stop_ids=[[5, 6], [9]]),
              Request(prompt="14 50 51", images=[], max_new_tokens=3, repetition_penalty=1.0, bad_words_ids=[[4, 8]], no_repeat_ngram_size=3,
                      guided_choice=["a", "b"]),
              Request(prompt="15 50 51", images=[], max_new_tokens=3, top_k=0, top_p=1.0, min_p=0.0, stop_ids=[[100, 100]], on_done=follow),
              Request(prompt="16 50 51", images=[], max_new_tokens=3, guided_regex="x+", min_new_tokens=4, stop_ids=[[9]],
                      no_repeat_ngram_size=2, logit_bias={})):
        sched.submit(r)
    sched.run()
    return installs(model.engine.log)


# The log of scheduler_log() on the commit before ChainRequest existed (six `_set_*` methods in ChainScheduler), pasted as data:
#   python -c "import sys, types, pprint; sys.path[:0] = ['.', 'tests']; \
#     sys.modules['zoomearth_amd.chain_request'] = types.SimpleNamespace(ChainRequest=lambda **kw: None); \
#     import test_chain_request_cpu as T; pprint.pprint(T.scheduler_log(), width=150)"
PARENT_LOG = [
    (11, "reset", [("seen", [11, 50, 51]), ("filter", 20, 1.0, 0.0), ("logprobs", 2), ("adjust", 0.0, 0.25, 1, {})]),
    (12, "reset", [("seen", [12, 50, 51]), ("sampling", False, 0.9, 7, 1.1), ("logprobs", 0)]),
    (13, "reset", [("seen", [13, 50, 51]), ("sampling", True, 0.5, 3, 1.1), ("filter", 20, 0.8, 0.1), ("logprobs", 2),
                   ("adjust", -0.5, 0.25, 1, {9: -100.0}), ("rules", 0, [[5, 6], [9]], [], None)]),
    (14, "reset", [("sampling", True, 0.9, 7, 1.0), ("filter", 20, 1.0, 0.0), ("logprobs", 2), ("adjust", 0.0, 0.25, 1, {}),
                   ("rules", 3, [], [[4, 8]], [14, 50, 51]), ("grammar", 0)]),
    (15, "reset", [("seen", [15, 50, 51]), ("logprobs", 2), ("adjust", 0.0, 0.25, 1, {}), ("rules", 0, [[100, 100]], [], None)]),
    (16, "reset", [("seen", [16, 50, 51]), ("filter", 20, 1.0, 0.0), ("logprobs", 2), ("adjust", 0.0, 0.25, 4, {}),
                   ("rules", 2, [[9]], [], [16, 50, 51]), ("grammar", 1)]),
    (15, "truncate", [("seen", [15, 50, 51, 100, 100, 60]), ("sampling", False, 0.9, 7, 1.1), ("logprobs", 5),
                      ("adjust", 0.0, 0.25, 1, {}), ("grammar", 1)]),
]


def test_scheduler_installs_what_the_parent_commit_installed():
    assert scheduler_log() == PARENT_LOG


# ---------------------------------------------------------------- generate(): one install per row, the scheduler's calls
class GenStubEngine(FullStubEngine):
    """... and what generate() drives: the single-chain and the batched prefill / decode calls."""

    def prefill(self, slot, ids, emb, pos, delta, want_logits=False):
        self.prefill_batch([slot], [ids], [emb], [pos], [delta])

    def set_decode_regime(self, regime):
        pass

    def generate(self, slot, max_new_tokens, **kw):
        self.chain_begin(slot, kw, 0)
        return [100] * max_new_tokens

    def generate_batch(self, slots, max_new_tokens, **kw):
        return [self.generate(s, max_new_tokens, **kw) for s in slots]

    def chain_logprobs_batch(self, slots, top_n, cap=0):
        return [self.chain_logprobs(s, cap) for s in slots]


SETTINGS = dict(logprobs=2, presence_penalty=0.5, min_new_tokens=2, logit_bias={9: -1.0}, no_repeat_ngram_size=3, bad_words_ids=[[4, 8]])


def generate_log(rows, **kw):
    m = wrapper()
    m.engine = GenStubEngine(max_seqs=2)
    m.compile_grammar = lambda *a, **k: "automaton"
    m.generate(input_ids=torch.tensor(rows), max_new_tokens=2, do_sample=True, temperature=0.7, top_k=40, seed=9, repetition_penalty=1.2,
               stop_token_ids=[5], guided_choice=["a", "b"], tokenizer=object(), **SETTINGS, **kw)
    return installs(m.engine.log)


def test_generate_installs_the_same_calls_for_one_row_and_for_a_batch_and_the_schedulers():
    one = generate_log([[11, 50, 51]])
    assert one == [(11, "reset", [("seen", [11, 50, 51]), ("logprobs", 2), ("adjust", 0.5, 0.0, 2, {9: -1.0}),
                                  ("rules", 3, [[5]], [[4, 8]], [11, 50, 51]), ("grammar", 0)])]
    two = generate_log([[11, 50, 51], [12, 50, 52]])
    assert [x[0] for x in two] == [11, 12]
    for first, emptied, calls in two:   # every row of a batch: the single row's calls, with its own prompt as the bans' context
        assert emptied == "reset" and len(calls) == len(one[0][2])
        assert [c for c in calls if c[0] not in ("seen", "rules")] == [c for c in one[0][2] if c[0] not in ("seen", "rules")]
        ids = [first, 50, 51 if first == 11 else 52]
        assert [c for c in calls if c[0] in ("seen", "rules")] == [("seen", ids), ("rules", 3, [[5]], [[4, 8]], ids)]
    # the scheduler, given the same settings under its own names: the same calls, and in front of them the sampling request and
    # the filter that generate() hands to Engine.generate instead
    model = la_model(max_seqs=2)
    model.engine = FullStubEngine(max_seqs=2)
    model.compile_grammar = lambda tokenizer=None, **kw: "automaton"
    sched = ChainScheduler(model, Proc(), burst=2, share_prefix=False)
    sched.submit(Request(prompt="11 50 51", images=[], max_new_tokens=2, do_sample=True, temperature=0.7, top_k=40, seed=9,
                         repetition_penalty=1.2, stop_ids=[[5]], guided_choice=["a", "b"], **SETTINGS))
    sched.run()
    (first, emptied, calls), = installs(model.engine.log)
    assert (first, emptied) == (11, "reset")
    assert [c for c in calls if c[0] in ("sampling", "filter")] == [("sampling", True, 0.7, 9, 1.2), ("filter", 40, 1.0, 0.0)]
    assert [c for c in calls if c[0] not in ("sampling", "filter")] == one[0][2]


# ---------------------------------------------------------------- the server: one scheduler, the parsed fields and no others
class ServeStub(GatedStub):
    """test_chain_sampling_cpu's gated engine, with the other per-chain setters accepted."""

    def set_sampling_filter(self, slot, top_k=0, top_p=1.0, min_p=0.0):
        pass

    def set_logprobs(self, slot, top_n=0):
        pass

    def seq_set_logit_adjust(self, slot, *a):
        pass

    def set_token_rules(self, slot, *a, context=None):
        pass

    def chain_logprobs(self, slot, cap=0):
        m = len(self.chain_tokens(slot, cap))
        return np.full(m, -0.5, np.float32), np.zeros((m, 20), np.int32), np.zeros((m, 20), np.float32)


def test_server_submits_every_kind_to_one_scheduler_with_exactly_the_parsed_fields(monkeypatch):
    from zoomearth_amd import scheduler, serve

    built, submitted = [], []

    class Counted(ChainScheduler):
        def __init__(self, *a, **kw):
            built.append(self)
            super().__init__(*a, **kw)

        def submit(self, req):
            submitted.append(req)
            super().submit(req)

    monkeypatch.setattr(scheduler, "ChainScheduler", Counted)
    model = make_model(max_seqs=4)
    model.engine = ServeStub(max_seqs=4)
    model.config.text = type("T", (), {"vocab_size": 2048})
    model.generate = lambda **kw: pytest.fail("the dispatcher never falls back to generate()")

    class SProc(WordProc):
        def __call__(self, text, images=None, return_tensors="pt", padding=None, **kw):
            body = text[0].split("user\n")[1].split("<|im_end|>")[0]
            return dict(input_ids=torch.tensor([[ord(c) % 50 + 10 for c in body[:4]]]))

    def req(text, **kw):
        return dict(messages=[{"role": "user", "content": text}], **kw)

    bodies = [req("aaaa", max_tokens=12),
              req("cccc", max_tokens=12, repetition_penalty=1.5, logprobs=True, top_logprobs=3, stop_token_ids=[9]),
              req("eeee", max_tokens=6, temperature=0.7, seed=9, top_k=40, top_p=0.9, min_p=0.05, presence_penalty=0.5,
                  frequency_penalty=-1.0, logit_bias={"17": -100}, min_tokens=2, no_repeat_ngram_size=3),
              req("gggg", max_tokens=500, temperature=1.5, repetition_penalty=1.0)]
    srv = serve.ChatServer(model, SProc(), "stub", batch_window_s=0.0)
    first = srv.submit(bodies[0])
    assert model.engine.decoding.wait(timeout=30)                    # the greedy chain is inside its first burst
    rest = [srv.submit(b) for b in bodies[1:]]
    model.engine.go.set()
    for f in [first] + rest:
        assert f.result(timeout=30)["object"] == "chat.completion"
    srv.close()
    assert len(built) == 1 and built[0] is srv.scheduler and srv.scheduler.stats["admitted"] == 4
    named = [dict(),
             dict(repetition_penalty=1.5, logprobs=3, stop_ids=[[9]]),
             dict(do_sample=True, temperature=0.7, seed=9, top_k=40, top_p=0.9, min_p=0.05, presence_penalty=0.5, frequency_penalty=-1.0,
                  logit_bias={17: -100.0}, min_new_tokens=2, no_repeat_ngram_size=3),
             dict(do_sample=True, temperature=1.5, seed=0, top_k=0, top_p=1.0, min_p=0.0, repetition_penalty=1.0)]
    budgets = [12, 12, 6, 256]                                       # (the last one clamped to the engine's max_ctx)
    assert len(submitted) == 4
    for r, body, own, budget in zip(submitted, bodies, named, budgets):
        p = srv._parse(body)
        want = dict(prompt=p.prompt, images=[], max_new_tokens=budget, stream_id=0, tag=None,
                    # what a request does not name: the parsed off values for the kinds the server always forwards, None elsewhere
                    top_k=None, top_p=None, min_p=None, do_sample=None, temperature=None, seed=None, repetition_penalty=None,
                    logprobs=None, presence_penalty=0.0, frequency_penalty=0.0, logit_bias={}, min_new_tokens=0, stop_ids=[],
                    bad_words_ids=None, no_repeat_ngram_size=0, guided_regex=None, guided_choice=None)
        want.update(own)
        got = {f.name: getattr(r, f.name) for f in dataclasses.fields(Request)}
        for k in ("on_done", "on_error"):
            assert callable(got.pop(k))
        for k in ("slot", "n_prompt", "tokens", "text", "token_logprobs", "top_logprobs"):   # (filled by the scheduler)
            got.pop(k)
        assert got == want

"""CPU: the token-rule restatement against the installed transformers' processors (or hand-worked cases), the text-level stop
cut, the host layers (scheduler, server, model wrapper) on stubs, and the presence of the C entry points."""
import os
import re

import numpy as np
import pytest
import torch

import token_rules_ref as R
from test_logit_adjust_cpu import AdjustStubEngine, la_model
from test_sampling_filters_cpu import Proc, wrapper
from zoomearth_amd import hostloop
from zoomearth_amd.scheduler import ChainScheduler, Request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_on_hand_worked_cases():
    assert R.banned_ids([1, 2, 3, 1, 2], 0, 3, []) == {3}                 # "1 2" was followed by 3
    assert R.banned_ids([1, 2, 3, 1, 2], 5, 3, []) == {3}                 # (where the context ends does not matter to a ban)
    assert R.banned_ids([4, 4, 4, 4], 0, 3, []) == {4}
    assert R.banned_ids([1, 2, 3], 0, 1, []) == {1, 2, 3}
    assert R.banned_ids([1], 0, 3, []) == set() and R.banned_ids([], 0, 1, []) == set()
    assert R.banned_ids([1, 2], 0, 0, [[1, 2, 9], [2, 8], [7], [3, 1, 2, 6]]) == {9, 8, 7}
    assert R.banned_ids([], 0, 0, [[1, 2], [5]]) == {5}
    row = R.ban_row(np.asarray([0.5, -0.0, 2.0], np.float32), [2, 0], 0, 1, [[9]])
    assert row.tolist() == [-np.inf, 0.0, -np.inf] and np.signbit(row[1])
    assert R.stop_hit([3, 4], [[3, 4]]) and not R.stop_hit([3], [[2, 3]]) and not R.stop_hit([], [[1]])
    assert not R.stop_hit([3, 4], [[3, 4]], min_new=3) and R.stop_hit([3, 4], [[3, 4]], min_new=2)
    assert R.first_hit([5, 3, 4, 3, 4], [[3, 4]]) == 3 and R.first_hit([5, 3, 4, 3, 4], [[3, 4]], 4) == 5
    assert R.first_hit([5, 6], [[7]]) is None
    # the library's own host helper is the same function
    for g, recs, mn in (([5, 3, 4, 3, 4], [[3, 4]], 0), ([5, 3, 4, 3, 4], [[3, 4]], 4), ([5, 6], [[7]], 0), ([1, 2], [[2], [1]], 0)):
        assert hostloop.first_stop_hit(g, recs, mn) == R.first_hit(g, recs, mn)


def test_restatement_equals_the_transformers_processors():
    lp = pytest.importorskip("transformers.generation.logits_process")
    rng = np.random.default_rng(3)
    vocab = 12
    for trial in range(120):
        L = int(rng.integers(0, 30))
        h = rng.integers(0, 4 if trial % 2 else vocab, size=L).tolist()
        n = int(rng.integers(1, 6))
        scores = torch.zeros((1, vocab))
        ids = torch.tensor([h], dtype=torch.long)
        got = lp.NoRepeatNGramLogitsProcessor(n)(ids, scores.clone())[0]
        assert set(torch.nonzero(torch.isinf(got)).flatten().tolist()) == R.banned_ids(h, 0, n, []), (h, n)
        recs = [rng.integers(0, 4 if trial % 2 else vocab, size=int(rng.integers(1, 5))).tolist() for _ in range(int(rng.integers(1, 6)))]
        recs = [r for i, r in enumerate(recs) if r not in recs[:i]]
        got = lp.NoBadWordsLogitsProcessor(recs, eos_token_id=vocab + 5)(ids, scores.clone())[0]
        assert set(torch.nonzero(torch.isinf(got)).flatten().tolist()) == R.banned_ids(h, 0, 0, recs), (h, recs)


def test_first_stop_cut_is_exact_at_text_level():
    from tiny_tok import make_bpe_tokenizer, make_tokenizer
    tok = make_tokenizer()
    ids = tok.encode("w1 w2 w3 w4 w5 w6")
    dec = lambda x: tok.decode(x, skip_special_tokens=True)   # noqa: E731
    # a string split across tokens: found after its last token, cut before its first character
    assert hostloop.first_stop_cut(tok, ids, ["w3 w4"]) == (4, "w1 w2 ") == R.text_cut(dec, ids, ["w3 w4"])
    assert hostloop.first_stop_cut(tok, ids, ["w9", "w5", "w2 w3"]) == (3, "w1 ")          # the earliest hit wins
    assert hostloop.first_stop_cut(tok, ids, ["w7"]) is None and hostloop.first_stop_cut(tok, [], ["w1"]) is None
    assert hostloop.first_stop_cut(tok, ids, ["w2"], min_new=4) == (4, "w1 ")              # (held back, then cut at the same text)
    assert hostloop.stop_string_records(tok, ["w3 w4", "w3 w4", "w9"]) == [[3, 4], [9]]
    # a prefix of a longer word is a hit at text level though no token sequence of the device's record occurs
    ids2 = tok.encode("w1 w23 w4")
    assert hostloop.first_stop_cut(tok, ids2, ["w2"]) == (2, "w1 ") and hostloop.first_stop_hit(ids2, [tok.encode("w2")]) is None
    # a string reachable by two tokenizations (byte-level BPE: merged pieces, or the same text spelled in smaller pieces)
    bpe = make_bpe_tokenizer()
    s = " w3 w6"
    merged = bpe.encode(" w9" + s + " w12")
    pieces = bpe.encode(" w9") + [t for ch in s for t in bpe.encode(ch)] + bpe.encode(" w12")
    assert merged != pieces and bpe.decode(merged) == bpe.decode(pieces)
    rec = hostloop.stop_string_records(bpe, [s])
    cut_m, cut_p = hostloop.first_stop_cut(bpe, merged, [s]), hostloop.first_stop_cut(bpe, pieces, [s])
    assert cut_m[1] == cut_p[1] == " w9"                                                   # the same text either way
    assert hostloop.first_stop_hit(merged, rec) == cut_m[0]                                 # the device's record ends the merged run there
    assert hostloop.first_stop_hit(pieces, rec) is None                                     # ... and the other runs on, cut by the host
    assert cut_m == R.text_cut(lambda x: bpe.decode(x, skip_special_tokens=True), merged, [s])


# ---------------------------------------------------------------- host layers on stubs
class RulesStubEngine(AdjustStubEngine):
    def set_token_rules(self, slot, no_repeat_ngram_size=0, stop=(), bad_words=(), context=None):
        self.log.append(("rules", slot, no_repeat_ngram_size, [list(r) for r in stop], [list(r) for r in bad_words],
                         None if context is None else list(context)))


def rules_before_begin(log):
    out = {}
    for i, ev in enumerate(log):
        if ev[0] == "begin":
            j = max(k for k in range(i) if log[k][0] in ("reset", "truncate", "copy") and log[k][1] == ev[1])
            out[ev[2]] = [x[2:] for x in log[j + 1:i] if x[0] == "rules" and x[1] == ev[1]]
    return out


def test_scheduler_forwards_the_rules_with_the_prompt_as_context():
    model = la_model(max_seqs=2)
    model.engine = RulesStubEngine(max_seqs=2)
    sched = ChainScheduler(model, Proc(), burst=2, share_prefix=False)
    reqs = [Request(prompt="11 50 51", images=[], max_new_tokens=3, stop_ids=[[5, 6], [9]]),
            Request(prompt="12 50 51", images=[], max_new_tokens=3, bad_words_ids=[[4, 8]], no_repeat_ngram_size=3),
            Request(prompt="13 50 51", images=[], max_new_tokens=3),
            Request(prompt="14 50 51", images=[], max_new_tokens=3, stop_ids=[], bad_words_ids=[], no_repeat_ngram_size=0)]
    for r in reqs:
        sched.submit(r)
    sched.run()
    got = rules_before_begin(model.engine.log)
    assert got[11] == [(0, [[5, 6], [9]], [], None)]                 # (stop records never look at the context)
    assert got[12] == [(3, [], [[4, 8]], [12, 50, 51])]
    assert got[13] == [] and got[14] == []                           # no rules: nothing is forwarded
    # a chain that a stop sequence finished is retired with its ids cut behind the match (what follows is the device's pad)
    model = la_model(max_seqs=1)
    model.engine = RulesStubEngine(max_seqs=1)
    sched = ChainScheduler(model, Proc(), burst=2, share_prefix=False)
    r = Request(prompt="11 50 51", images=[], max_new_tokens=4, stop_ids=[[100, 100]])
    sched.submit(r)
    sched.run()
    assert list(r.tokens) == [100, 100]


def test_server_parses_forwards_and_rejects_the_fields():
    from tiny_tok import make_tokenizer
    from zoomearth_amd.serve import BadRequest, ChatServer, _Parsed

    srv = ChatServer(la_model(), Proc())
    msg = [{"role": "user", "content": "hi"}]
    p = srv._parse(dict(messages=msg))
    assert (p.stop, p.stop_token_ids, p.no_repeat_ngram_size) == ([], [], 0) and not p.rules() and not p.adjusts() and p.adjust_kw() == {}
    p = srv._parse(dict(messages=msg, stop="</answer>", stop_token_ids=[5, 2047], no_repeat_ngram_size=3))
    assert (p.stop, p.stop_token_ids, p.no_repeat_ngram_size) == (["</answer>"], [5, 2047], 3) and p.rules() and p.adjusts()
    kw = p.adjust_kw("TOK")
    assert kw["stop_strings"] == ["</answer>"] and kw["tokenizer"] == "TOK" and kw["stop_token_ids"] == [5, 2047]
    assert kw["no_repeat_ngram_size"] == 3
    assert srv._parse(dict(messages=msg, stop=["a", "b", "c", "d"])).stop == ["a", "b", "c", "d"]
    for bad in (dict(stop=5), dict(stop=["a", 5]), dict(stop=["a"] * 5), dict(stop=[""]), dict(stop={"a": 1}), dict(stop_token_ids="x"),
                dict(stop_token_ids=[2048]), dict(stop_token_ids=[-1]), dict(stop_token_ids=[1.5]), dict(stop_token_ids=[True]),
                dict(stop_token_ids=5), dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size="2"), dict(no_repeat_ngram_size=17),
                dict(no_repeat_ngram_size=1.5)):
        with pytest.raises(BadRequest):
            srv._parse(dict(messages=msg, **bad))
    with pytest.raises(BadRequest):                                   # routed like a request with adjustments: never batched
        srv.complete_many([dict(messages=msg, stop="x"), dict(messages=msg)])
    # the response: the text is cut BEFORE the stop string, a stop token id is kept; finish_reason is "stop"
    tok = make_tokenizer()
    srv = ChatServer(la_model(), type("P", (), {"tokenizer": tok})())
    out = tok.encode("w11 w12 w13 w14 w15") + [0, 0]   # (the stub model: EOS 3, pad 0)
    p = srv._parse(dict(messages=msg, stop=["w13 w14"], max_tokens=7))
    res = srv._response(p, out, 3)
    assert res["choices"][0]["message"]["content"] == "w11 w12" and res["choices"][0]["finish_reason"] == "stop"
    assert res["usage"]["completion_tokens"] == 4
    p = srv._parse(dict(messages=msg, stop_token_ids=[13], max_tokens=7))
    res = srv._response(p, out, 3)
    assert res["choices"][0]["message"]["content"] == "w11 w12 w13" and res["choices"][0]["finish_reason"] == "stop"
    assert res["usage"]["completion_tokens"] == 3
    p = srv._parse(dict(messages=msg, stop=["w9"], max_tokens=5))
    res = srv._response(p, out, 3)
    assert res["choices"][0]["message"]["content"] == "w11 w12 w13 w14 w15" and res["choices"][0]["finish_reason"] == "length"
    assert p.stop_records(tok) == [[9]] and isinstance(p, _Parsed)


def test_model_generate_forwards_the_rules_and_raises_hf_errors():
    from tiny_tok import make_tokenizer
    ids = torch.tensor([[11, 12, 13]])
    m = wrapper()
    log = []
    m.engine.set_token_rules = lambda slot, *a, **kw: log.append((slot,) + a + (kw.get("context"),))
    m.generate(input_ids=ids, max_new_tokens=2)
    m.generate(input_ids=ids, max_new_tokens=2, no_repeat_ngram_size=0, bad_words_ids=None, stop_token_ids=[], stop_strings=None)
    assert log == []                                                  # off values launch nothing
    m.generate(input_ids=ids, max_new_tokens=2, no_repeat_ngram_size=3, bad_words_ids=[[5, 6], [9]])
    assert log[-1][1:] == (3, [], [[5, 6], [9]], [11, 12, 13])
    m.generate(input_ids=ids, max_new_tokens=2, stop_token_ids=[7], stop_strings="w3 w4", tokenizer=make_tokenizer())
    assert log[-1][1:] == (0, [[7], [3, 4]], [], None)
    n = len(log)
    with pytest.raises(ValueError, match="could not locate a tokenizer"):
        m.generate(input_ids=ids, max_new_tokens=2, stop_strings=["x"])
    with pytest.raises(ValueError, match="strictly positive integer"):
        m.generate(input_ids=ids, max_new_tokens=2, no_repeat_ngram_size=-2)
    with pytest.raises(ValueError, match="non-empty list"):
        m.generate(input_ids=ids, max_new_tokens=2, bad_words_ids=[])
    with pytest.raises(ValueError, match="list of lists"):
        m.generate(input_ids=ids, max_new_tokens=2, bad_words_ids=[5])
    with pytest.raises(ValueError, match="list of positive integers"):
        m.generate(input_ids=ids, max_new_tokens=2, bad_words_ids=[[5, -1]])
    for bad in (dict(no_repeat_ngram_size=1.5), dict(no_repeat_ngram_size=17), dict(bad_words_ids=[[]]), dict(bad_words_ids="x"),
                dict(bad_words_ids=[[1.5]]), dict(stop_token_ids=[-1]), dict(stop_token_ids="5"), dict(bad_words_ids=[[1]] * 65),
                dict(bad_words_ids=[list(range(17))])):
        with pytest.raises(ValueError):
            m.generate(input_ids=ids, max_new_tokens=2, **bad)
    assert len(log) == n                                              # refused before anything ran
    with pytest.raises(ValueError, match="single token"):             # multi-token sequence_bias stays refused: bad_words_ids is the road
        m.generate(input_ids=ids, max_new_tokens=2, sequence_bias={(5, 6): 2.0})


def test_new_symbols_are_in_the_header_and_the_loader():
    from zoomearth_amd import _lib, engine

    with open(os.path.join(ROOT, "include", "zoomearth.h"), encoding="utf-8") as f:
        header = f.read()
    for name, val in (("ZE_MAX_RULE_INTS", 1024), ("ZE_MAX_RULE_WORDS", 64), ("ZE_MAX_RULE_LEN", 16)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), header), name
    assert (engine.MAX_RULE_INTS, engine.MAX_RULE_WORDS, engine.MAX_RULE_LEN) == (1024, 64, 16)
    assert engine.pack_records([[5, 6], [9]]).tolist() == [2, 5, 6, 1, 9]
    for name in ("ze_seq_set_token_rules", "ze_op_token_rules"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib._SIGS, name
        assert name in _lib.EXPORTS, name
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.lib()
    assert lib.ze_version() >= 104
    assert lib.ze_seq_set_token_rules is not None and lib.ze_op_token_rules is not None
    with open(os.path.join(ROOT, "zoomearth_amd", "csrc", "Makefile"), encoding="utf-8") as f:
        assert "ze_token_rules.hip" in f.read()

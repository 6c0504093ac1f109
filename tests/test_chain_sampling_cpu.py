"""CPU: per-chain sampling requests (ze_seq_set_sampling) -- the numpy restatement of one row (tests/chain_sampling_ref.py) checks
itself, and the host layers (scheduler, server) set, forward and reject a request's own values on recording stub engines."""
import os
import re
import threading

import numpy as np
import pytest
import torch

import chain_sampling_ref as R
from oracle import qwen25vl as Q
from test_logit_adjust_cpu import AdjustStubEngine, la_model
from test_sampling_filters_cpu import Proc
from test_scheduler_cpu import EOS, StubEngine, expected, make_model
from test_scheduler_cpu import Proc as WordProc
from zoomearth_amd.scheduler import ChainScheduler, Request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# ---------------------------------------------------------------- the reference checks itself
def test_greedy_rows_of_the_reference():
    l = np.asarray([1.0, 3.0, -2.0, 3.0, 0.5], dtype=f32)
    assert R.sample_row(l, [], 0.0, 1.0, 0, 0, 0) == (1, float("inf"))          # lowest index on a tie
    assert R.sample_row(l, [1], 0.0, 1.5, 0, 0, 0)[0] == 3                       # 3.0 / 1.5 = 2.0 < 3.0
    assert R.sample_row(l, [1, 3], 0.0, 8.0, 0, 0, 0)[0] == 0                    # both down to 0.375: 1.0 wins
    neg = np.asarray([-1.0, -1.5, -4.0], dtype=f32)
    assert R.sample_row(neg, [0], 0.0, 2.0, 0, 0, 0)[0] == 1                     # a negative score is multiplied: -2.0 < -1.5
    assert R.sample_row(l, [1], 0.0, 1.0, 0, 0, 0)[0] == 1                       # penalty 1: the seen-set does not matter
    nan = np.full(7, np.nan, dtype=f32)
    assert R.sample_row(nan, [], 0.0, 1.0, 0, 0, 0)[0] == 0                      # nothing comparable: torch.argmax gives 0
    nan[4] = -np.inf
    assert R.sample_row(nan, [], 0.0, 1.0, 0, 0, 0)[0] == 4                      # NaN is skipped, -inf is comparable
    assert R.greedy_token(l) == int(torch.argmax(torch.from_numpy(l)))


def test_sampled_rows_of_the_reference_are_the_oracles_draw():
    lg = (np.random.default_rng(5).normal(size=2000) * 3).astype(f32)
    for seed, stream, index, T, pen in ((1, 0, 0, 0.7, 1.0), (2, 3, 17, 1.0, 1.3), (9, 1, 300, 0.01, 1.3)):
        want = Q.sample_temperature(lg, [4, 9], pen, T, seed=seed, slot=stream, index=index)
        assert R.sample_row(lg, [4, 9], T, pen, seed, stream, index) == (int(want[0]), float(want[1]))
    # the seed, the stream and the index each move the draw; T -> 0 is the arg-max
    draws = {R.sample_row(lg, [], 1.0, 1.0, s, st, i)[0] for s in (1, 2) for st in (0, 1) for i in (0, 1)}
    assert len(draws) > 4
    assert {R.sample_row(lg, [], 0.01, 1.0, s, 0, i)[0] for s in range(3) for i in range(5)} == {int(lg.argmax())}
    # the frequencies follow softmax(l / T) (a coarse check of the distribution: 4000 draws on 8 tokens, 5 sigma)
    small = np.asarray([2.0, 1.0, 0.5, 0.0, -1.0, -1.0, 1.5, -3.0], dtype=f32)
    p = np.exp(small.astype(np.float64) / 0.8)
    p /= p.sum()
    n = 4000
    counts = np.bincount([R.sample_row(small, [], 0.8, 1.0, 77, 0, i)[0] for i in range(n)], minlength=8)
    assert (np.abs(counts - n * p) <= 5 * np.sqrt(n * p * (1 - p)) + 1).all(), (counts, n * p)


def test_gated_draws_of_the_unit_op_cases_stay_far_below_the_cap():
    """What the GPU test gates (draws whose CDF gap is below GAP) is a property of the inputs: counted here, on the reference alone."""
    for vocab, _, rows in R.SHAPES:
        draws = gated = 0
        for r in range(rows):
            lg, seen, T, pen, seed, stream = R.case_row(r, vocab)
            for i in R.INDICES:
                tok, gap = R.sample_row(lg, seen, T, pen, seed, stream, i)
                assert 0 <= tok < vocab
                if T > 0:
                    draws += 1
                    gated += gap <= R.GAP
        print(f"vocab {vocab} rows {rows}: {gated} of {draws} draws gated")
        assert gated <= 0.10 * max(draws, 1) / 2


# ---------------------------------------------------------------- scheduler on a recording stub
class SamplingStubEngine(AdjustStubEngine):
    def set_sampling(self, slot, do_sample=None, temperature=1.0, seed=0, repetition_penalty=1.0):
        self.log.append(("sampling", slot, do_sample, temperature, seed, repetition_penalty))


def sampling_before_begin(log):
    """first prompt id of every chain_begin -> [(what emptied the slot, the sampling calls on it since, the filter calls since)]"""
    out = {}
    for i, ev in enumerate(log):
        if ev[0] == "begin":
            j = max(k for k in range(i) if log[k][0] in ("reset", "truncate", "copy") and log[k][1] == ev[1])
            mine = [x for x in log[j + 1:i] if x[1] == ev[1]]
            out.setdefault(ev[2], []).append((log[j][0], [x[2:] for x in mine if x[0] == "sampling"], [x[2:] for x in mine if x[0] == "filter"]))
    return out


def test_scheduler_sets_a_requests_own_values_before_chain_begin():
    model = la_model(max_seqs=2)
    model.engine = SamplingStubEngine(max_seqs=2)
    sched = ChainScheduler(model, Proc(), do_sample=False, repetition_penalty=1.2, seed=4, burst=2, share_prefix=False)
    reqs = [Request(prompt="11 50 51", images=[], max_new_tokens=3, do_sample=True, temperature=0.8, seed=5, top_k=40),
            Request(prompt="12 50 51", images=[], max_new_tokens=3, repetition_penalty=1.3),          # greedy, its own penalty
            Request(prompt="13 50 51", images=[], max_new_tokens=3, top_k=40),                         # names none: the scheduler's
            Request(prompt="14 50 51", images=[], max_new_tokens=3, do_sample=True)]                  # only the mode: the rest is the scheduler's
    for r in reqs:
        sched.submit(r)
    sched.run()
    got = sampling_before_begin(model.engine.log)
    assert got[11] == [("reset", [(True, 0.8, 5, 1.2)], [(40, 1.0, 0.0)])]        # the filter too: its effective mode is sampled
    assert got[12] == [("reset", [(False, 1.0, 4, 1.3)], [])]
    assert got[13] == [("reset", [], [])]                                           # a greedy chain: no request, no filter
    assert got[14] == [("reset", [(True, 1.0, 4, 1.2)], [])]
    # a sampling scheduler: a request may turn greedy, and then has no filter
    model.engine = SamplingStubEngine(max_seqs=2)
    sched = ChainScheduler(model, Proc(), do_sample=True, temperature=0.9, seed=7, top_p=0.5, burst=2, share_prefix=False)
    for r in (Request(prompt="11 50 51", images=[], max_new_tokens=3, do_sample=False),
              Request(prompt="12 50 51", images=[], max_new_tokens=3)):
        sched.submit(r)
    sched.run()
    got = sampling_before_begin(model.engine.log)
    assert got[11] == [("reset", [(False, 0.9, 7, 1.0)], [])]
    assert got[12] == [("reset", [], [(0, 0.5, 0.0)])]


def test_a_request_that_names_no_value_never_touches_the_method():
    model = la_model(max_seqs=2)              # (its stub engine has no set_sampling at all)
    assert not hasattr(model.engine, "set_sampling")
    for do_sample in (False, True):
        sched = ChainScheduler(model, Proc(), do_sample=do_sample, temperature=1.0, burst=2, share_prefix=False)
        reqs = [Request(prompt=f"{11 + i} 50 51", images=[], max_new_tokens=3) for i in range(3)]
        for r in reqs:
            sched.submit(r)
        sched.run()
        assert all(len(r.tokens) == 3 for r in reqs)
    # ... and one that does reaches for it
    sched = ChainScheduler(model, Proc(), burst=2, share_prefix=False)
    errors = []
    sched.submit(Request(prompt="11 50 51", images=[], max_new_tokens=3, seed=3, on_error=lambda r, ex: errors.append(ex)))
    with pytest.raises(AttributeError):
        sched.run()


def test_scheduler_sets_the_values_again_after_a_stage_two_truncate():
    model = la_model(max_seqs=1)
    model.engine = SamplingStubEngine(max_seqs=1)
    sched = ChainScheduler(model, Proc(), burst=2, share_prefix=False)

    def done1(req, tokens, text):
        return Request(prompt=req.prompt + " 100 100 60", images=[], max_new_tokens=2, do_sample=True, temperature=0.5, seed=8)

    sched.submit(Request(prompt="11 50 51", images=[], max_new_tokens=3, repetition_penalty=1.1, on_done=done1))
    sched.run()
    # (the engine clears the request on truncate: the follow-up's own values are written afresh)
    assert sampling_before_begin(model.engine.log)[11] == [("reset", [(False, 1.0, 0, 1.1)], []), ("truncate", [(True, 0.5, 8, 1.0)], [])]


def test_a_requests_own_penalty_decides_whether_its_prompt_is_marked():
    class Marks(SamplingStubEngine):
        def mark_seen(self, slot, ids):
            self.log.append(("seen", slot, list(ids)))

    model = la_model(max_seqs=2)
    model.engine = Marks(max_seqs=2)
    sched = ChainScheduler(model, Proc(), burst=2, share_prefix=False)           # the scheduler's own penalty is 1.0
    for r in (Request(prompt="11 50 51", images=[], max_new_tokens=2, repetition_penalty=1.3),
              Request(prompt="12 50 51", images=[], max_new_tokens=2)):
        sched.submit(r)
    sched.run()
    assert [x[2] for x in model.engine.log if x[0] == "seen"] == [[11, 50, 51]]


# ---------------------------------------------------------------- server
def test_server_parses_forwards_and_rejects_the_fields():
    from zoomearth_amd.serve import BadRequest, ChatServer

    srv = ChatServer(la_model(), Proc())
    msg = [{"role": "user", "content": "hi"}]
    p = srv._parse(dict(messages=msg))
    assert (p.sample, p.temperature, p.seed, p.repetition_penalty) == (False, None, 0, None)
    p = srv._parse(dict(messages=msg, temperature=0.7, seed=11, repetition_penalty=1.25))
    assert (p.sample, p.temperature, p.seed, p.repetition_penalty) == (True, 0.7, 11, 1.25)
    assert srv._parse(dict(messages=msg, temperature=0, repetition_penalty=1)).repetition_penalty == 1.0
    for bad in (dict(repetition_penalty=0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("inf")),
                dict(repetition_penalty=float("nan")), dict(repetition_penalty="1.2"), dict(repetition_penalty=True)):
        with pytest.raises(BadRequest):
            srv._parse(dict(messages=msg, **bad))
    with pytest.raises(BadRequest):                                   # generate() gives every row of a call one penalty
        srv.complete_many([dict(messages=msg, repetition_penalty=1.2), dict(messages=msg)])


class GatedStub(StubEngine):
    """test_scheduler_cpu's engine with set_sampling; its first burst waits until the test has submitted one more request."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.decoding, self.go, self.requests = threading.Event(), threading.Event(), []

    def set_sampling(self, slot, do_sample=None, temperature=1.0, seed=0, repetition_penalty=1.0):
        self.requests.append((self.chains[slot]["ids"][0], do_sample, temperature, seed, repetition_penalty))

    def decode_burst(self, slots, steps, params):
        if not self.decoding.is_set():
            self.decoding.set()
            assert self.go.wait(timeout=30)
        return super().decode_burst(slots, steps, params)


def test_server_admits_a_sampled_request_into_the_running_greedy_batch(monkeypatch):
    from zoomearth_amd import scheduler, serve

    built = []

    class Counted(ChainScheduler):
        def __init__(self, *a, **kw):
            built.append((self, kw))
            super().__init__(*a, **kw)

    monkeypatch.setattr(scheduler, "ChainScheduler", Counted)
    model = make_model(max_seqs=3)
    model.engine = GatedStub(max_seqs=3)
    model.generate = lambda **kw: pytest.fail("the dispatcher never falls back to generate()")

    class SProc(WordProc):
        def __call__(self, text, images=None, return_tensors="pt", padding=None, **kw):
            body = text[0].split("user\n")[1].split("<|im_end|>")[0]
            return dict(input_ids=torch.tensor([[ord(c) % 50 + 10 for c in body[:4]]]))

    def req(text, **kw):
        return dict(messages=[{"role": "user", "content": text}], **kw)

    srv = serve.ChatServer(model, SProc(), "stub", batch_window_s=0.0)
    greedy = [srv.submit(req("aaaa", max_tokens=12)), srv.submit(req("cccc", max_tokens=12, repetition_penalty=1.5))]
    assert model.engine.decoding.wait(timeout=30)                    # the greedy chains are inside their first burst
    sampled = srv.submit(req("eeee", max_tokens=6, temperature=0.7, seed=9))
    model.engine.go.set()
    res = [f.result(timeout=30) for f in greedy + [sampled]]
    for r, c, n in zip(res, "ace", (12, 12, 6)):
        want = expected(ord(c) % 50 + 10, n)
        assert r["choices"][0]["message"]["content"] == " ".join(str(t) for t in want if t != EOS)
    assert len(built) == 1 and built[0][0] is srv.scheduler and built[0][1]["do_sample"] is False
    assert srv.scheduler.stats["admitted"] == 3
    bursts = [x for x in model.engine.log if x[0] == "burst"]
    assert any(x[1] == 3 for x in bursts)                            # the three chains shared a burst
    first = ord("e") % 50 + 10
    assert model.engine.requests == [(ord("c") % 50 + 10, False, 1.0, 0, 1.5), (first, True, 0.7, 9, 1.0)]
    srv.close()


# ---------------------------------------------------------------- the ABI's surfaces
def test_new_symbols_are_in_the_header_and_the_loader():
    from zoomearth_amd import _lib, engine

    with open(os.path.join(ROOT, "include", "zoomearth.h"), encoding="utf-8") as f:
        header = f.read()
    for name in ("ze_seq_set_sampling", "ze_op_sample_rows"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib._SIGS, name
    assert callable(engine.Engine.set_sampling) and callable(engine.Engine.sample_rows)

"""CPU: the logit-adjustment restatement on hand-worked rows, the host layers (scheduler, server, model wrapper) on stubs, and
the presence of the C entry points."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import logit_adjust_ref as R
from test_sampling_filters_cpu import EOS, PAD, FilterStubEngine, Proc, wrapper
from zoomearth_amd.scheduler import ChainScheduler, Request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_restatement_on_hand_worked_rows():
    l = np.asarray([1.0, -2.0, 0.5, 3.0, -0.0, 0.25], dtype=F)
    # no request: the very bits, the sign of -0 included
    assert R.adjust_row(l).tobytes() == l.tobytes()
    # presence 0.5, frequency 0.25 over counts (0, 1, 4, 0, 0, 2): t = (0, 0.75, 1.5, 0, 0, 1.0)
    a = R.adjust_row(l, counts=[0, 1, 4, 0, 0, 2], presence=0.5, frequency=0.25)
    assert a.tolist() == [1.0, -2.75, -1.0, 3.0, 0.0, -0.75] and a.dtype == F
    assert not np.signbit(a[4])                                    # (-0 + 0) - 0 = +0: a row WITH a request is recomputed
    # negative penalties reward repeats
    assert R.adjust_row(l, counts=[0, 2, 0, 0, 0, 0], presence=-1.0, frequency=-0.5).tolist() == [1.0, 0.0, 0.5, 3.0, 0.0, 0.25]
    # bias: finite and -inf (banned); the penalty of a biased token still applies
    a = R.adjust_row(l, counts=[0, 0, 0, 3, 0, 0], frequency=1.0, bias={3: 2.0, 0: float("-inf"), 5: -0.25})
    assert a.tolist() == [-np.inf, -2.0, 0.5, 2.0, 0.0, 0.0]
    # EOS masking is applied last: it beats a +100 bias, and only while masked
    a = R.adjust_row(l, bias={2: 100.0}, eos_ids=(2, 5, 77), eos_masked=True)
    assert a.tolist() == [1.0, -2.0, -np.inf, 3.0, 0.0, -np.inf]
    assert R.adjust_row(l, bias={2: 100.0}, eos_ids=(2, 5), eos_masked=False).tolist() == [1.0, -2.0, 100.5, 3.0, 0.0, 0.25]
    # each operation is rounded on its own: (l + b) - t, with t = f * c (+ p), is not l + (b - t)
    l1 = np.asarray([1e8], dtype=F)
    a = R.adjust_row(l1, counts=[3], presence=1.0, frequency=1.0, bias={0: 4.0})
    assert a[0] == F(F(l1[0] + F(4.0)) - F(F(F(1.0) * F(3.0)) + F(1.0)))
    f, c = F(0.1), 7
    assert R.adjust_row([0.0], counts=[c], presence=0.3, frequency=f)[0] == F(F(0.0) - F(F(f * F(c)) + F(0.3)))


def test_counts_saturate_at_65535():
    c = R.saturating_counts([4] * 70000 + [2] * 65535 + [1], 6)
    assert c.dtype == np.uint16 and c.tolist() == [0, 1, 65535, 0, 65535, 0]
    a = R.adjust_row(np.zeros(6, F), counts=c, presence=0.0, frequency=1.0)
    assert a.tolist() == [0.0, -1.0, -65535.0, 0.0, -65535.0, 0.0]
    assert R.argmax_lowest([1.0, 3.0, 3.0, np.nan]) == 1


# ---------------------------------------------------------------- host layers on stubs
class AdjustStubEngine(FilterStubEngine):
    def seq_set_logit_adjust(self, slot, presence_penalty=0.0, frequency_penalty=0.0, min_new_tokens=0, logit_bias=None):
        self.log.append(("adjust", slot, presence_penalty, frequency_penalty, min_new_tokens, dict(logit_bias or {})))


def la_model(**kw):
    cfg = SimpleNamespace(image_token_id=7, eos_token_ids=(EOS,), pad_token_id=PAD, vision=SimpleNamespace(spatial_merge_size=2),
                          text=SimpleNamespace(vocab_size=2048))
    return SimpleNamespace(engine=AdjustStubEngine(**kw), config=cfg, _chains={}, device="cpu",
                           generation_config=SimpleNamespace(repetition_penalty=1.0, temperature=None))


def adjusts_before_begin(log):
    """first prompt id of every chain_begin -> (what emptied the slot, the adjust calls on it since)"""
    out = {}
    for i, ev in enumerate(log):
        if ev[0] == "begin":
            j = max(k for k in range(i) if log[k][0] in ("reset", "truncate", "copy") and log[k][1] == ev[1])
            out.setdefault(ev[2], []).append((log[j][0], [x[2:] for x in log[j + 1:i] if x[0] == "adjust" and x[1] == ev[1]]))
    return out


@pytest.mark.parametrize("do_sample", [False, True])
def test_scheduler_sets_each_requests_own_values_before_its_first_draw(do_sample):
    model = la_model(max_seqs=2)
    sched = ChainScheduler(model, Proc(), do_sample=do_sample, temperature=1.0, burst=2, share_prefix=False, frequency_penalty=0.25)
    reqs = [Request(prompt="11 50 51", images=[], max_new_tokens=3, presence_penalty=0.5, logit_bias={9: -100.0}),
            Request(prompt="12 50 51", images=[], max_new_tokens=3, min_new_tokens=2, frequency_penalty=-1.0),
            Request(prompt="13 50 51", images=[], max_new_tokens=3),                              # the scheduler's default
            Request(prompt="14 50 51", images=[], max_new_tokens=3, frequency_penalty=0.0)]       # explicitly off
    for r in reqs:
        sched.submit(r)
    sched.run()
    got = adjusts_before_begin(model.engine.log)
    assert got[11] == [("reset", [(0.5, 0.25, 0, {9: -100.0})])]
    assert got[12] == [("reset", [(0.0, -1.0, 2, {})])]
    assert got[13] == [("reset", [(0.0, 0.25, 0, {})])]
    assert got[14] == [("reset", [])]                               # off values forward nothing: the reset cleared the slot
    # a scheduler without defaults and requests without values never touch the tables
    model = la_model(max_seqs=1)
    sched = ChainScheduler(model, Proc(), do_sample=do_sample, temperature=1.0, burst=2, share_prefix=False)
    sched.submit(Request(prompt="15 50 51", images=[], max_new_tokens=2, presence_penalty=0.0, logit_bias={}, min_new_tokens=0))
    sched.run()
    assert not [x for x in model.engine.log if x[0] == "adjust"]


def test_scheduler_sets_the_request_again_for_a_follow_up_on_a_parked_slot():
    model = la_model(max_seqs=1)
    sched = ChainScheduler(model, Proc(), burst=2, share_prefix=False)

    def done1(req, tokens, text):
        return Request(prompt=req.prompt + " 100 100 60", images=[], max_new_tokens=2, frequency_penalty=0.5)

    sched.submit(Request(prompt="11 50 51", images=[], max_new_tokens=3, presence_penalty=1.0, on_done=done1))
    sched.run()
    # (the engine clears request and counts on truncate: the follow-up's own request starts from zero counts)
    assert adjusts_before_begin(model.engine.log)[11] == [("reset", [(1.0, 0.0, 0, {})]), ("truncate", [(0.0, 0.5, 0, {})])]


def test_server_parses_forwards_and_rejects_the_fields():
    from zoomearth_amd.serve import BadRequest, ChatServer

    srv = ChatServer(la_model(), Proc())
    msg = [{"role": "user", "content": "hi"}]
    p = srv._parse(dict(messages=msg))
    assert (p.presence_penalty, p.frequency_penalty, p.logit_bias, p.min_tokens) == (0.0, 0.0, {}, 0)
    assert not p.adjusts() and p.adjust_kw() == {}
    p = srv._parse(dict(messages=msg, presence_penalty=-2, frequency_penalty=1.5, logit_bias={"17": -100, "2047": 3.5}, min_tokens=4))
    assert (p.presence_penalty, p.frequency_penalty, p.logit_bias, p.min_tokens) == (-2.0, 1.5, {17: -100.0, 2047: 3.5}, 4)
    assert p.adjusts() and p.adjust_kw() == dict(presence_penalty=-2.0, frequency_penalty=1.5, logit_bias={17: -100.0, 2047: 3.5},
                                                 min_new_tokens=4)
    assert srv._parse(dict(messages=msg, logit_bias={str(i): 1 for i in range(300)})).adjusts()
    for bad in (dict(presence_penalty=2.1), dict(presence_penalty=-2.5), dict(presence_penalty="1"), dict(presence_penalty=True),
                dict(frequency_penalty=3), dict(frequency_penalty=float("nan")), dict(frequency_penalty=[1]),
                dict(logit_bias=[1, 2]), dict(logit_bias={"x": 1}), dict(logit_bias={"2048": 1}), dict(logit_bias={"-1": 1}),
                dict(logit_bias={"5": 101}), dict(logit_bias={"5": -100.5}), dict(logit_bias={"5": "1"}), dict(logit_bias={"5": None}),
                dict(logit_bias={"5": 1, "05": 2}), dict(logit_bias={str(i): 1 for i in range(301)}),
                dict(min_tokens=-1), dict(min_tokens=2.5), dict(min_tokens="3"), dict(min_tokens=True)):
        with pytest.raises(BadRequest):
            srv._parse(dict(messages=msg, **bad))
    # a request that carries adjustments is never batched with others: generate() gives every row the same values
    with pytest.raises(BadRequest):
        srv.complete_many([dict(messages=msg, frequency_penalty=1.0), dict(messages=msg)])


def test_model_generate_forwards_the_request_and_raises_hf_errors():
    ids = torch.tensor([[11, 12, 13]])
    m = wrapper()
    log = []
    m.engine.seq_set_logit_adjust = lambda slot, *a: log.append((slot,) + a)
    m.generate(input_ids=ids, max_new_tokens=2)
    m.generate(input_ids=ids, max_new_tokens=2, min_new_tokens=0, presence_penalty=0.0, frequency_penalty=0, logit_bias={},
               suppress_tokens=[], sequence_bias=None)
    assert log == []                                               # off values launch nothing
    m.generate(input_ids=ids, max_new_tokens=2, min_new_tokens=3, sequence_bias={(5,): 2.5, (9,): -1.0}, frequency_penalty=0.7)
    assert log[-1][1:] == (0.0, 0.7, 3, {5: 2.5, 9: -1.0})
    m.generate(input_ids=ids, max_new_tokens=2, do_sample=True, suppress_tokens=[4, 8], logit_bias={8: 5.0, 6: -2}, presence_penalty=-1)
    assert log[-1][1:] == (-1.0, 0.0, 0, {8: float("-inf"), 6: -2.0, 4: float("-inf")})     # suppress wins over a bias
    m.generate(input_ids=ids, max_new_tokens=2, sequence_bias=[[[5], 1.5]])                 # HF's list-of-lists form
    assert log[-1][1:] == (0.0, 0.0, 0, {5: 1.5})
    n = len(log)
    with pytest.raises(ValueError, match="single token"):
        m.generate(input_ids=ids, max_new_tokens=2, sequence_bias={(5, 6): 2.0})
    for bad in (dict(min_new_tokens=-1), dict(min_new_tokens=1.5), dict(min_new_tokens="2"), dict(sequence_bias={}),
                dict(sequence_bias="x"), dict(sequence_bias={5: 1.0}), dict(sequence_bias={(): 1.0}), dict(sequence_bias={(-1,): 1.0}),
                dict(sequence_bias={(5,): 1}), dict(sequence_bias={("a",): 1.0}), dict(suppress_tokens=[-1]), dict(suppress_tokens=[1.5]),
                dict(logit_bias=[1]), dict(logit_bias={5: "x"}), dict(presence_penalty="1"), dict(frequency_penalty=float("inf")),
                dict(logit_bias={i: 1.0 for i in range(513)})):
        with pytest.raises(ValueError):
            m.generate(input_ids=ids, max_new_tokens=2, **bad)
    assert len(log) == n and len(m.engine.calls) == 5               # refused before anything ran


def test_new_symbols_are_in_the_header_and_the_loader():
    from zoomearth_amd import _lib

    with open(os.path.join(ROOT, "include", "zoomearth.h"), encoding="utf-8") as f:
        header = f.read()
    assert re.search(r"#define\s+ZE_MAX_LOGIT_BIAS\s+512\b", header)
    for name in ("ze_seq_set_logit_adjust", "ze_op_logit_adjust"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib._SIGS, name
        assert name in _lib.EXPORTS, name
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.lib()
    assert lib.ze_version() >= 103
    assert lib.ze_seq_set_logit_adjust is not None and lib.ze_op_logit_adjust is not None
    with open(os.path.join(ROOT, "zoomearth_amd", "csrc", "Makefile"), encoding="utf-8") as f:
        assert "ze_logit_adjust.hip" in f.read()

"""CPU: the log-probability definition against torch, tie rows, the host layers (scheduler, server, model wrapper) on stubs,
and the presence of the C entry points."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import logprobs_ref as R
from test_sampling_filters_cpu import EOS, PAD, FilterStubEngine, Proc, wrapper
from zoomearth_amd.scheduler import ChainScheduler, Request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("vocab", [2048, 151936])
def test_restatement_equals_torch_on_rows_without_ties(vocab):
    g = torch.Generator().manual_seed(vocab)
    lg = (torch.randn((6, vocab), generator=g) * 4).float()
    tg = torch.randint(0, vocab, (6,), generator=g)
    for n in (0, 1, 5, 20):
        ok = R.decided(lg.numpy(), 20)    # (no exact tie among the 21 largest: torch.topk's order is then the only one)
        assert ok.all()
        lp, ids, tlp = R.token_logprobs_ref(lg.numpy(), tg.numpy(), n)
        ls = torch.log_softmax(lg.double(), -1)
        assert np.abs(lp - ls.gather(1, tg[:, None])[:, 0].numpy()).max() < 1e-12
        if n:
            v, i = torch.topk(lg, n, dim=-1)
            assert np.array_equal(ids, i.numpy().astype(np.int32))
            assert np.abs(tlp - ls.gather(1, i).numpy()).max() < 1e-12
            assert (np.diff(tlp, axis=1) <= 0).all()


def test_restatement_on_tie_rows():
    flat = np.full((1, 2048), 0.25, dtype=np.float32)
    lp, ids, tlp = R.token_logprobs_ref(flat, [7], 5)
    assert ids[0].tolist() == [0, 1, 2, 3, 4] and np.allclose(tlp, -np.log(2048)) and np.isclose(lp[0], -np.log(2048))
    row = np.zeros((1, 2048), dtype=np.float32)
    row[0, [900, 17]] = 3.0                                   # the maximum twice: the lower id first
    row[0, [5, 1000]] = 1.0
    _, ids, tlp = R.token_logprobs_ref(row, [0], 5)
    assert ids[0].tolist() == [17, 900, 5, 1000, 0] and tlp[0, 0] == tlp[0, 1] and tlp[0, 2] == tlp[0, 3]
    assert not R.decided(flat, 5)[0] and R.decided(row, 2)[0] and not R.decided(row, 1)[0]
    masked = np.full((1, 2048), -np.inf, dtype=np.float32)
    masked[0, [3, 30, 300]] = [0.0, 2.0, 1.0]
    lp, ids, tlp = R.token_logprobs_ref(masked, [30], 5)
    assert ids[0].tolist() == [30, 300, 3, -1, -1] and np.isneginf(tlp[0, 3:]).all() and np.isfinite(tlp[0, :3]).all()
    big = np.zeros((1, 2048), dtype=np.float32)
    big[0, 77] = 1e4
    lp, ids, tlp = R.token_logprobs_ref(big, [77], 1)
    assert lp[0] == 0.0 and ids[0, 0] == 77 and tlp[0, 0] == 0.0


# ---------------------------------------------------------------- host layers on stubs
class LogprobStubEngine(FilterStubEngine):
    def set_logprobs(self, slot, top_n=0):
        self.log.append(("logprobs", slot, top_n))
        self.chains[slot]["lp"] = top_n

    def seq_truncate(self, slot, keep):
        super().seq_truncate(slot, keep)
        self.chains[slot].pop("lp", None)          # the engine clears the request with the filter

    def chain_logprobs(self, slot, cap=0):
        n, c = self.chains[slot]["lp"], self.chains[slot]
        m = len(c["out"][: cap or None])
        return (np.full(m, -0.5, np.float32), np.tile(np.arange(n, dtype=np.int32), (m, 1)),
                np.tile(-np.arange(1, n + 1, dtype=np.float32), (m, 1)))


def lp_model(**kw):
    cfg = SimpleNamespace(image_token_id=7, eos_token_ids=(EOS,), pad_token_id=PAD, vision=SimpleNamespace(spatial_merge_size=2))
    return SimpleNamespace(engine=LogprobStubEngine(**kw), config=cfg, _chains={}, device="cpu",
                           generation_config=SimpleNamespace(repetition_penalty=1.0, temperature=None))


def sets_before_begin(log):
    """first prompt id of every chain_begin -> the set_logprobs calls on its slot since the slot's last reset / truncate / copy"""
    out = []
    for i, ev in enumerate(log):
        if ev[0] == "begin":
            j = max(k for k in range(i) if log[k][0] in ("reset", "truncate", "copy") and log[k][1] == ev[1])
            out.append((ev[2], log[j][0], [x[2] for x in log[j + 1:i] if x[0] == "logprobs" and x[1] == ev[1]]))
    return out


def test_scheduler_sets_the_request_after_prefill_and_attaches_results():
    model = lp_model(max_seqs=2)
    sched = ChainScheduler(model, Proc(), burst=2, share_prefix=False, logprobs=None)
    seen = {}

    def done(req, tokens, text):
        seen[req.prompt] = (list(tokens), list(req.token_logprobs), [list(x) for x in req.top_logprobs])

    reqs = [Request(prompt="11 50 51", images=[], max_new_tokens=3, logprobs=3, on_done=done),
            Request(prompt="12 50 51", images=[], max_new_tokens=4, logprobs=0, on_done=done),
            Request(prompt="13 50 51", images=[], max_new_tokens=3, on_done=done)]           # none: nothing is set or fetched
    for r in reqs:
        sched.submit(r)
    sched.run()
    by_first = {first: sets for first, _, sets in sets_before_begin(model.engine.log)}
    assert by_first == {11: [3], 12: [0], 13: []}
    toks, lps, tops = seen["11 50 51"]
    assert len(toks) == 3 and lps == [-0.5] * 3 and tops == [[(0, -1.0), (1, -2.0), (2, -3.0)]] * 3
    toks, lps, tops = seen["12 50 51"]
    assert len(toks) == 4 and len(lps) == 4 and tops == [[]] * 4
    assert seen["13 50 51"][1:] == ([], [])
    # the scheduler-wide default reaches a request that names none
    model = lp_model(max_seqs=1)
    sched = ChainScheduler(model, Proc(), burst=2, share_prefix=False, logprobs=2)
    r = Request(prompt="14 50 51", images=[], max_new_tokens=2)
    sched.submit(r)
    sched.run()
    assert len(r.token_logprobs) == len(r.tokens) == 2 and [len(x) for x in r.top_logprobs] == [2, 2]


def test_scheduler_sets_the_request_again_after_a_stage_two_truncate():
    model = lp_model(max_seqs=1)
    sched = ChainScheduler(model, Proc(), burst=2, share_prefix=False, logprobs=1)
    got = []

    def done2(req, tokens, text):
        got.append(("two", len(tokens), len(req.token_logprobs)))

    def done1(req, tokens, text):
        got.append(("one", len(tokens), len(req.token_logprobs)))
        return Request(prompt=req.prompt + " 100 100 60", images=[], max_new_tokens=2, on_done=done2)   # continues on the slot

    sched.submit(Request(prompt="11 50 51", images=[], max_new_tokens=3, on_done=done1))
    sched.run()
    assert got == [("one", 3, 3), ("two", 2, 2)]
    begins = sets_before_begin(model.engine.log)
    assert [(b[1], b[2]) for b in begins] == [("reset", [1]), ("truncate", [1])]


class Tok:
    @staticmethod
    def decode(ids, skip_special_tokens=True):
        return " ".join(f"t{int(i)}" for i in ids if not (skip_special_tokens and int(i) == EOS))


def test_server_rejects_bad_fields_and_shapes_the_block():
    from zoomearth_amd.serve import BadRequest, ChatServer

    srv = ChatServer(lp_model(), SimpleNamespace(tokenizer=Tok))
    msg = [{"role": "user", "content": "hi"}]
    assert srv._parse(dict(messages=msg)).logprobs is None
    assert srv._parse(dict(messages=msg, logprobs=False)).logprobs is None
    assert srv._parse(dict(messages=msg, logprobs=True)).logprobs == 0
    assert srv._parse(dict(messages=msg, logprobs=True, top_logprobs=20)).logprobs == 20
    for bad in (dict(top_logprobs=3), dict(logprobs=False, top_logprobs=3), dict(logprobs=True, top_logprobs=21),
                dict(logprobs=True, top_logprobs=-1), dict(logprobs=True, top_logprobs=2.5), dict(logprobs=True, top_logprobs="3"),
                dict(logprobs=True, top_logprobs=True), dict(logprobs=1)):
        with pytest.raises(BadRequest):
            srv._parse(dict(messages=msg, **bad))
    p = srv._parse(dict(messages=msg, logprobs=True, top_logprobs=2, max_tokens=8))
    lp = ([-0.1, -0.2, -0.3, -9.0], [[(5, -0.1), (6, -1.0)], [(6, -0.2), (5, -2.0)], [(EOS, -0.3), (9, -3.0)], [(1, -1.0), (2, -2.0)]])
    res = srv._response(p, [5, 6, EOS, PAD], 3, lp)
    c = res["choices"][0]
    assert list(c) == ["index", "message", "logprobs", "finish_reason"] and c["finish_reason"] == "stop"
    content = c["logprobs"]["content"]
    assert len(content) == res["usage"]["completion_tokens"] == 3               # one entry per returned token, EOS included
    assert [x["token"] for x in content] == ["t5", "t6", f"t{EOS}"] and [x["logprob"] for x in content] == [-0.1, -0.2, -0.3]
    assert all(set(x) == {"token", "logprob", "bytes", "top_logprobs"} and x["bytes"] == list(x["token"].encode()) for x in content)
    assert [[t["token"] for t in x["top_logprobs"]] for x in content] == [["t5", "t6"], ["t6", "t5"], [f"t{EOS}", "t9"]]
    assert all(set(t) == {"token", "logprob", "bytes"} for x in content for t in x["top_logprobs"])
    # without the field the response is what it always was
    plain = srv._response(srv._parse(dict(messages=msg, max_tokens=8)), [5, 6, EOS, PAD], 3)
    assert list(plain["choices"][0]) == ["index", "message", "finish_reason"] and "logprobs" not in plain["choices"][0]
    assert plain["choices"][0]["message"] == c["message"] and plain["usage"] == res["usage"]


def test_model_generate_checks_logprobs_and_returns_the_tensors():
    ids = torch.tensor([[11, 12, 13]])
    m = wrapper()
    for bad in (-1, 21, 2.5, "3", True):
        with pytest.raises(ValueError):
            m.generate(input_ids=ids, max_new_tokens=2, logprobs=bad)
    assert not m.engine.calls                                   # refused before anything ran
    assert isinstance(m.generate(input_ids=ids, max_new_tokens=2), torch.Tensor)
    log = []
    m.engine.set_logprobs = lambda slot, n: log.append((slot, n))
    m.engine.chain_logprobs = lambda slot, cap=0: (np.full(2, -0.25, np.float32), np.tile(np.arange(3, dtype=np.int32), (2, 1)),
                                                   np.tile(-np.arange(1, 4, dtype=np.float32), (2, 1)))
    out = m.generate(input_ids=ids, max_new_tokens=2, logprobs=3)
    assert [n for _, n in log] == [3] and out.sequences.shape == (1, 5)
    assert out.logprobs.dtype == torch.float32 and out.logprobs.tolist() == [[-0.25, -0.25]]
    assert out.top_ids.shape == (1, 2, 3) and out.top_ids[0, 1].tolist() == [0, 1, 2]
    assert out.top_logprobs.shape == (1, 2, 3) and out.top_logprobs[0, 0].tolist() == [-1.0, -2.0, -3.0]


def test_new_symbols_are_in_the_header_and_the_loader():
    from zoomearth_amd import _lib

    with open(os.path.join(ROOT, "include", "zoomearth.h"), encoding="utf-8") as f:
        header = f.read()
    assert re.search(r"#define\s+ZE_MAX_TOP_LOGPROBS\s+20\b", header)
    for name in ("ze_seq_set_logprobs", "ze_chain_logprobs", "ze_chain_logprobs_batch", "ze_op_token_logprobs"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib._SIGS, name

"""CPU: the host side of prompt log-probabilities (ze_score_batch_detail) -- the numpy restatement of the kernel against float64,
the scheduler's choice of pass on the stub engine of tests/test_scheduler_cpu.py, and the server's parsing and response shape."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import score_detail_ref as R
from test_scheduler_cpu import EOS, PAD, Proc, StubEngine, make_model
from zoomearth_amd.engine import ScoreDetail
from zoomearth_amd.scheduler import ChainScheduler, Request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the reference
def _rows():
    rng = np.random.default_rng(0)
    rows = [R.to_bf16(rng.standard_normal(n).astype(np.float32) * 3) for n in (8, 77, 1003, 4099)]
    rows.append(R.to_bf16(np.round(rng.standard_normal(3001) * 2).astype(np.float32)))       # nine or so distinct values
    rows.append(np.full(2500, -2.25, np.float32))
    holes = R.to_bf16(rng.standard_normal(600).astype(np.float32))
    holes[::2] = -np.inf
    rows.append(holes)
    return rows


@pytest.mark.parametrize("k", range(7))
def test_reference_against_float64_log_softmax_and_a_stable_sort(k):
    l = _rows()[k]
    n = len(l)
    z = l.astype(np.float64)
    logp = z - z.max() - np.log(np.exp(z - z.max()).sum())
    with np.errstate(invalid="ignore"):                         # (0 * -inf where an entry is -inf: not taken)
        ent64 = -np.sum(np.where(np.isfinite(logp), np.exp(logp) * logp, 0.0))
    stable = np.argsort(-z, kind="stable")                       # value descending, ties in id order
    stable = stable[np.isfinite(z[stable])]
    for target in (0, n // 2, n - 1):
        lp, ent, rank, ids, tlp = R.score_detail(l, target, 20)
        if np.isfinite(logp[target]):
            assert abs(float(lp) - logp[target]) <= 2e-5
            assert rank == int(np.nonzero(stable == target)[0][0])
        assert abs(float(ent) - ent64) <= 1e-4
        m = min(20, len(stable))
        assert ids[:m].tolist() == stable[:m].tolist() and ids[m:].tolist() == [-1] * (20 - m)
        assert np.allclose(tlp[:m], logp[stable[:m]], atol=2e-5) and np.all(np.isneginf(tlp[m:]))
    assert R.score_detail(l, -1, 0)[:3:2] == (np.float32(0), -1) and R.score_detail(l, n, 0)[2] == -1


def test_reference_row_without_a_finite_maximum():
    lp, ent, rank, ids, tlp = R.score_detail(np.full(40, -np.inf, np.float32), 3, 4)
    assert np.isnan(ent) and rank == -1 and ids.tolist() == [-1] * 4 and np.all(np.isneginf(tlp))


# ---------------------------------------------------------------- the scheduler
class DetailEngine(StubEngine):
    """The stub with the scoring form of the pass: position j of a chain's new ids scores -(j + 1) / 8, rank j, ids 40 + j .."""

    def score_batch_detail(self, slots, ids_l, emb_l, pos_l, dl, score_from=None, top_n=0, entropy=False, rank=False):
        self.log.append(("score_detail", list(slots), [len(x) for x in ids_l], list(score_from), top_n, entropy, rank))
        StubEngine.prefill_batch(self, slots, ids_l, emb_l, pos_l, dl)
        self.log.pop()                                            # (the pass is ONE engine call: no "prefill" entry of its own)
        lps, ranks, tids, tlps, off = [], [], [], [], [0]
        for ids, sf in zip(ids_l, score_from):
            for j in range(sf, len(ids) - 1):
                lps.append(-(j + 1) / 8)
                ranks.append(j)
                tids.append([40 + j + k for k in range(top_n)])
                tlps.append([-(k + 1) / 4 for k in range(top_n)])
            off.append(len(lps))
        t = torch.tensor
        return ScoreDetail(t(lps, dtype=torch.float32), None, t(ranks, dtype=torch.int32),
                           t(tids, dtype=torch.int32).reshape(-1, top_n) if top_n else None,
                           t(tlps, dtype=torch.float32).reshape(-1, top_n) if top_n else None, off)


def detail_model(**kw):
    m = make_model(**kw)
    e = DetailEngine(**kw)
    m.engine = e
    return m


def test_a_pass_with_one_asking_chain_scores_it_and_only_it():
    model = detail_model(max_seqs=4)
    sched = ChainScheduler(model, Proc(), burst=2, share_prefix=False)
    done = {}
    reqs = [Request(prompt="11 50 51 52", images=[], max_new_tokens=3, on_done=lambda r, t, x: done.__setitem__(0, list(t))),
            Request(prompt="12 60 61 62 63 64", images=[], max_new_tokens=3, prompt_logprobs=2,
                    on_done=lambda r, t, x: done.__setitem__(1, (list(t), list(r.prompt_token_logprobs), list(r.prompt_ranks),
                                                                 list(r.prompt_top_logprobs)))),
            Request(prompt="13 70", images=[], max_new_tokens=3, on_done=lambda r, t, x: done.__setitem__(2, list(t)))]
    for r in reqs:
        sched.submit(r)
    sched.run()
    calls = [x for x in model.engine.log if x[0] in ("prefill", "score_detail")]
    assert len(calls) == 1 and calls[0][0] == "score_detail"
    _, slots, lens, sf, top_n, entropy, rank = calls[0]
    asker = slots.index(reqs[1].slot)
    assert lens[asker] == 6 and sf[asker] == 0 and top_n == 2 and rank and not entropy
    assert all(sf[k] == lens[k] - 1 for k in range(3) if k != asker)      # the others: len - 1, nothing scored
    toks, lps, ranks, tops = done[1]
    assert lps == [None] + [-(j + 1) / 8 for j in range(5)] and ranks == [None, 0, 1, 2, 3, 4]
    assert tops[0] is None and tops[1] == [(40, -0.25), (41, -0.5)] and len(tops) == 6
    # the others' tokens and the asker's own are what a run without the request gives
    plain = make_model(max_seqs=4)
    sched0 = ChainScheduler(plain, Proc(), burst=2, share_prefix=False)
    want = {}
    for i, r in enumerate(reqs):
        sched0.submit(Request(prompt=r.prompt, images=[], max_new_tokens=3, on_done=lambda r, t, x, i=i: want.__setitem__(i, list(t))))
    sched0.run()
    assert [done[0], done[1][0], done[2]] == [want[0], want[1], want[2]]
    assert not reqs[0].prompt_token_logprobs and not reqs[2].prompt_ranks


def _shared_run(model, ask):
    sched = ChainScheduler(model, Proc(), burst=2, share_prefix=True, min_shared=3)
    out = {}
    reqs = []
    for q in range(4):
        reqs.append(Request(prompt=f"71 72 73 <img> {20 + q} 50", images=["viewA"], max_new_tokens=40 if q == 0 else 12,
                            prompt_logprobs=1 if q in ask else None,
                            on_done=lambda r, t, x, q=q: out.__setitem__(q, (list(t), r.n_prompt))))
        sched.submit(reqs[-1])
    sched.step()
    model.engine.log.append(("late",))                            # what follows belongs to the late request's round
    reqs.append(Request(prompt="71 72 73 <img> 33 50 51", images=["viewA"], max_new_tokens=3, prompt_logprobs=1 if 4 in ask else None,
                        on_done=lambda r, t, x: out.__setitem__(4, (list(t), r.n_prompt))))
    sched.submit(reqs[-1])
    sched.run()
    log = model.engine.log
    late = log.index(("late",))
    return out, [x for x in log if x != ("late",)], reqs, (log[:late], log[late + 1:])


def test_an_asking_chain_is_never_a_prefix_receiver_but_still_a_donor():
    plain = _shared_run(make_model(max_seqs=4), ())[0]
    for ask in ((0,), (2,), (4,), (0, 2)):
        out, log, reqs, (first, late) = _shared_run(detail_model(max_seqs=4), ask)
        assert out == plain
        copies = [x for x in log if x[0] == "copy"]
        for q in ask:
            mine = late if q == 4 else first                                         # (slots are handed on: the request's own round)
            assert all(c[1] != reqs[q].slot for c in mine if c[0] == "copy"), (ask, q)   # nothing is copied INTO its slot
            lps = reqs[q].prompt_token_logprobs
            assert len(lps) == reqs[q].n_prompt and lps[0] is None and all(v is not None for v in lps[1:])   # every row its own
        if ask == (0,):
            # alive, chain 0 donates its prefix to the later request as any chain does
            assert (reqs[4].slot, reqs[0].slot, 7) in [c[1:] for c in copies]
        assert len(copies) >= 1


def test_a_run_with_nobody_asking_makes_the_call_log_it_makes_today():
    log_stub = _shared_run(make_model(max_seqs=4), ())[1]
    log_detail = _shared_run(detail_model(max_seqs=4), ())[1]
    assert log_detail == log_stub and not [x for x in log_detail if x[0] == "score_detail"]
    pre = [x for x in log_stub if x[0] == "prefill"]
    assert pre[0][2] == [7] and sorted(pre[1][2]) == [2, 2, 2, 2]                   # (tests/test_scheduler_cpu.py's own figures)


def test_a_cached_prefix_of_the_own_slot_has_no_entries():
    model = detail_model(max_seqs=1)
    sched = ChainScheduler(model, Proc(), burst=2, share_prefix=False)
    got = {}

    def done2(req, tokens, text):
        got["two"] = (list(req.prompt_token_logprobs), req.n_prompt)

    def done1(req, tokens, text):
        nxt = req.prompt + " " + " ".join(str(t) for t in tokens if t not in (EOS, PAD)) + " 60 61"
        return Request(prompt=nxt, images=[], max_new_tokens=2, prompt_logprobs=0, on_done=done2)

    sched.submit(Request(prompt="11 50 51", images=[], max_new_tokens=3, on_done=done1))
    sched.run()
    lps, n = got["two"]
    tr = [x for x in model.engine.log if x[0] == "truncate"]
    assert tr and len(lps) == n
    keep = tr[0][2]
    assert keep >= 3 and all(v is None for v in lps[:keep + 1]) and all(v is not None for v in lps[keep + 1:]) and len(lps) > keep + 1


# ---------------------------------------------------------------- the server
class Tok:
    @staticmethod
    def decode(ids, skip_special_tokens=True):
        return " ".join(f"t{int(i)}" for i in ids if not (skip_special_tokens and int(i) == EOS))


def test_server_parses_prompt_logprobs_rejects_bad_values_and_shapes_the_list():
    from zoomearth_amd.serve import BadRequest, ChatServer

    srv = ChatServer(make_model(), SimpleNamespace(tokenizer=Tok))
    msg = [{"role": "user", "content": "hi"}]
    assert srv._parse(dict(messages=msg)).prompt_logprobs is None
    assert srv._parse(dict(messages=msg, prompt_logprobs=0)).prompt_logprobs == 0
    assert srv._parse(dict(messages=msg, prompt_logprobs=20)).prompt_logprobs == 20
    for bad in (21, -1, 2.5, "3", True, [1]):
        with pytest.raises(BadRequest, match="prompt_logprobs"):
            srv._parse(dict(messages=msg, prompt_logprobs=bad))
    with pytest.raises(BadRequest, match="prompt_logprobs"):
        srv.complete_many([dict(messages=msg, prompt_logprobs=1), dict(messages=msg)])
    p = srv._parse(dict(messages=msg, prompt_logprobs=2, max_tokens=8))
    prompt = ([9, 5, 6, 7], [None, -0.5, -3.0, None], [None, 0, 4, None],
              [None, [(5, -0.5), (8, -1.5)], [(8, -0.25), (4, -2.0)], None])
    res = srv._response(p, [5, 6, EOS, PAD], 4, None, prompt)
    plp = res["prompt_logprobs"]
    assert plp[0] is None and plp[3] is None and len(plp) == 4
    assert plp[1] == {"5": {"logprob": -0.5, "rank": 1, "decoded_token": "t5"}, "8": {"logprob": -1.5, "rank": 2, "decoded_token": "t8"}}
    assert list(plp[2]) == ["6", "8", "4"] and plp[2]["6"] == {"logprob": -3.0, "rank": 5, "decoded_token": "t6"}
    assert plp[2]["8"]["rank"] == 1 and plp[2]["4"]["rank"] == 2
    # without the field the response is what it always was
    plain = srv._response(srv._parse(dict(messages=msg, max_tokens=8)), [5, 6, EOS, PAD], 4)
    assert "prompt_logprobs" not in plain and list(plain) == ["id", "object", "created", "model", "choices", "usage"]
    res.pop("prompt_logprobs")
    assert {k: v for k, v in res.items() if k not in ("id", "created")} == {k: v for k, v in plain.items() if k not in ("id", "created")}


def test_new_symbols_are_in_the_header_and_the_loader():
    from zoomearth_amd import _lib

    with open(os.path.join(ROOT, "include", "zoomearth.h"), encoding="utf-8") as f:
        header = f.read()
    for name in ("ze_score_batch_detail", "ze_op_score_detail"):
        assert re.search(rf"^int\s+{name}\s*\(", header, flags=re.M) and name in _lib.EXPORTS
    assert len(_lib._SIGS["ze_score_batch_detail"][1]) == len(_lib._SIGS["ze_score_batch"][1]) + 5

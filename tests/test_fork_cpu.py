"""CPU: parallel sampling on the host side -- `ze_seq_fork` in the C ABI, `Request.n` and the scheduler's bookkeeping around the fork
(on a stub engine that speaks the Engine methods the scheduler calls), and the server's `n`.

The stub's "model": token i of a chain on stream s = 100 + (first prompt id + s + i) % 7, so completions of one prompt differ by
their stream alone and a completion that was handed the wrong stream or the wrong rows is seen at once."""
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from zoomearth_amd import serve
from zoomearth_amd.scheduler import ChainScheduler, Request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS, PAD, IMG = 3, 0, 7


# ---------------------------------------------------------------- the C ABI
def test_ze_seq_fork_is_declared_bound_and_exported():
    from zoomearth_amd import _lib
    with open(os.path.join(ROOT, "include", "zoomearth.h"), encoding="utf-8") as f:
        header = f.read()
    assert re.search(r"int ze_seq_fork\(ze_engine\* e, int src_seq, const int32_t\* dst_seqs, int n, void\* stream\);", header)
    assert "ze_seq_fork" in _lib.EXPORTS
    if os.path.exists(_lib.LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert re.search(r" T ze_seq_fork$", syms, re.M)


# ---------------------------------------------------------------- the stub
class StubEngine:
    def __init__(self, max_seqs=4, max_ctx=256, max_prefill_rows=256, max_patches=64):
        self.max_seqs, self.max_ctx, self.max_prefill_rows, self.max_patches = max_seqs, max_ctx, max_prefill_rows, max_patches
        self.chains, self.log, self.grammar_of = {}, [], {}

    def gen_params(self, **kw):
        return kw

    def rope_index(self, ids, grids):
        return np.zeros((3, len(ids)), np.int32), 0

    def vit_forward(self, pv, grids):
        return torch.zeros((sum(g[0] * g[1] * g[2] for g in grids) // 4, 8))

    def seq_reset(self, slot):
        self.chains[slot] = dict(ids=[], out=[], stream=None, fresh=False)

    def seq_len(self, slot):
        c = self.chains.get(slot)
        return 0 if c is None else len(c["ids"]) + max(len(c["out"]) - 1, 0)

    def seq_retire(self, slot, stream=None):
        pass

    def seq_copy_prefix(self, dst, src, n):
        assert n <= len(self.chains[src]["ids"]) and dst != src
        self.log.append(("copy", dst, src, n))
        self.chains[dst] = dict(ids=list(self.chains[src]["ids"][:n]), out=[], stream=None, fresh=False)

    def seq_fork(self, src, dsts):
        c = self.chains[src]
        assert c["fresh"] and not c["out"] and src not in dsts and len(set(dsts)) == len(dsts)
        self.log.append(("fork", src, list(dsts), len(c["ids"])))
        for d in dsts:
            self.chains[d] = dict(ids=list(c["ids"]), out=[], stream=None, fresh=True)

    def seq_truncate(self, slot, keep):
        c = self.chains[slot]
        self.log.append(("truncate", slot, keep))
        c["ids"], c["out"], c["fresh"] = (c["ids"] + c["out"][:-1])[:keep], [], False

    def prefill_batch(self, slots, ids_l, emb_l, pos_l, dl):
        self.log.append(("prefill", list(slots), [len(x) for x in ids_l]))
        for s, ids in zip(slots, ids_l):
            self.chains[s]["ids"] += list(ids)
            self.chains[s]["fresh"] = True

    def mark_seen(self, slot, ids):
        pass

    def set_sampling(self, slot, **kw):
        self.log.append(("sampling", slot))

    def set_sampling_filter(self, slot, *a):
        pass

    def grammar_create(self, automaton):
        return 0

    def grammar_destroy(self, gid):
        pass

    def set_grammar(self, slot, gid):
        self.grammar_of[slot] = gid
        self.log.append(("grammar", slot, gid))

    def _next(self, c):
        c["out"].append(100 + (c["ids"][0] + c["stream"] + len(c["out"])) % 7)
        c["fresh"] = False

    def chain_begin(self, slot, params, stream):
        c = self.chains[slot]
        assert c["fresh"], "a chain draws its first token from the logits a prefill or a fork left"
        c["stream"] = stream
        self.log.append(("begin", slot, stream))
        self._next(c)

    def decode_burst(self, slots, steps, params):
        assert len(set(slots)) == len(slots)
        for _ in range(steps):
            for s in slots:
                self._next(self.chains[s])
        return steps, [len(self.chains[s]["out"]) for s in slots], [False] * len(slots)

    def decode_burst_begin(self, slots, steps, params):
        self._burst = self.decode_burst(slots, steps, params)
        return self._burst[0]

    def decode_burst_end(self, slots):
        return self._burst[1], self._burst[2]

    def chain_tokens(self, slot, cap=0, stream=None):
        return self.chains[slot]["out"][: cap or None]


class Tok:
    def decode(self, ids, skip_special_tokens=True):
        return " ".join(str(i) for i in ids if not (skip_special_tokens and i in (PAD, EOS)))


class Proc:
    """text -> ids: one id per whitespace word (`<img>` expands to 4 image tokens per image)."""
    tokenizer = Tok()

    def __call__(self, text, images=None, return_tensors="pt", **kw):
        out, n = [], 0
        for w in text[0].split():
            if w == "<img>":
                out += [IMG] * 4
                n += 1
            else:
                out.append(int(w))
        d = dict(input_ids=torch.tensor([out]))
        if images:
            d.update(image_grid_thw=torch.tensor([[1, 4, 4]] * n), pixel_values=torch.zeros((16 * n, 3)),
                     image_keys=[("k", im) for im in images])
        return d


def make_model(**kw):
    cfg = SimpleNamespace(image_token_id=IMG, eos_token_ids=(EOS,), pad_token_id=PAD, vision=SimpleNamespace(spatial_merge_size=2),
                          text=SimpleNamespace(vocab_size=2048))
    return SimpleNamespace(engine=StubEngine(**kw), config=cfg, generation_config=SimpleNamespace(repetition_penalty=1.0, temperature=None),
                           _chains={}, device="cpu", compile_grammar=lambda **k: object())


def expected(first, stream, budget):
    return [100 + (first + stream + i) % 7 for i in range(budget)]


SAMPLED = dict(do_sample=True, temperature=0.8, seed=1)


# ---------------------------------------------------------------- Request.n
def test_n_is_validated_at_submit():
    sched = ChainScheduler(make_model(max_seqs=4), Proc(), overlap=False)
    assert Request(prompt="11 50", images=[]).n == 1 and Request(prompt="11 50", images=[]).index == 0
    for bad in (0, -1, 5, 2.0, "2", True, None):
        with pytest.raises(ValueError, match="`n` has to be an integer"):
            sched.submit(Request(prompt="11 50", images=[], n=bad, **SAMPLED))
    with pytest.raises(ValueError, match="need a sampled request"):
        sched.submit(Request(prompt="11 50", images=[], n=2))                       # greedy scheduler, greedy request
    with pytest.raises(ValueError, match="need a sampled request"):
        sched.submit(Request(prompt="11 50", images=[], n=2, do_sample=False, temperature=0.8))
    assert not sched.waiting
    sched.submit(Request(prompt="11 50", images=[], n=4, **SAMPLED))
    sampling = ChainScheduler(make_model(max_seqs=4), Proc(), overlap=False, do_sample=True, temperature=0.7)
    sampling.submit(Request(prompt="11 50", images=[], n=2))                        # the scheduler's own mode counts
    # `n` is no field a request carries into its decode steps
    import dataclasses
    assert "n" not in {f.name for f in dataclasses.fields(Request)}


# ---------------------------------------------------------------- bookkeeping
@pytest.mark.parametrize("overlap", [False, True])
def test_siblings_get_their_streams_indices_and_one_callback_each(overlap):
    model = make_model(max_seqs=6)
    e = model.engine
    sched = ChainScheduler(model, Proc(), burst=3, overlap=overlap)
    done = []
    parent = Request(prompt="21 <img> 50", images=["view"], max_new_tokens=5, stream_id=40, n=4, tag="t",
                     on_done=lambda r, toks, text: done.append((r.index, r.stream_id, list(toks), r.parent, r.tag, r.n_prompt)), **SAMPLED)
    other = Request(prompt="33 50 51", images=[], max_new_tokens=4, on_done=lambda r, toks, text: done.append(("other", list(toks))))
    sched.submit(parent)
    sched.submit(other)
    sched.run()
    assert ("other", expected(33, 0, 4)) in done
    mine = sorted(d for d in done if d[0] != "other")
    assert [(d[0], d[1]) for d in mine] == [(0, 40), (1, 41), (2, 42), (3, 43)]
    assert all(d[2] == expected(21, 40 + d[0], 5) and d[3] is parent and d[4] == "t" and d[5] == 6 for d in mine)
    forks = [x for x in e.log if x[0] == "fork"]
    assert len(forks) == 1 and len(forks[0][2]) == 3 and forks[0][3] == 6
    assert [x for x in e.log if x[0] == "prefill"][0][2][0] == 6 and not [x for x in e.log if x[0] == "copy"]   # one whole prefill, no tails
    begun = {x[1]: x[2] for x in e.log if x[0] == "begin"}
    assert sorted(begun[s] for s in [forks[0][1]] + forks[0][2]) == [40, 41, 42, 43]
    assert sched.stats["forked_chains"] == 3 and sched.stats["forked_rows"] == 18 and sched.stats["admitted"] == 5
    assert not sched.live and sorted(sched.free) == list(range(6)) and not sched.busy()


def test_a_follow_up_from_a_sibling_keeps_its_slot():
    model = make_model(max_seqs=4)
    e = model.engine
    sched = ChainScheduler(model, Proc(), burst=2, overlap=False)
    out = {}

    def stage1(r, toks, text):
        if r.index != 2:
            out[r.index] = (r.slot, list(toks))
            return None
        return Request(prompt="23 50 51 " + " ".join(str(t) for t in toks[:-1]) + " 60", images=[], max_new_tokens=3, stream_id=9,
                       on_done=lambda r2, t2, x2: out.__setitem__("stage2", (r2.slot, list(t2), r.slot)), **SAMPLED)
    sched.submit(Request(prompt="23 50 51", images=[], max_new_tokens=4, n=3, on_done=stage1, **SAMPLED))
    sched.run()
    slot2, toks2, slot1 = out["stage2"]
    assert slot2 == slot1 and toks2 == expected(23, 9, 3)
    assert ("truncate", slot1, 6) in e.log                                       # the sibling's forked rows are the follow-up's prefix
    assert out[0][1] == expected(23, 0, 4) and out[1][1] == expected(23, 1, 4)
    assert sorted(sched.free) == list(range(4))


def test_overflow_siblings_become_ordinary_requests():
    model = make_model(max_seqs=2)
    e = model.engine
    sched = ChainScheduler(model, Proc(), burst=2, overlap=False)
    done = {}
    parent = Request(prompt="25 <img> 50", images=["v"], max_new_tokens=4, stream_id=10, n=5,
                     on_done=lambda r, toks, text: done.__setitem__(r.index, (r.stream_id, list(toks))), **SAMPLED)
    with pytest.raises(ValueError):
        sched.submit(parent)                                                     # more completions than the engine has slots
    model = make_model(max_seqs=6)
    e = model.engine
    sched = ChainScheduler(model, Proc(), burst=2, overlap=False, max_batch=2)
    sched.submit(parent)
    sched.run()
    assert done == {i: (10 + i, expected(25, 10 + i, 4)) for i in range(5)}
    forks = [x for x in e.log if x[0] == "fork"]
    assert len(forks) == 1 and len(forks[0][2]) == 1                             # one sibling had a slot; three came in later
    assert sched.stats["forked_chains"] == 1 and sched.stats["admitted"] == 5
    assert sorted(sched.free) == [0, 1] and not sched.busy()


def test_a_siblings_slot_is_nobodys_between_planning_and_fork():
    """The shape of the chunked-admission hazard: a donor finishes between two chunks while an anchor's item is carried, its slot
    returns to `free` (LIFO) and the next chunk's first request pops it.  The siblings' slots were taken out of `free` when the
    anchor was planned, so whatever is admitted in between gets another slot, and every completion comes out as it would alone."""
    model = make_model(max_seqs=8, max_prefill_rows=64)
    e = model.engine
    sched = ChainScheduler(model, Proc(), burst=1, overlap=True, admit_chunk_rows=1)
    done = {}

    def rec(name):
        return lambda r, toks, text: done.__setitem__((name, r.index), (r.stream_id, list(toks)))
    donor = Request(prompt="31 <img> 50", images=["tile0"], max_new_tokens=5, on_done=rec("donor"))
    sched.submit(donor)
    sched.step()
    sched.step()
    assert sched.live                                                            # the donor decodes; it finishes within the next steps
    sched.submit(Request(prompt="41 <img> 50", images=["tile1"], max_new_tokens=4, stream_id=5, n=3, on_done=rec("fork"), **SAMPLED))
    for q in range(4):
        sched.submit(Request(prompt=f"{51 + q} <img> 50", images=[f"tile{2 + q}"], max_new_tokens=3, on_done=rec(f"q{q}")))
    pinned_seen = False
    for _ in range(200):
        if not sched.busy():
            break
        sched.step()
        pending = [k.slot for g in list(sched._groups) + [sched._carry] for it in g for k in (getattr(it["req"], "_forks", None) or [])]
        if pending:
            pinned_seen = True
            taken = [it["req"].slot for g in list(sched._groups) + [sched._carry] for it in g] + list(sched.live) + \
                    [r.slot for r, _, _ in sched._ready]
            assert not set(pending) & set(sched.free) and not set(pending) & set(taken) and len(set(pending)) == len(pending)
    assert not sched.busy()
    assert {k: v for k, v in done.items() if k[0] == "fork"} == {("fork", i): (5 + i, expected(41, 5 + i, 4)) for i in range(3)}
    for q in range(4):
        assert done[(f"q{q}", 0)] == (0, expected(51 + q, 0, 3))
    assert done[("donor", 0)] == (0, expected(31, 0, 5))
    assert pinned_seen and sorted(sched.free) == list(range(8)) and sched.stats["forked_chains"] == 2


def test_grammar_users_balance_over_the_siblings():
    model = make_model(max_seqs=4)
    sched = ChainScheduler(model, Proc(), burst=2, overlap=False)
    sched.submit(Request(prompt="27 50", images=[], max_new_tokens=3, n=3, guided_choice=["a", "b"], **SAMPLED))
    sched.run()
    calls = [x for x in model.engine.log if x[0] == "grammar"]
    assert len([x for x in calls if x[2] is not None]) == 3 and len({x[1] for x in calls}) == 3   # acquired once per sibling ...
    assert sum(sched.grammars.users.values()) == 0                                               # ... and all given back
    assert all(v is None for v in model.engine.grammar_of.values())


def test_a_failing_anchor_fails_every_completion_once():
    model = make_model(max_seqs=4)
    sched = ChainScheduler(model, Proc(), burst=2, overlap=False)
    errors = []
    sched.submit(Request(prompt="29 <img> 50", images=[], max_new_tokens=3, n=3, on_error=lambda r, ex: errors.append(r.index), **SAMPLED))
    sched.run()                                                                  # an image token without an image: the request is malformed
    assert sorted(errors) == [0, 1, 2] and sorted(sched.free) == list(range(4)) and not sched.busy()
    e = model.engine
    e.seq_fork = lambda src, dsts: (_ for _ in ()).throw(RuntimeError("no fork"))
    got = {}
    sched.submit(Request(prompt="29 50", images=[], max_new_tokens=3, n=3, on_error=lambda r, ex: errors.append(("fork", r.index)),
                         on_done=lambda r, toks, text: got.__setitem__(r.index, list(toks)), **SAMPLED))
    sched.run()
    assert sorted(x for x in errors if isinstance(x, tuple)) == [("fork", 1), ("fork", 2)] and got == {0: expected(29, 0, 3)}
    assert sorted(sched.free) == list(range(4))


# ---------------------------------------------------------------- the server
def test_server_parses_n():
    srv = serve.ChatServer(make_model(max_seqs=16), Proc(), "stub")
    msg = [{"role": "user", "content": "5 6"}]
    assert srv._parse(dict(messages=msg)).n == 1 and srv._parse(dict(messages=msg, n=1)).n == 1
    assert srv._parse(dict(messages=msg, n=None)).n == 1
    assert srv._parse(dict(messages=msg, n=3, temperature=0.7)).n == 3
    assert srv._parse(dict(messages=msg, n=16, temperature=0.7)).n == 16
    for bad, text in ((0, r"n must be in \[1, 16\], got 0"), (17, r"n must be in \[1, 16\], got 17"), (-2, "n must be in"),
                      ("2", "n must be an integer, got '2'"), (2.0, "n must be an integer"), (True, "n must be an integer")):
        with pytest.raises(serve.BadRequest, match=text):
            srv._parse(dict(messages=msg, n=bad, temperature=0.7))
    for t in (None, 0, 0.0):
        with pytest.raises(serve.BadRequest, match="n = 2 needs temperature > 0"):
            srv._parse(dict(messages=msg, n=2, temperature=t))
    with pytest.raises(serve.BadRequest, match="n = 5 exceeds the engine's 4 chain slots"):
        serve.ChatServer(make_model(max_seqs=4), Proc(), "stub")._parse(dict(messages=msg, n=5, temperature=0.7))
    with pytest.raises(serve.BadRequest, match="n > 1 go through submit"):
        srv.complete_many([dict(messages=msg, n=2, temperature=0.7)])
    assert "n must be 1" not in open(serve.__file__, encoding="utf-8").read()


def test_server_merges_the_choices():
    srv = serve.ChatServer(make_model(max_seqs=4), Proc(), "stub")
    p = srv._parse(dict(messages=[{"role": "user", "content": "5 6"}], n=3, temperature=0.7, max_tokens=8))
    parts = [srv._response(p, out, 4) for out in ([5, 6, EOS, PAD], [9, 9, 9, 9, 9, 9, 9, 9], [EOS])]
    res = srv._merge_choices(parts, 4)
    assert [c["index"] for c in res["choices"]] == [0, 1, 2]
    assert [c["finish_reason"] for c in res["choices"]] == ["stop", "length", "stop"]
    assert res["usage"] == {"prompt_tokens": 4, "completion_tokens": 3 + 8 + 1, "total_tokens": 4 + 12}

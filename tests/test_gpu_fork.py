"""GPU: the fork of a prefilled chain (ze_seq_fork, zoomearth_amd/csrc/ze_fork.hip) and the parallel sampling built on it
(`Request.n`, `generate(num_return_sequences=)`, the server's `n`).

Everything here is an equality: a fork copies bits, and a forked chain's tokens and log-probabilities are BIT FOR BIT those of a
chain that prefilled the whole prompt itself with the same marks, requests and stream (the contract in include/zoomearth.h) -- so
rows are compared with torch.equal, tokens and log-probabilities with ==.  No tolerance appears anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_util import CHAIN_W
from oracle import prng
from zoomearth_amd._lib import ZoomEarthError

pytestmark = pytest.mark.gpu

CTX = 512
N_TOK = 24
BURSTS = (8, 5, 10)            # 1 + 23 tokens; the source of test 3 leaves behind the first burst (8 steps)


def make_engine(slots):
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.engine import Engine
    e = Engine(ModelConfig.tiny(), device=0, max_seqs=slots, max_ctx=CTX, max_patches=1024, max_tile_side=1024)
    e.fill_synthetic(**CHAIN_W)
    return e


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(slots):
        if slots not in made:
            made[slots] = make_engine(slots)
        return made[slots]
    yield get
    for e in made.values():
        e.close()


def text_ids(seed, n):
    return prng.uniform_ints(seed, n, 10, 1990).tolist()


def prefill_text(e, seq, ids):
    pos, delta = e.rope_index(ids, [])
    e.seq_reset(seq)
    e.prefill(seq, ids, None, pos, delta, want_logits=False)


def kv_rows(e, seq, start, n):
    return [torch.cat(e.op_kv_read(seq, layer, start, n)).clone() for layer in range(e.config.text.num_hidden_layers)]


# ---------------------------------------------------------------- 1. rows
def second_trip_rows(cfg):
    """A row count whose 16-byte pieces per (layer, kv head, K|V) run exceed gridDim.x * 256 of the fork's launch (ze_kv_fork_blocks:
    min(16, 2048 / (runs + 2)) blocks per run), by a ragged part of a trip"""
    t = cfg.text
    per_row = (t.hidden_size // t.num_attention_heads) * 2 // 16
    blocks = min(16, 2048 // (t.num_hidden_layers * t.num_key_value_heads * 2 + 2))
    return blocks * 256 // per_row + 37


SLOTS = 20
PLACES = {1: (19, [0]), 3: (0, [19, 5, 11]), 16: (7, [0, 19] + [s for s in range(1, 19) if s != 7][:14])}


@pytest.mark.parametrize("n", [1, 3, 16])
@pytest.mark.parametrize("rows", [1, 7, 129, "second trip"])
def test_fork_copies_exactly_the_sources_rows(engines, rows, n):
    e = engines(SLOTS)
    L = second_trip_rows(e.config) if rows == "second trip" else rows
    assert L + 40 <= CTX and (rows != "second trip" or L * 16 > 16 * 256)
    src, dsts = PLACES[n]
    assert len(dsts) == n and len(set(dsts + [src])) == n + 1
    prefill_text(e, dsts[0], text_ids(900 + n, L + 40))          # a longer other chain: its rows beyond L must survive
    before = kv_rows(e, dsts[0], 0, L + 40)
    prefill_text(e, src, text_ids(700 + L, L))
    want = kv_rows(e, src, 0, L)
    e.seq_fork(src, dsts)
    for d in dsts:
        assert e.seq_len(d) == L
        got = kv_rows(e, d, 0, L)
        assert all(torch.equal(g, w) for g, w in zip(got, want)), (L, n, d)
    after = kv_rows(e, dsts[0], L, 40)
    assert all(torch.equal(a, b[:, L:]) for a, b in zip(after, before))
    assert not all(torch.equal(w, b[:, :L]) for w, b in zip(want, before))       # (the copy had something to change)
    assert all(torch.equal(g, w) for g, w in zip(kv_rows(e, src, 0, L), want))   # the source is untouched
    for s in dsts + [src]:
        e.seq_reset(s)


# ---------------------------------------------------------------- 2 / 3. chains
def image_prompt(e):
    """ids / grids / feature rows of a prompt with one image block in the middle: rope delta and split row are non-zero"""
    c = e.config
    grid = [1, 4, 6]                                              # 24 patches -> 6 image tokens
    ids = text_ids(31, 9) + [c.vision_start_token_id] + [c.image_token_id] * 6 + [c.vision_end_token_id] + text_ids(32, 13)
    g = torch.Generator().manual_seed(5)
    emb = (torch.randn((6, c.text.hidden_size), generator=g) * 0.5).to(torch.bfloat16).cuda()
    pos, delta = e.rope_index(ids, [grid])
    assert delta != 0
    return ids, emb, pos, delta


REQUESTS = [dict(seed=11 + i, temperature=0.7 + 0.1 * i, top_k=40 + 10 * i, stream=3 + 2 * i) for i in range(3)]
OTHERS = [text_ids(61, 17), text_ids(62, 40)]


def install(e, slot, rq):
    e.set_sampling(slot, do_sample=True, temperature=rq["temperature"], seed=rq["seed"], repetition_penalty=1.3)
    e.set_sampling_filter(slot, top_k=rq["top_k"])
    e.set_logprobs(slot, 5)


def result_of(e, slot):
    lp, ids, tlp = e.chain_logprobs(slot, N_TOK)
    return e.chain_tokens(slot, N_TOK), lp.tobytes(), ids.tobytes(), tlp.tobytes()


_ALONE = {}


def alone(e, key):
    """the three requests, each on a chain that prefilled the whole prompt itself and decoded alone: made once per engine"""
    if key not in _ALONE:
        ids, emb, pos, delta = image_prompt(e)
        params = e.gen_params(repetition_penalty=1.0, ignore_eos=True, do_sample=False)
        out = []
        for rq in REQUESTS:
            e.seq_reset(1)
            e.prefill(1, ids, emb, pos, delta, want_logits=False)
            e.mark_seen(1, ids)
            install(e, 1, rq)
            e.chain_begin(1, params, rq["stream"])
            for steps in BURSTS:
                e.decode_burst([1], steps, params)
            out.append(result_of(e, 1))
        e.seq_reset(1)
        assert all(len(o[0]) == N_TOK for o in out) and len({tuple(o[0]) for o in out}) == 3
        _ALONE[key] = out
    return _ALONE[key]


def forked_run(e, retire_source):
    ids, emb, pos, delta = image_prompt(e)
    last = e.max_seqs - 1
    src, sibs, others = 2, [0, last, 5], [3, 7]
    params = e.gen_params(repetition_penalty=1.0, ignore_eos=True, do_sample=False)
    e.seq_reset(src)
    e.prefill(src, ids, emb, pos, delta, want_logits=False)
    e.mark_seen(src, ids)                                        # the marks travel with the fork
    e.seq_fork(src, sibs)
    assert [e.seq_len(s) for s in sibs] == [len(ids)] * 3
    assert [e.seq_prefix_hint(s) for s in sibs] == [(src, len(ids))] * 3       # one copy of the prompt is streamed for all
    for s, rq in zip(sibs, REQUESTS):
        install(e, s, rq)
    e.set_sampling(src, do_sample=True, temperature=0.9, seed=77, repetition_penalty=1.1)
    for s, p in zip(others, OTHERS):
        prefill_text(e, s, p)
    for s, rq in zip(sibs, REQUESTS):
        e.chain_begin(s, params, rq["stream"])
    for s in [src] + others:
        e.chain_begin(s, params, 0)
    live = [others[0], sibs[0], src, sibs[1], others[1], sibs[2]]
    for k, steps in enumerate(BURSTS):
        e.decode_burst(live, steps, params)
        if k == 0 and retire_source:
            e.seq_retire(src)                                    # the readers move to a sibling's copy ...
            assert all(e.seq_prefix_hint(s)[0] != src for s in sibs)
            prefill_text(e, src, text_ids(63, 50))               # ... and the slot goes to an unrelated prompt
            e.chain_begin(src, params, 9)
    got = [result_of(e, s) for s in sibs]
    for s in live:
        e.seq_reset(s)
    return got


@pytest.mark.parametrize("slots", [SLOTS, 72], ids=["fragment family", "row-streaming family"])
@pytest.mark.parametrize("retire_source", [False, True], ids=["source alive", "source retired"])
def test_forked_chains_equal_chains_that_prefilled_alone(engines, slots, retire_source):
    e = engines(slots)
    assert (e.max_seqs > 64) == (slots == 72)
    want = alone(e, slots)
    got = forked_run(e, retire_source)
    for i in range(3):
        assert got[i][0] == want[i][0], f"tokens of sibling {i}"
        assert got[i][1:] == want[i][1:], f"log-probabilities of sibling {i}"


# ---------------------------------------------------------------- 4. errors
def test_a_refused_fork_changes_nothing(engines):
    e = engines(SLOTS)
    lib, h, st = e.lib, e.h, e._stream()
    prefill_text(e, 4, text_ids(71, 12))
    prefill_text(e, 5, text_ids(72, 30))
    prefill_text(e, 6, text_ids(73, 21))
    e.seq_reset(9)
    dsts = [5, 6]

    def snapshot():
        return ([e.seq_len(s) for s in dsts], [lib.ze_seq_prefix_hint(h, s) for s in dsts], [kv_rows(e, s, 0, 30) for s in dsts])

    def same(a, b):
        return a[0] == b[0] and a[1] == b[1] and all(torch.equal(x, y) for p, q in zip(a[2], b[2]) for x, y in zip(p, q))

    def fork(src, table, n=None):
        if table is None:
            return lib.ze_seq_fork(h, src, None, 1 if n is None else n, st)
        arr = np.asarray(table, dtype=np.int32)
        return lib.ze_seq_fork(h, src, arr.ctypes.data_as(C.POINTER(C.c_int32)), len(table) if n is None else n, st)

    before = snapshot()
    INVALID, NOTFOUND = -1, -4
    assert fork(4, None) == INVALID                              # null table
    assert fork(4, [5, 6], n=0) == INVALID and fork(4, [5, 6], n=-1) == INVALID
    assert fork(4, [5, SLOTS]) == NOTFOUND and fork(4, [-1, 6]) == NOTFOUND and fork(SLOTS, [5, 6]) == NOTFOUND
    assert fork(4, [5, 4]) == INVALID                            # a destination equal to the source
    assert fork(4, [5, 6, 5]) == INVALID                         # a destination named twice
    assert fork(9, [5, 6]) == INVALID                            # an empty source
    torch.cuda.synchronize()
    assert same(before, snapshot())
    # a source that is no longer what its prefill left: it drew, it stepped, it was truncated, it was copied into
    params = e.gen_params(repetition_penalty=1.0, ignore_eos=True, do_sample=False)
    e.chain_begin(4, params, 0)
    assert fork(4, [5, 6]) == INVALID
    with pytest.raises(ZoomEarthError):
        e.seq_fork(4, [5, 6])
    prefill_text(e, 4, text_ids(71, 12))
    e.decode_batch([4], [17])
    assert fork(4, [5, 6]) == INVALID
    prefill_text(e, 4, text_ids(71, 12))
    e.seq_truncate(4, 8)
    assert fork(4, [5, 6]) == INVALID
    e.seq_copy_prefix(4, 5, 6)
    assert fork(4, [5, 6]) == INVALID
    torch.cuda.synchronize()
    assert same(before, snapshot())
    prefill_text(e, 4, text_ids(71, 12))                         # and what is refused above is accepted from a fresh prefill
    assert fork(4, [5, 6]) == 0 and [e.seq_len(s) for s in dsts] == [12, 12]
    for s in (4, 5, 6):
        e.seq_reset(s)


# ---------------------------------------------------------------- 5. public faces
@pytest.fixture(scope="module")
def stack():
    from tiny_tok import make_tokenizer
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.modeling import ZoomEarthForConditionalGeneration
    from zoomearth_amd.processor import ZoomEarthProcessor
    model = ZoomEarthForConditionalGeneration.from_synthetic(ModelConfig.tiny(), **CHAIN_W, max_seqs=6, max_ctx=1024,
                                                            max_patches=1024, max_tile_side=1024)
    proc = ZoomEarthProcessor(make_tokenizer(), min_pixels=3136, max_pixels=128 * 128 * 28 * 28)
    proc.tokenizer.padding_side = "left"
    yield model, proc
    model.engine.close()


def words(seed, n):
    return " ".join(f"w{int(v)}" for v in prng.uniform_ints(seed, n, 10, 1990))


def test_generate_returns_k_sequences_per_row(stack):
    model, proc = stack
    inp = proc(text=[words(81, 12), words(82, 7)], return_tensors="pt", padding="longest").to(model.device)
    kw = dict(max_new_tokens=10, do_sample=True, temperature=0.9, seed=4, repetition_penalty=1.2, ignore_eos=True)
    got = model.generate(**inp, num_return_sequences=3, logprobs=2, **kw)
    # today's way to the same chains: every row three times in the batch (streams 0 .. 5, batch-major)
    rep = {k: v.repeat_interleave(3, 0) for k, v in inp.items() if isinstance(v, torch.Tensor)}
    want = model.generate(**rep, logprobs=2, **kw)
    assert got.sequences.shape[0] == 6 and torch.equal(got.sequences, want.sequences)
    assert torch.equal(got.logprobs, want.logprobs) and torch.equal(got.top_ids, want.top_ids) and torch.equal(got.top_logprobs, want.top_logprobs)
    new = got.sequences[:, inp["input_ids"].shape[1]:].tolist()
    assert len({tuple(r) for r in new}) == 6
    # one row: three single chains on streams 0 .. 2
    one = proc(text=[words(81, 12)], return_tensors="pt").to(model.device)
    three = model.generate(**one, num_return_sequences=3, **kw)
    assert three[:, one["input_ids"].shape[1]:].tolist() == new[:3]
    assert torch.equal(model.generate(**one, num_return_sequences=1, **kw), model.generate(**one, **kw))
    with pytest.raises(ValueError):
        model.generate(**one, max_new_tokens=4, num_return_sequences=3)
    with pytest.raises(ValueError):
        model.generate(**one, max_new_tokens=4, do_sample=True, num_return_sequences=0)


def run_sched(model, proc, reqs, **kw):
    from zoomearth_amd.scheduler import ChainScheduler
    sched = ChainScheduler(model, proc, do_sample=False, burst=4, **kw)
    for r in reqs:
        sched.submit(r)
    sched.run()
    return sched


def test_one_request_of_n_equals_n_requests(stack):
    from zoomearth_amd.scheduler import Request
    model, proc = stack
    own = dict(prompt=words(83, 15), images=[], max_new_tokens=12, do_sample=True, temperature=0.9, seed=6, repetition_penalty=1.2,
               top_k=50, logprobs=2)
    singles = [Request(stream_id=20 + i, **own) for i in range(4)]
    run_sched(model, proc, singles)
    want = [(list(r.tokens), list(r.token_logprobs), list(r.top_logprobs)) for r in singles]
    assert len({tuple(w[0]) for w in want}) == 4
    for max_batch, forked in ((None, 3), (2, 1)):                # all siblings fit / two of them overflow into ordinary requests
        done = {}
        req = Request(stream_id=20, n=4, on_done=lambda r, t, x: done.__setitem__(r.index, r), **own)
        sched = run_sched(model, proc, [req], max_batch=max_batch)
        assert sorted(done) == [0, 1, 2, 3] and all(r.parent is req for r in done.values())
        assert [(list(done[i].tokens), list(done[i].token_logprobs), list(done[i].top_logprobs)) for i in range(4)] == want
        assert sched.stats["forked_chains"] == forked and sched.stats["forked_rows"] == forked * done[0].n_prompt
        assert sched.stats["admitted"] == 4 and sorted(sched.free) == list(range(sched.max_batch))


def test_server_returns_n_indexed_choices(stack):
    from fastapi.testclient import TestClient
    from zoomearth_amd import serve
    from zoomearth_amd.scheduler import Request
    model, proc = stack
    client = TestClient(serve.create_app(serve.ChatServer(model, proc, "ZoomEarth")))
    msgs = [{"role": "user", "content": words(84, 12)}]
    body = {"model": "ZoomEarth", "messages": msgs, "max_tokens": 10, "temperature": 0.9, "seed": 8, "logprobs": True, "top_logprobs": 2}
    r = client.post("/v1/chat/completions", json={**body, "n": 3})
    assert r.status_code == 200
    res = r.json()
    assert [c["index"] for c in res["choices"]] == [0, 1, 2]
    one = client.post("/v1/chat/completions", json=body).json()
    assert res["choices"][0] == one["choices"][0]
    # choice i = the request alone on stream i of the same seed
    prompt = serve.build_prompt(msgs)[0]
    lone = [Request(prompt=prompt, images=[], max_new_tokens=10, do_sample=True, temperature=0.9, seed=8, stream_id=i, top_k=0, top_p=1.0,
                    min_p=0.0, logprobs=2) for i in range(3)]
    run_sched(model, proc, lone)
    for c, l in zip(res["choices"], lone):
        assert c["message"]["content"] == proc.tokenizer.decode(list(l.tokens), skip_special_tokens=True).strip()
        assert [x["logprob"] for x in c["logprobs"]["content"]] == [float(v) for v in l.token_logprobs][:len(c["logprobs"]["content"])]
    assert len({c["message"]["content"] for c in res["choices"]}) == 3
    done = sum(len(c["logprobs"]["content"]) for c in res["choices"])
    assert res["usage"] == {"prompt_tokens": one["usage"]["prompt_tokens"], "completion_tokens": done,
                            "total_tokens": one["usage"]["prompt_tokens"] + done}
    for bad in ({"n": 2, "temperature": 0}, {"n": 2, "temperature": None}, {"n": 0}, {"n": 17}, {"n": "2"}):
        r = client.post("/v1/chat/completions", json={**body, **bad})
        assert r.status_code == 400, bad

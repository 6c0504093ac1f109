"""GPU: the prefix cache -- the engine's pool of K/V blocks (ze_prefix_*, zoomearth_amd/csrc/ze_prefix.hip), its host side
(zoomearth_amd/prefix_cache.py) and the scheduler / server paths built on them.

Everything here is an equality, as for ze_seq_copy_prefix and ze_seq_fork: a save and a load copy bits, and a chain that loads a cached
prefix and prefills its tail is compared with a chain that prefilled the whole prompt itself -- rows with torch.equal, tokens and
log-probabilities with ==.  No tolerance appears anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_util import CHAIN_W
from oracle import prng

pytestmark = pytest.mark.gpu

CTX, SLOTS, BR, POOL = 512, 6, 16, 8
A, B_, C_, D, E = 0, 1, 2, 3, 4
INVALID, NOMEM, NOTFOUND = -1, -3, -4


@pytest.fixture(scope="module")
def eng():
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.engine import Engine
    e = Engine(ModelConfig.tiny(), device=0, max_seqs=SLOTS, max_ctx=CTX, max_patches=1024, max_tile_side=1024)
    e.fill_synthetic(**CHAIN_W)
    yield e
    e.close()


def fresh_pool(e, n_blocks=POOL, block_rows=BR):
    e.prefix_pool_destroy()
    e.prefix_pool_create(n_blocks, block_rows)


def text_ids(seed, n):
    return prng.uniform_ints(seed, n, 10, 1990).tolist()


def prefill_text(e, seq, ids):
    pos, delta = e.rope_index(ids, [])
    e.seq_reset(seq)
    e.prefill(seq, ids, None, pos, delta, want_logits=False)


def kv_rows(e, seq, start, n):
    return [torch.cat(e.op_kv_read(seq, layer, start, n)).clone() for layer in range(e.config.text.num_hidden_layers)]


def i32(a):
    a = np.asarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


def raw_save(e, seq, row0, blocks, n=None):
    a, p = i32(blocks)
    return e.lib.ze_prefix_save(e.h, seq, row0, p, len(a) if n is None else n, e._stream())


def raw_load(e, blocks, n_rows, split, dsts, n_blocks=None, n=None):
    a, p = i32(blocks)
    d, dp = i32(dsts)
    return e.lib.ze_prefix_load(e.h, p, len(a) if n_blocks is None else n_blocks, n_rows, split, dp, len(d) if n is None else n, e._stream())


# ---------------------------------------------------------------- 1. round trip
def test_round_trip_is_bit_for_bit_and_touches_nothing_else(eng):
    e = eng
    fresh_pool(e)
    assert e.prefix_pool_info()[:2] == (POOL, BR)
    for s in (B_, C_, D, E):                                     # prior chains: their rows from 59 on are the sentinel
        prefill_text(e, s, text_ids(900 + s, 90))
    before = {s: kv_rows(e, s, 0, 90) for s in (B_, C_, D, E)}
    prefill_text(e, A, text_ids(700, 70))
    want = kv_rows(e, A, 0, 59)
    e.prefix_save(A, 0, [5, 2, 7, 0])                            # rows 0 .. 63: ids neither sorted nor contiguous
    e.prefix_load([5, 2, 7, 0], 59, 0, [B_])                     # ends inside the last block
    e.prefix_load([5, 2, 7, 0], 59, 0, [C_, D, E])
    for s in (B_, C_, D, E):
        assert e.seq_len(s) == 59
        assert all(torch.equal(g, w) for g, w in zip(kv_rows(e, s, 0, 59), want)), s
        assert all(torch.equal(a, b[:, 59:]) for a, b in zip(kv_rows(e, s, 59, 31), before[s])), s
        assert not all(torch.equal(w, b[:, :59]) for w, b in zip(want, before[s]))       # (the load had something to change)
    assert e.seq_prefix_hint(D) == (C_, 59) and e.seq_prefix_hint(E) == (C_, 59)
    assert e.seq_prefix_hint(B_) == (B_, 0) and e.seq_prefix_hint(C_) == (C_, 0)
    assert all(torch.equal(g, w) for g, w in zip(kv_rows(e, A, 0, 59), want)) and e.seq_len(A) == 70
    # a second save from another row, into other blocks; the two chains' blocks chained in one load
    e.prefix_save(A, 48, [1])
    e.prefix_load([5, 2, 7, 1], 64, 0, [B_])
    assert all(torch.equal(g, w) for g, w in zip(kv_rows(e, B_, 0, 64), kv_rows(e, A, 0, 64)))
    e.seq_retire(C_)                                             # the readers move as for ze_seq_copy_prefix
    assert {e.seq_prefix_hint(D)[0], e.seq_prefix_hint(E)[0]} <= {D, E}
    for s in range(5):
        e.seq_reset(s)


# ---------------------------------------------------------------- 2. the contract
N_TOK = 12


def image_prompt(e):
    """5 text ids, one image block of 6 tokens (rows 5 .. 12, split row 13), 25 text ids: 38 rows, two full blocks"""
    c = e.config
    grid = [1, 4, 6]
    ids = text_ids(31, 5) + [c.vision_start_token_id] + [c.image_token_id] * 6 + [c.vision_end_token_id] + text_ids(32, 25)
    g = torch.Generator().manual_seed(5)
    emb = (torch.randn((6, c.text.hidden_size), generator=g) * 0.5).to(torch.bfloat16).cuda()
    pos, delta = e.rope_index(ids, [grid])
    assert delta != 0
    return ids, emb, pos, delta, 32, 13


def text_prompt(e):
    ids = text_ids(41, 70)
    pos, delta = e.rope_index(ids, [])
    return ids, None, pos, delta, 59, 0


def decode(e, slot, params):
    e.set_logprobs(slot, 5)
    e.chain_begin(slot, params, 0)
    e.decode_burst([slot], 8, params)
    e.decode_burst([slot], N_TOK - 1 - 8, params)
    lp, ids, tlp = e.chain_logprobs(slot, N_TOK)
    return e.chain_tokens(slot, N_TOK), lp.tobytes(), ids.tobytes(), tlp.tobytes()


@pytest.mark.parametrize("regime", [0, 1], ids=["fragment family", "row-streaming family"])
@pytest.mark.parametrize("prompt", [text_prompt, image_prompt], ids=["text", "image block inside the prefix"])
def test_a_chain_on_a_cached_prefix_equals_a_chain_that_prefilled_everything(eng, prompt, regime):
    e = eng
    assert e.set_decode_regime(regime) == regime
    fresh_pool(e)
    ids, emb, pos, delta, n_rows, split = prompt(e)
    params = e.gen_params(repetition_penalty=1.0, ignore_eos=True, do_sample=False)
    e.seq_reset(1)
    e.prefill(1, ids, emb, pos, delta, want_logits=False)        # the yardstick: the whole prompt, prefilled by the chain itself
    want_rows = kv_rows(e, 1, 0, len(ids))
    want = decode(e, 1, params)
    assert len(want[0]) == N_TOK
    # the holder: prefills, is saved, is reset, and its slot goes to an unrelated chain
    e.seq_reset(2)
    e.prefill(2, ids, emb, pos, delta, want_logits=False)
    blocks = [6, 1, 4, 3][:(n_rows + BR - 1) // BR]
    e.prefix_save(2, 0, blocks)
    prefill_text(e, 2, text_ids(63, 100))
    e.chain_begin(2, params, 9)
    # the chain under test: the pool's rows, then only the tail
    prefill_text(e, 3, text_ids(64, 80))                         # (what the slot held before)
    e.prefix_load(blocks, n_rows, split, [3])
    assert e.seq_len(3) == n_rows
    e.prefill(3, ids[n_rows:], None, pos[:, n_rows:], delta, want_logits=False)
    assert e.seq_len(3) == len(ids)
    assert all(torch.equal(g, w) for g, w in zip(kv_rows(e, 3, 0, len(ids)), want_rows))
    e.decode_burst([2], 3, params)                               # (the unrelated chain runs on)
    got = decode(e, 3, params)
    assert got[0][0] == want[0][0], "first token"
    assert got[0] == want[0], "tokens"
    assert got[1:] == want[1:], "log-probabilities"
    for s in (1, 2, 3):
        e.seq_reset(s)
    e.set_decode_regime(-1)


# ---------------------------------------------------------------- 4. staleness
def test_a_weight_change_makes_every_block_unsaved(eng):
    from zoomearth_amd.prefix_cache import PrefixCache
    e = eng
    e.prefix_pool_destroy()
    cache = PrefixCache(e, POOL * BR, BR)
    try:
        ids = text_ids(51, 50)
        prefill_text(e, A, ids)
        assert cache.save(A, ids, (), len(ids)) == 48
        m = cache.match(ids + [5, 6])
        assert m.rows == 48 and raw_load(e, m.blocks, 48, 0, [B_]) == 0 and e.seq_len(B_) == 48
        gen = e.prefix_pool_info()[2]
        e.weights_invalidate()
        assert e.prefix_pool_info()[2] != gen
        gen = e.prefix_pool_info()[2]
        family = e.set_decode_regime(-1)
        e.set_decode_regime(family)                              # the same family: nothing moves
        assert e.prefix_pool_info()[2] == gen
        e.set_decode_regime(1 - family)                          # the other decode family writes other rows: a new generation
        assert e.prefix_pool_info()[2] != gen
        e.set_decode_regime(-1)
        e.seq_reset(B_)
        assert raw_load(e, m.blocks, 48, 0, [B_]) == INVALID and e.seq_len(B_) == 0
        assert cache.match(ids + [5, 6]).rows == 0 and not cache.blocks
        prefill_text(e, A, ids)                                  # saved again under the new generation, the blocks load again
        assert cache.save(A, ids, (), len(ids)) == 48
        m = cache.match(ids + [5, 6])
        assert m.rows == 48 and raw_load(e, m.blocks, 48, 0, [B_]) == 0
        assert all(torch.equal(g, w) for g, w in zip(kv_rows(e, B_, 0, 48), kv_rows(e, A, 0, 48)))
    finally:
        cache.close()
        e.seq_reset(A), e.seq_reset(B_)


# ---------------------------------------------------------------- 5. errors
def test_refused_calls_change_nothing(eng):
    e = eng
    lib, h = e.lib, e.h
    e.prefix_pool_destroy()
    assert raw_save(e, A, 0, [0]) == INVALID and raw_load(e, [0], 16, 0, [B_]) == INVALID        # no pool
    assert lib.ze_prefix_pool_create(h, 8, 12) == INVALID        # block_rows: a multiple of 8 ...
    assert lib.ze_prefix_pool_create(h, 8, CTX + 8) == INVALID   # ... at most max_ctx
    assert lib.ze_prefix_pool_create(h, 0, 16) == INVALID and lib.ze_prefix_pool_create(h, 8, 0) == INVALID
    assert lib.ze_prefix_pool_create(h, 1 << 28, 16) == NOMEM    # 8 TiB: the allocation fails, the engine stays usable
    assert e.prefix_pool_info()[:2] == (0, 0)
    assert lib.ze_prefix_pool_create(h, POOL, BR) == 0
    assert lib.ze_prefix_pool_create(h, POOL, BR) == INVALID     # one pool per engine
    prefill_text(e, A, text_ids(71, 40))
    prefill_text(e, B_, text_ids(72, 60))
    prefill_text(e, C_, text_ids(73, 45))
    assert raw_save(e, A, 0, [3, 4]) == 0

    def snapshot():
        return ([e.seq_len(s) for s in (A, B_, C_)], [lib.ze_seq_prefix_hint(h, s) for s in (A, B_, C_)],
                [kv_rows(e, s, 0, 60) for s in (A, B_, C_)])

    def same(x, y):
        return x[0] == y[0] and x[1] == y[1] and all(torch.equal(u, v) for p, q in zip(x[2], y[2]) for u, v in zip(p, q))

    before = snapshot()
    assert raw_save(e, A, 8, [5]) == INVALID                     # row0 no multiple of block_rows
    assert raw_save(e, A, -16, [5]) == INVALID
    assert raw_save(e, A, 32, [5]) == INVALID                    # rows 32 .. 47 of a chain of 40
    assert raw_save(e, A, 0, [5, 6, 7]) == INVALID
    assert raw_save(e, A, 0, [5, 5]) == INVALID                  # a block named twice
    assert raw_save(e, A, 0, [5], n=0) == INVALID and e.lib.ze_prefix_save(h, A, 0, None, 1, e._stream()) == INVALID
    assert raw_save(e, A, 0, [POOL]) == NOTFOUND and raw_save(e, A, 0, [-1]) == NOTFOUND
    assert raw_save(e, SLOTS, 0, [5]) == NOTFOUND and raw_save(e, -1, 0, [5]) == NOTFOUND
    assert raw_load(e, [3, 4], 0, 0, [B_]) == INVALID
    assert raw_load(e, [3, 4], 33, 0, [B_]) == INVALID           # past the blocks
    assert raw_load(e, [3, 4], 16, 0, [B_]) == INVALID           # does not reach into the last block
    assert raw_load(e, [3, 4], 20, 21, [B_]) == INVALID and raw_load(e, [3, 4], 20, -1, [B_]) == INVALID   # split row outside the rows
    assert raw_load(e, [3, 5], 20, 0, [B_]) == INVALID           # block 5 was never saved
    assert raw_load(e, [3, 4], 20, 0, [B_, C_, B_]) == INVALID   # a destination named twice
    assert raw_load(e, [3, 4], 20, 0, [B_], n=0) == INVALID and raw_load(e, [3, 4], 20, 0, [B_], n_blocks=0) == INVALID
    assert raw_load(e, [3, POOL], 20, 0, [B_]) == NOTFOUND and raw_load(e, [-1], 10, 0, [B_]) == NOTFOUND
    assert raw_load(e, [3, 4], 20, 0, [B_, SLOTS]) == NOTFOUND and raw_load(e, [3, 4], 20, 0, [-1]) == NOTFOUND
    torch.cuda.synchronize()
    assert same(before, snapshot())
    assert raw_load(e, [3, 4], 20, 0, [B_, C_]) == 0             # and what the refused calls named is accepted when it is right
    assert e.seq_len(B_) == 20 and e.seq_len(C_) == 20
    assert all(torch.equal(g, w) for g, w in zip(kv_rows(e, C_, 0, 20), kv_rows(e, A, 0, 20)))
    assert lib.ze_prefix_pool_destroy(h) == 0 and lib.ze_prefix_pool_destroy(h) == 0
    for s in (A, B_, C_):
        e.seq_reset(s)


# ---------------------------------------------------------------- 3 / 6 / 7. scheduler and server
@pytest.fixture(scope="module")
def stack():
    from tiny_tok import make_tokenizer
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.modeling import ZoomEarthForConditionalGeneration
    from zoomearth_amd.processor import ZoomEarthProcessor
    model = ZoomEarthForConditionalGeneration.from_synthetic(ModelConfig.tiny(), **CHAIN_W, max_seqs=4, max_ctx=1024,
                                                            max_patches=1024, max_tile_side=1024)
    proc = ZoomEarthProcessor(make_tokenizer(), min_pixels=3136, max_pixels=128 * 128 * 28 * 28)
    proc.tokenizer.padding_side = "left"
    yield model, proc
    model.engine.close()


def words(seed, n):
    return " ".join(f"w{int(v)}" for v in prng.uniform_ints(seed, n, 10, 1990))


def one_by_one(sched, reqs):
    """server style: every request is submitted once the one before it has finished"""
    for r in reqs:
        sched.submit(r)
        sched.run()


def test_stage_two_as_a_separate_request_hits_the_rows_stage_one_left(stack):
    """With the trained byte-level BPE of tests/tiny_tok.py: stage 2 re-tokenises the DECODED reply, so its ids follow the generated
    ones only as far as the two tokenisations agree -- the match stops there, at the last full block."""
    from tiny_tok import bpe_word, make_bpe_tokenizer
    from zoomearth_amd.processor import ZoomEarthProcessor
    from zoomearth_amd.scheduler import ChainScheduler, Request
    model, _ = stack
    proc = ZoomEarthProcessor(make_bpe_tokenizer(), min_pixels=3136, max_pixels=128 * 128 * 28 * 28)
    tok = lambda s: proc(text=[s], return_tensors="pt")["input_ids"][0].tolist()   # noqa: E731
    say = lambda seed, n: " ".join(bpe_word(int(v)) for v in prng.uniform_ints(seed, n, 0, 260))   # noqa: E731
    p1 = say(91, 45)
    cfg = model.config
    special = (cfg.image_token_id, cfg.vision_start_token_id, cfg.vision_end_token_id)

    def flow(**kw):
        sched = ChainScheduler(model, proc, do_sample=False, burst=4, ignore_eos=True, **kw)
        r1 = Request(prompt=p1, images=[], max_new_tokens=40)
        one_by_one(sched, [r1])
        text = "".join(ch for ch in r1.text if ch.isprintable()) or "w3"
        r2 = Request(prompt=p1 + " " + text + " " + say(92, 9), images=[], max_new_tokens=12)
        one_by_one(sched, [r2])
        return sched, r1, r2

    off, a1, a2 = flow()
    on, b1, b2 = flow(prefix_cache_rows=64 * BR, prefix_cache_block_rows=BR)
    try:
        assert list(b1.tokens) == list(a1.tokens) and b1.text == a1.text and b2.prompt == a2.prompt
        # what stage 1 left: its prompt's rows and those of the generated ids that went through the model (up to an id that could
        # open or close an image block)
        gen = [int(t) for t in b1.tokens[:-1]]
        gen = gen[:next((i for i, t in enumerate(gen) if t in special), len(gen))]
        held, ids2, n1 = tok(p1) + gen, tok(b2.prompt), len(tok(p1))
        agree = next((i for i in range(min(len(held), len(ids2))) if held[i] != ids2[i]), min(len(held), len(ids2)))
        saved = len(held) // BR * BR
        hit = min(min(agree, saved) // BR * BR, len(ids2) - 1)
        print(f"prompt {n1} rows, held {len(held)}, saved {saved}, agree {agree}, stage-2 prompt {len(ids2)}, hit {hit}")
        assert n1 >= 2 * BR and agree >= n1 and hit >= n1 // BR * BR
        assert agree < len(held), "the re-tokenised reply has to leave the generated ids somewhere"
        assert hit < saved, "the match has to stop short of what stage 1 left"
        assert on.stats["prefix_cache_hit_rows"] == hit and b2.cached_tokens == hit
        assert on.stats["prefix_cache_saved_rows"] >= saved
        assert on.stats["prefill_rows"] == off.stats["prefill_rows"] - hit
        assert "prefix_cache_hit_rows" not in off.stats
        assert list(b2.tokens) == list(a2.tokens) and b2.text == a2.text
    finally:
        on.close()


def test_eviction_under_pressure_never_serves_stale_rows(stack):
    from zoomearth_amd.scheduler import ChainScheduler, Request
    model, proc = stack
    prompts = [words(101 + i, 50) for i in range(3)]             # three blocks and a part each
    order = [0, 1, 2, 0, 2, 1, 1]

    def flow(**kw):
        sched = ChainScheduler(model, proc, do_sample=False, burst=4, ignore_eos=True, reuse_generated=False, **kw)
        reqs = [Request(prompt=prompts[i], images=[], max_new_tokens=6) for i in order]
        seen = []
        for r in reqs:
            c = sched.prefix_cache
            if c is not None:
                seen.append(c.match(proc(text=[r.prompt], return_tensors="pt")["input_ids"][0].tolist()).rows)
            one_by_one(sched, [r])
            if c is not None:                                    # the pool never over-commits
                held = [b.id for b in c.blocks.values()]
                assert len(held) + len(c.free) == 4 and sorted(held + c.free) == [0, 1, 2, 3]
        return sched, reqs, seen

    off, want, _ = flow()
    on, got, seen = flow(prefix_cache_rows=4 * BR, prefix_cache_block_rows=BR)
    try:
        n = len(proc(text=[prompts[0]], return_tensors="pt")["input_ids"][0].tolist())
        assert n // BR >= 3
        assert [r.cached_tokens for r in got] == seen
        assert seen[:3] == [0, 0, 0] and seen[3] < n // BR * BR   # prompt 0 again: its blocks went when 1 and 2 were stored -- a miss, or a part
        assert seen[6] >= 3 * BR                                 # the same prompt twice in a row: a hit
        assert on.stats["prefix_cache_evicted_blocks"] > 0 and on.stats["prefix_cache_hit_rows"] == sum(seen)
        assert [list(r.tokens) for r in got] == [list(r.tokens) for r in want]
    finally:
        on.close()


def test_the_server_reports_cached_tokens_and_answers_as_without_the_cache(stack):
    from fastapi.testclient import TestClient
    from zoomearth_amd import serve
    model, proc = stack
    first = [{"role": "user", "content": words(111, 60)}]

    def talk(server):
        client = TestClient(serve.create_app(server))
        r1 = client.post("/v1/chat/completions", json={"model": "ZoomEarth", "messages": first, "max_tokens": 24})
        assert r1.status_code == 200, r1.text
        reply = r1.json()["choices"][0]["message"]["content"]
        msgs = first + [{"role": "assistant", "content": reply}, {"role": "user", "content": words(112, 8)}]
        r2 = client.post("/v1/chat/completions", json={"model": "ZoomEarth", "messages": msgs, "max_tokens": 12})
        assert r2.status_code == 200, r2.text
        server.close()
        return r1.json(), r2.json()

    a1, a2 = talk(serve.ChatServer(model, proc, "ZoomEarth"))
    cached = serve.ChatServer(model, proc, "ZoomEarth", prefix_cache_rows=2048)
    try:
        b1, b2 = talk(cached)
        assert "prompt_tokens_details" not in a1["usage"] and "prompt_tokens_details" not in a2["usage"]
        assert b1["usage"]["prompt_tokens_details"] == {"cached_tokens": 0}
        assert b2["usage"]["prompt_tokens_details"]["cached_tokens"] >= 32
        assert b2["usage"]["prompt_tokens_details"]["cached_tokens"] % 32 == 0
        assert b1["choices"] == a1["choices"] and b2["choices"] == a2["choices"]
        strip = lambda u: {k: v for k, v in u.items() if k != "prompt_tokens_details"}   # noqa: E731
        assert strip(b1["usage"]) == a1["usage"] and strip(b2["usage"]) == a2["usage"]
        assert cached.prefix_cache is None and model.engine.prefix_pool_info()[:2] == (0, 0)   # close() gave the pool back
    finally:
        cached.close()


def test_repeated_rollouts_on_the_same_samples_hit_the_pool_and_draw_the_same_chains():
    """rollout_two_stage(prefix_cache=): the cache outlives the call's scheduler; the second call's stage-1 prompts (system turn, view,
    question) come from the pool, and every completion is the one a call without a cache draws."""
    from test_gpu_rollout import bbox_tokenizer
    from test_gpu_infer_e2e import word
    from zoomearth_amd import hostloop as H
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.image import DeviceImage
    from zoomearth_amd.modeling import ZoomEarthForConditionalGeneration
    from zoomearth_amd.prefix_cache import PrefixCache
    from zoomearth_amd.processor import ZoomEarthProcessor
    from zoomearth_amd.rollout import rollout_two_stage
    model = ZoomEarthForConditionalGeneration.from_synthetic(ModelConfig.tiny(), **CHAIN_W, max_seqs=8, max_ctx=2048,
                                                            max_patches=8192, max_tile_side=2048, max_prefill_rows=8192)
    try:
        proc = ZoomEarthProcessor(bbox_tokenizer(), min_pixels=3136, max_pixels=128 * 128 * 28 * 28)
        tiles = [DeviceImage.from_numpy(prng.synthetic_tile(90 + t, 700, 900), model.engine) for t in range(2)]
        samples = []
        for i in range(3):
            q = " ".join(word(int(v)) for v in prng.uniform_ints(70 + i, 5, 0, 1999))
            samples.append(dict(prompt=H.stage1_prompt(q), image=tiles[i % 2], bbox=[1, 2, 3, 4] if i != 1 else []))
        kw = dict(num_generations=4, temperature=0.9, max_new_tokens=10, seed=11, with_logps=False)
        want = rollout_two_stage(model, proc, samples, **kw)
        cache = PrefixCache(model.engine, 8192, BR)
        first = rollout_two_stage(model, proc, samples, prefix_cache=cache, **kw)
        saved, hit = cache.stats["saved_rows"], cache.stats["hit_rows"]
        assert saved > 0
        second = rollout_two_stage(model, proc, samples, prefix_cache=cache, **kw)
        from zoomearth_amd.scheduler import cut_at_image_run
        ids1 = [proc(text=[s["prompt"]], images=[r.images[0]], return_tensors="pt")["input_ids"][0].tolist() for s, r in zip(samples, want[::4])]
        # what the pool can hold of a stage-1 prompt: its full blocks, less than the whole prompt, not ending inside the image run
        covered = [cut_at_image_run(i, min(len(i) // BR * BR, len(i) - 1), model.config.image_token_id) for i in ids1]
        print(f"stage-1 prompts {[len(i) for i in ids1]} rows, coverable {covered}; hit rows {hit} after the first call, "
              f"{cache.stats['hit_rows']} after the second")
        assert min(covered) >= BR and cache.stats["hit_rows"] - hit >= sum(covered)
        for got in (first, second):
            assert all(r.error is None for r in got)
            assert [(r.completion1_ids, r.completion2_ids) for r in got] == [(r.completion1_ids, r.completion2_ids) for r in want]
        cache.close()
    finally:
        model.engine.close()

"""CPU: the host side of the prefix cache (zoomearth_amd/prefix_cache.py) and its place in the scheduler, against a stub engine that
records the pool calls and keeps, per pool block, the TOKENS whose rows it was given -- so a chain assembled from loaded blocks and a
prefilled tail can be compared with the prompt it stands for, id for id.  Also: the C ABI exports and declares the five entries."""
import os
import re
from types import SimpleNamespace

import pytest

from conftest import ROOT
from test_scheduler_cpu import IMG, Proc, StubEngine, expected, make_model
from zoomearth_amd import _lib
from zoomearth_amd.prefix_cache import PrefixCache
from zoomearth_amd.scheduler import ChainScheduler, Request

B = 4   # rows per block in these tests


class PoolEngine(StubEngine):
    """StubEngine with the five pool entries: block id -> the ids whose rows it holds."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.config = SimpleNamespace(image_token_id=IMG)
        self.pool, self.generation, self.block_rows = None, 1, 0

    def prefix_pool_create(self, n_blocks, block_rows):
        assert self.pool is None
        self.log.append(("pool_create", n_blocks, block_rows))
        self.pool, self.block_rows, self.n_blocks = {}, block_rows, n_blocks

    def prefix_pool_destroy(self):
        self.log.append(("pool_destroy",))
        self.pool = None

    def prefix_pool_info(self):
        return (self.n_blocks, self.block_rows, self.generation) if self.pool is not None else (0, 0, self.generation)

    def prefix_save(self, slot, row0, blocks, stream=None):
        c = self.chains[slot]
        rows = c["ids"] + c["out"][:-1]
        n = len(blocks) * self.block_rows
        assert row0 % self.block_rows == 0 and row0 + n <= len(rows) and len(set(blocks)) == len(blocks)
        assert all(0 <= b < self.n_blocks for b in blocks)
        self.log.append(("save", slot, row0, list(blocks)))
        for j, b in enumerate(blocks):
            self.pool[b] = (self.generation, rows[row0 + j * self.block_rows: row0 + (j + 1) * self.block_rows])

    def prefix_load(self, blocks, n_rows, split_row, dsts):
        assert (len(blocks) - 1) * self.block_rows < n_rows <= len(blocks) * self.block_rows
        assert all(self.pool[b][0] == self.generation for b in blocks), "stale block"
        self.log.append(("load", list(blocks), n_rows, split_row, list(dsts)))
        rows = [t for b in blocks for t in self.pool[b][1]][:n_rows]
        for d in dsts:
            self.chains[d] = dict(ids=list(rows), out=[], fin=False)


def pool_calls(e):
    return [x for x in e.log if x[0] in ("pool_create", "pool_destroy", "save", "load")]


def text(first, n):
    return [first + i for i in range(n)]


# ------------------------------------------------------------------ keys
def test_keys_are_chained_over_ids_and_the_images_that_reach_into_a_block():
    c = PrefixCache(PoolEngine(), 64, B)
    a = text(10, 12)
    ka = c.block_keys(a, [])
    assert len(ka) == 3 and len(set(ka)) == 3
    assert c.block_keys(a + [99], []) == ka                              # only full blocks
    assert c.block_keys(a, [], n_rows=9) == ka[:2]
    b = list(a)
    b[5] = 77                                                            # block 1 differs: its key and every later one
    kb = c.block_keys(b, [])
    assert kb[0] == ka[0] and kb[1] != ka[1] and kb[2] != ka[2]
    same_block_elsewhere = text(50, 4) + a[4:8]
    assert c.block_keys(same_block_elsewhere, [])[1] != ka[1]            # the same ids behind another prefix are another block
    # an image run over rows 2 .. 5 reaches into blocks 0 and 1; block 2 holds no image token but follows them
    ids = [10, 11] + [IMG] * 4 + text(20, 6)
    k1, k2 = c.block_keys(ids, ["view A"]), c.block_keys(ids, ["view B"])
    assert len(k1) == 3 and all(x != y for x, y in zip(k1, k2))
    two = text(10, 4) + [IMG] * 4 + [30, 31, 32, 33] + [IMG] * 4         # blocks: text | image 0 | text | image 1
    ka, kb = c.block_keys(two, ["a", "b"]), c.block_keys(two, ["a", "c"])
    assert ka[:3] == kb[:3] and ka[3] != kb[3]
    assert c.block_keys(two, ["a", None]) == ka[:3]                      # no key: that block and what follows is never stored
    assert c.block_keys(two, [None, "b"]) == ka[:1]
    assert c.block_keys(two, ["a"]) == ka[:3]                            # (a run without an entry counts as keyless)


# ------------------------------------------------------------------ match
def filled(cache, e, slot, ids, keys=()):
    """a chain of `ids` in `slot`, saved"""
    e.chains[slot] = dict(ids=list(ids), out=[], fin=False)
    return cache.save(slot, ids, keys, len(ids))


def test_match_is_the_longest_present_chain_trimmed_like_a_shared_prefix():
    e = PoolEngine()
    c = PrefixCache(e, 64, B)
    assert c.match(text(10, 12)).rows == 0
    a = text(10, 14)
    assert filled(c, e, 0, a) == 12                                      # three full blocks; the two odd rows are not stored
    m = c.match(a + [1, 2, 3])
    assert (m.rows, len(m.blocks), m.images) == (12, 3, 0)
    assert [e.pool[b][1] for b in m.blocks] == [a[0:4], a[4:8], a[8:12]]
    assert c.match(a[:12]).rows == 11 and len(c.match(a[:12]).blocks) == 3     # a non-empty tail stays
    assert c.match(a[:9]).rows == 8 and len(c.match(a[:9]).blocks) == 2
    assert c.match(a[:6] + [999] + a[7:]).rows == 4                      # diverges inside block 1
    assert c.match([999] + a[1:]).rows == 0
    # an image run over rows 6 .. 9: a match that would end at row 8 backs off to the run's start, and counts no image
    ids = text(10, 6) + [IMG] * 4 + text(30, 6)
    assert filled(c, e, 1, ids, ["v"]) == 12                              # (block 0 is `a`'s: stored once)
    assert c.match(ids + [5], ["v"]).rows == 16 and c.match(ids + [5], ["v"]).images == 1
    cut = c.match(ids[:9] + [IMG, 41, 42, 43], ["v"])                     # same first two blocks, then another continuation
    assert (cut.rows, len(cut.blocks), cut.images) == (6, 2, 0)
    assert c.match(ids + [5], ["w"]).rows == 4                            # another image: only the block in front of it
    assert c.match(ids + [5], [None]).rows == 4
    whole = c.match(ids[:10] + [77, 78, 79], ["v"])                      # the run ends at row 10: block 2 differs, the cut falls inside the run
    assert (whole.rows, whole.images) == (6, 0)


def test_lru_eviction_leaves_first_and_never_a_pinned_block():
    e = PoolEngine()
    c = PrefixCache(e, 6 * B, B)                                          # six blocks
    a, b = text(100, 8), text(200, 8)
    assert filled(c, e, 0, a) == 8 and filled(c, e, 1, b) == 8 and len(c.free) == 2
    ma = c.match(a + [1])                                                 # `a` is the more recently used chain now
    assert ma.rows == 8
    x = text(300, 16)                                                     # four blocks: two free, two evicted -- b's, leaf first
    assert filled(c, e, 2, x) == 16
    assert c.stats["evicted_blocks"] == 2 and c.match(b + [1]).rows == 0 and c.match(a + [1]).rows == 8
    assert c.match(x + [1]).rows == 16
    # a pinned chain survives pressure; what does not fit is left out from the chain's end, and the pool never over-commits
    c.pin(ma)
    y = text(400, 24)                                                     # six blocks wanted, four evictable (x's)
    assert filled(c, e, 3, y) == 16
    assert c.match(a + [1]).rows == 8 and c.match(x + [1]).rows == 0 and c.match(y).rows == 16
    assert len(c.blocks) + len(c.free) == 6 and len({blk.id for blk in c.blocks.values()} | set(c.free)) == 6
    c.unpin(ma)
    z = text(500, 8)
    c.match(y)                                                            # y most recent: a goes, its leaf first
    assert filled(c, e, 0, z) == 8 and c.match(a + [1]).rows == 0 and c.match(y).rows == 16
    saves = [x for x in e.log if x[0] == "save"]
    assert all(len(s[3]) == len(set(s[3])) for s in saves)
    # a parent is never evicted before its child: every present block's parent is present
    assert all(blk.parent is None or blk.parent in c.blocks for blk in c.blocks.values())
    # extending a stored chain stores only the new blocks, from the right row
    e.chains[1] = dict(ids=z + text(600, 4), out=[], fin=False)
    assert c.save(1, z + text(600, 4), (), 12) == 4 and e.log[-1][:3] == ("save", 1, 8)


def test_a_generation_change_empties_the_cache():
    e = PoolEngine()
    c = PrefixCache(e, 32, B)
    a = text(10, 8)
    filled(c, e, 0, a)
    assert c.match(a + [1]).rows == 8
    e.generation += 1                                                     # what ze_weights_invalidate does
    assert c.match(a + [1]).rows == 0 and not c.blocks and len(c.free) == 8 and c.stats["flushes"] == 1
    assert filled(c, e, 0, a) == 8 and c.match(a + [1]).rows == 8         # saved again under the new generation
    loads = len([x for x in e.log if x[0] == "load"])
    c.load(c.match(a + [1]), [1, 2])
    assert len([x for x in e.log if x[0] == "load"]) == loads + 1 and e.chains[2]["ids"] == a


# ------------------------------------------------------------------ scheduler
def pool_model(**kw):
    m = make_model()
    m.engine = PoolEngine(**kw)
    return m


def run(sched, reqs):
    for r in reqs:
        sched.submit(r)
    sched.run()


def words(ids):
    return " ".join(str(i) for i in ids)


def test_without_the_argument_the_scheduler_makes_no_pool_call():
    model = pool_model(max_seqs=2)
    sched = ChainScheduler(model, Proc(), burst=2)
    assert sched.prefix_cache is None and not any(k.startswith("prefix_cache") for k in sched.stats)
    reqs = [Request(prompt=words(text(11 + 2 * q, 9)), images=[], max_new_tokens=4) for q in range(3)]
    run(sched, reqs)
    assert pool_calls(model.engine) == [] and all(r.tokens == expected(11 + 2 * q, 4) for q, r in enumerate(reqs))
    # and a plain StubEngine, which has no pool entry at all, serves it
    sched = ChainScheduler(make_model(max_seqs=2), Proc(), burst=2, prefix_cache_rows=0)
    run(sched, [Request(prompt=words(text(11, 9)), images=[], max_new_tokens=4)])


def test_retired_chains_feed_later_ones_through_the_pool():
    model = pool_model(max_seqs=3)
    e = model.engine
    sched = ChainScheduler(model, Proc(), burst=2, prefix_cache_rows=16 * B, prefix_cache_block_rows=B)
    assert pool_calls(e) == [("pool_create", 16, B)]
    p1 = text(11, 10)                                                     # odd first id: no EOS
    r1 = Request(prompt=words(p1), images=[], max_new_tokens=6)
    run(sched, [r1])
    gen = expected(11, 6)
    assert r1.tokens == gen and sched.stats["prefix_cache_hit_rows"] == 0 and r1.cached_tokens == 0
    # saved on retirement: the prompt's rows and those of the generated tokens that went through the model (all but the last)
    assert sched.stats["prefix_cache_saved_rows"] == (10 + 5) // B * B == 12
    assert e.log[-1][0] == "save" or [x[0] for x in e.log].index("save") > 0
    # stage-2 shape: the next prompt repeats prompt + reply, then goes on; a sibling prompt shares only the first two blocks
    p2 = p1 + gen + [70, 71, 72]
    p3 = p1[:9] + [80, 81, 82, 83]
    r2 = Request(prompt=words(p2), images=[], max_new_tokens=3)
    r3 = Request(prompt=words(p3), images=[], max_new_tokens=3)
    r4 = Request(prompt=words(p3), images=[], max_new_tokens=3)
    run(sched, [r2, r3, r4])
    loads = [x for x in e.log if x[0] == "load"]
    assert sorted((x[2], len(x[4])) for x in loads) == [(8, 2), (12, 1)]  # r3 and r4: ONE load of two blocks for both
    assert (r2.cached_tokens, r3.cached_tokens, r4.cached_tokens) == (12, 8, 8)
    assert sched.stats["prefix_cache_hit_rows"] == 12 + 8 + 8
    prefills = [x for x in e.log if x[0] == "prefill"][1:]
    assert sorted(n for x in prefills for n in x[2]) == sorted([len(p2) - 12, len(p3) - 8, len(p3) - 8])
    assert (r2.tokens, r3.tokens) == (expected(11, 3), expected(11, 3)) and r4.tokens == r3.tokens
    assert not sched.live and sorted(sched.free) == [0, 1, 2] and not any(b.pins for b in sched.prefix_cache.blocks.values())


def test_a_prompt_logprobs_request_takes_nothing_from_the_pool_but_saves():
    model = pool_model(max_seqs=2)
    e = model.engine
    e.score_batch_detail = None   # (never reached: the stub has no scoring pass; the plan is what is checked)
    sched = ChainScheduler(model, Proc(), burst=2, prefix_cache_rows=8 * B, prefix_cache_block_rows=B)
    run(sched, [Request(prompt=words(text(11, 10)), images=[], max_new_tokens=2)])
    item = dict(req=SimpleNamespace(_chain=SimpleNamespace(wants_prompt_logprobs=True), slot=0), ids=text(11, 10) + [1, 2], keys=[],
                reuse=0, n_reused=0, copy_from=None)
    plain = dict(item, req=SimpleNamespace(_chain=SimpleNamespace(wants_prompt_logprobs=False), slot=1))
    assert sched._plan_sharing([item, plain]) == []
    assert "cached" not in item and item["reuse"] == 0
    assert plain["cached"].rows == 8 and plain["reuse"] == 8
    sched._unpin(plain)


def test_a_prompt_logprobs_chain_runs_without_the_pool_and_leaves_its_rows_there():
    import torch
    model = pool_model(max_seqs=2)
    e = model.engine

    def score_batch_detail(slots, ids_l, emb_l, pos_l, dl, score_from=None, top_n=0, rank=False):
        e.prefill_batch(slots, ids_l, emb_l, pos_l, dl)
        e.log.append(("score", list(slots), list(score_from)))
        n = [len(x) - 1 - f for x, f in zip(ids_l, score_from)]
        return SimpleNamespace(chain=lambda k: SimpleNamespace(logps=torch.zeros(n[k]), rank=torch.zeros(n[k], dtype=torch.int64),
                                                               top_ids=None, top_logprobs=None))
    e.score_batch_detail = score_batch_detail
    sched = ChainScheduler(model, Proc(), burst=2, prefix_cache_rows=8 * B, prefix_cache_block_rows=B)
    p = text(11, 10)
    run(sched, [Request(prompt=words(p), images=[], max_new_tokens=2)])
    assert sched.stats["prefix_cache_saved_rows"] == 8
    # the same prompt with prompt_logprobs: every row goes through its own pass although the pool holds two blocks of it ...
    asker = Request(prompt=words(p + [70, 71, 72, 73, 74]), images=[], max_new_tokens=3, prompt_logprobs=0)
    run(sched, [asker])
    assert not [x for x in e.log if x[0] == "load"] and asker.cached_tokens == 0
    assert [x for x in e.log if x[0] == "score"][-1][2] == [0] and len(asker.prompt_token_logprobs) == 15
    # ... and when it retires its rows go to the pool like any chain's: the two blocks it adds, from row 8
    assert sched.stats["prefix_cache_saved_rows"] == 8 + 8 and e.log[-1][:3] == ("save", asker.slot if asker.slot >= 0 else 0, 8)
    after = Request(prompt=words(p + [70, 71, 72, 73, 74, 75, 76, 77]), images=[], max_new_tokens=2)
    run(sched, [after])
    assert after.cached_tokens == 12 and sched.stats["prefix_cache_hit_rows"] == 12   # (block 3 ends in a generated id, not in 75)
    sched.close()
    assert e.pool is None and e.log[-1] == ("pool_destroy",)


def test_a_chain_that_is_released_after_its_prefill_saves_its_prompt():
    """`_release` of a chain that ran: a request whose grammar cannot be had fails when it would join the live set, behind its
    completed prefill pass -- its prompt's rows go to the pool before the slot is reset.  A request that fails BEFORE its pass saves
    nothing."""
    model = pool_model(max_seqs=2)
    e = model.engine
    sched = ChainScheduler(model, Proc(), burst=2, prefix_cache_rows=8 * B, prefix_cache_block_rows=B)
    errors = []
    p = text(21, 11)
    bad = Request(prompt=words(p), images=[], max_new_tokens=2, guided_regex="a", guided_choice=["b"],
                  on_error=lambda r, ex: errors.append(ex))
    run(sched, [bad])
    assert len(errors) == 1 and isinstance(errors[0], ValueError)
    saves = [x for x in e.log if x[0] == "save"]
    assert len(saves) == 1 and saves[0][2] == 0 and len(saves[0][3]) == 2           # rows 0 .. 7 of its eleven
    assert [x[0] for x in e.log].index("save") > [x[0] for x in e.log].index("prefill")
    assert sched.stats["prefix_cache_saved_rows"] == 8 and sorted(sched.free) == [0, 1]
    too_long = Request(prompt=words(text(31, 300)), images=[], max_new_tokens=2, on_error=lambda r, ex: errors.append(ex))
    run(sched, [too_long])
    assert len(errors) == 2 and sched.stats["prefix_cache_saved_rows"] == 8
    nxt = Request(prompt=words(p + [5, 6]), images=[], max_new_tokens=2)
    run(sched, [nxt])
    assert nxt.cached_tokens == 8
    # a save the engine refuses is counted and kept, and fails no request
    def refuse(*a, **k):
        raise RuntimeError("engine refused the save")
    e.prefix_save = refuse
    ok = Request(prompt=words(text(41, 9)), images=[], max_new_tokens=2)
    run(sched, [ok])
    assert ok.tokens == expected(41, 2) and sched.stats["prefix_cache_save_errors"] == 1
    assert "refused" in str(sched.prefix_cache_last_error)
    assert len(sched.prefix_cache.blocks) + len(sched.prefix_cache.free) == 8      # the block ids it had taken are free again
    sched.close()


def test_a_second_owner_adopts_the_pool_and_a_flush_voids_planned_matches():
    e = PoolEngine()
    first = PrefixCache(e, 8 * B, B)
    a = text(10, 8)
    filled(first, e, 0, a)
    second = PrefixCache(e, 8 * B, B)                                     # same shape: adopted, empty
    assert pool_calls(e)[0] == ("pool_create", 8, B) and len([x for x in pool_calls(e) if x[0] == "pool_create"]) == 1
    assert second.match(a + [1]).rows == 0
    with pytest.raises(ValueError):
        PrefixCache(e, 4 * B, B)
    m = first.match(a + [1])
    first.pin(m)
    e.generation += 1                                                     # a weight change between the plan and the load
    filled(first, e, 1, text(50, 8))                                      # ... and a save that takes the flushed ids
    loads = len([x for x in e.log if x[0] == "load"])
    with pytest.raises(RuntimeError):
        first.load(m, [2])
    assert len([x for x in e.log if x[0] == "load"]) == loads
    first.close()
    assert e.pool is None
    third = PrefixCache(e, 4 * B, B)                                      # after close any shape may be created
    assert third.n_blocks == 4


def test_the_pool_prefers_a_live_donor_and_replaces_the_rounds_anchor_pass():
    model = pool_model(max_seqs=4, max_ctx=512, max_prefill_rows=512)
    e = model.engine
    sched = ChainScheduler(model, Proc(), burst=2, prefix_cache_rows=64 * B, prefix_cache_block_rows=B, min_shared=8)
    head = words(text(21, 9)) + " <img> " + words(text(41, 7))            # 9 + 4 + 7 = 20 shared rows
    run(sched, [Request(prompt=head + " 90 91", images=["view"], max_new_tokens=2)])
    assert sched.stats["prefix_cache_saved_rows"] == 20
    n_vit = sched.stats["vit_calls"]
    # three questions about the same view arrive together after the first has retired: no pass A, one load for all three
    qs = [Request(prompt=head + f" {92 + q} 60 61", images=["view"], max_new_tokens=2) for q in range(3)]
    run(sched, qs)
    loads = [x for x in e.log if x[0] == "load"]
    assert len(loads) == 1 and loads[0][2] == 20 and len(loads[0][4]) == 3
    assert not [x for x in e.log if x[0] == "copy"]
    assert [q.cached_tokens for q in qs] == [20, 20, 20] and sched.stats["vit_calls"] == n_vit   # the image inside the match is not encoded again


# ------------------------------------------------------------------ the C ABI
def test_the_five_entries_are_declared_and_exported():
    names = {"ze_prefix_pool_create", "ze_prefix_pool_destroy", "ze_prefix_pool_info", "ze_prefix_save", "ze_prefix_load"}
    assert names <= set(_lib.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "zoomearth.h")).read()
    declared = set(re.findall(r"^int\s+(ze_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    assert names <= declared
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.lib()
    for n in names:
        assert getattr(lib, n) is not None
    src = open(os.path.join(ROOT, "zoomearth_amd", "csrc", "Makefile")).read()
    assert "ze_prefix.hip" in src

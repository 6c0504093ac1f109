"""GPU: per-chain token rules (ze_seq_set_token_rules / ze_op_token_rules) -- the two kernels against the restatement
(tests/token_rules_ref.py), the decode path against the logits of its own steps, mixed rules under one graph, the request's
lifetime, and the public surfaces end to end.

No tolerance anywhere: a ban is a store of -inf and a stop is a flag, so rows are compared by their bit patterns and tokens by
equality."""
import numpy as np
import pytest
import torch

import token_rules_ref as R
from gpu_util import CHAIN_W, tiny_engine  # noqa: F401
from oracle import prng
from zoomearth_amd._lib import ZoomEarthError

pytestmark = pytest.mark.gpu

VOCAB, MAX_CTX, PAD = 2048, 1024, 2043   # ModelConfig.tiny(), the tiny_engine fixture
ALPHABET = [0, 2047, 7, 300, 1999, 64]    # few distinct ids, so that n-grams repeat; the vocabulary's two ends among them


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


# ---------------------------------------------------------------- 1. the kernels alone against the restatement
def op_cases():
    """(history, n_context, n, ban records, stop records, min_new) per row"""
    rng = np.random.default_rng(7)
    cases = []
    for n in (1, 2, 3, 16):
        for L in sorted({0, max(n - 2, 0), n - 1, n, 255, 256, 257, MAX_CTX}):
            k = 2 if n == 16 else len(ALPHABET)          # (two symbols: 15-id tails do repeat)
            h = rng.choice(ALPHABET[:k], size=L).tolist()
            if n == 16 and L >= 64:
                h[-15:] = h[20:35]                        # a certain match of the whole tail
            cases.append((h, int(rng.integers(0, L + 1)), n, [], [], 0))
    cases += [
        ([5, 6, 7, 9, 5, 6], 2, 3, [], [], 0),             # the matched 3-gram straddles the context / generated boundary
        ([4, 4, 4, 4], 1, 3, [], [], 0),                   # periodic: the tail overlaps its own matches
        ([4, 4, 4, 4], 4, 2, [], [], 0),
        ([11, 12, 13], 1, 0, [[0], [2047]], [], 0),        # one-id records: always banned, the vocabulary's two ends
        ([8, 9], 0, 0, [[8, 9, 11], [9, 12], [7, 8, 9, 13]], [], 0),   # a prefix that IS the history; one longer than the history
        ([9], 1, 0, [[8, 9, 11]], [], 0),
        ([], 0, 0, [[8, 9], [3]], [], 0),                  # empty history: only the one-id record
        ([1, 2, 3, 4], 2, 0, [], [[3, 4]], 0),             # a stop record equal to the whole generated tail
        ([1, 2, 3, 4], 2, 0, [], [[9], [1, 2, 3, 4], [4]], 0),   # (the long record would reach into the context; the last one hits)
        ([1, 2, 3], 2, 0, [], [[2, 3]], 0),                # would match only by reaching into the context
        ([1, 2, 3, 4], 2, 0, [], [[3, 4]], 3),             # suppressed by min_new
        ([1, 2, 3, 4], 2, 0, [], [[3, 4]], 2),
        ([1, 2, 3, 4], 4, 0, [], [[4]], 0),                # nothing generated
        ([3, 1, 4, 1, 5], 2, 0, [], [], 0),                # a row without a request among rows with one
        ([3, 1, 4, 1, 5, 9, 2, 6], 3, 2, [[6, 10], [2, 6, 0]], [[2, 6], [7]], 1),   # all three at once
    ]
    # 64 records, 16 ids each where the list allows (1024 ints in all): some match the tail, some do not
    h = rng.choice(ALPHABET, size=40).tolist()
    recs = [h[-15:] + [int(1000 + i)] if i % 3 == 0 else rng.choice(ALPHABET, size=int(rng.integers(1, 15))).tolist() + [int(1100 + i)]
            for i in range(64)]
    while sum(1 + len(r) for r in recs) > 1024:
        recs[[len(r) for r in recs].index(16)] = [int(1200 + sum(len(r) for r in recs) % 100)]
    cases.append((h, 17, 0, recs, recs[:64], 0))
    return cases


def test_kernels_equal_the_restatement(tiny_engine):
    e = tiny_engine
    cases = op_cases()
    rows, pad = len(cases), 5
    g = torch.Generator().manual_seed(11)
    host = (torch.randn((rows, VOCAB + pad), generator=g) * 4).float().numpy()
    host[:, 5] = -0.0
    host[3, 7] = -np.inf
    dev = torch.from_numpy(host).cuda()
    out = torch.full((rows, VOCAB + pad), 123.0, dtype=torch.float32, device="cuda")
    got, hit = e.op_token_rules(dev[:, :VOCAB], [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases],
                                [c[3] for c in cases], [c[4] for c in cases], [c[5] for c in cases], out=out[:, :VOCAB])
    torch.cuda.synchronize()
    full, hit = out.cpu().numpy(), hit.cpu().numpy()
    assert (full[:, VOCAB:] == 123.0).all()                              # the padding of the row stride stays untouched
    some_ban = some_stop = 0
    for r, (h, nc, n, ban, stop, mn) in enumerate(cases):
        want = R.ban_row(host[r, :VOCAB], h, nc, n, ban)
        assert same_bits(full[r, :VOCAB], want), (r, len(h), n)
        assert int(hit[r]) == int(R.stop_hit(h[nc:], stop, mn)), (r, h, stop)
        some_ban += int(not same_bits(want, host[r, :VOCAB]))
        some_stop += int(hit[r])
    assert some_ban >= 15 and some_stop >= 4                             # (the cases are not vacuous)
    assert same_bits(full[-3, :VOCAB], host[-3, :VOCAB])                  # the row without a request


# ---------------------------------------------------------------- 2. the decode path applies the rules to every step's own row
def text_ids(seed, n):
    return prng.uniform_ints(seed, n, 10, 1990).tolist()


def prefill_text(e, seq, ids):
    pos, delta = e.rope_index(ids, [])
    e.seq_reset(seq)
    return e.prefill(seq, ids, None, pos, delta, want_logits=True)


PROMPTS = [text_ids(41, 23), text_ids(42, 9), text_ids(43, 60)]
STEPS = 12
_FREE = {}


def free_run(e, w=0):
    """the free greedy run of prompt w under ignore_eos (made once)"""
    if w not in _FREE:
        prefill_text(e, 0, PROMPTS[w])
        _FREE[w] = e.generate(0, STEPS, ignore_eos=True)
    return _FREE[w]


def run_with(e, path, graph, ids, rules, steps=STEPS):
    first = prefill_text(e, 0, ids).cpu().numpy()
    e.set_token_rules(0, **rules)
    kw = dict(ignore_eos=True, use_graph=graph)
    toks = e.generate(0, steps, **kw) if path == "single" else e.generate_batch([0], steps, **kw)[0]
    return first, toks


def own_rows(e, path, ids, first, toks):
    """the raw row of every step: the prefill's, then the chain's ids teacher-forced through the same kind of step"""
    raw = [first]
    prefill_text(e, 0, ids)
    for t in range(len(toks) - 1):
        raw.append((e.decode_step(0, toks[t]) if path == "single" else e.decode_batch([0], [toks[t]])[0]).cpu().numpy())
    return raw


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("path", ["single", "batched"])
def test_decode_path_applies_the_rules_to_every_step(tiny_engine, path, graph):
    e = tiny_engine
    e.fill_synthetic(**CHAIN_W)
    ids = PROMPTS[0]
    g = free_run(e)
    assert len(g) == STEPS

    def check(rules, toks, first):
        raw = own_rows(e, path, ids, first, toks)
        for t, row in enumerate(raw):                                    # the first token too
            want = R.ban_row(row, list(ids) + toks[:t], len(ids), rules.get("no_repeat_ngram_size", 0), rules.get("bad_words", []))
            assert toks[t] == R.argmax_lowest(want), (rules, t, toks)

    # every step has bans: all generated ids are distinct and absent from the context
    rules = dict(no_repeat_ngram_size=1, context=ids)
    first, toks = run_with(e, path, graph, ids, rules)
    assert len(toks) == STEPS and len(set(toks)) == STEPS and not set(toks) & set(ids)
    check(rules, toks, first)
    # a two-id ban: the run follows g until g[3] is followed by g[4] for the first time
    rules = dict(bad_words=[[g[3], g[4]]], context=ids)
    first, toks = run_with(e, path, graph, ids, rules)
    k = next(t for t in range(1, STEPS) if g[t - 1] == g[3] and g[t] == g[4]) if ids[-1] != g[3] or g[0] != g[4] else 0
    assert toks[:k] == g[:k] and toks[k] != g[k], (k, g, toks)
    check(rules, toks, first)
    # a stop record: the run equals g up to the restatement's first hit, pads follow
    stop = [g[5:7]]
    n = R.first_hit(g, stop)
    assert n is not None and n <= 7
    first, toks = run_with(e, path, graph, ids, dict(stop=stop))
    assert toks == g[:n] + [PAD] * (STEPS - n), (n, g, toks)
    # min_new_tokens of the logit-adjust request holds a match back (vLLM's order): the next hit at or after it counts
    prefill_text(e, 0, ids)
    e.set_token_rules(0, stop=stop)
    e.seq_set_logit_adjust(0, min_new_tokens=n + 1)
    kw = dict(ignore_eos=True, use_graph=graph)
    toks = e.generate(0, STEPS, **kw) if path == "single" else e.generate_batch([0], STEPS, **kw)[0]
    n2 = R.first_hit(g, stop, n + 1)
    assert toks == (g if n2 is None else g[:n2] + [PAD] * (STEPS - n2)), (n, n2, g, toks)


def test_a_stopped_chain_is_finished_at_the_step_of_the_hit(tiny_engine):
    e = tiny_engine
    e.fill_synthetic(**CHAIN_W)
    g = free_run(e)
    stop = [g[5:7], [g[8]]]
    n = R.first_hit(g, stop)
    prefill_text(e, 0, PROMPTS[0])
    prefill_text(e, 1, PROMPTS[0])
    e.set_token_rules(0, stop=stop)
    params = e.gen_params(ignore_eos=True)                               # ignore_eos does not switch stop sequences off
    e.chain_begin(0, params)
    e.chain_begin(1, params)
    seen = []
    for _ in range(STEPS - 1):
        ran, ng, fin = e.decode_burst([0, 1], 1, params)
        seen.append((ng[0], fin[0], fin[1]))
    assert [f for _, f, _ in seen] == [ng >= n for ng, _, _ in seen] and not any(f for _, _, f in seen), (n, seen)
    t0 = e.chain_tokens(0, STEPS)                                        # (PAD is an EOS id: a finished chain's ids are trimmed at it)
    assert t0[:n] == g[:n] and set(t0[n:]) <= {PAD} and e.chain_tokens(1, STEPS) == g


# ---------------------------------------------------------------- 3. company and the default path
def test_mixed_rules_share_a_graph_and_do_not_depend_on_company(tiny_engine):
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.engine import Engine
    e = tiny_engine
    e.fill_synthetic(**CHAIN_W)
    kw = dict(repetition_penalty=1.1, ignore_eos=True)

    def run(eng, slots, rows, graph, rules=None, **more):
        for s, w in zip(slots, rows):
            prefill_text(eng, s, PROMPTS[w])
            eng.mark_seen(s, PROMPTS[w])
            if rules is not None and rules[w] is not None:
                eng.set_token_rules(s, **rules[w])
        return eng.generate_batch(slots, STEPS, use_graph=graph, **kw, **more)

    fresh = Engine(ModelConfig.tiny(), device=0, max_seqs=3, max_ctx=1024, max_patches=1024, max_tile_side=1024)
    try:   # an engine that never saw a request
        fresh.fill_synthetic(**CHAIN_W)
        never = run(fresh, [0, 1, 2], [0, 1, 2], True)
        never_s = run(fresh, [0, 1, 2], [0, 1, 2], True, do_sample=True, temperature=0.9, seed=3)
    finally:
        fresh.close()
    for more, base in ((dict(), never), (dict(do_sample=True, temperature=0.9, seed=3), never_s)):
        # chain 0: none; chain 1: its own first token banned + no repeated 2-gram; chain 2: stops on its own ids 3..4
        rules = [None, dict(no_repeat_ngram_size=2, bad_words=[[base[1][0]]], context=PROMPTS[1]), dict(stop=[base[2][3:5]])]
        assert run(e, [0, 1, 2], [0, 1, 2], True, **more) == base         # nobody asks: what the engine always computed
        mixed = run(e, [0, 1, 2], [0, 1, 2], True, rules, **more)
        assert mixed[0] == base[0]                                        # the chain without rules, next to two with some
        assert mixed[1][0] != base[1][0]
        n = R.first_hit(base[2], rules[2]["stop"])
        assert mixed[2] == base[2][:n] + [PAD] * (STEPS - n)
        assert run(e, [0, 1, 2], [0, 1, 2], False, rules, **more) == mixed   # eager
        if not more:
            for w in (1, 2):                                              # alone, in another slot, graph and eager: the same tokens
                slot = (w + 1) % 3
                alone = [None] * 3
                alone[w] = rules[w]
                assert run(e, [slot], [w], False, alone) == [mixed[w]]
                assert run(e, [slot], [w], True, alone) == [mixed[w]]
        # flipping the rules on a running engine re-captures the step and keeps the tokens
        assert run(e, [0, 1, 2], [0, 1, 2], True, **more) == base
        assert run(e, [0, 1, 2], [0, 1, 2], True, rules, **more) == mixed


# ---------------------------------------------------------------- 4. lifetime
def test_the_rules_end_with_the_slot(tiny_engine):
    e = tiny_engine
    e.fill_synthetic(**CHAIN_W)
    ids = PROMPTS[0]
    pos, delta = e.rope_index(ids, [])
    kw = dict(ignore_eos=True)
    prefill_text(e, 0, ids)
    plain = free_run(e)
    rules = dict(no_repeat_ngram_size=1, stop=[[ids[0]]], bad_words=[[plain[0]]], context=ids)   # (ids[0] is banned: no hit)

    def bring(how):
        """slot 1 becomes the prompt again, its last-position logits ready, by the route under test"""
        if how == "reset":
            prefill_text(e, 1, ids)
            return
        if how == "truncate":
            e.seq_truncate(1, len(ids) - 1)
        else:
            e.seq_copy_prefix(1, 0, len(ids) - 1)
        e.prefill(1, ids[-1:], None, pos[:, -1:], delta, want_logits=False)

    for how in ("reset", "truncate", "copy"):
        prefill_text(e, 1, ids)
        bring(how)
        assert e.generate(1, STEPS, **kw) == plain
        bring(how)
        e.set_token_rules(1, **rules)
        ruled = e.generate(1, STEPS, **kw)                                # (a graph of the slot exists: the request re-captures)
        assert ruled[0] != plain[0] and len(set(ruled)) == STEPS
        bring(how)
        assert e.generate(1, STEPS, **kw) == plain, how                   # the slot's next chain inherits nothing
    # all-off values clear the request
    prefill_text(e, 1, ids)
    e.set_token_rules(1, **rules)
    e.set_token_rules(1)
    assert e.generate(1, STEPS, **kw) == plain
    # over-limit requests are refused with a message and change nothing
    prefill_text(e, 1, ids)
    e.set_token_rules(1, bad_words=[[plain[0]]])
    for bad in (dict(no_repeat_ngram_size=17), dict(no_repeat_ngram_size=-1), dict(stop=[[1]] * 65), dict(bad_words=[[1]] * 65),
                dict(stop=[list(range(17))]), dict(stop=[[]]), dict(bad_words=[list(range(16))] * 64), dict(stop=[[VOCAB]]),
                dict(bad_words=[[3, -1]]), dict(no_repeat_ngram_size=2, context=[1] * (MAX_CTX + 1)),
                dict(no_repeat_ngram_size=2, context=[VOCAB])):
        with pytest.raises(ZoomEarthError) as err:
            e.set_token_rules(1, **bad)
        assert len(str(err.value)) > 10, bad
    with pytest.raises(ZoomEarthError):
        e.set_token_rules(3, no_repeat_ngram_size=2)                      # no such slot
    assert e.generate(1, 4, **kw)[0] != plain[0]                          # the request before them still holds
    e.set_token_rules(1, stop=[[1] * 15] * 64, bad_words=[[2] * 15] * 64, no_repeat_ngram_size=16, context=[1] * MAX_CTX)   # the largest
    e.seq_reset(1)
    prefill_text(e, 1, ids)
    assert e.generate(1, STEPS, **kw) == plain


# ---------------------------------------------------------------- 5. surfaces
@pytest.fixture(scope="module")
def stack():
    from tiny_tok import make_tokenizer
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.modeling import ZoomEarthForConditionalGeneration
    from zoomearth_amd.processor import ZoomEarthProcessor
    model = ZoomEarthForConditionalGeneration.from_synthetic(ModelConfig.tiny(), **CHAIN_W, max_seqs=4, max_ctx=2048,
                                                            max_patches=4096, max_tile_side=2048)
    proc = ZoomEarthProcessor(make_tokenizer(), min_pixels=3136, max_pixels=128 * 128 * 28 * 28)
    proc.tokenizer.padding_side = "left"
    yield model, proc
    model.engine.close()


def words(seed, n):
    return " ".join(f"w{int(v)}" for v in prng.uniform_ints(seed, n, 10, 1990))


SPECIAL = list(range(2000, 2048))   # kept out of the runs below, so that every generated id is a word of the tiny tokenizer


def test_generate_and_scheduler_stop_where_the_host_cut_says(stack):
    from zoomearth_amd.hostloop import first_stop_cut
    from zoomearth_amd.scheduler import ChainScheduler, Request
    model, proc = stack
    tok = proc.tokenizer
    prompt = words(31, 14)
    inp = proc(text=[prompt], return_tensors="pt").to(model.device)
    L = inp["input_ids"].shape[1]
    free = model.generate(**inp, max_new_tokens=STEPS, suppress_tokens=SPECIAL)[0, L:].tolist()
    assert len(free) == STEPS and max(free) < 2000
    s = tok.decode(free[5:7])
    n, text = first_stop_cut(tok, free, [s])
    assert n <= 7 and s not in text
    got = model.generate(**inp, max_new_tokens=STEPS, suppress_tokens=SPECIAL, stop_strings=[s], tokenizer=tok)[0, L:].tolist()
    assert got[:n] == free[:n] and all(t == model.config.pad_token_id for t in got[n:]), (n, free, got)
    with pytest.raises(ValueError, match="could not locate a tokenizer"):
        model.generate(**inp, max_new_tokens=2, stop_strings=[s])
    # a stop token id is kept; two rows of one call carry the rules each
    got = model.generate(**inp, max_new_tokens=STEPS, suppress_tokens=SPECIAL, stop_token_ids=[free[4]])[0, L:].tolist()
    k = free.index(free[4]) + 1
    assert got[:k] == free[:k] and all(t == model.config.pad_token_id for t in got[k:])
    two = proc(text=[prompt, prompt], return_tensors="pt", padding="longest").to(model.device)
    both = model.generate(**two, max_new_tokens=STEPS, suppress_tokens=SPECIAL, no_repeat_ngram_size=1, bad_words_ids=[[free[0]]])
    for b in range(2):
        row = both[b, L:].tolist()
        assert row[0] != free[0] and len(set(row)) == STEPS and not set(row) & set(inp["input_ids"][0].tolist())
    # under the scheduler a stopped request frees its slot for the one that waits
    ban = {i: float("-inf") for i in SPECIAL}
    req = Request(prompt=prompt, images=[], max_new_tokens=STEPS, logit_bias=ban, stop_ids=[tok.encode(s)])
    other = Request(prompt=prompt, images=[], max_new_tokens=STEPS, logit_bias=ban)
    sched = ChainScheduler(model, proc, burst=1, max_batch=1)
    sched.submit(req)
    sched.submit(other)
    sched.run()
    assert list(req.tokens) == free[:n] and list(other.tokens) == free
    assert sched.stats["steps"] <= (n - 1) + (STEPS - 1)                 # the first chain ran n - 1 steps, not STEPS - 1


def test_server_cuts_the_text_before_the_stop_string(stack):
    from zoomearth_amd import serve
    from zoomearth_amd.hostloop import first_stop_cut
    model, proc = stack
    tok = proc.tokenizer
    srv = serve.ChatServer(model, proc, "ZoomEarth")
    msgs = [{"role": "user", "content": words(21, 12)}]
    base = {"messages": msgs, "max_tokens": STEPS, "logit_bias": {str(i): -100 for i in SPECIAL}}
    plain = srv.complete(base)
    inp = proc(text=[serve.build_prompt(msgs)[0]], return_tensors="pt").to(model.device)
    L = inp["input_ids"].shape[1]
    free = model.generate(**inp, max_new_tokens=STEPS, logit_bias={i: -100.0 for i in SPECIAL})[0, L:].tolist()
    assert max(free) < 2000 and tok.decode(free, skip_special_tokens=True).strip() == plain["choices"][0]["message"]["content"]
    s = tok.decode(free[5:7])
    n, text = first_stop_cut(tok, free, [s])
    res = srv.complete({**base, "stop": s})
    assert res["choices"][0]["message"]["content"] == text.strip() and res["choices"][0]["finish_reason"] == "stop"
    assert res["usage"]["completion_tokens"] == n
    res = srv.complete({**base, "stop": ["never said", s]})
    assert res["choices"][0]["message"]["content"] == text.strip()
    # a stop token id is kept, as an EOS is
    res = srv.complete({**base, "stop_token_ids": [free[4]]})
    k = free.index(free[4]) + 1
    assert res["choices"][0]["message"]["content"] == tok.decode(free[:k]).strip() and res["choices"][0]["finish_reason"] == "stop"
    assert res["usage"]["completion_tokens"] == k
    assert srv.complete(base)["choices"][0]["message"] == plain["choices"][0]["message"]      # the next request inherits nothing
    for bad in (dict(stop=5), dict(stop=["a", 5]), dict(stop=["a"] * 5), dict(stop=[""]), dict(stop_token_ids="x"),
                dict(stop_token_ids=[2048]), dict(stop_token_ids=[1.5]), dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size="2")):
        with pytest.raises(serve.BadRequest):
            srv.complete({**base, **bad})

"""GPU: guided decoding (ze_grammar_create / ze_seq_set_grammar / ze_op_grammar_*) -- the kernels against the restatement
(tests/grammar_ref.py), the decode path against the logits of its own steps, the text against `re`, mixed grammars under one graph,
the request's lifetime, and the server end to end.

No tolerance anywhere: the mask is a store of -inf and the advance a table look-up, so rows are compared by their bit patterns and
tokens and states by equality."""
import copy
import re

import numpy as np
import pytest
import torch

import grammar_ref as R
import logit_adjust_ref as LA
import logprobs_ref as LP
import token_rules_ref as TR
from gpu_util import CHAIN_W, tiny_engine  # noqa: F401
from oracle import prng
from zoomearth_amd import grammar as G
from zoomearth_amd._lib import ZoomEarthError
from zoomearth_amd.config import ModelConfig
from zoomearth_amd.engine import Engine
from zoomearth_amd.grammar import TokenAutomaton

pytestmark = pytest.mark.gpu

VOCAB, PAD, EOS = 2048, 2043, (2045, 2043)   # ModelConfig.tiny(), the tiny_engine fixture
STEPS = 12


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def random_automaton(vocab, eos, n_states, n_classes, seed, keep=0.5, eos_only=None):
    """no dead ends; the classes of the EOS ids are out of range on purpose (they are never looked at)"""
    rng = np.random.default_rng(seed)
    tc = rng.integers(0, n_classes, vocab).astype(np.uint16)
    tc[:n_classes] = np.arange(n_classes)                                # every class has a token
    tc[[t for t in eos if t < vocab]] = 65535
    trans = rng.integers(0, n_states, (n_states, n_classes)).astype(np.int16)
    trans[rng.random((n_states, n_classes)) > keep] = -1
    accepting = (np.arange(n_states) % 2).astype(np.uint8)
    for s in range(n_states):
        trans[s, s % n_classes] = (s + 1) % n_states
    if eos_only is not None:
        trans[eos_only, :] = -1
        accepting[eos_only] = 1
    return TokenAutomaton(tc, trans, accepting)


# ---------------------------------------------------------------- 1. the kernels alone against the restatement
def test_kernels_equal_the_restatement():
    cfg = copy.deepcopy(ModelConfig.tiny())
    cfg.eos_token_ids, cfg.pad_token_id = (1001, 17), 17                 # EOS ids inside the 1007 columns of the rows below
    eos = cfg.eos_token_ids
    e = Engine(cfg, device=0, max_seqs=2, max_ctx=64, max_patches=1024, max_tile_side=1024)
    try:
        auto = random_automaton(VOCAB, eos, 7, 9, seed=3, eos_only=3)
        gid = e.grammar_create(auto)
        vocab, ld = 1007, 1024                                           # the last mask word of a row is partial
        g = torch.Generator().manual_seed(5)
        host = (torch.randn((5, ld), generator=g) * 4).float().numpy()
        host[4, ::3] = -np.inf
        host[4, 1::7] = np.nan
        host[:, 5] = -0.0
        states = [-1, 1, 2, 3, 4]     # none | accepting: EOS kept | not accepting: EOS -inf | EOS only | a row that holds -inf and NaN
        assert auto.accepting[1] and not auto.accepting[2] and auto.accepting[3] and not (auto.trans[3] >= 0).any()
        out = torch.full((5, ld), 123.0, dtype=torch.float32, device="cuda")
        e.op_grammar_mask(gid, torch.from_numpy(host).cuda()[:, :vocab], states, out=out[:, :vocab])
        torch.cuda.synchronize()
        full = out.cpu().numpy()
        assert (full[:, vocab:] == 123.0).all()                           # the columns beyond vocab stay untouched
        for r, s in enumerate(states):
            assert same_bits(full[r, :vocab], R.mask_row(host[r, :vocab], auto, s, eos)), (r, s)
        assert same_bits(full[0, :vocab], host[0, :vocab])
        assert np.isfinite(full[1, [1001, 17]]).all() and np.isneginf(full[2, [1001, 17]]).all()
        assert np.isfinite(full[3, :vocab]).sum() == 2                    # EOS only
        assert np.isnan(full[4, :vocab]).any()
        # the build kernel's masks, read back through an all-zero row per state
        zero = torch.zeros((7, VOCAB), dtype=torch.float32, device="cuda")
        got = e.op_grammar_mask(gid, zero, list(range(7))).cpu().numpy()
        for s in range(7):
            assert np.array_equal(got[s] == 0.0, R.allowed(auto, s, eos)), s
        # the advance kernel on every (state, token) pair
        st, tk = np.meshgrid(np.arange(-1, 8), np.arange(VOCAB), indexing="ij")
        nxt = e.op_grammar_advance(gid, st.reshape(-1), tk.reshape(-1)).cpu().numpy().reshape(st.shape)
        want = np.array([[R.advance(auto, int(s), int(t), eos) for t in range(VOCAB)] for s in range(-1, 8)])
        assert np.array_equal(nxt, want) and (want >= 0).sum() > 1000 and (want < 0).sum() > 1000
    finally:
        e.close()


def test_mask_kernel_at_the_real_vocabulary():
    cfg = copy.deepcopy(ModelConfig.tiny())
    cfg.text.vocab_size, cfg.eos_token_ids, cfg.pad_token_id = 151936, (151645, 151643), 151643
    e = Engine(cfg, device=0, max_seqs=1, max_ctx=64, max_patches=1024, max_tile_side=1024)
    try:
        auto = random_automaton(151936, cfg.eos_token_ids, 5, 40, seed=8, keep=0.05)
        gid = e.grammar_create(auto)
        g = torch.Generator().manual_seed(6)
        host = torch.randn((3, 151936), generator=g).float().numpy()
        got = e.op_grammar_mask(gid, torch.from_numpy(host).cuda(), [4, -1, 1]).cpu().numpy()
        for r, s in enumerate([4, -1, 1]):
            assert same_bits(got[r], R.mask_row(host[r], auto, s, cfg.eos_token_ids)), r
        assert np.isneginf(got[0]).mean() > 0.8 and np.isfinite(got[2, [151645, 151643]]).all()
    finally:
        e.close()


# ---------------------------------------------------------------- 2. every step of a chain is masked with its own state
def text_ids(seed, n):
    return prng.uniform_ints(seed, n, 10, 1990).tolist()


def prefill_text(e, seq, ids):
    pos, delta = e.rope_index(ids, [])
    e.seq_reset(seq)
    return e.prefill(seq, ids, None, pos, delta, want_logits=True)


PROMPTS = [text_ids(41, 23), text_ids(42, 9), text_ids(43, 60)]
_GRAMMARS = {}


def grammars(e):
    """two grammars of the shared engine, made once: (id, automaton) each"""
    if id(e) not in _GRAMMARS:
        autos = [random_automaton(VOCAB, EOS, 11, 13, seed=21, keep=0.3), random_automaton(VOCAB, EOS, 6, 5, seed=22, keep=0.6)]
        _GRAMMARS[id(e)] = [(e.grammar_create(a), a) for a in autos]
    return _GRAMMARS[id(e)]


def own_rows(e, path, ids, first, toks):
    """the raw row of every step: the prefill's, then the chain's ids teacher-forced through the same kind of step"""
    raw = [first]
    prefill_text(e, 0, ids)
    for t in range(len(toks) - 1):
        raw.append((e.decode_step(0, toks[t]) if path == "single" else e.decode_batch([0], [toks[t]])[0]).cpu().numpy())
    return raw


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("path", ["single", "batched"])
def test_every_step_is_masked_with_the_chains_own_state(tiny_engine, path, graph):
    e = tiny_engine
    e.fill_synthetic(**CHAIN_W)
    ids = PROMPTS[0]
    gid, auto = grammars(e)[0]
    kw = dict(ignore_eos=True, use_graph=graph)

    def run(extra=None):
        first = prefill_text(e, 0, ids).cpu().numpy()
        e.set_grammar(0, gid, 2)                                         # (not the start state: the setter's state is honoured)
        if extra:
            extra()
        toks = e.generate(0, STEPS, **kw) if path == "single" else e.generate_batch([0], STEPS, **kw)[0]
        return first, toks, e.chain_grammar_state(0)

    first, toks, final = run()
    raw = own_rows(e, path, ids, first, toks)
    state, violated = 2, 0
    for t, row in enumerate(raw):                                        # the first token too
        assert toks[t] == R.argmax_lowest(R.mask_row(row, auto, state, EOS)), (t, toks)
        state, violated = R.chain_advance(auto, state, violated, toks[t], EOS)
    assert final == (state, 0) and violated == 0
    assert any(toks[t] != int(np.argmax(raw[t])) for t in range(STEPS))  # the mask changed the run
    # with a logit bias, min_new_tokens, a ban record and no_repeat_ngram_size: the composed restatement; log-probs stay raw
    bias = {toks[0]: -3.0, toks[1]: float("-inf"), 7: 1.5}
    bad = [[toks[2]], [toks[3], toks[4]]]

    def extra():
        e.seq_set_logit_adjust(0, min_new_tokens=4, logit_bias=bias)
        e.set_token_rules(0, no_repeat_ngram_size=1, bad_words=bad, context=ids)
        e.set_logprobs(0, 0)

    first, toks2, final = run(extra)
    lp = e.chain_logprobs(0)[0]
    raw = own_rows(e, path, ids, first, toks2)
    state, violated = 2, 0
    for t, row in enumerate(raw):
        a = LA.adjust_row(row, bias=bias, eos_ids=EOS, eos_masked=t < 4)
        a = TR.ban_row(a, list(ids) + toks2[:t], len(ids), 1, bad)
        assert toks2[t] == R.argmax_lowest(R.mask_row(a, auto, state, EOS)), (t, toks2)
        state, violated = R.chain_advance(auto, state, violated, toks2[t], EOS)
    assert final == (state, violated) and toks2 != toks and len(set(toks2)) == STEPS
    want = LP.token_logprobs_ref(np.stack(raw), toks2, 0)[0]
    assert np.abs(lp - want).max() < 2e-5                                # (the tolerance of tests/test_gpu_logprobs.py)


# ---------------------------------------------------------------- 3. the text matches
@pytest.fixture(scope="module")
def stack():
    from tiny_tok import make_bpe_tokenizer
    from zoomearth_amd.modeling import ZoomEarthForConditionalGeneration
    from zoomearth_amd.processor import ZoomEarthProcessor
    model = ZoomEarthForConditionalGeneration.from_synthetic(ModelConfig.tiny(), **CHAIN_W, max_seqs=4, max_ctx=2048,
                                                            max_patches=4096, max_tile_side=2048)
    proc = ZoomEarthProcessor(make_bpe_tokenizer(), min_pixels=3136, max_pixels=128 * 128 * 28 * 28)
    proc.tokenizer.padding_side = "left"
    yield model, proc
    model.engine.close()


def viable(pattern, data: bytes) -> bool:
    table, _ = G.byte_automaton(pattern)
    s = 0
    for b in data:
        s = int(table[s, b])
        if s < 0:
            return False
    return True


def test_generated_text_matches_the_pattern(stack):
    model, proc = stack
    tok = proc.tokenizer
    vb = G.token_bytes(tok)
    eos = set(model.config.eos_token_ids)
    pattern = r'w\d{1,3}( "bbox_2d":\[\d{1,3},\d{1,3}\]){1,2}!'
    inp = proc(text=["w3 w6 w9", "w12 which w3 is next to the w6 ?"], return_tensors="pt", padding="longest").to(model.device)
    L = inp["input_ids"].shape[1]
    done = cut = 0
    for budget in (64, 5):
        out = model.generate(**inp, max_new_tokens=budget, guided_regex=pattern, tokenizer=tok)[:, L:].tolist()
        for row in out:
            n = next((i for i, t in enumerate(row) if t in eos), None)
            data = b"".join(vb[t] for t in (row if n is None else row[:n]))
            if n is not None:                                            # finished by EOS: a full match
                assert re.fullmatch(pattern.encode(), data), data
                assert all(t == model.config.pad_token_id for t in row[n + 1:])
                done += 1
            else:                                                        # cut by max_new_tokens: a prefix the automaton has not rejected
                assert len(row) == budget and viable(pattern, data), data
                cut += 1
    assert done >= 1 and cut >= 1, (done, cut)
    choices = ["w3 w6", "w3 w9 w12", '"bbox_2d":[1,2,3,4]']
    one = proc(text=["w3 w6 w9"], return_tensors="pt").to(model.device)
    row = model.generate(**one, max_new_tokens=40, guided_choice=choices, tokenizer=tok)[0, one["input_ids"].shape[1]:].tolist()
    n = next(i for i, t in enumerate(row) if t in eos)
    assert tok.decode(row[:n]) in choices
    with pytest.raises(ValueError, match="exclude"):
        model.generate(**one, max_new_tokens=2, guided_choice=choices, guided_regex="a", tokenizer=tok)
    assert model.engine.chain_grammar_state(0) == (-1, 0)                 # the call's grammar is gone with the call
    for _ in range(17):                                                  # (and its id: 17 calls fit an engine of 16)
        model.generate(**one, max_new_tokens=2, guided_choice=choices, tokenizer=tok)


# ---------------------------------------------------------------- 4. company does not matter
def test_company_does_not_matter_and_one_graph_serves_all(tiny_engine):
    e = tiny_engine
    e.fill_synthetic(**CHAIN_W)
    (g0, a0), (g1, a1) = grammars(e)
    params = e.gen_params(ignore_eos=True)

    def burst(chains, split=None):
        """chains: (slot, prompt, grammar id or None, state, sampled) -> tokens per slot"""
        for slot, w, gid, state, sampled in chains:
            prefill_text(e, slot, PROMPTS[w])
            if gid is not None:
                e.set_grammar(slot, gid, state)
            if sampled:
                e.set_sampling(slot, do_sample=True, temperature=0.9, seed=5)
        slots = [c[0] for c in chains]
        for slot in slots:
            e.chain_begin(slot, params)
        for n in (split or [STEPS - 1]):
            e.decode_burst(slots, n, params)
        return {slot: e.chain_tokens(slot, STEPS) for slot in slots}

    fresh = Engine(ModelConfig.tiny(), device=0, max_seqs=3, max_ctx=1024, max_patches=1024, max_tile_side=1024)
    try:   # an engine on which no grammar was ever created
        fresh.fill_synthetic(**CHAIN_W)
        for slot, w in ((1, 1), (2, 2)):
            prefill_text(fresh, slot, PROMPTS[w])
        fresh.set_sampling(2, do_sample=True, temperature=0.9, seed=5)
        for slot in (1, 2):
            fresh.chain_begin(slot, params)
        fresh.decode_burst([1, 2], STEPS - 1, params)
        never = {slot: fresh.chain_tokens(slot, STEPS) for slot in (1, 2)}
    finally:
        fresh.close()
    alone = burst([(0, 0, g0, 0, False)])[0]
    mixed = burst([(0, 0, g0, 0, False), (1, 1, None, 0, False), (2, 2, None, 0, True)])
    assert mixed[0] == alone and mixed[1] == never[1] and mixed[2] == never[2]
    mixed2 = burst([(1, 0, g0, 0, False), (0, 1, g1, 3, False), (2, 2, g1, 1, True)])     # other slots, other grammars and states
    assert mixed2[1] == alone
    assert burst([(0, 0, g0, 0, False), (1, 1, g1, 3, False), (2, 2, None, 0, True)], split=[4, STEPS - 5])[0] == alone
    assert alone != burst([(0, 0, None, 0, False)])[0]


def test_states_and_ids_do_not_recapture_the_step(tiny_engine):
    """A burst of three chains is captured once; later bursts that differ only in grammar ids and states replay it.  The engine
    does not export its graph count, so the claim is checked on the host clock: capturing and instantiating the step's graph
    takes far longer than enqueueing a replay, and the first burst below captures for certain (no other test uses its penalty,
    which is part of the step's key), so every later burst's enqueue must be faster than the first one's."""
    import time
    e = tiny_engine
    e.fill_synthetic(**CHAIN_W)
    (g0, _), (g1, _) = grammars(e)
    params = e.gen_params(ignore_eos=True, repetition_penalty=1.0625)
    took = []
    for ga, sa, gb, sb in ((g0, 0, g1, 0), (g1, 2, g0, 5), (g0, 7, None, 0), (g1, 1, g1, 4)):
        for slot, w in ((0, 0), (1, 1), (2, 2)):
            prefill_text(e, slot, PROMPTS[w])
        e.set_grammar(0, ga, sa)
        if gb is not None:
            e.set_grammar(1, gb, sb)
        e.set_grammar(2, g0, 1)
        for slot in range(3):
            e.chain_begin(slot, params)
        e.sync()
        t0 = time.perf_counter()
        e.decode_burst_begin([0, 1, 2], 3, params)
        took.append(time.perf_counter() - t0)
        e.decode_burst_end([0, 1, 2])
    print("burst enqueue times (s):", [f"{t:.4f}" for t in took])
    assert max(took[1:]) < took[0], took


# ---------------------------------------------------------------- 5. life cycle and errors
def test_life_cycle_and_errors(tiny_engine):
    e = tiny_engine
    e.fill_synthetic(**CHAIN_W)
    ids = PROMPTS[0]
    pos, delta = e.rope_index(ids, [])
    kw = dict(ignore_eos=True)
    prefill_text(e, 0, ids)
    plain = e.generate(0, STEPS, **kw)
    (g0, a0), (g1, a1) = grammars(e)

    def bring(how):
        if how == "reset":
            prefill_text(e, 1, ids)
            return
        if how == "truncate":
            e.seq_truncate(1, len(ids) - 1)
        else:
            e.seq_copy_prefix(1, 0, len(ids) - 1)
        e.prefill(1, ids[-1:], None, pos[:, -1:], delta, want_logits=False)

    prefill_text(e, 0, ids)
    for how in ("reset", "truncate", "copy"):
        prefill_text(e, 1, ids)
        e.set_grammar(1, g0)
        guided = e.generate(1, STEPS, **kw)
        assert guided != plain and e.chain_grammar_state(1)[0] >= 0
        bring(how)
        assert e.chain_grammar_state(1) == (-1, 0), how
        assert e.generate(1, STEPS, **kw) == plain, how                   # the slot's next chain inherits nothing
    # destroy: refused while a chain uses the grammar
    extra = e.grammar_create(a1)
    prefill_text(e, 1, ids)
    e.set_grammar(1, extra)
    with pytest.raises(ZoomEarthError, match="still set"):
        e.grammar_destroy(extra)
    e.set_grammar(1, None)
    assert e.chain_grammar_state(1) == (-1, 0)
    e.grammar_destroy(extra)
    with pytest.raises(ZoomEarthError):
        e.set_grammar(1, extra)                                           # gone
    # a 17th grammar is refused
    made = []
    try:
        with pytest.raises(ZoomEarthError, match="16"):
            for _ in range(17):
                made.append(e.grammar_create(a1))
        assert len(made) == 16 - len(grammars(e))
    finally:
        for g in made:
            e.grammar_destroy(g)
    # malformed tables are refused, the engine and the chain's request unchanged
    prefill_text(e, 1, ids)
    e.set_grammar(1, g0, 4)
    tc, tr, ac = a1.token_class, a1.trans, a1.accepting

    def broken(**kw2):
        f = dict(token_class=tc.copy(), trans=tr.copy(), accepting=ac.copy())
        f.update(kw2)
        return TokenAutomaton(**f)

    bad_class = tc.copy()
    bad_class[100] = tr.shape[1]
    bad_hi, bad_lo, dead = tr.copy(), tr.copy(), tr.copy()
    bad_hi[1, 1], bad_lo[1, 1] = tr.shape[0], -2
    dead[2, :] = -1                                                       # state 2 is not accepting
    assert not ac[2]
    cases = [broken(token_class=bad_class), broken(trans=bad_hi), broken(trans=bad_lo), broken(trans=dead),
             TokenAutomaton(tc, np.zeros((2049, 2), np.int16), np.ones(2049, np.uint8)),
             TokenAutomaton(np.zeros(VOCAB, np.uint16), np.zeros((2, 4097), np.int16), np.ones(2, np.uint8))]
    for k, a in enumerate(cases):
        with pytest.raises(ZoomEarthError) as err:
            e.grammar_create(a)
        assert len(str(err.value)) > 30, k
    for bad in ((1, g0, 11), (1, g0, -1), (1, 16, 0), (1, -2, 0), (3, g0, 0)):
        with pytest.raises(ZoomEarthError):
            e.set_grammar(*bad)
    assert e.chain_grammar_state(1) == (4, 0)
    assert e.grammar_create(a1) == extra and e.grammar_destroy(extra) is None     # the refusals took no id
    # violated: a -inf bias on every id the state allows forces id 0; the state stays
    narrow = random_automaton(VOCAB, EOS, 4, 64, seed=23, keep=0.02)      # a state allows few ids: they fit one bias list
    narrow.trans[2, 0] = -1                                               # id 0 (class 0) is not allowed in state 2
    ok = np.nonzero(R.allowed(narrow, 2, EOS))[0]
    assert not narrow.accepting[2] and 0 < ok.size <= 512 and 0 not in ok
    gn = e.grammar_create(narrow)
    try:
        prefill_text(e, 1, ids)
        e.set_grammar(1, gn, 2)
        e.seq_set_logit_adjust(1, logit_bias={int(t): float("-inf") for t in ok})
        toks = e.generate(1, 3, **kw)
        assert toks == [0, 0, 0] and e.chain_grammar_state(1) == (2, 1)
    finally:
        e.seq_reset(1)
        e.grammar_destroy(gn)


# ---------------------------------------------------------------- 6. the server
def test_server_batches_a_guided_request_with_an_unguided_one(stack):
    from fastapi.testclient import TestClient
    from zoomearth_amd import serve
    model, proc = stack
    srv = serve.ChatServer(model, proc, "ZoomEarth", batch_window_s=0.2)
    special = {str(i): -100 for i in range(2002, 2048) if i not in model.config.eos_token_ids}
    msgs = [{"role": "user", "content": "w3 w6 w9"}]
    plain = {"messages": msgs, "max_tokens": 8, "logit_bias": special}
    choices = ["w3 w6", '"bbox_2d":[1,2,3,4]']
    want_plain = srv.complete(plain)["choices"][0]["message"]["content"]
    try:
        futures = [srv.submit({"messages": msgs, "max_tokens": 40, "guided_choice": choices}), srv.submit(plain)]
        res = [f.result(timeout=120) for f in futures]
        assert res[0]["choices"][0]["message"]["content"] in choices and res[0]["choices"][0]["finish_reason"] == "stop"
        assert res[1]["choices"][0]["message"]["content"] == want_plain
        assert srv.scheduler.stats["admitted"] == 2
        client = TestClient(serve.create_app(srv))
        r = client.post("/v1/chat/completions", json={"messages": msgs, "max_tokens": 40, "guided_regex": r"w\d w\d!"})
        assert r.status_code == 200 and re.fullmatch(r"w\d w\d!", r.json()["choices"][0]["message"]["content"])
        for bad in ({"guided_regex": "a*?"}, {"guided_regex": 5}, {"guided_regex": "a", "guided_choice": ["a"]}, {"guided_choice": "a"}):
            r = client.post("/v1/chat/completions", json={"messages": msgs, "max_tokens": 4, **bad})
            assert r.status_code == 400 and "guided" in r.json()["error"]["message"], bad
    finally:
        srv.close()

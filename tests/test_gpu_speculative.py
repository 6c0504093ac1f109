"""GPU: speculative decoding by prompt lookup (ze_seq_set_speculation; zoomearth_amd/csrc/ze_spec.hip) -- the drafter and the accept
pass against the restatement (tests/spec_ref.py), the row contract, the exactness of speculative bursts against plain family-0
bursts (ids AND K/V rows), and the exclusions.

No tolerance anywhere: the feature is lossless, so ids are compared by equality and rows by their bit patterns."""
import dataclasses

import numpy as np
import pytest
import torch

import spec_ref as S
from gpu_util import CHAIN_W, tiny_engine  # noqa: F401
from zoomearth_amd._lib import ZoomEarthError

pytestmark = pytest.mark.gpu

VOCAB, MAX_CTX, K = 2048, 1024, 4   # ModelConfig.tiny(), the tiny_engine fixture
EOS = (2045, 2043)


def bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


@pytest.fixture(scope="module")
def eng(tiny_engine):
    tiny_engine.fill_synthetic(**CHAIN_W)
    assert tiny_engine.set_decode_regime(0) == 0
    yield tiny_engine
    tiny_engine.set_decode_regime(-1)
    for s in range(3):
        tiny_engine.seq_reset(s)


def prefill_text(e, seq, ids):
    pos, delta = e.rope_index(ids, [])
    e.seq_reset(seq)
    e.prefill(seq, ids, None, pos, delta, want_logits=False)
    e.mark_seen(seq, ids)


def kv_rows(e, seq, n):
    n_layers = e.config.text.num_hidden_layers
    return [tuple(bits(x) for x in e.op_kv_read(seq, li, 0, n)) for li in range(n_layers)]


def run_chains(e, prompts, n_new, penalty, spec, ignore_eos=False, steps=6, lookup=None):
    """Chains 0 .. of `prompts` through bursts of `steps` steps until each has n_new tokens, finished or ran out of room;
    spec[i] = k of chain i (0: plain); lookup[i]: the ids handed to set_speculation (None: the prompt).  Returns (ids per chain,
    stats per chain)."""
    seqs = list(range(len(prompts)))
    p = e.gen_params(repetition_penalty=penalty, ignore_eos=ignore_eos)
    for s, ids in zip(seqs, prompts):
        prefill_text(e, s, ids)
        if spec[s]:
            e.set_speculation(s, spec[s], ids if lookup is None or lookup[s] is None else lookup[s], 1, 3)
        e.chain_begin(s, p)
    last = None
    for _ in range(n_new + 2):
        ran, ng, fin = e.decode_burst(seqs, min(steps, max(1, n_new - 1)), p)
        if all(n >= n_new or f for n, f in zip(ng, fin)) or ng == last:
            break
        last = ng
    toks = [e.chain_tokens(s) for s in seqs]
    stats = [e.spec_stats(s) for s in seqs]
    return toks, stats


def predicted_stats(lookup, n_prompt, ids, n_new, k=K):
    """What the drafter and the accept pass must have counted for a chain that emitted `ids` (EOS ignored) in bursts of one step until
    it had n_new tokens: the restatement run over the ids themselves."""
    steps = drafted = accepted = 0
    i = 1                                    # tokens emitted so far (the first comes from the prefill's logits)
    while i < n_new:
        ctx = n_prompt + i - 1
        d = S.draft(list(lookup) + ids[:i], k, 1, 3, cap=min(MAX_CTX - 1 - ctx, MAX_CTX - i - 1))
        a = 0
        while a < len(d) and d[a] == ids[i + a]:
            a += 1
        steps, drafted, accepted, i = steps + 1, drafted + len(d), accepted + a, i + a + 1
    return (steps, drafted, accepted), i


# ---------------------------------------------------------------- 1. the drafter alone
def histories():
    rng = np.random.default_rng(3)
    out = []
    for n in (1, 7, 64, 300):
        out.append(rng.integers(0, 5, size=n).tolist())          # five symbols: n-grams repeat
        out.append(rng.integers(0, VOCAB, size=n).tolist())      # (almost) no repeat
    out += [[1, 2, 3, 7, 8, 3, 9, 2, 3], [5, 6, 10, 5, 6, 20, 30, 5, 6], [1, 2, 3, 4], [4, 4], [1, 2, 8, 3, 2], [9] * 40]
    return out


@pytest.mark.parametrize("gmin,gmax", [(1, 3), (2, 2), (1, 8)])
def test_drafter_equals_the_restatement(eng, gmin, gmax):
    hs = histories()
    got = eng.op_spec_draft(hs, K, gmin, gmax)
    for h, g in zip(hs, got):
        assert g == S.draft(h, K, gmin, gmax), (h[-12:], gmin, gmax)
    three = [hs[0], hs[5], hs[6]]                                  # 3 chains of different lengths in one launch
    assert eng.op_spec_draft(three, K, 1, 3) == [S.draft(h, K, 1, 3) for h in three]


# ---------------------------------------------------------------- 2. the accept pass alone
def accept_inputs():
    rng = np.random.default_rng(5)
    n = 6
    host = (rng.standard_normal((n * (K + 1), VOCAB)) * 3).astype(np.float32)
    drafts, want_rows = [], []
    plans = [[1, 1, 1, 1], [0], [1, 1, 0, 1], [], [1, 2, 1], [1, 1, 1, 1]]      # 1: the row picks the draft id; 0: another; 2: EOS
    for c, plan in enumerate(plans):
        d = []
        for j, kind in enumerate(plan):
            tok = EOS[0] if kind == 2 else int(rng.integers(0, 2000))
            d.append(tok)
            host[c * (K + 1) + j, tok if kind else (tok + 1) % 2000] = 40.0
        host[c * (K + 1) + len(plan), 77 + c] = 40.0
        drafts.append(d)
    # chain 5: the penalty flips row 1 -- draft id d0 (emitted by row 0, hence seen) at 40 against id 1999 at 35: 40 / 1.3 < 35
    d5 = drafts[5]
    host[5 * (K + 1) + 1, d5[1]] = 0.0
    d5[1] = d5[0]
    host[5 * (K + 1) + 1, d5[0]] = 40.0
    host[5 * (K + 1) + 1, 1999] = 35.0
    pens = [1.0, 1.3, 1.0, 1.3, 1.0, 1.3]
    room = [K + 1, K + 1, 2, K + 1, K + 1, K + 1]                                # chain 2: the room ends the walk mid-draft
    seen0 = (rng.random((n, VOCAB)) < 0.05).astype(np.uint8)
    seen0[:, 1999] = 0
    # the condition on the inputs: every arg-max the walk can meet is decided (top-2 gap > 0), whatever the seen-set does
    for r in range(n * (K + 1)):
        for sn in (np.zeros(VOCAB, np.uint8), np.ones(VOCAB, np.uint8)):
            v = np.sort(S.penalised(host[r], sn, 1.3))
            assert v[-1] - v[-2] > 0
    want, fins, seen_want = [], [], seen0.copy()
    for c in range(n):
        ids, fin = S.accept(host[c * (K + 1):(c + 1) * (K + 1)][:len(drafts[c]) + 1], drafts[c], seen_want[c], pens[c], EOS, room[c])
        want.append(ids)
        fins.append(fin)
    assert want[5] == [d5[0], 1999] and len(want[2]) == 2 and fins[4] and len(want[4]) == 2 and len(want[0]) == K + 1 and len(want[1]) == 1
    return host, drafts, pens, room, seen0, want, fins, seen_want


def test_accept_equals_the_restatement(eng):
    host, drafts, pens, room, seen0, want, fins, seen_want = accept_inputs()
    seen = torch.from_numpy(seen0.copy()).cuda()
    got, gfin = eng.op_spec_accept(torch.from_numpy(host).cuda(), drafts, K, seen, pens, room)
    assert got == want and gfin == fins
    assert np.array_equal(seen.cpu().numpy() != 0, seen_want != 0)


# ---------------------------------------------------------------- 3. exactness: speculative bursts against plain family-0 bursts
PATTERN = [11, 12, 13, 14, 15, 16, 17]


def repeating(n, shift=0):
    return [PATTERN[(i + shift) % len(PATTERN)] + 100 * shift for i in range(n)]


def exact_case(e, prompt, penalty, n_new=48, lookup_own=False):
    """Greedy speculative generation against plain family-0 bursts of the same chain: the same ids, the same K/V rows, and the
    counters the restatement predicts from those ids.  lookup_own: the lookup text is the prompt followed by the plain run's own ids
    (as a stage-2 prompt holds stage 1's text), so that every draft hits -- a randomly initialised decoder does not continue the
    pattern of its prompt (measured on the tiny config, 40-id prompt of a 7-id pattern, 48 tokens: 4 ids drafted, none accepted)."""
    (ref,), _ = run_chains(e, [prompt], n_new + K + 1, penalty, [0], True)
    ref = ref[:n_new + K + 1]
    assert len(ref) == min(n_new + K + 1, MAX_CTX - len(prompt) + 1)
    n_new = min(n_new, len(ref))
    rows = len(prompt) + n_new - 1
    kv_plain = kv_rows(e, 0, rows)
    lookup = (prompt + ref)[-MAX_CTX:] if lookup_own else prompt      # (the lookup text holds at most max_ctx ids)
    (spec,), (stats,) = run_chains(e, [prompt], n_new, penalty, [K], True, steps=1, lookup=[lookup])
    want, emitted = predicted_stats(lookup, len(prompt), ref + [-1] * (K + 1), n_new)
    print(f"prompt {len(prompt)} penalty {penalty}: {len(spec)} ids, (steps, drafted, accepted) {stats}, predicted {want}")
    assert spec == ref[:len(spec)] and len(spec) == min(emitted, len(ref))
    assert stats == want
    assert e.seq_len(0) >= rows
    for li, (a, b) in enumerate(zip(kv_plain, kv_rows(e, 0, rows))):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f"K/V rows of layer {li} differ"
    return ref, stats


@pytest.mark.parametrize("penalty", [1.0, 1.3])
@pytest.mark.parametrize("lookup_own", [False, True])
def test_exact_on_a_repeating_prompt(eng, penalty, lookup_own):
    ref, (steps, drafted, accepted) = exact_case(eng, repeating(40), penalty, lookup_own=lookup_own)
    if lookup_own:   # a path that silently never speculates fails here
        assert accepted > 0 and steps < 47


@pytest.mark.parametrize("start", [186, 378])
def test_exact_across_the_attention_part_boundaries(eng, start):
    # positions start .. start + 47: accepted drafts straddle key 192 (the part of the 192-key kernel) and key 384 (the pipelined one's)
    ref, (steps, drafted, accepted) = exact_case(eng, repeating(start), 1.0, lookup_own=True)
    assert accepted > 0


def test_a_prompt_without_repeats_never_drafts(eng):
    for seed in range(11, 19):   # a prompt of distinct ids whose first generated ids repeat nothing either (the first such seed)
        prompt = np.random.default_rng(seed).permutation(1900)[:40].tolist()
        (ref,), _ = run_chains(eng, [prompt], 4, 1.0, [0], True)
        if len(set(prompt + ref[:4])) == len(prompt) + 4:
            break
    else:
        pytest.fail("every candidate prompt's continuation repeats an id")
    assert S.draft(prompt, K, 1, 3) == [] and S.draft(prompt + ref[:3], K, 1, 3) == []
    (spec,), ((steps, drafted, accepted),) = run_chains(eng, [prompt], 4, 1.0, [K], True, steps=1)
    assert spec == ref[:4] and (steps, drafted, accepted) == (3, 0, 0)


def test_two_speculating_chains_and_a_plain_one_share_a_burst(eng):
    prompts = [repeating(40), repeating(33, shift=2), repeating(25, shift=4)]
    alone = [run_chains(eng, [p], 40, 1.3, [0], True)[0][0] for p in prompts]
    lookup = [prompts[0] + alone[0], prompts[1] + alone[1][:12], None]     # chain 0 hits throughout, chain 1 for a while
    together, stats = run_chains(eng, prompts, 32, 1.3, [K, 2, 0], True, steps=3, lookup=lookup)
    print("stats", stats)
    for got, want in zip(together, alone):
        m = min(len(got), len(want))     # (a chain whose drafts hit runs ahead of the others within the shared bursts)
        assert m >= 32 and got[:m] == want[:m]
    assert stats[0][2] > 0 and stats[1][2] > 0 and stats[2] == (0, 0, 0)
    assert stats[0][2] != stats[1][2]


def test_a_chain_reaches_max_ctx_mid_draft(eng):
    prompt = repeating(MAX_CTX - 9)
    ref, (steps, drafted, accepted) = exact_case(eng, prompt, 1.0, n_new=48, lookup_own=True)
    assert len(ref) == 10            # max_ctx - len(prompt) + 1: the last token is never fed
    assert accepted > 0 and eng.seq_len(0) == MAX_CTX
    assert eng.chain_tokens(0) == ref


def test_eos_inside_an_accepted_draft():
    # an engine whose EOS id is a token the greedy continuation emits: found with EOS ignored, then honoured
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.engine import Engine
    prompt = repeating(40)
    small = dict(device=0, max_seqs=1, max_ctx=MAX_CTX, max_patches=64, max_tile_side=64)
    e = Engine(ModelConfig.tiny(), **small)
    try:
        e.fill_synthetic(**CHAIN_W)
        e.set_decode_regime(0)
        (free,), _ = run_chains(e, [prompt], 32, 1.0, [0], True)
    finally:
        e.close()
    at = next(i for i in range(6, 32) if free[i] not in free[:i] and free[i] not in EOS)
    e = Engine(dataclasses.replace(ModelConfig.tiny(), eos_token_ids=(int(free[at]), 2043)), **small)
    try:
        e.fill_synthetic(**CHAIN_W)
        e.set_decode_regime(0)
        (plain,), _ = run_chains(e, [prompt], 32, 1.0, [0], False)
        assert plain == free[:at + 1]
        kv_plain = kv_rows(e, 0, len(prompt) + at)
        (spec,), ((steps, drafted, accepted),) = run_chains(e, [prompt], 32, 1.0, [K], False, steps=8, lookup=[prompt + free])
        assert spec == plain and accepted > 0 and steps < at
        assert e.seq_len(0) == len(prompt) + at         # the EOS id stopped the walk: nothing behind it was accepted
        for a, b in zip(kv_plain, kv_rows(e, 0, len(prompt) + at)):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    finally:
        e.close()


# ---------------------------------------------------------------- 4. the row contract
@pytest.mark.parametrize("start", [40, 190, 382])
def test_rows_of_one_chain_equal_single_steps(eng, start):
    prompt, toks = repeating(start), [21, 22, 23]
    prefill_text(eng, 0, prompt)
    singles = [eng.decode_batch([0], [t]).cpu().numpy()[0] for t in toks]
    kv_a = kv_rows(eng, 0, start + 3)
    prefill_text(eng, 0, prompt)
    rows = eng.decode_rows(0, toks).cpu().numpy()
    assert eng.seq_len(0) == start + 3
    for j in range(3):
        assert same_bits(rows[j], singles[j]), f"row {j}"
    for a, b in zip(kv_a, kv_rows(eng, 0, start + 3)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------- 5. exclusions
def test_exclusions_both_ways(eng):
    """Each setter pair refuses with ZE_ERR_INVALID and leaves the state as it was: a refused setter leaves the chain speculating
    (its counters go on from where they were), a refused set_speculation leaves the chain without it."""
    import types
    e = eng
    prompt = repeating(20)
    auto = types.SimpleNamespace(token_class=np.zeros(VOCAB, np.uint16), trans=np.zeros((1, 1), np.int16), accepting=np.ones(1, np.uint8))
    gid = e.grammar_create(auto)
    p = e.gen_params(ignore_eos=True)
    setters = [
        lambda: e.set_sampling(0, True, 0.7, 1, 1.0),
        lambda: e.set_sampling_filter(0, top_k=5),
        lambda: e.seq_set_logit_adjust(0, presence_penalty=0.5),
        lambda: e.set_token_rules(0, no_repeat_ngram_size=3, context=prompt),
        lambda: e.set_logprobs(0, 0),
        lambda: e.set_grammar(0, gid),
    ]
    try:
        (ref,), _ = run_chains(e, [prompt], 8, 1.0, [0], True)
        for setter in setters:
            prefill_text(e, 0, prompt)
            e.set_speculation(0, K, prompt + ref)        # (a lookup text that makes drafts hit)
            e.chain_begin(0, p)
            e.decode_burst([0], 1, p)
            before = e.spec_stats(0)
            assert before[0] == 1
            with pytest.raises(ZoomEarthError) as err:
                setter()
            assert err.value.code == -1
            assert e.spec_stats(0) == before              # the request and its counters are what they were ...
            e.decode_burst([0], 1, p)
            after = e.spec_stats(0)
            assert after[0] == 2 and after[2] > 0         # ... and the chain still speculates
            assert e.chain_tokens(0) == ref[:len(e.chain_tokens(0))]
            prefill_text(e, 0, prompt)                    # (the reset clears the request)
            setter()
            with pytest.raises(ZoomEarthError) as err:
                e.set_speculation(0, K, prompt)
            assert err.value.code == -1
            assert e.spec_stats(0) == (0, 0, 0)
            e.chain_begin(0, p)
            e.decode_burst([0], 2, p)
            assert e.spec_stats(0) == (0, 0, 0) and e.seq_len(0) == len(prompt) + 2    # plain steps: one token each
    finally:
        e.seq_reset(0)
        e.grammar_destroy(gid)
    prefill_text(e, 0, prompt)
    e.set_sampling(0, False, repetition_penalty=1.3)   # greedy with a penalty of its own is what speculation allows
    e.set_speculation(0, K, prompt)
    for bad in [dict(k=9), dict(k=-1), dict(k=2, ngram_min=0), dict(k=2, ngram_min=3, ngram_max=2), dict(k=2, ngram_max=9)]:
        with pytest.raises(ZoomEarthError) as err:
            e.set_speculation(0, bad.pop("k"), prompt, **bad)
        assert err.value.code == -1
    e.set_speculation(0, 0)
    assert e.spec_stats(0) == (0, 0, 0)
    e.seq_reset(0)


def test_a_second_begin_before_the_end_is_refused(eng):
    e, prompt = eng, repeating(20)
    p = e.gen_params(ignore_eos=True)
    prefill_text(e, 0, prompt)
    e.set_speculation(0, K, prompt)
    e.chain_begin(0, p)
    assert e.decode_burst_begin([0], 2, p) == 2
    with pytest.raises(ZoomEarthError) as err:          # the chain's length is the device's to know until the burst is collected
        e.decode_burst_begin([0], 2, p)
    assert err.value.code == -1
    n_gen, _ = e.decode_burst_end([0])
    assert e.seq_len(0) == len(prompt) + n_gen[0] - 1
    assert e.decode_burst_begin([0], 1, p) == 1
    e.decode_burst_end([0])
    e.seq_reset(0)


def test_the_row_streaming_family_refuses(eng):
    prompt = repeating(20)
    prefill_text(eng, 0, prompt)
    assert eng.set_decode_regime(1) == 1
    try:
        with pytest.raises(ZoomEarthError) as err:
            eng.set_speculation(0, K, prompt)
        assert err.value.code == -1
        assert eng.spec_stats(0) == (0, 0, 0)
    finally:
        assert eng.set_decode_regime(0) == 0


# ---------------------------------------------------------------- 6. the Python surface
def test_generate_with_prompt_lookup_equals_generate_on_family_0():
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.modeling import ZoomEarthForConditionalGeneration
    model = ZoomEarthForConditionalGeneration.from_synthetic(ModelConfig.tiny(), **CHAIN_W, max_seqs=2, max_ctx=512, max_patches=64,
                                                             max_tile_side=64)
    e = model.engine
    try:
        with pytest.raises(ValueError):
            model.generate(input_ids=torch.tensor([repeating(40)]), max_new_tokens=4, prompt_lookup_num_tokens=4, do_sample=True)
        for rows, pen in (([repeating(40)], 1.0), ([repeating(40), repeating(40, shift=2)], 1.3)):
            ids = torch.tensor(rows)
            # generate() on family 0: the batched path of the same engine (one row: the burst path itself)
            plain = e_generate_family0(model, rows, 24, pen)
            got = model.generate(input_ids=ids, max_new_tokens=24, prompt_lookup_num_tokens=4, repetition_penalty=pen, ignore_eos=True)
            assert got.shape == (len(rows), 40 + 24)
            assert got[:, 40:].tolist() == plain
            assert all(e.spec_stats(s)[0] > 0 for s in range(len(rows)))     # the call did go through speculative steps
            # a lookup text that holds the answer: fewer steps, the same ids
            for s, row in enumerate(rows):
                prefill_text(e, s, row)
                e.set_speculation(s, 4, row + plain[s])
            again = e.generate_speculative(list(range(len(rows))), 24, repetition_penalty=pen, ignore_eos=True)
            assert again == plain and all(e.spec_stats(s)[2] > 0 and e.spec_stats(s)[0] < 23 for s in range(len(rows)))
    finally:
        e.close()


def e_generate_family0(model, rows, n, pen):
    e = model.engine
    e.set_decode_regime(0)
    for s, row in enumerate(rows):
        prefill_text(e, s, row)
    if len(rows) > 1:
        return e.generate_batch(list(range(len(rows))), n, repetition_penalty=pen, ignore_eos=True)
    return e.generate_speculative([0], n, repetition_penalty=pen, ignore_eos=True)     # (no request set: plain family-0 bursts)


# ---------------------------------------------------------------- 7. the captured step is the eager step; no step leaks into the next
LONG = [repeating(378), repeating(186, shift=2), repeating(25, shift=4)]   # 24 new tokens: chain 0 crosses key 384, chain 1 key 192


def burst_run(e, prompts, spec_k, lookup, n_new, use_graph):
    """generate_speculative over chains 0 .. of `prompts` (spec_k[i] = 0: a plain chain); returns (ids per chain, stats per chain)."""
    seqs = list(range(len(prompts)))
    for s, ids in zip(seqs, prompts):
        prefill_text(e, s, ids)
        if spec_k[s]:
            e.set_speculation(s, spec_k[s], lookup[s], 1, 3)
    toks = e.generate_speculative(seqs, n_new, repetition_penalty=1.3, ignore_eos=True, use_graph=use_graph)
    return toks, [e.spec_stats(s) for s in seqs]


def test_captured_speculative_bursts_equal_eager_ones(eng):
    """Two speculating chains (k = 3) and a plain one through the same bursts, 24 new tokens, once with every step replayed from the
    engine's step cache and once with every step enqueued: the same launches on the same rows, so the ids and the counters are equal.
    The lookup texts hold (part of) the plain continuation, so that drafts are accepted across the part boundaries."""
    plain, _ = burst_run(eng, LONG, [0, 0, 0], None, 24, True)
    lookup = [LONG[0] + plain[0], LONG[1] + plain[1][:14], None]
    captured = burst_run(eng, LONG, [3, 3, 0], lookup, 24, True)
    eager = burst_run(eng, LONG, [3, 3, 0], lookup, 24, False)
    print("stats", captured[1], eager[1])
    assert captured[0] == eager[0] and captured[1] == eager[1]
    assert captured[0] == plain and all(len(t) == 24 for t in plain)
    assert captured[1][0][2] > 0 and captured[1][1][2] > 0 and captured[1][2] == (0, 0, 0)   # a run that never speculated fails here


SHORT = [repeating(40), repeating(33, shift=2), repeating(25, shift=4)]


def step_calls(plain_ids):
    """The kinds of batched step by name, each a function of an engine that prefills its own chains and returns what the call gave."""
    def f32_bits(t):
        return t.cpu().numpy().view(np.uint32)

    def plain(e):
        return burst_run(e, SHORT, [0, 0, 0], None, 9, True)[0]

    def spec(e):
        return burst_run(e, SHORT, [3, 2, 0], [SHORT[0] + plain_ids[0], SHORT[1] + plain_ids[1], None], 9, True)

    def rows(e):
        prefill_text(e, 1, SHORT[1])
        return f32_bits(e.decode_rows(1, [21, 22, 23, 24, 25])).tolist()

    def beam(e):
        prefill_text(e, 0, SHORT[2])
        tokens, scores, indices = e.beam_search([0, 1, 2], 1, 3, 6, num_return_sequences=3, repetition_penalty=1.3, sync_every=2)
        return tokens, scores.view(np.uint32).tolist(), indices

    def decode_batch(e):
        for s, ids in enumerate(SHORT):
            prefill_text(e, s, ids)
        return f32_bits(e.decode_batch([2, 0, 1], [31, 32, 33])).tolist()

    return dict(plain=plain, spec=spec, rows=rows, beam=beam, decode_batch=decode_batch)


def test_no_step_leaks_into_the_next(eng):
    """Every kind of batched step in a row on ONE engine -- a plain captured burst of 3 chains, a speculative burst, decode_rows of 5
    rows, a beam search, decode_batch, the plain burst again -- each against the same call made first on an engine of its own.  A step
    takes its rows from the ze_step_rows it is handed and no engine member changes while it is enqueued (there is no guard that swaps
    the engine's buffers and puts them back), so this holds by construction: a step that read another step's row table, logits,
    partials or tickets fails here."""
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.engine import Engine

    def first_on_a_fresh_engine(call):
        e = Engine(ModelConfig.tiny(), device=0, max_seqs=3, max_ctx=MAX_CTX, max_patches=64, max_tile_side=64)
        try:
            e.fill_synthetic(**CHAIN_W)
            e.set_decode_regime(0)
            return call(e)
        finally:
            e.close()

    plain_ids = first_on_a_fresh_engine(step_calls(None)["plain"])
    calls = step_calls(plain_ids)
    want = {name: first_on_a_fresh_engine(call) for name, call in calls.items() if name != "plain"}
    want["plain"] = plain_ids
    assert want["spec"][1][0][2] > 0 and want["spec"][0][2] == plain_ids[2]      # drafts were accepted; the plain chain is the plain chain
    order = ["plain", "spec", "rows", "beam", "decode_batch", "plain"]
    got = [calls[name](eng) for name in order]
    for name, g in zip(order, got):
        assert g == want[name], name
    assert got[0] == got[-1]

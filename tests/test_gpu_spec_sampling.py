"""GPU: speculative decoding for sampled chains (ze_seq_set_speculation_mode mode 1; zoomearth_amd/csrc/ze_spec.hip) -- the sampled
accept pass against the restatement (tests/spec_sample_ref.py), the exactness of sampled-mode speculative bursts against plain
family-0 bursts with the same values (ids, counters, K/V rows), the exclusions, and generate().

No tolerance anywhere: ids are compared by equality, rows by their bit patterns.  The seen-set is held bit for bit by the unit test;
in the engine tests it is held through the ids under penalty 1.3, which every later draw reads it for."""
import dataclasses
import types

import numpy as np
import pytest
import torch

import spec_sample_ref as R
from gpu_util import CHAIN_W
from test_gpu_speculative import kv_rows, predicted_stats, prefill_text, repeating
from zoomearth_amd._lib import ZoomEarthError

pytestmark = pytest.mark.gpu

VOCAB, MAX_CTX, K = 2048, 1024, 4   # ModelConfig.tiny()
SEED = 77


@pytest.fixture(scope="module")
def eng():
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.engine import Engine
    e = Engine(ModelConfig.tiny(), device=0, max_seqs=4, max_ctx=MAX_CTX, max_patches=64, max_tile_side=64)
    e.fill_synthetic(**CHAIN_W)
    assert e.set_decode_regime(0) == 0
    yield e
    e.close()


# ---------------------------------------------------------------- 1. the sampled accept pass alone
@pytest.mark.parametrize("k", R.KS)
@pytest.mark.parametrize("vocab,ld", R.SHAPES)
def test_sampled_accept_equals_the_restatement(eng, vocab, ld, k):
    u = R.unit_case(vocab, k)
    host = np.zeros((u["logits"].shape[0], ld), dtype=np.float32)
    host[:, :vocab] = u["logits"]
    host[:, vocab:] = 1e30                     # (the padding of a row is never read)
    seen = torch.from_numpy(u["seen0"].copy()).cuda()
    got, fins = eng.op_spec_accept_sampled(torch.from_numpy(host).cuda()[:, :vocab], u["drafts"], k, u["temperature"], u["seed"], u["stream"],
                                           u["index0"], seen=seen, repetition_penalty=u["penalty"], room=u["room"], top_k=u["filt"][0],
                                           top_p=u["filt"][1], min_p=u["filt"][2])
    print(f"vocab {vocab} ld {ld} k {k}: counts {[len(g) for g in got]} (restatement {[len(w) for w in u['want']]}), finished {fins}")
    assert got == u["want"] and fins == u["fins"]
    assert np.array_equal(seen.cpu().numpy() != 0, u["seen_after"] != 0)
    if u["eos"]:   # the same launch with EOS ignored walks past the EOS id
        seen = torch.from_numpy(u["seen0"].copy()).cuda()
        got, fins = eng.op_spec_accept_sampled(torch.from_numpy(host).cuda()[:, :vocab], u["drafts"], k, u["temperature"], u["seed"], u["stream"],
                                               u["index0"], seen=seen, repetition_penalty=u["penalty"], room=u["room"], top_k=u["filt"][0],
                                               top_p=u["filt"][1], min_p=u["filt"][2], ignore_eos=True)
        assert not any(fins) and len(got[3]) > len(u["want"][3]) and got[3][:len(u["want"][3])] == u["want"][3]


# ---------------------------------------------------------------- 2. exactness against plain family-0 bursts
def run_chain(e, prompt, n_new, T, pen, spec_k=0, lookup=None, filt=None, own=True, slot=0, stream=0, steps=6, ignore_eos=True, sampled=True,
              use_graph=True):
    """One chain through bursts of `steps` steps until it has n_new tokens, finished or stopped growing.  own: the request is the
    chain's (set_sampling), else the call's gen_params.  Returns (ids, stats)."""
    prefill_text(e, slot, prompt)
    if own:
        e.set_sampling(slot, T > 0, T if T > 0 else 1.0, SEED, pen)
        p = e.gen_params(ignore_eos=ignore_eos, use_graph=use_graph)
    else:
        p = e.gen_params(repetition_penalty=pen, ignore_eos=ignore_eos, do_sample=T > 0, temperature=T if T > 0 else 1.0, seed=SEED,
                         use_graph=use_graph)
    if filt:
        e.set_sampling_filter(slot, **filt)
    if spec_k:
        e.set_speculation(slot, spec_k, prompt if lookup is None else lookup, 1, 3, sampled=sampled)
    e.chain_begin(slot, p, stream)
    last = None
    for _ in range(n_new + 2):
        ran, ng, fin = e.decode_burst([slot], min(steps, max(1, n_new - 1)), p)
        if ng[0] >= n_new or fin[0] or ng == last:
            break
        last = ng
    return e.chain_tokens(slot), e.spec_stats(slot)


def exact_case(e, prompt, T, pen, n_new=48, lookup_own=True, **kw):
    """Sampled-mode speculative generation against plain family-0 bursts of the same chain with the same values: the same ids, the
    counters the restatement of the drafter predicts from those ids, the same K/V rows."""
    slot = kw.get("slot", 0)
    ref, _ = run_chain(e, prompt, n_new + K + 1, T, pen, **kw)
    ref = ref[:n_new + K + 1]
    assert len(ref) == min(n_new + K + 1, MAX_CTX - len(prompt) + 1)
    n_new = min(n_new, len(ref))
    rows = len(prompt) + n_new - 1
    kv_plain = kv_rows(e, slot, rows)
    lookup = (prompt + ref)[-MAX_CTX:] if lookup_own else prompt
    spec, stats = run_chain(e, prompt, n_new, T, pen, spec_k=K, lookup=lookup, steps=1, **kw)
    want, emitted = predicted_stats(lookup, len(prompt), ref + [-1] * (K + 1), n_new)
    print(f"prompt {len(prompt)} T {T} penalty {pen} {kw}: {len(spec)} ids, (steps, drafted, accepted) {stats}, predicted {want}")
    assert spec == ref[:len(spec)] and len(spec) == min(emitted, len(ref))
    assert stats == want
    assert e.seq_len(slot) >= rows
    for li, (a, b) in enumerate(zip(kv_plain, kv_rows(e, slot, rows))):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f"K/V rows of layer {li} differ"
    return ref, stats


@pytest.mark.parametrize("pen", [1.0, 1.3])
@pytest.mark.parametrize("T", [0.01, 0.7])
def test_exact_with_the_plain_runs_own_continuation(eng, T, pen):
    ref, (steps, drafted, accepted) = exact_case(eng, repeating(40), T, pen)
    assert accepted > 0 and steps < 47          # a run that never hits proves nothing
    if T == 0.7:    # the chain does sample: the greedy chain under the same penalty gives other ids
        greedy, _ = run_chain(eng, repeating(40), 48, 0.0, pen)
        assert greedy[:48] != ref[:48]


def test_exact_under_top_k_and_top_p(eng):
    ref, (steps, drafted, accepted) = exact_case(eng, repeating(40), 0.7, 1.3, filt=dict(top_k=5, top_p=0.9))
    assert accepted > 0 and steps < 47
    free, _ = run_chain(eng, repeating(40), 48, 0.7, 1.3)
    assert free[:48] != ref[:48]                # the filter is in force


def test_exact_with_the_prompt_alone_as_lookup_text(eng):
    exact_case(eng, repeating(40), 0.7, 1.3, lookup_own=False)


@pytest.mark.parametrize("start", [186, 378])
def test_exact_across_the_attention_part_boundaries(eng, start):
    ref, (steps, drafted, accepted) = exact_case(eng, repeating(start), 0.7, 1.0)
    assert accepted > 0


def test_a_chain_reaches_max_ctx_mid_draft(eng):
    prompt = repeating(MAX_CTX - 9)
    ref, (steps, drafted, accepted) = exact_case(eng, prompt, 0.7, 1.3)
    assert len(ref) == 10 and accepted > 0 and eng.seq_len(0) == MAX_CTX
    assert eng.chain_tokens(0) == ref


def test_the_same_chain_in_another_slot(eng):
    a, sa = exact_case(eng, repeating(40), 0.7, 1.3, stream=2)
    b, sb = exact_case(eng, repeating(40), 0.7, 1.3, stream=2, slot=3)
    assert a == b and sa == sb
    c, _ = run_chain(eng, repeating(40), 48, 0.7, 1.3, stream=1)
    assert c[:48] != a[:48]                     # the stream is the chain's, not the slot's


def test_the_per_call_form(eng):
    ref, (steps, drafted, accepted) = exact_case(eng, repeating(40), 0.7, 1.3, own=False)
    own, _ = run_chain(eng, repeating(40), 48, 0.7, 1.3)
    assert accepted > 0 and ref[:48] == own[:48]       # gen_params(do_sample=True, temperature=) and set_sampling: one chain


def test_eos_inside_an_accepted_draft():
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.engine import Engine
    prompt = repeating(40)
    small = dict(device=0, max_seqs=1, max_ctx=MAX_CTX, max_patches=64, max_tile_side=64)
    e = Engine(ModelConfig.tiny(), **small)
    try:
        e.fill_synthetic(**CHAIN_W)
        e.set_decode_regime(0)
        free, _ = run_chain(e, prompt, 32, 0.7, 1.0)
    finally:
        e.close()
    at = next(i for i in range(6, 32) if free[i] not in free[:i] and free[i] not in (2045, 2043))
    e = Engine(dataclasses.replace(ModelConfig.tiny(), eos_token_ids=(int(free[at]), 2043)), **small)
    try:
        e.fill_synthetic(**CHAIN_W)
        e.set_decode_regime(0)
        plain, _ = run_chain(e, prompt, 32, 0.7, 1.0, ignore_eos=False)
        assert plain == free[:at + 1]
        kv_plain = kv_rows(e, 0, len(prompt) + at)
        spec, (steps, drafted, accepted) = run_chain(e, prompt, 32, 0.7, 1.0, spec_k=K, lookup=prompt + free, steps=8, ignore_eos=False)
        assert spec == plain and accepted > 0 and steps < at
        assert e.seq_len(0) == len(prompt) + at         # the EOS id stopped the walk: nothing behind it was accepted
        for a, b in zip(kv_plain, kv_rows(e, 0, len(prompt) + at)):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    finally:
        e.close()


# ---------------------------------------------------------------- 3. the four kinds of chain in one burst, captured and eager
PROMPTS = [repeating(40), repeating(33, shift=2), repeating(25, shift=4), repeating(37, shift=1)]
# slot: (temperature, penalty, speculation k, sampled mode): plain greedy, plain sampled, greedy-mode speculating, sampled-mode speculating
KINDS = [(0.0, 1.3, 0, False), (0.7, 1.1, 0, False), (0.0, 1.3, 3, False), (0.7, 1.3, 4, True)]


def mixed_burst(e, lookups, n_new, use_graph):
    seqs = [0, 1, 2, 3]
    for s in seqs:
        T, pen, k, mode = KINDS[s]
        prefill_text(e, s, PROMPTS[s])
        e.set_sampling(s, T > 0, T if T > 0 else 1.0, SEED + s, pen)
        if k:
            e.set_speculation(s, k, lookups[s], 1, 3, sampled=mode)
    toks = e.generate_speculative(seqs, n_new, ignore_eos=True, use_graph=use_graph, burst=3, sample_streams=[5, 6, 7, 8])
    return toks, [e.spec_stats(s) for s in seqs]


def test_four_kinds_of_chain_share_a_burst_captured_and_eager(eng):
    alone = []
    for s in range(4):
        T, pen, _, _ = KINDS[s]
        prefill_text(eng, s, PROMPTS[s])
        eng.set_sampling(s, T > 0, T if T > 0 else 1.0, SEED + s, pen)
        alone.append(eng.generate_speculative([s], 40, ignore_eos=True, sample_streams=[5 + s])[0])     # solo plain family-0 bursts
    lookups = [None, None, PROMPTS[2] + alone[2], PROMPTS[3] + alone[3]]
    captured = mixed_burst(eng, lookups, 32, True)
    eager = mixed_burst(eng, lookups, 32, False)
    print("stats", captured[1], eager[1])
    assert captured == eager
    for s in range(4):
        assert len(captured[0][s]) == 32 and captured[0][s] == alone[s][:32], f"chain {s}"
    assert captured[1][0] == captured[1][1] == (0, 0, 0) and captured[1][2][2] > 0 and captured[1][3][2] > 0


# ---------------------------------------------------------------- 4. exclusions
def test_mode_1_refuses_what_stays_excluded_both_ways(eng):
    e = eng
    prompt = repeating(20)
    auto = types.SimpleNamespace(token_class=np.zeros(VOCAB, np.uint16), trans=np.zeros((1, 1), np.int16), accepting=np.ones(1, np.uint8))
    gid = e.grammar_create(auto)
    p = e.gen_params(ignore_eos=True, do_sample=True, temperature=0.7, seed=SEED)
    setters = [
        lambda: e.set_entropy_filter(0, typical_p=0.9),
        lambda: e.seq_set_logit_adjust(0, presence_penalty=0.5),
        lambda: e.set_token_rules(0, no_repeat_ngram_size=3, context=prompt),
        lambda: e.set_logprobs(0, 0),
        lambda: e.set_grammar(0, gid),
    ]
    try:
        ref, _ = run_chain(e, prompt, 8, 0.7, 1.0, own=False)
        for setter in setters:
            prefill_text(e, 0, prompt)
            e.set_speculation(0, K, prompt + ref, sampled=True)
            e.chain_begin(0, p)
            e.decode_burst([0], 1, p)
            before = e.spec_stats(0)
            assert before[0] == 1
            with pytest.raises(ZoomEarthError) as err:
                setter()
            assert err.value.code == -1 and e.spec_stats(0) == before
            e.decode_burst([0], 1, p)
            after = e.spec_stats(0)
            assert after[0] == 2 and after[2] > 0                     # the chain still speculates, and still hits
            assert e.chain_tokens(0) == ref[:len(e.chain_tokens(0))]
            prefill_text(e, 0, prompt)
            setter()
            with pytest.raises(ZoomEarthError) as err:
                e.set_speculation(0, K, prompt, sampled=True)
            assert err.value.code == -1 and e.spec_stats(0) == (0, 0, 0)
            e.chain_begin(0, p)
            e.decode_burst([0], 2, p)
            assert e.spec_stats(0) == (0, 0, 0) and e.seq_len(0) == len(prompt) + 2
    finally:
        e.seq_reset(0)
        e.grammar_destroy(gid)
    # what mode 1 allows, in either order
    prefill_text(e, 0, prompt)
    e.set_speculation(0, K, prompt, sampled=True)
    e.set_sampling(0, True, 0.7, 1, 1.3)
    e.set_sampling_filter(0, top_k=5, top_p=0.9)
    prefill_text(e, 0, prompt)
    e.set_sampling(0, True, 0.7, 1, 1.3)
    e.set_sampling_filter(0, top_k=5, top_p=0.9)
    e.set_speculation(0, K, prompt, sampled=True)
    with pytest.raises(ZoomEarthError) as err:                         # a mode that does not exist
        e._check(e.lib.ze_seq_set_speculation_mode(e.h, 0, K, 1, 3, None, 0, 2, e._stream()))
    assert err.value.code == -1
    e.seq_reset(0)


def test_mode_0_refuses_sampling_as_before(eng):
    e, prompt = eng, repeating(20)
    prefill_text(e, 0, prompt)
    e.set_speculation(0, K, prompt)
    for setter in (lambda: e.set_sampling(0, True, 0.7, 1, 1.0), lambda: e.set_sampling_filter(0, top_k=5)):
        with pytest.raises(ZoomEarthError) as err:
            setter()
        assert err.value.code == -1
    with pytest.raises(ZoomEarthError) as err:                         # ... and a burst whose call samples
        e.decode_burst([0], 1, e.gen_params(do_sample=True, temperature=0.7))
    assert err.value.code == -1
    prefill_text(e, 0, prompt)
    e.set_sampling(0, True, 0.7, 1, 1.0)
    with pytest.raises(ZoomEarthError) as err:
        e.set_speculation(0, K, prompt)
    assert err.value.code == -1 and e.spec_stats(0) == (0, 0, 0)
    e.set_speculation(0, K, prompt, sampled=True)                      # the switch is what allows it
    e.seq_reset(0)


def test_the_row_streaming_family_refuses_mode_1(eng):
    prompt = repeating(20)
    prefill_text(eng, 0, prompt)
    assert eng.set_decode_regime(1) == 1
    try:
        with pytest.raises(ZoomEarthError) as err:
            eng.set_speculation(0, K, prompt, sampled=True)
        assert err.value.code == -1 and eng.spec_stats(0) == (0, 0, 0)
    finally:
        assert eng.set_decode_regime(0) == 0


# ---------------------------------------------------------------- 5. generate()
def test_generate_with_prompt_lookup_sampling_equals_sampled_generate_on_family_0():
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.modeling import ZoomEarthForConditionalGeneration
    model = ZoomEarthForConditionalGeneration.from_synthetic(ModelConfig.tiny(), **CHAIN_W, max_seqs=4, max_ctx=512, max_patches=64,
                                                             max_tile_side=64)
    e = model.engine
    kw = dict(do_sample=True, temperature=0.7, seed=SEED, top_k=20, top_p=0.95)
    try:
        for rows, pen in (([repeating(40)], 1.0), ([repeating(40), repeating(40, shift=2)], 1.3)):
            e.set_decode_regime(0)
            for s, row in enumerate(rows):
                prefill_text(e, s, row)
            e._apply_filter(range(len(rows)), 20, 0.95, 0.0)
            plain = e.generate_speculative(list(range(len(rows))), 24, repetition_penalty=pen, ignore_eos=True, do_sample=True, temperature=0.7,
                                           seed=SEED)                 # (no request set: plain family-0 bursts)
            got = model.generate(input_ids=torch.tensor(rows), max_new_tokens=24, prompt_lookup_num_tokens=4, prompt_lookup_sampling=True,
                                 repetition_penalty=pen, ignore_eos=True, **kw)
            assert got.shape == (len(rows), 40 + 24) and got[:, 40:].tolist() == plain
            assert all(e.spec_stats(s)[0] > 0 for s in range(len(rows)))
        with pytest.raises(ValueError):                               # without the keyword: today's refusal
            model.generate(input_ids=torch.tensor([repeating(40)]), max_new_tokens=4, prompt_lookup_num_tokens=4, **kw)
        two = model.generate(input_ids=torch.tensor([repeating(40)]), max_new_tokens=12, prompt_lookup_num_tokens=4, prompt_lookup_sampling=True,
                             num_return_sequences=2, ignore_eos=True, **kw)
        want = model.generate(input_ids=torch.tensor([repeating(40)] * 2), max_new_tokens=12, prompt_lookup_num_tokens=4,
                              prompt_lookup_sampling=True, ignore_eos=True, **kw)
        assert two.shape == (2, 52) and two.tolist() == want.tolist() and two[0].tolist() != two[1].tolist()
    finally:
        e.close()

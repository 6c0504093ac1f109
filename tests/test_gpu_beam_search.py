"""GPU: beam search on the device (zoomearth_amd/csrc/ze_beam.hip) against the float64 restatement tests/beam_ref.py.

Decisions -- tokens, parents, beam indices, finished hypotheses, done words -- are compared with ==, wherever the restatement's step
is DECIDED (every comparison between unequal keys wider than beam_ref.TAU, the margin derived from HF's own fp32 error); scores
within TAU; copied K/V rows bit for bit."""
import numpy as np
import pytest
import torch

import beam_ref as R
from gpu_util import CHAIN_W
from oracle import prng
from zoomearth_amd._lib import ZoomEarthError

pytestmark = pytest.mark.gpu

CTX, SLOTS, V = 256, 80, 2048
EOS = (2045, 2043)


@pytest.fixture(scope="module")
def eng():
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.engine import Engine
    e = Engine(ModelConfig.tiny(), device=0, max_seqs=SLOTS, max_ctx=CTX, max_patches=1024, max_tile_side=1024)
    e.fill_synthetic(**CHAIN_W)
    yield e
    e.close()


def text_ids(seed, n):
    return prng.uniform_ints(seed, n, 10, 1990).tolist()


def prefill_text(e, seq, ids, want_logits=False):
    pos, delta = e.rope_index(ids, [])
    e.seq_reset(seq)
    return e.prefill(seq, ids, None, pos, delta, want_logits=want_logits)


def kv_rows(e, seq, start, n):
    return [torch.cat(e.op_kv_read(seq, layer, start, n)).clone() for layer in range(e.config.text.num_hidden_layers)]


# ---------------------------------------------------------------- a. the step alone, on crafted logits
def base_rows(rng, n, vocab):
    """Well separated rows: a coarse grid of distinct values per row (neighbours 1/32 apart before the softmax), shuffled."""
    x = np.stack([rng.permutation(vocab).astype(np.float32) / 32.0 - 40.0 for _ in range(n)])
    # (a jitter per element: without it every row is a permutation of one grid and sums across rows coincide)
    return (x + rng.uniform(-0.004, 0.004, size=x.shape)).astype(np.float32)


def plant(row, pairs):
    for t, v in pairs:
        row[t] = v


def sc_ranked_eos(rank, B=4):
    """First step, EOS id 2045 at overall rank `rank` (1-based) of the one row that counts; a random step follows."""
    def gen(t, rng, n, vocab):
        x = base_rows(rng, n, vocab)
        if t == 0:
            tops = [30.0 - 0.5 * i for i in range(B + 2)]
            x[:, :] = np.minimum(x, 20.0)
            toks = [100 + 7 * i for i in range(B + 2)]
            for r in range(n):
                plant(x[r], zip(toks, tops))
                x[r, EOS[0]] = tops[rank - 1] + 0.25
        return x
    return dict(B=B, gen=gen, steps=2)


def sc_both_eos(t, rng, n, vocab):
    x = base_rows(rng, n, vocab)
    if t == 0:
        x[:, EOS[0]], x[:, EOS[1]] = 31.0, 30.5
    return x


def sc_one_parent(t, rng, n, vocab):
    x = base_rows(rng, n, vocab)
    if t == 0:   # one token takes nearly all the mass: beam 0 leaves the others far behind ...
        x[:, 77] = 60.0
    if t == 1:   # ... so its children fill the next step
        x[:, :] = np.minimum(x, 10.0)
        for r in range(n):
            plant(x[r], [(200 + r, 12.0), (300 + r, 11.5), (400 + r, 11.0)])
    return x


def sc_identity(t, rng, n, vocab):
    x = base_rows(rng, n, vocab)
    if t == 0:
        for r in range(n):
            plant(x[r], [(10, 25.0), (11, 24.5), (12, 24.0), (13, 23.5)])
    else:   # every beam has one continuation far ahead of all others
        for r in range(n):
            x[r, 500 + 3 * r + t] = 60.0
    return x


def sc_tie(t, rng, n, vocab):
    x = base_rows(rng, n, vocab)
    if t == 0:   # B = 4: three clear winners, then two equal logits at the fourth place -- the lower id wins it
        x[:, :] = np.minimum(x, 20.0)
        for r in range(n):
            plant(x[r], [(900, 30.0), (901, 29.0), (902, 28.0), (1500, 27.0), (640, 27.0)])
    return x


def sc_eos_every_step(t, rng, n, vocab):
    """An EOS id inside the top beams at every step: the finished pool fills, and with length_penalty 2 later (longer) hypotheses
    displace earlier ones"""
    x = base_rows(rng, n, vocab)
    x[:, :] = np.minimum(x, 18.0)
    for r in range(n):
        plant(x[r], [(50 + r, 20.0), (60 + r, 19.8), (70 + r, 19.6), (80 + r, 19.4)])
        x[r, EOS[t % 2]] = 19.9
    return x


def sc_random(t, rng, n, vocab):
    # (a wide grid, 0.37 apart with a jitter: the 3 B + 1 best candidates of a group of 16 beams rarely come within TAU)
    x = np.stack([rng.permutation(vocab) * 0.37 - 700.0 for _ in range(n)])
    x = (x + rng.uniform(-0.05, 0.05, size=x.shape)).astype(np.float32)
    for e in EOS:
        if e < vocab:
            x[:, e] += 8.0 * (rng.random(n) < 0.5)
    return x


SCENARIOS = {
    "eos_rank_1": sc_ranked_eos(1), "eos_rank_B": sc_ranked_eos(4), "eos_rank_B_plus_1": sc_ranked_eos(5),
    "both_eos_in_row": dict(B=4, gen=sc_both_eos, steps=2),
    "one_parent": dict(B=3, gen=sc_one_parent, steps=3),
    "identity_parents": dict(B=4, gen=sc_identity, steps=3),
    "tie_at_Bth": dict(B=4, gen=sc_tie, steps=2),
    "displace_false": dict(B=2, gen=sc_eos_every_step, steps=8, max_new=8, lp=2.0, early=False, until_done=True),
    "displace_true": dict(B=2, gen=sc_eos_every_step, steps=8, max_new=8, lp=2.0, early=True, until_done=True),
    "displace_never": dict(B=2, gen=sc_eos_every_step, steps=8, max_new=8, lp=2.0, early="never", until_done=True),
    "stop_false_lp0": dict(B=3, gen=sc_eos_every_step, steps=8, max_new=8, lp=0.0, early=False, until_done=True),
    "random_B1": dict(B=1, gen=sc_random, steps=4, groups=3, pen=1.3),
    "random_B3_g3": dict(B=3, gen=sc_random, steps=4, groups=3, pen=1.3),
    "random_B16": dict(B=16, gen=sc_random, steps=4, groups=1),
    "random_B16_g3": dict(B=16, gen=sc_random, steps=2, groups=3, pen=1.3),
    "random_vocab_2043": dict(B=4, gen=sc_random, steps=4, groups=3, vocab=2043, ld=2048, pen=1.3),
    "random_ld_wide": dict(B=4, gen=sc_random, steps=4, groups=1, ld=2056),
    "random_ld_odd": dict(B=4, gen=sc_random, steps=3, groups=2, vocab=2043, ld=2045, pen=1.3),   # (ld % 4 != 0: the element-wise row loop)
    "last_step": dict(B=4, gen=sc_random, steps=3, max_new=3, groups=1, until_done=True),
}


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_beam_step_against_the_restatement(eng, name):
    sc = SCENARIOS[name]
    e, B, G = eng, sc["B"], sc.get("groups", 1)
    vocab, ld = sc.get("vocab", V), sc.get("ld", sc.get("vocab", V))
    max_new, lp, early, pen = sc.get("max_new", 12), sc.get("lp", 1.0), sc.get("early", False), sc.get("pen", 1.0)
    n = G * B
    slots = list(range(SLOTS - 1, SLOTS - 1 - n, -1))   # (not the identity: a slot id is not a row number)
    for s in slots:
        e.seq_reset(s)
    rng = np.random.default_rng(sum(map(ord, name)))
    refs = [R.BeamGroup(B, vocab, EOS, max_new, lp, early, pen) for _ in range(G)]
    done_at = None
    for t in range(sc["steps"]):
        x = sc["gen"](t, rng, n, vocab)
        full = np.full((n, ld), 1.0e4, np.float32)   # (columns past vocab: poison, never to be read)
        full[:, :vocab] = x
        want = []
        for g in range(G):
            if refs[g].done:   # (a finished group rides along: nothing of it moves)
                want.append(None)
                continue
            want.append(refs[g].step(x[g * B:(g + 1) * B]))
            assert want[g]["decided"], f"{name}: reference step {t} of group {g} is not decided (margin {want[g]['margin']:.3g})"
        got = e.op_beam_step(slots, G, torch.from_numpy(full).cuda(), t == 0, B, max_new, lp, early, pen, vocab=vocab)
        for g in range(G):
            sl = slice(g * B, (g + 1) * B)
            if want[g] is None:
                assert got["done"][g] == 1 and got["parent"][sl].tolist() == list(range(B)), (name, t, g)
                continue
            assert got["parent"][sl].tolist() == want[g]["parent"], (name, t, g)
            assert got["token"][sl].tolist() == want[g]["token"], (name, t, g)
            assert got["rank"][sl].tolist() == want[g]["rank"], (name, t, g)
            assert bool(got["done"][g]) == want[g]["done"], (name, t, g)
            for a, b in zip(got["score"][sl], want[g]["score"]):
                if b > -1.0e8:
                    assert abs(float(a) - b) <= R.TAU, (name, t, g, float(a), b)
        if all(r.done for r in refs):
            done_at = t
            break
    if sc.get("until_done"):
        assert done_at is not None, f"{name}: the scenario is meant to reach its stopping step"
    fin = e.op_beam_finished(G, B, max_new)
    for g in range(G):
        for r, w in enumerate(refs[g].results(B)):
            i = g * B + r
            assert bool(fin["finished"][i]) == w["finished"], (name, g, r)
            if w["finished"]:
                assert fin["tokens"][i] == w["tokens"] and fin["beam_indices"][i] == [b + g * B for b in w["bidx"]], (name, g, r)
                assert abs(float(fin["scores"][i]) - w["score"]) <= R.TAU, (name, g, r)
    # the generated ids of every slot are its hypothesis' (the reorder moved them with it)
    for g in range(G):
        for j in range(B):
            ids, _ = chain_ids(e, slots[g * B + j], max_new)
            assert ids[:len(refs[g].tokens[j])] == refs[g].tokens[j], (name, g, j)
    if name.startswith("displace"):   # (early_stopping True stops at the step that fills the pool; the others go on and displace)
        assert all(f["finished"] for f in refs[0].fin) and (early is True or refs[0].n > B), "the finished pool was to fill up and be displaced"


def chain_ids(e, slot, cap):
    import ctypes as C
    out = (C.c_int32 * cap)()
    n = C.c_int()
    e._check(e.lib.ze_chain_tokens(e.h, slot, out, cap, C.byref(n), e._stream()))
    return list(out[:n.value]), n.value


# ---------------------------------------------------------------- b. the reorder alone
@pytest.mark.parametrize("row0", [0, 5])
@pytest.mark.parametrize("rows", [0, 1, 7, 33])
def test_kv_reorder_copies_exactly_the_named_rows(eng, rows, row0):
    e, L = eng, 40
    for s in range(6):
        prefill_text(e, s, text_ids(100 + s, L))
    before = [kv_rows(e, s, 0, L) for s in range(6)]
    pairs = [(0, 3), (1, 2), (1, 4), (1, 5)]   # fan-out 1 and 3
    e.op_kv_reorder(pairs, row0, rows)
    after = [kv_rows(e, s, 0, L) for s in range(6)]
    src_of = {d: s for s, d in pairs}
    for s in range(6):
        for layer in range(len(after[s])):
            want = before[s][layer].clone()
            if s in src_of and rows:
                want[:, row0:row0 + rows] = before[src_of[s]][layer][:, row0:row0 + rows]
            assert torch.equal(after[s][layer], want), (s, layer)
    for bad in ([(0, 1), (1, 2)], [(0, 2), (1, 2)]):   # a destination that is also a source; a destination named twice
        with pytest.raises(ZoomEarthError) as err:
            e.op_kv_reorder(bad, row0, max(rows, 1))
        assert err.value.code == -1
    again = [kv_rows(e, s, 0, L) for s in range(6)]
    assert all(torch.equal(a, b) for s in range(6) for a, b in zip(after[s], again[s]))


# ---------------------------------------------------------------- c. end to end, closed loop on the engine's own logits
STEPS, B_E2E = 12, 4
# prompts of different length per case, chosen so that every step of the reference is decided (the test fails where one is not)
PROMPT_SEEDS = {(0, 1.0): (7, 8), (0, 1.3): (7, 8), (1, 1.0): (7, 8), (1, 1.3): (9, 10)}


def reference_run(e, pen, prompts):
    """beam_ref driven by logits that existing entries produce: the hypotheses live in two alternating sets of spare slots; a step
    copies each parent's rows into the other set (ze_seq_copy_prefix) and feeds the chosen ids (ze_decode_batch)."""
    G, B = len(prompts), B_E2E
    sets = [[16 + g * B + j for g in range(G) for j in range(B)], [32 + g * B + j for g in range(G) for j in range(B)]]
    refs = [R.BeamGroup(B, V, EOS, STEPS, 1.0, False, pen, prompt_ids=prompts[g]) for g in range(G)]
    logits = []
    for g in range(G):
        row = prefill_text(e, sets[0][g * B], prompts[g], want_logits=True).cpu().numpy()
        logits.append(np.stack([row] * B))
    trace, cur = [], 0
    for t in range(STEPS):
        outs = [refs[g].step(logits[g]) for g in range(G)]
        trace.append(outs)
        if t == STEPS - 1:
            break
        old, new = sets[cur], sets[1 - cur]
        for g in range(G):
            for j in range(B):
                src = old[g * B + (outs[g]["parent"][j] if t > 0 else 0)]
                e.seq_copy_prefix(new[g * B + j], src, e.seq_len(src))
        toks = [outs[g]["token"][j] for g in range(G) for j in range(B)]
        lg = e.decode_batch(new, toks).cpu().numpy()
        logits = [lg[g * B:(g + 1) * B] for g in range(G)]
        cur = 1 - cur
    return refs, trace, sets[cur]


@pytest.mark.parametrize("pen", [1.0, 1.3])
@pytest.mark.parametrize("regime", [0, 1])
def test_beam_search_end_to_end(eng, regime, pen):
    e, B = eng, B_E2E
    prompts = (text_ids(PROMPT_SEEDS[regime, pen][0], 23), text_ids(PROMPT_SEEDS[regime, pen][1], 31))
    G = len(prompts)
    e.set_decode_regime(regime)
    try:
        refs, trace, shadow = reference_run(e, pen, prompts)
        margins = [min(trace[t][g]["margin"] for g in range(G)) for t in range(STEPS)]
        print("margins per step:", " ".join(f"{m:.2e}" for m in margins), "TAU", R.TAU)
        # every step is compared: the K/V and whole-call comparisons below are never conditional
        assert all(trace[t][g]["decided"] for t in range(STEPS) for g in range(G)), "an undecided reference step: pick other prompt seeds"
        # ---- the device, step by step through the unit entry (the forward of a step is ze_decode_batch on the chains' own tokens)
        slots = list(range(G * B))
        for g in range(G):
            prefill_text(e, slots[g * B], prompts[g])
            if pen != 1.0:
                e.mark_seen(slots[g * B], prompts[g])
            e.seq_fork(slots[g * B], slots[g * B + 1:(g + 1) * B])
        first = torch.stack([prefill_text(e, 15, prompts[g], want_logits=True) for g in range(G) for _ in range(B)])
        moved = False
        for t in range(STEPS):
            lg = first if t == 0 else e.decode_batch(slots)
            got = e.op_beam_step(slots, G, lg, t == 0, B, STEPS, 1.0, False, pen)
            for g in range(G):
                sl, w = slice(g * B, (g + 1) * B), trace[t][g]
                assert got["token"][sl].tolist() == w["token"] and got["parent"][sl].tolist() == w["parent"], (t, g)
                assert got["rank"][sl].tolist() == w["rank"] and bool(got["done"][g]) == w["done"], (t, g)
                moved = moved or w["parent"] != list(range(B))
        assert moved, "no step with a non-identity parent table"
        fin = e.op_beam_finished(G, B, STEPS)
        for g in range(G):
            for r, w in enumerate(refs[g].results(B)):
                assert bool(fin["finished"][g * B + r]) == w["finished"] and fin["tokens"][g * B + r] == w["tokens"], (g, r)
            for j in range(B):
                # (the last step moved the hypotheses once more; the shadow set holds them as they were fed)
                a, b = slots[g * B + j], shadow[g * B + trace[-1][g]["parent"][j]]
                assert e.seq_len(a) == e.seq_len(b) == len(prompts[g]) + STEPS - 1
                for x, y in zip(kv_rows(e, a, 0, e.seq_len(a)), kv_rows(e, b, 0, e.seq_len(b))):
                    assert torch.equal(x, y), (g, j)
        # ---- the whole call
        for g in range(G):
            prefill_text(e, slots[g * B], prompts[g])
            if pen != 1.0:
                e.mark_seen(slots[g * B], prompts[g])
        tokens, scores, indices = e.beam_search(slots, G, B, STEPS, num_return_sequences=B, repetition_penalty=pen, sync_every=3)
        for g in range(G):
            for r, w in enumerate(refs[g].results(B)):
                assert tokens[g][r] == w["tokens"] and indices[g][r] == [b + g * B for b in w["bidx"]], (g, r)
                assert abs(float(scores[g, r]) - w["score"]) <= R.TAU, (g, r, float(scores[g, r]), w["score"])
            for j in range(B):   # afterwards the slots are ordinary chains holding the last running beams
                a, b = slots[g * B + j], shadow[g * B + trace[-1][g]["parent"][j]]
                for x, y in zip(kv_rows(e, a, 0, e.seq_len(a)), kv_rows(e, b, 0, e.seq_len(b))):
                    assert torch.equal(x, y), (g, j)
    finally:
        e.set_decode_regime(-1)


# ---------------------------------------------------------------- d. one beam is greedy decoding
def test_one_beam_is_greedy(eng):
    e, ids = eng, text_ids(21, 19)
    prefill_text(e, 0, ids)
    want = e.generate_batch([0], 12)[0]
    assert len(want) == 12 and not set(want) & set(EOS), "the comparison is for a greedy run without an EOS"
    prefill_text(e, 1, ids)
    tokens, _, _ = e.beam_search([1], 1, 1, 12)
    assert tokens[0][0] == want


# ---------------------------------------------------------------- e. refusals, the model's method, the server
def slot_state(e, slots):
    return [(e.seq_len(s), [r.clone() for r in kv_rows(e, s, 0, max(e.seq_len(s), 1))]) for s in slots]


def same_state(a, b):
    return all(x[0] == y[0] and all(torch.equal(p, q) for p, q in zip(x[1], y[1])) for x, y in zip(a, b))


def test_refusals_change_nothing(eng):
    from types import SimpleNamespace
    e, ids = eng, text_ids(31, 17)
    slots = [0, 1, 2]
    e.set_decode_regime(0)   # (speculation can be requested in family 0 only)
    prefill_text(e, 0, ids)
    prefill_text(e, 1, text_ids(32, 9))   # the other slots of the call hold chains of their own: a refusal leaves them alone
    prefill_text(e, 2, text_ids(33, 11))
    gid = e.grammar_create(SimpleNamespace(token_class=np.zeros(V, np.uint16), trans=np.zeros((1, 1), np.int16), accepting=np.ones(1, np.uint8)))
    setters = {
        "sampling": (lambda: e.set_sampling(0, True, 0.7, 3), lambda: e.set_sampling(0, None)),
        "filter": (lambda: e.set_sampling_filter(0, top_k=5), lambda: e.set_sampling_filter(0)),
        "entropy": (lambda: e.set_entropy_filter(0, typical_p=0.5), lambda: e.set_entropy_filter(0)),
        "logprobs": (lambda: e.set_logprobs(0, 2), lambda: e.set_logprobs(0, None)),
        "adjust": (lambda: e.seq_set_logit_adjust(0, presence_penalty=0.5), lambda: e.seq_set_logit_adjust(0)),
        "rules": (lambda: e.set_token_rules(0, no_repeat_ngram_size=2, context=ids), lambda: e.set_token_rules(0)),
        "grammar": (lambda: e.set_grammar(0, gid), lambda: e.set_grammar(0, None)),
        "speculation": (lambda: e.set_speculation(0, 2, ids), lambda: e.set_speculation(0, 0)),
    }
    try:
        for name, (on, off) in setters.items():
            on()
            before = slot_state(e, slots)
            with pytest.raises(ZoomEarthError) as err:
                e.beam_search(slots, 1, 3, 4)
            assert err.value.code == -1, name
            assert same_state(before, slot_state(e, slots)), name
            off()
        # after every refusal the source is still the prefilled, unstepped chain: the call goes through and equals a fresh one; a
        # second call on the stepped source does not
        tokens, _, _ = e.beam_search(slots, 1, 3, 4, num_return_sequences=3)
        prefill_text(e, 4, ids)
        again, _, _ = e.beam_search([4, 5, 6], 1, 3, 4, num_return_sequences=3)
        assert tokens == again
        before = slot_state(e, slots)
        with pytest.raises(ZoomEarthError) as err:
            e.beam_search(slots, 1, 3, 4)
        assert err.value.code == -1 and same_state(before, slot_state(e, slots))
        # more than 64 rows in family 0: five valid sources, 80 rows -- refused there, served by family 1
        short = text_ids(34, 6)
        for g in range(5):
            prefill_text(e, g * 16, short)
        before = slot_state(e, [0, 16, 32, 48, 64])
        with pytest.raises(ZoomEarthError) as err:
            e.beam_search(list(range(80)), 5, 16, 3)
        assert err.value.code == -1 and same_state(before, slot_state(e, [0, 16, 32, 48, 64]))
        e.set_decode_regime(1)
        wide, _, _ = e.beam_search(list(range(80)), 5, 16, 3)
        assert len(wide) == 5 and all(w == wide[0] for w in wide)   # (five copies of one prompt)
    finally:
        e.set_decode_regime(-1)
        e.grammar_destroy(gid)


@pytest.fixture(scope="module")
def stack():
    from tiny_tok import make_tokenizer
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.modeling import ZoomEarthForConditionalGeneration
    from zoomearth_amd.processor import ZoomEarthProcessor
    model = ZoomEarthForConditionalGeneration.from_synthetic(ModelConfig.tiny(), **CHAIN_W, max_seqs=8, max_ctx=512,
                                                            max_patches=1024, max_tile_side=1024)
    proc = ZoomEarthProcessor(make_tokenizer(), min_pixels=3136, max_pixels=128 * 128 * 28 * 28)
    proc.tokenizer.padding_side = "left"
    yield model, proc
    model.engine.close()


def words(seed, n):
    return " ".join(f"w{int(v)}" for v in prng.uniform_ints(seed, n, 10, 1990))


def test_model_beam_search_is_the_engine_call(stack):
    """model.beam_search on two left-padded rows returns, in generate's shape, what Engine.beam_search -- the call section c holds
    to the reference -- returns for the same ids."""
    model, proc = stack
    e, B, R_, N = model.engine, 4, 3, 10
    inp = proc(text=[words(91, 12), words(92, 7)], return_tensors="pt", padding="longest").to(model.device)
    got = model.beam_search(**inp, num_beams=B, max_new_tokens=N, num_return_sequences=R_, repetition_penalty=1.3, length_penalty=2.0,
                            early_stopping="never", return_dict_in_generate=True, output_scores=True)
    ids_cpu, mask = inp["input_ids"].cpu().numpy(), inp["attention_mask"].cpu().numpy().astype(bool)
    rows = [ids_cpu[b][mask[b]].tolist() for b in range(2)]
    for b in range(2):
        prefill_text(e, b * B, rows[b])
        e.mark_seen(b * B, rows[b])
    tokens, scores, indices = e.beam_search(list(range(2 * B)), 2, B, N, num_return_sequences=R_, repetition_penalty=1.3,
                                            length_penalty=2.0, early_stopping="never")
    width, pad = ids_cpu.shape[1], model.config.pad_token_id
    assert got.sequences.shape[0] == 2 * R_ and torch.equal(got.sequences[:, :width].cpu(), inp["input_ids"].cpu().repeat_interleave(R_, 0))
    for b in range(2):
        for r in range(R_):
            row = got.sequences[b * R_ + r, width:].tolist()
            t = tokens[b][r]
            assert row[:len(t)] == t and all(x == pad for x in row[len(t):]), (b, r)
            bi = got.beam_indices[b * R_ + r].tolist()
            assert bi[:len(t)] == indices[b][r] and all(x == -1 for x in bi[len(t):]), (b, r)
            assert float(got.sequences_scores[b * R_ + r]) == float(scores[b, r])
    plain = model.beam_search(**inp, num_beams=B, max_new_tokens=N, num_return_sequences=R_, repetition_penalty=1.3, length_penalty=2.0,
                              early_stopping="never")
    assert torch.equal(plain, got.sequences)
    with pytest.raises(NotImplementedError):
        model.generate(**inp, max_new_tokens=4, num_beams=2)
    for bad in (dict(num_beams=1), dict(num_beams=2, num_return_sequences=3), dict(num_beams=2, do_sample=True), dict(num_beams=2, top_k=5)):
        with pytest.raises(ValueError):
            model.beam_search(**inp, max_new_tokens=4, **bad)


def test_server_use_beam_search_round_trip(stack):
    from fastapi.testclient import TestClient
    from zoomearth_amd import serve
    model, proc = stack
    client = TestClient(serve.create_app(serve.ChatServer(model, proc, "ZoomEarth")))
    msgs = [{"role": "user", "content": words(93, 12)}]
    body = {"model": "ZoomEarth", "messages": msgs, "max_tokens": 8, "use_beam_search": True, "n": 3, "length_penalty": 0.0,
            "repetition_penalty": 1.3}
    r = client.post("/v1/chat/completions", json=body)
    assert r.status_code == 200, r.text
    res = r.json()
    assert [c["index"] for c in res["choices"]] == [0, 1, 2]
    inp = proc(text=[serve.build_prompt(msgs)[0]], return_tensors="pt").to(model.device)
    want = model.beam_search(**inp, num_beams=3, num_return_sequences=3, max_new_tokens=8, length_penalty=0.0, repetition_penalty=1.3)
    eos = set(model.config.eos_token_ids)
    for c, row in zip(res["choices"], want[:, inp["input_ids"].shape[1]:].tolist()):
        stop = next((i for i, t in enumerate(row) if t in eos), None)
        ids = row if stop is None else row[:stop + 1]
        while stop is None and ids and ids[-1] == model.config.pad_token_id:
            ids = ids[:-1]
        assert c["message"]["content"] == proc.tokenizer.decode(ids, skip_special_tokens=True).strip()
        assert c["finish_reason"] == ("stop" if stop is not None else "length")
    assert len({c["message"]["content"] for c in res["choices"]}) == 3
    # an ordinary request behind it is served as ever
    assert client.post("/v1/chat/completions", json={"model": "ZoomEarth", "messages": msgs, "max_tokens": 4}).status_code == 200
    for bad in ({"temperature": 0.7}, {"logprobs": True}, {"prompt_logprobs": 1}, {"guided_regex": "a+"}, {"guided_choice": ["a", "b"]},
                {"n": 1}, {"use_beam_search": "yes"}, {"length_penalty": "long"}, {"presence_penalty": 0.5}):
        r = client.post("/v1/chat/completions", json={**body, **bad})
        assert r.status_code == 400, (bad, r.text)
    assert client.post("/v1/chat/completions", json={"model": "ZoomEarth", "messages": msgs, "length_penalty": 1.0}).status_code == 400


def test_server_runs_a_beam_request_that_waited_for_running_chains(stack):
    """A beam request that arrives while an ordinary request is decoding waits for that chain to end -- and is then served, with what
    waited behind it, without any further arrival to wake the dispatcher; close() leaves no future unresolved."""
    from zoomearth_amd import serve
    model, proc = stack
    srv = serve.ChatServer(model, proc, "ZoomEarth")
    msgs = [{"role": "user", "content": words(94, 9)}]
    plain = {"model": "ZoomEarth", "messages": msgs, "max_tokens": 24}
    beam = {"model": "ZoomEarth", "messages": msgs, "max_tokens": 6, "use_beam_search": True, "n": 2}
    futures = [srv.submit(plain), srv.submit(beam), srv.submit(plain), srv.submit(beam)]
    srv.close()   # (stop is asked for while all four are pending: the dispatcher finishes them first)
    res = [f.result(timeout=120) for f in futures]
    srv._worker.join(timeout=120)
    assert not srv._worker.is_alive()
    assert [len(r["choices"]) for r in res] == [1, 2, 1, 2]
    assert res[0]["choices"] == res[2]["choices"] and res[1]["choices"] == res[3]["choices"]
    alone = serve.ChatServer(model, proc, "ZoomEarth")
    assert alone.complete(beam)["choices"] == res[1]["choices"] and alone.complete(plain)["choices"] == res[0]["choices"]


# ---------------------------------------------------------------- f. the captured forward of a beam step is the eager one
@pytest.mark.parametrize("regime", [0, 1])
def test_captured_beam_search_equals_eager(eng, regime):
    """2 groups x 3 beams, 8 new tokens, a host check every 3 steps: the call whose forwards replay a captured step (the unsampled
    kind of the engine's one step cache) against the call that enqueues every forward.  The same launches on the same rows, so
    tokens and beam indices are equal and the scores are the same float32 bits -- no tolerance."""
    e, G, B, N = eng, 2, 3, 8
    prompts = (text_ids(31, 23), text_ids(32, 31))
    slots = list(range(G * B))
    e.set_decode_regime(regime)
    try:
        runs = []
        for use_graph in (True, False):
            for g in range(G):
                prefill_text(e, slots[g * B], prompts[g])
                e.mark_seen(slots[g * B], prompts[g])
            runs.append(e.beam_search(slots, G, B, N, num_return_sequences=B, repetition_penalty=1.3, use_graph=use_graph, sync_every=3))
        (tok_c, sc_c, ix_c), (tok_e, sc_e, ix_e) = runs
        assert all(len(t) == N for g in tok_c for t in g), "the comparison is for hypotheses of full length"
        assert tok_c == tok_e and ix_c == ix_e
        assert np.array_equal(sc_c.view(np.uint32), sc_e.view(np.uint32)), (sc_c, sc_e)
    finally:
        e.set_decode_regime(-1)

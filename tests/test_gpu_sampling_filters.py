"""GPU: top-k / top-p / min-p sampling filters through the C ABI -- the selection kernel against the numpy restatement
(tests/sampling_filters_ref.py), filtered draws against the oracle's draw on masked logits, generate / generate_batch /
the scheduler's layers end to end.  Tokens inside a float64 decision margin (1e-5 of the mass for top-p, 1e-4 relative
for min-p) may differ between correct implementations; their number per row is capped (64 at vocab 151,936, 4 at 2,048)."""
import numpy as np
import pytest
import torch

import sampling_filters_ref as R
from gpu_util import CHAIN_W, tiny_engine  # noqa: F401
from oracle import prng
from oracle import qwen25vl as Q

pytestmark = pytest.mark.gpu

GAP = 1e-5


def text_ids(seed, n):
    return prng.uniform_ints(seed, n, 10, 1990).tolist()


def prefill_text(e, seq, ids):
    pos, delta = e.rope_index(ids, [])
    e.seq_reset(seq)
    return e.prefill(seq, ids, None, pos, delta, want_logits=True)


# ---------------------------------------------------------------- 4. the selection kernel alone
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("rows", [1, 3, 130])
@pytest.mark.parametrize("vocab", [2048, 151936])
def test_op_sample_filter_vs_restatement(tiny_engine, vocab, rows, pad):
    e = tiny_engine
    ld = vocab + pad
    host = np.zeros((rows, ld), dtype=np.float32)
    sets = [R.SETTINGS[r % len(R.SETTINGS)] for r in range(rows)]
    for r in range(rows):
        host[r, :vocab] = R.rand_logits(7000 + r, vocab, (3.0, 1.0, 0.3)[r % 3])
    host[:, vocab:] = 1e9   # the padding must never be read
    dev = torch.from_numpy(host).cuda()[:, :vocab]
    T, K, P, M = (np.array([s[i] for s in sets]) for i in range(4))
    cut, kept = e.sample_filter(dev, T, K, P, M)
    cut, kept = cut.cpu().numpy(), kept.cpu().numpy()
    inside = 0
    for r in range(rows):
        t, k, p, m = sets[r]
        want, wcut, wkept = R.filter_ref(host[r, :vocab], t, k, p, m)
        _, near = R.filter_f64(host[r, :vocab], t, k, p, m)
        got = R.scaled(host[r, :vocab], t) >= cut[r]
        only_k = p >= 1.0 and m <= 0.0
        what = f"vocab {vocab} row {r} setting {sets[r]}: cut {cut[r]} (restatement {wcut}), kept {kept[r]} ({wkept})"
        inside += R.assert_same_keep(got, want, near, vocab, only_k, what)
        assert kept[r] == int(got.sum()), what           # out_kept and {z >= out_cut} say the same
        assert got[int(host[r, :vocab].argmax())]
    print(f"vocab {vocab} rows {rows} ld {ld}: {inside} tokens differ from the restatement, all inside the margins")
    # the same rows one launch each: bit-equal cuts (a row's cut does not depend on its company)
    for r in sorted({0, rows // 2, rows - 1}):
        c1, k1 = e.sample_filter(dev[r:r + 1], T[r:r + 1], K[r:r + 1], P[r:r + 1], M[r:r + 1])
        assert c1.cpu().numpy().view(np.uint32)[0] == cut[r:r + 1].view(np.uint32)[0] and int(k1[0]) == kept[r]


def test_op_sample_filter_ties_masked_rows_and_arguments(tiny_engine):
    e = tiny_engine
    vocab = 2048
    lg = R.rand_logits(3, vocab, 2.0)
    order = np.argsort(-lg)
    lg[order[9:14]] = lg[order[9]]
    flat = np.full(vocab, 0.25, dtype=np.float32)
    masked = R.rand_logits(4, vocab, 1.0)
    masked[100:2040] = -np.inf
    allinf = np.full(vocab, -np.inf, dtype=np.float32)
    dev = torch.from_numpy(np.stack([lg, flat, flat, masked, allinf, lg])).cuda()
    cut, kept = e.sample_filter(dev, 1.0, [10, 0, 5, 50, 10, 0], [1.0, 1e-6, 0.3, 0.999, 0.5, 1.0], [0.0, 0.0, 1.0, 0.0, 0.1, 0.0])
    cut, kept = cut.cpu().numpy(), kept.cpu().numpy()
    assert kept[0] == 14 and cut[0] == lg[order[9]]                 # the k-th value repeated: every copy kept
    assert kept[1] == vocab and kept[2] == vocab                    # equal logits: everything, for every top_p
    assert np.isfinite(cut[3]) and kept[3] <= 50 and cut[3] > -np.inf
    assert 1 <= kept[4] <= vocab                                    # nothing finite: memory-safe, some answer
    assert kept[5] == vocab and cut[5] == -np.inf                   # no filter: no cut
    from zoomearth_amd._lib import ZoomEarthError
    for bad in (dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(min_p=-0.1), dict(min_p=1.5)):
        kw = dict(top_k=0, top_p=1.0, min_p=0.0)
        kw.update(bad)
        with pytest.raises(ZoomEarthError):
            e.set_sampling_filter(0, **kw)
        with pytest.raises(ZoomEarthError):
            e.sample_filter(dev[:1], 1.0, kw["top_k"], kw["top_p"], kw["min_p"])


# ---------------------------------------------------------------- 5. filtered draws
@pytest.mark.parametrize("setting", R.SETTINGS)
@pytest.mark.parametrize("penalty", [1.0, 1.3])
def test_filtered_draw_equals_the_oracle_on_masked_logits(tiny_engine, setting, penalty):
    e = tiny_engine
    t, k, p, m = setting
    vocab = e.config.text.vocab_size
    lg = R.rand_logits(17, vocab, 3.0)
    seen = [3, 77, 1500, 219, 1999]
    dl = torch.from_numpy(lg).cuda()
    scores = Q.apply_repetition_penalty(lg, seen, penalty) if penalty != 1.0 else lg
    keep, _, _ = R.filter_ref(scores, t, k, p, m)
    _, near = R.filter_f64(scores, t, k, p, m)
    assert near.sum() <= R.cap_for(vocab)
    # the device's own keep-set may differ from the restatement's on margin tokens only; the draw is checked against the
    # oracle on the DEVICE's keep-set, read back through the unit op on the penalised scores
    cut, kept = e.sample_filter(torch.from_numpy(scores[None]).cuda(), t, k, p, m)
    dkeep = R.scaled(scores, t) >= float(cut[0])
    R.assert_same_keep(dkeep, keep, near, vocab, p >= 1.0 and m <= 0.0, f"setting {setting}")
    masked = R.masked(lg, dkeep)
    gated, n = 0, 300
    e.seq_reset(1)
    e.mark_seen(1, seen)
    e.set_sampling_filter(1, k, p, m)
    for i in range(n):
        want, gap = Q.sample_temperature(masked, seen, penalty, t, seed=4321, slot=0, index=i)
        got = e.sample_temperature(1, dl, t, seed=4321, index=i, repetition_penalty=penalty)
        e.seq_reset(1)   # the op marks its own pick as seen: restore the chain (the reset clears the filter too)
        e.mark_seen(1, seen)
        e.set_sampling_filter(1, k, p, m)
        assert dkeep[got], (i, got)                       # every drawn token lies in the keep-set
        if gap > GAP:
            assert got == want, (i, gap)
        else:
            gated += 1
    e.seq_reset(1)
    assert gated <= n * 0.10


def test_a_vanishing_nucleus_and_min_p_one_give_the_arg_max(tiny_engine):
    e = tiny_engine
    lg = R.rand_logits(5, e.config.text.vocab_size, 3.0)
    dl = torch.from_numpy(lg).cuda()
    for kw in (dict(top_p=1e-6), dict(min_p=1.0), dict(top_k=1)):
        e.seq_reset(0)
        picks = set()
        for i in range(40):
            e.set_sampling_filter(0, **kw)
            picks.add(e.sample_temperature(0, dl, 1.0, seed=i, index=i))
            e.seq_reset(0)
        assert picks == {int(lg.argmax())}, kw


# ---------------------------------------------------------------- 6. generate: graph == eager, replay through the oracle
def test_generate_with_a_filter_replays_through_the_oracle(tiny_engine):
    e = tiny_engine
    e.fill_synthetic(**CHAIN_W)
    ids = text_ids(3, 60)
    k, p, m, T, pen = 40, 0.9, 0.01, 0.8, 1.3
    outs = {}
    for graph in (True, False):
        prefill_text(e, 1, ids)
        e.mark_seen(1, ids)
        outs[graph] = e.generate(1, 24, repetition_penalty=pen, ignore_eos=True, use_graph=graph, do_sample=True,
                                 temperature=T, seed=99, top_k=k, top_p=p, min_p=m)
    assert outs[True] == outs[False] and len(set(outs[True])) > 4
    prefill_text(e, 1, ids)
    e.mark_seen(1, ids)
    plain = e.generate(1, 24, repetition_penalty=pen, ignore_eos=True, do_sample=True, temperature=T, seed=99)
    assert plain != outs[True]                       # the filter changes the sample
    toks, seen, gated = outs[True], list(ids), 0
    lg = prefill_text(e, 1, ids).cpu().numpy()
    for i, tok in enumerate(toks):
        scores = Q.apply_repetition_penalty(lg, seen, pen)
        keep, _, _ = R.filter_ref(scores, T, k, p, m)
        _, near = R.filter_f64(scores, T, k, p, m)
        assert keep[tok] or near[tok], (i, tok)
        want, gap = Q.sample_temperature(R.masked(lg, keep), seen, pen, T, seed=99, slot=0, index=i)
        if gap > GAP and not near.any():
            assert want == tok, (i, gap)
        else:
            gated += 1
        seen.append(tok)
        if i + 1 < len(toks):
            lg = e.decode_step(1, tok).cpu().numpy()
    assert gated <= 4


# ---------------------------------------------------------------- 7. company does not matter
def test_chains_with_different_filters_share_a_batch_and_keep_their_tokens(tiny_engine):
    e = tiny_engine
    e.fill_synthetic(**CHAIN_W)
    prompts = [text_ids(31, 40), text_ids(32, 9), text_ids(33, 77)]
    filters = [dict(top_k=30, top_p=1.0, min_p=0.0), None, dict(top_k=0, top_p=0.8, min_p=0.02)]
    kw = dict(repetition_penalty=1.1, ignore_eos=True, do_sample=True, temperature=0.9, seed=5)

    def run(slots, rows=(0, 1, 2), graph=True):   # prompt rows[i] in chain slot slots[i]
        for s, w in zip(slots, rows):
            prefill_text(e, s, prompts[w])
            if filters[w] is not None:
                e.set_sampling_filter(s, **filters[w])
        return e.generate_batch(slots, 16, use_graph=graph, **kw)

    full = run([0, 1, 2])
    assert run([0, 1, 2]) == full and run([0, 1, 2], graph=False) == full
    assert run([2, 0, 1]) == full and run([1, 2, 0]) == full          # other chain slots, same rows: same sample
    for s, w in zip([0, 1, 2], range(3)):
        prefill_text(e, s, prompts[w])
    plain = e.generate_batch([0, 1, 2], 16, **kw)
    assert plain[1] == full[1]                                          # the chain without a filter: as if nobody had one
    assert plain[0] != full[0] and plain[2] != full[2]
    # each row alone, in the same row's random stream: the burst interface names the stream
    for w in range(3):
        prefill_text(e, 0, prompts[w])
        if filters[w] is not None:
            e.set_sampling_filter(0, **filters[w])
        params = e.gen_params(repetition_penalty=1.1, ignore_eos=True, do_sample=True, temperature=0.9, seed=5)
        e.chain_begin(0, params, w)
        e.decode_burst([0], 15, params)
        assert e.chain_tokens(0) == full[w], w


# ---------------------------------------------------------------- 8. nothing changes without a filter
def test_an_off_filter_and_a_reset_slot_draw_the_unfiltered_tokens(tiny_engine):
    e = tiny_engine
    e.fill_synthetic(**CHAIN_W)
    ids = text_ids(8, 50)
    kw = dict(repetition_penalty=1.2, ignore_eos=True, do_sample=True, temperature=0.9, seed=7)
    prefill_text(e, 2, ids)
    e.mark_seen(2, ids)
    base = e.generate(2, 20, **kw)
    prefill_text(e, 2, ids)
    e.mark_seen(2, ids)
    e.set_sampling_filter(2, 0, 1.0, 0.0)
    assert e.generate(2, 20, **kw) == base
    prefill_text(e, 2, ids)
    e.mark_seen(2, ids)
    filtered = e.generate(2, 20, top_k=3, **kw)
    assert filtered != base
    prefill_text(e, 2, ids)        # the reset inside hands the slot on without the filter
    e.mark_seen(2, ids)
    assert e.generate(2, 20, **kw) == base
    # truncate and a prefix copy into the slot clear it as well: the same steps with and without a filter set beforehand
    pos, delta = e.rope_index(ids, [])

    def via(how, with_filter):
        prefill_text(e, 0, ids)
        prefill_text(e, 1, ids)
        if with_filter:
            e.set_sampling_filter(1, 3, 1.0, 0.0)
        if how == "copy":
            e.seq_copy_prefix(1, 0, len(ids) - 1)
        else:
            e.seq_truncate(1, len(ids) - 1)
        e.prefill(1, ids[-1:], None, pos[:, -1:], delta, want_logits=False)
        e.mark_seen(1, ids)
        return e.generate(1, 20, **kw)

    for how in ("copy", "truncate"):
        assert via(how, True) == via(how, False), how


# ---------------------------------------------------------------- 9. end to end
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


def test_server_honours_top_p_and_rejects_bad_values(stack):
    from fastapi.testclient import TestClient
    from zoomearth_amd import serve
    model, proc = stack
    client = TestClient(serve.create_app(serve.ChatServer(model, proc, "ZoomEarth")))
    # Logits are bf16-rounded, so two tokens can share the top value exactly; the nucleus keeps equal scores together and then
    # draws among them, where greedy takes the lowest index.  The comparison below needs a prompt whose greedy completion never
    # meets such a tie: the first of a few candidates that has none (decided on the greedy logits alone).
    e = model.engine
    msgs = None
    for seed in range(21, 31):
        cand = [{"role": "user", "content": words(seed, 12)}]
        ids = proc(text=[serve.build_prompt(cand)[0]], return_tensors="pt")["input_ids"][0].tolist()
        lg = prefill_text(e, 3, ids).cpu().numpy()
        tie = False
        for _ in range(12):
            top2 = np.partition(lg, -2)[-2:]
            tie |= bool(top2[0] == top2[1])
            lg = e.decode_batch([3], [int(lg.argmax())])[0].cpu().numpy()
        if not tie:
            msgs = cand
            break
    assert msgs is not None, "every candidate prompt meets an exact tie at the top"

    def ask(**kw):
        r = client.post("/v1/chat/completions", json={"model": "ZoomEarth", "messages": msgs, "max_tokens": 12, **kw})
        return r.status_code, r.json()

    code, greedy = ask()
    assert code == 200
    code, nucleus = ask(temperature=1.0, top_p=1e-6, seed=3)
    assert code == 200
    assert nucleus["choices"][0]["message"]["content"] == greedy["choices"][0]["message"]["content"]
    code, free = ask(temperature=1.0, seed=3)
    assert code == 200 and free["choices"][0]["message"]["content"] != greedy["choices"][0]["message"]["content"]
    for bad in (dict(top_p=2), dict(top_k=-5), dict(min_p=3)):
        code, body = ask(temperature=1.0, **bad)
        assert code == 400 and body["error"]["type"] == "invalid_request_error", bad


def test_model_generate_with_top_p_and_top_k_is_reproducible_per_seed(stack):
    model, proc = stack
    inp = proc(text=["<|im_start|> " + words(5, 9) + " <|im_start|>"], return_tensors="pt").to(model.device)
    L = inp["input_ids"].shape[1]
    kw = dict(max_new_tokens=12, do_sample=True, temperature=1.0, top_p=0.9, top_k=50, ignore_eos=True)
    a = model.generate(**inp, seed=1, **kw)[0, L:].tolist()
    assert model.generate(**inp, seed=1, **kw)[0, L:].tolist() == a
    assert model.generate(**inp, seed=2, **kw)[0, L:].tolist() != a
    with pytest.raises(ValueError):
        model.generate(**inp, max_new_tokens=2, do_sample=True, top_p=1.5)


def test_rollout_with_top_k_stays_inside_the_replayed_keep_set():
    from test_gpu_rollout import bbox_tokenizer, word
    from zoomearth_amd import hostloop as H
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.image import DeviceImage
    from zoomearth_amd.modeling import ZoomEarthForConditionalGeneration
    from zoomearth_amd.processor import ZoomEarthProcessor
    from zoomearth_amd.rollout import rollout_two_stage
    model = ZoomEarthForConditionalGeneration.from_synthetic(ModelConfig.tiny(), **CHAIN_W, max_seqs=8, max_ctx=2048,
                                                            max_patches=8192, max_tile_side=2048, max_prefill_rows=8192)
    try:
        e = model.engine
        proc = ZoomEarthProcessor(bbox_tokenizer(), min_pixels=3136, max_pixels=128 * 128 * 28 * 28)
        tile = DeviceImage.from_numpy(prng.synthetic_tile(90, 700, 900), e)
        q = " ".join(word(int(v)) for v in prng.uniform_ints(70, 5, 0, 1999))
        samples = [dict(prompt=H.stage1_prompt(q), image=tile, bbox=[])]
        T, K = 0.9, 50
        ros = rollout_two_stage(model, proc, samples, num_generations=3, temperature=T, max_new_tokens=8, seed=11,
                                with_logps=False, top_k=K)
        assert all(r.error is None for r in ros) and len({tuple(r.completion1_ids) for r in ros}) > 1
        for r in ros:   # replay: teacher-force the chain, the keep-set of every step from the engine's own logits
            inp = proc(text=[r.prompt1], images=list(r.images), return_tensors="pt")
            ids = inp["input_ids"][0].tolist()
            grids = inp["image_grid_thw"].tolist()
            emb = e.vit_forward(inp["pixel_values"].to("cuda"), grids)
            pos, delta = e.rope_index(ids, grids)
            e.seq_reset(0)
            lg = e.prefill(0, ids, emb, pos, delta, want_logits=True).cpu().numpy()
            for i, tok in enumerate(r.completion1_ids):
                keep, _, _ = R.filter_ref(lg, T, top_k=K)
                assert keep[tok], (r.generation, i, tok)
                if i + 1 < len(r.completion1_ids):   # the batched step, as the scheduler ran it (a row does not depend on its batch)
                    lg = e.decode_batch([0], [tok])[0].cpu().numpy()
    finally:
        model.engine.close()

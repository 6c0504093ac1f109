"""GPU: typical-p / epsilon / eta cutoffs through the C ABI -- the band selection (ze_op_sample_band) against the numpy restatement
(tests/entropy_filters_ref.py), draws under a band against the restated draw, chains with different settings in one burst, and
generate / the server end to end.  Tokens inside a float64 decision margin (1e-5 of the mass at the typical target, 1e-4 relative
on s at the typical threshold and on p at the epsilon / eta thresholds, plus the older filters' margins) may differ between correct
implementations; their number per row is capped (64 at vocab 151,936, 4 up to 2,048) -- tests/test_entropy_filters_cpu.py asserts
that the float64 reference alone stays within the cap on every row used here."""
import numpy as np
import pytest
import torch

import entropy_filters_ref as E
from gpu_util import CHAIN_W, tiny_engine  # noqa: F401
from oracle import prng
from oracle import qwen25vl as Q
from zoomearth_amd._lib import ZoomEarthError

pytestmark = pytest.mark.gpu

GAP = 1e-5
_REF = {}


def text_ids(seed, n):
    return prng.uniform_ints(seed, n, 10, 1990).tolist()


def prefill_text(e, seq, ids):
    pos, delta = e.rope_index(ids, [])
    e.seq_reset(seq)
    return e.prefill(seq, ids, None, pos, delta, want_logits=True)


def reference(vocab):
    """[(what, scores, setting, keep, near, cut, ceil, kept)] of one vocabulary, made once: every row with every setting, at the
    real width one setting per row"""
    if vocab not in _REF:
        rows = E.case_rows(vocab)
        pairs = [(r, s) for r in range(len(rows)) for s in range(len(E.SETTINGS))]
        if vocab > 2048:
            pairs = [(s % len(rows), s) for s in range(len(E.SETTINGS))]
        out = []
        for r, s in pairs:
            name, lg = rows[r]
            st = E.SETTINGS[s]
            keep, cut, ceil, kept = E.band_ref(lg, *st)
            out.append((f"vocab {vocab} row '{name}' setting {st}", lg, st, keep, E.band_f64(lg, *st)[1], cut, ceil, kept))
        _REF[vocab] = out
    return _REF[vocab]


# ---------------------------------------------------------------- 1. the selection alone
@pytest.mark.parametrize("vocab", E.VOCABS)
def test_op_sample_band_vs_restatement(tiny_engine, vocab):
    e = tiny_engine
    ref = reference(vocab)
    ld = vocab + (3 if vocab % 4 else 0)
    host = np.full((len(ref), ld), 1e9, dtype=np.float32)   # the padding must never be read
    for i, c in enumerate(ref):
        host[i, :vocab] = c[1]
    dev = torch.from_numpy(host).cuda()[:, :vocab]
    cols = [np.array([c[2][j] for c in ref]) for j in range(7)]
    cut, ceil, kept = (t.cpu().numpy() for t in e.sample_band(dev, *cols))
    inside = 0
    for i, (what, lg, st, keep, near, wcut, wceil, wkept) in enumerate(ref):
        got = E.in_band(lg, st[0], cut[i], ceil[i])
        what += f": band [{cut[i]}, {ceil[i]}] kept {kept[i]} (restatement [{wcut}, {wceil}] {wkept})"
        d = E.assert_same_keep(got, keep, near, vocab, what)
        inside += d
        assert kept[i] == int(got.sum()) >= 1, what            # out_kept and the band say the same
        assert (ceil[i] == np.inf) == (st[4] >= 1.0), what
        if d == 0:
            assert cut[i] == wcut and ceil[i] == wceil and kept[i] == wkept, what
    print(f"vocab {vocab}: {inside} tokens differ from the restatement, all inside the margins")
    # a row's band does not depend on its company
    for i in sorted({0, len(ref) // 2, len(ref) - 1}):
        c1, h1, k1 = e.sample_band(dev[i:i + 1], *[c[i:i + 1] for c in cols])
        assert c1.cpu().numpy().view(np.uint32)[0] == cut[i:i + 1].view(np.uint32)[0]
        assert h1.cpu().numpy().view(np.uint32)[0] == ceil[i:i + 1].view(np.uint32)[0] and int(k1[0]) == kept[i]


def test_op_sample_band_analytic_rows_and_arguments(tiny_engine):
    e = tiny_engine
    vocab = 1000
    peaked = np.zeros(vocab, dtype=np.float32)
    peaked[17] = np.float32(np.log(0.4 / (0.6 / (vocab - 1))))
    flat = np.full(vocab, 0.25, dtype=np.float32)
    uniform = np.full(vocab, -40.0, dtype=np.float32)
    uniform[:64] = 0.0
    allinf = np.full(vocab, -np.inf, dtype=np.float32)
    nan = np.full(vocab, np.nan, dtype=np.float32)
    lg = E.row_for(3, vocab, 1.0)
    dev = torch.from_numpy(np.stack([peaked, lg, flat, flat, uniform, lg, allinf, nan])).cuda()
    cut, ceil, kept = (t.cpu().numpy() for t in e.sample_band(
        dev, 1.0, typical_p=[0.5, 1.0, 0.01, 1.0, 1.0, 1e-6, 0.5, 0.5], epsilon_cutoff=[0.0, 0.0, 0.0, 0.5, 0.0, 0.999, 0.5, 0.5],
        eta_cutoff=[0.0, 0.0, 0.0, 0.0, 0.5, 0.999, 0.5, 0.5]))
    assert (cut[0], ceil[0], kept[0]) == (0.0, 0.0, vocab - 1)             # typical drops the arg-max
    assert (cut[1], ceil[1], kept[1]) == (-np.inf, np.inf, vocab)         # every stage off: no band
    assert kept[2] == vocab and kept[3] == vocab                          # ties live together; nobody reaches eps: the top stays
    assert (cut[4], ceil[4], kept[4]) == (0.0, np.inf, 64)                # eta over 64 uniform tokens: exp(-log 64)
    assert kept[5] == 1                                                    # every stage keeps one token at least
    assert 1 <= kept[6] <= vocab and 1 <= kept[7] <= vocab                 # nothing finite: memory-safe, some answer
    for bad in (dict(typical_p=0.0), dict(typical_p=1.5), dict(epsilon_cutoff=1.0), dict(epsilon_cutoff=-0.1), dict(eta_cutoff=1.0),
                dict(typical_p=float("nan"))):
        with pytest.raises(ZoomEarthError) as err:
            e.set_entropy_filter(0, **bad)
        assert err.value.code == -1
        with pytest.raises(ZoomEarthError):
            e.sample_band(dev[:1], 1.0, **bad)


# ---------------------------------------------------------------- 2. the draw under a band
@pytest.mark.parametrize("penalty", [1.0, 1.3])
@pytest.mark.parametrize("setting", E.SETTINGS)
def test_draw_under_a_band_equals_the_restated_draw(tiny_engine, setting, penalty):
    e = tiny_engine
    vocab, n = 1000, 64
    lg = E.row_for(17, vocab, 2.0)
    seen_ids = [3, 77, 500, 219, 999, int(lg.argmax())]
    scores = Q.apply_repetition_penalty(lg, seen_ids, penalty) if penalty != 1.0 else lg
    cut, ceil, kept = e.sample_band(torch.from_numpy(scores[None]).cuda(), *setting)
    cut, ceil = float(cut[0]), float(ceil[0])
    keep = E.in_band(scores, setting[0], cut, ceil)      # the DEVICE's band (it may differ from the restatement's inside the margins)
    E.assert_same_keep(keep, E.band_ref(scores, *setting)[0], E.band_f64(scores, *setting)[1], vocab, f"setting {setting}")
    rows = torch.from_numpy(np.tile(lg, (n, 1))).cuda()
    seen = np.zeros((n, vocab), dtype=np.uint8)
    seen[:, seen_ids] = 1
    seeds, idx = 4321 + np.arange(n) // 8, np.arange(n) % 8 * 37
    got = e.sample_rows_band(rows, setting[0], cut, ceil, repetition_penalty=penalty, seed=seeds, sample_stream=2, index=idx,
                             seen=torch.from_numpy(seen).cuda()).cpu().numpy()
    gated = 0
    for i in range(n):
        want, gap = E.draw_ref(scores, keep, setting[0], int(seeds[i]), 2, int(idx[i]))
        assert keep[got[i]], (i, got[i])                  # no drawn token lies outside the band
        if gap > GAP:
            assert got[i] == want, (i, gap)
        else:
            gated += 1
    assert gated <= n * 0.10
    # an open band is the plain draw
    plain = e.sample_rows(rows, setting[0], penalty, seeds, 2, idx, seen=torch.from_numpy(seen).cuda()).cpu().numpy()
    assert np.array_equal(e.sample_rows_band(rows, setting[0], -np.inf, np.inf, repetition_penalty=penalty, seed=seeds, sample_stream=2,
                                             index=idx, seen=torch.from_numpy(seen).cuda()).cpu().numpy(), plain)


# ---------------------------------------------------------------- 3. chains
@pytest.fixture(scope="module")
def engine():
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.engine import Engine
    e = Engine(ModelConfig.tiny(), device=0, max_seqs=8, max_ctx=256, max_patches=1024, max_tile_side=1024)
    e.fill_synthetic(**CHAIN_W)
    yield e
    e.close()


PROMPTS = [text_ids(51, 12), text_ids(52, 30), text_ids(53, 7), text_ids(54, 21)]
# per chain: its entropy filter, its older filter, its own sampling request (the call's params are sampled)
ENT = [None, dict(typical_p=0.3), dict(typical_p=0.6, epsilon_cutoff=2e-3, eta_cutoff=4e-3), dict(typical_p=0.2, eta_cutoff=1e-3)]
FILT = [None, None, dict(top_p=0.95), None]
GREEDY = [False, False, False, True]
N_TOK = 14
KW = dict(repetition_penalty=1.1, ignore_eos=True, do_sample=True, temperature=0.9, seed=5)


def setup_chain(e, s, w, entropy=True):
    prefill_text(e, s, PROMPTS[w])
    e.mark_seen(s, PROMPTS[w])
    if GREEDY[w]:
        e.set_sampling(s, do_sample=False, repetition_penalty=1.1)
    if FILT[w]:
        e.set_sampling_filter(s, **FILT[w])
    if ENT[w] and entropy:
        e.set_entropy_filter(s, **ENT[w])


def burst(e, slots, chains, graph=True, entropy=True, streams=None):
    params = e.gen_params(use_graph=graph, **KW)
    for s, w in zip(slots, chains):
        setup_chain(e, s, w, entropy)
    for i, (s, w) in enumerate(zip(slots, chains)):
        e.chain_begin(s, params, w if streams is None else streams[i])
    e.decode_burst(list(slots), N_TOK - 1, params)
    out = [e.chain_tokens(s) for s in slots]
    for s in slots:
        e.seq_reset(s)
    return out


@pytest.mark.parametrize("family", [0, 1])
def test_chains_with_different_settings_share_a_burst(engine, family):
    e = engine
    assert e.set_decode_regime(family) == family
    try:
        alone = [burst(e, [0], [w])[0] for w in range(4)]
        assert all(len(t) == N_TOK for t in alone)
        full = burst(e, [0, 1, 2, 3], [0, 1, 2, 3])
        assert full == alone                                                      # bit for bit the chain run alone
        assert burst(e, [0, 1, 2, 3], [0, 1, 2, 3], graph=False) == full          # captured == eager
        assert burst(e, [5, 2, 7, 0], [0, 1, 2, 3]) == full                       # other slots, the same streams
        # nobody has an entropy filter: the parent's launch sequence.  The chain without one and the greedy chain emit exactly that
        plain = burst(e, [0, 1, 2, 3], [0, 1, 2, 3], entropy=False)
        assert plain[0] == full[0] and plain[3] == full[3]
        assert plain[1] != full[1] and plain[2] != full[2]
    finally:
        e.set_decode_regime(-1)


def test_the_single_chain_call_honours_the_settings(engine):
    """The two batched families round their logits differently (their unfiltered chains part ways after some ten sampled tokens on
    the parent's path too), so ids are compared within a path: each family above, the single-chain call here -- captured against
    eager, the setter against the keywords, the chain without a filter against a call where nobody has one.  The single-chain call
    against the unit ops on its own logits: test_model_generate_with_typical_p_equals_an_engine_level_loop."""
    e = engine
    outs = {}
    for graph in (True, False):
        for w in range(4):
            setup_chain(e, 1, w)
            outs[(graph, w)] = e.generate(1, N_TOK, use_graph=graph, **KW)
    assert all(outs[(True, w)] == outs[(False, w)] and len(outs[(True, w)]) == N_TOK for w in range(4))
    plain = []
    for w in range(4):
        setup_chain(e, 1, w, entropy=False)
        plain.append(e.generate(1, N_TOK, **KW))
    assert plain[0] == outs[(True, 0)] and plain[3] == outs[(True, 3)]           # no filter / greedy: what they always drew
    assert plain[1] != outs[(True, 1)] and plain[2] != outs[(True, 2)]
    for w in (1, 2):   # the settings as keywords, like the older filters
        setup_chain(e, 1, w, entropy=False)
        assert e.generate(1, N_TOK, **KW, **ENT[w]) == outs[(True, w)]
    e.seq_reset(1)


def test_reset_truncate_and_copy_prefix_clear_the_entropy_filter(engine):
    e = engine
    ids = PROMPTS[1]
    pos, delta = e.rope_index(ids, [])

    def via(how, with_filter):
        prefill_text(e, 0, ids)
        prefill_text(e, 1, ids)
        if with_filter:
            e.set_entropy_filter(1, typical_p=0.2)
        if how == "copy":
            e.seq_copy_prefix(1, 0, len(ids) - 1)
        elif how == "truncate":
            e.seq_truncate(1, len(ids) - 1)
        elif how == "off":
            e.set_entropy_filter(1)
            return e.generate(1, 12, **KW)
        e.prefill(1, ids[-1:], None, pos[:, -1:], delta, want_logits=False)
        e.mark_seen(1, ids)
        return e.generate(1, 12, **KW)

    for how in ("copy", "truncate", "off"):
        assert via(how, True) == via(how, False), how
    prefill_text(e, 1, ids)
    e.set_entropy_filter(1, typical_p=0.2)
    kept = e.generate(1, 12, **KW)
    prefill_text(e, 1, ids)                 # the reset inside hands the slot on without the filter
    assert e.generate(1, 12, **KW) != kept
    e.seq_reset(0)
    e.seq_reset(1)


# ---------------------------------------------------------------- 4. exclusions
def test_speculation_and_the_entropy_filter_exclude_each_other(tiny_engine):
    e = tiny_engine
    e.fill_synthetic(**CHAIN_W)
    assert e.set_decode_regime(0) == 0
    prompt = (text_ids(61, 5) * 6)[:24]
    p = e.gen_params(ignore_eos=True)
    try:
        prefill_text(e, 0, prompt)
        e.set_speculation(0, 4, prompt)
        e.chain_begin(0, p)
        e.decode_burst([0], 1, p)
        before = e.spec_stats(0)
        assert before[0] == 1
        with pytest.raises(ZoomEarthError) as err:
            e.set_entropy_filter(0, typical_p=0.5)
        assert err.value.code == -1 and e.spec_stats(0) == before          # the request and its counters are what they were ...
        e.set_entropy_filter(0)                                            # (all off is no filter: accepted)
        e.decode_burst([0], 1, p)
        assert e.spec_stats(0)[0] == 2                                     # ... and the chain still speculates
        # the other way round: the filter stays, speculation does not come
        sampled = dict(repetition_penalty=1.0, ignore_eos=True, do_sample=True, temperature=0.9, seed=3)
        prefill_text(e, 0, prompt)
        e.set_entropy_filter(0, typical_p=0.2, eta_cutoff=1e-3)
        want = e.generate(0, 10, **sampled)
        prefill_text(e, 0, prompt)
        plain = e.generate(0, 10, **sampled)
        assert plain != want
        prefill_text(e, 0, prompt)
        e.set_entropy_filter(0, typical_p=0.2, eta_cutoff=1e-3)
        with pytest.raises(ZoomEarthError) as err:
            e.set_speculation(0, 4, prompt)
        assert err.value.code == -1 and e.spec_stats(0) == (0, 0, 0)
        assert e.generate(0, 10, **sampled) == want                        # the filter is what it was
    finally:
        e.set_decode_regime(-1)
        e.seq_reset(0)


# ---------------------------------------------------------------- 5. end to end
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


def test_model_generate_with_typical_p_equals_an_engine_level_loop(stack):
    model, proc = stack
    e = model.engine
    inp = proc(text=["<|im_start|> " + words(5, 9) + " <|im_start|>"], return_tensors="pt").to(model.device)
    L = inp["input_ids"].shape[1]
    n, T, seed = 12, 1.0, 7
    kw = dict(max_new_tokens=n, do_sample=True, temperature=T, seed=seed, ignore_eos=True, repetition_penalty=1.0)
    got = model.generate(**inp, typical_p=0.3, **kw)[0, L:].tolist()
    assert model.generate(**inp, typical_p=0.3, **kw)[0, L:].tolist() == got
    assert model.generate(**inp, **kw)[0, L:].tolist() != got              # the setting is no longer dropped
    assert model.generate(**inp, typical_p=1.0, **kw)[0, L:].tolist() == model.generate(**inp, **kw)[0, L:].tolist()
    # the same ids from the engine's unit ops: the step's logits, their band, the draw under it
    ids = inp["input_ids"][0].tolist()
    lg = prefill_text(e, 3, ids)
    loop = []
    for i in range(n):
        cut, ceil, _ = e.sample_band(lg[None], T, typical_p=0.3)
        tok = int(e.sample_rows_band(lg[None], T, float(cut[0]), float(ceil[0]), seed=seed, sample_stream=0, index=i)[0])
        loop.append(tok)
        if i + 1 < n:
            lg = e.decode_step(3, tok)
    e.seq_reset(3)
    assert loop == got
    for name in ("typical_p", "epsilon_cutoff", "eta_cutoff"):
        with pytest.raises(ValueError, match=name):
            model.generate(**inp, max_new_tokens=2, do_sample=True, **{name: 1.5})
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
        model.generate(**inp, max_new_tokens=2, prompt_lookup_num_tokens=2, eta_cutoff=1e-3)


def test_server_honours_each_field_and_rejects_bad_values(stack):
    from fastapi.testclient import TestClient
    from zoomearth_amd import serve
    model, proc = stack
    client = TestClient(serve.create_app(serve.ChatServer(model, proc, "ZoomEarth")))
    msgs = [{"role": "user", "content": words(23, 12)}]

    def ask(**kw):
        r = client.post("/v1/chat/completions", json={"model": "ZoomEarth", "messages": msgs, "max_tokens": 12, **kw})
        return r.status_code, r.json()

    code, free = ask(temperature=1.0, seed=3)
    assert code == 200
    # a vanishing typical mass keeps one token per step, the largest cutoffs keep the arg-max alone: three completions that differ from
    # the free one, each reproducible
    for field, value in (("typical_p", 1e-6), ("epsilon_cutoff", 0.999), ("eta_cutoff", 0.999)):
        code, body = ask(temperature=1.0, seed=3, **{field: value})
        assert code == 200, (field, body)
        text = body["choices"][0]["message"]["content"]
        assert text != free["choices"][0]["message"]["content"], field
        assert ask(temperature=1.0, seed=3, **{field: value})[1]["choices"][0]["message"]["content"] == text, field
    for bad in (dict(typical_p=2), dict(typical_p=0), dict(epsilon_cutoff=1), dict(eta_cutoff=-0.5), dict(eta_cutoff="x")):
        code, body = ask(temperature=1.0, **bad)
        assert code == 400 and body["error"]["type"] == "invalid_request_error", bad

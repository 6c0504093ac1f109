"""GPU: per-chain sampling requests (ze_seq_set_sampling / ze_op_sample_rows) -- the per-chain kernels against the numpy restatement of
one row (tests/chain_sampling_ref.py), memory safety on NaN rows, a burst of chains with different requests against each chain's
run alone through the uniform path (bit for bit: tokens by equality), the request's lifetime, the single-chain call, and the
scheduler / server end to end.

Greedy rows are exact.  A sampled row is compared where the reference's CDF gap exceeds GAP = 1e-5 (tests/test_gpu_sampling.py: a
draw closer to a boundary may differ where expf differs in its last bit); such gated draws are counted and capped at 10 % of a
shape's draws (the reference alone gates 0 / 0 / 4 of the 4 / 12 / 208 draws of the three shapes: test_chain_sampling_cpu.py)."""
import numpy as np
import pytest
import torch

import chain_sampling_ref as R
import sampling_filters_ref as F
from gpu_util import CHAIN_W
from oracle import prng
from zoomearth_amd._lib import ZoomEarthError

pytestmark = pytest.mark.gpu

_CASES = {}


@pytest.fixture(scope="module")
def engine():
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.engine import Engine
    e = Engine(ModelConfig.tiny(), device=0, max_seqs=8, max_ctx=256, max_patches=1024, max_tile_side=1024)
    e.fill_synthetic(**CHAIN_W)
    yield e
    e.close()


def text_ids(seed, n):
    return prng.uniform_ints(seed, n, 10, 1990).tolist()


def prefill_text(e, seq, ids):
    pos, delta = e.rope_index(ids, [])
    e.seq_reset(seq)
    return e.prefill(seq, ids, None, pos, delta, want_logits=True)


# ---------------------------------------------------------------- 1. the unit op against the reference
def cases_of(vocab, rows):
    """the rows of one shape and the reference's (token, gap) per row and index, made once"""
    if (vocab, rows) not in _CASES:
        case = [R.case_row(r, vocab) for r in range(rows)]
        want = [[R.sample_row(lg, seen, T, pen, seed, stream, i) for i in R.INDICES] for lg, seen, T, pen, seed, stream in case]
        _CASES[(vocab, rows)] = (case, want)
    return _CASES[(vocab, rows)]


def device_rows(case, vocab, ld):
    rows = len(case)
    host = np.full((rows, ld), 1e9, dtype=np.float32)          # the padding must never be read
    seen = np.zeros((rows, vocab), dtype=np.uint8)
    for r, c in enumerate(case):
        host[r, :vocab] = c[0]
        seen[r, c[1]] = 1
    return torch.from_numpy(host).cuda()[:, :vocab], torch.from_numpy(seen).cuda()


@pytest.mark.parametrize("vocab,ld,rows", R.SHAPES)
def test_op_sample_rows_vs_the_reference(engine, vocab, ld, rows):
    case, want = cases_of(vocab, rows)
    dev, seen = device_rows(case, vocab, ld)
    T, pen, seed, stream = (np.array([c[k] for c in case]) for k in (2, 3, 4, 5))
    draws = gated = 0
    for k, i in enumerate(R.INDICES):
        got = engine.sample_rows(dev, T, pen, seed, stream, i, seen=seen).cpu().numpy()
        for r in range(rows):
            tok, gap = want[r][k]
            if T[r] > 0:
                draws += 1
            if gap > R.GAP:
                assert got[r] == tok, (r, i, T[r], gap)
            else:
                gated += 1
                assert 0 <= got[r] < vocab
    print(f"vocab {vocab} ld {ld} rows {rows}: {gated} of {draws} draws gated")
    assert gated <= 0.10 * draws
    # a row alone gives the same token as the row in company (its own launch, its own tables)
    for r in sorted({0, rows // 2, rows - 1}):
        one = engine.sample_rows(dev[r:r + 1], T[r:r + 1], pen[r:r + 1], seed[r:r + 1], stream[r:r + 1], R.INDICES[1], seen=seen[r:r + 1])
        all_ = engine.sample_rows(dev, T, pen, seed, stream, R.INDICES[1], seen=seen)
        assert int(one[0]) == int(all_[r])
    # without a seen-set the penalty has nothing to act on
    got = engine.sample_rows(dev, 0.0, pen).cpu().numpy()
    assert got.tolist() == [int(c[0].argmax()) for c in case]


def test_op_sample_rows_with_a_filter_per_row(engine):
    vocab, ld, rows = R.SHAPES[2]
    case, _ = cases_of(vocab, rows)
    dev, seen = device_rows(case, vocab, ld)
    T, pen, seed, stream = (np.array([c[k] for c in case]) for k in (2, 3, 4, 5))
    filt = [((5, 1.0, 0.0), (0, 0.9, 0.0), (0, 1.0, 0.0))[r % 3] for r in range(rows)]       # top-k 5 / top-p 0.9 / off
    K, P, M = (np.array([f[k] for f in filt]) for k in range(3))
    # the reference draws on the DEVICE's keep-set (tests/test_gpu_sampling_filters.py: the selection kernel has margins of its own
    # and its own test), read back through the selection op on the penalised scores
    keeps = []
    for r, (lg, sn, t, p, _, _) in enumerate(case):
        sc = R.scores_of(lg, sn, p)
        if t > 0 and filt[r] != (0, 1.0, 0.0):
            cut, _ = engine.sample_filter(torch.from_numpy(sc[None]).cuda(), t, *filt[r])
            keeps.append(F.scaled(sc, t) >= float(cut[0]))
            want_keep, _, _ = F.filter_ref(sc, t, *filt[r])
            _, near = F.filter_f64(sc, t, *filt[r])
            F.assert_same_keep(keeps[-1], want_keep, near, vocab, filt[r][1] >= 1.0, f"row {r}")
        else:
            keeps.append(np.ones(vocab, dtype=bool))
    draws = gated = changed = 0
    for i in R.INDICES:
        got = engine.sample_rows(dev, T, pen, seed, stream, i, seen=seen, top_k=K, top_p=P, min_p=M).cpu().numpy()
        plain = engine.sample_rows(dev, T, pen, seed, stream, i, seen=seen).cpu().numpy()
        for r, (lg, sn, t, p, sd, st) in enumerate(case):
            tok, gap = R.sample_row(F.masked(lg, keeps[r]), sn, t, p, sd, st, i)
            assert keeps[r][got[r]] or t == 0, (r, i)
            if t == 0 or filt[r] == (0, 1.0, 0.0):
                assert got[r] == plain[r], (r, i)                    # greedy rows and rows without a filter: the unfiltered token
            draws += t > 0
            changed += got[r] != plain[r]
            if gap > R.GAP:
                assert got[r] == tok, (r, i, gap)
            else:
                gated += 1
    assert gated <= 0.10 * draws and changed > 10


# ---------------------------------------------------------------- 2. NaN rows
def test_nan_rows_stay_inside_the_vocabulary(engine):
    e = engine
    vocab = e.config.text.vocab_size
    rows = torch.full((2, vocab), float("nan"), dtype=torch.float32, device="cuda")
    got = e.sample_rows(rows, [0.0, 0.8], [1.3, 1.3], [1, 2], seen=torch.ones((2, vocab), dtype=torch.uint8, device="cuda"))
    assert got.tolist() == [0, 0]
    got = e.sample_rows(rows, [0.0, 0.8], 1.0, [1, 2], top_k=[5, 5], top_p=[0.9, 0.9], min_p=[0.0, 0.1])
    assert all(0 <= t < vocab for t in got.tolist())


# ---------------------------------------------------------------- 3. a mixed burst equals the uniform runs
PROMPTS = [text_ids(41, 12), text_ids(42, 30), text_ids(43, 7), text_ids(44, 21), text_ids(45, 16)]
# per chain: its request (None = none) and its filter; the call's params are greedy at penalty 1.0
MIX = [None,
       dict(do_sample=False, repetition_penalty=1.3),
       dict(do_sample=True, temperature=0.8, seed=5),
       dict(do_sample=True, temperature=0.8, seed=6, repetition_penalty=1.1),
       dict(do_sample=True, temperature=0.01, seed=5)]
FILTERS = [None, None, None, dict(top_p=0.9), None]
N_TOK = 16
_ALONE = {}


def alone(e, w, stream):
    """chain w by itself through the uniform path: no request anywhere, its values in the call's gen_params"""
    if (w, stream) not in _ALONE:
        req = MIX[w] or {}
        prefill_text(e, 0, PROMPTS[w])
        e.mark_seen(0, PROMPTS[w])
        if FILTERS[w]:
            e.set_sampling_filter(0, **FILTERS[w])
        params = e.gen_params(repetition_penalty=req.get("repetition_penalty", 1.0), ignore_eos=True, do_sample=req.get("do_sample", False),
                              temperature=req.get("temperature", 1.0), seed=req.get("seed", 0))
        e.chain_begin(0, params, stream)
        e.decode_burst([0], N_TOK - 1, params)
        _ALONE[(w, stream)] = e.chain_tokens(0)
        e.seq_reset(0)
    return _ALONE[(w, stream)]


def mixed(e, slots, graph, streams=None):
    """chain w in slot slots[w], all in one burst under greedy params"""
    streams = streams or list(range(len(slots)))
    params = e.gen_params(repetition_penalty=1.0, ignore_eos=True, use_graph=graph, do_sample=False)
    for w, s in enumerate(slots):
        prefill_text(e, s, PROMPTS[w])
        e.mark_seen(s, PROMPTS[w])
        if MIX[w]:
            e.set_sampling(s, **MIX[w])
        if FILTERS[w]:
            e.set_sampling_filter(s, **FILTERS[w])
    for w, s in enumerate(slots):
        e.chain_begin(s, params, streams[w])
    e.decode_burst(list(slots), N_TOK - 1, params)
    out = [e.chain_tokens(s) for s in slots]
    for s in slots:
        e.seq_reset(s)
    return out


@pytest.mark.parametrize("graph", [True, False])
def test_a_mixed_burst_equals_each_chain_alone(engine, graph):
    e = engine
    want = [alone(e, w, w) for w in range(5)]
    assert all(len(t) == N_TOK for t in want)
    assert want[2] != want[3][:N_TOK] and len({tuple(t) for t in want}) == 5
    assert mixed(e, [0, 1, 2, 3, 4], graph) == want
    assert mixed(e, [6, 3, 0, 7, 2], graph) == want                       # other slots, the same streams: the same tokens


def test_the_requests_change_what_the_chains_draw(engine):
    e = engine
    params = e.gen_params(repetition_penalty=1.0, ignore_eos=True, do_sample=False)
    plain = []
    for w in range(5):
        prefill_text(e, w, PROMPTS[w])
        e.mark_seen(w, PROMPTS[w])
        e.chain_begin(w, params, w)
    e.decode_burst([0, 1, 2, 3, 4], N_TOK - 1, params)
    plain = [e.chain_tokens(w) for w in range(5)]
    want = [alone(e, w, w) for w in range(5)]
    assert plain[0] == want[0] and all(plain[w] != want[w] for w in (2, 3))


# ---------------------------------------------------------------- 4. chains without a request are untouched
def test_chains_without_a_request_are_untouched(engine):
    e = engine
    kw = dict(repetition_penalty=1.1, ignore_eos=True, do_sample=True, temperature=0.9, seed=3)

    def run(with_request):
        for s, w in ((0, 0), (1, 1), (2, 2)):
            prefill_text(e, s, PROMPTS[w])
            e.mark_seen(s, PROMPTS[w])
        if with_request:
            e.set_sampling(2, do_sample=False, repetition_penalty=1.4)
        out = e.generate_batch([0, 1, 2], N_TOK, **kw)
        for s in range(3):
            e.seq_reset(s)
        return out

    plain = run(False)                       # no chain of the engine has a request: the scalar kernels
    got = run(True)
    assert got[0] == plain[0] and got[1] == plain[1] and got[2] != plain[2]
    assert run(False) == plain


# ---------------------------------------------------------------- 5. the request's lifetime
def test_reset_truncate_and_copy_prefix_clear_the_request(engine):
    e = engine
    ids = PROMPTS[1]
    pos, delta = e.rope_index(ids, [])
    kw = dict(repetition_penalty=1.0, ignore_eos=True, do_sample=False)

    def request(slot):
        e.set_sampling(slot, do_sample=True, temperature=1.5, seed=11)

    def run(path, with_request):
        """the tokens of the chain that FOLLOWS `path` in slot 1 under greedy params; the chain before it had a request or not"""
        if path == "copy":
            prefill_text(e, 2, ids)
            prefill_text(e, 1, text_ids(9, 5))
        else:
            prefill_text(e, 1, ids)
        if with_request:
            request(1)
        if path == "reset":
            prefill_text(e, 1, ids)                              # (seq_reset inside)
        elif path == "truncate":
            e.generate(1, 4, **kw)
            e.seq_truncate(1, len(ids) - 1)
            e.prefill(1, ids[-1:], None, pos[:, -1:], delta, want_logits=False)
        elif path == "copy":
            e.seq_copy_prefix(1, 2, len(ids) - 1)
            e.prefill(1, ids[-1:], None, pos[:, -1:], delta, want_logits=False)
        elif path == "clear":
            e.set_sampling(1, None)
        return e.generate(1, 10, **kw)

    prefill_text(e, 1, ids)
    greedy = e.generate(1, 10, **kw)
    assert run("keep", True) != greedy                          # the request holds until something clears it
    for path in ("reset", "truncate", "copy", "clear"):
        assert run(path, True) == run(path, False), path
    assert run("reset", True) == greedy
    e.seq_reset(1)
    e.seq_reset(2)


# ---------------------------------------------------------------- 6. single-chain generate
@pytest.mark.parametrize("graph", [True, False])
def test_generate_follows_the_chains_request(engine, graph):
    e = engine
    ids = PROMPTS[3]
    prefill_text(e, 1, ids)
    e.mark_seen(1, ids)
    want = e.generate(1, 12, repetition_penalty=1.2, ignore_eos=True, use_graph=graph, do_sample=True, temperature=0.8, seed=21)
    prefill_text(e, 1, ids)
    e.mark_seen(1, ids)
    e.set_sampling(1, do_sample=True, temperature=0.8, seed=21, repetition_penalty=1.2)
    assert e.generate(1, 12, repetition_penalty=1.0, ignore_eos=True, use_graph=graph, do_sample=False) == want
    # the other way round: a greedy request under a sampling call, and the graph follows the change of the effective values
    prefill_text(e, 1, ids)
    e.mark_seen(1, ids)
    greedy = e.generate(1, 12, repetition_penalty=1.2, ignore_eos=True, use_graph=graph, do_sample=False)
    prefill_text(e, 1, ids)
    e.mark_seen(1, ids)
    e.set_sampling(1, do_sample=False, repetition_penalty=1.2)
    assert e.generate(1, 12, repetition_penalty=1.0, ignore_eos=True, use_graph=graph, do_sample=True, temperature=0.8, seed=21) == greedy
    assert greedy != want
    e.seq_reset(1)


# ---------------------------------------------------------------- 7. scheduler and server on the real engine
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


def test_one_scheduler_serves_greedy_and_sampled_requests(stack):
    from zoomearth_amd.scheduler import ChainScheduler, Request
    model, proc = stack

    def make():
        return [Request(prompt=words(51, 14), images=[], max_new_tokens=12),
                Request(prompt=words(52, 9), images=[], max_new_tokens=12, do_sample=True, temperature=0.9, seed=5, top_k=50),
                Request(prompt=words(53, 20), images=[], max_new_tokens=12, do_sample=True, temperature=0.9, seed=6,
                        repetition_penalty=1.2)]

    lone = []
    for r in make():
        sched = ChainScheduler(model, proc, do_sample=False, burst=4)
        sched.submit(r)
        sched.run()
        lone.append(list(r.tokens))
    reqs = make()
    sched = ChainScheduler(model, proc, do_sample=False, burst=4)
    for r in reqs:
        sched.submit(r)
    sched.run()
    assert [list(r.tokens) for r in reqs] == lone and sched.stats["admitted"] == 3
    # the sampled requests drew something else than the greedy scheduler would have
    plain = Request(prompt=words(52, 9), images=[], max_new_tokens=12)
    sched = ChainScheduler(model, proc, do_sample=False, burst=4)
    sched.submit(plain)
    sched.run()
    assert list(plain.tokens) != lone[1]
    # a sampling scheduler with the same values draws the same tokens: the request's values ARE the scheduler's for that chain
    same = Request(prompt=words(52, 9), images=[], max_new_tokens=12, top_k=50)
    sched = ChainScheduler(model, proc, do_sample=True, temperature=0.9, seed=5, burst=4)
    sched.submit(same)
    sched.run()
    assert list(same.tokens) == lone[1]


def test_server_answers_a_sampled_request_that_joins_a_greedy_one(stack):
    """The dispatcher's answer to a sampled request that joins a decoding greedy one, against `complete` of the same request on an
    idle server.  `complete` decodes its lone chain with the single-chain (GEMV) kernels, the dispatcher with the batched step:
    two correct paths whose logits agree within bf16 rounding.  An inverse-CDF draw is comparable across them only where the
    target lies farther from a CDF boundary than that rounding moves it.  At T = 0.8 the tiny model's distribution over its 2,048
    tokens is nearly flat (an interval is ~5e-4 of the mass) and the two paths part within a few tokens (measured: equal for 4
    tokens, then neighbouring ids); so that request is compared with its run ALONE ON A SCHEDULER -- the same kernels, bit for
    bit -- and the comparison with `complete` uses the reference's own sampling temperature, 0.01 (src/eval/infer.py:109-115),
    whose intervals are wide (measured on this prompt: complete / lone scheduler / dispatcher agree at T = 0.01 and part at 0.1,
    0.3 and 0.8, the last two always equal to each other)."""
    from zoomearth_amd import serve
    from zoomearth_amd.scheduler import ChainScheduler, Request
    model, proc = stack
    msg = lambda seed, n: [{"role": "user", "content": words(seed, n)}]  # noqa: E731
    long_ = dict(messages=msg(61, 12), max_tokens=48)
    cold = dict(messages=msg(62, 10), max_tokens=10, temperature=0.01, seed=13)
    warm = dict(messages=msg(63, 11), max_tokens=10, temperature=0.8, seed=14, repetition_penalty=1.15)
    idle = serve.ChatServer(model, proc, "ZoomEarth")
    want_long, want_cold = idle.complete(long_), idle.complete(cold)
    lone = Request(prompt=serve.build_prompt(warm["messages"])[0], images=[], max_new_tokens=10)
    sched = ChainScheduler(model, proc, do_sample=True, temperature=0.8, seed=14, repetition_penalty=1.15, burst=8)
    sched.submit(lone)
    sched.run()
    srv = serve.ChatServer(model, proc, "ZoomEarth", batch_window_s=0.0)
    futs = [srv.submit(long_), srv.submit(cold), srv.submit(warm)]
    got_long, got_cold, got_warm = (f.result(timeout=120) for f in futs)
    assert got_cold["choices"] == want_cold["choices"] and got_cold["usage"] == want_cold["usage"]
    assert got_long["choices"] == want_long["choices"]
    assert got_warm["choices"][0]["message"]["content"] == proc.tokenizer.decode(list(lone.tokens), skip_special_tokens=True).strip()
    assert srv.scheduler.stats["admitted"] == 3
    srv.close()


# ---------------------------------------------------------------- 8. invalid arguments
def test_invalid_arguments_leave_the_request_in_force(engine):
    e = engine
    ids = PROMPTS[2]
    kw = dict(repetition_penalty=1.0, ignore_eos=True, do_sample=False)
    prefill_text(e, 1, ids)
    e.set_sampling(1, do_sample=True, temperature=1.2, seed=4)
    want = e.generate(1, 8, **kw)
    prefill_text(e, 1, ids)
    e.set_sampling(1, do_sample=True, temperature=1.2, seed=4)
    nan, inf = float("nan"), float("inf")
    lib, h, st = e.lib, e.h, e._stream()
    for mode in (-2, 2, 7):
        assert lib.ze_seq_set_sampling(h, 1, mode, 1.0, 0, 1.0, st) == -1
    for t in (0.0, -1.0, nan, inf):
        assert lib.ze_seq_set_sampling(h, 1, 1, t, 0, 1.0, st) == -1
        with pytest.raises(ZoomEarthError):
            e.set_sampling(1, do_sample=True, temperature=t)
    for p in (0.0, -1.0, nan, inf):
        for mode in (0, 1):
            assert lib.ze_seq_set_sampling(h, 1, mode, 1.0, 0, p, st) == -1
    with pytest.raises(ZoomEarthError):
        e.set_sampling(8, do_sample=False)                        # no such slot
    assert e.generate(1, 8, **kw) == want                        # the request set before the refused calls still holds
    for bad in (dict(temperature=-1.0), dict(temperature=nan), dict(repetition_penalty=0.0), dict(index=-1)):
        with pytest.raises(ZoomEarthError):
            e.sample_rows(torch.zeros((1, 64), device="cuda"), **{"temperature": 1.0, **bad})
    e.seq_reset(1)

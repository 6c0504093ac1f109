"""GPU: per-chain logit adjustments (ze_seq_set_logit_adjust / ze_op_logit_adjust) -- the kernel against the numpy float32
restatement (tests/logit_adjust_ref.py) bit for bit, the decode path against the logits of its own steps, effects that need no
reference, mixed requests under one graph, the request's lifetime, and the public surfaces end to end.

No tolerance anywhere: the adjustment is elementwise fp32 arithmetic with specified rounding, so rows are compared by their bit
patterns and tokens by equality."""
import numpy as np
import pytest
import torch

import logit_adjust_ref as R
from gpu_util import CHAIN_W, tiny_engine  # noqa: F401
from oracle import prng
from zoomearth_amd._lib import ZoomEarthError

pytestmark = pytest.mark.gpu

EOS_IDS = (2045, 2043)       # ModelConfig.tiny()
NINF = float("-inf")
_ROWS, _MIX = {}, {}


def rows_of(vocab):
    """130 rows of randn x 4 (made once per vocabulary), a few -0 / -inf entries among them"""
    if vocab not in _ROWS:
        g = torch.Generator().manual_seed(2000 + vocab)
        h = (torch.randn((130, vocab), generator=g) * 4).float().numpy()
        h[:, 5] = -0.0
        h[1, 9] = -np.inf
        _ROWS[vocab] = h
    return _ROWS[vocab]


def mix_of(vocab, rows):
    """per row a different request (made once per vocabulary): (counts, presence, frequency, bias pairs, eos_masked)"""
    if (vocab, rows) not in _MIX:
        _MIX[(vocab, rows)] = _mix_of(vocab, rows)
    return _MIX[(vocab, rows)]


def _mix_of(vocab, rows):
    rng = np.random.default_rng(vocab)
    counts = np.zeros((rows, vocab), dtype=np.uint16)
    pres, freq, bias, masked = np.zeros(rows, np.float32), np.zeros(rows, np.float32), [[] for _ in range(rows)], np.zeros(rows, np.int32)
    for r in range(rows):
        kind = r % 7
        if kind == 0:
            continue                                             # no request: the row must come back identical
        pool = np.setdiff1d(np.arange(1, vocab - 1), EOS_IDS)          # (0, vocab - 1 and the EOS ids are placed by hand)
        ids = rng.choice(pool, size=600, replace=False)
        counts[r, ids[:40]] = 1
        counts[r, ids[40:80]] = 7
        counts[r, ids[80:90]] = 65535
        counts[r, [0, vocab - 1]] = (3, 65535)
        if kind in (1, 4, 5):
            pres[r], freq[r] = (0.5, 0.7) if kind != 4 else (-1.25, -0.3)
        if kind == 6:
            freq[r] = 0.1                                        # (no presence: t = f * c alone)
        if kind == 2:
            bias[r] = [(int(ids[100]), 2.5)]
        if kind in (3, 5):
            n = 512 if kind == 3 else 17
            b = [0, vocab - 1] + [int(i) for i in ids[88:88 + n - 2]]      # (some of them on counted tokens)
            v = rng.uniform(-100, 100, size=n).astype(np.float32)
            v[1], v[3] = NINF, NINF
            bias[r] = list(zip(b, v.tolist()))
        if kind in (4, 5, 3):
            masked[r] = 1
            if kind == 5 and EOS_IDS[0] < vocab:
                bias[r].append((EOS_IDS[0], 100.0))              # EOS masking wins over the bias
    return counts, pres, freq, bias, masked


def run_op(e, host, counts, pres, freq, bias, masked, pad=0):
    rows, vocab = host.shape
    buf = np.full((rows, vocab + pad), 1e9, dtype=np.float32)   # the padding must never be read or written
    buf[:, :vocab] = host
    dev = torch.from_numpy(buf).cuda()[:, :vocab]
    out = torch.full((rows, vocab + pad), -7.0, dtype=torch.float32, device="cuda")[:, :vocab]
    got = e.op_logit_adjust(dev, counts, pres, freq, masked, bias, out=out)
    torch.cuda.synchronize()
    full = got._base.cpu().numpy() if got._base is not None else got.cpu().numpy()
    if pad:
        assert (full.reshape(rows, vocab + pad)[:, vocab:] == -7.0).all()
    return got.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


# ---------------------------------------------------------------- 1. the kernel against the restatement, bit for bit
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("rows", [1, 3, 130])
@pytest.mark.parametrize("vocab", [2048, 1031, 151936])
def test_kernel_equals_the_restatement_bit_for_bit(tiny_engine, vocab, rows, pad):
    host = rows_of(vocab)[:rows] if rows > 1 else rows_of(vocab)[3:4]      # (one row alone: a row WITH a request)
    counts, pres, freq, bias, masked = mix_of(vocab, 130)
    sl = slice(0, rows) if rows > 1 else slice(3, 4)
    args = (counts[sl], pres[sl], freq[sl], bias[sl], masked[sl])
    got = run_op(tiny_engine, host, *args, pad=pad)
    want = R.adjust_rows(host, args[0], args[1], args[2], args[3], EOS_IDS, args[4])
    assert same_bits(got, want)
    if rows > 1:
        assert same_bits(got[0], host[0]) and np.signbit(got[0, 5])        # no request: the very bits, -0 included
        assert not same_bits(got[1], host[1])
    # without a count table every count is zero
    got = run_op(tiny_engine, host, None, *args[1:], pad=pad)
    assert same_bits(got, R.adjust_rows(host, None, args[1], args[2], args[3], EOS_IDS, args[4]))


# ---------------------------------------------------------------- 2. determinism
def test_same_rows_same_bits_whatever_their_place(tiny_engine):
    vocab = 151936
    host = rows_of(vocab)
    counts, pres, freq, bias, masked = mix_of(vocab, 130)
    a = run_op(tiny_engine, host, counts, pres, freq, bias, masked)
    for r in (3, 5, 129):
        alone = run_op(tiny_engine, host[r:r + 1], counts[r:r + 1], pres[r:r + 1], freq[r:r + 1], bias[r:r + 1], masked[r:r + 1])
        assert same_bits(alone[0], a[r])
    rev = run_op(tiny_engine, host[::-1].copy(), counts[::-1].copy(), pres[::-1].copy(), freq[::-1].copy(), bias[::-1], masked[::-1].copy())
    assert same_bits(rev[::-1], a)


# ---------------------------------------------------------------- 3. the decode path applies it to every step's own row
def text_ids(seed, n):
    return prng.uniform_ints(seed, n, 10, 1990).tolist()


def prefill_text(e, seq, ids):
    pos, delta = e.rope_index(ids, [])
    e.seq_reset(seq)
    return e.prefill(seq, ids, None, pos, delta, want_logits=True)


PROMPTS = [text_ids(41, 23), text_ids(42, 9), text_ids(43, 60)]
BIAS5 = {20: 3.0, 700: -4.0, 1500: NINF, 0: 1.5, 2047: -2.5}
REQ = dict(presence_penalty=0.5, frequency_penalty=0.7, logit_bias=BIAS5)
STEPS = 24


def restated_rows(raw, toks, req, min_new=0):
    out = []
    for t, row in enumerate(raw):
        c = R.saturating_counts(toks[:t], row.shape[0])
        out.append(R.adjust_row(row, c, req.get("presence_penalty", 0.0), req.get("frequency_penalty", 0.0), req.get("logit_bias"),
                                EOS_IDS, t < min_new))
    return out


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("path", ["single", "batched"])
@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_decode_path_adjusts_the_row_of_every_step(tiny_engine, mode, path, graph):
    """A chain generates 24 tokens with a request; its ids are then teacher-forced through the same kind of step (ze_decode_step /
    ze_decode_batch return each step's raw logits), the restatement is applied with the counts of the prefix generated so far,
    and every token must be the restated row's arg-max (the sampler's tie rule: lowest id) or, sampled, what
    ze_op_sample_temperature draws from the restated row at that index."""
    e = tiny_engine
    e.fill_synthetic(**CHAIN_W)
    kw = dict(repetition_penalty=1.0, ignore_eos=True, use_graph=graph)
    if mode == "sampled":
        kw.update(do_sample=True, temperature=0.9, seed=4)
    ids = PROMPTS[0]
    first = prefill_text(e, 0, ids).cpu().numpy()
    e.seq_set_logit_adjust(0, **REQ)
    if path == "single":
        toks = e.generate(0, STEPS, **kw)
    else:   # (row 0 of the call: random stream 0, what ze_op_sample_temperature draws from; company with another request)
        prefill_text(e, 1, PROMPTS[1])
        e.seq_set_logit_adjust(1, frequency_penalty=-0.4, min_new_tokens=3)
        toks = e.generate_batch([0, 1], STEPS, **kw)[0]
    assert len(toks) == STEPS
    raw = [first]
    prefill_text(e, 0, ids)
    for t in range(STEPS - 1):
        raw.append((e.decode_step(0, toks[t]) if path == "single" else e.decode_batch([0], [toks[t]])[0]).cpu().numpy())
    want_rows = restated_rows(raw, toks, REQ)
    e.seq_reset(2)
    for t, a in enumerate(want_rows):
        if mode == "greedy":
            assert toks[t] == R.argmax_lowest(a), (t, toks)
        else:
            assert toks[t] == e.sample_temperature(2, torch.from_numpy(a).cuda(), 0.9, 4, index=t), (t, toks)
    assert 1500 not in toks
    # the request mattered: the raw rows alone do not explain the tokens
    assert any(toks[t] != R.argmax_lowest(raw[t]) for t in range(STEPS)) or mode == "sampled"


# ---------------------------------------------------------------- 4. effects that need no reference
def test_effects_that_need_no_reference(tiny_engine):
    e = tiny_engine
    e.fill_synthetic(**CHAIN_W)
    ids = PROMPTS[0]
    kw = dict(ignore_eos=True)
    prefill_text(e, 0, ids)
    plain = e.generate(0, 64, **kw)
    assert len(set(plain)) < 64                                    # (left alone, the tiny model repeats itself)
    prefill_text(e, 0, ids)
    e.seq_set_logit_adjust(0, frequency_penalty=1e4)
    toks = e.generate(0, 64, **kw)
    assert len(toks) == 64 and len(set(toks)) == 64
    prefill_text(e, 0, ids)
    e.seq_set_logit_adjust(0, logit_bias={1234: 100.0})
    assert e.generate(0, 16, **kw) == [1234] * 16
    prefill_text(e, 0, ids)
    e.seq_set_logit_adjust(0, logit_bias={plain[0]: NINF})
    banned = e.generate(0, 8, **kw)
    assert banned[0] != plain[0] and plain[0] not in banned
    for batched in (False, True):                                   # EOS pushed by +100 and held back by min_new_tokens = 5
        prefill_text(e, 0, ids)
        e.seq_set_logit_adjust(0, min_new_tokens=5, logit_bias={EOS_IDS[0]: 100.0})
        toks = e.generate_batch([0], 12)[0] if batched else e.generate(0, 12)
        assert len(toks) == 6 and toks[5] == EOS_IDS[0] and not set(toks[:5]) & set(EOS_IDS), toks


# ---------------------------------------------------------------- 5. company and the default path
def test_mixed_requests_share_a_graph_and_do_not_depend_on_company(tiny_engine):
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.engine import Engine
    e = tiny_engine
    e.fill_synthetic(**CHAIN_W)
    kw = dict(repetition_penalty=1.1, ignore_eos=True)
    reqs = [None, None, dict(min_new_tokens=4, logit_bias={77: 50.0})]

    def run(eng, slots, rows, graph, requests=True, logprobs=None, **more):
        for s, w in zip(slots, rows):
            prefill_text(eng, s, PROMPTS[w])
            eng.mark_seen(s, PROMPTS[w])
            if requests and reqs[w] is not None:
                eng.seq_set_logit_adjust(s, **reqs[w])
            if logprobs is not None:
                eng.set_logprobs(s, logprobs)
        return eng.generate_batch(slots, 12, use_graph=graph, **kw, **more)

    fresh = Engine(ModelConfig.tiny(), device=0, max_seqs=3, max_ctx=1024, max_patches=1024, max_tile_side=1024)
    try:   # an engine that never saw a request
        fresh.fill_synthetic(**CHAIN_W)
        never = run(fresh, [0, 1, 2], [0, 1, 2], True, requests=False)
        never_s = run(fresh, [0, 1, 2], [0, 1, 2], True, requests=False, do_sample=True, temperature=0.9, seed=3)
    finally:
        fresh.close()
    # (chain 1: penalties, a small bias, and its own unconstrained first token banned -- so the request certainly matters)
    reqs[1] = dict(presence_penalty=0.5, frequency_penalty=0.7, logit_bias={20: 3.0, never[1][0]: NINF})
    for more, base in ((dict(), never), (dict(do_sample=True, temperature=0.9, seed=3), never_s)):
        plain = run(e, [0, 1, 2], [0, 1, 2], True, requests=False, **more)
        assert plain == base                                          # nobody asks: what the engine always computed
        mixed = run(e, [0, 1, 2], [0, 1, 2], True, **more)
        assert mixed[0] == base[0]                                    # the chain without a request, next to two with one
        assert mixed[2] != base[2] and (more or mixed[1][0] != base[1][0])
        assert run(e, [0, 1, 2], [0, 1, 2], False, **more) == mixed   # eager
        if not more:
            for w in (1, 2):                                          # alone, in another slot, graph and eager: the same tokens
                slot = (w + 1) % 3
                assert run(e, [slot], [w], False) == [mixed[w]]
                assert run(e, [slot], [w], True) == [mixed[w]]
        # flipping the requests on a running engine re-captures the step and keeps the tokens
        assert run(e, [0, 1, 2], [0, 1, 2], True, requests=False, **more) == base
        assert run(e, [0, 1, 2], [0, 1, 2], True, **more) == mixed
    # log-probabilities requested alongside report the RAW row: the values of a run with the same tokens and no adjustment
    with_lp = run(e, [0, 1, 2], [0, 1, 2], True, logprobs=3)
    lps = e.chain_logprobs_batch([0, 1, 2], 3)
    rows = [[prefill_text(e, s, PROMPTS[s]).cpu().numpy()] for s in range(3)]
    for t in range(11):
        lg = e.decode_batch([0, 1, 2], [with_lp[s][t] for s in range(3)]).cpu().numpy()
        for s in range(3):
            rows[s].append(lg[s])
    import logprobs_ref
    for s in range(3):
        host = np.stack(rows[s])
        wlp, wids, _ = logprobs_ref.token_logprobs_ref(host, with_lp[s], 3)
        ok = logprobs_ref.decided(host, 3)
        assert np.abs(lps[s][0] - wlp).max() < 2e-5 and np.array_equal(lps[s][1][ok], wids[ok])
    assert np.isfinite(lps[1][0]).all()


# ---------------------------------------------------------------- 6. lifetime
def test_the_request_and_the_counts_end_with_the_slot(tiny_engine):
    e = tiny_engine
    e.fill_synthetic(**CHAIN_W)
    ids = PROMPTS[0]
    pos, delta = e.rope_index(ids, [])
    kw = dict(ignore_eos=True)
    prefill_text(e, 0, ids)
    request = dict(frequency_penalty=1e4, logit_bias={1234: 100.0}, min_new_tokens=2)

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
        plain = e.generate(1, 10, **kw)
        bring(how)
        e.seq_set_logit_adjust(1, **request)
        forced = e.generate(1, 10, **kw)
        assert forced[0] == 1234 and len(set(forced)) == 10 and forced != plain
        bring(how)
        assert e.generate(1, 10, **kw) == plain, how                 # the slot's next chain inherits nothing
        # a new request on the slot starts from zero counts: the first run again, token for token
        bring(how)
        e.seq_set_logit_adjust(1, **request)
        assert e.generate(1, 10, **kw) == forced, how
    prefill_text(e, 1, ids)
    plain = e.generate(1, 10, **kw)
    # all-off values clear the request
    prefill_text(e, 1, ids)
    e.seq_set_logit_adjust(1, logit_bias={1234: 100.0})
    e.seq_set_logit_adjust(1)
    assert e.generate(1, 10, **kw) == plain
    # invalid arguments are refused and change nothing
    prefill_text(e, 1, ids)
    e.seq_set_logit_adjust(1, logit_bias={1234: 100.0})
    for bad in (dict(logit_bias={2048: 1.0}), dict(logit_bias={-1: 1.0}), dict(logit_bias=[(5, 1.0), (5, 2.0)]),
                dict(logit_bias={5: float("nan")}), dict(logit_bias={5: float("inf")}), dict(presence_penalty=float("inf")),
                dict(frequency_penalty=float("nan")), dict(min_new_tokens=-1), dict(logit_bias={i: 1.0 for i in range(513)})):
        with pytest.raises(ZoomEarthError):
            e.seq_set_logit_adjust(1, **bad)
    with pytest.raises(ZoomEarthError):
        e.seq_set_logit_adjust(3, presence_penalty=1.0)               # no such slot
    assert e.generate(1, 6, **kw) == [1234] * 6
    e.seq_set_logit_adjust(1, logit_bias={i: -1.0 for i in range(512)})   # the largest list is fine
    e.seq_reset(1)


# ---------------------------------------------------------------- 7. surfaces
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


def test_generate_equals_the_scheduler_run_of_the_same_request(stack):
    from zoomearth_amd.scheduler import ChainScheduler, Request
    model, proc = stack
    prompt = words(31, 14)
    inp = proc(text=[prompt], return_tensors="pt").to(model.device)
    L = inp["input_ids"].shape[1]
    plain = model.generate(**inp, max_new_tokens=12)[0, L:].tolist()
    eos = int(model.config.eos_token_ids[0])
    got = model.generate(**inp, max_new_tokens=12, min_new_tokens=4, sequence_bias={(eos,): 100.0, (25,): 2.0},
                         frequency_penalty=0.8)[0, L:].tolist()
    assert got != plain[:len(got)] and len(got) == 5 and got[4] == eos and eos not in got[:4]
    req = Request(prompt=prompt, images=[], max_new_tokens=12, min_new_tokens=4, logit_bias={eos: 100.0, 25: 2.0}, frequency_penalty=0.8)
    other = Request(prompt=words(32, 9), images=[], max_new_tokens=12)               # company without a request
    sched = ChainScheduler(model, proc, burst=4)
    sched.submit(req)
    sched.submit(other)
    sched.run()
    assert list(req.tokens) == got
    # suppress_tokens bans the unconstrained first token
    sup = model.generate(**inp, max_new_tokens=4, suppress_tokens=[plain[0]])[0, L:].tolist()
    assert sup[0] != plain[0] and plain[0] not in sup
    # two rows of one generate call carry the request each
    two = proc(text=[prompt, prompt], return_tensors="pt", padding="longest").to(model.device)
    both = model.generate(**two, max_new_tokens=12, min_new_tokens=4, sequence_bias={(eos,): 100.0, (25,): 2.0}, frequency_penalty=0.8)
    assert both[0, L:L + 5].tolist() == both[1, L:L + 5].tolist() and both[0, L + 4] == eos and eos not in both[0, L:L + 4].tolist()
    with pytest.raises(ValueError):
        model.generate(**inp, max_new_tokens=2, sequence_bias={(5, 6): 1.0})


def test_server_applies_the_requests_own_values(stack):
    from fastapi.testclient import TestClient
    from zoomearth_amd import serve
    model, proc = stack
    client = TestClient(serve.create_app(serve.ChatServer(model, proc, "ZoomEarth")))
    msgs = [{"role": "user", "content": words(21, 12)}]

    def ask(**kw):
        r = client.post("/v1/chat/completions", json={"model": "ZoomEarth", "messages": msgs, "max_tokens": 10, **kw})
        return r.status_code, r.json()

    code, plain = ask()
    assert code == 200
    fields = dict(frequency_penalty=1.5, presence_penalty=0.5, logit_bias={"25": 8, "1500": -100})
    code, res = ask(**fields)
    assert code == 200 and res["choices"][0]["message"] != plain["choices"][0]["message"]
    direct = serve.ChatServer(model, proc, "ZoomEarth").complete({"messages": msgs, "max_tokens": 10, **fields})
    assert direct["choices"][0]["message"] == res["choices"][0]["message"] and direct["usage"] == res["usage"]
    inp = proc(text=[serve.build_prompt(msgs)[0]], return_tensors="pt").to(model.device)
    L = inp["input_ids"].shape[1]
    g = model.generate(**inp, max_new_tokens=10, frequency_penalty=1.5, presence_penalty=0.5, logit_bias={25: 8.0, 1500: -100.0})
    ids = g[0, L:L + res["usage"]["completion_tokens"]].tolist()
    assert proc.tokenizer.decode(ids, skip_special_tokens=True).strip() == res["choices"][0]["message"]["content"]
    code, res2 = ask(min_tokens=10, logit_bias={str(model.config.eos_token_ids[0]): 100})
    assert code == 200 and res2["usage"]["completion_tokens"] == 10 and res2["choices"][0]["finish_reason"] == "length"
    code, again = ask()
    assert code == 200 and again["choices"][0]["message"] == plain["choices"][0]["message"]      # the next request inherits nothing
    for bad in (dict(presence_penalty=2.5), dict(frequency_penalty="x"), dict(logit_bias={"2048": 1}), dict(logit_bias={"5": 101}),
                dict(logit_bias=[1]), dict(min_tokens=-1), dict(min_tokens=1.5)):
        code, body = ask(**bad)
        assert code == 400 and body["error"]["type"] == "invalid_request_error", bad

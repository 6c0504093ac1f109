"""GPU: per-token log-probabilities of generated tokens (ze_seq_set_logprobs / ze_chain_logprobs* / ze_op_token_logprobs) --
the kernel against the numpy restatement (tests/logprobs_ref.py), the decode path against the logits of its own steps, ze_score,
batch invariance under mixed requests and graphs, the request's lifetime, and the public surfaces end to end.

Tolerances: the kernel is fp32 arithmetic on given fp32 logits -> 2e-5 absolute against float64 on the same rows (the bound
tests/test_gpu_score.py holds k_token_logprob to).  Decode against ze_score inherits the bf16 model error: 2 x the HF-bf16 /
HF-fp32 spread of tests/golden/score.npz, as the score tests."""
import numpy as np
import pytest
import torch

import logprobs_ref as R
import parity_ledger
from gpu_util import CHAIN_W, tiny_engine  # noqa: F401
from oracle import prng
from zoomearth_amd._lib import ZoomEarthError

pytestmark = pytest.mark.gpu

TOL = 2e-5
_ROWS = {}


def rows_of(vocab):
    """130 rows of randn x 4 (made once per vocabulary) and their targets"""
    if vocab not in _ROWS:
        g = torch.Generator().manual_seed(1000 + vocab)
        _ROWS[vocab] = ((torch.randn((130, vocab), generator=g) * 4).float().numpy(),
                        torch.randint(0, vocab, (130,), generator=g, dtype=torch.int32).numpy())
    return _ROWS[vocab]


def text_ids(seed, n):
    return prng.uniform_ints(seed, n, 10, 1990).tolist()


def prefill_text(e, seq, ids):
    pos, delta = e.rope_index(ids, [])
    e.seq_reset(seq)
    return e.prefill(seq, ids, None, pos, delta, want_logits=True)


def run_op(e, host, targets, n, pad=0):
    rows, vocab = host.shape
    buf = np.full((rows, vocab + pad), 1e9, dtype=np.float32)   # the padding must never be read
    buf[:, :vocab] = host
    dev = torch.from_numpy(buf).cuda()[:, :vocab]
    lp, ids, tlp = e.op_token_logprobs(dev, torch.from_numpy(np.asarray(targets, dtype=np.int32)).cuda(), n)
    return lp.cpu().numpy(), ids.cpu().numpy(), tlp.cpu().numpy()


def check_against_ref(got, host, targets, n, what):
    lp, ids, tlp = got
    wlp, wids, wtlp = R.token_logprobs_ref(host, targets, n)
    err = float(np.abs(lp - wlp).max())
    print(f"{what}: max |logprob - float64| = {err:.3g}")
    assert err < TOL, what
    if n:
        ok = R.decided(host, n)
        assert np.array_equal(ids[ok], wids[ok]), what
        fin = wids[ok] >= 0
        terr = float(np.abs(tlp[ok][fin] - wtlp[ok][fin]).max()) if fin.any() else 0.0
        print(f"{what}: max |top logprob - float64| = {terr:.3g}, {int((~ok).sum())} rows undecided")
        assert terr < TOL and np.isneginf(tlp[ok][~fin]).all(), what
        return ok
    return np.ones(len(host), dtype=bool)


# ---------------------------------------------------------------- 1. the kernel against the restatement
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("rows", [1, 3, 130])
@pytest.mark.parametrize("vocab", [2048, 151936])
def test_kernel_vs_restatement(tiny_engine, vocab, rows, pad):
    host, tg = rows_of(vocab)
    host, tg = host[:rows], tg[:rows]
    for n in (0, 1, 5, 20):
        ok = check_against_ref(run_op(tiny_engine, host, tg, n, pad), host, tg, n, f"vocab {vocab} rows {rows} pad {pad} top_n {n}")
        assert (~ok).sum() <= max(0, rows // 100)     # at most 1 % of the rows hinge on an exact tie


def test_inputs_leave_at_most_one_percent_undecided():
    for vocab in (2048, 151936):
        host, _ = rows_of(vocab)
        for n in (1, 5, 20):
            assert (~R.decided(host, n)).sum() <= 1


# ---------------------------------------------------------------- 2. ties and edges
@pytest.mark.parametrize("vocab", [2048, 151936])
def test_ties_and_edges(tiny_engine, vocab):
    e = tiny_engine
    flat = np.full((1, vocab), 0.25, dtype=np.float32)          # (at 151,936: every entry is a candidate -> the overflow path)
    for n in (5, 20):
        lp, ids, tlp = run_op(e, flat, [7], n)
        assert ids[0].tolist() == list(range(n))
        assert abs(lp[0] + np.log(vocab)) < TOL and np.abs(tlp[0] + np.log(vocab)).max() < TOL
    two = rows_of(vocab)[0][:1].copy()
    two[0, [vocab - 3, 17]] = 50.0                                # the maximum at two ids: the lower id first
    lp, ids, tlp = run_op(e, two, [vocab - 3], 5)
    wlp, wids, wtlp = R.token_logprobs_ref(two, [vocab - 3], 5)
    assert ids[0, :2].tolist() == [17, vocab - 3] and np.array_equal(ids, wids)
    assert tlp[0, 0] == tlp[0, 1] == lp[0] and np.abs(tlp - wtlp).max() < TOL
    dup = np.zeros((1, vocab), dtype=np.float32)                  # the maximum thousands of times (overflow), lower values behind
    dup[0, ::2] = 3.0
    lp, ids, tlp = run_op(e, dup, [1], 20)
    assert ids[0].tolist() == list(range(0, 40, 2)) and abs(lp[0] - R.token_logprobs_ref(dup, [1], 0)[0][0]) < TOL
    masked = np.full((1, vocab), -np.inf, dtype=np.float32)
    masked[0, [3, vocab - 1, 300]] = [0.0, 2.0, 1.0]
    lp, ids, tlp = run_op(e, masked, [300], 5)
    assert ids[0].tolist() == [vocab - 1, 300, 3, -1, -1] and np.isneginf(tlp[0, 3:]).all()
    wlp, _, wtlp = R.token_logprobs_ref(masked, [300], 5)
    assert abs(lp[0] - wlp[0]) < TOL and np.abs(tlp[0, :3] - wtlp[0, :3]).max() < TOL
    if vocab == 2048:
        big = np.zeros((1, vocab), dtype=np.float32)
        big[0, 77] = 1e4
        lp, ids, tlp = run_op(e, big, [77], 1)
        assert lp[0] == 0.0 and ids[0, 0] == 77 and tlp[0, 0] == 0.0
        with pytest.raises(ZoomEarthError):
            run_op(e, big, [77], 21)
        with pytest.raises(ZoomEarthError):
            e.set_logprobs(0, 21)
        with pytest.raises(ZoomEarthError):
            e.set_logprobs(0, -2)


# ---------------------------------------------------------------- 3. determinism
def test_same_rows_same_bits_whatever_their_place(tiny_engine):
    host, tg = rows_of(151936)
    a = run_op(tiny_engine, host, tg, 20)
    b = run_op(tiny_engine, host, tg, 20)
    c = run_op(tiny_engine, host[::-1].copy(), tg[::-1].copy(), 20)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        assert np.array_equal(x.view(np.uint32), z[::-1].view(np.uint32))


# ---------------------------------------------------------------- 4. the decode path against the logits of its own steps
PROMPTS = [text_ids(41, 23), text_ids(42, 9), text_ids(43, 60)]


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_decode_path_reports_the_raw_row_of_every_step(tiny_engine, mode):
    """The chains generate with set_logprobs(5); their ids are then teacher-forced through ze_decode_batch, which returns each
    step's logits (a row does not depend on its batch): every reported entry is the restatement on the RAW row of its step --
    also under repetition penalty 1.3 and temperature sampling, which change the draw and not the report."""
    e = tiny_engine
    e.fill_synthetic(**CHAIN_W)
    kw = dict(repetition_penalty=1.3, ignore_eos=True)
    if mode == "sampled":
        kw.update(do_sample=True, temperature=0.9, seed=4)
    steps = 7
    for s, ids in enumerate(PROMPTS):
        prefill_text(e, s, ids)
        e.mark_seen(s, ids)
        e.set_logprobs(s, 5)
    toks = e.generate_batch([0, 1, 2], steps, **kw)
    got = e.chain_logprobs_batch([0, 1, 2], 5)
    assert [len(t) for t in toks] == [steps] * 3 and [len(g[0]) for g in got] == [steps] * 3
    rows = [[] for _ in PROMPTS]
    for s, ids in enumerate(PROMPTS):
        rows[s].append(prefill_text(e, s, ids).cpu().numpy())
    for t in range(steps - 1):
        lg = e.decode_batch([0, 1, 2], [toks[s][t] for s in range(3)]).cpu().numpy()
        for s in range(3):
            rows[s].append(lg[s])
    worst = 0.0
    for s in range(3):
        host = np.stack(rows[s])
        wlp, wids, wtlp = R.token_logprobs_ref(host, toks[s], 5)
        ok = R.decided(host, 5)
        lp, ids, tlp = got[s]
        worst = max(worst, float(np.abs(lp - wlp).max()), float(np.abs(tlp[ok] - wtlp[ok]).max()))
        assert np.abs(lp - wlp).max() < TOL, (mode, s)
        assert np.array_equal(ids[ok], wids[ok]) and np.abs(tlp[ok] - wtlp[ok]).max() < TOL, (mode, s)
        assert ok.sum() >= steps - 1
    print(f"{mode}: max |reported - float64 on the step's row| = {worst:.3g}")
    if mode == "sampled":   # (the penalised, tempered draw is not always the raw arg-max: the report is not that of the draw's scores)
        assert any(toks[s][t] != int(np.argmax(rows[s][t])) for s in range(3) for t in range(steps))


# ---------------------------------------------------------------- 5. agreement with ze_score
def test_decode_time_logprobs_agree_with_score(tiny_engine, golden_npz):
    e = tiny_engine
    e.fill_synthetic(**CHAIN_W)
    s = golden_npz("score.npz")
    yard = float(np.abs(s["logps_bf16_logits_fp32_softmax"] - s["logps_fp32"]).max())
    ids = PROMPTS[0]
    prefill_text(e, 0, ids)
    e.set_logprobs(0, 0)
    toks = e.generate(0, 12, ignore_eos=True, do_sample=True, temperature=0.9, seed=2)
    lp, _, _ = e.chain_logprobs(0)
    full = ids + toks
    pos, delta = e.rope_index(full, [])
    e.seq_reset(1)
    sc = e.score(1, full, None, pos, delta).cpu().numpy()[len(ids) - 1:]
    err = float(np.abs(lp - sc).max())
    print(f"max |decode-time - ze_score| = {err:.4f}, yardstick {yard:.4f}, ratio {err / yard:.3f}")
    parity_ledger.record(err, yard, "test_gpu_logprobs.py: decode-time logprob vs ze_score")
    assert len(lp) == len(toks) == len(sc) and err <= 2.0 * yard


# ---------------------------------------------------------------- 6. batch invariance, mixed requests, graphs
def test_mixed_requests_share_a_graph_and_do_not_depend_on_company(tiny_engine):
    e = tiny_engine
    e.fill_synthetic(**CHAIN_W)
    kw = dict(repetition_penalty=1.1, ignore_eos=True)
    want_n = [None, 0, 20]

    def run(slots, rows, graph, requests=True):
        for s, w in zip(slots, rows):
            prefill_text(e, s, PROMPTS[w])
            e.mark_seen(s, PROMPTS[w])
            if requests and want_n[w] is not None:
                e.set_logprobs(s, want_n[w])
        return e.generate_batch(slots, 12, use_graph=graph, **kw)

    plain = run([0, 1, 2], [0, 1, 2], True, requests=False)
    toks = run([0, 1, 2], [0, 1, 2], True)
    assert toks == plain
    with pytest.raises(ZoomEarthError):
        e.chain_logprobs(0)                                       # it never asked
    mixed = {1: e.chain_logprobs(1), 2: e.chain_logprobs(2)}
    assert mixed[1][1].shape == (12, 0) and mixed[2][1].shape == (12, 20)
    both = e.chain_logprobs_batch([2, 1], 20)                     # the batched gather says the same
    assert np.array_equal(both[0][0], mixed[2][0]) and np.array_equal(both[0][1], mixed[2][1])
    assert np.array_equal(both[1][0], mixed[1][0]) and (both[1][1] == -1).all() and np.isneginf(both[1][2]).all()
    for w in (1, 2):                                              # alone, in another slot, launched eagerly: the same bits
        slot = (w + 1) % 3
        assert run([slot], [w], False) == [plain[w]]
        alone = e.chain_logprobs(slot)
        for x, y in zip(alone, mixed[w]):
            assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), w
    # flipping the request on a running engine re-captures the step and keeps the tokens
    assert run([0, 1, 2], [0, 1, 2], True, requests=False) == plain
    assert run([0, 1, 2], [0, 1, 2], True) == plain
    assert run([0, 1, 2], [0, 1, 2], True, requests=False) == plain
    # the single-chain path (folded greedy arg-max) reports the same values as the batched step within the kernel's bound
    prefill_text(e, 0, PROMPTS[2])
    e.mark_seen(0, PROMPTS[2])
    e.set_logprobs(0, 20)
    for graph in (True, False):
        if not graph:
            prefill_text(e, 0, PROMPTS[2])
            e.mark_seen(0, PROMPTS[2])
            e.set_logprobs(0, 20)
        one = e.generate(0, 12, use_graph=graph, **kw)
        lp1 = e.chain_logprobs(0)
        assert lp1[0].shape == (12,) and np.isfinite(lp1[0]).all() and (lp1[0] <= 0).all()
        if one == plain[2]:   # (GEMV and GEMM logits differ in the last bf16 bits: only equal ids are comparable)
            assert np.abs(lp1[0] - mixed[2][0]).max() < 0.05


# ---------------------------------------------------------------- 7. lifetime
def test_the_request_ends_with_the_slot_and_eos_trims_the_entries(tiny_engine):
    e = tiny_engine
    e.fill_synthetic(**CHAIN_W)
    ids = PROMPTS[0]
    pos, delta = e.rope_index(ids, [])
    for how in ("reset", "truncate", "copy"):
        prefill_text(e, 0, ids)
        prefill_text(e, 1, ids)
        e.set_logprobs(1, 3)
        e.generate(1, 2, ignore_eos=True)
        assert len(e.chain_logprobs(1)[0]) == 2
        if how == "reset":
            e.seq_reset(1)
        elif how == "truncate":
            e.seq_truncate(1, len(ids) - 1)
        else:
            e.seq_copy_prefix(1, 0, len(ids) - 1)
        with pytest.raises(ZoomEarthError):
            e.chain_logprobs(1)
        with pytest.raises(ZoomEarthError):
            e.chain_logprobs_batch([1], 3)
    # a chain that meets its EOS in the middle of a burst: exactly the entries of its tokens
    for s, p in enumerate(PROMPTS):
        prefill_text(e, s, p)
        e.mark_seen(s, p)
    free = e.generate_batch([0, 1, 2], 12, repetition_penalty=1.3, ignore_eos=True)
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.engine import Engine
    cfg = ModelConfig.tiny()
    cfg.eos_token_ids = (free[1][4],)
    e2 = Engine(cfg, max_seqs=3, max_ctx=512, max_patches=1024, max_tile_side=1024)
    try:
        e2.fill_synthetic(**CHAIN_W)
        for s, p in enumerate(PROMPTS):
            prefill_text(e2, s, p)
            e2.mark_seen(s, p)
            e2.set_logprobs(s, 2)
        got = e2.generate_batch([0, 1, 2], 12, repetition_penalty=1.3, sync_every=8)
        cut = free[1].index(free[1][4]) + 1
        assert got[1] == free[1][:cut] and cut < 12
        each = [e2.chain_logprobs(s) for s in range(3)]
        assert [len(x[0]) for x in each] == [len(t) for t in got] and each[1][1].shape == (cut, 2)
        assert [e2.chain_tokens(s) for s in range(3)] == got
        for a, b in zip(each, e2.chain_logprobs_batch([0, 1, 2], 2)):
            assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
    finally:
        e2.close()


# ---------------------------------------------------------------- 8. surfaces
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


def test_server_returns_the_logprobs_of_a_direct_generate(stack, golden_npz):
    from fastapi.testclient import TestClient
    from zoomearth_amd import serve
    model, proc = stack
    client = TestClient(serve.create_app(serve.ChatServer(model, proc, "ZoomEarth")))
    msgs = [{"role": "user", "content": words(21, 12)}]

    def ask(**kw):
        r = client.post("/v1/chat/completions", json={"model": "ZoomEarth", "messages": msgs, "max_tokens": 10, **kw})
        return r.status_code, r.json()

    code, plain = ask()
    assert code == 200 and "logprobs" not in plain["choices"][0]
    code, res = ask(logprobs=True, top_logprobs=3)
    assert code == 200 and res["choices"][0]["message"] == plain["choices"][0]["message"]
    content = res["choices"][0]["logprobs"]["content"]
    assert len(content) == res["usage"]["completion_tokens"]
    inp = proc(text=[serve.build_prompt(msgs)[0]], return_tensors="pt").to(model.device)
    L = inp["input_ids"].shape[1]
    g = model.generate(**inp, max_new_tokens=10, logprobs=3)
    ids = g.sequences[0, L:L + len(content)].tolist()
    tok = proc.tokenizer
    assert [c["token"] for c in content] == [tok.decode([i]) for i in ids]
    assert tok.decode(ids, skip_special_tokens=True).strip() == res["choices"][0]["message"]["content"]
    # ChatServer.complete runs the request through model.generate itself: the same values, bit for bit
    direct = serve.ChatServer(model, proc, "ZoomEarth").complete({"messages": msgs, "max_tokens": 10, "logprobs": True, "top_logprobs": 3})
    dcontent = direct["choices"][0]["logprobs"]["content"]
    assert [c["token"] for c in dcontent] == [c["token"] for c in content]
    assert [c["logprob"] for c in dcontent] == g.logprobs[0, :len(content)].tolist()
    for t, c in enumerate(dcontent):
        assert c["bytes"] == list(c["token"].encode("utf-8")) and len(c["top_logprobs"]) == 3
        assert [x["logprob"] for x in c["top_logprobs"]] == g.top_logprobs[0, t].tolist()
        assert [x["token"] for x in c["top_logprobs"]] == [tok.decode([i]) for i in g.top_ids[0, t].tolist()]
    # The endpoint decodes on the scheduler's batched step (MFMA GEMM logits), generate() of one row on the single-chain step
    # (GEMV logits): the same ids, logits that differ in their last bf16 bits -- the two paths are held to the bound between the
    # project's decode and prefill paths (2 x the HF-bf16 / HF-fp32 spread of tests/golden/score.npz)
    s = golden_npz("score.npz")
    yard = float(np.abs(s["logps_bf16_logits_fp32_softmax"] - s["logps_fp32"]).max())
    err = float(np.abs(np.asarray([c["logprob"] for c in content]) - g.logprobs[0, :len(content)].numpy()).max())
    print(f"max |endpoint - generate| = {err:.5f}, yardstick {yard:.4f}")
    parity_ledger.record(err, yard, "test_gpu_logprobs.py: endpoint (batched step) vs generate (single-chain step)")
    assert err <= 2.0 * yard
    for c in content:
        assert c["bytes"] == list(c["token"].encode("utf-8")) and len(c["top_logprobs"]) == 3
        assert all(x["logprob"] <= 0 for x in c["top_logprobs"])
    assert g.logprobs.shape == (1, g.sequences.shape[1] - L) and g.top_ids.shape == (1, g.sequences.shape[1] - L, 3)
    for bad in (dict(top_logprobs=3), dict(logprobs=True, top_logprobs=21), dict(logprobs=True, top_logprobs=1.5)):
        code, body = ask(**bad)
        assert code == 400 and body["error"]["type"] == "invalid_request_error", bad
    with pytest.raises(ValueError):
        model.generate(**inp, max_new_tokens=2, logprobs=21)


def test_rollout_fills_the_sampled_logps_of_both_stages(golden_npz):
    from test_gpu_rollout import bbox_tokenizer, word
    from zoomearth_amd import hostloop as H
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.image import DeviceImage
    from zoomearth_amd.modeling import ZoomEarthForConditionalGeneration
    from zoomearth_amd.processor import ZoomEarthProcessor
    from zoomearth_amd.rollout import rollout_two_stage
    s = golden_npz("score.npz")
    yard = float(np.abs(s["logps_bf16_logits_fp32_softmax"] - s["logps_fp32"]).max())
    model = ZoomEarthForConditionalGeneration.from_synthetic(ModelConfig.tiny(), **CHAIN_W, max_seqs=8, max_ctx=2048,
                                                            max_patches=8192, max_tile_side=2048, max_prefill_rows=8192)
    try:
        proc = ZoomEarthProcessor(bbox_tokenizer(), min_pixels=3136, max_pixels=128 * 128 * 28 * 28)
        tile = DeviceImage.from_numpy(prng.synthetic_tile(90, 700, 900), model.engine)
        q = " ".join(word(int(v)) for v in prng.uniform_ints(70, 5, 0, 1999))
        samples = [dict(prompt=H.stage1_prompt(q), image=tile, bbox=[10, 10, 200, 200])]
        ros = rollout_two_stage(model, proc, samples, num_generations=2, temperature=0.9, max_new_tokens=6, seed=11,
                                with_logps=True, sampled_logps=True)
        assert all(r.error is None for r in ros)
        worst = 0.0
        for r in ros:
            assert r.prompt2 is not None
            for ids, lps in ((r.completion1_ids, r.completion1_logps), (r.completion2_ids, r.completion2_logps)):
                assert len(lps) == len(ids) > 0 and all(np.isfinite(v) and v <= 0 for v in lps)
            tail = r.logps[-len(r.completion2_ids):].cpu().numpy()
            worst = max(worst, float(np.abs(tail - np.asarray(r.completion2_logps, dtype=np.float32)).max()))
        print(f"max |logps tail - completion2_logps| = {worst:.4f}, yardstick {yard:.4f}")
        parity_ledger.record(worst, yard, "test_gpu_logprobs.py: rollout sampled logps vs scored logps")
        assert worst <= 2.0 * yard
        plain = rollout_two_stage(model, proc, samples, num_generations=2, temperature=0.9, max_new_tokens=6, seed=11,
                                  with_logps=False)
        assert [r.completion2_ids for r in plain] == [r.completion2_ids for r in ros]
        assert all(r.completion1_logps == [] and r.completion2_logps == [] for r in plain)
    finally:
        model.engine.close()

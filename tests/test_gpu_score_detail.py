"""GPU: what a scored position reports beyond its log-probability (k_score_detail / ze_op_score_detail / ze_score_batch_detail,
Engine.score_batch_detail, the scheduler's and the server's prompt_logprobs).

Rank, top ids and the empty places are exact (tests/score_detail_ref.py); the top log-probabilities are the bits the same call gives
for that id as target; the log-probability is the bits of k_token_logprob.  Tolerances:
  logprob vs float64          2e-5, the bound tests/test_gpu_score.py::test_token_logprob_kernel holds k_token_logprob to
  entropy vs float64          ENT_BOUND = 4 x the worst error measured over the rows of this file on an MI355X
                              (profiles/score_detail_kernel_stats.csv): measured 1.765e-06 at entropies 0 .. 9.85 (two ulps of
                              fp32 at 8 .. 16), so 7.06e-06
  entropy vs the numpy float32 restatement (same order of operations; numpy's exp / log are not the device's): measured
                              9.537e-07 (one ulp at 8 .. 16), held to the same ENT_BOUND
Model level: bit equality throughout."""
import numpy as np
import pytest
import torch

import score_detail_ref as R
from gpu_util import CHAIN_W, tiny_engine  # noqa: F401
from zoomearth_amd._lib import ZoomEarthError
from zoomearth_amd.config import ModelConfig
from zoomearth_amd.engine import Engine

pytestmark = pytest.mark.gpu

ENT_MEASURED = 1.765e-06      # max |entropy - float64| over the rows of this file, MI355X
ENT_F32_MEASURED = 9.537e-07  # max |entropy - numpy float32 restatement|, same rows
ENT_BOUND = 4 * ENT_MEASURED
BIG = 151936


def _rand(seed, rows, vocab, scale=3.0):
    return R.to_bf16(np.random.default_rng(seed).standard_normal((rows, vocab)).astype(np.float32) * scale)


def _cases():
    """name -> (logits f32 [rows, vocab] of bf16 values, ld, targets, top_n)"""
    c = {}
    c["vocab8_top20"] = (_rand(1, 2, 8), 8, [3, 7], 20)
    c["vocab77_tail"] = (_rand(2, 3, 77), 80, [0, 76, 40], 5)
    c["vocab1003"] = (_rand(3, 3, 1003), 1008, [1002, 5, 500], 20)
    c["vocab1003_top1"] = (_rand(3, 3, 1003), 1008, [1002, 5, 500], 1)
    c["vocab1003_top0"] = (_rand(3, 3, 1003), 1008, [1002, 5, 500], 0)
    c["all_equal"] = (np.full((2, 5003), 1.5, np.float32), 5008, [4100, 0], 20)
    shared = _rand(4, 1, 8197)
    m = np.float32(shared.max() + 1)
    pick = np.random.default_rng(5).permutation(8197)[:5000]
    shared[0, pick] = m
    c["max_shared_5000"] = (shared, 8200, [int(np.sort(pick)[2500])], 20)
    holes = _rand(6, 2, 1003)
    holes[0, ::3] = -np.inf
    holes[1, 7:] = -np.inf               # seven finite entries: places 7 .. cannot be filled
    c["minus_inf_entries"] = (holes, 1008, [4, 9], 20)
    c["all_minus_inf"] = (np.full((1, 77), -np.inf, np.float32), 80, [3], 4)
    um = _rand(7, 3, 1003)
    um[0, 611] = 40.0
    c["target_unique_max_and_out_of_range"] = (um, 1008, [611, -1, 1003], 3)
    zeros = _rand(8, 1, 1003)
    zeros[0, 100:140:2] = 0.0
    zeros[0, 101:140:2] = -0.0
    zeros[0, zeros[0] > 0] *= -1         # the zeros of both signs are the maximum, tied
    c["signed_zeros"] = (zeros, 1008, [131], 20)
    c["rows130"] = (_rand(9, 130, 1003), 1008, np.random.default_rng(10).integers(0, 1003, 130).tolist(), 7)
    big = _rand(11, 2, BIG, 2.0)
    # row 1: five unique values on top, then one value shared by ids on both sides of id 131,072 (the second chunk of the id walk)
    tied = [130000, 131071, 131072, 131073, 140000, 151935]
    big[1, tied] = np.float32(big[1].max() + 1)
    big[1, [7, 70000, 131500, 99, 151000]] = big[1, tied[0]] + np.float32([8, 6, 4, 2, 1])
    c["vocab151936"] = (big, BIG, [123456, 131073], 8)
    return {k: (R.to_bf16(v[0]),) + v[1:] for k, v in c.items()}


@pytest.fixture(scope="module")
def results(tiny_engine):
    """every case through ze_op_score_detail and ze_op_token_logprob once; the reference once"""
    e = tiny_engine
    out = {}
    for name, (lg, ld, targets, n) in _cases().items():
        rows, vocab = lg.shape
        buf = torch.full((rows, ld), 1e30, dtype=torch.bfloat16, device="cuda")   # a read of the padding would win every maximum
        buf[:, :vocab] = torch.from_numpy(lg).cuda().to(torch.bfloat16)
        tg = torch.tensor(targets, dtype=torch.int32, device="cuda")
        d = e.op_score_detail(buf[:, :vocab], tg, n)
        plain = e.op_token_logprob(buf[:, :vocab], tg)
        torch.cuda.synchronize()
        ref = [R.score_detail(lg[r], targets[r], n) for r in range(rows)]
        f64 = [R.score_detail_f64(lg[r], targets[r]) for r in range(rows)]
        out[name] = dict(lg=lg, targets=targets, n=n, buf=buf, lp=d.logps.cpu().numpy(), ent=d.entropy.cpu().numpy(),
                         rank=d.rank.cpu().numpy(), ids=None if n == 0 else d.top_ids.cpu().numpy(),
                         tlp=None if n == 0 else d.top_logprobs.cpu().numpy(), plain=plain.cpu().numpy(), ref=ref, f64=f64)
    return out


CASES = list(_cases())


@pytest.mark.parametrize("name", CASES)
def test_rank_top_ids_and_empty_places_are_exact(results, name):
    r = results[name]
    for i, (lp, ent, rank, ids, tlp) in enumerate(r["ref"]):
        assert int(r["rank"][i]) == rank, (name, i)
        if r["n"]:
            assert r["ids"][i].tolist() == ids.tolist(), (name, i)
            empty = ids < 0
            assert np.all(np.isneginf(r["tlp"][i][empty])) and np.all(np.isfinite(r["tlp"][i][~empty])), (name, i)


def test_the_stated_edge_cases(results):
    eq = results["all_equal"]
    assert eq["ids"][0].tolist() == list(range(20)) and eq["rank"].tolist() == [4100, 0]
    assert results["vocab8_top20"]["ids"][0][8:].tolist() == [-1] * 12
    assert results["minus_inf_entries"]["ids"][1][7:].tolist() == [-1] * 13
    none = results["all_minus_inf"]
    assert np.isnan(none["ent"][0]) and none["rank"][0] == -1 and none["ids"][0].tolist() == [-1] * 4
    um = results["target_unique_max_and_out_of_range"]
    assert um["rank"].tolist() == [0, -1, -1] and um["lp"][1] == 0.0 and um["lp"][2] == 0.0 and um["ids"][0][0] == 611
    sh = results["max_shared_5000"]
    assert sh["rank"][0] == 2500 and np.all(np.diff(sh["ids"][0]) > 0)
    big = results["vocab151936"]
    assert big["ids"][1].tolist() == [7, 70000, 131500, 99, 151000, 130000, 131071, 131072] and big["rank"][1] == 8
    z = results["signed_zeros"]
    assert z["ids"][0].tolist() == list(range(100, 120)) and z["rank"][0] == 31


@pytest.mark.parametrize("name", CASES)
def test_top_logprobs_are_the_bits_of_the_logprob_output_for_that_id(results, tiny_engine, name):
    r = results[name]
    if not r["n"]:
        return
    ids = r["ids"]
    vocab = r["lg"].shape[1]
    for k in range(r["n"]):                                         # place k of every row as that row's target
        col = np.ascontiguousarray(ids[:, k])
        if np.all(col < 0):
            continue
        d = tiny_engine.op_score_detail(r["buf"][:, :vocab], torch.from_numpy(col).cuda(), 0)
        lp = d.logps.cpu().numpy()
        has = col >= 0
        assert np.array_equal(lp[has].view(np.uint32), r["tlp"][:, k][has].view(np.uint32)), (name, k)
        assert np.all(d.rank.cpu().numpy()[has] == k), (name, k)   # and place k holds the id of rank k


@pytest.mark.parametrize("name", CASES)
def test_logprob_is_bit_equal_to_k_token_logprob(results, name):
    r = results[name]
    assert np.array_equal(r["lp"].view(np.uint32), r["plain"].view(np.uint32)), name


def test_logprob_and_entropy_against_float64_and_the_float32_restatement(results):
    worst_lp = worst_ent = worst_f32 = 0.0
    ents = []
    for name, r in results.items():
        for i, ((lp64, ent64), (lp32, ent32, *_)) in enumerate(zip(r["f64"], r["ref"])):
            if np.isnan(ent64):
                continue
            if 0 <= r["targets"][i] < r["lg"].shape[1] and np.isfinite(lp64):
                worst_lp = max(worst_lp, abs(float(r["lp"][i]) - lp64))
            worst_ent = max(worst_ent, abs(float(r["ent"][i]) - ent64))
            worst_f32 = max(worst_f32, abs(float(r["ent"][i]) - float(ent32)))
            ents.append(ent64)
    print(f"score_detail: max|logprob - f64| = {worst_lp:.3e} (allowed 2e-5); max|entropy - f64| = {worst_ent:.3e}, "
          f"max|entropy - numpy f32 restatement| = {worst_f32:.3e} (allowed {ENT_BOUND:.3e}); entropies {min(ents):.3f} .. {max(ents):.3f}")
    assert worst_lp <= 2e-5
    assert worst_ent <= ENT_BOUND and worst_f32 <= ENT_BOUND


def test_bad_arguments_raise(tiny_engine):
    e = tiny_engine
    buf = torch.zeros((2, 77), dtype=torch.bfloat16, device="cuda")            # ld = 77
    tg = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(ZoomEarthError, match="score_detail"):
        e.op_score_detail(buf, tg, 0)
    ok = torch.zeros((2, 80), dtype=torch.bfloat16, device="cuda")
    for n in (-1, 21):
        with pytest.raises(ZoomEarthError, match="top_n"):
            e.op_score_detail(ok, tg, n)


# ---------------------------------------------------------------- 3. model level: the tiny engine, bit equality
def text_ids(seed, n):
    from oracle import prng
    return [int(t) for t in prng.uniform_ints(seed, n, 10, 1990)]


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


def _detail(e, slots, seqs, sf=None, top_n=5):
    pl = [e.rope_index(ids, []) for ids in seqs]
    for s in slots:
        e.seq_reset(s)
    return e.score_batch_detail(slots, seqs, [None] * len(seqs), [p[0] for p in pl], [p[1] for p in pl], sf, top_n=top_n,
                                entropy=True, rank=True)


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a[:5], b[:5]))


@pytest.fixture(scope="module")
def small_engine():
    """max_prefill_rows 256: the MLP workspace holds 172 rows of 2048 logits, 128 per lm_head launch (ze_score_chunk_rows)"""
    cfg = ModelConfig.tiny()
    e = Engine(cfg, device=0, max_seqs=3, max_ctx=256, max_patches=1024, max_tile_side=1024)
    e.fill_synthetic(**CHAIN_W)
    cap = e.max_prefill_rows * cfg.text.intermediate_size // cfg.text.vocab_size
    assert (cap & ~127 if cap >= 128 else cap) == 128
    yield e
    e.close()


def test_a_chains_outputs_do_not_depend_on_the_pass_the_chunk_or_the_other_chains(small_engine):
    e = small_engine
    lens = [80, 90, 70]
    seqs = [text_ids(940 + i, n) for i, n in enumerate(lens)]
    alone = [_detail(e, [0], [ids]) for ids in seqs]
    for i, ids in enumerate(seqs):                                 # logps: the bits of score_batch
        pos, delta = e.rope_index(ids, [])
        e.seq_reset(0)
        flat, _ = e.score_batch([0], [ids], [None], [pos], [delta])
        assert torch.equal(_bits(flat), _bits(alone[i].logps))
    # 79 + 89 + 69 = 237 scored rows: the chunk boundary at 128 falls between rows of chain 1; then other first positions
    for sf in ([0, 0, 0], [40, 0, 30], [0, 88, 3]):
        d = _detail(e, [2, 0, 1], seqs, sf)
        assert d.offsets[-1] == sum(n - 1 - f for n, f in zip(lens, sf))
        for i in range(3):
            mine, want = d.chain(i), alone[i]
            assert _same(mine, [x[sf[i]:] for x in want[:5]]), (sf, i)
    # rank 0: the first place is the target, with the log-probability's bits
    d = alone[1]
    targets = torch.tensor(seqs[1][1:], dtype=torch.int32)
    top = d.rank.cpu() == 0
    assert torch.equal(d.top_ids.cpu()[top, 0], targets[top])
    assert torch.equal(_bits(d.top_logprobs)[top, 0], _bits(d.logps)[top])
    hit = d.top_ids.cpu() == targets[:, None]                       # wherever the target is among the places: its place is its rank
    assert torch.equal(hit.float().argmax(1)[hit.any(1)], d.rank.cpu()[hit.any(1)].long())
    assert float(d.entropy.min()) > 0 and float(d.entropy.max()) <= np.log(2048) + 1e-3


def test_nothing_asked_is_score_batch_and_the_chain_goes_on_as_after_prefill_batch(small_engine):
    e = small_engine
    seqs = [text_ids(950 + i, n) for i, n in enumerate((33, 140, 71))]
    pl = [e.rope_index(ids, []) for ids in seqs]
    args = ([0, 1, 2], seqs, [None] * 3, [p[0] for p in pl], [p[1] for p in pl])
    for s in range(3):
        e.seq_reset(s)
    flat, off = e.score_batch(*args, [0, 100, 3])
    for s in range(3):
        e.seq_reset(s)
    none = e.score_batch_detail(*args, [0, 100, 3])
    assert none.entropy is None and none.rank is None and none.top_ids is None and none.offsets == off
    assert torch.equal(_bits(none.logps), _bits(flat))
    _detail(e, [0, 1, 2], seqs, [0, 100, 3], top_n=20)
    got = [e.generate(s, 8, ignore_eos=True) for s in range(3)]
    for s in range(3):
        e.seq_reset(s)
    e.prefill_batch(*args)
    assert got == [e.generate(s, 8, ignore_eos=True) for s in range(3)] and all(len(t) == 8 for t in got)
    with pytest.raises(ZoomEarthError, match="top_n"):
        _detail(e, [0], [seqs[0]], top_n=21)
    with pytest.raises(ZoomEarthError, match="score_from"):
        _detail(e, [0], [seqs[0]], [33])


def test_per_token_details_pads_as_per_token_logps_and_keeps_its_bits(small_engine):
    from zoomearth_amd.modeling import ZoomEarthForConditionalGeneration as M
    e = small_engine
    m = M(e.config, e)
    pad = e.config.pad_token_id
    seqs = [text_ids(960, 21), text_ids(961, 30), text_ids(962, 9)]
    L = 34
    left = (4, 0, 2)
    rows = [[pad] * left[i] + ids + [pad] * (L - left[i] - len(ids)) for i, ids in enumerate(seqs)]
    mask = [[0] * left[i] + [1] * len(ids) + [0] * (L - left[i] - len(ids)) for i, ids in enumerate(seqs)]
    inp, am = torch.tensor(rows), torch.tensor(mask)
    for k in (None, 12):
        want = m.per_token_logps(inp, am, score_from=k)
        d = m.per_token_details(inp, am, score_from=k, top_n=3, entropy=True, rank=True)
        assert set(d) == {"logps", "entropy", "rank", "top_ids", "top_logprobs"}
        assert torch.equal(_bits(d["logps"]), _bits(want)) and d["top_ids"].shape == (3, L - 1, 3)
        scored = want != 0
        assert torch.equal(d["entropy"] > 0, scored) and torch.equal(d["rank"] >= 0, scored)
        assert torch.equal((d["top_ids"] >= 0).all(-1), scored) and torch.isneginf(d["top_logprobs"][~scored]).all()
        first = d["rank"] == 0
        assert torch.equal(_bits(d["top_logprobs"][..., 0])[first], _bits(d["logps"])[first])
    ent = m.per_token_details(inp, am)                              # the default: entropy alone
    assert set(ent) == {"logps", "entropy"} and torch.equal(_bits(ent["entropy"]), _bits(m.per_token_details(inp, am, rank=True)["entropy"]))


# ---------------------------------------------------------------- 4. the scheduler and the server
@pytest.fixture(scope="module")
def stack():
    from tiny_tok import make_tokenizer
    from zoomearth_amd.modeling import ZoomEarthForConditionalGeneration
    from zoomearth_amd.processor import ZoomEarthProcessor
    model = ZoomEarthForConditionalGeneration.from_synthetic(ModelConfig.tiny(), **CHAIN_W, max_seqs=4, max_ctx=2048,
                                                            max_patches=4096, max_tile_side=2048)
    proc = ZoomEarthProcessor(make_tokenizer(), min_pixels=3136, max_pixels=128 * 128 * 28 * 28)
    proc.tokenizer.padding_side = "left"
    yield model, proc
    model.engine.close()


def words(seed, n):
    from oracle import prng
    return " ".join(f"w{int(v)}" for v in prng.uniform_ints(seed, n, 10, 1990))


def test_scheduler_scores_the_asking_prompt_and_leaves_the_others_alone(stack):
    from zoomearth_amd.scheduler import ChainScheduler, Request
    model, proc = stack
    e = model.engine
    prompts = [words(60 + i, n) for i, n in enumerate((14, 23, 9))]

    def run(ask):
        sched = ChainScheduler(model, proc, burst=4, share_prefix=False)
        reqs = [Request(prompt=p, images=[], max_new_tokens=6, prompt_logprobs=2 if (ask and i == 1) else None)
                for i, p in enumerate(prompts) if ask or i != 1]
        for r in reqs:
            sched.submit(r)
        sched.run()
        return reqs

    with_asker, without = run(True), run(False)
    assert [with_asker[0].tokens, with_asker[2].tokens] == [without[0].tokens, without[1].tokens]
    r = with_asker[1]
    ids = proc(text=[prompts[1]], return_tensors="pt")["input_ids"][0].tolist()
    pos, delta = e.rope_index(ids, [])
    e.seq_reset(0)
    want, _ = e.score_batch([0], [ids], [None], [pos], [delta])
    assert r.prompt_token_logprobs[0] is None and r.prompt_ranks[0] is None and len(r.prompt_token_logprobs) == len(ids) == r.n_prompt
    got = np.asarray(r.prompt_token_logprobs[1:], dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), want.cpu().numpy().view(np.uint32))
    assert all(len(t) == 2 and t[0][1] >= t[1][1] for t in r.prompt_top_logprobs[1:])
    for t in range(1, len(ids)):
        if r.prompt_ranks[t] < 2:
            assert r.prompt_top_logprobs[t][r.prompt_ranks[t]][0] == ids[t]
    assert len(r.tokens) == 6 and not with_asker[0].prompt_token_logprobs


def test_server_returns_vllms_prompt_logprobs_list(stack):
    from fastapi.testclient import TestClient
    from zoomearth_amd import serve
    model, proc = stack
    client = TestClient(serve.create_app(serve.ChatServer(model, proc, "ZoomEarth")))
    msgs = [{"role": "user", "content": words(71, 12)}]

    def ask(**kw):
        r = client.post("/v1/chat/completions", json={"model": "ZoomEarth", "messages": msgs, "max_tokens": 6, **kw})
        return r.status_code, r.json()

    code, plain = ask()
    assert code == 200 and "prompt_logprobs" not in plain
    for bad in (21, -1, "2", True, 1.5):
        assert ask(prompt_logprobs=bad)[0] == 400
    code, res = ask(prompt_logprobs=2)
    assert code == 200 and res["choices"] == plain["choices"] and res["usage"] == plain["usage"]
    ids = proc(text=[serve.build_prompt(msgs)[0]], return_tensors="pt")["input_ids"][0].tolist()
    plp = res["prompt_logprobs"]
    assert len(plp) == len(ids) and plp[0] is None
    e = model.engine
    pos, delta = e.rope_index(ids, [])
    e.seq_reset(0)
    want = e.score_batch([0], [ids], [None], [pos], [delta])[0].cpu().numpy()
    tok = proc.tokenizer
    for t in range(1, len(ids)):
        mine = plp[t][str(ids[t])]
        assert np.float32(mine["logprob"]) == want[t - 1] and mine["rank"] >= 1
        assert mine["decoded_token"] == tok.decode([ids[t]], skip_special_tokens=False)
        assert 2 <= len(plp[t]) <= 3 and sorted(v["rank"] for k, v in plp[t].items() if k != str(ids[t]) or v["rank"] <= 2)[:2] == [1, 2]


def test_rollout_entropies_come_from_the_same_planned_call(stack):
    from oracle import prng
    from test_gpu_infer_e2e import word
    from test_gpu_rollout import bbox_tokenizer
    from zoomearth_amd import hostloop as H
    from zoomearth_amd.image import DeviceImage
    from zoomearth_amd.processor import ZoomEarthProcessor
    from zoomearth_amd.rollout import rollout_two_stage
    model, _ = stack
    proc = ZoomEarthProcessor(bbox_tokenizer(), min_pixels=3136, max_pixels=128 * 128 * 28 * 28)
    tile = DeviceImage.from_numpy(prng.synthetic_tile(91, 500, 640), model.engine)
    q = " ".join(word(int(v)) for v in prng.uniform_ints(80, 5, 0, 1999))
    samples = [dict(prompt=H.stage1_prompt(q), image=tile, bbox=[])]
    kw = dict(num_generations=2, temperature=0.9, max_new_tokens=5, seed=11)
    plain = rollout_two_stage(model, proc, samples, **kw)
    passes = model.last_score_stats["passes"]
    ros = rollout_two_stage(model, proc, samples, entropies=True, **kw)
    assert model.last_score_stats["passes"] == passes and all(r.error is None for r in ros)
    for a, b in zip(plain, ros):
        assert a.entropies is None and torch.equal(_bits(a.logps), _bits(b.logps))
        assert b.entropies.shape == b.logps.shape and b.entropies.dtype == torch.float32 and bool((b.entropies > 0).all())

"""GPU: batched rollout scoring (ze_score_batch, Engine.score_batch, model.score_sequences) on the tiny config.

Everything here is BIT equality with ze_score (Engine.score) of a chain alone: the batched prefill is bit-identical per chain to
the single-chain one, the GEMM family accumulates every output element in the same K order whatever tile serves a row count, the
gathering norm shares the row norm's arithmetic, and the log-softmax pick is a function of its row alone.  The one tolerance is
the fixture's own (tests/test_gpu_score.py): within 2 x E_hf of the transformers fp32 log-probabilities."""
import os
import re

import numpy as np
import pytest
import torch

from gpu_util import CHAIN_W, tiny_engine, tiny_weights  # noqa: F401
from oracle import prng
from test_gpu_model import chain  # noqa: F401
from zoomearth_amd._lib import ZoomEarthError
from zoomearth_amd.config import ModelConfig
from zoomearth_amd.engine import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def prefill_tile_rows():
    """Query rows per attention tile of a prefill pass (prefill_bq, ze_forward.hip: ZE_FA_BQ_LONG unless a tuning knob is set)."""
    with open(os.path.join(ROOT, "zoomearth_amd", "csrc", "ze_kernels.h"), encoding="utf-8") as f:
        bq = int(re.search(r"#define\s+ZE_FA_BQ_LONG\s+(\d+)", f.read()).group(1))
    with open(os.path.join(ROOT, "zoomearth_amd", "csrc", "ze_forward.hip"), encoding="utf-8") as f:
        assert re.search(r"static int prefill_bq\(\) \{ return .* \? 64 : ZE_FA_BQ_LONG; \}", f.read())
    return bq


@pytest.fixture(scope="module")
def eng8():
    e = Engine(ModelConfig.tiny(), device=0, max_seqs=8, max_ctx=1024, max_patches=4096, max_tile_side=5200)
    e.fill_synthetic(**CHAIN_W)
    yield e
    e.close()


def text_ids(seed, n):
    return [int(t) for t in prng.uniform_ints(seed, n, 10, 1990)]


def score_alone(e, ids, emb=None, grids=(), slot=0):
    pos, delta = e.rope_index(ids, list(grids))
    e.seq_reset(slot)
    return e.score(slot, ids, emb, pos, delta)


def batch(e, slots, seqs, score_from=None, embs=None, grids=None, reset=True):
    pl = [e.rope_index(ids, list(grids[i]) if grids else []) for i, ids in enumerate(seqs)]
    if reset:
        for s in slots:
            e.seq_reset(s)
    return e.score_batch(slots, seqs, embs or [None] * len(seqs), [p[0] for p in pl], [p[1] for p in pl], score_from)


# ---------------------------------------------------------------- 1. bit equality, text only
def test_text_chains_equal_score_alone_bit_for_bit(eng8):
    e = eng8
    bq = prefill_tile_rows()
    lens = [1, 2, 3, bq - 1, bq, bq + 1, 2 * bq + 1]
    seqs = [text_ids(500 + i, n) for i, n in enumerate(lens)]
    alone = [score_alone(e, ids).clone() for ids in seqs]
    assert [a.numel() for a in alone] == [n - 1 for n in lens]
    flat, off = batch(e, list(range(7)), seqs, [0] * 7)
    assert off == np.concatenate([[0], np.cumsum([n - 1 for n in lens])]).tolist() and flat.numel() == off[-1]
    for i in range(7):
        assert torch.equal(flat[off[i]:off[i + 1]], alone[i]), lens[i]
    none_flat, none_off = batch(e, list(range(7)), seqs, None)            # NULL score_from = 0 everywhere
    assert none_off == off and torch.equal(none_flat, flat)
    # another order, other slots, mixed first positions: every scored value keeps its bits
    order = [6, 2, 4, 0, 5, 1, 3]
    slots = [3, 7, 0, 5, 1, 6, 2]
    sf = {6: bq, 2: 2, 4: 0, 0: 0, 5: bq, 1: 0, 3: (bq - 1) // 2}       # chain 2 (3 ids) and chain 0 (1 id): len - 1, nothing
    flat2, off2 = batch(e, slots, [seqs[i] for i in order], [sf[i] for i in order])
    for k, i in enumerate(order):
        assert off2[k + 1] - off2[k] == lens[i] - 1 - sf[i]
        assert torch.equal(flat2[off2[k]:off2[k + 1]], alone[i][sf[i]:]), (lens[i], sf[i])


# ---------------------------------------------------------------- 2. images and the pinned reference
def _image_inputs(e, chain, golden_npz):
    s = golden_npz("score.npz")
    ids = s["ids"].tolist()
    grids = [chain["g_v"], chain["g_c"]]
    feats = [e.vit_forward(chain["pv_v"], [chain["g_v"]]), e.vit_forward(chain["pv_c"], [chain["g_c"]])]
    both = e.vit_forward(torch.cat([chain["pv_v"], chain["pv_c"]]), grids)
    assert torch.equal(torch.cat(feats), both)
    return s, ids, grids, feats, both


def test_two_image_sequence_shares_a_pass_and_meets_the_fixture_bound(tiny_engine, chain, golden_npz):
    e = tiny_engine
    s, ids, grids, feats, emb = _image_inputs(e, chain, golden_npz)
    full = score_alone(e, ids, emb, grids).clone()
    texts = [text_ids(520, 37), text_ids(521, 150)]
    t_alone = [score_alone(e, t).clone() for t in texts]
    seqs, embs, gl = [texts[0], ids, texts[1]], [None, emb, None], [[], grids, []]
    flat, off = batch(e, [2, 0, 1], seqs, [0, 0, 0], embs, gl)
    assert torch.equal(flat[off[1]:off[2]], full)
    assert torch.equal(flat[off[0]:off[1]], t_alone[0]) and torch.equal(flat[off[2]:off[3]], t_alone[1])
    k = int(s["prompt_len"]) - 1
    flat, off = batch(e, [2, 0, 1], seqs, [5, k, len(texts[1]) - 1], embs, gl)
    tail = flat[off[1]:off[2]]
    assert tail.numel() == len(ids) - 1 - k and torch.equal(tail, full[k:])
    assert torch.equal(flat[off[0]:off[1]], t_alone[0][5:]) and off[3] == off[2]
    ref32, ref16 = s["logps_fp32"], s["logps_bf16_logits_fp32_softmax"]
    e_hf = np.abs(ref16 - ref32).max()
    e_me = np.abs(tail.cpu().numpy() - ref32[k:]).max()
    print(f"max|score_batch tail - fp32| = {e_me:.4f}, E_hf = {e_hf:.4f}, ratio {e_me / e_hf:.3f} of the 2.0 allowed")
    assert e_me <= 2.0 * e_hf


# ---------------------------------------------------------------- 3. cached prefix
def test_tail_behind_a_copied_prefix_equals_the_whole_sequence(tiny_engine, chain, golden_npz):
    e = tiny_engine
    s, ids, grids, feats, emb = _image_inputs(e, chain, golden_npz)
    img = e.config.image_token_id
    is_img = np.asarray(ids) == img
    starts = np.nonzero(is_img & ~np.concatenate([[False], is_img[:-1]]))[0]
    ends = np.nonzero(is_img & ~np.concatenate([is_img[1:], [False]]))[0] + 1
    assert len(starts) == 2
    full = score_alone(e, ids, emb, grids, slot=1).clone()               # chain B's whole sequence, alone
    pos, delta = e.rope_index(ids, grids)
    # chain A: the same beginning, then ids of its own behind the second image block
    a_ids = ids[: int(ends[1]) + 1] + text_ids(530, 9)
    pa, da = e.rope_index(a_ids, grids)
    e.seq_reset(0)
    e.prefill(0, a_ids, emb, pa, da, want_logits=False)
    # p before the second image run (its rows are prefilled by B), right behind it, and one further
    for p, n_cached_images in ((int(starts[1]), 1), (int(ends[1]), 2), (int(ends[1]) + 1, 2)):
        e.seq_reset(1)
        e.seq_copy_prefix(1, 0, p)
        rest = feats[n_cached_images:]
        flat, off = e.score_batch([1], [ids[p:]], [torch.cat(rest) if rest else None], [pos[:, p:]], [delta], [0])
        assert off == [0, len(ids) - p - 1]
        assert torch.equal(flat, full[p:]), p
        mid = (len(ids) - p) // 2                                          # ... and from a later position of the tail
        e.seq_reset(1)
        e.seq_copy_prefix(1, 0, p)
        flat, off = e.score_batch([1], [ids[p:]], [torch.cat(rest) if rest else None], [pos[:, p:]], [delta], [mid])
        assert torch.equal(flat, full[p + mid:]), (p, mid)


# ---------------------------------------------------------------- 4. more than one logits chunk, and none
def test_scored_rows_beyond_one_logits_chunk_and_a_pass_without_any():
    cfg = ModelConfig.tiny()
    e = Engine(cfg, device=0, max_seqs=3, max_ctx=256, max_patches=1024, max_tile_side=1024)
    try:
        e.fill_synthetic(**CHAIN_W)
        # the lm_head writes its bf16 logits into the MLP workspace: max_prefill_rows x intermediate elements hold
        # 256 * 1376 / 2048 = 172 rows of 2048 logits, rounded down to 128 per launch (ze_score_chunk_rows)
        cap = e.max_prefill_rows * cfg.text.intermediate_size // cfg.text.vocab_size
        chunk = cap & ~127 if cap >= 128 else cap
        assert chunk == 128
        lens = [80, 90, 70]
        scored = sum(lens) - 3
        assert sum(lens) <= e.max_prefill_rows and scored > chunk and (scored % chunk) % 8 != 0   # 128 + 109: a ragged last chunk
        seqs = [text_ids(540 + i, n) for i, n in enumerate(lens)]
        alone = [score_alone(e, ids).clone() for ids in seqs]
        flat, off = batch(e, [0, 1, 2], seqs, [0, 0, 0])
        for i in range(3):
            assert torch.equal(flat[off[i]:off[i + 1]], alone[i]), i
        # zero scored rows: OK, nothing comes back, and the chains are where prefill_batch leaves them
        flat, off = batch(e, [0, 1, 2], seqs, [n - 1 for n in lens])
        assert flat.numel() == 0 and off == [0, 0, 0, 0]
        got = [e.generate(sl, 6, ignore_eos=True) for sl in range(3)]
        pl = [e.rope_index(ids, []) for ids in seqs]
        for sl in range(3):
            e.seq_reset(sl)
        e.prefill_batch([0, 1, 2], seqs, [None] * 3, [p[0] for p in pl], [p[1] for p in pl])
        assert got == [e.generate(sl, 6, ignore_eos=True) for sl in range(3)]
    finally:
        e.close()


# ---------------------------------------------------------------- 5. chains continue
def test_chains_continue_after_score_batch(eng8):
    e = eng8
    seqs = [text_ids(550 + i, n) for i, n in enumerate((33, 140, 71))]
    batch(e, [4, 1, 6], seqs, [0, 100, 3])
    assert [e.seq_len(s) for s in (4, 1, 6)] == [33, 140, 71]
    got = [e.generate(s, 8, ignore_eos=True) for s in (4, 1, 6)]
    pl = [e.rope_index(ids, []) for ids in seqs]
    for s in (4, 1, 6):
        e.seq_reset(s)
    e.prefill_batch([4, 1, 6], seqs, [None] * 3, [p[0] for p in pl], [p[1] for p in pl])
    want = [e.generate(s, 8, ignore_eos=True) for s in (4, 1, 6)]
    assert got == want and all(len(t) == 8 for t in got)


# ---------------------------------------------------------------- 6. errors
def test_errors_are_raised_before_anything_runs(eng8):
    e = eng8
    a, b = text_ids(560, 20), text_ids(561, 12)
    for s in (0, 1):
        e.seq_reset(s)
    for sf in ([-1, 0], [0, 12], [20, 0]):
        with pytest.raises(ZoomEarthError, match="score_from"):
            batch(e, [0, 1], [a, b], sf)
    with pytest.raises(ZoomEarthError, match="twice"):
        batch(e, [1, 1], [a, b], [0, 0])
    big = [text_ids(562 + i, 600) for i in range(2)]
    assert 1200 > e.max_prefill_rows
    with pytest.raises(ZoomEarthError, match="max_prefill_rows"):
        batch(e, [0, 1], big, [0, 0])
    assert e.seq_len(0) == 0 and e.seq_len(1) == 0                        # no chain moved
    flat, off = batch(e, [0, 1], [a, b], [19, 11], reset=False)           # the largest legal values
    assert flat.numel() == 0 and e.seq_len(0) == 20 and e.seq_len(1) == 12


# ---------------------------------------------------------------- 7. callers
def test_per_token_logps_equals_the_score_loop(eng8):
    from zoomearth_amd.modeling import ZoomEarthForConditionalGeneration as M

    e = eng8
    m = M(e.config, e)
    pad = e.config.pad_token_id
    head = text_ids(570, 80)
    seqs = [head + text_ids(571, 21), text_ids(572, 95), head + text_ids(573, 30), text_ids(574, 9)]
    L = 118
    rows, mask = [], []
    for i, ids in enumerate(seqs):
        left = (4, 0, 2, 0)[i]
        rows.append([pad] * left + ids + [pad] * (L - left - len(ids)))
        mask.append([0] * left + [1] * len(ids) + [0] * (L - left - len(ids)))
    inp, am = torch.tensor(rows), torch.tensor(mask)
    # the parent's loop: one chain at a time through slot 0, scattered by the layout rule (value j -> column valid[j + 1] - 1)
    want = torch.zeros(4, L - 1)
    for b, ids in enumerate(seqs):
        valid = np.nonzero(np.asarray(mask[b]))[0]
        want[b, torch.as_tensor(valid[1:] - 1)] = score_alone(e, ids).cpu()
    for share in (True, False):
        assert torch.equal(m.per_token_logps(inp, am, share_prefix=share).cpu(), want)
    k = 84
    for share in (True, False):
        got = m.per_token_logps(inp, am, score_from=k, share_prefix=share).cpu()
        assert torch.equal(got[:, k:], want[:, k:]) and torch.equal(got[:, :k], torch.zeros(4, k))
        # row 2 copies the 80 common rows of row 0 (its first scored value sits at column 84: position 82 of its ids)
        assert m.last_score_stats["shared_rows"] == (80 if share else 0)
    assert (want[0, k:] != 0).any() and (want[2, k:] != 0).any() and not want[3].abs().sum() == 0


def test_rollout_logps_equal_the_per_chain_loop(eng8):
    from test_gpu_infer_e2e import word
    from test_gpu_rollout import bbox_tokenizer
    from zoomearth_amd import hostloop as H
    from zoomearth_amd.image import DeviceImage
    from zoomearth_amd.modeling import ZoomEarthForConditionalGeneration as M
    from zoomearth_amd.processor import ZoomEarthProcessor
    from zoomearth_amd.rollout import rollout_two_stage

    e = eng8
    model = M(e.config, e)
    proc = ZoomEarthProcessor(bbox_tokenizer(), min_pixels=3136, max_pixels=128 * 128 * 28 * 28)
    tile = DeviceImage.from_numpy(prng.synthetic_tile(91, 500, 640), e)
    samples = []
    for i in range(2):
        q = " ".join(word(int(v)) for v in prng.uniform_ints(80 + i, 5, 0, 1999))
        samples.append(dict(prompt=H.stage1_prompt(q), image=tile, bbox=[1, 2, 3, 4] if i == 0 else []))
    G = 3
    ros = rollout_two_stage(model, proc, samples, num_generations=G, temperature=0.9, max_new_tokens=6, seed=11)
    assert len(ros) == 2 * G and all(r.error is None for r in ros)
    stats = model.last_score_stats
    assert stats["shared_rows"] > 0 and all(n <= e.max_prefill_rows for n in stats["rows_per_pass"])
    for r in ros:
        prompt = r.prompt2 if r.prompt2 is not None else r.prompt1
        tail = r.completion2_ids if r.prompt2 is not None else r.completion1_ids
        inp = proc(text=[prompt], images=list(r.images), return_tensors="pt")
        ids = inp["input_ids"][0].tolist() + list(tail)
        grids = inp["image_grid_thw"].tolist()
        offs = np.concatenate([[0], np.cumsum([g[0] * g[1] * g[2] for g in grids])]).astype(int)
        feats = [e.vit_forward(inp["pixel_values"][offs[i]:offs[i + 1]].contiguous(), [grids[i]]) for i in range(len(grids))]
        want = score_alone(e, ids, torch.cat(feats) if len(feats) > 1 else feats[0], grids).cpu()[max(r.n_prompt1 - 1, 0):]
        assert r.logps.shape == want.shape and r.logps.shape[0] == len(ids) - r.n_prompt1
        assert torch.equal(r.logps.cpu(), want), (r.sample, r.generation)

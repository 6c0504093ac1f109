"""CPU: the planner of batched rollout scoring (zoomearth_amd/score_plan.py), the column mapping of per_token_logps with
score_from, the wrapper's pass bookkeeping on a stub engine, and the presence of the C entry point."""
import os
import re

import numpy as np
import pytest
import torch

from zoomearth_amd.scheduler import shared_prefix_len
from zoomearth_amd.score_plan import PlanItem, plan_score_passes, reader_prefix, score_columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG = 9


def _prompt(n_text=70, n_img=8):
    """A prompt with one image run: n_text text ids, n_img image tokens, three more text ids."""
    return list(range(100, 100 + n_text)) + [IMG] * n_img + [5, 6, 7]


def _check_limits(passes, items, max_rows, max_seqs):
    seen = []
    for p in passes:
        assert 1 <= len(p) <= max_seqs
        assert len({en.slot for en in p}) == len(p) and all(0 <= en.slot < max_seqs for en in p)
        assert sum(len(items[en.item].ids) - en.start for en in p) <= max_rows
        seen += [en.item for en in p]
    assert len(seen) == len(set(seen))
    return seen


def test_planner_splits_at_the_row_and_slot_limits():
    items = [PlanItem(list(range(1000 * i, 1000 * i + 30 + i)), [], 0) for i in range(7)]
    # rows: 30 + 31 + 32 = 93 <= 100 < 93 + 33
    passes = plan_score_passes(items, 100, 8, IMG)
    assert [[en.item for en in p] for p in passes] == [[0, 1, 2], [3, 4], [5, 6]]
    assert sorted(_check_limits(passes, items, 100, 8)) == list(range(7))
    # slots: two chains per pass however few the rows
    passes = plan_score_passes(items, 10000, 2, IMG)
    assert [[en.item for en in p] for p in passes] == [[0, 1], [2, 3], [4, 5], [6]]
    _check_limits(passes, items, 10000, 2)
    passes = plan_score_passes(items, 10000, 1, IMG)
    assert [len(p) for p in passes] == [1] * 7 and all(p[0].slot == 0 for p in passes)
    assert all(en.copy_from is None and en.start == 0 for p in passes for en in p)
    with pytest.raises(ValueError, match="max_prefill_rows"):
        plan_score_passes(items, 32, 8, IMG)
    with pytest.raises(ValueError, match="score_from"):
        plan_score_passes([PlanItem([1, 2, 3], [], 3)], 100, 8, IMG)
    # nothing to score: one id, or scored from the last position
    assert plan_score_passes([PlanItem([1], [], 0), PlanItem([1, 2, 3], [], 2), PlanItem([], [], 0)], 100, 8, IMG) == []


def test_planner_groups_only_when_ids_and_image_keys_agree():
    a = _prompt()
    n = len(a)
    items = [PlanItem(a + [1, 2, 3], ["k"], n - 1), PlanItem(a + [4, 5], ["k"], n - 1),     # same prompt, same image
             PlanItem(a + [4, 5, 8], ["other"], n - 1),                                      # same ids, another image
             PlanItem([7] + a[1:] + [1, 2], ["k"], n - 1),                                   # same image, ids differ at 0
             PlanItem(a + [6], [None], n - 1)]                                               # an image of unknown identity
    passes = plan_score_passes(items, 10000, 8, IMG, min_shared=16)
    by_item = {en.item: en for p in passes for en in p}
    assert by_item[1].copy_from == by_item[0].slot and by_item[1].start == n - 1 and by_item[1].n_images == 1
    for i in (0, 2, 3, 4):
        assert by_item[i].copy_from is None and by_item[i].start == 0 and by_item[i].n_images == 0
    # share_prefix off: nobody copies
    off = plan_score_passes(items, 10000, 8, IMG, share_prefix=False, min_shared=16)
    assert all(en.copy_from is None and en.start == 0 for p in off for en in p) and len(off) == 1
    # below the minimum length nothing is shared
    short = plan_score_passes(items, 10000, 8, IMG, min_shared=n + 5)
    assert all(en.copy_from is None for p in short for en in p)
    # text-only sequences share as well (no image to disagree about)
    t = list(range(200, 300))
    txt = plan_score_passes([PlanItem(t + [1, 2], [], 100), PlanItem(t + [3, 4], [], 100)], 10000, 4, IMG, min_shared=16)
    assert {en.item: (en.start, en.copy_from is not None) for p in txt for en in p} == {0: (0, False), 1: (100, True)}


def test_planner_never_shares_past_the_first_scored_position():
    a = _prompt()
    n = len(a)
    for sf in (0, 15, 16, 40, 69, n - 1, n):
        items = [PlanItem(a + [1, 2, 3], ["k"], 0), PlanItem(a + [4, 5, 6], ["k"], sf)]
        by_item = {en.item: en for p in plan_score_passes(items, 10000, 4, IMG, min_shared=16) for en in p}
        en = by_item[1]
        assert en.start <= sf and en.start <= n
        if sf < 16:
            assert en.copy_from is None and en.start == 0
        else:
            assert en.copy_from == by_item[0].slot
            assert en.start == min(sf, shared_prefix_len(items[0].ids, items[1].ids, IMG)) == min(sf, n)
        # the row of the first scored position is a NEW row of the reader's pass
        assert sf - en.start >= 0 and len(items[1].ids) - en.start >= 1


def test_planner_cuts_at_image_run_boundaries():
    a = _prompt(70, 8)                                     # image run = positions 70 .. 77
    long = a + [1, 2, 3, 4]
    anchor = PlanItem(long, ["k"], 0)
    for sf, want, imgs in ((70, 70, 0), (71, 70, 0), (74, 70, 0), (77, 70, 0), (78, 78, 1), (79, 79, 1)):
        assert reader_prefix(anchor, PlanItem(a + [8, 8, 8, 8], ["k"], sf), IMG, 16) == (want, imgs), sf
    # ids that part inside the run: cut back to the run's start
    inside = PlanItem(a[:74] + [3] * 20, ["k"], 80)
    assert reader_prefix(anchor, inside, IMG, 16) == (70, 0)
    # a cut behind the run needs the image's key; before it the key does not matter
    assert reader_prefix(anchor, PlanItem(a + [8, 8], ["z"], 80), IMG, 16) == (0, 0)
    assert reader_prefix(anchor, PlanItem(a + [8, 8], ["z"], 70), IMG, 16) == (70, 0)
    # both sequences keep a non-empty tail
    assert reader_prefix(anchor, PlanItem(long[:-1], ["k"], len(long) - 2), IMG, 16)[0] == len(long) - 2


def test_planner_orders_anchors_before_their_readers():
    G, S = 4, 5
    items = []
    for s in range(S):
        p = [1000 + s] + _prompt()[1:]
        for g in range(G):
            items.append(PlanItem(p + [20 + g] * (10 + g), [f"img{s}"], len(p) - 1))
    for max_seqs, max_rows in ((4, 10000), (16, 10000), (3, 200), (2, 120)):
        passes = plan_score_passes(items, max_rows, max_seqs, IMG, min_shared=16)
        assert sorted(_check_limits(passes, items, max_rows, max_seqs)) == list(range(S * G))
        where = {en.item: (pi, en) for pi, p in enumerate(passes) for en in p}
        holder = {}   # slot -> item whose rows it holds, as the passes run
        for pi, p in enumerate(passes):
            for en in p:
                if en.copy_from is not None:
                    # the slot copied from holds, at that moment, an anchor of the same sample prefilled whole in an earlier pass
                    src = holder[en.copy_from]
                    assert where[src][0] < pi and where[src][1].start == 0 and src // G == en.item // G
                    assert en.copy_from not in {x.slot for x in p}
            for en in p:
                holder[en.slot] = en.item
        assert sum(en.copy_from is not None for p in passes for en in p) == S * (G - 1)


def test_score_columns_with_padding_and_score_from():
    # a row of 8 columns: two left pads, five tokens, one right pad -> tokens at columns 2 .. 6, values at columns 2 .. 5
    valid = np.nonzero(np.array([0, 0, 1, 1, 1, 1, 1, 0]))[0]
    assert score_columns(valid, None) == (0, [2, 3, 4, 5])
    assert score_columns(valid, 0) == (0, [2, 3, 4, 5]) and score_columns(valid, 2) == (0, [2, 3, 4, 5])
    assert score_columns(valid, 3) == (1, [3, 4, 5])
    assert score_columns(valid, 5) == (3, [5])
    assert score_columns(valid, 6) == (4, []) and score_columns(valid, 99) == (4, [])
    # a hole in the mask: value j sits at the column before token j + 1
    valid = np.nonzero(np.array([1, 1, 0, 0, 1, 1]))[0]
    assert score_columns(valid, None) == (0, [0, 3, 4])
    assert score_columns(valid, 1) == (1, [3, 4]) and score_columns(valid, 3) == (1, [3, 4]) and score_columns(valid, 4) == (2, [4])
    assert score_columns(np.array([3]), None) == (0, [])


class _ScoreStub:
    """An engine whose score of a chain is a function of (token, position) alone: what per_token_logps scatters is checkable."""
    def __init__(self, max_seqs=4, max_prefill_rows=64):
        self.max_seqs, self.max_prefill_rows, self.device = max_seqs, max_prefill_rows, torch.device("cpu")
        self.ctx = {}
        self.calls = []

    def rope_index(self, ids, grids):
        return np.tile(np.arange(len(ids), dtype=np.int32), (3, 1)), 0

    def seq_reset(self, slot):
        self.ctx[slot] = 0

    def seq_copy_prefix(self, dst, src, n):
        assert self.ctx[src] >= n
        self.ctx[dst] = n

    def score_batch(self, seqs, ids_list, embeds_list, pos_list, deltas, score_from=None):
        assert len(set(seqs)) == len(seqs) <= self.max_seqs and sum(len(x) for x in ids_list) <= self.max_prefill_rows
        vals, off = [], [0]
        for s, ids, pos, sf in zip(seqs, ids_list, pos_list, score_from):
            assert pos.shape == (3, len(ids)) and int(pos[0, 0]) == self.ctx[s] and 0 <= sf <= len(ids) - 1
            vals += [-(1000.0 * ids[t + 1] + int(pos[0, t])) for t in range(sf, len(ids) - 1)]
            off.append(len(vals))
            self.ctx[s] += len(ids)
        self.calls.append((list(seqs), [len(x) for x in ids_list], list(score_from)))
        return torch.tensor(vals, dtype=torch.float32), off


def test_per_token_logps_scatter_on_a_stub_engine():
    from types import SimpleNamespace

    from zoomearth_amd.modeling import ZoomEarthForConditionalGeneration as M

    m = M.__new__(M)
    m.engine, m.config = _ScoreStub(), SimpleNamespace(image_token_id=IMG, pad_token_id=0)
    m._chains, m._next_slot = {}, 0
    P = 0
    base = list(range(11, 31))                                   # 20 shared ids
    rows = [[P, P] + base + [41, 42, 43] + [P],                  # left and right padding
            base + [51, 52] + [P, P, P, P],
            [P, P, P] + [61, 62, 63] + [P] * 20,                 # ends before column k below: contributes nothing there
            [71] + [P] * 25]                                     # one token
    mask = [[int(t != P) for t in r] for r in rows]
    ids, am = torch.tensor(rows), torch.tensor(mask)

    def want(k):
        out = torch.zeros(len(rows), ids.shape[1] - 1)
        for b, r in enumerate(rows):
            cols = [c for c in range(len(r)) if mask[b][c]]
            for j in range(len(cols) - 1):
                if cols[j + 1] - 1 >= k:
                    out[b, cols[j + 1] - 1] = -(1000.0 * r[cols[j + 1]] + j)
        return out

    assert torch.equal(m.per_token_logps(ids, am), want(0))
    assert m.last_score_stats["shared_rows"] == 0 and len(m.engine.calls) == 1
    for share in (True, False):
        m.engine.calls.clear()
        got = m.per_token_logps(ids, am, score_from=19, share_prefix=share, min_shared=8)
        assert torch.equal(got, want(19))
        assert torch.equal(got[:, :19], torch.zeros(len(rows), 19))
        # row 0 is scored from value 17 (column 2 + 17), row 1 from value 19: it copies 19 of the 20 common rows
        assert m.last_score_stats["shared_rows"] == (19 if share else 0)
        assert sum(len(c[0]) for c in m.engine.calls) == 2       # rows 2 and 3 never reach the engine


def test_new_symbol_is_in_the_header_and_the_loader():
    from zoomearth_amd import _lib

    with open(os.path.join(ROOT, "include", "zoomearth.h"), encoding="utf-8") as f:
        header = f.read()
    name = "ze_score_batch"
    assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert name in _lib._SIGS and name in _lib.EXPORTS
    assert len(_lib._SIGS[name][1]) == 12                        # engine, 8 of ze_prefill_batch, score_from, out, stream
    assert "bit-identical to the corresponding entries of ze_score" in header and "last CACHED row" in header
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert _lib.lib().ze_score_batch is not None
    with open(os.path.join(ROOT, "zoomearth_amd", "csrc", "Makefile"), encoding="utf-8") as f:
        mk = f.read()
    assert "ze_score.hip" in mk and "ze_rmsnorm.h" in mk

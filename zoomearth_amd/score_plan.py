"""Planning of batched rollout scoring: which sequences share a `ze_score_batch` pass, which chain slot each takes and which
leading K/V rows a sequence copies from another instead of prefilling them again.

A pure function of ids, image keys, first scored positions and the engine's two limits -- no engine, no tensors -- so that the
plan is testable on the CPU.  `ZoomEarthForConditionalGeneration.score_sequences` (modeling.py) carries a plan out.

The sharing rules are the scheduler's (`scheduler.shared_prefix_len`, `images_in`): a common id prefix that leaves every
sequence a non-empty tail, cut at image-run boundaries, of at least `min_shared` rows, with the same images (by key) inside it.
Scoring adds one rule: a shared prefix never reaches past a sequence's first scored position, because the logit row of that
position has to be computed in the sequence's own pass (a copied K/V row carries no hidden state).
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

from .scheduler import cut_at_image_run, images_in, shared_prefix_len


class PlanItem(NamedTuple):
    """One sequence as the planner sees it: its ids, the keys of its images in order (None: an image of unknown identity, never
    shared) and the first position whose next-token log-probability is wanted."""
    ids: Sequence[int]
    keys: Sequence
    score_from: int = 0


class PlanEntry(NamedTuple):
    """One chain of one pass: sequence `item` on chain slot `slot`; its first `start` rows are copied from slot `copy_from`
    (None: nothing is copied, start = 0), rows [start, len) are prefilled and scored from `score_from - start` on; `n_images`
    images lie inside the copied rows."""
    item: int
    slot: int
    start: int
    copy_from: Optional[int]
    n_images: int


def reader_prefix(anchor: PlanItem, reader: PlanItem, image_token_id: int, min_shared: int):
    """(rows, images) of `anchor`'s prefix that `reader` may copy, (0, 0) when there is nothing worth sharing."""
    n = shared_prefix_len(anchor.ids, reader.ids, image_token_id)
    n = cut_at_image_run(reader.ids, min(n, int(reader.score_from)), image_token_id)
    if n < max(1, min_shared):
        return 0, 0
    ni = images_in(reader.ids, n, image_token_id)
    if len(anchor.keys) < ni or len(reader.keys) < ni:
        return 0, 0
    if any(k is None for k in reader.keys[:ni]) or tuple(anchor.keys[:ni]) != tuple(reader.keys[:ni]):
        return 0, 0
    return n, ni


def plan_score_passes(items: Sequence[PlanItem], max_rows: int, max_seqs: int, image_token_id: int, share_prefix: bool = True,
                      min_shared: int = 64) -> List[List[PlanEntry]]:
    """Passes in the order they have to run.  Every pass holds at most `max_rows` new rows and at most `max_seqs` chains on
    distinct slots; an anchor -- a sequence others copy from -- is prefilled whole in an EARLIER pass than any of its readers
    and keeps its slot until the last of them has run.  A sequence with nothing to score (fewer than two ids, or scored
    from its last position) appears in no pass."""
    for i, it in enumerate(items):
        if len(it.ids) > max_rows:
            raise ValueError(f"a sequence of {len(it.ids)} rows exceeds max_prefill_rows = {max_rows}")
        if len(it.ids) and not 0 <= int(it.score_from) <= len(it.ids) - 1:
            raise ValueError(f"score_from = {it.score_from} outside [0, {len(it.ids) - 1}]")
    live = [i for i, it in enumerate(items) if int(it.score_from) < len(it.ids) - 1]
    # groups: the first sequence of a group is its anchor; (reader, rows, images) for those that copy from it
    groups, taken = [], set()
    probe = max(1, min_shared)
    for a, i in enumerate(live):
        if i in taken:
            continue
        readers = []
        if share_prefix and max_seqs >= 2:
            head = tuple(items[i].ids[:probe])
            for j in live[a + 1:]:
                if j in taken or items[j].score_from < probe or tuple(items[j].ids[:probe]) != head:
                    continue
                n, ni = reader_prefix(items[i], items[j], image_token_id, min_shared)
                if n:
                    readers.append((j, n, ni))
                    taken.add(j)
        groups.append((i, readers))

    passes: List[List[PlanEntry]] = []

    def pack(entries, slots, fixed=None):
        """Greedy, in order: (item, start, copy_from, images) onto `slots` (or the slot `fixed` names for the item)."""
        cur, rows, used = [], 0, set()
        for item, start, copy_from, ni in entries:
            need = len(items[item].ids) - start
            slot = fixed[item] if fixed else next((s for s in slots if s not in used), None)
            if cur and (rows + need > max_rows or slot is None or len(cur) >= max_seqs):
                passes.append(cur)
                cur, rows, used = [], 0, set()
                slot = fixed[item] if fixed else slots[0]
            cur.append(PlanEntry(item, slot, start, copy_from, ni))
            rows += need
            used.add(slot)
        if cur:
            passes.append(cur)

    # rounds: up to half the slots hold the anchors of the round, the others serve its readers and the lone sequences
    k_max = max(1, max_seqs // 2)
    g = 0
    while g < len(groups):
        anchors, others = [], []
        while g < len(groups) and (len(anchors) < k_max or not groups[g][1]):
            i, readers = groups[g]
            (anchors if readers else others).append((i, readers))
            g += 1
        slot_of = {i: s for s, (i, _) in enumerate(anchors)}
        pack([(i, 0, None, 0) for i, _ in anchors], None, fixed=slot_of)
        pool = list(range(len(anchors), max_seqs))
        rest = [(j, n, slot_of[i], ni) for i, readers in anchors for j, n, ni in readers] + [(i, 0, None, 0) for i, _ in others]
        rest.sort(key=lambda t: t[0])   # (the caller's order, so that the passes' results come back nearly in order)
        pack(rest, pool)
    return passes


def score_columns(valid, score_from: Optional[int]):
    """Where the values of one padded row go.  `valid`: the ascending column indices of the row's real tokens (attention
    mask 1); the sequence is the row's tokens at those columns, value j of its score -- log p(token j + 1 | tokens 0 .. j) --
    belongs to column valid[j + 1] - 1 of the [B, L - 1] result (the layout of the trainer's `_get_per_token_logps`).
    score_from = k keeps the columns >= k (the trainer's `[:, prompt_length - 1:]`).  Returns (first, columns): the
    sequence's first scored position and the columns of values first, first + 1, ..."""
    cols = [int(v) - 1 for v in valid[1:]]
    k = 0 if score_from is None else int(score_from)
    first = sum(1 for c in cols if c < k)
    return first, cols[first:]

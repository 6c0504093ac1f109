"""Beam search, restated in numpy float64: the semantics of `transformers` 5.15 `GenerationMixin._beam_search` with do_sample=False at
batch size 1 (generation/utils.py:3208-3560), which the device follows per group (zoomearth_amd/csrc/ze_beam.hip), plus the two
rules that are this project's own:

* the tie rule -- candidates are ordered by score descending, then by the flat index `beam * vocab + token` ascending (torch.topk
  promises no order among equal values; equal logits in one row give bit-equal scores);
* the slot assignment -- where a hypothesis lives.  HF gathers the whole cache into beam order every step; the device lets a parent
  with surviving children keep its first child (in candidate order) in its own slot and sends the other children to the slots whose
  hypothesis had no child, free slots in ascending order.  So no slot that is read in a step is written in it.

A `BeamGroup` is one prompt.  `step(logits)` takes the fp32 logits rows BY SLOT (row j = the hypothesis living in slot j, whose HF
beam index is `rank[j]`), and returns what the device's step returns plus the step's decision margin.

Decision margin.  TAU is the gap below which a comparison between two unequal keys may come out differently on the device, whose
fp32 log-softmax sums the vocabulary in another order.  Measured on tests/golden/beam_search.npz (tests/test_beam_search_cpu.py
::test_tau_is_derived_from_hf_fp32): the largest difference between HF's own fp32 `sequences_scores` and this float64 restatement on
the same logits is MEASURED_HF_FP32_VS_F64; TAU = 16 x that (the factor covers a different fp32 summation order over the
vocabulary).  A step is DECIDED when every comparison it makes between unequal keys -- neighbours in the candidate order down to the
first candidate that is not looked at, a new finished score against the pool's, the early-stop heuristic's two sides -- has a gap
above TAU.
"""
from __future__ import annotations

import numpy as np

MEASURED_HF_FP32_VS_F64 = 1.9e-06   # max |HF fp32 sequences_scores - float64 restatement| over the fixture (1.826e-06, rounded up)
TAU = 16 * MEASURED_HF_FP32_VS_F64  # = 3.04e-05

NEG = -1.0e9


def log_softmax64(row):
    x = np.asarray(row, np.float64)
    m = x.max()
    return (x - m) - np.log(np.exp(x - m).sum())


def assign_slots(parent_of_child):
    """parent_of_child[k] = the slot of the parent of child k (children in candidate order).  Returns slot_of_child: a parent keeps
    its first child, the other children take the childless slots in ascending order."""
    B = len(parent_of_child)
    has, slot_of = [False] * B, [-1] * B
    for k, pj in enumerate(parent_of_child):
        if not has[pj]:
            slot_of[k] = pj
            has[pj] = True
    free = [j for j in range(B) if not has[j]]
    for k in range(B):
        if slot_of[k] < 0:
            slot_of[k] = free.pop(0)
    return slot_of


def order_candidates(scores, flat):
    """Indices that sort by (score descending, flat index ascending)."""
    return np.lexsort((np.asarray(flat), -np.asarray(scores, np.float64)))


class BeamGroup:
    def __init__(self, num_beams, vocab, eos_ids, max_new_tokens, length_penalty=1.0, early_stopping=False, repetition_penalty=1.0,
                 prompt_ids=(), seen=None):
        assert early_stopping in (False, True, "never")
        self.B, self.vocab, self.eos = num_beams, vocab, [e for e in eos_ids if e < vocab]
        self.max_new, self.lp, self.early, self.pen = max_new_tokens, float(length_penalty), early_stopping, float(repetition_penalty)
        B = num_beams
        # by SLOT
        self.rank = list(range(B))
        self.score = [0.0] + [NEG] * (B - 1)
        self.tokens = [[] for _ in range(B)]
        self.bidx = [[] for _ in range(B)]
        base = set(int(t) for t in prompt_ids) if seen is None else set(seen)
        self.seen = [set(base) for _ in range(B)]
        # the finished list, best first: dicts(score, tokens, bidx, finished)
        self.fin = [dict(score=NEG, tokens=[], bidx=[], finished=False) for _ in range(B)]
        self.heur, self.n, self.done = True, 0, False
        self.K = max(2, 1 + len(eos_ids)) * B

    # -- one step; logits [B, >= vocab] by slot
    def step(self, logits):
        assert not self.done
        B, V, n = self.B, self.vocab, self.n
        gaps = []
        acc = np.empty((B, V), np.float64)
        for j in range(B):
            lp = log_softmax64(np.asarray(logits[j])[:V])
            if self.pen != 1.0 and self.seen[j]:
                idx = np.fromiter((t for t in self.seen[j] if t < V), int)
                lp[idx] = np.where(lp[idx] < 0, lp[idx] * self.pen, lp[idx] / self.pen)
            acc[j] = lp + self.score[j]
        flat = (np.asarray(self.rank)[:, None] * V + np.arange(V)[None, :]).reshape(-1)
        slot_of_flat = np.repeat(np.arange(B), V)
        sc = acc.reshape(-1)
        # the top K + 1 under the total order (K = HF's beams_to_keep: the candidates HF looks at; one more for the margin)
        K = min(self.K, sc.size)
        part = np.argpartition(-sc, min(K, sc.size - 1))[: K + 1] if sc.size > K + 1 else np.arange(sc.size)
        kth = sc[part].min()
        pool = np.nonzero(sc >= kth)[0]   # (every tie of the boundary value included, so the order below is the global one)
        order = pool[order_candidates(sc[pool], flat[pool])]
        top = order[:K]
        s_sorted = sc[order[: K + 1]]
        d = -np.diff(s_sorted)
        rows = slot_of_flat[order[: K + 1]]
        # (equal scores in ONE row are bit-equal on the device too -- the tie rule decides; across rows they are a gap of 0)
        gaps += [float(g) for i, g in enumerate(d) if g > 0 or rows[i] != rows[i + 1]]
        last = n + 1 >= self.max_new
        tok = flat[top] % V
        hits = np.array([bool(last or (t in self.eos)) for t in tok])
        # e. running beams: the best B that did not stop (at the last step all are masked alike: the first B)
        run = [i for i in range(len(top)) if last or not hits[i]][:B]
        assert len(run) == B, "fewer than num_beams continuations"
        # f. finished beams
        all_fin = all(f["finished"] for f in self.fin)
        admit = self.heur and not (all_fin and self.early is True)
        div = float(n + 1) ** self.lp
        merged = list(self.fin)
        for i in range(min(B, len(top))):
            if not hits[i] or not admit:
                continue
            j = int(slot_of_flat[top[i]])
            s = sc[top[i]] / div
            gaps += [abs(s - f["score"]) for f in merged if f["score"] != s]
            new = dict(score=s, tokens=self.tokens[j] + [int(tok[i])], bidx=self.bidx[j] + [self.rank[j]], finished=True)
            pos = len(merged)
            while pos > 0 and merged[pos - 1]["score"] < s:
                pos -= 1
            merged.insert(pos, new)
        self.fin = merged[:B]
        # the slots
        parents = [int(slot_of_flat[top[i]]) for i in run]
        slot_of = assign_slots(parents)
        new = {}
        for k, i in enumerate(run):
            j, pj = slot_of[k], parents[k]
            new[j] = dict(rank=k, parent=pj, token=int(tok[i]), score=float(sc[top[i]]) + (NEG if last else 0.0),
                          tokens=self.tokens[pj] + [int(tok[i])], bidx=self.bidx[pj] + [self.rank[pj]],
                          seen=self.seen[pj] | {int(tok[i])})
        out = dict(parent=[new[j]["parent"] for j in range(B)], token=[new[j]["token"] for j in range(B)],
                   score=[new[j]["score"] for j in range(B)], rank=[new[j]["rank"] for j in range(B)])
        for j in range(B):
            self.rank[j], self.score[j] = new[j]["rank"], new[j]["score"]
            self.tokens[j], self.bidx[j], self.seen[j] = new[j]["tokens"], new[j]["bidx"], new[j]["seen"]
        self.n = n + 1
        # g. the stop conditions, at the new length
        hyp_len = self.max_new if (self.early == "never" and self.lp > 0.0) else self.n
        best = out["score"][out["rank"].index(0)] / (float(hyp_len) ** self.lp)
        worst = min(f["score"] for f in self.fin)
        sides = [worst if f["finished"] else NEG for f in self.fin]
        if not last:
            gaps += [abs(best - w) for w in sides if best != w]
        self.heur = self.heur and any(best > w for w in sides)
        all_fin = all(f["finished"] for f in self.fin)
        self.done = (not self.heur) or (all_fin and self.early is True) or last
        out["done"] = self.done
        out["margin"] = min(gaps) if gaps else float("inf")
        out["decided"] = out["margin"] > TAU
        return out

    def results(self, num_return_sequences=1):
        return [dict(f) for f in self.fin[:num_return_sequences]]


def hf_equivalent_top(scores_flat, vocab, eos_ids, B):
    """HF's own way to the running beams: the top (1 + n_eos) * B (at least 2 B) candidates with the EOS ones masked by -1e9, then
    the top B of those.  Returns the flat indices, in order, under this file's tie rule."""
    sc = np.asarray(scores_flat, np.float64)
    K = max(2, 1 + len(eos_ids)) * B
    order = order_candidates(sc, np.arange(sc.size))[:K]
    masked = sc[order] + np.where(np.isin(order % vocab, list(eos_ids)), NEG, 0.0)
    second = np.lexsort((np.arange(len(order)), -masked))[:B]
    return [int(order[i]) for i in second]


def best_non_eos(scores_flat, vocab, eos_ids, B):
    """The device's way: the best B candidates that are no EOS id."""
    sc = np.asarray(scores_flat, np.float64)
    order = order_candidates(sc, np.arange(sc.size))
    return [int(i) for i in order if (i % vocab) not in eos_ids][:B]

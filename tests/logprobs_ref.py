"""Numpy restatement of the per-token log-probabilities (include/zoomearth.h, ze_seq_set_logprobs): a float64 log-softmax and
the top-N by (value descending, id ascending), places a row cannot fill with finite entries as (-1, -inf)."""
import numpy as np


def log_softmax64(row):
    x = np.asarray(row, dtype=np.float64)
    m = x.max()
    return x - m - np.log(np.exp(x - m).sum())


def top_n(row, n):
    """(ids int32 [n], values of `row` at them float64 [n]); -1 / -inf where fewer than n entries are finite."""
    x = np.asarray(row)
    ids = np.full(n, -1, dtype=np.int32)
    if n:
        order = np.lexsort((np.arange(x.size), -x.astype(np.float64)))[: n]   # value descending, then id ascending
        order = order[np.isfinite(x[order])]
        ids[: order.size] = order
    return ids


def token_logprobs_ref(logits, targets, n):
    """logits [rows, vocab], targets [rows] -> (logprob f64 [rows], top ids int32 [rows, n], top logprobs f64 [rows, n])."""
    logits = np.asarray(logits)
    rows = logits.shape[0]
    lp = np.zeros(rows, dtype=np.float64)
    ids = np.full((rows, n), -1, dtype=np.int32)
    tlp = np.full((rows, n), -np.inf, dtype=np.float64)
    for r in range(rows):
        ls = log_softmax64(logits[r])
        lp[r] = ls[int(targets[r])]
        ids[r] = top_n(logits[r], n)
        ok = ids[r] >= 0
        tlp[r, ok] = ls[ids[r, ok]]
    return lp, ids, tlp


def decided(logits, n):
    """Rows whose top-n id list does not hinge on an exact float32 tie at its end: the n-th and (n + 1)-th values differ."""
    logits = np.asarray(logits, dtype=np.float32)
    if n == 0 or n >= logits.shape[1]:
        return np.ones(logits.shape[0], dtype=bool)
    part = -np.partition(-logits, n, axis=1)[:, : n + 1]
    part.sort(axis=1)
    return part[:, 0] != part[:, 1]

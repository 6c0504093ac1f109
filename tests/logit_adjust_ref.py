"""The numpy float32 restatement of the logit adjustments (include/zoomearth.h, ze_seq_set_logit_adjust): every operation
rounded to float32 on its own, in the order the header gives."""
import numpy as np


def has_request(presence=0.0, frequency=0.0, bias=None, eos_masked=False) -> bool:
    return bool(np.float32(presence) != 0 or np.float32(frequency) != 0 or bias or eos_masked)


def adjust_row(l, counts=None, presence=0.0, frequency=0.0, bias=None, eos_ids=(), eos_masked=False):
    """l f32 [vocab]; counts [vocab] (None = all zero); bias: {id: value} or (id, value) pairs; EOS ids outside the row are
    ignored.  A row without a request comes back unchanged (not even l + 0, which would turn -0 into +0)."""
    l = np.asarray(l, dtype=np.float32)
    pairs = list(bias.items()) if hasattr(bias, "items") else list(bias or ())
    if not has_request(presence, frequency, pairs, eos_masked):
        return l.copy()
    c = np.zeros(l.shape, dtype=np.int64) if counts is None else np.asarray(counts).astype(np.int64)
    b = np.zeros(l.shape, dtype=np.float32)
    for i, v in pairs:
        b[int(i)] = np.float32(v)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.float32(frequency) * c.astype(np.float32)
        t = np.where(c > 0, t + np.float32(presence), t).astype(np.float32)
        a = ((l + b).astype(np.float32) - t).astype(np.float32)
    if eos_masked:
        for e in eos_ids:
            if 0 <= int(e) < l.shape[0]:
                a[int(e)] = -np.inf
    return a


def adjust_rows(l, counts=None, presence=0.0, frequency=0.0, bias=None, eos_ids=(), eos_masked=0):
    """adjust_row for every row of l [rows, vocab]: presence / frequency / eos_masked per row (scalars broadcast), bias a list
    per row (or None), counts [rows, vocab] or None."""
    l = np.asarray(l, dtype=np.float32)
    rows = l.shape[0]
    pr, fr = np.broadcast_to(np.asarray(presence, np.float32), (rows,)), np.broadcast_to(np.asarray(frequency, np.float32), (rows,))
    em = np.broadcast_to(np.asarray(eos_masked), (rows,))
    return np.stack([adjust_row(l[r], None if counts is None else counts[r], pr[r], fr[r], None if bias is None else bias[r],
                                eos_ids, bool(em[r])) for r in range(rows)])


def saturating_counts(tokens, vocab, cap=65535):
    """counts after the chain generated `tokens`: uint16, saturating."""
    c = np.bincount(np.asarray(tokens, dtype=np.int64), minlength=vocab)
    return np.minimum(c, cap).astype(np.uint16)


def argmax_lowest(a) -> int:
    """the sampler's tie rule: the largest value, the lowest id among equals (NaN never wins)"""
    a = np.asarray(a, dtype=np.float32)
    return int(np.argmax(np.where(np.isnan(a), -np.inf, a)))

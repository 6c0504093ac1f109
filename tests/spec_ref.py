"""numpy restatement of speculative decoding by prompt lookup (zoomearth_amd/csrc/ze_spec.hip): the drafter and the accept pass."""
import numpy as np


def draft(history, k, ngram_min=1, ngram_max=3, cap=None):
    """The draft for a chain whose history is `history` (prompt ids + generated ids).  For g = ngram_max down to ngram_min the most
    recent earlier occurrence of the last g ids that has at least one id behind it is looked for; the first g with one wins; the draft
    is what follows it, at most k ids, cut at the end of the history and at `cap` (the room the chain has left)."""
    h = [int(t) for t in history]
    n = len(h)
    for g in range(int(ngram_max), int(ngram_min) - 1, -1):
        if g >= n:
            continue
        tail = h[n - g:]
        for p in range(n - g - 1, -1, -1):   # the occurrence at n - g is the tail itself: nothing follows it
            if h[p:p + g] == tail:
                out = h[p + g:p + g + int(k)]
                return out if cap is None else out[:max(int(cap), 0)]
    return []


def penalised(row, seen, penalty):
    """HF's RepetitionPenaltyLogitsProcessor in float32: score < 0 ? score * p : score / p on the seen ids."""
    row = np.asarray(row, dtype=np.float32)
    if np.float32(penalty) == np.float32(1.0):
        return row
    p = np.float32(penalty)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(np.asarray(seen, dtype=bool), np.where(row < 0, row * p, row / p), row).astype(np.float32)


def argmax(row):
    """torch.argmax: the lowest index of the maximum, NaN entries never win; 0 for a row without a comparable entry."""
    row = np.asarray(row, dtype=np.float32)
    ok = ~np.isnan(row)
    if not ok.any():
        return 0
    m = row[ok].max()
    return int(np.flatnonzero(ok & (row == m))[0])


def accept(rows, drafted, seen, penalty=1.0, eos_ids=(), room=None, ignore_eos=False):
    """The accept pass of one chain: rows f32 [len(drafted) + 1, vocab] (row j: the logits behind the chain's last token for j = 0,
    behind draft id j - 1 otherwise), seen bool/uint8 [vocab] (updated in place).  Returns (emitted ids, finished)."""
    drafted = [int(t) for t in drafted]
    room = len(drafted) + 1 if room is None else max(int(room), 1)
    out, finished = [], False
    for j in range(len(drafted) + 1):
        tok = argmax(penalised(rows[j], seen, penalty))
        out.append(tok)
        seen[tok] = 1
        eos = (not ignore_eos) and tok in tuple(int(t) for t in eos_ids)
        finished = finished or eos
        if j == len(drafted) or tok != drafted[j] or eos or j + 1 >= room:
            break
    return out, finished

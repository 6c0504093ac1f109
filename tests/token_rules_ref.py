"""numpy / plain-Python restatement of the token rules (ze_seq_set_token_rules, ze_token_rules.hip): HF's
NoRepeatNGramLogitsProcessor and NoBadWordsLogitsProcessor over a history = context + generated ids, vLLM's stop sequences over
the generated ids alone, and the text-level cut of stop strings in HF's order (the first token after which the decoded text
holds a stop string)."""
import numpy as np


def banned_ids(history, n_context, n, ban_records):
    """The set of ids that are -inf before the next draw.  `n_context` does not matter to the bans (the history is one
    sequence); it is here so that callers pass the same description they give the kernel."""
    h = [int(t) for t in history]
    L = len(h)
    out = set()
    if n >= 1 and L >= n - 1:
        tail = h[L - (n - 1):] if n > 1 else []
        for j in range(n - 1, L):                       # j = index of the id that completed an n-gram
            if h[j - (n - 1): j] == tail:
                out.add(h[j])
    for rec in ban_records:
        rec = [int(t) for t in rec]
        m = len(rec)
        if m == 1 or (m - 1 <= L and h[L - (m - 1):] == rec[:-1]):
            out.add(rec[-1])
    return out


def ban_row(row, history, n_context, n, ban_records):
    """The row the sampler reads: the input bits with -inf exactly at the banned ids inside the vocabulary."""
    out = np.array(row, dtype=np.float32, copy=True)
    for i in banned_ids(history, n_context, n, ban_records):
        if 0 <= i < out.shape[0]:
            out[i] = -np.inf
    return out


def stop_hit(generated, stop_records, min_new=0):
    """Whether the chain finishes now: a whole record ends the GENERATED ids, and at least min_new ids were generated."""
    g = [int(t) for t in generated]
    if len(g) < min_new:
        return False
    return any(0 < len(r) <= len(g) and g[len(g) - len(r):] == [int(t) for t in r] for r in stop_records)


def first_hit(generated, stop_records, min_new=0):
    """Ids kept by a chain that stops at its first hit (None: it never stops)."""
    for n in range(1, len(generated) + 1):
        if stop_hit(generated[:n], stop_records, min_new):
            return n
    return None


def text_cut(decode, ids, strings):
    """HF's order at text level: -> (n, text before the earliest stop string) for the smallest n whose decoded ids[:n] holds one
    of `strings`, or None."""
    for n in range(1, len(ids) + 1):
        text = decode(ids[:n])
        at = [text.find(s) for s in strings if s in text]
        if at:
            return n, text[:min(at)]
    return None


def argmax_lowest(row):
    return int(np.argmax(np.where(np.isnan(row), -np.inf, row)))

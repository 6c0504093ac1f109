"""numpy restatement of the SAMPLED accept pass of speculative decoding (zoomearth_amd/csrc/ze_spec.hip, ze_seq_set_speculation_mode
mode 1 / ze_op_spec_accept_sampled): row j of a chain is drawn as the plain step's sampler draws it -- chain_sampling_ref.sample_row on
the row's fp32 logits under the chain's seen-set plus the tokens of rows 0 .. j - 1, at draw index index0 + j, behind the filter's cut
(sampling_filters_ref.filter_ref) -- and the walk is spec_ref.accept's: emit, mark seen, stop behind the last row, a token that is
not draft id j, an EOS id, or when the room is used up."""
import numpy as np

import chain_sampling_ref as C
import sampling_filters_ref as F

f32 = np.float32


def draw(logits, seen, temperature, penalty, seed, stream, index, top_k=0, top_p=1.0, min_p=0.0, near=None):
    """(token, CDF gap) of one row under the seen mask `seen`; near (a list): gets the number of tokens inside the filter's float64
    decision margins (sampling_filters_ref.filter_f64), where two correct selections may differ"""
    seen_ids = np.flatnonzero(np.asarray(seen)).tolist()
    if not temperature > 0.0:
        return C.sample_row(logits, seen_ids, 0.0, penalty, seed, stream, index)
    scores = C.scores_of(logits, seen_ids, penalty)
    if (0 < top_k < len(scores)) or top_p < 1.0 or min_p > 0.0:
        keep, _, _ = F.filter_ref(scores, temperature, top_k, top_p, min_p)
        if near is not None:
            near.append(int(F.filter_f64(scores, temperature, top_k, top_p, min_p)[1].sum()))
        scores = F.masked(scores, keep)
    return C.sample_row(scores, [], temperature, 1.0, seed, stream, index)   # (already penalised)


def accept_sampled(rows, drafted, seen, temperature, penalty=1.0, seed=0, stream=0, index0=0, eos_ids=(), room=None, ignore_eos=False,
                   top_k=0, top_p=1.0, min_p=0.0, near=None):
    """The sampled accept pass of one chain: rows f32 [len(drafted) + 1, vocab], seen bool/uint8 [vocab] (updated in place).  Returns
    (emitted ids, finished, the CDF gap of every draw made)."""
    drafted = [int(t) for t in drafted]
    room = len(drafted) + 1 if room is None else max(int(room), 1)
    out, gaps, finished = [], [], False
    for j in range(len(drafted) + 1):
        tok, gap = draw(rows[j], seen, temperature, penalty, seed, stream, index0 + j, top_k, top_p, min_p, near)
        out.append(tok)
        gaps.append(gap)
        seen[tok] = 1
        eos = (not ignore_eos) and tok in tuple(int(t) for t in eos_ids)
        finished = finished or eos
        if j == len(drafted) or tok != drafted[j] or eos or j + 1 >= room:
            break
    return out, finished, gaps


# ---- the cases of the unit test (tests/test_gpu_spec_sampling.py), shared with the CPU self-check
SHAPES = ((257, 257), (2049, 2056))   # vocab, ld
KS = (1, 8)
EOS = (2045, 2043)                    # ModelConfig.tiny(): inside the larger vocabulary only
# name, temperature, penalty, filter (top_k, top_p, min_p), what the draft does
CHAINS = (
    ("all accepted", 0.7, 1.0, (0, 1.0, 0.0)),
    ("none accepted", 0.7, 1.3, (0, 1.0, 0.0)),
    ("middle stop", 1.0, 1.3, (0, 1.0, 0.0)),
    ("eos inside the draft", 0.7, 1.0, (0, 1.0, 0.0)),
    ("room ends mid-draft", 0.7, 1.3, (0, 1.0, 0.0)),
    ("greedy row", 0.0, 1.3, (0, 1.0, 0.0)),
    ("seen flips a later row", 0.01, 1.3, (0, 1.0, 0.0)),
    ("filtered", 0.7, 1.3, (5, 0.9, 0.0)),
)
SEED0 = 4100


def unit_case(vocab, k):
    """The inputs of one launch and what the restatement makes of them: dict(logits [n * (k + 1), vocab], drafts, temperature, penalty,
    seed, stream, index0, filt (three lists), room, seen0 [n, vocab], want ids, fins, seen_after, gaps)."""
    n = len(CHAINS)
    rng = np.random.default_rng(77 + vocab + k)
    logits = (rng.standard_normal((n * (k + 1), vocab)) * 3).astype(f32)
    seen0 = (rng.random((n, vocab)) < 0.05).astype(np.uint8)
    eos = tuple(t for t in EOS if t < vocab)
    temperature = [c[1] for c in CHAINS]
    penalty = [c[2] for c in CHAINS]
    filt = [[c[3][i] for c in CHAINS] for i in range(3)]
    seed = [SEED0 + 7 * c for c in range(n)]
    stream = [c % 3 for c in range(n)]
    index0 = [0, 1, 7, 300, 2, 5, 0, 40]
    room = [k + 1] * n
    room[4] = max(1, min(2, k))
    drafts = []
    for c, (name, t, pen, (tk, tp, mp)) in enumerate(CHAINS):
        rows = logits[c * (k + 1):(c + 1) * (k + 1)]
        kw = dict(temperature=t, penalty=pen, seed=seed[c], stream=stream[c], top_k=tk, top_p=tp, min_p=mp)
        if name == "seen flips a later row":
            # row 0 draws d0 (40 against noise); row 1 holds d0 at 40 and x at 35: d0 is seen by then, 40 / 1.3 < 35, so x is drawn
            d0, x = 11, 200
            seen0[c, [d0, x]] = 0
            rows[0, d0] = 40.0
            rows[1, d0], rows[1, x] = 40.0, 35.0
            drafts.append([d0] * k)
            continue
        if name == "eos inside the draft" and eos:
            at = min(1, k - 1)
            rows[at, eos[0]] = 60.0     # the row draws the EOS id (and the draft names it: an accepted id that ends the walk)
        accept = {"all accepted": k, "none accepted": 0, "middle stop": k // 2, "eos inside the draft": k, "room ends mid-draft": k,
                  "greedy row": k, "filtered": k}[name]
        seen, d = seen0[c].copy(), []
        for j in range(accept):        # the restatement's own walk: the accepted prefix ...
            tok, _ = draw(rows[j], seen, index=index0[c] + j, **kw)
            d.append(tok)
            seen[tok] = 1
        if accept < k:                 # ... then one differing id (and ids behind it that are never reached)
            tok, _ = draw(rows[accept], seen, index=index0[c] + accept, **kw)
            d.append((tok + 1) % vocab if (tok + 1) % vocab not in eos else (tok + 2) % vocab)
            d += [int(t) for t in rng.integers(0, vocab, size=k - accept - 1)]
        drafts.append(d)
    want, fins, gaps, near, seen_after = [], [], [], [], seen0.copy()
    for c, (name, t, pen, (tk, tp, mp)) in enumerate(CHAINS):
        ids, fin, g = accept_sampled(logits[c * (k + 1):(c + 1) * (k + 1)], drafts[c], seen_after[c], t, pen, seed[c], stream[c], index0[c], eos,
                                     room[c], False, tk, tp, mp, near)
        want.append(ids)
        fins.append(fin)
        gaps += g
    return dict(logits=logits, drafts=drafts, temperature=temperature, penalty=penalty, seed=seed, stream=stream, index0=index0, filt=filt,
                room=room, seen0=seen0, want=want, fins=fins, seen_after=seen_after, gaps=gaps, near=near, eos=eos)

"""numpy restatement of k_score_detail (zoomearth_amd/csrc/ze_score_detail.hip) for one row of bf16 logits held as float32.

logprob and entropy repeat the kernel's float32 arithmetic in the kernel's order: thread t of 256 owns the 8-element groups t, t + 256,
... and then the tail elements nv * 8 + t, + 256, ...; it adds its terms in that order; the 64 lanes of a wave are folded by xor
shuffles (32, 16, ... 1), the four waves as (w0 + w1) + (w2 + w3).  Every operation is rounded to float32 on its own.  (numpy's
float32 exp / log are not the device's, so agreement with the kernel is close, not bitwise.)  rank and top-N are exact integer logic
under the total order (value descending, id ascending), float comparison (-0 == +0)."""
import numpy as np

F = np.float32


def to_bf16(x):
    """float32 values rounded to the nearest bfloat16 (ties to even), returned as float32; infinities stay"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def _ownership(vocab):
    """[256, K] element ids in the order thread t visits them, -1 where it has none"""
    nv = vocab // 8
    per = []
    for t in range(256):
        g = np.arange(t, nv, 256)
        ids = (g[:, None] * 8 + np.arange(8)[None, :]).reshape(-1)
        per.append(np.concatenate([ids, np.arange(nv * 8 + t, vocab, 256)]))
    k = max(len(p) for p in per)
    own = np.full((256, max(k, 1)), -1, dtype=np.int64)
    for t, p in enumerate(per):
        own[t, :len(p)] = p
    return own


def _wg_sum(x):
    """the workgroup reduction of 256 per-thread float32 values"""
    x = x.astype(F).reshape(4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = (x + x[:, lane ^ o]).astype(F)
    r = x[:, 0]
    return F(F(r[0] + r[1]) + F(r[2] + r[3]))


def row_sums(l):
    """(m, tot, S) of a row in the kernel's float32 order"""
    l = np.asarray(l, dtype=F)
    own = _ownership(len(l))
    with np.errstate(all="ignore"):
        m = F(np.max(l))
        tot, s = np.zeros(256, F), np.zeros(256, F)
        for k in range(own.shape[1]):
            has = own[:, k] >= 0
            v = l[np.where(has, own[:, k], 0)]
            d = (v - m).astype(F)
            e = np.exp(d).astype(F)
            tot = np.where(has, (tot + e).astype(F), tot)
            term = (e * d).astype(F)
            s = np.where(has & (v > -np.inf), (s + term).astype(F), s)
        return m, _wg_sum(tot), _wg_sum(s)


def order(l):
    """ids of the finite entries in the total order"""
    l = np.asarray(l, dtype=F)
    ids = np.nonzero(np.isfinite(l))[0]
    return ids[np.lexsort((ids, -l[ids].astype(np.float64)))]


def score_detail(l, target, top_n):
    """(logprob, entropy, rank, top_ids [top_n], top_logprobs [top_n]) of one row"""
    l = np.asarray(l, dtype=F)
    vocab = len(l)
    m, tot, s = row_sums(l)
    with np.errstate(all="ignore"):
        lse = F(np.log(tot))
        ok = 0 <= target < vocab
        lp = F(F(l[target] - m) - lse) if ok else F(0)
        ids = np.full(top_n, -1, dtype=np.int32)
        tlp = np.full(top_n, -np.inf, dtype=F)
        if not np.isfinite(m):
            return lp, F(np.nan), -1, ids, tlp
        ent = F(lse - F(s / tot))
        rank = int((l > l[target]).sum() + (l[:target] == l[target]).sum()) if ok else -1
        first = order(l)[:top_n]
        ids[:len(first)] = first
        tlp[:len(first)] = ((l[first] - m).astype(F) - lse).astype(F)
        return lp, ent, rank, ids, tlp


def score_detail_f64(l, target):
    """(logprob, entropy) of the row in float64"""
    l = np.asarray(l, dtype=np.float64)
    with np.errstate(all="ignore"):
        m = l.max()
        if not np.isfinite(m):
            return np.nan, np.nan
        z = l - m
        lse = np.log(np.exp(z).sum())
        logp = z - lse
        p = np.exp(logp)
        ent = -np.sum(np.where(p > 0, p * logp, 0.0))
        return (logp[target] if 0 <= target < len(l) else 0.0), ent

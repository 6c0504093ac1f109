"""numpy restatement of the sampling filters (top-k -> top-p -> min-p after the temperature, HF's order) with the mass
definition of zoomearth_amd/csrc/ze_sample_filter.hip, plus the float64 decision margin of every token.

    z_i = fp32(score_i / T)                 e_i = fp32 exp(z_i - z_max)              w_i = uint64 rint(e_i * 2^40)
    top-k   keep z_i >= k-th largest z (ties at that value all kept; k >= vocab: off)
    top-p   over the survivors: M = sum w, target = ceil(float64(fp32 top_p) * float64(M));
            keep i iff  sum of w_j over z_j > z_i  <  target
    min-p   keep e_i >= fp32 min_p
    cut = smallest kept z, kept = number of kept tokens

The margins say which tokens two correct implementations may disagree on: a token whose float64 top-p decision lies
within 1e-5 of the total mass of the boundary, or whose e lies within 1e-4 (relative) of min_p.
"""
import numpy as np

f32 = np.float32
TOP_P_MARGIN = 1e-5
MIN_P_MARGIN = 1e-4
SETTINGS = [  # (T, top_k, top_p, min_p); 0 / 1.0 / 0.0 = off
    (1.0, 50, 1.0, 0.0), (1.0, 0, 0.9, 0.0), (0.7, 50, 0.95, 0.0), (1.0, 0, 1.0, 0.05), (0.8, 20, 0.9, 0.02),
    (1.0, 0, 0.5, 0.0), (1.3, 1000, 0.99, 0.0),
]


def cap_for(vocab):
    """Most tokens of one row that may sit inside the margins (a condition of the check, not a measurement)."""
    return 64 if vocab > 2048 else 4


def rand_logits(seed, vocab, scale):
    return (np.random.default_rng(seed).normal(size=vocab) * scale).astype(f32)


def _above(z, w):
    """Per token: the sum of w over the tokens with a strictly larger z (exact integer / float64 sums)."""
    order = np.argsort(-z, kind="stable")
    zs = z[order]
    cum = np.cumsum(w[order])
    first = np.searchsorted(-zs, -zs, side="left")  # start of each run of equal scores
    ab = np.where(first > 0, cum[np.maximum(first - 1, 0)], cum.dtype.type(0))
    out = np.empty_like(ab)
    out[order] = ab
    return out


def scaled(scores, temperature):
    return (np.asarray(scores, dtype=f32) / f32(temperature)).astype(f32)


def filter_ref(scores, temperature, top_k=0, top_p=1.0, min_p=0.0):
    """(keep mask, cut, kept) of one row of (already penalised) fp32 scores, by the kernel's definition."""
    z = scaled(scores, temperature)
    vocab = z.shape[0]
    zmax = z.max()
    e = np.exp((z - zmax).astype(f32)).astype(f32)
    e[~np.isfinite(e)] = 0
    w = np.rint(e * f32(2.0 ** 40)).astype(np.uint64)
    keep = np.ones(vocab, dtype=bool)
    if 0 < top_k < vocab:
        vk = np.partition(z, vocab - top_k)[vocab - top_k]
        keep &= z >= vk
    if top_p < 1.0:
        ws = np.where(keep, w, np.uint64(0))
        total = int(ws.sum())
        target = int(np.ceil(np.float64(f32(top_p)) * np.float64(total)))
        keep &= _above(z, ws) < np.uint64(target)
    if min_p > 0.0:
        keep &= e >= f32(min_p)
    return keep, (z[keep].min() if keep.any() else f32(-np.inf)), int(keep.sum())


def filter_f64(scores, temperature, top_k=0, top_p=1.0, min_p=0.0):
    """The same rules in float64 with no fixed point: (keep mask, near mask); near = tokens inside a decision margin."""
    z = scaled(scores, temperature).astype(np.float64)
    vocab = z.shape[0]
    e = np.exp(z - z.max())
    keep = np.ones(vocab, dtype=bool)
    near = np.zeros(vocab, dtype=bool)
    if 0 < top_k < vocab:
        vk = np.partition(z, vocab - top_k)[vocab - top_k]
        keep &= z >= vk
    if top_p < 1.0:
        es = np.where(keep, e, 0.0)
        total = es.sum()
        frac = _above(z, es) / total
        near |= keep & (np.abs(frac - float(f32(top_p))) < TOP_P_MARGIN)
        keep &= frac < float(f32(top_p))
    if min_p > 0.0:
        near |= np.abs(e - float(f32(min_p))) < MIN_P_MARGIN * float(f32(min_p))
        keep &= e >= float(f32(min_p))
    return keep, near


def assert_same_keep(got, want, near, vocab, top_k_only=False, what=""):
    """Keep-sets equal outside the margins; the number of tokens inside them is capped."""
    if top_k_only:
        assert np.array_equal(got, want), f"{what}: top-k keep-sets differ on {np.nonzero(got != want)[0][:8]}"
        return 0
    n_near = int(near.sum())
    assert n_near <= cap_for(vocab), f"{what}: {n_near} tokens inside the margins (cap {cap_for(vocab)})"
    bad = np.nonzero((got != want) & ~near)[0]
    assert bad.size == 0, f"{what}: keep-sets differ outside the margins on tokens {bad[:8]}"
    return int(((got != want) & near).sum())


def masked(scores, keep):
    out = np.asarray(scores, dtype=f32).copy()
    out[~keep] = -np.inf
    return out

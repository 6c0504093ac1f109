"""numpy restatement of the entropy filters (typical -> epsilon -> eta behind top-k -> top-p -> min-p, HF's order) with the
integer definitions of zoomearth_amd/csrc/ze_sample_band.hip, plus the float64 decision margin of every token.

    z, e, w as tests/sampling_filters_ref.py;  S = the survivors of the three older filters (z >= their cut)
    u_i = uint64 rint(fp32(fp32(e_i * (z_max - z_i)) * 2^40)), 0 where e_i is 0
    H(S) = log(M * 2^-40) + U / M   float64 from the integers M = sum w, U = sum u over S
    typical   s_i = fp32 |((z_max - z_i) + fp32(log(M * 2^-40))) - fp32(H)|;  target = ceil(float64(fp32 typical_p) * float64(M));
              keep i iff  sum of w_j over s_j < s_i  <  target;  band [lo, hi] = smallest / largest kept z
    epsilon   M2 over the band: keep w_i >= ceil(float64(fp32 eps) * float64(M2)), and the largest kept z
    eta       H3, M3 over what epsilon left: thr = min(eta, sqrt(eta) * exp(-H3)) in float64; keep w_i >= ceil(thr * float64(M3)),
              and the largest kept z
    cut = smallest kept z, ceil = hi when typical ran (+inf otherwise), kept = number of kept tokens

The margins say which tokens two correct implementations may disagree on: a token whose float64 mass fraction lies within 1e-5 of
the typical target, whose s lies within 1e-4 (relative) of the typical threshold, or whose probability lies within 1e-4
(relative) of the epsilon / eta threshold -- on top of the margins of the older filters.
"""
import math

import numpy as np

import sampling_filters_ref as R
from sampling_filters_ref import cap_for, f32, masked, rand_logits, scaled  # noqa: F401

MASS_MARGIN = 1e-5
REL_MARGIN = 1e-4
# (T, top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff); 0 / 1.0 / 0.0 / 1.0 / 0.0 / 0.0 = off
SETTINGS = [
    (1.0, 0, 1.0, 0.0, 0.9, 0.0, 0.0),       # each stage alone
    (1.0, 0, 1.0, 0.0, 1.0, 3e-4, 0.0),
    (1.0, 0, 1.0, 0.0, 1.0, 0.0, 2e-3),
    (0.8, 50, 0.95, 0.001, 0.8, 1e-3, 3e-3),  # all three behind top-k / top-p / min-p
    (1.0, 0, 1.0, 0.0, 0.02, 0.0, 0.0),       # typical_p close to 0 and close to 1
    (1.0, 0, 1.0, 0.0, 0.99, 0.0, 0.0),
    (1.3, 0, 0.98, 0.0, 0.5, 0.0, 6e-4),      # a second temperature
    (0.8, 0, 1.0, 0.0, 0.3, 9e-4, 0.0),
]


def row_for(seed, vocab, scale):
    """The rows every test draws its logits from: a normal row, with its arg-max lifted so that some mass is peaked (typical
    sampling has something to drop)."""
    lg = rand_logits(seed, vocab, scale)
    lg[int(lg.argmax())] += f32(2.0)
    return lg


def _quantities(z):
    zmax = z.max()
    with np.errstate(invalid="ignore", over="ignore"):
        d = (zmax - z).astype(f32)
        e = np.exp((z - zmax).astype(f32)).astype(f32)
        e[~((e >= 0) & (e <= 1))] = 0
        ed = (e * d).astype(f32)
    ed[e == 0] = 0
    w = np.rint(e * f32(2.0 ** 40)).astype(np.uint64)
    u = np.rint(ed * f32(2.0 ** 40)).astype(np.uint64)
    return zmax, d, w, u


def _entropy(M, U):
    return math.log(float(M) * 2.0 ** -40) + float(U) / float(M)


def band_ref(scores, temperature, top_k=0, top_p=1.0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
    """(keep mask, cut, ceil, kept) of one row of (already penalised) fp32 scores, by the kernels' definition."""
    keep, cut, kept = R.filter_ref(scores, temperature, top_k, top_p, min_p)
    if not (0 < top_k < len(keep) or top_p < 1.0 or min_p > 0.0):
        cut = f32(-np.inf)   # no filter: no cut
    ceil = f32(np.inf)
    on_t, on_e, on_h = 0.0 < typical_p < 1.0, 0.0 < epsilon_cutoff < 1.0, 0.0 < eta_cutoff < 1.0
    if not (on_t or on_e or on_h):
        return keep, cut, ceil, kept
    z = scaled(scores, temperature)
    keep = keep & ~np.isnan(z)
    zmax, d, w, u = _quantities(z)
    M = int(w[keep].sum(dtype=np.uint64))
    if M == 0:
        return keep, cut, ceil, kept
    if on_t:
        U = int(u[keep].sum(dtype=np.uint64))
        lm, H = f32(math.log(float(M) * 2.0 ** -40)), f32(_entropy(M, U))
        with np.errstate(invalid="ignore"):
            s = np.abs(((d + lm).astype(f32) - H).astype(f32))
        target = int(np.ceil(np.float64(f32(typical_p)) * np.float64(M)))
        ws = np.where(keep, w, np.uint64(0))
        before = R._above(-np.where(keep, s, f32(np.inf)), ws)   # the mass of the survivors with a strictly smaller s
        keep = keep & (before < np.uint64(target))
        ceil = z[keep].max()
    top = z == z[keep].max()
    if on_e:
        M2 = int(w[keep].sum(dtype=np.uint64))
        thr = int(np.ceil(np.float64(f32(epsilon_cutoff)) * np.float64(M2)))
        keep = keep & ((w >= np.uint64(thr)) | top)
    if on_h:
        M3, U3 = int(w[keep].sum(dtype=np.uint64)), int(u[keep].sum(dtype=np.uint64))
        eta = float(f32(eta_cutoff))
        thr = int(np.ceil(min(eta, math.sqrt(eta) * math.exp(-_entropy(M3, U3))) * np.float64(M3)))
        keep = keep & ((w >= np.uint64(thr)) | top)
    return keep, z[keep].min(), ceil, int(keep.sum())


def band_f64(scores, temperature, top_k=0, top_p=1.0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
    """HF's rules in float64 with no fixed point: (keep mask, near mask); near = tokens inside a decision margin."""
    keep, near = R.filter_f64(scores, temperature, top_k, top_p, min_p)
    z = scaled(scores, temperature).astype(np.float64)
    keep = keep & ~np.isnan(z)

    def probs(k):
        with np.errstate(invalid="ignore"):
            e = np.where(k, np.exp(z - z.max()), 0.0)
        e[np.isnan(e)] = 0.0
        return e / e.sum()

    def entropy(p):
        nz = p > 0
        return float(-(p[nz] * np.log(p[nz])).sum())

    if 0.0 < typical_p < 1.0:
        p = probs(keep)
        with np.errstate(divide="ignore"):
            s = np.where(keep, np.abs(-np.log(p) - entropy(p)), np.inf)
        frac = R._above(-s, p)
        t = float(f32(typical_p))
        near |= keep & (np.abs(frac - t) < MASS_MARGIN)
        new = keep & (frac < t)
        s_thr = s[new].max()
        near |= keep & (np.abs(s - s_thr) < REL_MARGIN * s_thr)
        keep = new
    top = z == z[keep].max()
    if 0.0 < epsilon_cutoff < 1.0:
        p, thr = probs(keep), float(f32(epsilon_cutoff))
        near |= keep & (np.abs(p - thr) < REL_MARGIN * thr)
        keep = keep & ((p >= thr) | top)
    if 0.0 < eta_cutoff < 1.0:
        p, eta = probs(keep), float(f32(eta_cutoff))
        thr = min(eta, math.sqrt(eta) * math.exp(-entropy(p)))
        near |= keep & (np.abs(p - thr) < REL_MARGIN * thr)
        keep = keep & ((p >= thr) | top)
    return keep, near


def in_band(scores, temperature, cut, ceil):
    z = scaled(scores, temperature)
    return (z >= cut) & (z <= ceil)


def assert_same_keep(got, want, near, vocab, what=""):
    """Keep-sets equal outside the margins; the number of tokens inside them is capped."""
    return R.assert_same_keep(got, want, near, vocab, False, what)


def draw_ref(scores, keep, temperature, seed, stream, index):
    """(token, gap) of the draw of ze_sample.hip under a band: oracle.qwen25vl.sample_temperature restated over the masked row --
    e_i = 0 outside `keep`, z_max still the maximum of the WHOLE row (the arg-max may lie outside the band), the same fp32
    summation order, inverse-CDF rule and counter-based uniform.  gap: distance of the target to the nearest boundary of the
    token's CDF interval, relative to the total mass (float64)."""
    from oracle import qwen25vl as Q
    sc = np.asarray(scores, dtype=f32)
    vocab = sc.shape[0]
    t = f32(temperature)
    zmax = f32(sc.max()) / t
    with np.errstate(invalid="ignore"):
        e = np.exp((sc / t - zmax).astype(f32)).astype(f32)
    e[~np.asarray(keep, dtype=bool)] = 0
    B = Q.SAMPLE_BLOCKS
    chunk = -(-vocab // B)
    run = -(-chunk // 256)
    pad = np.zeros(B * 256 * run, dtype=f32)
    idx = np.arange(vocab)
    pad[(idx // chunk) * (256 * run) + (idx % chunk)] = e
    grid = pad.reshape(B, 256, run)
    run_sum = np.cumsum(grid, axis=2, dtype=f32)[:, :, -1]
    chunk_sum = np.cumsum(run_sum, axis=1, dtype=f32)[:, -1]
    blk_cum = np.cumsum(chunk_sum, dtype=f32)
    u = Q.sample_uniform(seed, stream, index)
    target = f32(u * blk_cum[-1])
    hit = np.nonzero(blk_cum > target)[0]
    if hit.size == 0:
        blk, tgt_in = int(np.nonzero(chunk_sum > 0)[0][-1]), f32(-np.inf)
    else:
        blk = int(hit[0])
        tgt_in = f32(target - (blk_cum[blk - 1] if blk else f32(0)))
    end = min(vocab, (blk + 1) * chunk)
    token, cum = -1, f32(0)
    for th in range(256):
        if f32(cum + run_sum[blk, th]) > tgt_in:
            for j in range(run):
                i = blk * chunk + th * run + j
                if i >= end:
                    break
                cum = f32(cum + grid[blk, th, j])
                if cum > tgt_in:
                    token = i
                    break
            if token >= 0:
                break
        else:
            cum = f32(cum + run_sum[blk, th])
    if token < 0:
        token = blk * chunk + int(np.nonzero(e[blk * chunk:end] > 0)[0][-1])
    cdf = np.cumsum(e.astype(np.float64))
    x = float(u) * cdf[-1]
    lo = cdf[token - 1] if token else 0.0
    return int(token), float(min(abs(x - lo), abs(cdf[token] - x)) / cdf[-1])


# ---- the rows of the selection tests (tests/test_gpu_entropy_filters.py), shared with the CPU check of their margins
VOCABS = (1000, 2048, 151936)


def case_rows(vocab):
    """[(name, scores)]: three scales, a row with -inf entries, a row whose top token a repetition penalty has pushed down"""
    rows = [(f"scale {sc}", row_for(9100 + 10 * i + vocab % 7, vocab, sc)) for i, sc in enumerate((3.0, 1.0, 0.3))]
    holes = row_for(9200 + vocab % 7, vocab, 2.0)
    holes[vocab // 8: vocab // 2] = -np.inf
    rows.append(("with -inf", holes))
    pen = row_for(9300 + vocab % 7, vocab, 2.0)
    top = int(pen.argmax())
    pen[top] = pen[top] / f32(1.3) if pen[top] > 0 else pen[top] * f32(1.3)   # HF's repetition penalty on the arg-max
    rows.append(("penalised top", pen))
    return rows

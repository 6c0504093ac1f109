"""GPU: the single-chain decode GEMV family alone -- k_gemv (ze_gemv_kernel.h: bf16 stream ze_gemv.hip, FP8 stream ze_gemv8.hip) through
`ze_op_gemv` and k_logits_multi (ze_gemv_logits.hip) through `ze_op_logits_rows` -- against float64 numpy on the same bf16 values, at
the shapes where the kernels change path: partial last chunk, first trip past the last chunk, the K-split long-K form and its staging
loop, row tails, capped grids (grid-stride pair sets), the folded arg-max, every NX instantiation of the multi-row lm_head.

Inputs (oracle.prng, exact bf16 values, as test_gpu_ops.rnd): activations std 1, weights std 0.05, bias std 0.5.

Bounds.  "ulp" is the project's 2^-8 (the largest relative half-spacing of bf16); sc = 0.05 sqrt(K) 0.05 is the floor of a row's scale.
  * PLAIN / LOGITS (one rounding): test_gpu_ops.close_bf16 -- 1.5 ulps of max(|want|, sc).  LOGITS additionally equals bf16_round of
    itself bit for bit (the fp32 copy of a bf16 value).
  * RESIDUAL, bf16(h + bf16(dot + b)) (two roundings): the one-rounding bound of v = dot + b, plus 1.01 ulps of |h + v| for the
    second rounding (taken of a sum that already carries the first error: the 0.01).
  * SWIGLU, bf16(bf16(silu(bf16(g))) * bf16(u)) on rows interleaved [gate 0..15 | up 0..15 | ...]: the formula of
    test_gpu_ops.test_linear_3b_shapes -- 2^-8 (3 |want| + 1.2 max(|g|, sc) |u| + sc^2): four roundings, |silu'| <= 1.1.
  * QKV_ROPE, the embedding prologue, capped grids, a row of ze_op_logits_rows at another batch size: BITS (see the tests).

RMSNorm prologue.  Reference = HF's cast points in float64: xn = bf16(x inv), inv = 1 / sqrt(mean(x^2) + eps), y = bf16(xn g), then the
dot product.  The kernels' inv is fp32, so an element whose x inv lies next to a bf16 rounding boundary may land one ulp away.  How
near: the sum of squares is a sum of positive terms, each square exact in fp32 (8 x 8 significant bits), so its relative error is at
most u = 2^-24 per rounding on the longest path: a thread adds nv = ceil(K / 2048) vectors of 8 elements with at most 8 roundings each
(a pair a^2 + b^2, then the add into the sum; k_logits_multi: 8 fmas), the wave tree adds 6, the four waves 3, the division by K and the
+ eps one each: (8 nv + 11) u on the argument of the rsqrt, half of that behind it, plus 2 u for v_rsq_f32 (1 ulp) and u for the product
x inv: delta = (4 nv + 8.5) u relative.  The zone A of a row is the set of elements whose float64 x inv rounds differently at
(1 - delta) and (1 + delta); a row's tolerance grows by sum_{j in A} |W[r, j]| |g_j| ulp_bf16(xn_j) (act8: the E4M3 spacing at
xn_j / scale, times the scale), pushed through the epilogue's derivative where there is one.  Expected size of A: 2 delta over the mean
relative spacing 2^-7.5, i.e. about K 2^-12 at nv = 1 and 8 at K = 11008 ON AVERAGE -- the inputs are bf16 values, so a row has only 128
distinct mantissas times one inv: usually none of them lands in the zone, and when one does, every element that carries it does (32 of
2056 at one seed).  The tests assert len(A) <= 16 on the reference side, which keeps the term far below one dropped element (~ 0.05
against a bound of ~ 4e-4); the seeds below satisfy it (NORM_SEED, ROWS_SEED: the first of a decade scan that does, checked on the CPU).

Every output buffer is padded with sentinel values that must survive the launch (a store past the end shows there, not as a fault).
"""
import numpy as np
import pytest
import torch

import parity_ledger
from gpu_util import CHAIN_W, tiny_engine, to_dev_bf16  # noqa: F401
from oracle import fp8, prng
from oracle import qwen25vl as Q
from oracle.qwen25vl import bf16_round
from test_gpu_ops import close_bf16, rnd
from test_gpu_ops_kernels import _text_rope_ref

pytestmark = pytest.mark.gpu

QKV_ROPE, RESIDUAL, SWIGLU, LOGITS, PLAIN = 0, 1, 2, 3, 4
EPS = 1e-6
ULP = 2.0 ** -8
PAD = 64
ERR_INVALID, ERR_NOMEM = -1, -3


# ------------------------------------------------------------------ float64 side
def floor_scale(k):
    return 0.05 * np.sqrt(k) * 0.05


def bf16_round64(t):
    """float64 -> nearest-even bf16 (8 significant bits), as float64; no double rounding through fp32."""
    m, e = np.frexp(np.asarray(t, dtype=np.float64))
    return np.ldexp(np.rint(m * 256.0) / 256.0, e)


def ulp_bf16(v):
    """spacing of bf16 at v (0 at 0)"""
    _, e = np.frexp(np.abs(np.asarray(v, dtype=np.float64)))
    return np.where(v == 0, 0.0, np.ldexp(1.0, e - 8))


def zone_delta(k):
    return (4 * ((k + 2047) // 2048) + 8.5) * 2.0 ** -24


def norm_ref(x, g, act8=False):
    """-> (y float64 [K]: the normalised row the dot products read, step float64 [K]: what a one-ulp move of xn_j moves y_j by, on the
    zone A only (0 elsewhere)).  x, g: bf16 values."""
    xf, gf = x.astype(np.float64), g.astype(np.float64)
    t = xf / np.sqrt((xf * xf).mean() + EPS)
    d = zone_delta(len(x))
    xn = bf16_round64(t)
    zone = bf16_round64(t * (1.0 - d)) != bf16_round64(t * (1.0 + d))
    assert zone.sum() <= 16, int(zone.sum())
    y = bf16_round64(xn * gf)
    step = np.abs(gf) * ulp_bf16(xn)
    if act8:
        k = fp8.row_scale_exponent(y[None, :].astype(np.float32))[0]
        s = 2.0 ** float(k)
        assert not zone[np.abs(y).argmax()]   # (the element that sets the row's scale is not a doubtful one)
        y = fp8.e4m3_round((y / s).astype(np.float32)).astype(np.float64) * s
        e = np.maximum(np.floor(np.log2(np.maximum(np.abs(xn) / s, 2.0 ** -30))), -6.0)
        step = np.abs(gf) * np.exp2(e - 3.0) * s
    return y, np.where(zone, step, 0.0)


def expect(epi, full, k, extra=None, h=None):
    """(want, tol) of an epilogue from the float64 rows `full` = W y + b; extra: the rows' zone terms (norm prologue)."""
    sc = floor_scale(k)
    extra = np.zeros_like(full) if extra is None else extra
    one = np.maximum(np.abs(full), sc) * (1.5 * ULP + 1e-6) + extra
    if epi in (PLAIN, LOGITS):
        return full, one
    if epi == RESIDUAL:
        want = h.astype(np.float64) + full
        return want, one + 1.01 * ULP * np.abs(want)
    assert epi == SWIGLU
    blk, eb = full.reshape(-1, 2, 16), extra.reshape(-1, 2, 16)
    g, u, eg, eu = blk[:, 0].reshape(-1), blk[:, 1].reshape(-1), eb[:, 0].reshape(-1), eb[:, 1].reshape(-1)
    silu = g / (1.0 + np.exp(-g))
    want = silu * u
    tol = ULP * (3.0 * np.abs(want) + 1.2 * np.maximum(np.abs(g), sc) * np.abs(u) + sc * sc)
    return want, tol + 1.1 * eg * (np.abs(u) + eu) + np.abs(silu) * eu


class Worst:
    """worst error / tolerance of a family, for the parity ledger"""
    def __init__(self):
        self.ratio = 0.0

    def check(self, got, want, tol, what):
        r = np.abs(got.astype(np.float64) - want) / tol
        self.ratio = max(self.ratio, float(r.max()))
        print(f"{what}: worst error / tolerance {r.max():.3f} at {int(r.argmax())}")
        assert r.max() <= 1.0, (what, float(r.max()), int(r.argmax()))


# ------------------------------------------------------------------ device side
def padded(n, dtype, init=None):
    """an output buffer of n elements followed by PAD sentinel elements"""
    buf = torch.full((n + PAD,), -777.0, dtype=dtype, device="cuda")
    if init is not None:
        buf[:n] = init
    return buf


def pad_intact(buf, n=0):
    """the elements from n on still hold the sentinel"""
    return bool((buf[n:] == torch.full_like(buf[n:], -777.0)).all())


def launch(e, epi, dx, dw, db=None, h=None, w8=None, **kw):
    """one ze_op_gemv launch into a sentinel-padded buffer; returns the output tensor (RESIDUAL: the updated copy of h), or (out, token)"""
    n = (w8[0] if w8 is not None else dw).shape[0]
    n_out = {SWIGLU: n // 2, QKV_ROPE: e.config.text.hidden_size}.get(epi, n)
    buf = padded(n_out, torch.float32 if epi == LOGITS else torch.bfloat16, h)
    if w8 is not None:
        res = e.op_gemv(epi, dx, w8=w8[0], scale8=w8[1], bias=db, out=buf[:n_out], **kw)
    else:
        res = e.op_gemv(epi, dx, w=dw, bias=db, out=buf[:n_out], **kw)
    assert pad_intact(buf, n_out), "a store past the end of the output"
    return (buf[:n_out], res[1]) if isinstance(res, tuple) else buf[:n_out]


def quantised(e, w):
    """(dequantised values fp32 [N, K], (bytes, scales)) of ze_op_quantize_fp8 -- the kernel test_gpu_fp8 holds to oracle/fp8.py"""
    dw = to_dev_bf16(w)
    q, sc = e.op_quantize_fp8(dw)
    return dw.float().cpu().numpy(), (q, sc)


def epilogues_at(e, worst, k, ns, swiglu_ns, fp8_stream=False, seed=100):
    """PLAIN, RESIDUAL, LOGITS at every N of `ns` and SWIGLU at every N of `swiglu_ns`, one weight pool per K, against float64"""
    nmax = max(list(ns) + list(swiglu_ns))
    w, x, b, h = rnd(seed + 1, (nmax, k), 0.05), rnd(seed + 2, (k,)), rnd(seed + 3, (nmax,), 0.5), rnd(seed + 4, (nmax,))
    w8 = None
    if fp8_stream:
        w, w8 = quantised(e, w)
    dw, dx, db, dh = to_dev_bf16(w), to_dev_bf16(x), to_dev_bf16(b), to_dev_bf16(h)
    full = w.astype(np.float64) @ x.astype(np.float64) + b.astype(np.float64)
    for n, epis in [(n, (PLAIN, RESIDUAL, LOGITS)) for n in ns] + [(n, (SWIGLU,)) for n in swiglu_ns]:
        w8n = (w8[0][:n], w8[1][:n]) if w8 else None
        for epi in epis:
            got = launch(e, epi, dx, dw[:n], db[:n], h=dh[:n] if epi == RESIDUAL else None, w8=w8n).float().cpu().numpy()
            want, tol = expect(epi, full[:n], k, h=h[:n])
            worst.check(got, want, tol, f"epi {epi} N {n} K {k}{' fp8' if fp8_stream else ''}")
            if epi == LOGITS:
                assert np.array_equal(got, bf16_round(got)), "logits are the fp32 copy of bf16 values"
            if epi == PLAIN and w8 is None:
                close_bf16(got, want, scale=floor_scale(k))   # (the contract in its own words)


BF16_WORST, NORM_WORST, FP8_WORST, ACT8_WORST, ROWS_WORST = Worst(), Worst(), Worst(), Worst(), Worst()


def test_zone_arithmetic_of_the_reference():
    """the float64 helpers on their own: rounding to 8 significant bits (ties to even), spacing, and a zone that contains exactly the
    elements next to a rounding boundary"""
    v = np.array([1.0, 1.00390625, 1.01171875, 0.1, -3.3, 300.7])
    assert np.array_equal(bf16_round64(v), bf16_round(v.astype(np.float32)).astype(np.float64))
    assert bf16_round64(1.00390625) == 1.0 and bf16_round64(1.01171875) == 1.015625   # ties to even, both ways
    assert ulp_bf16(np.array([1.0, 1.5, 0.75, 0.0, -2.0])).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -8, 0.0, 2.0 ** -6]
    assert zone_delta(2048) == 12.5 * 2.0 ** -24 and zone_delta(11008) == 32.5 * 2.0 ** -24


# ------------------------------------------------------------------ bf16 stream, no prologue
@pytest.mark.parametrize("k", [8, 40, 504])
def test_single_partial_chunk(tiny_engine, k):
    """nch = 1 and the chunk is partial: every lane past K re-reads the row's last 16 B (last_off) against the zero chunk; the first
    trip of four chunks runs three chunks past the end.  P = 1, 3, 17: waves and workgroups without a pair set."""
    epilogues_at(tiny_engine, BF16_WORST, k, (2, 6, 34), (32,))


@pytest.mark.parametrize("k", [512, 520, 1024, 1376, 2048, 2056, 3584])
def test_chunk_boundaries(tiny_engine, k):
    """whole chunks, one element group past a boundary, first trip exactly full (2048) and one chunk into the tail (2056), full trip +
    tail (3584: 7 chunks)"""
    epilogues_at(tiny_engine, BF16_WORST, k, (34, 200), (32, 64, 224))


@pytest.mark.parametrize("k", [4104, 5632, 11008, 12288, 12296, 18944, 25088])
def test_long_k(tiny_engine, k):
    """K > 4096: PLAIN and RESIDUAL split K over the four waves (six clamped x vectors per thread up front; the staging loop beyond
    12288; a wave's six-chunk trip ends inside the first trip up to 12288, then tail, then full trip + tail) and reduce across waves;
    LOGITS and SWIGLU keep one wave per pair set and stage x in the loop"""
    epilogues_at(tiny_engine, BF16_WORST, k, (6, 96), (96,))


def test_refusals_leave_the_output_alone(tiny_engine):
    """x [29184] does not fit the LDS stage: ZE_ERR_NOMEM and an untouched output, for every epilogue -- not another kernel.  The FP8
    stream at K % 16 != 0: ZE_ERR_INVALID.  Eight staged rows of K = 3080 in ze_op_logits_rows: ZE_ERR_NOMEM."""
    from zoomearth_amd._lib import ZoomEarthError
    e = tiny_engine
    for k, fp8_stream, code in ((29184, False, ERR_NOMEM), (520, True, ERR_INVALID)):
        w, dx = torch.zeros((32, k), dtype=torch.bfloat16, device="cuda"), torch.ones(k, dtype=torch.bfloat16, device="cuda")
        w8 = (torch.zeros((32, k), dtype=torch.uint8, device="cuda"), torch.ones(32, dtype=torch.float32, device="cuda")) if fp8_stream else None
        for epi in (PLAIN, RESIDUAL, SWIGLU, LOGITS):
            buf = padded(32, torch.float32 if epi == LOGITS else torch.bfloat16)
            with pytest.raises(ZoomEarthError) as err:
                e.op_gemv(epi, dx, w=None if w8 else w, w8=w8[0] if w8 else None, scale8=w8[1] if w8 else None, out=buf[:32])
            assert err.value.code == code, (k, epi, err.value.code)
            assert pad_intact(buf), (k, epi)
    x, g = torch.ones((2, 3080), dtype=torch.bfloat16, device="cuda"), torch.ones(3080, dtype=torch.bfloat16, device="cuda")
    buf = padded(2 * 6, torch.float32)
    with pytest.raises(ZoomEarthError) as err:
        e.op_logits_rows(x, torch.zeros((6, 3080), dtype=torch.bfloat16, device="cuda"), g, EPS, out=buf[:12].view(2, 6))
    assert err.value.code == ERR_NOMEM and pad_intact(buf)


def block_weight(seed, n, k, blk=4096):
    """[n, k] on the device as test_lm_head_of_the_row_streaming_regime_at_full_vocabulary builds it: a blk-row random block repeated,
    each copy rolled by 17 rows and scaled by its own signed power of two; rows_of(v) expands a per-block-row vector to the n rows"""
    base = rnd(seed, (blk, k), 0.05)
    copies = (n + blk - 1) // blk
    scale = [(-1.0) ** c * 2.0 ** ((c % 5) - 2) for c in range(copies)]
    db = to_dev_bf16(base)
    dw = torch.cat([torch.roll(db, shifts=-17 * c, dims=0) * scale[c] for c in range(copies)])[:n].contiguous()
    assert dw.dtype == torch.bfloat16 and dw.shape == (n, k)

    def rows_of(v):
        return np.concatenate([np.roll(v, -17 * c) * scale[c] for c in range(copies)])[:n]
    return dw, base, rows_of


@pytest.mark.parametrize("k", [512, 520])
def test_two_pairs_per_wave_with_an_odd_pair_count(tiny_engine, k):
    """N >= 8192 gives a wave two row pairs (PAIRS = 2).  LOGITS at N = 8194: P = 4097 is odd -- the last wave's second pair is
    clamped on the load (min(p0 + i, P - 1)) and skipped on the store.  SWIGLU at N = 8224 behind variant knob 1 = 1."""
    e = tiny_engine
    x = rnd(131, (k,))
    dx = to_dev_bf16(x)
    for epi, n in ((LOGITS, 8194), (SWIGLU, 8224)):
        dw, base, rows_of = block_weight(130, n, k)
        full = rows_of(base.astype(np.float64) @ x.astype(np.float64))
        try:
            e.lib.ze_tune(1, 1)
            got = launch(e, epi, dx, dw).float().cpu().numpy()
        finally:
            e.lib.ze_tune(1, 0)
        want, tol = expect(epi, full, k)
        BF16_WORST.check(got, want, tol, f"epi {epi} N {n} K {k} two pairs")


# ------------------------------------------------------------------ capped grids
@pytest.mark.parametrize("k,ns,sw", [(512, (34, 200), 224), (520, (34, 200), 224), (3584, (34, 200), 224), (11008, (6, 96), 96),
                                     (18944, (6, 96), 96)])
def test_capped_grid_gives_the_same_bits(tiny_engine, k, ns, sw):
    """ze_tune knob 2 caps the grid at 1 and 3 workgroups: every wave then takes its second and later pair sets on the grid-stride path
    (no pre-issued first trip, epilogue operands loaded inside) -- the path the real lm_head runs at 2048 of 9496 workgroups.  A row's
    sum order does not depend on the grid: bits equal to the uncapped launch, which is itself held to float64 here."""
    e = tiny_engine
    nmax = max(ns + (sw,))
    w, x, b, h = rnd(141, (nmax, k), 0.05), rnd(142, (k,)), rnd(143, (nmax,), 0.5), rnd(144, (nmax,))
    dw, dx, db, dh = to_dev_bf16(w), to_dev_bf16(x), to_dev_bf16(b), to_dev_bf16(h)
    full = w.astype(np.float64) @ x.astype(np.float64) + b.astype(np.float64)
    cases = [(epi, n) for n in ns for epi in (PLAIN, RESIDUAL, LOGITS)] + [(SWIGLU, sw)]
    ref = {}
    try:
        for cap in (0, 1, 3):
            e.lib.ze_tune(2, cap)
            for epi, n in cases:
                got = launch(e, epi, dx, dw[:n], db[:n], h=dh[:n] if epi == RESIDUAL else None)
                if cap == 0:
                    ref[epi, n] = got.clone()
                    want, tol = expect(epi, full[:n], k, h=h[:n])
                    BF16_WORST.check(got.float().cpu().numpy(), want, tol, f"epi {epi} N {n} K {k}")
                else:
                    assert torch.equal(got, ref[epi, n]), (cap, epi, n)
    finally:
        e.lib.ze_tune(2, 0)


def test_lm_head_at_full_vocabulary_on_the_capped_grid(tiny_engine):
    """The real lm_head, N = 151,936 at K = 2048: 9496 natural workgroups of two pairs per wave on a grid of 2048 -- every wave runs
    one pre-issued and three or four grid-stride pair sets.  Every row against float64 (block-built weight: one [4096] product), and
    the folded arg-max of the launch = the lowest index of the maximum of its own logits."""
    e = tiny_engine
    n, k = 151936, 2048
    x = rnd(152, (k,))
    dw, base, rows_of = block_weight(151, n, k)
    got_t, tok = launch(e, LOGITS, to_dev_bf16(x), dw, argmax=True)
    got = got_t.cpu().numpy()
    want, tol = expect(LOGITS, rows_of(base.astype(np.float64) @ x.astype(np.float64)), k)
    BF16_WORST.check(got, want, tol, "lm_head 151936 x 2048")
    assert np.array_equal(got, bf16_round(got))
    assert tok == int(np.argmax(got)) and (got == got.max()).sum() >= 1
    del dw, got_t
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ folded arg-max
def penalised_argmax(logits, seen, pen):
    """k_argmax_partial's arithmetic in fp32: penalty on seen ids, the larger value, then the lower index"""
    p = logits.astype(np.float32).copy()
    if seen is not None:
        s = seen.astype(bool)
        pf = np.float32(pen)
        p[s] = np.where(p[s] < 0, p[s] * pf, p[s] / pf).astype(np.float32)
    return int(np.flatnonzero(p == p.max())[0]), p


@pytest.mark.parametrize("cap,rows", [(0, (10, 11)), (0, (17, 21)), (0, (21, 17)), (0, (50, 150)), (0, (150, 50)), (1, (3, 11)), (1, (9, 6)),
                                      (3, (2, 27)), (0, (0, 199))])
def test_folded_argmax_breaks_ties_towards_the_lower_index(tiny_engine, cap, rows):
    """Two identical rows carry the maximum (same bits): in one pair (10, 11); in two waves of one workgroup (17 and 21: pairs 8 and 10
    of workgroup 2); in two workgroups (50, 150); under a grid of one workgroup a pre-issued and a grid-stride pair set of one wave
    (3 and 11: pairs 1 and 5 of wave 1) and of two waves (9, 6); under three workgroups (2, 27).  The token is the lower index,
    whichever of the two the hardware finishes first."""
    e = tiny_engine
    n, k = 200, 512
    w, x, b = rnd(161, (n, k), 0.05), rnd(162, (k,)), rnd(163, (n,), 0.5)
    top = bf16_round(0.1 * np.sign(x)).astype(np.float32)     # a row whose logit (~ 40) beats every random one (|.| < 6)
    for r in rows:
        w[r], b[r] = top, b[rows[0]]
    try:
        e.lib.ze_tune(2, cap)
        got_t, tok = launch(e, LOGITS, to_dev_bf16(x), to_dev_bf16(w), to_dev_bf16(b), argmax=True)
    finally:
        e.lib.ze_tune(2, 0)
    got = got_t.cpu().numpy()
    assert got[rows[0]] == got[rows[1]] == got.max() and (got == got.max()).sum() == 2
    assert tok == min(rows) == penalised_argmax(got, None, 1.0)[0]
    want, tol = expect(LOGITS, w.astype(np.float64) @ x.astype(np.float64) + b.astype(np.float64), k)
    BF16_WORST.check(got, want, tol, f"tie rows {rows}")


@pytest.mark.parametrize("n,k", [(200, 512), (8194, 520)])
@pytest.mark.parametrize("negative", [False, True])
def test_folded_argmax_applies_the_repetition_penalty(tiny_engine, n, k, negative):
    """Penalty 1.0 and 1.3 on seen ids, on the one- and the two-pair kernel: a seen maximum divided by 1.3 falls behind the runner-up
    (0.9 of it); with every logit negative (bias -50: the two rows at about -40 and -41, the rest below -44) the seen maximum is
    MULTIPLIED by the penalty (-52) and falls behind as well -- divided it would stay in front.  The expected token is computed from the
    GPU's own logits in fp32."""
    e = tiny_engine
    w, x = rnd(171, (n, k), 0.05), rnd(172, (k,))
    b = np.full(n, -50.0 if negative else 0.0, np.float32)
    first, second = n - 3, 5
    amp = 0.025 if negative else 0.1
    w[first], w[second] = bf16_round(amp * np.sign(x)), bf16_round(0.9 * amp * np.sign(x))
    seen = np.zeros(n, np.uint8)
    seen[[first, 7, n // 2]] = 1
    dseen = torch.from_numpy(seen).cuda()
    dx, dw, db = to_dev_bf16(x), to_dev_bf16(w), to_dev_bf16(b)
    toks = {}
    for pen in (1.0, 1.3):
        got_t, tok = launch(e, LOGITS, dx, dw, db, argmax=True, seen=dseen, penalty=pen)
        got = got_t.cpu().numpy()
        exp, p = penalised_argmax(got, seen, pen)
        assert tok == exp, (pen, tok, exp)
        assert (p == p.max()).sum() == 1
        toks[pen] = tok
    assert toks[1.0] == first and toks[1.3] == second
    assert bool((dseen.cpu().numpy() == seen).all())     # the caller's flags are read only


def test_folded_argmax_after_a_larger_grid(tiny_engine):
    """The partial slots persist in the engine.  A 151,936-row launch fills all 2048 of them with logits of ~ +-20; the 34-row launch
    after it (5 workgroups) resets the slots beyond its grid, so its token comes from its own rows (maximum ~ 8, at row 20)."""
    e = tiny_engine
    k = 512
    x = rnd(182, (k,))
    dx = to_dev_bf16(x)
    dw, _, _ = block_weight(181, 151936, k)
    big, tok_big = launch(e, LOGITS, dx, dw, argmax=True)
    big_max = float(big.max())
    assert tok_big == int(torch.argmax(big)) and tok_big >= 34
    del dw, big
    w = rnd(183, (34, k), 0.05)
    w[20] = bf16_round(0.02 * np.sign(x))
    got_t, tok = launch(e, LOGITS, dx, to_dev_bf16(w), argmax=True)
    got = got_t.cpu().numpy()
    assert got.max() < big_max, "the stale slots would win"
    assert tok == 20 == int(np.argmax(got))
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ QKV_ROPE and the embedding prologue: bits
def two_chains(e):
    """chain 0: 33 text tokens; chain 2: an image block (rope_delta != 0), as test_rope_and_kv_append_of_a_decode_step"""
    e.fill_synthetic(**CHAIN_W)
    cfg = Q.tiny_config()
    prompts = {0: (prng.uniform_ints(96, 33, 10, 1990).tolist(), []),
               2: ([11, cfg.vision_start_token_id] + [cfg.image_token_id] * 24 + [cfg.vision_end_token_id, 12, 13], [(1, 8, 12)])}
    ctx, delta = {}, {}
    for s, (ids, grids) in prompts.items():
        pos, d = e.rope_index(ids, grids)
        e.seq_reset(s)
        emb = to_dev_bf16(rnd(98, (24, cfg.text.hidden_size))) if grids else None
        e.prefill(s, ids, emb, pos, d, want_logits=False)
        ctx[s], delta[s] = len(ids), d
    assert delta[2] != 0 and delta[0] == 0
    return cfg, ctx, delta


@pytest.mark.parametrize("fp8_stream", [False, True])
def test_qkv_rope_epilogue_is_the_plain_projection_roped(tiny_engine, fp8_stream):
    """QKV_ROPE and PLAIN are one instantiation (<1, 1, 4>) below K = 4096 -- a lane-local fma chain in chunk order, a wave sum, one
    rounding -- so Q and K are _text_rope_ref (HF's cast points) of the PLAIN output of the same W, x and bias, and V is the PLAIN
    output, bit for bit; PLAIN itself is held to float64.  K and V land at row ctx of the layer's cache of the chain: rows ctx - 1 and
    ctx + 1 and the other layers keep their bits, and the chain's length does not change."""
    e = tiny_engine
    cfg, ctx, delta = two_chains(e)
    t = cfg.text
    nq, nkv, hd = t.num_attention_heads, t.num_key_value_heads, cfg.head_dim
    n, layer = (nq + 2 * nkv) * hd, 1
    for k in ((1040, 3584) if fp8_stream else (504, 512, 520, 2048, 3584)):
        w, x, b = rnd(191, (n, k), 0.05), rnd(192 + k, (k,)), rnd(193, (n,), 0.5)
        w8 = None
        if fp8_stream:
            w, w8 = quantised(e, w)
        dw, dx, db = to_dev_bf16(w), to_dev_bf16(x), to_dev_bf16(b)
        plain_t = launch(e, PLAIN, dx, dw, db, w8=w8)
        plain = plain_t.float().cpu().numpy()
        want, tol = expect(PLAIN, w.astype(np.float64) @ x.astype(np.float64) + b.astype(np.float64), k)
        (FP8_WORST if fp8_stream else BF16_WORST).check(plain, want, tol, f"qkv-shaped PLAIN K {k}")
        for s in (0, 2):
            around = [z.clone() for z in e.op_kv_read(s, layer, ctx[s] - 1, 3)]
            others = [[z.clone() for z in e.op_kv_read(s, l, ctx[s], 1)] for l in (0, 2)]
            q = launch(e, QKV_ROPE, dx, dw, db, w8=w8, seq=s, layer=layer).float().cpu().numpy()
            pos3 = np.full((3, 1), ctx[s] + delta[s])
            assert np.array_equal(q.reshape(1, nq, hd), _text_rope_ref(cfg, plain[: nq * hd].reshape(1, nq, hd), pos3)), (k, s)
            kc, vc = e.op_kv_read(s, layer, ctx[s] - 1, 3)
            assert np.array_equal(kc[:, 1].float().cpu().numpy(),
                                  _text_rope_ref(cfg, plain[nq * hd: (nq + nkv) * hd].reshape(1, nkv, hd), pos3)[0]), (k, s)
            assert np.array_equal(vc[:, 1].float().cpu().numpy(), plain[(nq + nkv) * hd:].reshape(nkv, hd)), (k, s)
            for got_c, old_c in ((kc, around[0]), (vc, around[1])):
                assert torch.equal(got_c[:, 0], old_c[:, 0]) and torch.equal(got_c[:, 2], old_c[:, 2]), (k, s)
            for l, old in zip((0, 2), others):
                now = e.op_kv_read(s, l, ctx[s], 1)
                assert torch.equal(now[0], old[0]) and torch.equal(now[1], old[1]), (k, s, l)
            assert e.seq_len(s) == ctx[s]


@pytest.mark.parametrize("k", [504, 2048, 5632])
def test_embedding_prologue_is_the_row_as_x(tiny_engine, k):
    """embed_out = the embedding row of the token, bit for bit, and every output = the same launch given that row as x -- plain, with
    the norm, on the K-split kernel (5632), and as layer 0 runs it: QKV_ROPE with the norm on a chain's own state."""
    e = tiny_engine
    n, vocab, token = 96, 50, 37
    emb, w, g = rnd(201, (vocab, k)), rnd(202, (n, k), 0.05), bf16_round(1.0 + rnd(203, (k,), 0.1))
    demb, dw, dg = to_dev_bf16(emb), to_dev_bf16(w), to_dev_bf16(g)
    for epi, norm in ((PLAIN, None), (PLAIN, dg), (LOGITS, dg), (SWIGLU, dg)):
        eo = padded(k, torch.bfloat16)
        a = launch(e, epi, None, dw, norm_w=norm, eps=EPS, embed=demb, token=token, embed_out=eo[:k])
        assert pad_intact(eo, k) and torch.equal(eo[:k], demb[token]), (epi, k)
        assert torch.equal(a, launch(e, epi, demb[token].contiguous(), dw, norm_w=norm, eps=EPS)), (epi, k)
    if k > 4096:
        return
    cfg, ctx, _ = two_chains(e)
    t = cfg.text
    nqkv = (t.num_attention_heads + 2 * t.num_key_value_heads) * cfg.head_dim
    dwq = to_dev_bf16(rnd(204, (nqkv, k), 0.05))
    eo = padded(k, torch.bfloat16)
    a = launch(e, QKV_ROPE, None, dwq, norm_w=dg, eps=EPS, embed=demb, token=token, embed_out=eo[:k], seq=2, layer=0).clone()
    kv_a = [z.clone() for z in e.op_kv_read(2, 0, ctx[2], 1)]
    assert pad_intact(eo, k) and torch.equal(eo[:k], demb[token])
    b = launch(e, QKV_ROPE, demb[token].contiguous(), dwq, norm_w=dg, eps=EPS, seq=2, layer=0)
    kv_b = e.op_kv_read(2, 0, ctx[2], 1)
    assert torch.equal(a, b) and torch.equal(kv_a[0], kv_b[0]) and torch.equal(kv_a[1], kv_b[1])
    assert float(kv_a[0].float().abs().max()) > 0


# ------------------------------------------------------------------ RMSNorm prologue
NORM_SEED = {2056: 220}   # (seed 210 puts 32 elements of one mantissa into the zone at K = 2056)
ROWS_SEED = {3072: 261}


def norm_inputs(seed, n, k):
    w, x, b = rnd(seed + 1, (n, k), 0.05), rnd(seed + 2, (k,), 2.0), rnd(seed + 3, (n,), 0.5)
    g, h = bf16_round(1.0 + rnd(seed + 4, (k,), 0.1)), rnd(seed + 5, (n,))
    return w, x, b, g, h


@pytest.mark.parametrize("k", [504, 512, 1376, 2048, 2056, 3584, 11008])
def test_norm_prologue(tiny_engine, k):
    """RMSNorm fused in front of every epilogue (x std 2, g = 1 + N(0, 0.1) as test_rmsnorm) against HF's cast points in float64, with
    the zone term of the module docstring; K > 2048 re-reads the norm weight past the pre-issued vector (v != tid)."""
    e = tiny_engine
    n = 96
    w, x, b, g, h = norm_inputs(NORM_SEED.get(k, 210), n, k)
    y, step = norm_ref(x, g)
    aw = np.abs(w.astype(np.float64))
    full, extra = w.astype(np.float64) @ y + b.astype(np.float64), aw @ step
    dw, dx, db, dg, dh = to_dev_bf16(w), to_dev_bf16(x), to_dev_bf16(b), to_dev_bf16(g), to_dev_bf16(h)
    for epi, rows in ((PLAIN, 34), (PLAIN, n), (RESIDUAL, n), (LOGITS, n), (SWIGLU, n)):
        got = launch(e, epi, dx, dw[:rows], db[:rows], h=dh[:rows] if epi == RESIDUAL else None, norm_w=dg, eps=EPS).float().cpu().numpy()
        want, tol = expect(epi, full[:rows], k, extra=extra[:rows], h=h[:rows])
        NORM_WORST.check(got, want, tol, f"norm epi {epi} N {rows} K {k} (zone: {int((step > 0).sum())})")


# ------------------------------------------------------------------ FP8 stream
@pytest.mark.parametrize("k", [16, 1008, 1024, 1040, 3584, 11008, 18944])
def test_fp8_stream(tiny_engine, k):
    """The E4M3 weight stream (1024-element chunks, 16 weights per lane and load, packed FMAs, the row's power-of-two scale applied
    once) against float64 on the dequantised values ze_op_quantize_fp8 leaves behind: one partial chunk (16, 1008), the boundary,
    one group past it, full trip + tail, the K-split form."""
    if k > 4096:
        epilogues_at(tiny_engine, FP8_WORST, k, (6, 96), (96,), fp8_stream=True, seed=220)
    else:
        epilogues_at(tiny_engine, FP8_WORST, k, (2, 6, 34, 200), (32, 224), fp8_stream=True, seed=220)


def test_fp8_stream_two_pairs_per_wave(tiny_engine):
    """the FP8 stream's default for N >= 8192: SWIGLU at N = 8224 and LOGITS at N = 8194 (odd P) on PAIRS = 2, K one group past a chunk"""
    e = tiny_engine
    k = 1040
    x = rnd(232, (k,))
    for epi, n in ((SWIGLU, 8224), (LOGITS, 8194)):
        w, w8 = quantised(e, rnd(231, (n, k), 0.05))
        got = launch(e, epi, to_dev_bf16(x), None, w8=w8).float().cpu().numpy()
        want, tol = expect(epi, w.astype(np.float64) @ x.astype(np.float64), k)
        FP8_WORST.check(got, want, tol, f"fp8 epi {epi} N {n} K {k} two pairs")


@pytest.mark.parametrize("k", [1040, 3584])
def test_fp8_activations_behind_the_norm(tiny_engine, k):
    """act8: the normalised row replaced by its E4M3 quantisation (one power-of-two scale for the row, oracle/fp8.py) before the dot
    products; the zone term uses the E4M3 spacing"""
    e = tiny_engine
    n = 96
    w, x, b, g, h = norm_inputs(240, n, k)
    w, w8 = quantised(e, w)
    dx, db, dg = to_dev_bf16(x), to_dev_bf16(b), to_dev_bf16(g)
    for act8, worst in ((False, FP8_WORST), (True, ACT8_WORST)):
        y, step = norm_ref(x, g, act8=act8)
        full, extra = w.astype(np.float64) @ y + b.astype(np.float64), np.abs(w.astype(np.float64)) @ step
        for epi in (PLAIN, LOGITS, SWIGLU):
            got = launch(e, epi, dx, None, db, w8=w8, norm_w=dg, eps=EPS, act8=act8).float().cpu().numpy()
            want, tol = expect(epi, full, k, extra=extra)
            worst.check(got, want, tol, f"fp8 norm act8={act8} epi {epi} K {k}")


# ------------------------------------------------------------------ k_logits_multi
@pytest.mark.parametrize("n,k", [(2, 8), (5, 8), (2, 504), (5, 512), (2, 520), (5, 2048), (2, 3072), (5, 3072), (2048, 504), (2048, 2048),
                                 (8191, 512), (8191, 3072), (40002, 8), (40002, 520)])
def test_logits_rows(tiny_engine, n, k):
    """ze_op_logits_rows at 1, 2, 3, 4, 5, 8, 9 and 17 rows (NX = 1, 2, 4, 4, 8, 8, 8 + 1, 8 + 8 + 1: spare slots repeat the last
    chain): every row against float64 through the norm bound, and row i the same bits at every batch size and position -- the file's
    stated contract.  N % 4 != 0: the clamped row load and the guarded store (the sentinel pad behind the last row must survive, and
    the first logits of row i + 1 must not carry row i's); N = 40002: the grid-stride loop."""
    e = tiny_engine
    rows = 17
    seed = ROWS_SEED.get(k, 251)
    x, g = rnd(seed, (rows, k), 2.0), bf16_round(1.0 + rnd(seed + 1, (k,), 0.1))
    if n > 4096:
        dw, base, rows_of = block_weight(250, n, k)
    else:
        base = rnd(250, (n, k), 0.05)
        dw, rows_of = to_dev_bf16(base), (lambda v: v)
    dx, dg = to_dev_bf16(x), to_dev_bf16(g)

    def run(lo, hi):
        buf = padded((hi - lo) * n, torch.float32)
        out = e.op_logits_rows(dx[lo:hi].contiguous(), dw, dg, EPS, out=buf[: (hi - lo) * n].view(hi - lo, n))
        assert pad_intact(buf, (hi - lo) * n), "a store past the end of the output"
        return out

    all_t = run(0, rows)
    got = all_t.cpu().numpy()
    assert np.array_equal(got, bf16_round(got))
    b64, ab = base.astype(np.float64), np.abs(base.astype(np.float64))
    for i in range(rows):
        y, step = norm_ref(x[i], g)
        want, tol = expect(LOGITS, rows_of(b64 @ y), k, extra=np.abs(rows_of(ab @ step)))
        ROWS_WORST.check(got[i], want, tol, f"logits_rows row {i} N {n} K {k}")
    for m in (1, 2, 3, 4, 5, 8, 9):
        assert torch.equal(run(0, m), all_t[:m]), m
    assert torch.equal(run(3, 8), all_t[3:8]) and torch.equal(run(16, 17), all_t[16:17])


def test_parity_ledger_of_the_gemv_family():
    """worst error over tolerance of each family of this file (bar 1.0: the tolerances above are the bounds themselves)"""
    for what, w in (("k_gemv bf16", BF16_WORST), ("k_gemv bf16 + norm", NORM_WORST), ("k_gemv fp8", FP8_WORST),
                    ("k_gemv fp8 + act8", ACT8_WORST), ("k_logits_multi", ROWS_WORST)):
        parity_ledger.record(w.ratio, 1.0, what=what, bar=1.0)
        assert w.ratio <= 1.0

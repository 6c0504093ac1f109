"""GPU: the MXFP4 fragment stream of the 2 .. 64-chain decode step (k_gemm_skinny / k_gemm_oneshot W4, k_pack_fragments4).

code * 2^e is exact in bf16, so the W4 kernels feed the MFMAs the operands the dequantised bf16 fragments hold, in the same order: every
check here is BIT equality, none has a tolerance.
  * unit: ze_op_gemm4 (row-major q / scale, packed inside the call) against ze_op_gemm on the dequantised bf16 weights, same launcher
    and epilogue, on operands built to hit the format's corners;
  * engine: bursts of 5 and 64 chains, greedy with a repetition penalty and sampled with per-chain seeds, and a burst with one
    speculating chain, under ze_tune knob 24 = 0 (4-bit fragments) and 1 (dequantised bf16 fragments): ids, logits and K/V rows;
  * ze_fragment_bytes, the life cycle around a weight write, the refusals.
The down projection of the step runs on the split-K ring from the dequantised arena (it has no fragment kernel, so no W4 form):
ze_op_gemm4 refuses its launcher."""
import numpy as np
import pytest
import torch

import gemm4_ref as G
import mxfp4_ref as R
from gpu_util import CHAIN_W, tiny_engine  # noqa: F401
from oracle import prng

pytestmark = pytest.mark.gpu

ERR_INVALID = -1
NONE, RESIDUAL, SWIGLU, F32 = 0, 2, 3, 4     # epilogues of ze_op_gemm
SKINNY, ONESHOT = 5, 6                        # its fragment launchers


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


# ----------------------------------------------------------------------------------------------------------------- unit
def corner_weights(n, k, seed):
    """bf16-representable weights [n, k] whose MXFP4 blocks hit the corners of the format: an all-zero block, blocks at both exponent
    clamps, codes +-6 and +-0.5 side by side, and neighbouring blocks (along K and along N) at opposite ends of the exponent range."""
    rng = np.random.default_rng(seed)
    nb = k // 32
    w = rng.standard_normal((n, k)) * np.exp2(rng.integers(-8, 9, size=(n, nb)).repeat(32, axis=1).astype(np.float64))
    w[0, 0:32] = 0.0                                                       # an all-zero block (scale byte 127)
    pattern = np.array([6.0, -6.0, 0.5, -0.5, 1.5, -3.0, 0.0, 4.0] * 4)   # as codes once the block's amax is 6
    w[1, 0:32] = pattern * 2.0 ** 125                                      # e = 125, the upper clamp: 6 * 2^125 is finite in bf16
    w[2, 0:32] = pattern * 2.0 ** -125                                     # e = -125, the lower clamp: 0.5 * 2^-125 is the least normal
    if nb >= 2:
        w[1, 32:64] = pattern[::-1] * 2.0 ** -125                          # ... next to each other along K
        w[2, 32:64] = pattern[::-1] * 2.0 ** 125
    w[3, k - 32:k] = pattern * 2.0 ** 125                                  # ... and in the LAST block of a row, next to row 2's along N
    w[n - 1, k - 32:k] = pattern * 2.0 ** -125
    return R.bf16_round_trip(w)


def activations(m, k, seed):
    """distinct per row and per k, small enough that 6 * 2^125 times a row stays finite in fp32"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((m, k)) * 0.25 + (np.arange(k)[None, :] % 13 - 6) / 64.0 + (np.arange(m)[:, None] + 1) / 128.0
    return R.bf16_round_trip(x * 2.0 ** -6)


def dev_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().to(torch.bfloat16).contiguous()


def quantised(e, n, k, seed):
    """(dequantised bf16 weights [n, k], q, scale) on the device, the quantiser checked against the restatement on the way"""
    w = corner_weights(n, k, seed)
    dw = dev_bf16(w)
    q, sc = e.op_quantize_mxfp4(dw)
    torch.cuda.synchronize()
    rq, rs, rdq = R.quantize(w)
    assert np.array_equal(sc.cpu().numpy(), rs) and np.array_equal(dw.float().cpu().numpy(), rdq)
    assert {2, 127, 252} <= set(rs.ravel().tolist())            # both clamps and the all-zero block are there
    return dw, q, sc


def both(e, launcher, epi, x, dw, q, sc, bias, m, n, k):
    """the launcher on the dequantised bf16 weights and on the 4-bit stream -> the two outputs' bits"""
    out = []
    for four in (False, True):
        width = n // 2 if epi == SWIGLU else n
        c = dev_bf16(activations(m, width, 99)) if epi == RESIDUAL else torch.full((m, width), -7.0, device="cuda",
                                                                                   dtype=torch.float32 if epi == F32 else torch.bfloat16)
        r = c if epi == RESIDUAL else None                      # residual in place
        if four:
            rc = e.op_gemm4(launcher, epi, x, k, q, sc, bias, r, width if r is not None else 0, c, width, m, n, k)
        else:
            rc = e.op_gemm(launcher, epi, x, k, dw, k, bias, r, width if r is not None else 0, c, width, None, m, n, k)
        torch.cuda.synchronize()
        assert rc == 0, (launcher, epi, m, n, k, four, rc)
        out.append(bits(c))
    return out


_operands = {}


def operands(e, n, k):
    if (n, k) not in _operands:
        _operands[(n, k)] = quantised(e, n, k, 1000 * n + k) + (dev_bf16(R.bf16_round_trip(np.random.default_rng(n).standard_normal(n) * 0.5)),)
    return _operands[(n, k)]


@pytest.mark.parametrize("k", [128, 160, 2048])
@pytest.mark.parametrize("m", [1, 16, 17, 33, 64])
def test_w4_kernels_equal_the_dequantised_bf16_kernels_bit_for_bit(tiny_engine, m, k):
    """every MT (1, 2, 4) with a partial last tile; K = 160 is five slices: unequal shares for the four (sixteen) waves"""
    e = tiny_engine
    x = dev_bf16(activations(m, k, 7 * m + k))
    cases = [(SKINNY, NONE, 48, True), (SKINNY, RESIDUAL, 48, False), (SKINNY, F32, 48, False),     # one block per workgroup
             (SKINNY, SWIGLU, 32, False), (SKINNY, SWIGLU, 96, True),                                # pairs of blocks (gate | up)
             (ONESHOT, NONE, 48, True), (ONESHOT, RESIDUAL, 48, False)]                              # the sixteen-wave kernel (qkv with bias / o)
    if k != 2048:                                                                                    # (wide: kept to the short K)
        cases += [(SKINNY, F32, 4112, False),                                                        # the lm_head form: two blocks per workgroup
                  (SKINNY, SWIGLU, 4160, False),                                                     # above 32 rows: the balanced gate/up, fewer pairs (130) than CUs
                  (SKINNY, SWIGLU, 8224, True)]                                                      # ... and 257 pairs: ranges of one and of two pairs
    for launcher, epi, n, with_bias in cases:
        dw, q, sc, bias = operands(e, n, k)
        ref, got = both(e, launcher, epi, x, dw, q, sc, bias if with_bias else None, m, n, k)
        assert ref.shape == got.shape and np.array_equal(ref, got), (launcher, epi, n, int((ref != got).sum()))
        assert not (ref == bits(torch.full((1,), -7.0, dtype=torch.float32 if epi == F32 else torch.bfloat16))[0]).all()   # something was written


def test_a_wrong_scale_or_nibble_would_show(tiny_engine):
    """The operands can tell: the same call with two scale bytes of neighbouring blocks exchanged, or the two nibbles of one byte
    exchanged, gives other bits."""
    e = tiny_engine
    m, n, k = 17, 48, 160
    x = dev_bf16(activations(m, k, 5))
    dw, q, sc, _ = operands(e, n, k)
    ref, got = both(e, SKINNY, NONE, x, dw, q, sc, None, m, n, k)
    assert np.array_equal(ref, got)
    sc2 = sc.clone()
    sc2[1, 0], sc2[1, 1] = sc[1, 1], sc[1, 0]                    # row 1: e = 125 next to e = -125
    assert not np.array_equal(both(e, SKINNY, NONE, x, dw, q, sc2, None, m, n, k)[1], ref)
    hs, hq = sc.cpu().numpy(), q.cpu().numpy()
    r = next(r for r in range(16, 47) if hs[r, 2] != hs[r + 1, 2])
    sc3 = sc.clone()
    sc3[r, 2], sc3[r + 1, 2] = sc[r + 1, 2], sc[r, 2]            # the same slice of two neighbouring rows
    assert not np.array_equal(both(e, SKINNY, NONE, x, dw, q, sc3, None, m, n, k)[1], ref)
    b = next(b for b in range(32, 80) if (hq[5, b] >> 4) != (hq[5, b] & 15))
    q2 = q.clone()
    q2[5, b] = int((hq[5, b] >> 4) | ((hq[5, b] & 15) << 4))     # the two nibbles of one byte
    assert not np.array_equal(both(e, ONESHOT, NONE, x, dw, q2, sc, None, m, n, k)[1], ref)


def test_refusals(tiny_engine):
    e = tiny_engine
    m, n = 4, 48
    c = torch.zeros((m, n), dtype=torch.bfloat16, device="cuda")
    for launcher, k, epi in ((SKINNY, 48, NONE), (ONESHOT, 48, NONE),            # K % 32
                             (3, 128, RESIDUAL), (0, 128, NONE), (4, 128, NONE),  # the down projection's launcher (split-K ring) and the others: no W4 form
                             (ONESHOT, 128, SWIGLU)):                             # an epilogue the one-shot kernel does not have
        x = dev_bf16(activations(m, k, 1))
        q = torch.zeros((n, max(k // 2, 1)), dtype=torch.uint8, device="cuda")
        sc = torch.full((n, max(k // 32, 1)), 127, dtype=torch.uint8, device="cuda")
        assert e.op_gemm4(launcher, epi, x, k, q, sc, None, c, n, c, n, m, n, k) == ERR_INVALID, (launcher, k, epi)
    torch.cuda.synchronize()
    assert not bits(c).any()


# ----------------------------------------------------------------------------------------------------------------- engine
def text_ids(seed, n):
    return prng.uniform_ints(seed, n, 10, 1990).tolist()


def repeating(n, shift=0):
    return [100 + (i + shift) % 7 for i in range(n)]


@pytest.fixture(scope="module")
def eng64():
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.engine import Engine
    e = Engine(ModelConfig.tiny(), device=0, max_seqs=64, max_ctx=512, max_patches=64, max_tile_side=64)
    e.fill_synthetic(**CHAIN_W)
    assert e.set_decode_regime(0) == 0
    yield e
    e.lib.ze_tune(24, 0)
    e.close()


def prefill_text(e, seq, ids):
    pos, delta = e.rope_index(ids, [])
    e.seq_reset(seq)
    e.prefill(seq, ids, None, pos, delta, want_logits=False)
    e.mark_seen(seq, ids)


def kv_rows(e, seq, n):
    return [tuple(bits(x) for x in e.op_kv_read(seq, li, 0, n)) for li in range(e.config.text.num_hidden_layers)]


def expected_fragment_bytes(e, four):
    t = e.config.text
    h, hd = t.hidden_size, t.hidden_size // t.num_attention_heads
    nq, nqkv, ip = t.num_attention_heads * hd, (t.num_attention_heads + 2 * t.num_key_value_heads) * hd, (t.intermediate_size + 63) // 64 * 64
    tensors = [(nqkv, h), (h, nq), (2 * ip, h)] * t.num_hidden_layers
    assert t.tie_word_embeddings                                 # the lm_head is the embedding table: never quantised, bf16 fragments
    layer = sum(G.fragment_bytes(n, k) if four else 2 * n * k for n, k in tensors)
    return layer + 2 * t.vocab_size * h


def burst(e, knob, prompts, sampled, n_new=12):
    """chains 0 .. through one family-0 burst of n_new tokens under knob 24 = `knob`; then one more step on forced tokens for its
    logits.  Returns (ids per chain, logits bits, K/V bits per chain, fragment bytes)."""
    e.lib.ze_tune(24, knob)
    seqs = list(range(len(prompts)))
    for s, ids in zip(seqs, prompts):
        prefill_text(e, s, ids)
        if sampled:
            e.set_sampling(s, True, temperature=0.7 + 0.01 * s, seed=1000 + s, repetition_penalty=1.0 + 0.01 * (s % 5))
    if sampled:
        toks = e.generate_batch(seqs, n_new, ignore_eos=True, do_sample=True, temperature=1.0, seed=3)
    else:
        toks = e.generate_batch(seqs, n_new, repetition_penalty=1.3, ignore_eos=True)
    assert all(len(t) == n_new for t in toks)
    fb = e.fragment_bytes()
    logits = bits(e.decode_batch(seqs, [t[-1] for t in toks]))
    kv = [kv_rows(e, s, len(p) + n_new) for s, p in zip(seqs, prompts)]
    return toks, logits, kv, fb


def same_kv(a, b):
    return all(np.array_equal(x, y) for ca, cb in zip(a, b) for la, lb in zip(ca, cb) for x, y in zip(la, lb))


@pytest.mark.parametrize("n_chains,sampled", [(5, False), (5, True), (64, False), (64, True)])
def test_bursts_under_the_4_bit_stream_equal_the_dequantised_fragments(eng64, n_chains, sampled):
    e = eng64
    e.quantize_mxfp4()
    assert e.weight_format == "mxfp4"
    prompts = [text_ids(300 + s, 9 + (5 * s) % 23) for s in range(n_chains)]
    try:
        four = burst(e, 0, prompts, sampled)
        bf16 = burst(e, 1, prompts, sampled)
        again = burst(e, 0, prompts, sampled)                    # ... and back: the knob rebuilds the copies both ways
    finally:
        e.lib.ze_tune(24, 0)
    assert four[3] == expected_fragment_bytes(e, True) and bf16[3] == expected_fragment_bytes(e, False) and again[3] == four[3]
    for got in (four, again):
        assert got[0] == bf16[0]
        assert np.array_equal(got[1], bf16[1])
        assert same_kv(got[2], bf16[2])
    assert len({tuple(t) for t in four[0]}) > n_chains // 2        # the chains do differ


def test_a_speculating_chain_goes_through_the_rows_epilogue_of_the_w4_kernel(eng64):
    """one chain drafting k = 4 from a lookup text that holds its continuation, two plain ones, in the same family-0 bursts"""
    e = eng64
    e.quantize_mxfp4()
    prompts = [repeating(40), repeating(33, shift=2), text_ids(77, 25)]
    seqs = [0, 1, 2]

    def run(knob, lookup):
        e.lib.ze_tune(24, knob)
        for s, ids in zip(seqs, prompts):
            prefill_text(e, s, ids)
        if lookup is not None:
            e.set_speculation(0, 4, lookup, 1, 3)
        toks = e.generate_speculative(seqs, 12, repetition_penalty=1.3, ignore_eos=True)
        return toks, e.spec_stats(0), [kv_rows(e, s, len(p) + 11) for s, p in zip(seqs, prompts)]

    try:
        plain = run(1, None)
        lookup = prompts[0] + plain[0][0]
        four, bf16 = run(0, lookup), run(1, lookup)
    finally:
        e.lib.ze_tune(24, 0)
    assert four[1] == bf16[1] and four[1][2] > 0                   # drafts were accepted: the step did run rows behind the context
    assert four[0] == bf16[0] == plain[0]
    assert same_kv(four[2], bf16[2]) and same_kv(four[2], plain[2])


def test_life_cycle_around_a_weight_write(eng64):
    e = eng64
    name = "model.language_model.norm.weight"
    prompts = [text_ids(500 + s, 14 + s) for s in range(5)]
    try:
        e.quantize_mxfp4()
        ref = burst(e, 1, prompts, False)
        four = burst(e, 0, prompts, False)
        assert four[0] == ref[0] and four[3] == expected_fragment_bytes(e, True)
        e.load_weight(name, np.ones(e.config.text.hidden_size, dtype=np.float32))    # a weight write: back to bf16, the copies are dropped
        assert e.weight_format == "bf16" and e.fragment_bytes() == 0
        after = burst(e, 0, prompts, False)
        assert after[3] == expected_fragment_bytes(e, False)       # bf16 fragments whatever the knob says
        e.quantize_mxfp4()                                          # (quantising the dequantised values again changes nothing)
        again4, again16 = burst(e, 0, prompts, False), burst(e, 1, prompts, False)
        assert again4[3] == expected_fragment_bytes(e, True) and again16[3] == expected_fragment_bytes(e, False)
        assert again4[0] == again16[0] == after[0] and np.array_equal(again4[1], again16[1]) and np.array_equal(again4[1], after[1])
    finally:
        e.lib.ze_tune(24, 0)
        e.fill_synthetic(**CHAIN_W)

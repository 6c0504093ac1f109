"""GPU: the measurement entries (ze_profile_decode_kernel / _batch_kernel / _prefill_kernel / _prefill_layer) through the C ABI.

What they report besides a time is a property of the code: the algorithmic bytes (or FLOP) of the launch they timed, which follows
what the forward pass launches -- bf16 weights on a bf16 engine, the FP8 copy (1 byte per weight + one fp32 scale per row) where the
pass streams it.  No time bound is asserted: times on a shared machine are not a property of the code.

Engines: ModelConfig.heads() (head_dim 128, 2 layers: the fragment and per-wave paths are reachable), 66 chain slots, so both
kernel families of the batched step can be pinned.  The quantised engine has the same shape with an UNTIED lm_head: a tied head is the
embedding table and stays bf16, an untied one is quantised with the layers, and the batched lm_head launch then streams FP8 too."""
import dataclasses
import math

import numpy as np
import pytest
import torch

from gpu_util import CHAIN_W
from oracle import prng

pytestmark = pytest.mark.gpu

LENS = (5, 9, 14)          # the three ragged chains the narrow-regime cases run on
H, NQ, NKV, INTER, VOCAB = 2048, 2048, 256, 1376, 2048
NQKV = NQ + 2 * NKV
# (rows, cols) of the real shape: 0 qkv, 1 o, 2 gate_up, 3 down, 4 lm_head
SHAPES = ((NQKV, H), (H, NQ), (2 * INTER, H), (H, INTER), (VOCAB, H))


def bf16_bytes(which):
    r, c = SHAPES[which]
    return 2.0 * r * c


def fp8_bytes(which):
    r, c = SHAPES[which]
    return r * c + 4.0 * r


def _ids(seed, n):
    return prng.uniform_ints(seed, n, 10, 1990).tolist()


def _engine(untied):
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.engine import Engine
    cfg = ModelConfig.heads()
    if untied:
        cfg = dataclasses.replace(cfg, text=dataclasses.replace(cfg.text, tie_word_embeddings=False))
    assert (cfg.text.hidden_size, cfg.text.intermediate_size, cfg.text.vocab_size) == (H, INTER, VOCAB)
    e = Engine(cfg, device=0, max_seqs=66, max_ctx=256, max_patches=1024, max_tile_side=1024, max_prefill_rows=256)
    e.fill_synthetic(**CHAIN_W)
    return e


def _prefill_all(e):
    """Chains 0..2 with the ragged prompts, chains 3..64 with three tokens each (n = 65 in the row-streaming regime runs on chains
    that hold a context), in one pass of 214 rows."""
    lens = list(LENS) + [3] * 62
    ids = [_ids(100 + s, n) for s, n in enumerate(lens)]
    pl = [e.rope_index(i, []) for i in ids]
    for s in range(len(lens)):
        e.seq_reset(s)
    e.prefill_batch(list(range(len(lens))), ids, [None] * len(lens), [p[0] for p in pl], [p[1] for p in pl])
    return lens


@pytest.fixture(scope="module")
def eng():
    e = _engine(untied=False)
    e.lens = _prefill_all(e)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng8():
    e = _engine(untied=True)
    e.quantize_fp8()
    e.lens = _prefill_all(e)
    yield e
    e.close()


def _ok_time(us):
    assert math.isfinite(us) and us > 0.0


def _invalid(call, *args):
    from zoomearth_amd._lib import ZoomEarthError
    with pytest.raises(ZoomEarthError) as ei:
        call(*args)
    assert ei.value.code == -1 and "bad argument" in str(ei.value)   # ZE_ERR_INVALID


@pytest.mark.parametrize("which", range(5))
def test_decode_kernel_bytes(eng, eng8, which):
    us, by = eng.profile_decode_kernel(which, 4)
    _ok_time(us)
    assert by == bf16_bytes(which)
    us, by = eng8.profile_decode_kernel(which, 4)
    _ok_time(us)
    assert by == fp8_bytes(which)


def _batch_bytes(e, which, n, weights):
    if which <= 4:
        return weights(which)
    if which == 5:
        return float(sum((e.lens[i] + 1) * NKV * 4 for i in range(n)))
    return float(n * (H if which == 6 else NQKV) * 4)


@pytest.mark.parametrize("n", (1, 3))
def test_batch_kernel_bytes_fragment_regime(eng, n):
    assert eng.set_decode_regime(0) == 0
    for which in range(8):
        us, by = eng.profile_batch_kernel(which, n, 4)
        print(f"bf16 n={n} which={which}: {us:.2f} us, {by:.0f} B")
        _ok_time(us)
        assert by == _batch_bytes(eng, which, n, bf16_bytes)


@pytest.mark.parametrize("n", (1, 3))
def test_batch_kernel_streams_fp8_on_a_quantised_engine(eng8, n):
    """The batched step of a quantised engine streams the FP8 fragments of qkv, o, gate/up and the (untied) lm_head; the down
    projection stays on the bf16 split-K ring.  The profiler times -- and counts -- the same."""
    assert eng8.set_decode_regime(0) == 0
    for which in range(8):
        us, by = eng8.profile_batch_kernel(which, n, 4)
        print(f"fp8 n={n} which={which}: {us:.2f} us, {by:.0f} B")
        _ok_time(us)
        assert by == _batch_bytes(eng8, which, n, lambda w: bf16_bytes(w) if w == 3 else fp8_bytes(w))


def test_batch_kernel_beyond_64_chains(eng):
    assert eng.set_decode_regime(0) == 0
    for which in range(8):
        _invalid(eng.profile_batch_kernel, which, 65, 4)   # the fragment kernels take at most 64 chains
    assert eng.set_decode_regime(1) == 1
    try:
        for which in range(7):
            us, by = eng.profile_batch_kernel(which, 65, 4)
            _ok_time(us)
            assert by == _batch_bytes(eng, which, 65, bf16_bytes)
    finally:
        eng.set_decode_regime(0)


@pytest.mark.parametrize("rows", (8, 130))
def test_prefill_profilers(eng, rows):
    flops = [2.0 * rows * r * c for r, c in SHAPES[:4]]
    # a hidden-state-dependent result before the profilers run ...
    ids = _ids(7, 11)
    pos, delta = eng.rope_index(ids, [])
    eng.seq_reset(65)
    before = eng.prefill(65, ids, None, pos, delta).cpu().numpy()
    step_before = eng.decode_step(65, 123).cpu().numpy()
    for which in range(4):
        us, fl = eng.profile_prefill_kernel(which, rows, 2)
        _ok_time(us)
        assert fl == flops[which]
    lay = eng.profile_prefill_layer(rows, 2)
    for which, name in enumerate(("qkv", "o", "gate_up", "down")):
        _ok_time(lay[name][0])
        assert lay[name][1] == flops[which]
    # ... and after: the residual stream is read, never written
    eng.seq_truncate(65, len(ids))
    assert np.array_equal(eng.decode_step(65, 123).cpu().numpy(), step_before)
    eng.seq_reset(65)
    assert np.array_equal(eng.prefill(65, ids, None, pos, delta).cpu().numpy(), before)


def test_bad_arguments(eng):
    eng.set_decode_regime(0)
    _invalid(eng.profile_decode_kernel, 0, 0)            # iters = 0
    _invalid(eng.profile_batch_kernel, 0, 1, 0)
    _invalid(eng.profile_batch_kernel, 0, 0, 4)          # n = 0
    _invalid(eng.profile_prefill_kernel, 0, 8, 0)
    _invalid(eng.profile_prefill_kernel, 0, 0, 2)        # rows = 0
    _invalid(eng.profile_prefill_kernel, 0, 257, 2)      # rows > max_prefill_rows
    _invalid(eng.profile_prefill_kernel, 4, 8, 2)
    _invalid(eng.profile_prefill_layer, 0, 2)
    _invalid(eng.profile_prefill_layer, 257, 2)
    _invalid(eng.profile_prefill_layer, 8, 0)

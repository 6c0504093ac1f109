"""GPU: every attention kernel against float64 on PLANTED inputs (tests/attn_edge_ref.py): needle queries whose mass sits on one or
two keys at a mask edge, a segment end, a key-tile edge or a part boundary, and poison in the rows just outside the visible set.
tests/test_attn_edge_cpu.py proves that one key too many, too few or read twice at any of those places moves the reference by at
least 16 x the bounds applied here -- the bounds of the existing float64 tests on diffuse inputs, unchanged: 2^-6 max(1, max |want|)
for the flash kernel, 2^-7 max |V visible| for the decode kernels."""
import numpy as np
import pytest
import torch

import attn_edge_ref as R
import parity_ledger
from gpu_util import CHAIN_W, tiny_engine, to_dev_bf16  # noqa: F401
from oracle import prng

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------ flash
@pytest.mark.parametrize("D,causal,ci,kvh", R.flash_cases())
def test_flash_attention_on_planted_edges(tiny_engine, D, causal, ci, kvh):
    """ze_op_attention in every form the unit op reaches -- 128-row query tiles (knob 1 = 0), 64-row tiles (9) and, for D = 128 causal,
    the register-staged form (7) next to the LDS-DMA one -- on q / k / v allocated with 64 poison rows behind T: the probed rows
    against float64 over their true visible set, and the same bits from every form."""
    e, c = tiny_engine, R.flash_case(D, causal, ci, kvh)
    T = c.T
    dq, dk, dv = to_dev_bf16(c.q), to_dev_bf16(c.k), to_dev_bf16(c.v)
    assert dq.shape[0] == T + R.FLASH_PAD and np.array_equal(dk.float().cpu().numpy(), c.k)
    forms = [0, 9] + ([7] if D == 128 and causal else [])
    outs = {}
    try:
        for knob in forms:
            e.lib.ze_tune(1, knob)
            outs[knob] = e.op_attention(dq[:T], dk[:T], dv[:T], c.cu, causal)
    finally:
        e.lib.ze_tune(1, 0)
    rows = torch.tensor([p.where for p in c.probes], device="cuda")
    heads = torch.tensor([p.head for p in c.probes], device="cuda")
    for knob in forms:
        got = outs[knob][rows, heads].float().cpu().numpy()
        err = np.abs(got - c.want).max(axis=1)
        worst = int(err.argmax())
        p = c.probes[worst]
        print(f"flash D {D} causal {causal} cu {ci} kv heads {kvh} knob 1 = {knob}: worst error / bound {err.max() / c.bound:.3f} "
              f"(query {p.where}, head {p.head}, targets {p.pair}, mode {p.mode})")
        parity_ledger.record(float(err.max()), c.bound, f"flash attention on planted edges, D {D} causal {causal} cu {ci} kv heads {kvh} "
                             f"knob 1 = {knob}: max |got - float64| over the probed rows / (2^-6 max(1, max |want|))", bar=1.0)
        assert err.max() <= c.bound, (knob, p.where, p.head, p.pair, p.mode, float(err.max()), c.bound)
    for knob in forms[1:]:
        assert torch.equal(outs[knob], outs[0]), knob


# ------------------------------------------------------------------------------------------------------------------ decode
def _attn_engine(n, name):
    """the engine of tests/test_gpu_ops_kernels.py's float64 decode-attention test: 16 q heads on 2 kv heads, one layer, max_ctx 1024"""
    from zoomearth_amd.config import ModelConfig, TextConfig, VisionConfig
    from zoomearth_amd.engine import Engine
    cfg = ModelConfig(vision=VisionConfig(depth=1, hidden_size=160, num_heads=2, intermediate_size=220, out_hidden_size=2048,
                                          fullatt_block_indexes=(0,)),
                      text=TextConfig(hidden_size=2048, num_hidden_layers=1, num_attention_heads=R.HEADS, num_key_value_heads=R.KV_HEADS,
                                      intermediate_size=1024, vocab_size=2048, tie_word_embeddings=True),
                      image_token_id=2005, vision_start_token_id=2002, vision_end_token_id=2003, eos_token_ids=(2045, 2043),
                      pad_token_id=2043, name=name)
    e = Engine(cfg, device=0, max_seqs=n, max_ctx=R.MAX_CTX, max_patches=256, max_tile_side=256)
    e.fill_synthetic(seed=3, std=0.02, matrix_gain=4.0, bias_std=0.5, norm_jitter=0.1)
    return e


def _prefill(e, seq, n_rows, seed):
    ids = prng.uniform_ints(seed, n_rows, 10, 1990).tolist()
    e.seq_reset(seq)
    e.prefill(seq, ids, None, *e.rope_index(ids, []), want_logits=False)


def _plant(e, seq, rows, past):
    """rows [n, (heads + 2 kv) x 128] -> the chain's K / V cache at `past`, through the M-RoPE append at position 0 (a rotation by
    the angle 0: K goes in bit for bit, V is never rotated); then read back and compared -- the premise of every check below"""
    n = rows.shape[0]
    e.op_mrope_kv(seq, 0, to_dev_bf16(rows), np.zeros((3, n), np.int32), past)
    k, v = [x.float().cpu().numpy() for x in e.op_kv_read(seq, 0, past, n)]
    nq, nkv = R.HEADS * R.HD, R.KV_HEADS * R.HD
    assert np.array_equal(k, rows[:, nq: nq + nkv].reshape(n, R.KV_HEADS, R.HD).transpose(1, 0, 2)), seq
    assert np.array_equal(v, rows[:, nq + nkv:].reshape(n, R.KV_HEADS, R.HD).transpose(1, 0, 2)), seq


def _check_rows(form, chains, r, got, worst):
    """got [len(chains), heads, 128] of pass r against float64; worst[form] = the largest error / bound so far"""
    for b, c in enumerate(chains):
        for p in c.probes(r):
            err = float(np.abs(got[b, p.head] - c.result(p)).max())
            bound = c.bound[p.kvh]
            worst[form] = max(worst.get(form, 0.0), err / bound)
            assert err <= bound, (form, c.ctx, c.split, c.own_from, r, p.head, p.pair, p.mode, err, bound)


def _record(worst, what):
    for form, ratio in worst.items():
        print(f"{what}, {form}: worst error / bound {ratio:.3f}")
        parity_ledger.record(ratio, 1.0, f"{what}, {form}: max |got - float64| / (2^-7 max |V visible|) over every chain, pass and head", bar=1.0)


FORMS = {0: "knob 8 = 0 k_attn_decode_wave_long (384-key parts)", 4: "knob 8 = 4 k_attn_decode_wave (192-key parts)",
         2: "knob 8 = 2 k_attn_decode_stream", 1: "knob 8 = 1 k_attn_decode_split<8, 1> (64-key slices)"}
SINGLE = "k_attn_decode_split<24, 1> (the single-chain step)"
SPLIT = "knob 23 = 2 k_attn_decode_wave_long cut at the split row"


def test_decode_attention_on_planted_part_boundaries():
    """ze_op_attn_decode in all four forms (ze_tune knob 8), the split-row form (knob 23 = 2: split 347 under contexts 731 and 384) and
    ze_op_attn_decode_single (the <24, 1> instantiation the batch-1 decode step launches) on planted caches: rows 0 .. ctx hold the
    planted K / V, the DEAD rows behind ctx hold poison, the queries are needles on the last rows, on row 0 and on either side of the
    last part boundary of every partition.  Contexts: those of the existing float64 test.  A chain's row alone = in the batch."""
    chains = R.decode_chains()
    n = len(chains)
    e = _attn_engine(n, "attn-edges")
    worst = {}
    try:
        for s, c in enumerate(chains):
            _prefill(e, s, c.ctx, 300 + s)
            assert e.seq_len(s) == c.ctx
        seqs = list(range(n))
        for r in range(max(c.passes for c in chains)):
            for s, c in enumerate(chains):
                rows = c.cache_rows(r)
                if r == 0:
                    _plant(e, s, rows, 0)
                else:                                                   # the dead rows follow the pass's targets; rows 0 .. ctx stay
                    _plant(e, s, rows[c.ctx + 1:], c.ctx + 1)
            qkv = to_dev_bf16(np.stack([c.qkv_row(r) for c in chains]))
            for knob, form in FORMS.items():
                e.lib.ze_tune(8, knob)
                out = e.op_attn_decode(seqs, 0, qkv)
                _check_rows(form, chains, r, out.float().cpu().numpy().reshape(n, R.HEADS, R.HD), worst)
                for b in (0, 6, 12, 17, n - 2):
                    assert torch.equal(e.op_attn_decode([b], 0, qkv[b:b + 1].contiguous())[0], out[b]), (form, chains[b].ctx)
            e.lib.ze_tune(8, 0)
            single = torch.stack([e.op_attn_decode_single(s, 0, qkv[s].contiguous()) for s in seqs])
            _check_rows(SINGLE, chains, r, single.float().cpu().numpy().reshape(n, R.HEADS, R.HD), worst)
            for s, c in enumerate(chains):
                e.seq_set_split(s, c.split)
            e.lib.ze_tune(23, 2)
            out = e.op_attn_decode(seqs, 0, qkv)
            _check_rows(SPLIT, chains, r, out.float().cpu().numpy().reshape(n, R.HEADS, R.HD), worst)
            for b in (n - 2, n - 1):
                assert torch.equal(e.op_attn_decode([b], 0, qkv[b:b + 1].contiguous())[0], out[b]), (SPLIT, chains[b].ctx)
            e.lib.ze_tune(23, 0)
            for s in seqs:
                e.seq_set_split(s, 0)
        _record(worst, "decode attention on planted part boundaries")
        assert set(worst) == set(FORMS.values()) | {SINGLE, SPLIT}
    finally:
        e.lib.ze_tune(8, 0)
        e.lib.ze_tune(23, 0)
        e.close()


def test_decode_attention_reads_a_hinted_prefix_from_the_holder():
    """ze_seq_set_prefix_hint(B, A, rows), rows in {347, 383, 384}: the per-wave kernels (knob 8 = 0 and 4, the ones that take the
    hint) read rows [0, rows) from A's slot and rows rows .. ctx from B's own.  A holds the true prefix, B's own rows below `rows`
    hold poison, A's row `rows` holds poison; the needles sit on row rows - 1 (A's) and on row rows (B's)."""
    pairs = R.prefix_pairs()
    chains = [c for ab in pairs for c in ab]
    e = _attn_engine(len(chains), "attn-prefix")
    worst = {}
    try:
        for s, c in enumerate(chains):
            _prefill(e, s, c.ctx, 500 + s)
            _plant(e, s, c.cache_rows(0), 0)
        readers = [2 * i + 1 for i in range(len(pairs))]
        for b in readers:
            e.seq_set_prefix_hint(b, b - 1, chains[b].own_from)
        qkv = to_dev_bf16(np.stack([chains[b].qkv_row(0) for b in readers]))
        for knob in (0, 4):
            e.lib.ze_tune(8, knob)
            out = e.op_attn_decode(readers, 0, qkv)
            _check_rows(FORMS[knob], [chains[b] for b in readers], 0, out.float().cpu().numpy().reshape(len(readers), R.HEADS, R.HD), worst)
            for i, b in enumerate(readers):
                assert torch.equal(e.op_attn_decode([b], 0, qkv[i:i + 1].contiguous())[0], out[i]), (knob, chains[b].own_from)
        _record(worst, "decode attention over a hinted prefix")
    finally:
        e.lib.ze_tune(8, 0)
        e.close()


@pytest.mark.parametrize("keep", [191, 383, 384])
def test_a_decode_step_over_dead_rows_gives_the_bits_of_a_fresh_chain(tiny_engine, keep):
    """Dead rows end to end: a chain prefilled to 400 rows and truncated to `keep` (rows keep .. 399 stay in the cache, as rejected
    speculative rows and reused slots leave them) takes one batched decode step and one single-chain decode step; the logits are the
    bits of a chain that was prefilled with the first `keep` ids and nothing else."""
    e = tiny_engine
    e.fill_synthetic(**CHAIN_W)
    ids = prng.uniform_ints(811, 400, 10, 1990).tolist()
    tok = 77

    def chain(seq, n_rows):
        e.seq_reset(seq)
        e.prefill(seq, ids[:n_rows], None, *e.rope_index(ids[:n_rows], []), want_logits=False)

    chain(0, 400)
    e.seq_truncate(0, keep)
    chain(1, keep)
    chain(2, keep)
    assert e.seq_len(0) == keep == e.seq_len(1)
    dead, fresh = e.decode_batch([0], [tok]), e.decode_batch([1], [tok])
    assert torch.equal(dead, fresh)
    e.seq_truncate(0, keep)                      # row `keep`, written by the step, is dead again; rows keep + 1 .. 399 still are
    assert torch.equal(e.decode_step(0, tok), e.decode_step(2, tok))
    assert torch.equal(e.decode_step(0, tok + 1), e.decode_step(2, tok + 1))

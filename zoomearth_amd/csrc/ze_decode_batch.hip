// The batched decode of the engine: the step over a set of rows (one launch function per kind, one layer loop, one sampler launch,
// one cache of captured steps), the plain, beam and speculative ways of running it, and continuous batching on top of them.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ze_engine.h"

// ================================================================== batched decode (BASELINE configs[2])
// One token for each of n chains per step: the weights are streamed ONCE for the whole batch through the MFMA GEMM
// path (rows = chains), each chain keeps its own KV cache / position / seen-set.  Rows are computed independently of
// the batch composition (same per-element accumulation order for every tile shape), so a chain's tokens do not
// depend on which other chains share its steps.
// Fragment-major copies of the wide, short-K decode projections for the batched step (see ze_engine.h).  Shapes the
// fragment kernel does not cover (rows % 16, K % 32, K > 4096) keep wf = null and stay on the row-major launchers.
// MXFP4 engine: the 4-bit fragment stream of the 2 .. 64-chain step (ze_tune knob 24 = 1: dequantised bf16 fragments, the form before
// the W4 kernels -- same bits; kept for the A/B and the bit-equality test)
static bool want_frag4(const ze_engine* e) { return e->mx4_ready && ze_knobs[ZE_KNOB_MX4_BF16_FRAGMENTS] != ZE_KNOB_ON; }

int ensure_fragments(ze_engine* e, hipStream_t s) {
    if (e->frag_ready && e->frag_w4 == want_frag4(e)) return ZE_OK;
    const ze_config& c = e->cfg;
    const int H = c.hidden, hd = e->head_dim, nq = c.heads * hd, nqkv = nq + 2 * c.kv_heads * hd, ip = e->text_ipad;
    const bool ok = H % 32 == 0 && H <= 4096 && nq % 32 == 0 && nq <= 4096 && nqkv % 16 == 0 && (2 * ip) % 32 == 0 && c.vocab % 16 == 0;
    for (int li = 0; li < c.layers; ++li) {
        ze_text_layer& L = e->tl[li];
        L.qkv.wf = L.o.wf = L.gate_up.wf = nullptr;
        L.qkv.wf8 = L.o.wf8 = L.gate_up.wf8 = nullptr;   // (these stayed stale in the row-streaming regime)
        L.qkv.wf4 = L.o.wf4 = L.gate_up.wf4 = nullptr;
        L.qkv.sf4 = L.o.sf4 = L.gate_up.sf4 = nullptr;
        L.qkv.wp = L.qkv.bias_p = nullptr;
    }
    e->lm_head_f = nullptr;
    e->lm_head8.wf8 = nullptr;
    e->lm_head8.wf4 = e->lm_head8.sf4 = nullptr;
    e->frag_ready = false;
    // Each kernel family gets only the copies it reads: the row-streaming regime the permuted qkv rows (0.38 GB at the
    // 3B shape), the fragment family the fragment-major arena (4.5 GB) -- an engine of 64 slots never runs the first, one of 768
    // never the second.  ze_set_decode_regime clears frag_ready, so a regime change rebuilds what the new family needs.
    const bool wide = e->wide_regime();
    // ... and the OTHER family's copies are given back (after ze_set_decode_regime the 4.5-GB fragment arena, its FP8 twin
    // and the permuted qkv rows all stayed allocated).  A regime change is rare and never concurrent with a step: wait for the device.
    if (wide ? (e->arena_f || e->arena_f8 || e->arena_f4) : (e->arena_p != nullptr)) {
        ZE_HIP(hipDeviceSynchronize());
        if (wide) {
            if (e->arena_f) hipFree(e->arena_f);
            if (e->arena_f8) hipFree(e->arena_f8);
            if (e->arena_f4) hipFree(e->arena_f4);
            e->arena_f = nullptr;
            e->arena_f8 = nullptr;
            e->arena_f4 = nullptr;
            e->arena_f_bytes = e->arena_f8_bytes = e->arena_f4_bytes = 0;
        } else {
            hipFree(e->arena_p);
            e->arena_p = nullptr;
        }
    }
    // row-streaming regime: the qkv rows permuted per head, so that M-RoPE + the KV append run as the projection's epilogue
    if (wide && hd == 128 && H % 64 == 0 && H / 64 >= 4 && nqkv % 128 == 0) {
        const size_t per_layer = (size_t)nqkv * H + nqkv;
        if (!e->arena_p) ZE_HIP(hipMalloc((void**)&e->arena_p, per_layer * c.layers * sizeof(bf16_t)));
        if (!e->qkv_epi_dev) ZE_HIP(hipMalloc((void**)&e->qkv_epi_dev, sizeof(ze_qkv_epi) * c.layers));
        std::vector<ze_qkv_epi> host(c.layers);
        for (int li = 0; li < c.layers; ++li) {
            ze_text_layer& L = e->tl[li];
            bf16_t* wp = e->arena_p + per_layer * li;
            bf16_t* bp = wp + (size_t)nqkv * H;
            ze_launch_permute_qkv(L.qkv.w, L.qkv.ld, L.qkv.bias, nqkv / 128, H, wp, L.qkv.bias ? bp : nullptr, s);
            L.qkv.wp = wp;
            L.qkv.bias_p = L.qkv.bias ? bp : nullptr;
            ze_qkv_epi& q = host[li];
            memset(&q, 0, sizeof(q));
            q.st = e->st_dev;
            q.seq_ids = e->bseq;
            q.cosT = e->cosT;
            q.sinT = e->sinT;
            q.kcache = e->kc(li, 0);
            q.vcache = e->vc(li, 0);
            q.cache_seq_stride = (size_t)c.kv_heads * c.max_ctx * hd;
            q.max_ctx = c.max_ctx;
            q.heads = c.heads;
            q.kv_heads = c.kv_heads;
        }
        ZE_HIP(hipMemcpyAsync(e->qkv_epi_dev, host.data(), sizeof(ze_qkv_epi) * c.layers, hipMemcpyHostToDevice, s));
        ZE_HIP(hipStreamSynchronize(s));  // (host is a local)
        ZE_KCHECK();
    }
    if (ok && !wide) {
        // MXFP4 engine (want_frag4): a tensor the quantiser took (w4: K % 32 == 0) gets the 4-bit fragment copy INSTEAD of the bf16 one --
        // codes + fragment-major scales, 4.25 bits per weight; every other tensor (a tied lm_head: the embedding table) bf16 fragments
        const bool f4 = want_frag4(e);
        struct item {
            ze_linear* l;
            int rows, cols, rope_dim;
        };
        std::vector<item> items;
        for (int li = 0; li < c.layers; ++li) {
            ze_text_layer& L = e->tl[li];
            items.push_back({&L.qkv, nqkv, H, hd});  // rows permuted per head for the fused M-RoPE epilogue (ze_gemm_oneshot.hip)
            items.push_back({&L.o, H, nq, 0});
            items.push_back({&L.gate_up, 2 * ip, H, 0});
        }
        const bool head4 = f4 && e->lm_head8.w4 != nullptr;
        size_t elems16 = head4 ? 0 : (size_t)c.vocab * H, bytes4 = head4 ? (size_t)c.vocab * H / 2 + (size_t)c.vocab * H / 32 : 0;
        for (const item& it : items) {
            if (f4 && it.l->w4) bytes4 += (size_t)it.rows * it.cols / 2 + (size_t)it.rows * it.cols / 32;
            else elems16 += (size_t)it.rows * it.cols;
        }
        // (the two arenas are sized for the format in force: a format or knob change is rare and never concurrent with a step)
        if (e->arena_f_bytes != elems16 * sizeof(bf16_t) || e->arena_f4_bytes != bytes4) {
            ZE_HIP(hipDeviceSynchronize());
            if (e->arena_f) hipFree(e->arena_f);
            if (e->arena_f4) hipFree(e->arena_f4);
            e->arena_f = nullptr;
            e->arena_f4 = nullptr;
            e->arena_f_bytes = e->arena_f4_bytes = 0;
            if (elems16) ZE_HIP(hipMalloc((void**)&e->arena_f, elems16 * sizeof(bf16_t)));
            e->arena_f_bytes = elems16 * sizeof(bf16_t);
            if (bytes4) ZE_HIP(hipMalloc((void**)&e->arena_f4, bytes4));
            e->arena_f4_bytes = bytes4;
        }
        bf16_t* cur = e->arena_f;
        uint8_t* cur4 = e->arena_f4;
        auto pack = [&](ze_linear& l, int rows, int cols, int rope_dim) {
            if (f4 && l.w4) {
                l.wf4 = cur4;
                l.sf4 = cur4 + (size_t)rows * cols / 2;
                ze_launch_pack_fragments4(l.w4, l.scale4, rows, cols, l.wf4, l.sf4, s, rope_dim);
                cur4 = l.sf4 + (size_t)rows * cols / 32;
                return;
            }
            ze_launch_pack_fragments(l.w, l.ld, rows, cols, cur, s, rope_dim);
            l.wf = cur;
            cur += (size_t)rows * cols;
        };
        for (const item& it : items) pack(*it.l, it.rows, it.cols, it.rope_dim);
        if (head4) {
            pack(e->lm_head8, c.vocab, H, 0);
        } else {
            ze_launch_pack_fragments(e->lm_head, H, c.vocab, H, cur, s);
            e->lm_head_f = cur;
        }
        // FP8 engine: the same fragments at one byte per weight (qkv, o, gate/up, an untied lm_head); the batched step
        // streams these and dequantises in registers -- identical values, half the weight bytes
        for (int li = 0; li < c.layers; ++li) {
            ze_text_layer& L = e->tl[li];
            L.qkv.wf8 = L.o.wf8 = L.gate_up.wf8 = nullptr;
        }
        e->lm_head8.wf8 = nullptr;
        if (e->fp8_ready) {
            const bool head8 = e->lm_head8.w8 != nullptr;
            const size_t bytes = ((size_t)(nqkv + 2 * ip) * H + (size_t)H * nq) * c.layers + (head8 ? (size_t)c.vocab * H : 0);
            if (!e->arena_f8) ZE_HIP(hipMalloc((void**)&e->arena_f8, bytes));
            e->arena_f8_bytes = bytes;
            uint8_t* c8 = e->arena_f8;
            auto pack8 = [&](ze_linear& l, int rows, int cols, int rope_dim) {
                ze_launch_pack_fragments8(l.w8, l.ld8, rows, cols, c8, s, rope_dim);
                l.wf8 = c8;
                c8 += (size_t)rows * cols;
            };
            for (int li = 0; li < c.layers; ++li) {
                ze_text_layer& L = e->tl[li];
                pack8(L.qkv, nqkv, H, hd);
                pack8(L.o, H, nq, 0);
                pack8(L.gate_up, 2 * ip, H, 0);
            }
            if (head8) pack8(e->lm_head8, c.vocab, H, 0);
        }
        ZE_KCHECK();
    }
    e->frag_ready = true;
    e->frag_w4 = want_frag4(e);
    return ZE_OK;
}

// parts of `keys` keys as the per-wave attention kernels cut them: 192 keys, and the pipelined kernel's 384
static int parts_192(int keys) { return (keys + 191) / 192; }
static int parts_384(int keys) { return (keys + 383) / 384; }

// the attention grid's extent for the next `steps` decode steps of these chains: the parts of the longest context
void set_live_parts(ze_engine* e, const int32_t* seqs, int n, int steps) {
    int mx = 0, ml = 0;
    for (int i = 0; i < n; ++i) {
        const int c = e->ctx_host[seqs[i]] + std::max(1, steps) + 1, sp = e->split_host[seqs[i]];
        mx = std::max(mx, e->ctx_host[seqs[i]]);
        ml = std::max(ml, parts_384(sp) + parts_384(c - sp));   // (the pipelined kernel's 384-key parts under the chain's split)
    }
    e->live_parts = parts_192(mx + std::max(1, steps) + 1);
    e->live_parts_long = ml;
}
// ... of a step whose rows name a chain more than once (no split rows: spec_step_ok): the longest context any row can reach is mx
static void set_live_parts_reach(ze_engine* e, int mx) {
    e->live_parts = parts_192(mx);
    e->live_parts_long = parts_384(mx);
}

// Round 6: which rows of the step share their PREFIX parts (ze_attn_batch.hip).  Two chains pair when they have the same split row and
// read the rows below it from the same holder -- the holder itself included -- under the hints this very step uses (sync_prefix ran on
// this stream just before): first come, first paired, in batch order (the questions of a tile sit next to each other).  Symmetric;
// -1 = alone.  A pairing changes who computes a partial, never its bits.
static void upload_mates(ze_engine* e, const int32_t* seqs, int n, hipStream_t s) {
    std::vector<int> mate(n, -1);
    if (e->prefix_hints && ze_knobs[ZE_KNOB_NO_PREFIX_HINTS] != ZE_KNOB_ON) {
        std::map<long long, int> open;   // (holder, split) -> the row waiting for a partner
        for (int i = 0; i < n; ++i) {
            const int q = seqs[i], sp = e->split_host[q];
            if (sp <= 0) continue;
            const int h = e->pfx_pushed[q];
            const int holder = (h != 0 && (h & 0xffff) >= sp) ? (h >> 16) : q;
            const long long key = ((long long)holder << 20) | (long long)sp;
            auto it = open.find(key);
            if (it == open.end()) open[key] = i;
            else {
                mate[i] = it->second;
                mate[it->second] = i;
                open.erase(it);
            }
        }
    }
    ze_launch_set_ints(e->bmate, mate.data(), n, s);
}

// Before `steps` steps of the chains `seqs` on the engine's own buffers: the row table, the prefix hints, the mates and the grids'
// extents.  stage_batch trusts its chains (ze_profile_batch_kernel's are slots 0 .. n - 1); begin_batch checks them first.
void stage_batch(ze_engine* e, const int32_t* seqs, int n, int steps, hipStream_t s) {
    ze_launch_set_ints(e->bseq, seqs, n, s);
    sync_prefix(e, seqs, n, s);
    upload_mates(e, seqs, n, s);
    set_live_parts(e, seqs, n, steps);
}

static int begin_batch(ze_engine* e, const int32_t* seqs, int n, int steps, hipStream_t s) {
    if (n <= 0 || n > e->cfg.max_seqs) return ze_fail(e, ZE_ERR_INVALID, "batch size out of range");
    if (n > 64 && !e->wide_regime())
        return ze_fail(e, ZE_ERR_INVALID, "more than 64 chains in a step of an engine pinned to the fragment kernels (ze_set_decode_regime)");
    for (int i = 0; i < n; ++i) {
        if (seqs[i] < 0 || seqs[i] >= e->cfg.max_seqs) return ze_fail(e, ZE_ERR_NOTFOUND, "sequence id out of range");
        for (int j = 0; j < i; ++j)
            if (seqs[j] == seqs[i]) return ze_fail(e, ZE_ERR_INVALID, "duplicate sequence id in a batch");
        if (e->ctx_host[seqs[i]] + 1 > e->cfg.max_ctx) return ze_fail(e, ZE_ERR_NOMEM, "sequence exceeds max_ctx");
    }
    stage_batch(e, seqs, n, steps, s);
    return ZE_OK;
}

// ... and behind them: every chain is `steps` rows longer, and its row of dlogits is no longer what its prefill left
static void end_batch(ze_engine* e, const int32_t* seqs, int n, int steps) {
    for (int i = 0; i < n; ++i) e->ctx_host[seqs[i]] += steps, e->logits_fresh[seqs[i]] = 0;
}

// The rows of a step (ze_engine.h).  The plain step, beam search, ze_decode_batch and the profiler run on the engine's own buffers.
ze_step_rows ze_rows_own(const ze_engine* e) {
    return ze_step_rows{e->bseq, nullptr, e->bmate, e->bqkv, e->bo, e->blogits, e->bpartial, e->atickets};
}
// The speculative row table, with logits, partials and tickets of its own (a step may have more rows than the engine has slots).
// Its chain ids are NOT in e->bseq -- and in the row-streaming regime the fused qkv epilogue reads its chain ids through
// ze_qkv_epi::seq_ids, which ensure_fragments bakes in from e->bseq once: a step of that regime must use e->bseq as its row table.
// The callers of this function refuse that regime (spec_step_ok).
ze_step_rows ze_rows_spec(const ze_engine* e) {
    const ze_spec& q = e->spec;
    return ze_step_rows{q.row_seq, q.row_off, nullptr, e->bqkv, e->bo, q.logits, q.partial, q.tickets};
}
// The chains of e->bseq on the caller's q / out rows, unpaired (no upload_mates ran for them).
ze_step_rows ze_rows_caller(const ze_engine* e, const bf16_t* q, bf16_t* out) {
    return ze_step_rows{e->bseq, nullptr, nullptr, q, out, e->blogits, e->bpartial, e->atickets};
}

// whether the step's decode attention is a per-wave kernel (192- or 384-key parts whatever the context): ceil(max_ctx / 192) parts must
// fit the partial buffer (max(max_splits, 8) parts per chain) and the merge's 64 lanes; 128-wide heads, the q heads of a kv head as
// MFMA columns.  One predicate for the plain step and for the steps whose rows name a chain more than once (spec_step_ok).
static bool attn_per_wave(const ze_engine* e) {
    const ze_config& c = e->cfg;
    const int wparts = (c.max_ctx + 191) / 192;
    return ze_knobs[ZE_KNOB_BATCH_ATTN] != ZE_ATTN_RING && ze_knobs[ZE_KNOB_RING_ATTN_PART] == 0 && wparts <= std::max(e->max_splits, 8) && wparts <= 64 && e->head_dim == 128 &&
           c.heads / c.kv_heads <= 16;
}

// decode attention of the batched step: the per-wave streaming kernel k_attn_decode_wave (ze_attn_batch.hip); knob 8 = 2:
// its predecessor k_attn_decode_stream (a workgroup-wide LDS-DMA ring); knob 8 = 1: the 64-token-slice kernel of the
// single-chain step with a chain dimension (the round-1 form) -- both kept for A/B measurements
void launch_batch_attention(ze_engine* e, const ze_step_rows& rows, int li, int n, bool frag_out, hipStream_t s) {
    const ze_config& c = e->cfg;
    const int hd = e->head_dim, nq = c.heads * hd, nqkv = nq + 2 * c.kv_heads * hd;
    const size_t seq_stride = (size_t)c.kv_heads * c.max_ctx * hd;
    const float scale = 1.0f / sqrtf((float)hd);
    if (rows.off) {  // rows at offsets behind their chains' contexts (spec_step_ok: the pipelined kernel is the one in force)
        ze_launch_attn_decode_rows(rows.q, nqkv, e->kc(li, 0), e->vc(li, 0), seq_stride, rows.out, frag_out ? -(nq / 32) : nq, e->st_dev, rows.seq,
                                   rows.off, n, c.heads, c.kv_heads, c.max_ctx, scale, rows.partial, rows.tickets, e->live_parts_long, e->pfx_dev, s);
        return;
    }
    if (ze_knobs[ZE_KNOB_BATCH_ATTN] == ZE_ATTN_SLICE)
        ze_launch_attn_decode(rows.q, nqkv, e->kc(li, 0), e->vc(li, 0), seq_stride, rows.out, frag_out ? -(nq / 32) : nq, e->st_dev,
                              rows.seq, n, c.heads, c.kv_heads, hd, c.max_ctx, scale, rows.partial, e->max_splits, rows.tickets, s);
    else {
        // tokens per part (a multiple of 32; knob 11 for measurements): a function of nothing but the build, so a chain's
        // partition depends on its own context length alone
        // the per-wave kernel cuts 192-key parts whatever the context: ceil(max_ctx / 192) of them must fit the partial buffer
        // (max(max_splits, 8) parts per chain) and the merge's 64 lanes
        const int wparts = (c.max_ctx + 191) / 192;
        const bool per_wave = attn_per_wave(e);
        const int chunk = ze_knobs[ZE_KNOB_RING_ATTN_PART] >= 64 ? ze_knobs[ZE_KNOB_RING_ATTN_PART] / 32 * 32 : 0;  // 0: a sixth of the chain's context
        const int max_parts = chunk ? (c.max_ctx + chunk - 1) / chunk : 8;           // (at most 8 parts: 128-token floor)
        ze_launch_attn_decode_stream(rows.q, nqkv, e->kc(li, 0), e->vc(li, 0), seq_stride, rows.out, frag_out ? -(nq / 32) : nq,
                                     e->st_dev, rows.seq, n, c.heads, c.kv_heads, c.max_ctx, scale, rows.partial, max_parts,
                                     rows.tickets, s, chunk, per_wave ? (e->live_parts > 0 ? e->live_parts : wparts) : 0, e->pfx_dev,
                                     rows.mate, e->live_parts_long, 1);
    }
}

// Which kernel family the projections of a batched step run on, decided here and nowhere else.
//   fr / fl: every layer projection / the lm_head on fragment-major operands when the copy exists (ensure_fragments) and n <= 64:
//     the norms, the attention merge and the SwiGLU epilogue then write their outputs in that layout too
//   tiled: beyond 64 chains (no fragment kernels) the prefill tile policy for qkv / o / gate-up / lm_head (one pass over K
//     per output tile, no split: at 256 chains qkv 12.0 against 24.7 us on the split-K streaming launcher, o 11.9 /
//     17.7, gate/up 43.6 / 56.9, lm_head 250 / 336; tools/bench_midm.py), the streaming launcher for down (32.4 / 44.3).
//     Every one of them sums an output's K range in an order fixed by (N, K): batch invariance within this path.
//   a8q / a8g: FP8 activations -- the fragment path with FP8 weight fragments takes the row as FP8 fragments + a scale (fp8 x
//     fp8 MFMA); any other path takes the same values as bf16
struct batch_regime {
    bool fr, tiled, a8q, a8g, fl;
};
// the FP8 fragment stream of a projection (quantised engine; ze_tune knob 10 = 1: the bf16 fragments)
static bool frag8(const ze_linear& l) { return l.wf8 && ze_knobs[ZE_KNOB_BF16_FRAGMENTS] != ZE_KNOB_ON; }
// the weight operand of a fragment launch: the MXFP4 copy where ensure_fragments built one (there is no bf16 copy then), else the
// FP8 copy of a quantised engine, else bf16 fragments
struct frag_w {
    const bf16_t* wf;
    const float* scale8;
    const uint8_t* scale4;
    bool w8;
};
static frag_w frag_of(const ze_linear& l, const bf16_t* wf16) {
    if (l.wf4) return frag_w{(const bf16_t*)l.wf4, nullptr, l.sf4, false};
    if (frag8(l)) return frag_w{(const bf16_t*)l.wf8, l.scale8, nullptr, true};
    return frag_w{wf16, nullptr, nullptr, false};
}
static batch_regime regime_of(const ze_engine* e, int li) {
    const ze_text_layer& L = e->tl[li];
    batch_regime r;
    r.fr = L.qkv.has_frag() && !e->wide_regime() && ze_knobs[ZE_KNOB_SKINNY] != ZE_SKINNY_OFF;
    r.tiled = e->wide_regime() && ze_knobs[ZE_KNOB_WIDE_DECODE] != ZE_WIDE_STREAM;
    r.a8q = e->fp8_act && r.fr && frag8(L.qkv);
    r.a8g = e->fp8_act && r.fr && frag8(L.gate_up);
    r.fl = (e->lm_head_f || e->lm_head8.wf4) && !e->wide_regime() && ze_knobs[ZE_KNOB_SKINNY] != ZE_SKINNY_OFF;
    return r;
}

// The launches of a batched decode step over the n rows of `rows`, one function per kind: the step is their sequence, and
// ze_profile_batch_kernel times these very functions.  A projection returns whether it streamed FP8 weights.
void batch_norm(ze_engine* e, const ze_step_rows& rows, int li, int n, int which, hipStream_t s) {
    const ze_config& c = e->cfg;
    const int H = c.hidden;
    const batch_regime r = regime_of(e, li);
    if (which == ZE_NORM_FINAL) {
        ze_launch_rmsnorm(e->bh, H, e->final_norm, e->by, H, n, H, c.rms_eps, s, r.fl ? 1 : 2);
        return;
    }
    const bool a8 = which == ZE_NORM_IN ? r.a8q : r.a8g;
    ze_launch_rmsnorm(e->bh, H, which == ZE_NORM_IN ? e->tl[li].in_norm : e->tl[li].post_norm, e->by, H, n, H, c.rms_eps, s, r.fr ? 1 : 2,
                      a8 ? 2 : (e->fp8_act ? 1 : 0), e->ty8, e->ty8_scale);
}

bool batch_qkv(ze_engine* e, const ze_step_rows& rows, int li, int n, hipStream_t s) {
    const ze_config& c = e->cfg;
    const int H = c.hidden, hd = e->head_dim, nqkv = (c.heads + 2 * c.kv_heads) * hd;
    const size_t seq_stride = (size_t)c.kv_heads * c.max_ctx * hd;
    const ze_text_layer& L = e->tl[li];
    const batch_regime r = regime_of(e, li);
    const ze_gemm_ws ws = e->gemm_ws();
    if (r.fr) {  // projection + M-RoPE + KV append in one launch (the fragment copy of qkv is packed for it)
        const frag_w w = frag_of(L.qkv, L.qkv.wf);
        ze_launch_qkv_rope_oneshot(r.a8q ? (const bf16_t*)e->ty8 : e->by, w.wf, L.qkv.bias,
                                   e->bqkv, nqkv, n, H, c.heads, c.kv_heads, e->cosT, e->sinT, e->st_dev, rows.seq,
                                   e->kc(li, 0), e->vc(li, 0), seq_stride, c.max_ctx, s, w.scale8,
                                   r.a8q ? e->ty8_scale : nullptr, rows.off, w.scale4);
        return w.w8;
    }
    // row streaming: projection + M-RoPE + KV append in ONE launch on the permuted rows (same bits as the pair of
    // launches below; knob 13 = 2 keeps the pair, for A/B runs and the bit-equality test); its chain ids are e->bseq's (ze_rows_spec)
    if (r.tiled && L.qkv.wp && ze_knobs[ZE_KNOB_WIDE_DECODE] != ZE_WIDE_QKV_PAIR) {
        ze_launch_gemm_qkv_rope(e->by, H, L.qkv.wp, H, L.qkv.bias_p, e->qkv_epi_dev + li, e->bqkv, nqkv, n, nqkv, H, s);
        return false;
    }
    if (r.tiled) ze_launch_gemm_wide(ZE_EPI_NONE, e->by, H, L.qkv.w, L.qkv.ld, L.qkv.bias, nullptr, 0, e->bqkv, nqkv, n, nqkv, H, ws, s);
    else ze_launch_gemm_stream(ZE_EPI_NONE, e->by, H, L.qkv.w, L.qkv.ld, L.qkv.bias, nullptr, 0, e->bqkv, nqkv, n, nqkv, H, ws, s);
    ze_launch_rope_kv_batch(e->bqkv, n, c.heads, c.kv_heads, hd, e->cosT, e->sinT, e->st_dev, rows.seq, e->kc(li, 0), e->vc(li, 0),
                            seq_stride, c.max_ctx, s);
    return false;
}

void batch_attention(ze_engine* e, const ze_step_rows& rows, int li, int n, hipStream_t s) {
    launch_batch_attention(e, rows, li, n, regime_of(e, li).fr, s);
}

bool batch_o(ze_engine* e, const ze_step_rows& rows, int li, int n, hipStream_t s) {
    const int H = e->cfg.hidden, nq = e->cfg.heads * e->head_dim;
    const ze_text_layer& L = e->tl[li];
    const batch_regime r = regime_of(e, li);
    if (r.fr && ze_knobs[ZE_KNOB_O_SKINNY] != ZE_KNOB_ON) {
        const frag_w w = frag_of(L.o, L.o.wf);
        ze_launch_gemm_oneshot(ZE_EPI_RESIDUAL, rows.out, w.wf, nullptr, e->bh, H, e->bh, H, n, H, nq, s, w.scale8, nullptr, w.scale4);
        return w.w8;
    }
    if (r.fr)  // (knob 9: bf16 fragments, or the MXFP4 ones where they are the only copy)
        ze_launch_gemm_frag(ZE_EPI_RESIDUAL, rows.out, L.o.wf4 ? (const bf16_t*)L.o.wf4 : L.o.wf, nullptr, e->bh, H, e->bh, H, n, H, nq, s, nullptr,
                            nullptr, L.o.wf4 ? L.o.sf4 : nullptr);
    else if (r.tiled) ze_launch_gemm_wide(ZE_EPI_RESIDUAL, rows.out, nq, L.o.w, L.o.ld, nullptr, e->bh, H, e->bh, H, n, H, nq, e->gemm_ws(), s);
    else ze_launch_gemm_stream(ZE_EPI_RESIDUAL, rows.out, nq, L.o.w, L.o.ld, nullptr, e->bh, H, e->bh, H, n, H, nq, e->gemm_ws(), s);
    return false;
}

bool batch_gate_up(ze_engine* e, const ze_step_rows& rows, int li, int n, hipStream_t s) {
    const int H = e->cfg.hidden, ip = e->text_ipad;
    const ze_text_layer& L = e->tl[li];
    const batch_regime r = regime_of(e, li);
    if (r.fr) {
        const frag_w w = frag_of(L.gate_up, L.gate_up.wf);
        ze_launch_gemm_frag(ZE_EPI_SWIGLU, r.a8g ? (const bf16_t*)e->ty8 : e->by, w.wf, nullptr, nullptr, 0, e->ba, ip, n, 2 * ip, H, s,
                            w.scale8, r.a8g ? e->ty8_scale : nullptr, w.scale4);
        return w.w8;
    }
    if (r.tiled) ze_launch_gemm_wide(ZE_EPI_SWIGLU, e->by, H, L.gate_up.w, L.gate_up.ld, nullptr, nullptr, 0, e->ba, ip, n, 2 * ip, H, e->gemm_ws(), s);
    else ze_launch_gemm_stream(ZE_EPI_SWIGLU, e->by, H, L.gate_up.w, L.gate_up.ld, nullptr, nullptr, 0, e->ba, ip, n, 2 * ip, H, e->gemm_ws(), s);
    return false;
}

// the down projection (K = 11008) stays on the split-K ring: the fragment kernel with K split over 8 x 32
// workgroups measured 22.6-25.3 us against 17.9 (slab reduction included in both)
bool batch_down(ze_engine* e, const ze_step_rows& rows, int li, int n, hipStream_t s) {
    const int H = e->cfg.hidden, ip = e->text_ipad;
    const ze_text_layer& L = e->tl[li];
    if (regime_of(e, li).tiled) ze_launch_gemm_wide(ZE_EPI_RESIDUAL, e->ba, ip, L.down.w, L.down.ld, nullptr, e->bh, H, e->bh, H, n, H, ip, e->gemm_ws(), s);
    else ze_launch_gemm_stream(ZE_EPI_RESIDUAL, e->ba, ip, L.down.w, L.down.ld, nullptr, e->bh, H, e->bh, H, n, H, ip, e->gemm_ws(), s);
    return false;
}

// (li: unused -- the regime's fl does not depend on the layer)
bool batch_lm_head(ze_engine* e, const ze_step_rows& rows, int li, int n, hipStream_t s) {
    const ze_config& c = e->cfg;
    const int H = c.hidden;
    const batch_regime r = regime_of(e, li);
    if (r.fl) {
        const frag_w w = frag_of(e->lm_head8, e->lm_head_f);
        ze_launch_gemm_frag(ZE_EPI_F32, e->by, w.wf, nullptr, nullptr, 0, (bf16_t*)rows.logits, c.vocab, n, c.vocab, H, s, w.scale8, nullptr,
                            w.scale4);
        return w.w8;
    }
    if (r.tiled)  // (one pass over K whatever the row count: batch invariance)
        ze_launch_gemm_wide(ZE_EPI_F32, e->by, H, e->lm_head, H, nullptr, nullptr, 0, (bf16_t*)rows.logits, c.vocab, n, c.vocab, H, e->gemm_ws(), s);
    else
        ze_launch_gemm_stream(ZE_EPI_F32, e->by, H, e->lm_head, H, nullptr, nullptr, 0, (bf16_t*)rows.logits, c.vocab, n, c.vocab, H, e->gemm_ws(), s);
    return false;
}

// The forward of a step over the n rows of `rows`, behind the embedding launch its caller issued into e->bh: the layers, the final
// norm, the lm_head into rows.logits.  The one layer loop of the batched decode.
static void enqueue_forward(ze_engine* e, const ze_step_rows& rows, int n, hipStream_t s) {
    for (int li = 0; li < e->cfg.layers; ++li) {
        batch_norm(e, rows, li, n, ZE_NORM_IN, s);
        batch_qkv(e, rows, li, n, s);
        batch_attention(e, rows, li, n, s);
        batch_o(e, rows, li, n, s);
        batch_norm(e, rows, li, n, ZE_NORM_POST, s);
        batch_gate_up(e, rows, li, n, s);
        batch_down(e, rows, li, n, s);
    }
    batch_norm(e, rows, 0, n, ZE_NORM_FINAL, s);
    batch_lm_head(e, rows, 0, n, s);
}

// The sampler of rows [0, n) of `rows`, one chain each, with what the chains' requests launch before and behind it.  sample = 0:
// teacher forcing -- the chain states move on, nothing is drawn and no request is served.
static void enqueue_sampler(ze_engine* e, const ze_step_rows& rows, int n, float penalty, int ignore_eos, int sample, const ze_sample_opts& so,
                            hipStream_t s) {
    const ze_config& c = e->cfg;
    ze_launch_sample_batch(sample ? ze_requests_rows(e, rows.logits, rows.seq, 0, n, s) : rows.logits, c.vocab, e->seen, penalty, e->st_dev,
                           rows.seq, n, e->eos_dev, c.n_eos, c.pad_token_id, ignore_eos, 1, sample, e->out_tokens, c.max_ctx, e->bsample,
                           e->bsample + (size_t)c.max_seqs * 2 * 128, so, s);
    if (sample) ze_requests_after_token(e, rows.logits, rows.seq, 0, n, s);
}

static int enqueue_decode_batch(ze_engine* e, int n, float penalty, int ignore_eos, int sample, const ze_sample_opts& so,
                                hipStream_t s) {
    const ze_step_rows rows = ze_rows_own(e);
    ze_launch_embed_tokens_batch(e->st_dev, rows.seq, n, e->embed, e->bh, e->cfg.hidden, s);
    enqueue_forward(e, rows, n, s);
    enqueue_sampler(e, rows, n, penalty, ignore_eos, sample, so, s);
    ZE_KCHECK();
    return ZE_OK;
}

extern "C" int ze_decode_batch(ze_engine* e, const int32_t* seqs, int n, const int32_t* tokens, float* out_logits,
                               void* stream) {
    if (!e || !seqs) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    const ze_config& c = e->cfg;
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    ZE_TRY(ensure_fragments(e, s));
    ZE_TRY(begin_batch(e, seqs, n, 1, s));
    if (tokens) {  // (all of them checked before the first is written: a refused call leaves every chain as it was)
        for (int i = 0; i < n; ++i)
            if (tokens[i] >= c.vocab) return ze_fail(e, ZE_ERR_INVALID, "token id out of range");
        for (int i = 0; i < n; ++i)
            if (tokens[i] >= 0) ze_launch_set_ints(&(e->st_dev + seqs[i])->token, &tokens[i], 1, s);
    }
    const int th = ze_timer_begin(e, 3, s);
    ZE_TRY(enqueue_decode_batch(e, n, 1.0f, 1, 0, ze_sample_opts{}, s));
    ze_timer_end(e, th, s);
    end_batch(e, seqs, n, 1);
    if (out_logits)
        ZE_HIP(hipMemcpyAsync(out_logits, e->blogits, (size_t)n * c.vocab * sizeof(float), hipMemcpyDeviceToDevice, s));
    return ZE_OK;
}

// The captured batched steps of the engine, one cache for every kind (ze_step_key::kind): *exec = the graph captured under `key`,
// which `enqueue` is captured into when there is none yet.  Chain ids and positions live in device memory, so one graph per key
// serves every composition.  A ze_tune change flushes the cache.
static int step_graph(ze_engine* e, const ze_step_key& key, const std::function<int(hipStream_t)>& enqueue, hipGraphExec_t* exec) {
    if (e->bgraph_epoch != ze_tune_epoch) {
        for (auto& kv : e->bgraphs) hipGraphExecDestroy(kv.second);
        e->bgraphs.clear();
        e->bgraph_epoch = ze_tune_epoch;
    }
    auto it = e->bgraphs.find(key);
    if (it == e->bgraphs.end()) {
        hipGraphExec_t ex = nullptr;
        ZE_TRY(capture_step(e, enqueue, &ex));
        it = e->bgraphs.emplace(key, ex).first;
    }
    *exec = it->second;
    return ZE_OK;
}

// `steps` times the step `enqueue` puts on a stream: replays of `gx`, or eagerly on s when there is no graph
static int run_steps(ze_engine* e, hipGraphExec_t gx, const std::function<int(hipStream_t)>& enqueue, int steps, hipStream_t s) {
    for (int i = 0; i < steps; ++i) {
        if (gx)
            ZE_HIP(hipGraphLaunch(gx, s));
        else
            ZE_TRY(enqueue(s));
    }
    return ZE_OK;
}

// The forward of a beam step (ze_beam.hip): the batched step without its sampler -- teacher forcing on the tokens the chain states
// hold, as ze_decode_batch runs it; captured, it is the same linear chain of launches under a key of its own kind
int ze_beam_forward(ze_engine* e, const int32_t* seqs, int n, int use_graph, hipStream_t s) {
    ZE_TRY(begin_batch(e, seqs, n, 1, s));
    const ze_sample_opts so{};
    const auto step = [&](hipStream_t cs) { return enqueue_decode_batch(e, n, 1.0f, 1, 0, so, cs); };
    hipGraphExec_t gx = nullptr;
    if (use_graph) ZE_TRY(step_graph(e, ze_step_key_of(e, n, 0, 1.0f, 1, so, ZE_STEP_UNSAMPLED), step, &gx));
    ZE_TRY(run_steps(e, gx, step, 1, s));
    end_batch(e, seqs, n, 1);
    return ZE_OK;
}

// `steps` sampled decode steps for the chains in `active` (all with room for them)
static int run_burst(ze_engine* e, const std::vector<int>& active, int steps, const ze_gen_params* p, float pen, int ign,
                     const ze_sample_opts& bso, hipStream_t s) {
    const int na = (int)active.size();
    ZE_TRY(begin_batch(e, active.data(), na, steps, s));
    const auto step = [&](hipStream_t cs) { return enqueue_decode_batch(e, na, pen, ign, 1, bso, cs); };
    hipGraphExec_t gx = nullptr;
    if (p->use_graph) ZE_TRY(step_graph(e, ze_step_key_of(e, na, 0, pen, ign, bso), step, &gx));
    ZE_TRY(run_steps(e, gx, step, steps, s));
    end_batch(e, active.data(), na, steps);
    return ZE_OK;
}

// ================================================================== speculative bursts (ze_spec.hip: drafter, accept pass, setter)
// A step of a burst in which some chain speculates: draft -> row table -> the fragment family's launches over the rows -> the usual
// sampler for the chains without speculation (the first n_plain rows, one each) -> the accept pass for the others.  Row j of a chain
// is fed at position ctx + j and every kernel of the family computes a row independently of what shares the step, so its logits are
// the bits a plain step of the chain alone at that position produces.  The launches are the step's own functions
// (enqueue_forward) on the row set of the speculative table (ze_rows_spec).
struct spec_layout {
    int rows = 0, n_plain = 0, n_chains = 0;
    // the chains that speculate in sampled mode come last: n_drawn of them, the last n_drawn_rows rows
    int n_drawn = 0, n_drawn_rows = 0;
};

// the multi-row forms exist for the fragment kernels and the pipelined attention alone
static bool spec_step_ok(const ze_engine* e) {
    const batch_regime r = regime_of(e, 0);
    const int k8 = ze_knobs[ZE_KNOB_BATCH_ATTN], k23 = ze_knobs[ZE_KNOB_ATTN_SPLIT];
    // the plain step must be on the very kernel the ROWS form instantiates: per-wave, 384-key parts (knob 8 not 1 / 4), no split rows
    return r.fr && r.fl && attn_per_wave(e) && k8 != ZE_ATTN_SLICE && k8 != ZE_ATTN_PART192 && k23 != ZE_SPLIT_ROWS && k23 != ZE_SPLIT_PAIRED;
}

static int enqueue_spec_step(ze_engine* e, const spec_layout& L, float penalty, int ign, const ze_sample_opts& so, hipStream_t s) {
    const ze_config& c = e->cfg;
    const ze_spec& q = e->spec;
    const ze_step_rows rows = ze_rows_spec(e);
    ze_spec_step a;
    a.st = e->st_dev, a.table = q.table, a.chains = q.chains, a.hist_ctx = e->req.tr_ctx, a.eos_ids = e->eos_dev;
    a.out_tokens = e->out_tokens, a.seen = e->seen, a.logits = q.logits, a.row_off = q.row_off, a.row_tok = q.row_tok, a.dlen = q.dlen;
    a.n_chains = L.n_chains, a.max_ctx = c.max_ctx, a.vocab = c.vocab, a.n_eos = c.n_eos, a.ignore_eos = ign;
    ze_launch_spec_draft(a, s);
    ze_launch_spec_embed(q.row_tok, L.rows, e->embed, e->bh, c.hidden, s);
    enqueue_forward(e, rows, L.rows, s);
    if (L.n_plain > 0) enqueue_sampler(e, rows, L.n_plain, penalty, ign, 1, so, s);  // rows 0 .. n_plain - 1: one chain each, and their usual sampler
    ze_spec_step g = a;  // the greedy-mode chains: [n_plain, n_chains - n_drawn)
    g.n_chains = L.n_chains - L.n_drawn;
    ze_launch_spec_accept(g, L.n_plain, s);
    // the sampled-mode chains behind them: their rows drawn by the plain step's sampler kernels, then the walk (a burst without such a
    // chain launches nothing here)
    if (L.n_drawn > 0)
        ze_launch_spec_accept_sampled(a, q.draw, L.n_chains - L.n_drawn, L.rows - L.n_drawn_rows, L.n_drawn_rows, so.temperature, so.seed, so.draws(), so.samp,
                                      so.filt, s);
    ZE_KCHECK();
    return ZE_OK;
}

// `steps` speculative steps for the chains of a burst; returns the steps enqueued or a negative ze_status
static int spec_burst(ze_engine* e, const std::vector<int>& chains, int steps, const ze_gen_params* p, float pen, int ign, hipStream_t s) {
    const ze_config& c = e->cfg;
    ze_spec& q = e->spec;
    if (e->wide_regime() || !spec_step_ok(e))
        return ze_fail(e, ZE_ERR_INVALID, "a speculative burst needs the fragment kernels and the pipelined decode attention (family 0, default ze_tune knobs)");
    for (size_t i = 0; i < chains.size(); ++i) {
        for (size_t j = 0; j < i; ++j)
            if (chains[i] == chains[j]) return ze_fail(e, ZE_ERR_INVALID, "duplicate sequence id in a batch");
        // how far a speculating chain came in a burst is the device's to know until ze_decode_burst_end has read it back
        if (q.on(chains[i]) && q.pending[chains[i]])
            return ze_fail(e, ZE_ERR_INVALID, "a speculating chain of this burst has a burst in flight: ze_decode_burst_end first");
        if (!q.on(chains[i]) && e->ctx_host[chains[i]] > c.max_ctx) return ze_fail(e, ZE_ERR_NOMEM, "sequence exceeds max_ctx");
    }
    const bool call_draws = p->do_sample && p->temperature > 0.f;
    // the row table: the chains without speculation first (one row each: the sampler's rows), then k + 1 rows per speculating chain --
    // the greedy-mode ones, then the sampled-mode ones, so that each accept launch covers one contiguous range
    std::vector<int> order;
    for (int pass = 0; pass < 3; ++pass)
        for (int ch : chains)
            if ((int)q.on(ch) + (int)q.sampled(ch) == pass) order.push_back(ch);
    spec_layout L;
    std::vector<int> row_seq, tab;
    int mx = 0;
    for (int ch : order) {
        const int k = q.on(ch) ? q.host[ch].k : 0;
        const ze_chain_sampling& own = e->req.samp_host[ch];
        if (k > 0 && !q.sampled(ch) && (own.penalty > 0.f ? own.temperature > 0.f : call_draws))
            return ze_fail(e, ZE_ERR_INVALID, "speculation is greedy only: the burst samples a speculating chain");
        if (k == 0) steps = std::min(steps, c.max_ctx - e->ctx_host[ch]);  // (a speculating chain out of room rides along with dead rows)
        const float cp = own.penalty > 0.f ? own.penalty : pen;
        int bits;
        memcpy(&bits, &cp, sizeof(bits));
        tab.insert(tab.end(), {ch, L.rows, k + 1, bits});
        if (q.sampled(ch)) {
            L.n_drawn += 1;
            L.n_drawn_rows += k + 1;
        }
        for (int j = 0; j <= k; ++j) row_seq.push_back(ch);
        L.rows += k + 1;
        L.n_chains += 1;
        if (k == 0) L.n_plain += 1;
    }
    if (L.rows > ZE_SP_MAX_ROWS) return ze_fail(e, ZE_ERR_INVALID, "more than 64 rows in a speculative step (one per plain chain, k + 1 per speculating chain)");
    if (steps <= 0) return 0;
    for (int ch : chains) mx = std::max(mx, std::min(c.max_ctx, e->ctx_host[ch] + steps * ((q.on(ch) ? q.host[ch].k : 0) + 1) + 1));
    ze_launch_set_ints(q.row_seq, row_seq.data(), L.rows, s);
    ze_launch_set_ints(q.chains, tab.data(), (int)tab.size(), s);
    sync_prefix(e, chains.data(), (int)chains.size(), s);
    set_live_parts_reach(e, mx);   // the longest context any row can reach in this burst
    const ze_sample_opts bso = ze_sample_opts_of(e, p, 0, true);
    const auto step = [&](hipStream_t cs) { return enqueue_spec_step(e, L, pen, ign, bso, cs); };
    hipGraphExec_t gx = nullptr;
    // the key of a plain step over `rows` rows, and the layout: nothing else decides what the step launches
    if (p->use_graph) ZE_TRY(step_graph(e, ze_step_key_of(e, L.rows, 0, pen, ign, bso, ZE_STEP_SPEC, L.n_plain, L.n_chains, L.n_drawn, L.n_drawn_rows), step, &gx));
    ZE_TRY(run_steps(e, gx, step, steps, s));
    // a speculating chain's length is the device's to know until ze_decode_burst_end reads it back
    for (int ch : chains) {
        if (!q.on(ch)) e->ctx_host[ch] += steps;
        else q.pending[ch] = 1;
        e->logits_fresh[ch] = 0;
    }
    return steps;
}

// The row contract alone: chain `seq` is fed tokens[0 .. r) at r consecutive positions in ONE family-0 step (teacher forcing, as
// ze_decode_batch: no sampling, the cache grows by r rows); out_logits f32 [r, vocab] device
extern "C" int ze_op_decode_rows(ze_engine* e, int seq, const int32_t* tokens, int r, float* out_logits, void* stream) {
    ZE_TRY(check_seq(e, seq));
    const ze_config& c = e->cfg;
    if (!tokens || r < 1) return ze_fail(e, ZE_ERR_INVALID, "null tokens or r < 1");
    if (r > ZE_SP_MAX_ROWS) return ze_fail(e, ZE_ERR_INVALID, "more than 64 rows in a step");
    for (int j = 0; j < r; ++j)
        if (tokens[j] < 0 || tokens[j] >= c.vocab) return ze_fail(e, ZE_ERR_INVALID, "token id out of range");
    if (e->ctx_host[seq] + r > c.max_ctx) return ze_fail(e, ZE_ERR_NOMEM, "sequence exceeds max_ctx");
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    ZE_TRY(ensure_fragments(e, s));
    if (e->wide_regime() || !spec_step_ok(e))
        return ze_fail(e, ZE_ERR_INVALID, "rows of one chain need the fragment kernels and the pipelined decode attention (family 0, default ze_tune knobs)");
    ZE_TRY(ze_spec_alloc(e));
    ze_spec& q = e->spec;
    std::vector<int> row_seq(r, seq), row_off(r);
    for (int j = 0; j < r; ++j) row_off[j] = j;
    ze_launch_set_ints(q.row_seq, row_seq.data(), r, s);
    ze_launch_set_ints(q.row_off, row_off.data(), r, s);
    ze_launch_set_ints(q.row_tok, tokens, r, s);
    sync_prefix(e, &seq, 1, s);
    set_live_parts_reach(e, e->ctx_host[seq] + r);
    ze_launch_spec_embed(q.row_tok, r, e->embed, e->bh, c.hidden, s);
    enqueue_forward(e, ze_rows_spec(e), r, s);
    e->ctx_host[seq] += r;
    e->logits_fresh[seq] = 0;
    e->tok_host[seq] = tokens[r - 1];
    ze_launch_set_ints(&(e->st_dev + seq)->ctx, &e->ctx_host[seq], 1, s);
    ze_launch_set_ints(&(e->st_dev + seq)->token, &tokens[r - 1], 1, s);
    ZE_KCHECK();
    if (out_logits) ZE_HIP(hipMemcpyAsync(out_logits, q.logits, (size_t)r * c.vocab * sizeof(float), hipMemcpyDeviceToDevice, s));
    return ZE_OK;
}

// first_token for a chain of a batch; `sample_stream` = the chain's random stream
static int begin_chain(ze_engine* e, int q, const ze_gen_params* p, int ign, int sample_stream, hipStream_t s) {
    const ze_sample_opts so = ze_sample_opts_of(e, p, q);
    if (so.temperature > 0.f) ze_launch_set_ints(&(e->st_dev + q)->stream, &sample_stream, 1, s);
    return first_token(e, q, ze_penalty_of(e, p, q), ign, so, s);
}

extern "C" int ze_generate_batch(ze_engine* e, const int32_t* seqs, int n, const ze_gen_params* p, int32_t* out_tokens,
                                 int32_t* n_out, void* stream) {
    if (!e || !seqs || !p || !out_tokens || !n_out) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    const ze_config& c = e->cfg;
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    const int max_new = p->max_new_tokens;
    if (max_new <= 0 || n <= 0) return ze_fail(e, ZE_ERR_INVALID, "max_new_tokens and n must be positive");
    ZE_TRY(ensure_fragments(e, s));
    // Per-chain budget, as ze_generate clamps it: the last generated token is never fed back, so a chain with `ctx`
    // cached tokens may produce max_ctx - ctx + 1 tokens.  A chain that reaches its budget leaves the batch like one
    // that hit EOS: what a request gets never depends on the other requests of its batch.
    std::vector<int> limit(c.max_seqs, 0);
    for (int i = 0; i < n; ++i) {
        if (seqs[i] < 0 || seqs[i] >= c.max_seqs) return ze_fail(e, ZE_ERR_NOTFOUND, "sequence id out of range");
        for (int j = 0; j < i; ++j)
            if (seqs[j] == seqs[i]) return ze_fail(e, ZE_ERR_INVALID, "duplicate sequence id in a batch");
        if (e->ctx_host[seqs[i]] > c.max_ctx) return ze_fail(e, ZE_ERR_NOMEM, "sequence exceeds max_ctx");
        limit[seqs[i]] = std::min(max_new, c.max_ctx - e->ctx_host[seqs[i]] + 1);
    }
    const float pen = p->repetition_penalty > 0.f ? p->repetition_penalty : 1.0f;
    const int ign = p->ignore_eos ? 1 : 0;
    const ze_sample_opts bso = ze_sample_opts_of(e, p, 0, true);
    // sampling stream of a chain = its row in this call (reproducible per request)
    for (int i = 0; i < n; ++i) ZE_TRY(begin_chain(e, seqs[i], p, ign, i, s));
    std::vector<int> active;
    std::vector<int> produced(c.max_seqs, 0);
    for (int i = 0; i < n; ++i) {
        produced[seqs[i]] = 1;
        if (limit[seqs[i]] > 1) active.push_back(seqs[i]);
    }
    const int sync_every = std::max(1, p->sync_every);
    const int td = ze_timer_begin(e, 3, s);
    int steps = 1;
    while (steps < max_new && !active.empty()) {
        int burst = std::min(sync_every, max_new - steps);
        for (int q : active) burst = std::min(burst, limit[q] - produced[q]);  // >= 1: exhausted chains were dropped
        ZE_TRY(run_burst(e, active, burst, p, pen, ign, bso, s));
        steps += burst;
        for (int q : active) produced[q] += burst;
        if (steps < max_new) {  // chains that emitted an EOS or used up their budget leave (continuous batching: others go on)
            if (!ign) {
                ZE_HIP(hipMemcpyAsync(e->bstate_host, e->st_dev, sizeof(ze_seq_dev) * c.max_seqs, hipMemcpyDeviceToHost, s));
                ZE_HIP(hipStreamSynchronize(s));
            }
            std::vector<int> still;
            for (int q : active)
                if ((ign || !e->bstate_host[q].finished) && produced[q] < limit[q]) still.push_back(q);
            active.swap(still);
        }
    }
    ze_timer_end(e, td, s);
    ZE_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i) {
        const int q = seqs[i];
        int32_t* dst = out_tokens + (size_t)i * max_new;
        // (on the caller's stream: a legacy-stream copy would synchronise with every other engine's stream of the process)
        ZE_HIP(hipMemcpyAsync(dst, e->out_tokens + (size_t)q * c.max_ctx, (size_t)produced[q] * sizeof(int), hipMemcpyDeviceToHost, s));
        ZE_HIP(hipStreamSynchronize(s));
        n_out[i] = ign ? produced[q] : trim_at_eos(c, dst, produced[q]);
    }
    return ZE_OK;
}

// ================================================================== continuous batching (chains join and leave between bursts)
extern "C" int ze_chain_begin(ze_engine* e, int seq, const ze_gen_params* p, int sample_stream, void* stream) {
    ZE_TRY(check_seq(e, seq));
    if (!p) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    ZE_TRY(ensure_fragments(e, s));
    const int t_s = ze_timer_begin(e, 4, s);
    const int r = begin_chain(e, seq, p, p->ignore_eos ? 1 : 0, sample_stream, s);
    ze_timer_end(e, t_s, s);
    return r;
}

// A burst in two halves, so that the host can enqueue other work (the prefill / ViT round of the next newcomers, on ANOTHER
// stream) while the burst runs: _begin enqueues `steps` captured decode steps for the live chains and returns at once (the
// number of steps actually enqueued: every chain must have room for all of them); _end waits for the burst and reports
// each chain's token count and EOS flag.  ze_decode_burst = _begin + _end.
extern "C" int ze_decode_burst_begin(ze_engine* e, const int32_t* seqs, int n, int steps, const ze_gen_params* p, void* stream) {
    if (!e || !seqs || !p || n <= 0 || steps < 0) return ze_fail(e, ZE_ERR_INVALID, "bad burst arguments");
    const ze_config& c = e->cfg;
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    ZE_TRY(ensure_fragments(e, s));
    std::vector<int> active(seqs, seqs + n);
    bool speculative = false;
    for (int q : active) {
        if (q < 0 || q >= c.max_seqs) return ze_fail(e, ZE_ERR_NOTFOUND, "sequence id out of range");
        speculative = speculative || e->spec.on(q);
    }
    const float pen = p->repetition_penalty > 0.f ? p->repetition_penalty : 1.0f;
    const int ign = p->ignore_eos ? 1 : 0;
    if (speculative) {  // some chain of the burst speculates (ze_seq_set_speculation): every step is draft -> rows -> step -> accept
        const int td = ze_timer_begin(e, 3, s);
        const int ran = spec_burst(e, active, steps, p, pen, ign, s);
        ze_timer_end(e, td, s);
        return ran;
    }
    for (int q : active) steps = std::min(steps, c.max_ctx - e->ctx_host[q]);  // every chain of the burst must have room for all its steps
    if (steps < 0) return ze_fail(e, ZE_ERR_NOMEM, "sequence exceeds max_ctx");
    const int td = ze_timer_begin(e, 3, s);
    if (steps > 0) ZE_TRY(run_burst(e, active, steps, p, pen, ign, ze_sample_opts_of(e, p, 0, true), s));
    ze_timer_end(e, td, s);
    return steps;
}

extern "C" int ze_decode_burst_end(ze_engine* e, const int32_t* seqs, int n, int32_t* n_generated, int32_t* finished, void* stream) {
    if (!e || !seqs || n <= 0) return ze_fail(e, ZE_ERR_INVALID, "bad burst arguments");
    const ze_config& c = e->cfg;
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    ZE_HIP(hipMemcpyAsync(e->bstate_host, e->st_dev, sizeof(ze_seq_dev) * c.max_seqs, hipMemcpyDeviceToHost, s));
    ZE_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i) {
        if (seqs[i] < 0 || seqs[i] >= c.max_seqs) return ze_fail(e, ZE_ERR_NOTFOUND, "sequence id out of range");
        if (n_generated) n_generated[i] = e->bstate_host[seqs[i]].n_gen;
        if (finished) finished[i] = e->bstate_host[seqs[i]].finished;
        // how far a speculating chain came is decided on the device (the accept pass)
        if (e->spec.on(seqs[i])) e->ctx_host[seqs[i]] = std::min(e->bstate_host[seqs[i]].ctx, c.max_ctx), e->spec.pending[seqs[i]] = 0;
    }
    return ZE_OK;
}

extern "C" int ze_decode_burst(ze_engine* e, const int32_t* seqs, int n, int steps, const ze_gen_params* p,
                               int32_t* n_generated, int32_t* finished, void* stream) {
    const int ran = ze_decode_burst_begin(e, seqs, n, steps, p, stream);
    if (ran < 0) return ran;
    ZE_TRY(ze_decode_burst_end(e, seqs, n, n_generated, finished, stream));
    return ran;
}

extern "C" int ze_chain_tokens(ze_engine* e, int seq, int32_t* out, int cap, int* n_out, void* stream) {
    ZE_TRY(check_seq(e, seq));
    if (!out || !n_out || cap < 0) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    const ze_config& c = e->cfg;
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    ze_seq_dev st;
    ZE_HIP(hipMemcpyAsync(&st, e->st_dev + seq, sizeof(st), hipMemcpyDeviceToHost, s));
    ZE_HIP(hipStreamSynchronize(s));
    int n = std::min(std::min(st.n_gen, cap), c.max_ctx);
    if (n > 0) {  // (on the caller's stream: a legacy-stream copy would synchronise with every other engine's stream of the process)
        ZE_HIP(hipMemcpyAsync(out, e->out_tokens + (size_t)seq * c.max_ctx, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
        ZE_HIP(hipStreamSynchronize(s));
    }
    *n_out = st.finished ? trim_at_eos(c, out, n) : n;
    return ZE_OK;
}

// ze_chain_tokens for the n chains a burst retires: one gather launch, one device -> host copy, one wait (the single-chain call
// costs two small copies and two waits per chain -- 1.5 ms each beside the 75-MB tile uploads of the stream).
// out_tokens: host int32 [n, capacity]; n_out [n].
extern "C" int ze_chain_tokens_batch(ze_engine* e, const int32_t* seqs, int n, int32_t* out, int cap, int32_t* n_out, void* stream) {
    if (!e || n < 0 || cap < 0 || (n > 0 && (!seqs || !out || !n_out))) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (n == 0) return ZE_OK;
    if (n > e->cfg.max_seqs) return ze_fail(e, ZE_ERR_INVALID, "more chains than slots");
    const ze_config& c = e->cfg;
    for (int i = 0; i < n; ++i) ZE_TRY(check_seq(e, seqs[i]));
    cap = std::min(cap, c.max_ctx);
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t words = 2 * (size_t)n + (size_t)n * cap;
    ZE_TRY(xfer_reserve(e, e->xt_host, e->xt_dev, e->xt_cap, words + (size_t)n, nullptr, s));
    // (the call waits for the stream before it returns, so the scratch is free again by the next call)
    int* slots_dev = e->xt_dev + words;
    memcpy(e->xt_host + words, seqs, (size_t)n * sizeof(int));
    ZE_HIP(hipMemcpyAsync(slots_dev, e->xt_host + words, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    ze_launch_gather_chain_tokens(e->st_dev, e->out_tokens, c.max_ctx, slots_dev, n, cap, e->xt_dev, s);
    ZE_KCHECK();
    ZE_HIP(hipMemcpyAsync(e->xt_host, e->xt_dev, words * sizeof(int), hipMemcpyDeviceToHost, s));
    ZE_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i) {
        const int* row = e->xt_host + 2 * (size_t)n + (size_t)i * cap;
        const bool finished = e->xt_host[2 * i + 1] != 0;
        const int m = finished ? trim_at_eos(c, row, e->xt_host[2 * i]) : e->xt_host[2 * i];  // (as ze_chain_tokens)
        memcpy(out + (size_t)i * cap, row, (size_t)m * sizeof(int));
        n_out[i] = m;
    }
    return ZE_OK;
}

// The log-probability entries of the tokens ze_chain_tokens_batch returns, the same way: one gather launch (tokens, for the
// EOS trim, and entries), one device -> host copy, one wait.
extern "C" int ze_chain_logprobs_batch(ze_engine* e, const int32_t* seqs, int n, float* out_logprobs, int32_t* out_top_ids,
                                       float* out_top_logprobs, int cap, int top_n_stride, int32_t* n_out, void* stream) {
    if (!e || n < 0 || cap < 0 || (n > 0 && (!seqs || !out_logprobs || !n_out))) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (n == 0) return ZE_OK;
    if (n > e->cfg.max_seqs) return ze_fail(e, ZE_ERR_INVALID, "more chains than slots");
    if (top_n_stride < 0 || top_n_stride > ZE_MAX_TOP_LOGPROBS) return ze_fail(e, ZE_ERR_INVALID, "top_n_stride must be in [0, 20]");
    const ze_config& c = e->cfg;
    for (int i = 0; i < n; ++i) {
        ZE_TRY(check_seq(e, seqs[i]));
        if (e->req.lp_host[seqs[i]] < 0) return ze_fail(e, ZE_ERR_INVALID, "the chain has no log-probability request (ze_seq_set_logprobs)");
    }
    cap = std::min(cap, c.max_ctx);
    const int stride = (out_top_ids && out_top_logprobs) ? top_n_stride : 0;
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t rows = (size_t)n * cap, words = 3 * (size_t)n + 2 * rows + 2 * rows * stride;
    ZE_TRY(xfer_reserve(e, e->xl_host, e->xl_dev, e->xl_cap, words + (size_t)n, nullptr, s));
    // (the call waits for the stream before it returns, so the scratch is free again by the next call)
    int* slots_dev = e->xl_dev + words;
    memcpy(e->xl_host + words, seqs, (size_t)n * sizeof(int));
    ZE_HIP(hipMemcpyAsync(slots_dev, e->xl_host + words, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    ze_launch_gather_chain_logprobs(e->st_dev, e->out_tokens, e->req.lp_bufs(), c.max_ctx, slots_dev, n, cap, stride, e->xl_dev, s);
    ZE_KCHECK();
    ZE_HIP(hipMemcpyAsync(e->xl_host, e->xl_dev, words * sizeof(int), hipMemcpyDeviceToHost, s));
    ZE_HIP(hipStreamSynchronize(s));
    const int* h_tok = e->xl_host + 3 * (size_t)n;
    const float* h_lp = reinterpret_cast<const float*>(e->xl_host + 3 * (size_t)n + rows);
    const int* h_ids = e->xl_host + 3 * (size_t)n + 2 * rows;
    const float* h_tlp = reinterpret_cast<const float*>(e->xl_host + 3 * (size_t)n + 2 * rows + rows * stride);
    for (int i = 0; i < n; ++i) {
        const bool finished = e->xl_host[3 * i + 1] != 0;
        const int m = finished ? trim_at_eos(c, h_tok + (size_t)i * cap, e->xl_host[3 * i]) : e->xl_host[3 * i];  // (as ze_chain_tokens)
        memcpy(out_logprobs + (size_t)i * cap, h_lp + (size_t)i * cap, (size_t)m * sizeof(float));
        if (stride) {
            memcpy(out_top_ids + (size_t)i * cap * stride, h_ids + (size_t)i * cap * stride, (size_t)m * stride * sizeof(int));
            memcpy(out_top_logprobs + (size_t)i * cap * stride, h_tlp + (size_t)i * cap * stride, (size_t)m * stride * sizeof(float));
        }
        n_out[i] = m;
    }
    return ZE_OK;
}

extern "C" int ze_chain_logprobs(ze_engine* e, int seq, float* out_logprobs, int32_t* out_top_ids, float* out_top_logprobs,
                                 int cap, int* n_out, int* top_n, void* stream) {
    ZE_TRY(check_seq(e, seq));
    if (!out_logprobs || !n_out || cap < 0) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    const int tn = e->req.lp_host[seq];
    if (tn < 0) return ze_fail(e, ZE_ERR_INVALID, "the chain has no log-probability request (ze_seq_set_logprobs)");
    if (top_n) *top_n = tn;
    const int32_t sq = seq;
    int32_t m = 0;
    ZE_TRY(ze_chain_logprobs_batch(e, &sq, 1, out_logprobs, tn > 0 ? out_top_ids : nullptr, tn > 0 ? out_top_logprobs : nullptr, cap,
                                   tn, &m, stream));
    *n_out = m;
    return ZE_OK;
}

// Forward passes of the text model: LLM prefill and scoring (one chain or a batch), the single-chain decode step (eager or hipGraph)
// and greedy / sampled generation on it.  The batched decode step: ze_decode_batch.hip; the ViT: ze_vision.hip; chain state: ze_seq.hip.
#include <math.h>
#include <string.h>

#include "ze_engine.h"

// A pinned staging buffer is rewritten by the next call: wait until the copies that read it have run -- an event right behind
// them, not the whole stream (which holds the ViT / prefill kernels enqueued since: the scheduler's thread used to sit 20-40 ms
// in every vit_forward / prefill_batch call, and with bursts shorter than that -- 64 chain slots -- the decode stream idled)
int stage_acquire(ze_engine* e, hipEvent_t& ev) {
    if (ev) ZE_HIP(hipEventSynchronize(ev));
    return ZE_OK;
}
int stage_release(ze_engine* e, hipEvent_t& ev, hipStream_t s) {
    if (!ev) ZE_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    ZE_HIP(hipEventRecord(ev, s));
    return ZE_OK;
}

// ================================================================== prefill
// The chain's SPLIT ROW (round 6; ze_seq_dev::split, ze_attn_batch.hip): the row behind its FIRST image block's <|vision_end|> --
// what the questions about one tile share (system turn + the view's image tokens) ends there.  Found where the tokens are
// prefilled, whatever pass brings them; a chain that copies the block (ze_seq_copy_prefix) inherits it.  A property of the
// chain's tokens alone: the decode attention may cut its parts there without a chain's sums depending on the batch.
static void note_split(ze_engine* e, int seq, const int32_t* ids, int len, int past) {
    if (e->split_host[seq] != 0 || e->cfg.vision_end_token_id < 0) return;
    for (int t = 0; t < len; ++t)
        if (ids[t] == e->cfg.vision_end_token_id) {
            if (past + t + 1 < 65536) e->split_host[seq] = past + t + 1;
            return;
        }
}

// RMSNorm (norm_w non-null) + the projection behind it, on `rows` prefill rows of e->th.  With FP8 activations on a quantised
// engine the row goes out as E4M3 bytes + one scale and the product runs on the block-scaled FP8 MFMA against the FP8 weight rows
// (k_gemm_ring_mx: the values of the fake-quantised bf16 path, another summation order; ze_tune knob 12 = 1 keeps that path).
// norm_w null (the profilers): the same GEMM on the rows the last pass left in e->ty / e->ty8p.
static void prefill_norm_gemm(ze_engine* e, const bf16_t* norm_w, const ze_linear& lin, const bf16_t* bias, int epi, bf16_t* out,
                              int ldo, int rows, int N, hipStream_t s) {
    const ze_config& c = e->cfg;
    const int H = c.hidden;
    if (e->fp8_act && lin.w8 && ze_knobs[ZE_KNOB_PREFILL_BF16_GEMM] != ZE_KNOB_ON && H % 128 == 0 && H >= 256 && lin.ld8 % 16 == 0) {
        if (norm_w) ze_launch_rmsnorm(e->th, H, norm_w, e->ty, H, rows, H, c.rms_eps, s, 0, 3, e->ty8p, e->ty8p_scale);
        if (ze_launch_gemm_mx(epi, e->ty8p, H, e->ty8p_scale, lin.w8, lin.ld8, lin.scale8, bias, out, ldo, rows, N, H, s)) return;
    }
    if (norm_w) ze_launch_rmsnorm(e->th, H, norm_w, e->ty, H, rows, H, c.rms_eps, s, 0, e->fp8_act ? 1 : 0);
    ze_launch_gemm(epi, e->ty, H, lin.w, lin.ld, bias, nullptr, 0, out, ldo, nullptr, rows, N, H, s, e->prefill_ws());
}

// Projection `which` (ZE_PROJ_*) of layer L on `rows` prefill rows, into out (leading dimension ldo): the ONE place a prefill
// projection is launched.  The pass gives norm = true and, for o and down, the residual stream itself (e->th, in place); a profiler
// gives norm = false and scratch rows, so that the residual stream is read, never written.
void prefill_projection(ze_engine* e, const ze_text_layer& L, int which, int rows, bool norm, bf16_t* out, int ldo, hipStream_t s) {
    const int H = e->cfg.hidden, nq = e->cfg.heads * e->head_dim, nqkv = nq + 2 * e->cfg.kv_heads * e->head_dim, ip = e->text_ipad;
    switch (which) {
        case ZE_PROJ_QKV:
            prefill_norm_gemm(e, norm ? L.in_norm : nullptr, L.qkv, L.qkv.bias, ZE_EPI_NONE, out, ldo, rows, nqkv, s);
            break;
        case ZE_PROJ_O:
            ze_launch_gemm(ZE_EPI_RESIDUAL, e->to, nq, L.o.w, L.o.ld, nullptr, e->th, H, out, ldo, nullptr, rows, H, nq, s, e->prefill_ws());
            break;
        case ZE_PROJ_GATE_UP:
            prefill_norm_gemm(e, norm ? L.post_norm : nullptr, L.gate_up, nullptr, ZE_EPI_SWIGLU, out, ldo, rows, 2 * ip, s);
            break;
        default:
            ze_launch_gemm(ZE_EPI_RESIDUAL, e->ta, ip, L.down.w, L.down.ld, nullptr, e->th, H, out, ldo, nullptr, rows, H, ip, s, e->prefill_ws());
            break;
    }
}

// query rows per attention tile: 128 -- two query tiles per wave, half the LDS fragment reads per MFMA -- on the LDS-DMA
// staging form of the kernel (no staging registers: 248 VGPRs, two workgroups per CU; with register staging the same tile
// needs 280 and lost: 120.5 against 116.9 ms per pass pair).  16-chain pass pair: register-staged 64-row tiles 107.0 ms,
// DMA 64-row 105.3, DMA 128-row 104.3.  ze_tune knob 1 = 9: 64-row tiles, 7: the register-staged form.  Same bits either way.
static int prefill_bq() { return (ze_knobs[ZE_KNOB_GATE_UP_FLASH] == ZE_FLASH_BQ64 || ze_knobs[ZE_KNOB_GATE_UP_FLASH] == ZE_FLASH_REG_STAGED) ? 64 : ZE_FA_BQ_LONG; }

// How a prefill pass addresses the KV cache: one chain appends behind its own `past` rows (no aux tables), a batch of chains
// goes through (chain slot, cache position) per row and (chain slot, position offset) per attention tile.
struct prefill_kv {
    int slot;             // K/V base of layer li: e->kc(li, slot) / e->vc(li, slot)
    int past;
    const int* row_aux;   // null: the single-chain form of the M-RoPE / KV-append kernel
    const int* tile_aux;  // null: the single-chain form of the flash kernel
    size_t seq_stride;
    int n_tiles;
    int rope_rows;        // rows of the pass's position table (ze_fa_rope::T)
};

// The decoder layers of a prefill pass over `rows` rows of e->th (tokens embedded, e->tpos / e->ttiles and the aux tables staged):
// norm + qkv, M-RoPE + KV append, flash attention, o, norm + gate/up, down.
static void prefill_layers(ze_engine* e, int rows, const prefill_kv& kv, hipStream_t s) {
    const ze_config& c = e->cfg;
    const int H = c.hidden, hd = e->head_dim, nq = c.heads * hd, nqkv = nq + 2 * c.kv_heads * hd;
    const float scale = 1.0f / sqrtf((float)hd);
    const int bq = prefill_bq();
    // the queries' M-RoPE inside the flash kernel (k_mrope_kv_vec then moves K and V only: a fifth of its rows); ze_tune knob 22 = 1:
    // the two-launch form of rounds 1-5 (the same bits: tests/test_gpu_model.py)
    const bool q_in_flash = hd == 128 && ze_mrope_vec_ok != 0 && ze_knobs[ZE_KNOB_MROPE_Q_IN_PLACE] != ZE_KNOB_ON;
    const ze_fa_rope rope = q_in_flash ? ze_fa_rope{e->cosT, e->sinT, e->tpos, c.mrope_section[0], c.mrope_section[0] + c.mrope_section[1], kv.rope_rows}
                                       : ze_fa_rope{nullptr, nullptr, nullptr, 0, 0, 0};
    for (int li = 0; li < c.layers; ++li) {
        const ze_text_layer& L = e->tl[li];
        bf16_t *k = e->kc(li, kv.slot), *v = e->vc(li, kv.slot);
        prefill_projection(e, L, ZE_PROJ_QKV, rows, true, e->tqkv, nqkv, s);
        ze_launch_mrope_kv(e->tqkv, rows, c.heads, c.kv_heads, hd, e->cosT, e->sinT, e->tpos, e->axis_of, k, v, c.max_ctx, kv.past,
                           kv.row_aux, kv.seq_stride, s, q_in_flash ? 1 : 0);
        ze_launch_flash_attn(hd, 1, e->tqkv, nqkv, hd, k, hd, c.max_ctx * hd, v, hd, c.max_ctx * hd, e->to, nq, hd, e->ttiles, kv.n_tiles,
                             c.heads, c.heads / c.kv_heads, scale, kv.past, s, kv.tile_aux, kv.seq_stride, bq, 0, rope);
        prefill_projection(e, L, ZE_PROJ_O, rows, true, e->th, H, s);
        prefill_projection(e, L, ZE_PROJ_GATE_UP, rows, true, e->ta, e->text_ipad, s);
        prefill_projection(e, L, ZE_PROJ_DOWN, rows, true, e->th, H, s);
    }
}

// the lm_head as a ze_linear: the bf16 rows (the embedding table when tied) and, for the decode step of a quantised engine with an
// untied head, its FP8 copy.  The prefill paths read the bf16 rows whatever the engine.
ze_linear lm_head_linear(const ze_engine* e, bool decode) {
    ze_linear l;
    l.w = e->lm_head;
    l.ld = e->cfg.hidden;
    if (decode) {
        l.w8 = e->lm_head8.w8;
        l.scale8 = e->lm_head8.scale8;
        l.ld8 = e->lm_head8.ld8;
        l.w4 = e->lm_head8.w4;
        l.scale4 = e->lm_head8.scale4;
    }
    return l;
}

// the fields every launch of the single-chain GEMV family shares; the caller adds its norm, bias, epilogue targets and extras
ze_gemv_args gemv_args_of(const ze_engine* e, const ze_linear& lin, int N, int K, const bf16_t* x) {
    ze_gemv_args a;
    memset(&a, 0, sizeof(a));
    a.W = lin.w;
    a.ldw = lin.ld;
    if (e->fp8_ready && lin.w8) {
        a.W8 = lin.w8;
        a.scale8 = lin.scale8;
        a.ldw8 = lin.ld8;
    }
    if (e->mx4_ready && lin.w4) {
        a.W4 = lin.w4;
        a.scale4 = lin.scale4;
    }
    a.N = N;
    a.K = K;
    a.x = x;
    a.D = e->head_dim;
    return a;
}

// Final norm + lm_head on the rows x[0..n) into out[0..n) (logits_to_keep = 1, HF:...:1386-1387): the weight matrix streamed once
// per EIGHT rows (ze_gemv_logits.hip), one kernel whatever n -- the first token does not depend on how the chain was prefilled;
// a shape that kernel does not cover takes the single-chain GEMV per row.
static void prefill_logits(ze_engine* e, const bf16_t* const* x, float* const* out, int n, hipStream_t s) {
    const ze_config& c = e->cfg;
    if (ze_launch_logits_rows(e->lm_head, c.hidden, c.vocab, c.hidden, e->final_norm, c.rms_eps, x, out, n, s)) return;
    for (int i = 0; i < n; ++i) {
        ze_gemv_args a = gemv_args_of(e, lm_head_linear(e, false), c.vocab, c.hidden, x[i]);
        a.norm_w = e->final_norm;
        a.eps = c.rms_eps;
        a.out_f32 = out[i];
        ze_launch_gemv(ZE_GV_LOGITS, a, s);
    }
}

// One chain's `len` rows of a prefill pass of `total` rows, from row `row0`, into the pinned staging: ids (an image token becomes
// -1 - its feature row, counted on in `img`) and the three position rows.
static int stage_chain(ze_engine* e, const int32_t* ids, const int32_t* position_ids, int len, int row0, int total, int* src, int* pos,
                       int& img) {
    const ze_config& c = e->cfg;
    for (int t = row0; t < row0 + len; ++t) {
        const int id = ids[t];
        if (id < 0 || id >= c.vocab) return ze_fail(e, ZE_ERR_INVALID, "token id out of range");
        src[t] = (id == c.image_token_id) ? -1 - img++ : id;
        for (int a = 0; a < 3; ++a) {
            const int p = position_ids[(size_t)a * total + t];
            if (p < 0 || p >= e->max_pos) return ze_fail(e, ZE_ERR_INVALID, "position id out of range");
            pos[(size_t)a * total + t] = p;
        }
    }
    return ZE_OK;
}

// the attention tiles of a chain's rows [row0, row0 + len) behind `past` cached rows; returns the new tile count
static int stage_tiles(int* tiles, int nt, int row0, int len, int past) {
    const int bq = prefill_bq();
    for (int q0 = 0; q0 < len; q0 += bq, ++nt) {
        tiles[4 * nt + 0] = row0 + q0;
        tiles[4 * nt + 1] = row0 + std::min(q0 + bq, len);
        tiles[4 * nt + 2] = 0;
        tiles[4 * nt + 3] = past + len;
    }
    return nt;
}

static int image_mismatch(ze_engine* e, int tokens, int features) {
    return ze_fail(e, ZE_ERR_MISMATCH, "Image features and image tokens do not match, tokens: " + std::to_string(tokens) +
                                           ", features: " + std::to_string(features));
}

static int prefill_impl(ze_engine* e, int seq, const int32_t* input_ids, int len, const void* image_embeds,
                        int n_image_rows, const int32_t* position_ids, int rope_delta, float* out_logits,
                        float* out_logps, void* stream) {
    ZE_TRY(check_seq(e, seq));
    if (!input_ids || !position_ids || len <= 0) return ze_fail(e, ZE_ERR_INVALID, "bad prefill arguments");
    const ze_config& c = e->cfg;
    const int past = e->ctx_host[seq];
    if (past + len > c.max_ctx) return ze_fail(e, ZE_ERR_NOMEM, "sequence exceeds max_ctx");
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    const int H = c.hidden;

    ZE_TRY(stage_acquire(e, e->t_staged));  // pinned staging reuse
    int* src = e->t_host_ints;
    int* pos = src + len;
    int* tiles = pos + 3 * len;
    int img = 0;
    ZE_TRY(stage_chain(e, input_ids, position_ids, len, 0, len, src, pos, img));
    if (img != n_image_rows || (img > 0 && !image_embeds)) return image_mismatch(e, img, n_image_rows);
    note_split(e, seq, input_ids, len, past);
    const int nt = stage_tiles(tiles, 0, 0, len, past);
    ZE_HIP(hipMemcpyAsync(e->tsrc, src, (size_t)len * sizeof(int), hipMemcpyHostToDevice, s));
    ZE_HIP(hipMemcpyAsync(e->tpos, pos, (size_t)3 * len * sizeof(int), hipMemcpyHostToDevice, s));
    ZE_HIP(hipMemcpyAsync(e->ttiles, tiles, (size_t)nt * 16, hipMemcpyHostToDevice, s));
    ZE_TRY(stage_release(e, e->t_staged, s));

    const int th = ze_timer_begin(e, 2, s);
    ze_launch_embed_rows(e->tsrc, e->embed, (const bf16_t*)image_embeds, e->th, len, H, s);
    prefill_layers(e, len, prefill_kv{seq, past, nullptr, nullptr, 0, nt, len}, s);
    {
        const bf16_t* xr = e->th + (size_t)(len - 1) * H;
        float* lo = e->dlogits + (size_t)seq * c.vocab;
        prefill_logits(e, &xr, &lo, 1, s);
    }
    if (out_logps && len > 1) {
        // every position: final norm, lm_head GEMM in row chunks (bf16 logits as HF's lm_head gives them), then the
        // log-softmax pick of the next id.  The logits live in the (now free) MLP activation workspace.
        const int ldl = (c.vocab + 7) & ~7;
        int chunk = (int)std::min<size_t>((size_t)e->prefill_rows * e->text_ipad / ldl, (size_t)len - 1);
        if (chunk >= 128) chunk &= ~127;
        if (chunk < 1) return ze_fail(e, ZE_ERR_NOMEM, "prefill workspace too small for one row of logits");
        ZE_HIP(hipMemcpyAsync(e->trow_aux, input_ids + 1, (size_t)(len - 1) * sizeof(int), hipMemcpyHostToDevice, s));
        ze_launch_rmsnorm(e->th, H, e->final_norm, e->ty, H, len - 1, H, c.rms_eps, s);
        for (int r0 = 0; r0 < len - 1; r0 += chunk) {
            const int m = std::min(chunk, len - 1 - r0);
            ze_launch_gemm(ZE_EPI_NONE, e->ty + (size_t)r0 * H, H, e->lm_head, H, nullptr, nullptr, 0, e->ta, ldl,
                           nullptr, m, c.vocab, H, s);
            ze_launch_token_logprob(e->ta, ldl, c.vocab, e->trow_aux + r0, out_logps + r0, m, s);
        }
    }
    ze_timer_end(e, th, s);
    ZE_KCHECK();
    if (out_logits)
        ZE_HIP(hipMemcpyAsync(out_logits, e->dlogits + (size_t)seq * c.vocab, (size_t)c.vocab * sizeof(float),
                              hipMemcpyDeviceToDevice, s));
    e->ctx_host[seq] = past + len;
    e->delta_host[seq] = rope_delta;
    e->logits_fresh[seq] = 1;  // (ze_prefill and ze_score alike: the chain is "as after ze_prefill")
    e->tok_host[seq] = input_ids[len - 1];
    return push_state(e, seq, s, input_ids[len - 1], 0, 0);
}

extern "C" int ze_prefill(ze_engine* e, int seq, const int32_t* input_ids, int len, const void* image_embeds,
                          int n_image_rows, const int32_t* position_ids, int rope_delta, float* out_logits,
                          void* stream) {
    return prefill_impl(e, seq, input_ids, len, image_embeds, n_image_rows, position_ids, rope_delta, out_logits,
                        nullptr, stream);
}

extern "C" int ze_score(ze_engine* e, int seq, const int32_t* input_ids, int len, const void* image_embeds,
                        int n_image_rows, const int32_t* position_ids, int rope_delta, float* out_logps,
                        void* stream) {
    if (!out_logps) return ze_fail(e, ZE_ERR_INVALID, "ze_score needs an output buffer");
    return prefill_impl(e, seq, input_ids, len, image_embeds, n_image_rows, position_ids, rope_delta, nullptr,
                        out_logps, stream);
}

// Prefill of n chains in one pass: all rows share every GEMM, attention and the KV append go per chain.  The staging and the pass
// of ze_prefill_batch and ze_score_batch: with out_logps (the scoring pass) chain i's new rows [score_from[i], lens[i] - 1) are
// listed with their next ids in e->tscore and, behind the layers and the chains' last-position logits, go through the scored-row
// path (ze_score.hip) into out_logps, packed in chain order.  Without it nothing more is staged or launched than the prefill's own.
static int prefill_batch_impl(ze_engine* e, const int32_t* seqs, int n, const int32_t* lens, const int32_t* input_ids,
                              const void* image_embeds, const int32_t* n_image_rows, const int32_t* position_ids,
                              const int32_t* rope_deltas, const int32_t* score_from, float* out_logps,
                              const ze_score_detail_out* detail, void* stream) {
    if (!e || !seqs || !lens || !input_ids || !position_ids || !rope_deltas || n <= 0)
        return ze_fail(e, ZE_ERR_INVALID, "bad prefill arguments");
    const ze_config& c = e->cfg;
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    const int H = c.hidden;
    int total = 0;
    for (int i = 0; i < n; ++i) {
        ZE_TRY(check_seq(e, seqs[i]));
        for (int k2 = 0; k2 < i; ++k2)
            if (seqs[k2] == seqs[i]) return ze_fail(e, ZE_ERR_INVALID, "a chain appears twice in the batch");
        if (lens[i] <= 0) return ze_fail(e, ZE_ERR_INVALID, "bad prefill arguments");
        if (e->ctx_host[seqs[i]] + lens[i] > c.max_ctx) return ze_fail(e, ZE_ERR_NOMEM, "sequence exceeds max_ctx");
        total += lens[i];
    }
    if (total > e->prefill_rows) return ze_fail(e, ZE_ERR_NOMEM, "batched prefill exceeds max_prefill_rows");
    int n_scored = 0;
    if (out_logps)
        for (int i = 0; i < n; ++i) {
            const int from = score_from ? score_from[i] : 0;
            if (from < 0 || from > lens[i] - 1) return ze_fail(e, ZE_ERR_INVALID, "score_from out of range");
            n_scored += lens[i] - 1 - from;
        }
    if (n_scored > 0 && ze_score_chunk_rows(e, n_scored) < 1)
        return ze_fail(e, ZE_ERR_NOMEM, "prefill workspace too small for one row of logits");

    ZE_TRY(stage_acquire(e, e->t_staged));  // pinned staging reuse
    int* src = e->t_host_ints;
    int* pos = src + total;
    int* row_aux = pos + 3 * total;
    int* score_tab = row_aux + 2 * total;  // [n_scored] rows of the pass, then [n_scored] target ids
    int* tiles = score_tab + 2 * n_scored;
    for (int i = 0, r0 = 0, k = 0; i < n && out_logps; r0 += lens[i], ++i)
        for (int t = score_from ? score_from[i] : 0; t < lens[i] - 1; ++t, ++k) {
            score_tab[k] = r0 + t;
            score_tab[n_scored + k] = input_ids[r0 + t + 1];
        }
    int img = 0, nt = 0, row0 = 0;
    std::vector<int> tile_aux;
    for (int i = 0; i < n; ++i) {
        const int seq = seqs[i], len = lens[i], past = e->ctx_host[seq], img0 = img;
        ZE_TRY(stage_chain(e, input_ids, position_ids, len, row0, total, src, pos, img));
        for (int t = 0; t < len; ++t) {
            row_aux[2 * (row0 + t)] = seq;
            row_aux[2 * (row0 + t) + 1] = past + t;
        }
        note_split(e, seq, input_ids + row0, len, past);
        const int want = n_image_rows ? n_image_rows[i] : 0;
        if (img - img0 != want || (img > img0 && !image_embeds)) return image_mismatch(e, img - img0, want);
        const int nt0 = nt;
        nt = stage_tiles(tiles, nt, row0, len, past);
        for (int t = nt0; t < nt; ++t) {
            tile_aux.push_back(seq);
            tile_aux.push_back(past - row0);  // key index visible to row r: <= r + (past - row0)
        }
        row0 += len;
    }
    int* taux = tiles + 4 * nt;
    memcpy(taux, tile_aux.data(), tile_aux.size() * sizeof(int));
    ZE_HIP(hipMemcpyAsync(e->tsrc, src, (size_t)total * sizeof(int), hipMemcpyHostToDevice, s));
    ZE_HIP(hipMemcpyAsync(e->tpos, pos, (size_t)3 * total * sizeof(int), hipMemcpyHostToDevice, s));
    ZE_HIP(hipMemcpyAsync(e->trow_aux, row_aux, (size_t)2 * total * sizeof(int), hipMemcpyHostToDevice, s));
    ZE_HIP(hipMemcpyAsync(e->ttiles, tiles, (size_t)nt * 16, hipMemcpyHostToDevice, s));
    ZE_HIP(hipMemcpyAsync(e->ttile_aux, taux, (size_t)nt * 2 * sizeof(int), hipMemcpyHostToDevice, s));
    if (n_scored > 0) ZE_HIP(hipMemcpyAsync(e->tscore, score_tab, (size_t)2 * n_scored * sizeof(int), hipMemcpyHostToDevice, s));
    ZE_TRY(stage_release(e, e->t_staged, s));

    const int th = ze_timer_begin(e, 2, s);
    ze_launch_embed_rows(e->tsrc, e->embed, (const bf16_t*)image_embeds, e->th, total, H, s);
    prefill_layers(e, total, prefill_kv{0, 0, e->trow_aux, e->ttile_aux, (size_t)c.kv_heads * c.max_ctx * e->head_dim, nt, total}, s);
    {  // last position of every chain
        std::vector<const bf16_t*> xr(n);
        std::vector<float*> lo(n);
        row0 = 0;
        for (int i = 0; i < n; ++i) {
            xr[i] = e->th + (size_t)(row0 + lens[i] - 1) * H;
            lo[i] = e->dlogits + (size_t)seqs[i] * c.vocab;
            row0 += lens[i];
        }
        prefill_logits(e, xr.data(), lo.data(), n, s);
    }
    if (n_scored > 0) ZE_TRY(ze_score_rows(e, n_scored, out_logps, detail, s));
    ze_timer_end(e, th, s);
    ZE_KCHECK();
    row0 = 0;
    for (int i = 0; i < n; ++i) {
        e->ctx_host[seqs[i]] += lens[i];
        e->delta_host[seqs[i]] = rope_deltas[i];
        e->logits_fresh[seqs[i]] = 1;
        e->tok_host[seqs[i]] = input_ids[row0 + lens[i] - 1];
        ZE_TRY(push_state(e, seqs[i], s, input_ids[row0 + lens[i] - 1], 0, 0));
        row0 += lens[i];
    }
    return ZE_OK;
}

extern "C" int ze_prefill_batch(ze_engine* e, const int32_t* seqs, int n, const int32_t* lens, const int32_t* input_ids,
                                const void* image_embeds, const int32_t* n_image_rows, const int32_t* position_ids,
                                const int32_t* rope_deltas, void* stream) {
    return prefill_batch_impl(e, seqs, n, lens, input_ids, image_embeds, n_image_rows, position_ids, rope_deltas, nullptr, nullptr, nullptr, stream);
}

extern "C" int ze_score_batch(ze_engine* e, const int32_t* seqs, int n, const int32_t* lens, const int32_t* input_ids,
                              const void* image_embeds, const int32_t* n_image_rows, const int32_t* position_ids,
                              const int32_t* rope_deltas, const int32_t* score_from, float* out_logps, void* stream) {
    if (!out_logps) return ze_fail(e, ZE_ERR_INVALID, "ze_score_batch needs an output buffer");
    return prefill_batch_impl(e, seqs, n, lens, input_ids, image_embeds, n_image_rows, position_ids, rope_deltas, score_from, out_logps,
                              nullptr, stream);
}

extern "C" int ze_score_batch_detail(ze_engine* e, const int32_t* seqs, int n, const int32_t* lens, const int32_t* input_ids,
                                     const void* image_embeds, const int32_t* n_image_rows, const int32_t* position_ids,
                                     const int32_t* rope_deltas, const int32_t* score_from, int top_n, float* out_logps,
                                     float* out_entropy, int32_t* out_rank, int32_t* out_top_ids, float* out_top_logprobs, void* stream) {
    if (!out_logps) return ze_fail(e, ZE_ERR_INVALID, "ze_score_batch_detail needs an output buffer");
    if (top_n < 0 || top_n > ZE_MAX_TOP_LOGPROBS) return ze_fail(e, ZE_ERR_INVALID, "top_n must be in [0, 20]");
    if (!out_top_ids != !out_top_logprobs || (out_top_ids && top_n < 1))
        return ze_fail(e, ZE_ERR_INVALID, "the top arrays are both null, or both set with top_n >= 1");
    ze_score_detail_out d;
    d.top_n = out_top_ids ? top_n : 0, d.entropy = out_entropy, d.rank = out_rank, d.top_ids = out_top_ids, d.top_lps = out_top_logprobs;
    return prefill_batch_impl(e, seqs, n, lens, input_ids, image_embeds, n_image_rows, position_ids, rope_deltas, score_from, out_logps,
                              &d, stream);
}

// ================================================================== decode
// decode attention of the single-chain step: no chain table, the chain's own device state, the <24, 1> instantiation of the
// slice kernel (ze_attn_decode.hip) over rows 0 .. ctx of the chain's cache
// (q_row / out_row: the step's own buffers, or the caller's -- ze_op_attn_decode_single)
void launch_step_attention(ze_engine* e, int li, int seq, hipStream_t s, const bf16_t* q_row, bf16_t* out_row) {
    const ze_config& c = e->cfg;
    const int hd = e->head_dim;
    const float scale = 1.0f / sqrtf((float)hd);
    ze_launch_attn_decode(q_row ? q_row : e->dq, 0, e->kc(li, seq), e->vc(li, seq), 0, out_row ? out_row : e->dattn, 0, e->st_dev + seq,
                          nullptr, 1, c.heads, c.kv_heads, hd, c.max_ctx, scale, e->dpartial, e->max_splits, e->atickets, s);
}

// One token for chain `seq`: everything is read from the device-side chain state, so the same launch
// sequence can be captured once into a hipGraph and replayed.
static int ze_enqueue_decode_step(ze_engine* e, int seq, float penalty, int ignore_eos, bool sample, const ze_sample_opts& so,
                                  hipStream_t s) {
    const ze_config& c = e->cfg;
    const int H = c.hidden, hd = e->head_dim, nq = c.heads * hd, nqkv = nq + 2 * c.kv_heads * hd;
    const ze_seq_dev* st = e->st_dev + seq;
    for (int li = 0; li < c.layers; ++li) {
        const ze_text_layer& L = e->tl[li];
        ze_gemv_args a = gemv_args_of(e, L.qkv, nqkv, H, e->dh);
        a.norm_w = L.in_norm;
        a.eps = c.rms_eps;
        a.bias = L.qkv.bias;
        a.out_bf16 = e->dq;
        a.st = st;
        a.cosT = e->cosT;
        a.sinT = e->sinT;
        a.kcache = e->kc(li, seq);
        a.vcache = e->vc(li, seq);
        a.heads = c.heads;
        a.kv_heads = c.kv_heads;
        a.max_ctx = c.max_ctx;
        a.act8 = e->fp8_act ? 1 : 0;
        if (li == 0) {
            a.embed = e->embed;
            a.embed_out = e->dh;
        }
        ze_launch_gemv(ZE_GV_QKV_ROPE, a, s);
        launch_step_attention(e, li, seq, s);
        ze_gemv_args o = gemv_args_of(e, L.o, H, nq, e->dattn);
        o.out_bf16 = e->dh;
        ze_launch_gemv(ZE_GV_RESIDUAL, o, s);
        ze_gemv_args g = gemv_args_of(e, L.gate_up, 2 * e->text_ipad, H, e->dh);
        g.norm_w = L.post_norm;
        g.eps = c.rms_eps;
        g.out_bf16 = e->dact;
        g.act8 = e->fp8_act ? 1 : 0;
        ze_launch_gemv(ZE_GV_SWIGLU, g, s);
        ze_gemv_args d = gemv_args_of(e, L.down, H, e->text_ipad, e->dact);
        d.out_bf16 = e->dh;
        ze_launch_gemv(ZE_GV_RESIDUAL, d, s);
    }
    ze_gemv_args a = gemv_args_of(e, lm_head_linear(e, true), c.vocab, H, e->dh);
    a.norm_w = e->final_norm;
    a.eps = c.rms_eps;
    a.out_f32 = e->dlogits + (size_t)seq * c.vocab;
    // greedy: the arg-max partials come out of the lm_head launch itself (knob 14 = 1: the separate partial kernel)
    // (a chain with a logit-adjust request, bans or a grammar keeps off it: the folded arg-max never sees the row)
    const bool folded = sample && so.temperature <= 0.f && ze_knobs[ZE_KNOB_SEPARATE_ARGMAX] != ZE_KNOB_ON && !e->req.la_host[seq].on() && !e->req.tr_host[seq].bans() &&
                        e->req.gr_host[seq] < 0;
    if (folded) {
        a.seen = e->seen + (size_t)seq * c.vocab;
        a.penalty = penalty;
        a.amax_ws = e->damax;
    }
    const bool gemv_ok = ze_launch_gemv(ZE_GV_LOGITS, a, s);
    if (folded && gemv_ok)
        ze_launch_sample_folded(e->damax, c.vocab, e->seen + (size_t)seq * c.vocab, e->st_dev + seq, e->eos_dev, c.n_eos,
                                c.pad_token_id, ignore_eos, /*advance_ctx=*/1, e->out_tokens + (size_t)seq * c.max_ctx, s);
    else if (sample)
        ze_launch_sample(ze_requests_rows(e, e->dlogits + (size_t)seq * c.vocab, nullptr, seq, 1, s), c.vocab, e->seen + (size_t)seq * c.vocab,
                         penalty, e->st_dev + seq, e->eos_dev, c.n_eos, c.pad_token_id, ignore_eos, /*advance_ctx=*/1,
                         e->out_tokens + (size_t)seq * c.max_ctx, e->dsample, so, s);
    else
        ze_launch_advance_ctx(e->st_dev + seq, s);  // teacher forcing: the caller chooses the next token
    if (sample) ze_requests_after_token(e, e->dlogits + (size_t)seq * c.vocab, nullptr, seq, 1, s);
    ZE_KCHECK();
    return ZE_OK;
}

extern "C" int ze_decode_step(ze_engine* e, int seq, int token, float* out_logits, void* stream) {
    ZE_TRY(check_seq(e, seq));
    const ze_config& c = e->cfg;
    if (e->ctx_host[seq] + 1 > c.max_ctx) return ze_fail(e, ZE_ERR_NOMEM, "sequence exceeds max_ctx");
    if (token >= c.vocab) return ze_fail(e, ZE_ERR_INVALID, "token id out of range");
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    e->logits_fresh[seq] = 0;
    if (token >= 0) ze_launch_set_ints(&(e->st_dev + seq)->token, &token, 1, s);
    const int th = ze_timer_begin(e, 3, s);
    ZE_TRY(ze_enqueue_decode_step(e, seq, 1.0f, 1, false, ze_sample_opts{}, s));
    ze_timer_end(e, th, s);
    e->ctx_host[seq] += 1;
    if (out_logits)
        ZE_HIP(hipMemcpyAsync(out_logits, e->dlogits + (size_t)seq * c.vocab, (size_t)c.vocab * sizeof(float),
                              hipMemcpyDeviceToDevice, s));
    return ZE_OK;
}

// One decode step, as `enqueue` puts it on the stream it is given, captured into an executable graph
int capture_step(ze_engine* e, const std::function<int(hipStream_t)>& enqueue, hipGraphExec_t* exec) {
    hipStream_t cs;
    ZE_HIP(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    hipGraph_t graph = nullptr;
    int r = ZE_OK;
    if (hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) != hipSuccess)
        r = ze_fail(e, ZE_ERR_HIP, "hipStreamBeginCapture failed");
    if (r == ZE_OK) r = enqueue(cs);
    if (hipStreamEndCapture(cs, &graph) != hipSuccess && r == ZE_OK)
        r = ze_fail(e, ZE_ERR_HIP, "hipStreamEndCapture failed");
    if (r == ZE_OK && hipGraphInstantiate(exec, graph, nullptr, nullptr, 0) != hipSuccess)
        r = ze_fail(e, ZE_ERR_HIP, "hipGraphInstantiate failed");
    if (graph) hipGraphDestroy(graph);
    hipStreamDestroy(cs);
    return r;
}

// first token of chain `q` from the logits its prefill left behind (no cache growth)
int first_token(ze_engine* e, int q, float pen, int ign, const ze_sample_opts& so, hipStream_t s) {
    const ze_config& c = e->cfg;
    const float* row = e->dlogits + (size_t)q * c.vocab;
    e->logits_fresh[q] = 0;  // (the draw marks the seen-set and moves the chain state: no longer what the prefill left)
    ze_launch_sample(ze_requests_rows(e, row, nullptr, q, 1, s), c.vocab, e->seen + (size_t)q * c.vocab, pen, e->st_dev + q, e->eos_dev,
                     c.n_eos, c.pad_token_id, ign, 0, e->out_tokens + (size_t)q * c.max_ctx, e->dsample, so, s);
    ze_requests_after_token(e, row, nullptr, q, 1, s);
    ZE_KCHECK();
    return ZE_OK;
}

// tokens up to and including the first EOS (those after it are pad, as HF emits for finished rows)
int trim_at_eos(const ze_config& c, const int32_t* tokens, int n) {
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < c.n_eos; ++k)
            if (tokens[i] == c.eos_token_ids[k]) return i + 1;
    return n;
}

extern "C" int ze_generate(ze_engine* e, int seq, const ze_gen_params* p, int32_t* out_tokens, int* n_out,
                           void* stream) {
    ZE_TRY(check_seq(e, seq));
    if (!p || !out_tokens || !n_out) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    const ze_config& c = e->cfg;
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    int max_new = p->max_new_tokens;
    if (max_new <= 0) {
        *n_out = 0;
        return ZE_OK;
    }
    // the last generated token is never fed back, so ctx grows by max_new - 1
    if (e->ctx_host[seq] + max_new - 1 > c.max_ctx) max_new = c.max_ctx - e->ctx_host[seq] + 1;
    if (max_new <= 0) return ze_fail(e, ZE_ERR_NOMEM, "sequence exceeds max_ctx");
    const float pen = ze_penalty_of(e, p, seq);  // (the graph below is keyed by the effective values: a new request re-captures it)
    const int ign = p->ignore_eos ? 1 : 0;
    const ze_sample_opts so = ze_sample_opts_of(e, p, seq);
    int32_t* dev_out = e->out_tokens + (size_t)seq * c.max_ctx;
    ze_seq_dev* st = e->st_dev + seq;

    const int t_s = ze_timer_begin(e, 4, s);
    const int r0 = first_token(e, seq, pen, ign, so, s);
    ze_timer_end(e, t_s, s);
    ZE_TRY(r0);

    // decode-step graph for this chain (re-captured when the sampling options change)
    hipGraphExec_t gexec = nullptr;
    if (p->use_graph && max_new > 1) {
        const ze_step_key key = ze_step_key_of(e, 0, seq, pen, ign, so);
        if (!e->graphs[seq] || !(e->graph_key[seq] == key)) {
            if (e->graphs[seq]) {
                hipGraphExecDestroy(e->graphs[seq]);
                e->graphs[seq] = nullptr;
            }
            ZE_TRY(capture_step(e, [&](hipStream_t cs) { return ze_enqueue_decode_step(e, seq, pen, ign, true, so, cs); }, &e->graphs[seq]));
            e->graph_key[seq] = key;
        }
        gexec = e->graphs[seq];
    }

    const int sync_every = std::max(1, p->sync_every);
    int produced = 1;  // tokens sampled so far (device side)
    int finished = 0;
    const int t_d = ze_timer_begin(e, 3, s);
    while (produced < max_new && !finished) {
        const int burst = std::min(sync_every, max_new - produced);
        for (int i = 0; i < burst; ++i) {
            if (gexec)
                ZE_HIP(hipGraphLaunch(gexec, s));
            else
                ZE_TRY(ze_enqueue_decode_step(e, seq, pen, ign, true, so, s));
        }
        produced += burst;
        e->ctx_host[seq] += burst;
        if (!ign && produced < max_new) {
            ZE_HIP(hipMemcpyAsync(e->d_host_ints + 32, &st->finished, sizeof(int), hipMemcpyDeviceToHost, s));
            ZE_HIP(hipStreamSynchronize(s));
            finished = e->d_host_ints[32];
        }
    }
    ze_timer_end(e, t_d, s);
    ZE_HIP(hipMemcpyAsync(out_tokens, dev_out, (size_t)produced * sizeof(int), hipMemcpyDeviceToHost, s));
    ZE_HIP(hipStreamSynchronize(s));
    *n_out = ign ? produced : trim_at_eos(c, out_tokens, produced);
    return ZE_OK;
}

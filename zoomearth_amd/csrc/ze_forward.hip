// Forward passes of the engine: image front-end, ViT, LLM prefill, the single-chain decode step (eager or hipGraph), greedy
// generation, plus the unit ops and the measurement hooks of the C ABI.  The batched decode step: ze_decode_batch.hip.
#include <math.h>
#include <cmath>
#include <string.h>

#include <algorithm>

#include "ze_engine.h"

extern int ze_gemv_knobs[25];

// ================================================================== front-end
// dst = crop(src, box).resize((dst_w, dst_h), BICUBIC), Pillow-exact (two passes, u8 intermediate).
static int frontend_acquire(ze_engine* e) {
    if (e->fe_in_flight) {
        ZE_HIP(hipEventSynchronize(e->fe_done));
        e->fe_in_flight = false;
    }
    return ZE_OK;
}
// called behind the last kernel that reads the workspace
static int frontend_release(ze_engine* e, hipStream_t s) {
    if (!e->fe_done) ZE_HIP(hipEventCreateWithFlags(&e->fe_done, hipEventDisableTiming));
    ZE_HIP(hipEventRecord(e->fe_done, s));
    e->fe_in_flight = true;
    return ZE_OK;
}
// A pinned staging buffer is rewritten by the next call: wait until the copies that read it have run -- an event right behind
// them, not the whole stream (which holds the ViT / prefill kernels enqueued since: the scheduler's thread used to sit 20-40 ms
// in every vit_forward / prefill_batch call, and with bursts shorter than that -- 64 chain slots -- the decode stream idled)
static int stage_acquire(ze_engine* e, hipEvent_t& ev) {
    if (ev) ZE_HIP(hipEventSynchronize(ev));
    return ZE_OK;
}
static int stage_release(ze_engine* e, hipEvent_t& ev, hipStream_t s) {
    if (!ev) ZE_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    ZE_HIP(hipEventRecord(ev, s));
    return ZE_OK;
}
static int crop_resize(ze_engine* e, const uint8_t* src, int src_h, int src_w, const int32_t box[4], uint8_t* dst,
                       int dst_h, int dst_w, hipStream_t s) {
    const int bx0 = box[0], by0 = box[1];
    const int bw = box[2] - box[0], bh = box[3] - box[1];
    if (bw <= 0 || bh <= 0 || dst_w <= 0 || dst_h <= 0) return ze_fail(e, ZE_ERR_INVALID, "empty crop box or output");
    const bool need_h = bw != dst_w, need_v = bh != dst_h;
    if (!need_h && !need_v) {
        ze_launch_crop(src, src_h, src_w, bx0, by0, dst, dst_h, dst_w, s);
        ZE_KCHECK();
        return ZE_OK;
    }
    ze_coeffs ch, cv;
    size_t ints = 0;
    if (need_h) {
        ze_bicubic_coeffs(bw, dst_w, &ch);
        ints += 2 * (size_t)dst_w + ch.kk.size();
    }
    if (need_v) {
        ze_bicubic_coeffs(bh, dst_h, &cv);
        ints += 2 * (size_t)dst_h + cv.kk.size();
    }
    if (ints > e->fe_coef_ints) return ze_fail(e, ZE_ERR_NOMEM, "bicubic coefficient table exceeds workspace");
    if (need_h && need_v && (size_t)bh * dst_w * 3 > e->fe_tmp_bytes)
        return ze_fail(e, ZE_ERR_NOMEM, "resize intermediate exceeds workspace (max_tile_side)");
    // ONE workspace per engine (coefficient tables, their pinned staging buffer, the horizontal-pass image, the resized
    // image) and callers on several streams (the scheduler crops on its side stream while the loop that feeds it resizes
    // the next tile's view on its own): wait for the previous front-end op, whatever stream it ran on
    ZE_TRY(frontend_acquire(e));
    int* hp = e->fe_coef_host;
    int* dp = e->fe_coef;
    size_t o = 0;
    const int *d_xmin = nullptr, *d_xcnt = nullptr, *d_xk = nullptr, *d_ymin = nullptr, *d_ycnt = nullptr,
              *d_yk = nullptr;
    auto put = [&](const std::vector<int>& v) {
        memcpy(hp + o, v.data(), v.size() * sizeof(int));
        const int* d = dp + o;
        o += v.size();
        return d;
    };
    if (need_h) {
        d_xmin = put(ch.xmin);
        d_xcnt = put(ch.xcnt);
        d_xk = put(ch.kk);
    }
    if (need_v) {
        d_ymin = put(cv.xmin);
        d_ycnt = put(cv.xcnt);
        d_yk = put(cv.kk);
    }
    ZE_HIP(hipMemcpyAsync(dp, hp, o * sizeof(int), hipMemcpyHostToDevice, s));
    if (need_h) {
        uint8_t* hout = need_v ? e->fe_tmp : dst;
        // widest source span of a 64-column block: 64*scale + 2*support  (+ slack)
        int max_span = 0;
        for (int c0 = 0; c0 < dst_w; c0 += 64) {
            const int last = std::min(dst_w, c0 + 64) - 1;
            max_span = std::max(max_span, ch.xmin[last] + ch.xcnt[last] - ch.xmin[c0]);
        }
        const int inside = bx0 >= 0 && by0 >= 0 && bx0 + bw <= src_w && by0 + bh <= src_h;
        ze_launch_resize_h(src, src_h, src_w, bx0, by0, bh, hout, dst_w, d_xmin, d_xcnt, d_xk, ch.ksize, max_span, s, inside);
        ZE_KCHECK();
        if (need_v) {
            ze_launch_resize_v(e->fe_tmp, bh, dst_w, 0, 0, dst_w * 3, dst, dst_h, d_ymin, d_ycnt, d_yk, cv.ksize, 0, s);
            ZE_KCHECK();
        }
    } else {
        ze_launch_resize_v(src, src_h, src_w, bx0, by0, dst_w * 3, dst, dst_h, d_ymin, d_ycnt, d_yk, cv.ksize, 1, s);
        ZE_KCHECK();
    }
    return ZE_OK;
}

extern "C" int ze_tile_upload(ze_engine* e, const uint8_t* host_rgb, int h, int w, uint8_t* dev_rgb, void* stream) {
    if (!e || !host_rgb || !dev_rgb || h <= 0 || w <= 0) return ze_fail(e, ZE_ERR_INVALID, "bad tile_upload arguments");
    hipSetDevice(e->device);
    ZE_HIP(hipMemcpyAsync(dev_rgb, host_rgb, (size_t)h * w * 3, hipMemcpyHostToDevice, (hipStream_t)stream));
    return ZE_OK;
}

extern "C" int ze_op_crop_resize(ze_engine* e, const uint8_t* src, int src_h, int src_w, const int32_t box[4],
                                 uint8_t* dst, int dst_h, int dst_w, void* stream) {
    if (!e || !src || !dst || !box) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    const int h = ze_timer_begin(e, 0, s);
    int r = crop_resize(e, src, src_h, src_w, box, dst, dst_h, dst_w, s);
    if (r == ZE_OK) r = frontend_release(e, s);
    ze_timer_end(e, h, s);
    return r;
}

extern "C" int ze_smart_resize(int height, int width, int factor, int64_t min_pixels, int64_t max_pixels, int* out_h,
                               int* out_w) {
    if (ze_smart_resize_impl(height, width, factor, min_pixels, max_pixels, out_h, out_w) != 0)
        return ze_fail(nullptr, ZE_ERR_INVALID, "absolute aspect ratio must be smaller than 200");
    return ZE_OK;
}

extern "C" int ze_op_patchify(ze_engine* e, const uint8_t* img, int h, int w, float* out, void* stream) {
    if (!e || !img || !out) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    const ze_config& c = e->cfg;
    const int f = c.patch_size * c.spatial_merge_size;
    if (h % f || w % f) return ze_fail(e, ZE_ERR_INVALID, "image size must be a multiple of patch*merge");
    hipSetDevice(e->device);
    ze_launch_patchify(img, h, w, e->lut, out, c.patch_size, c.spatial_merge_size, c.temporal_patch_size,
                       c.in_channels, (hipStream_t)stream);
    ZE_KCHECK();
    return ZE_OK;
}

extern "C" int ze_preprocess_image(ze_engine* e, const uint8_t* img, int h, int w, int64_t min_pixels,
                                   int64_t max_pixels, float* out, int64_t capacity_rows, int32_t grid_thw[3],
                                   void* stream) {
    if (!e || !img || !out || !grid_thw) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    const ze_config& c = e->cfg;
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    const int f = c.patch_size * c.spatial_merge_size;
    int rh, rw;
    if (ze_smart_resize_impl(h, w, f, min_pixels, max_pixels, &rh, &rw) != 0)
        return ze_fail(e, ZE_ERR_INVALID, "absolute aspect ratio must be smaller than 200");
    const int64_t rows = (int64_t)(rh / c.patch_size) * (rw / c.patch_size);
    if (rows > capacity_rows) return ze_fail(e, ZE_ERR_NOMEM, "pixel_values capacity too small");
    if ((size_t)rh * rw * 3 > e->fe_img_bytes) return ze_fail(e, ZE_ERR_NOMEM, "resized image exceeds workspace");
    const int th = ze_timer_begin(e, 0, s);
    const uint8_t* cur = img;
    if (rh != h || rw != w) {
        const int32_t box[4] = {0, 0, w, h};
        ZE_TRY(crop_resize(e, img, h, w, box, e->fe_img, rh, rw, s));
        cur = e->fe_img;
    }
    ze_launch_patchify(cur, rh, rw, e->lut, out, c.patch_size, c.spatial_merge_size, c.temporal_patch_size,
                       c.in_channels, s);
    if (cur == e->fe_img) ZE_TRY(frontend_release(e, s));
    ze_timer_end(e, th, s);
    ZE_KCHECK();
    grid_thw[0] = 1;
    grid_thw[1] = rh / c.patch_size;
    grid_thw[2] = rw / c.patch_size;
    return ZE_OK;
}

// ================================================================== index helpers (C ABI wrappers)
extern "C" int ze_vision_window_index(const ze_config* cfg, const int32_t* grid_thw, int n_images,
                                      int64_t* window_index, int32_t* cu_window, int cap_cu, int* n_cu) {
    if (!cfg || !grid_thw || !window_index || !cu_window || !n_cu)
        return ze_fail(nullptr, ZE_ERR_INVALID, "null argument");
    std::vector<int64_t> wi;
    std::vector<int32_t> cu;
    ze_window_index_impl(grid_thw, n_images, cfg->spatial_merge_size, cfg->window_size, cfg->patch_size, wi, cu);
    if ((int)cu.size() > cap_cu) return ze_fail(nullptr, ZE_ERR_NOMEM, "cu_window capacity too small");
    memcpy(window_index, wi.data(), wi.size() * sizeof(int64_t));
    memcpy(cu_window, cu.data(), cu.size() * sizeof(int32_t));
    *n_cu = (int)cu.size();
    return ZE_OK;
}

extern "C" int ze_rope_index(const ze_config* cfg, const int32_t* input_ids, int len, const int32_t* grid_thw,
                             int n_images, int32_t* position_ids, int32_t* rope_delta) {
    if (!cfg || !input_ids || !position_ids || !rope_delta) return ze_fail(nullptr, ZE_ERR_INVALID, "null argument");
    const int r = ze_rope_index_impl(input_ids, len, grid_thw, n_images, cfg->image_token_id, cfg->spatial_merge_size,
                                     position_ids, rope_delta);
    if (r != 0)
        return ze_fail(nullptr, ZE_ERR_MISMATCH, "Image features and image tokens do not match (rope index)");
    return ZE_OK;
}

// ================================================================== attention tile lists
// one tile = up to 64 query rows of one segment against that segment's keys
static int build_tiles(const int32_t* cu, int n_seg, int* out /* int4 rows */, int cap_tiles, int bq = 64) {
    int n = 0;
    for (int sgi = 0; sgi < n_seg; ++sgi)
        for (int q0 = cu[sgi]; q0 < cu[sgi + 1]; q0 += bq) {
            if (n >= cap_tiles) return -1;
            out[4 * n + 0] = q0;
            out[4 * n + 1] = std::min(q0 + bq, cu[sgi + 1]);
            out[4 * n + 2] = cu[sgi];
            out[4 * n + 3] = cu[sgi + 1];
            ++n;
        }
    return n;
}

// ================================================================== ViT
extern "C" int ze_vit_forward(ze_engine* e, const float* pixel_values, const int32_t* grid_thw, int n_images,
                              void* out_embeds, void* stream) {
    if (!e || !pixel_values || !grid_thw || !out_embeds || n_images <= 0)
        return ze_fail(e, ZE_ERR_INVALID, "null argument");
    const ze_config& c = e->cfg;
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    const int mu = c.spatial_merge_size * c.spatial_merge_size;
    int n = 0;
    for (int i = 0; i < n_images; ++i) {
        const int t = grid_thw[3 * i], h = grid_thw[3 * i + 1], w = grid_thw[3 * i + 2];
        if (t <= 0 || h <= 0 || w <= 0 || h % c.spatial_merge_size || w % c.spatial_merge_size)
            return ze_fail(e, ZE_ERR_INVALID, "bad grid_thw");
        n += t * h * w;
    }
    if (n > c.max_patches) return ze_fail(e, ZE_ERR_NOMEM, "too many patches for max_patches");
    const int vh = c.vit_hidden, hd = e->vit_head_dim, half = hd / 2, nh = c.vit_heads;
    const int pk = c.in_channels * c.temporal_patch_size * c.patch_size * c.patch_size;

    // ---- host index prep (integer): window permutation, segment tiles, rotary tables
    std::vector<int64_t> widx;
    std::vector<int32_t> cu_win, cu_full(1, 0), hw;
    ze_window_index_impl(grid_thw, n_images, c.spatial_merge_size, c.window_size, c.patch_size, widx, cu_win);
    for (int i = 0; i < n_images; ++i)
        for (int t = 0; t < grid_thw[3 * i]; ++t)
            cu_full.push_back(cu_full.back() + grid_thw[3 * i + 1] * grid_thw[3 * i + 2]);
    ze_vision_pos_ids_impl(grid_thw, n_images, c.spatial_merge_size, hw);
    ZE_TRY(stage_acquire(e, e->v_staged));  // pinned staging reuse
    int* hi = e->v_host_ints;
    int* perm = hi;              // [n]   new row r <- old row perm[r]
    int* inv = hi + n;           // [n/mu] merged row j (window order) -> HF order row
    int* tw = hi + 2 * n;        // window tiles
    for (int j = 0; j < n / mu; ++j) {
        for (int u = 0; u < mu; ++u) perm[j * mu + u] = (int)widx[j] * mu + u;
        inv[j] = (int)widx[j];
    }
    const int ntw = build_tiles(cu_win.data(), (int)cu_win.size() - 1, tw, n);
    int* tf = tw + 4 * ntw;
    int max_win = 0;  // longest window segment (64 tokens for 112-px windows of 14-px patches)
    for (size_t i = 1; i < cu_win.size(); ++i) max_win = std::max(max_win, cu_win[i] - cu_win[i - 1]);
    // (the full-attention blocks: segments of a whole image -- 128-query tiles, two per wave; ze_tune knob 1 = 9: 64)
    const int bq_full = ze_gemv_knobs[1] == 9 ? 64 : ZE_FA_BQ_LONG;
    const int ntf = build_tiles(cu_full.data(), (int)cu_full.size() - 1, tf, n, bq_full);
    if (ntw < 0 || ntf < 0) return ze_fail(e, ZE_ERR_NOMEM, "attention tile list overflow");
    // rotary: inv_freq over dim = head_dim/2 -> half/2 frequencies per axis (HF:...:125-134, 441-446)
    const int nf = half / 2;
    std::vector<float> invf(nf);
    for (int i = 0; i < nf; ++i) invf[i] = 1.0f / powf(10000.0f, (float)(2 * i) / (float)half);
    float* hc = e->v_host_f32;
    float* hs = hc + (size_t)n * half;
    for (int r = 0; r < n; ++r) {
        const int old = perm[r];
        for (int i = 0; i < nf; ++i) {
            const float fh = (float)hw[2 * old] * invf[i], fw = (float)hw[2 * old + 1] * invf[i];
            hc[(size_t)r * half + i] = cosf(fh);
            hs[(size_t)r * half + i] = sinf(fh);
            hc[(size_t)r * half + nf + i] = cosf(fw);
            hs[(size_t)r * half + nf + i] = sinf(fw);
        }
    }
    ZE_HIP(hipMemcpyAsync(e->vperm, perm, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    ZE_HIP(hipMemcpyAsync(e->vinv, inv, (size_t)(n / mu) * sizeof(int), hipMemcpyHostToDevice, s));
    ZE_HIP(hipMemcpyAsync(e->vtiles_win, tw, (size_t)ntw * 16, hipMemcpyHostToDevice, s));
    ZE_HIP(hipMemcpyAsync(e->vtiles_full, tf, (size_t)ntf * 16, hipMemcpyHostToDevice, s));
    ZE_HIP(hipMemcpyAsync(e->vcos, hc, (size_t)n * half * sizeof(float), hipMemcpyHostToDevice, s));
    ZE_HIP(hipMemcpyAsync(e->vsin, hs, (size_t)n * half * sizeof(float), hipMemcpyHostToDevice, s));
    ZE_TRY(stage_release(e, e->v_staged, s));

    const int th = ze_timer_begin(e, 1, s);
    // ---- patch embed on window-ordered rows (pixel_values.type(bf16), conv3d == GEMM, no bias)
    ze_launch_gather_cast_rows(pixel_values, pk, e->vperm, e->vx, pk, n, s);
    ze_launch_gemm(ZE_EPI_NONE, e->vx, pk, e->patch_embed.w, e->patch_embed.ld, nullptr, nullptr, 0, e->vh, vh,
                   nullptr, n, vh, pk, s);
    const float scale = 1.0f / sqrtf((float)hd);
    for (int li = 0; li < c.vit_depth; ++li) {
        const ze_vit_block& b = e->vb[li];
        bool full = false;
        for (int k = 0; k < c.n_fullatt; ++k) full |= c.fullatt_block_indexes[k] == li;
        ze_launch_rmsnorm(e->vh, vh, b.norm1, e->vy, vh, n, vh, 1e-6f, s);
        ze_launch_gemm(ZE_EPI_NONE, e->vy, vh, b.qkv.w, b.qkv.ld, b.qkv.bias, nullptr, 0, e->vqkv, 3 * vh, nullptr, n,
                       3 * vh, vh, s);
        ze_launch_vision_rope(e->vqkv, e->vcos, e->vsin, n, nh, hd, s);
        ze_launch_flash_attn(hd, 0, e->vqkv, 3 * vh, hd, e->vqkv + vh, 3 * vh, hd, e->vqkv + 2 * vh, 3 * vh, hd, e->vo,
                             vh, hd, full ? e->vtiles_full : e->vtiles_win, full ? ntf : ntw, nh, 1, scale, 0, s, nullptr, 0,
                             full ? bq_full : 64, full ? 0 : max_win);
        ze_launch_gemm(ZE_EPI_RESIDUAL, e->vo, vh, b.proj.w, b.proj.ld, b.proj.bias, e->vh, vh, e->vh, vh, nullptr, n,
                       vh, vh, s);
        ze_launch_rmsnorm(e->vh, vh, b.norm2, e->vy, vh, n, vh, 1e-6f, s);
        ze_launch_gemm(ZE_EPI_SWIGLU, e->vy, vh, b.gate_up.w, b.gate_up.ld, b.gate_up.bias, nullptr, 0, e->va,
                       e->vit_ipad, nullptr, n, 2 * e->vit_ipad, vh, s);
        ze_launch_gemm(ZE_EPI_RESIDUAL, e->va, e->vit_ipad, b.down.w, b.down.ld, b.down.bias, e->vh, vh, e->vh, vh,
                       nullptr, n, vh, e->vit_ipad, s);
    }
    // ---- merger: RMSNorm -> [n/mu, vh*mu] -> Linear+GELU -> Linear, rows scattered back to HF order
    ze_launch_rmsnorm(e->vh, vh, e->ln_q, e->vy, vh, n, vh, 1e-6f, s);
    const int mh = vh * mu;
    ze_launch_gemm(ZE_EPI_GELU, e->vy, mh, e->merger0.w, e->merger0.ld, e->merger0.bias, nullptr, 0, e->vz, mh, nullptr,
                   n / mu, mh, mh, s);
    ze_launch_gemm(ZE_EPI_NONE, e->vz, mh, e->merger2.w, e->merger2.ld, e->merger2.bias, nullptr, 0,
                   (bf16_t*)out_embeds, c.vit_out_hidden, e->vinv, n / mu, c.vit_out_hidden, mh, s);
    ze_timer_end(e, th, s);
    ZE_KCHECK();
    return ZE_OK;
}

// ================================================================== chains
// ---- shared-prefix hints (ze_engine::pfx_host / pfx_dev; the ownership rule is stated in ze_engine.h)
static void set_prefix_hint(ze_engine* e, int seq, int value) { e->pfx_host[seq] = value; }
// the K/V rows chain `d` copied (ze_seq_copy_prefix) have landed: nothing recorded, or the event behind the copy is over
static bool prefix_copy_done(ze_engine* e, int d) {
    hipEvent_t ev = e->pfx_copy_ev[d];
    return !ev || hipEventQuery(ev) == hipSuccess;
}
// rows below `keep` of chain `seq` are about to change (or the chain is over): chains that read their prefix from it move to
// the one among them with the longest prefix WHOSE COPY HAS LANDED (its own rows hold the same bits), which goes back to reading
// its own rows; readers it does not cover -- and all of them when no copy has landed yet -- go back to their own rows as well
// (a chain joins a decode step only behind its own prefill pass, so its own rows are always good by then)
void prefix_source_gone(ze_engine* e, int seq, int keep) {
    int leader = -1, lead_p = 0;
    const int n = (int)e->pfx_host.size();
    for (int d = 0; d < n; ++d) {
        const int h = e->pfx_host[d];
        if (h != 0 && (h >> 16) == seq && (h & 0xffff) > keep && (h & 0xffff) > lead_p && prefix_copy_done(e, d))
            leader = d, lead_p = h & 0xffff;
    }
    for (int d = 0; d < n; ++d) {
        const int h = e->pfx_host[d];
        if (h == 0 || (h >> 16) != seq || (h & 0xffff) <= keep) continue;
        const int p = h & 0xffff;
        set_prefix_hint(e, d, (leader < 0 || d == leader || p > lead_p) ? 0 : ((leader << 16) | p));
    }
}
// Before a batched decode step is enqueued on `s`: the device words of ITS chains follow the host's (the one place pfx_dev is
// written, on the one stream that reads it)
void sync_prefix(ze_engine* e, const int32_t* seqs, int n, hipStream_t s) {
    int idx[64], val[64], m = 0;
    for (int i = 0; i < n; ++i) {
        const int q = seqs[i];
        const int want = (e->prefix_hints && ze_gemv_knobs[17] != 1) ? e->pfx_host[q] : 0;
        if (e->pfx_pushed[q] == want) continue;
        e->pfx_pushed[q] = want;
        idx[m] = q, val[m] = want;
        if (++m == 64) ze_launch_scatter_ints(e->pfx_dev, idx, val, m, s), m = 0;
    }
    if (m) ze_launch_scatter_ints(e->pfx_dev, idx, val, m, s);
}

int push_state(ze_engine* e, int seq, hipStream_t s, int token, int n_gen, int finished) {
    ze_seq_dev st;
    memset(&st, 0, sizeof(st));
    st.ctx = e->ctx_host[seq];
    st.rope_delta = e->delta_host[seq];
    st.token = token;
    st.finished = finished;
    st.n_gen = n_gen;
    st.max_gen = e->cfg.max_ctx;
    st.split = e->split_host[seq];
    static_assert(sizeof(ze_seq_dev) == 8 * sizeof(int), "chain state is eight ints");
    ze_launch_set_ints(reinterpret_cast<int*>(e->st_dev + seq), reinterpret_cast<const int*>(&st), 8, s);
    return ZE_OK;
}

extern "C" int ze_seq_reset(ze_engine* e, int seq, void* stream) {
    ZE_TRY(check_seq(e, seq));
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    e->ctx_host[seq] = 0;
    e->delta_host[seq] = 0;
    e->split_host[seq] = 0;
    e->logits_fresh[seq] = 0;
    prefix_source_gone(e, seq, 0);
    e->pfx_host[seq] = 0;
    ZE_HIP(hipMemsetAsync(e->seen + (size_t)seq * e->cfg.vocab, 0, e->cfg.vocab, s));
    ze_requests_clear(e, seq, s);
    return push_state(e, seq, s, 0, 0, 0);
}

// The chain in `seq` is over and its slot may be given to another chain: no decode step ENQUEUED after this call reads a prefix
// from it (the step pushes the changed hints on its own stream first: sync_prefix).  The caller orders the call behind the
// steps already in flight that may still read the slot's rows -- a scheduler calls it between bursts -- before it lets anything
// overwrite them.  `stream` is unused since round 4 (kept for the ABI): hints are host state until a decode step picks them up.
extern "C" int ze_seq_retire(ze_engine* e, int seq, void* stream) {
    (void)stream;
    ZE_TRY(check_seq(e, seq));
    prefix_source_gone(e, seq, 0);
    set_prefix_hint(e, seq, 0);
    return ZE_OK;
}

// Declares that the first `rows` cached tokens of `seq` hold the same bits as the source chain's (the caller's knowledge: a
// prefix it wrote to both; ze_seq_copy_prefix records this by itself).  rows = 0 clears.  Also the measurement hook of
// bench.py / tools/pmc_kernel.py: the decode attention timed with the sharing the question stream has.
extern "C" int ze_seq_set_prefix_hint(ze_engine* e, int seq, int src_seq, int rows, void* stream) {
    (void)stream;
    ZE_TRY(check_seq(e, seq));
    if (rows <= 0 || src_seq == seq) {
        set_prefix_hint(e, seq, 0);
        return ZE_OK;
    }
    ZE_TRY(check_seq(e, src_seq));
    if (rows > e->ctx_host[seq] || rows > e->ctx_host[src_seq] || rows >= 65536 || !e->prefix_hints)
        return ze_fail(e, ZE_ERR_INVALID, "prefix hint: rows exceed a chain's context (or hints are switched off)");
    set_prefix_hint(e, seq, (src_seq << 16) | rows);
    return ZE_OK;
}

// (source chain << 16) | rows: where the decode attention reads the first rows of `seq` from; 0 = its own cache
// Measurement / test entry: declares row `rows` the chain's split row (what prefilling tokens with an image block does by itself,
// note_split) -- for chains built from text ids that stand in for image prompts (tools/pmc_kernel.py, bench.py's annex, tests).
extern "C" int ze_seq_set_split(ze_engine* e, int seq, int rows, void* stream) {
    ZE_TRY(check_seq(e, seq));
    if (rows < 0 || rows > e->ctx_host[seq] || rows >= 65536) return ze_fail(e, ZE_ERR_INVALID, "split row out of range");
    hipSetDevice(e->device);
    e->split_host[seq] = rows;
    ze_launch_set_ints(&(e->st_dev + seq)->split, &rows, 1, (hipStream_t)stream);
    return ZE_OK;
}

extern "C" int ze_seq_prefix_hint(ze_engine* e, int seq) {
    if (check_seq(e, seq) != 0) return ZE_ERR_NOTFOUND;
    return e->pfx_host[seq];
}

extern "C" int ze_seq_truncate(ze_engine* e, int seq, int keep_len, void* stream) {
    ZE_TRY(check_seq(e, seq));
    if (keep_len < 0 || keep_len > e->ctx_host[seq]) return ze_fail(e, ZE_ERR_INVALID, "keep_len out of range");
    hipSetDevice(e->device);
    e->ctx_host[seq] = keep_len;
    e->logits_fresh[seq] = 0;
    if (keep_len < e->split_host[seq]) e->split_host[seq] = 0;   // (the image block itself is cut: the rest is a chain without one)
    prefix_source_gone(e, seq, keep_len);   // rows from keep_len on will be rewritten
    if ((e->pfx_host[seq] & 0xffff) > keep_len) e->pfx_host[seq] = 0;
    // the seen-set belongs to the dropped continuation: the caller re-marks the (new) prompt
    ZE_HIP(hipMemsetAsync(e->seen + (size_t)seq * e->cfg.vocab, 0, e->cfg.vocab, (hipStream_t)stream));
    ze_requests_clear(e, seq, (hipStream_t)stream);
    return push_state(e, seq, (hipStream_t)stream, 0, 0, 0);
}

extern "C" int ze_seq_copy_prefix(ze_engine* e, int dst_seq, int src_seq, int n_tokens, void* stream) {
    ZE_TRY(check_seq(e, dst_seq));
    ZE_TRY(check_seq(e, src_seq));
    if (dst_seq == src_seq) return ze_fail(e, ZE_ERR_INVALID, "source and destination chain are the same");
    if (n_tokens <= 0 || n_tokens > e->ctx_host[src_seq]) return ze_fail(e, ZE_ERR_INVALID, "n_tokens exceeds the source chain's context");
    const ze_config& c = e->cfg;
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t head_stride = (size_t)c.max_ctx * e->head_dim, seq_stride = (size_t)c.kv_heads * head_stride;
    ze_launch_kv_copy_prefix(e->kcache, e->vcache, (size_t)c.max_seqs * seq_stride, seq_stride, head_stride, c.layers, c.kv_heads,
                             e->head_dim, src_seq, dst_seq, n_tokens, s);
    ZE_KCHECK();
    e->ctx_host[dst_seq] = n_tokens;
    e->delta_host[dst_seq] = 0;
    e->logits_fresh[dst_seq] = 0;
    // the split row travels with the rows: the copy holds the source's first image block iff it reaches past its end (the same
    // tokens, the same split -- however a chain came by its rows)
    e->split_host[dst_seq] = (e->split_host[src_seq] > 0 && e->split_host[src_seq] <= n_tokens) ? e->split_host[src_seq] : 0;
    prefix_source_gone(e, dst_seq, 0);
    if (!e->pfx_copy_ev[dst_seq]) ZE_HIP(hipEventCreateWithFlags(&e->pfx_copy_ev[dst_seq], hipEventDisableTiming));
    ZE_HIP(hipEventRecord(e->pfx_copy_ev[dst_seq], s));  // (a holder other chains may be pointed at only once this is over)
    // the copy stays (the prefill attention of a later pass reads the chain's own rows); the decode attention reads the
    // source's -- or the source's own source, when that one covers these rows
    {
        int src = src_seq;
        const int hs = e->pfx_host[src_seq];
        if (hs != 0 && (hs & 0xffff) >= n_tokens) src = hs >> 16;
        e->pfx_host[dst_seq] = (e->prefix_hints && n_tokens < 65536 && src != dst_seq) ? ((src << 16) | n_tokens) : 0;
    }
    ZE_HIP(hipMemsetAsync(e->seen + (size_t)dst_seq * c.vocab, 0, c.vocab, s));
    ze_requests_clear(e, dst_seq, s);
    return push_state(e, dst_seq, s, 0, 0, 0);
}

// The whole chain `src_seq`, n times (include/zoomearth.h): validation first -- after an error nothing was enqueued or changed --
// then the destination table, ONE launch of k_kv_fork (ze_fork.hip: K/V rows, logits row, seen-set), and per destination the host
// state ze_seq_copy_prefix keeps, with the rope delta and the prompt's last id handed on (no prefill follows).
extern "C" int ze_seq_fork(ze_engine* e, int src_seq, const int32_t* dst_seqs, int n, void* stream) {
    ZE_TRY(check_seq(e, src_seq));
    if (!dst_seqs || n <= 0) return ze_fail(e, ZE_ERR_INVALID, "fork needs a table of n > 0 destination chains");
    for (int i = 0; i < n; ++i) {
        ZE_TRY(check_seq(e, dst_seqs[i]));
        if (dst_seqs[i] == src_seq) return ze_fail(e, ZE_ERR_INVALID, "source and destination chain are the same");
        for (int j = 0; j < i; ++j)
            if (dst_seqs[j] == dst_seqs[i]) return ze_fail(e, ZE_ERR_INVALID, "a destination chain appears twice");
    }
    const int rows = e->ctx_host[src_seq];
    if (rows <= 0) return ze_fail(e, ZE_ERR_INVALID, "the source chain is empty");
    if (!e->logits_fresh[src_seq])
        return ze_fail(e, ZE_ERR_INVALID, "the source chain's logits are not those of its last row (it drew, stepped or changed since its prefill)");
    if (n > e->prefill_rows) return ze_fail(e, ZE_ERR_NOMEM, "more destinations than the id buffer holds");
    const ze_config& c = e->cfg;
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    // the destination slots travel as kernel arguments into the prefill's id buffer, in stream order behind whatever still reads it
    // (ze_seq_mark_seen's way: no allocation, no staging buffer to wait for)
    ze_launch_set_ints(e->tsrc, dst_seqs, n, s);
    const size_t head_stride = (size_t)c.max_ctx * e->head_dim, seq_stride = (size_t)c.kv_heads * head_stride;
    ze_launch_kv_fork(e->kcache, e->vcache, (size_t)c.max_seqs * seq_stride, seq_stride, head_stride, c.layers, c.kv_heads, e->head_dim,
                      src_seq, e->tsrc, n, rows, e->dlogits, e->seen, c.vocab, s);
    ZE_KCHECK();
    // the decode attention reads the prompt from the source -- or the source's own holder, when that one covers the rows (the rule
    // of ze_seq_copy_prefix): one copy of the prompt is streamed for all siblings
    // (looked up per destination, behind prefix_source_gone: a destination that WAS the source's holder is none afterwards)
    for (int i = 0; i < n; ++i) {
        const int d = dst_seqs[i];
        e->ctx_host[d] = rows;
        e->delta_host[d] = e->delta_host[src_seq];
        e->split_host[d] = e->split_host[src_seq];
        e->tok_host[d] = e->tok_host[src_seq];
        e->logits_fresh[d] = 1;
        prefix_source_gone(e, d, 0);
        if (!e->pfx_copy_ev[d]) ZE_HIP(hipEventCreateWithFlags(&e->pfx_copy_ev[d], hipEventDisableTiming));
        ZE_HIP(hipEventRecord(e->pfx_copy_ev[d], s));  // (a holder other chains may be pointed at only once this is over)
        const int hs = e->pfx_host[src_seq];
        const int holder = (hs != 0 && (hs & 0xffff) >= rows) ? (hs >> 16) : src_seq;
        e->pfx_host[d] = (e->prefix_hints && rows < 65536 && holder != d) ? ((holder << 16) | rows) : 0;
        ze_requests_clear(e, d, s);
        ZE_TRY(push_state(e, d, s, e->tok_host[d], 0, 0));
    }
    return ZE_OK;
}

extern "C" int ze_seq_len(ze_engine* e, int seq) {
    if (check_seq(e, seq) != 0) return ZE_ERR_NOTFOUND;
    return e->ctx_host[seq];
}

extern "C" int ze_seq_mark_seen(ze_engine* e, int seq, const int32_t* ids, int n, void* stream) {
    ZE_TRY(check_seq(e, seq));
    if (n < 0 || (n > 0 && !ids)) return ze_fail(e, ZE_ERR_INVALID, "bad ids");
    if ((size_t)n > e->t_host_ints_cap) return ze_fail(e, ZE_ERR_NOMEM, "too many ids");
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= e->cfg.vocab) return ze_fail(e, ZE_ERR_INVALID, "token id out of range");
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    // the ids travel as kernel arguments (128 per launch) into the prefill's id buffer, in stream order behind whatever still
    // reads it: no pinned staging buffer to wait for -- the stream synchronisation this call used to begin with made the
    // scheduler wait for its whole prefill pass once per request (2.1 ms per call on the real entry point)
    ze_launch_set_ints(e->tsrc, ids, n, s);
    ze_launch_mark_seen(e->seen + (size_t)seq * e->cfg.vocab, e->tsrc, n, s);
    ZE_KCHECK();
    return ZE_OK;
}

// pinned + device scratch of the batched id transfers, sized by the REQUEST and grown on demand (max_seqs x max_ctx ints per
// direction were ~100 MB four times over at 768 slots x 32 K context, for calls that move a few hundred KB): `need` ints, rounded up
// to the next power of two from 64 Ki ints on.  Growing waits for the work that may still read the old block (the caller's stream and
// the block's staging event), frees it, and allocates anew; a failed device allocation frees the pinned half it had just obtained.
int xfer_reserve(ze_engine* e, int*& host, int*& dev, size_t& cap, size_t need, hipEvent_t staged, hipStream_t s) {
    if (need <= cap) return ZE_OK;
    size_t want = (size_t)64 << 10;
    while (want < need) want <<= 1;
    if (cap) {
        if (staged) ZE_HIP(hipEventSynchronize(staged));
        ZE_HIP(hipStreamSynchronize(s));
        hipHostFree(host);
        hipFree(dev);
        host = dev = nullptr;
        cap = 0;
    }
    int *h = nullptr, *d = nullptr;
    ZE_HIP(hipHostMalloc((void**)&h, want * sizeof(int)));
    if (hipMalloc((void**)&d, want * sizeof(int)) != hipSuccess) {
        hipHostFree(h);
        return ze_fail(e, ZE_ERR_NOMEM, "hipMalloc of the id transfer scratch failed");
    }
    host = h;
    dev = d;
    cap = want;
    return ZE_OK;
}

// ze_seq_mark_seen for the n chains of a prefill pass at once: ONE host -> device copy and ONE launch instead of ~10 launches per
// chain (the scheduler's thread spent 1.4 ms per chain in the single-chain call on a busy GPU: 1.8 s per lane of the 15-s stream)
extern "C" int ze_seq_mark_seen_batch(ze_engine* e, const int32_t* seqs, const int32_t* counts, int n, const int32_t* ids, void* stream) {
    if (!e || n < 0 || (n > 0 && (!seqs || !counts))) return ze_fail(e, ZE_ERR_INVALID, "bad arguments");
    if (n == 0) return ZE_OK;
    if (n > e->cfg.max_seqs) return ze_fail(e, ZE_ERR_INVALID, "more chains than slots");
    size_t total = 0;
    int max_count = 0;
    for (int i = 0; i < n; ++i) {
        ZE_TRY(check_seq(e, seqs[i]));
        if (counts[i] < 0 || counts[i] > e->cfg.max_ctx) return ze_fail(e, ZE_ERR_INVALID, "bad id count");
        total += (size_t)counts[i];
        max_count = std::max(max_count, counts[i]);
    }
    if (total > 0 && !ids) return ze_fail(e, ZE_ERR_INVALID, "bad ids");
    for (size_t i = 0; i < total; ++i)
        if (ids[i] < 0 || ids[i] >= e->cfg.vocab) return ze_fail(e, ZE_ERR_INVALID, "token id out of range");
    if (total == 0) return ZE_OK;
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    // (the event is recorded BEHIND the kernel that reads the device block -- ADVICE r5: behind the copy alone, a second call on
    //  another stream could have overwritten xs_dev under the first call's kernel; acquire waits for that kernel now)
    ZE_TRY(stage_acquire(e, e->xs_staged));
    ZE_TRY(xfer_reserve(e, e->xs_host, e->xs_dev, e->xs_cap, (size_t)(2 * n + 1) + total, e->xs_staged, s));
    int* h = e->xs_host;
    h[0] = 0;
    for (int i = 0; i < n; ++i) {
        h[i + 1] = h[i] + counts[i];
        h[n + 1 + i] = seqs[i];
    }
    memcpy(h + 2 * n + 1, ids, total * sizeof(int));
    ZE_HIP(hipMemcpyAsync(e->xs_dev, h, ((size_t)(2 * n + 1) + total) * sizeof(int), hipMemcpyHostToDevice, s));
    ze_launch_mark_seen_batch(e->seen, e->cfg.vocab, e->xs_dev, e->xs_dev + 2 * n + 1, n, max_count, s);
    ZE_KCHECK();
    ZE_TRY(stage_release(e, e->xs_staged, s));
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
    if (e->fp8_act && lin.w8 && ze_gemv_knobs[12] != 1 && H % 128 == 0 && H >= 256 && lin.ld8 % 16 == 0) {
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
static int prefill_bq() { return (ze_gemv_knobs[1] == 9 || ze_gemv_knobs[1] == 7) ? 64 : ZE_FA_BQ_LONG; }

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
    const bool q_in_flash = hd == 128 && ze_mrope_vec_ok != 0 && ze_gemv_knobs[22] != 1;
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
static void launch_step_attention(ze_engine* e, int li, int seq, hipStream_t s, const bf16_t* q_row = nullptr, bf16_t* out_row = nullptr) {
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
    const bool folded = sample && so.temperature <= 0.f && ze_gemv_knobs[14] != 1 && !e->req.la_host[seq].on() && !e->req.tr_host[seq].bans() &&
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

// The selection alone, on caller-supplied rows (unit op: any vocab / ld, a filter and a temperature per row, no repetition penalty)
extern "C" int ze_op_sample_filter(ze_engine* e, const float* logits, int rows, int vocab, int ld, const float* temperature,
                                   const int32_t* top_k, const float* top_p, const float* min_p, float* out_cut,
                                   int32_t* out_kept, void* stream) {
    if (!e || !logits || !temperature || !top_k || !top_p || !min_p || !out_cut) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (rows <= 0 || vocab <= 0 || ld < vocab) return ze_fail(e, ZE_ERR_INVALID, "rows and vocab must be positive, ld >= vocab");
    std::vector<float> table((size_t)rows * 4);
    for (int r = 0; r < rows; ++r) {
        if (!(temperature[r] > 0.f)) return ze_fail(e, ZE_ERR_INVALID, "temperature must be positive");
        ZE_TRY(ze_check_filter(e, top_k[r], top_p[r], min_p[r]));
        memcpy(&table[4 * r], &top_k[r], sizeof(int));
        table[4 * r + 1] = top_p[r];
        table[4 * r + 2] = min_p[r];
        table[4 * r + 3] = temperature[r];
    }
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    float* dev = nullptr;
    ZE_HIP(hipMalloc((void**)&dev, table.size() * sizeof(float)));
    int r = ZE_OK;
    if (hipMemcpyAsync(dev, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess)
        r = ze_fail(e, ZE_ERR_HIP, "hipMemcpyAsync failed");
    if (r == ZE_OK) ze_launch_sample_filter(logits, vocab, ld, nullptr, nullptr, 0, rows, 1.0f, 1.0f, dev, out_cut, out_kept, nullptr, s);
    if (r == ZE_OK && hipGetLastError() != hipSuccess) r = ze_fail(e, ZE_ERR_HIP, "selection kernel launch failed");
    if (hipStreamSynchronize(s) != hipSuccess && r == ZE_OK) r = ze_fail(e, ZE_ERR_HIP, "hipStreamSynchronize failed");
    hipFree(dev);
    return r;
}

// One draw per caller row with a (temperature | greedy, penalty, seed, stream, index) of its own: the per-chain kernels of
// ze_sample.hip with row = slot, on tables built for the call
static int op_sample_rows(ze_engine* e, const float* logits, int rows, int vocab, int ld, const uint8_t* seen,
                          const float* temperature, const float* repetition_penalty, const uint64_t* seed,
                          const int32_t* sample_stream, const int32_t* index, const int32_t* top_k, const float* top_p,
                          const float* min_p, const float* band_cut, const float* band_ceil, int32_t* out_tokens, void* stream) {
    if (!e || !logits || !temperature || !repetition_penalty || !seed || !sample_stream || !index || !out_tokens)
        return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (rows <= 0 || vocab <= 0 || ld < vocab) return ze_fail(e, ZE_ERR_INVALID, "rows and vocab must be positive, ld >= vocab");
    const bool filters = top_k || top_p || min_p;
    if (filters && !(top_k && top_p && min_p)) return ze_fail(e, ZE_ERR_INVALID, "top_k, top_p and min_p come together or not at all");
    // one block of 4-byte words: requests (4 per row) | chain states (8) | filters (4) | row ids (1) | cuts (1) | ceilings (1) |
    // arg-max partials (256) | chunk sums (128); the 16-byte entries come first, so they stay aligned
    const size_t o_samp = 0, o_st = o_samp + 4 * (size_t)rows, o_filt = o_st + 8 * (size_t)rows, o_ids = o_filt + 4 * (size_t)rows,
                 o_cut = o_ids + rows, o_ceil = o_cut + rows, o_part = o_ceil + rows, o_sum = o_part + 256 * (size_t)rows,
                 words = o_sum + 128 * (size_t)rows;
    static_assert(sizeof(ze_chain_sampling) == 16 && sizeof(ze_seq_dev) == 32, "table strides");
    std::vector<int32_t> host(o_part, 0);
    bool draws = false;
    for (int r = 0; r < rows; ++r) {
        if (!(std::isfinite(temperature[r]) && temperature[r] >= 0.f)) return ze_fail(e, ZE_ERR_INVALID, "temperature must be finite and >= 0 (0 = greedy)");
        if (!(std::isfinite(repetition_penalty[r]) && repetition_penalty[r] > 0.f))
            return ze_fail(e, ZE_ERR_INVALID, "repetition_penalty must be finite and > 0 (1 = off)");
        if (index[r] < 0) return ze_fail(e, ZE_ERR_INVALID, "index must be >= 0");
        const ze_chain_sampling req{temperature[r], repetition_penalty[r], temperature[r] > 0.f ? (unsigned long long)seed[r] : 0ull};
        memcpy(&host[o_samp + 4 * (size_t)r], &req, sizeof(req));
        draws |= temperature[r] > 0.f;
        ze_seq_dev st;
        memset(&st, 0, sizeof(st));
        st.n_gen = index[r];
        st.stream = sample_stream[r];
        memcpy(&host[o_st + 8 * (size_t)r], &st, sizeof(st));
        host[o_ids + r] = r;
        if (filters) {
            ZE_TRY(ze_check_filter(e, top_k[r], top_p[r], min_p[r]));
            host[o_filt + 4 * (size_t)r] = top_k[r];
            memcpy(&host[o_filt + 4 * (size_t)r + 1], &top_p[r], sizeof(float));
            memcpy(&host[o_filt + 4 * (size_t)r + 2], &min_p[r], sizeof(float));
        }
        if (band_cut) {  // the caller's band [cut, ceil] of the row, z = score / temperature
            if (std::isnan(band_cut[r]) || std::isnan(band_ceil[r])) return ze_fail(e, ZE_ERR_INVALID, "a band is two numbers (-inf / +inf = open)");
            memcpy(&host[o_cut + r], &band_cut[r], sizeof(float));
            memcpy(&host[o_ceil + r], &band_ceil[r], sizeof(float));
        }
    }
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    int32_t* dev = nullptr;
    ZE_HIP(hipMalloc((void**)&dev, words * sizeof(int32_t)));
    int r = ZE_OK;
    if (hipMemcpyAsync(dev, host.data(), host.size() * sizeof(int32_t), hipMemcpyHostToDevice, s) != hipSuccess)
        r = ze_fail(e, ZE_ERR_HIP, "hipMemcpyAsync failed");
    if (r == ZE_OK)
        ze_launch_sample_rows(logits, vocab, ld, seen, reinterpret_cast<const ze_seq_dev*>(dev + o_st), dev + o_ids, rows,
                              reinterpret_cast<const ze_chain_sampling*>(dev + o_samp), draws,
                              filters ? reinterpret_cast<const float*>(dev + o_filt) : nullptr,
                              filters || band_cut ? reinterpret_cast<float*>(dev + o_cut) : nullptr,
                              band_cut ? reinterpret_cast<float*>(dev + o_ceil) : nullptr, reinterpret_cast<float*>(dev + o_part), reinterpret_cast<float*>(dev + o_sum), out_tokens, s);
    if (r == ZE_OK && hipGetLastError() != hipSuccess) r = ze_fail(e, ZE_ERR_HIP, "sampling kernel launch failed");
    if (hipStreamSynchronize(s) != hipSuccess && r == ZE_OK) r = ze_fail(e, ZE_ERR_HIP, "hipStreamSynchronize failed");
    hipFree(dev);
    return r;
}

extern "C" int ze_op_sample_rows(ze_engine* e, const float* logits, int rows, int vocab, int ld, const uint8_t* seen,
                                 const float* temperature, const float* repetition_penalty, const uint64_t* seed,
                                 const int32_t* sample_stream, const int32_t* index, const int32_t* top_k, const float* top_p,
                                 const float* min_p, int32_t* out_tokens, void* stream) {
    return op_sample_rows(e, logits, rows, vocab, ld, seen, temperature, repetition_penalty, seed, sample_stream, index, top_k, top_p,
                          min_p, nullptr, nullptr, out_tokens, stream);
}

// ... under a band per row as ze_op_sample_band (or anyone) found it: the _band draw kernels alone
extern "C" int ze_op_sample_rows_band(ze_engine* e, const float* logits, int rows, int vocab, int ld, const uint8_t* seen,
                                      const float* temperature, const float* repetition_penalty, const uint64_t* seed,
                                      const int32_t* sample_stream, const int32_t* index, const float* cut, const float* ceil,
                                      int32_t* out_tokens, void* stream) {
    if (!cut || !ceil) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    return op_sample_rows(e, logits, rows, vocab, ld, seen, temperature, repetition_penalty, seed, sample_stream, index, nullptr,
                          nullptr, nullptr, cut, ceil, out_tokens, stream);
}

// The whole warper chain's selection alone, on caller-supplied rows (unit op: the filter of every row, then its band)
extern "C" int ze_op_sample_band(ze_engine* e, const float* logits, int rows, int vocab, int ld, const float* temperature,
                                 const int32_t* top_k, const float* top_p, const float* min_p, const float* typical_p,
                                 const float* epsilon_cutoff, const float* eta_cutoff, float* out_cut, float* out_ceil,
                                 int32_t* out_kept, void* stream) {
    if (!e || !logits || !temperature || !top_k || !top_p || !min_p || !typical_p || !epsilon_cutoff || !eta_cutoff || !out_cut || !out_ceil)
        return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (rows <= 0 || vocab <= 0 || ld < vocab) return ze_fail(e, ZE_ERR_INVALID, "rows and vocab must be positive, ld >= vocab");
    std::vector<float> table((size_t)rows * 8);  // the filter table, then the entropy-filter table
    for (int r = 0; r < rows; ++r) {
        if (!(temperature[r] > 0.f)) return ze_fail(e, ZE_ERR_INVALID, "temperature must be positive");
        ZE_TRY(ze_check_filter(e, top_k[r], top_p[r], min_p[r]));
        ZE_TRY(ze_check_entropy_filter(e, typical_p[r], epsilon_cutoff[r], eta_cutoff[r]));
        float* f = &table[4 * (size_t)r];
        float* g = &table[4 * ((size_t)rows + r)];
        memcpy(f, &top_k[r], sizeof(int));
        f[1] = top_p[r], f[2] = min_p[r], f[3] = temperature[r];
        g[0] = typical_p[r], g[1] = epsilon_cutoff[r], g[2] = eta_cutoff[r], g[3] = temperature[r];
    }
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    float* dev = nullptr;
    ZE_HIP(hipMalloc((void**)&dev, table.size() * sizeof(float)));
    int r = ZE_OK;
    if (hipMemcpyAsync(dev, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess)
        r = ze_fail(e, ZE_ERR_HIP, "hipMemcpyAsync failed");
    if (r == ZE_OK) {
        ze_launch_sample_filter(logits, vocab, ld, nullptr, nullptr, 0, rows, 1.0f, 1.0f, dev, out_cut, out_kept, nullptr, s);
        ze_launch_sample_band(logits, vocab, ld, nullptr, nullptr, 0, rows, 1.0f, 1.0f, dev + 4 * (size_t)rows, out_cut, out_cut, out_ceil,
                              out_kept, nullptr, s);
    }
    if (r == ZE_OK && hipGetLastError() != hipSuccess) r = ze_fail(e, ZE_ERR_HIP, "selection kernel launch failed");
    if (hipStreamSynchronize(s) != hipSuccess && r == ZE_OK) r = ze_fail(e, ZE_ERR_HIP, "hipStreamSynchronize failed");
    hipFree(dev);
    return r;
}

// one sampling step on caller-supplied logits; `index` plays the role of the generated-token index of the draw
static int op_sample(ze_engine* e, int seq, const float* logits, float repetition_penalty, const ze_sample_opts& so,
                     int index, int32_t* out_token, hipStream_t s) {
    ZE_TRY(check_seq(e, seq));
    if (!logits || !out_token) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (index < 0 || index >= e->cfg.max_ctx) return ze_fail(e, ZE_ERR_INVALID, "index out of range");
    const ze_config& c = e->cfg;
    hipSetDevice(e->device);
    // n_gen is set so the sampled token lands in out_tokens[index] of this chain's slot
    e->logits_fresh[seq] = 0;
    ZE_TRY(push_state(e, seq, s, 0, 0, 0));
    if (index) ze_launch_set_ints(&(e->st_dev + seq)->n_gen, &index, 1, s);
    ze_launch_sample(logits, c.vocab, e->seen + (size_t)seq * c.vocab, repetition_penalty, e->st_dev + seq, e->eos_dev,
                     c.n_eos, c.pad_token_id, 1, 0, e->out_tokens + (size_t)seq * c.max_ctx, e->dsample, so, s);
    ze_requests_logprobs(e, logits, nullptr, seq, 1, s);
    ZE_KCHECK();
    ZE_HIP(hipMemcpyAsync(out_token, e->out_tokens + (size_t)seq * c.max_ctx + index, sizeof(int), hipMemcpyDeviceToHost, s));
    ZE_HIP(hipStreamSynchronize(s));
    return ZE_OK;
}

extern "C" int ze_op_sample_greedy(ze_engine* e, int seq, const float* logits, float repetition_penalty,
                                   int32_t* out_token, void* stream) {
    return op_sample(e, seq, logits, repetition_penalty, ze_sample_opts{}, 0, out_token, (hipStream_t)stream);
}

extern "C" int ze_op_sample_temperature(ze_engine* e, int seq, const float* logits, float repetition_penalty,
                                        float temperature, uint64_t seed, int index, int32_t* out_token, void* stream) {
    if (!(temperature > 0.f)) return ze_fail(e, ZE_ERR_INVALID, "temperature must be positive");
    ze_sample_opts so;
    so.temperature = temperature;
    so.seed = seed;
    so.slot = seq;
    if (check_seq(e, seq) == 0) ze_attach_filters(e, so, false);
    return op_sample(e, seq, logits, repetition_penalty, so, index, out_token, (hipStream_t)stream);
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

// ================================================================== unit ops
extern "C" int ze_op_logit_adjust(ze_engine* e, const float* logits, int rows, int vocab, int ld, const uint16_t* counts,
                                  const float* presence, const float* frequency, const int32_t* eos_masked, const int32_t* bias_offsets,
                                  const int32_t* bias_ids, const float* bias_vals, float* out, void* stream) {
    if (!e || !logits || !presence || !frequency || !eos_masked || !bias_offsets || !out || out == logits)
        return ze_fail(e, ZE_ERR_INVALID, "bad logit_adjust arguments");
    if (rows < 0 || vocab <= 0 || ld < vocab) return ze_fail(e, ZE_ERR_INVALID, "rows >= 0, vocab > 0 and ld >= vocab");
    hipSetDevice(e->device);
    ze_launch_logit_adjust(logits, rows, vocab, ld, counts, presence, frequency, eos_masked, bias_offsets, bias_ids, bias_vals, e->eos_dev,
                           e->cfg.n_eos, out, (hipStream_t)stream);
    ZE_KCHECK();
    return ZE_OK;
}

extern "C" int ze_op_token_rules(ze_engine* e, const float* logits, int rows, int vocab, int ld, const int32_t* hist_ids,
                                 const int32_t* hist_offsets, const int32_t* n_context, const int32_t* no_repeat_ngram,
                                 const int32_t* ban_seqs, const int32_t* ban_offsets, const int32_t* stop_seqs, const int32_t* stop_offsets,
                                 const int32_t* min_new, float* out_rows, int32_t* out_stop, void* stream) {
    if (!e || !logits || !hist_ids || !hist_offsets || !n_context || !no_repeat_ngram || !ban_seqs || !ban_offsets || !stop_seqs ||
        !stop_offsets || !min_new || !out_rows || !out_stop || out_rows == logits)
        return ze_fail(e, ZE_ERR_INVALID, "bad token_rules arguments");
    if (rows < 0 || vocab <= 0 || ld < vocab) return ze_fail(e, ZE_ERR_INVALID, "rows >= 0, vocab > 0 and ld >= vocab");
    if (rows == 0) return ZE_OK;
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    ZE_HIP(hipMemcpy2DAsync(out_rows, (size_t)ld * sizeof(float), logits, (size_t)ld * sizeof(float), (size_t)vocab * sizeof(float), rows,
                            hipMemcpyDeviceToDevice, s));
    ze_launch_token_ban(out_rows, rows, vocab, ld, hist_ids, hist_offsets, n_context, no_repeat_ngram, ban_seqs, ban_offsets, s);
    ze_launch_token_stop(rows, hist_ids, hist_offsets, n_context, stop_seqs, stop_offsets, min_new, out_stop, s);
    ZE_KCHECK();
    return ZE_OK;
}

extern "C" int ze_op_token_logprobs(ze_engine* e, const float* logits, int rows, int vocab, int ld, const int32_t* targets,
                                    int top_n, float* out_logprob, int32_t* out_top_ids, float* out_top_logprobs, void* stream) {
    if (!e || !logits || !targets || !out_logprob || rows < 0 || vocab <= 0 || ld < vocab)
        return ze_fail(e, ZE_ERR_INVALID, "bad token_logprobs arguments");
    if (top_n < 0 || top_n > ZE_MAX_TOP_LOGPROBS) return ze_fail(e, ZE_ERR_INVALID, "top_n must be in [0, 20]");
    if (top_n > 0 && (!out_top_ids || !out_top_logprobs)) return ze_fail(e, ZE_ERR_INVALID, "null top arrays");
    hipSetDevice(e->device);
    ze_launch_token_logprobs(logits, rows, vocab, ld, targets, top_n, out_logprob, out_top_ids, out_top_logprobs, (hipStream_t)stream);
    ZE_KCHECK();
    return ZE_OK;
}

extern "C" int ze_op_linear(ze_engine* e, const void* a, const void* w, const void* bias, void* cmat, int M, int N,
                            int K, int act, void* stream) {
    if (!e || !a || !w || !cmat) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (K % 8) return ze_fail(e, ZE_ERR_INVALID, "K must be a multiple of 8");
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    if (M == 1 && act == 0 && N % 2 == 0) {
        ze_gemv_args g;
        memset(&g, 0, sizeof(g));
        g.W = (const bf16_t*)w;
        g.ldw = K;
        g.N = N;
        g.K = K;
        g.x = (const bf16_t*)a;
        g.bias = (const bf16_t*)bias;
        g.out_bf16 = (bf16_t*)cmat;
        g.D = 128;
        if (!ze_launch_gemv(ZE_GV_PLAIN, g, s))
            ze_launch_gemm(ZE_EPI_NONE, (const bf16_t*)a, K, (const bf16_t*)w, K, (const bf16_t*)bias, nullptr, 0,
                           (bf16_t*)cmat, N, nullptr, M, N, K, s);
    } else if (act == 3 || act == 5) {  // the fragment-major kernels of the batched decode step, operands packed here
        if (M > 64 || N % 16 || K % 32 || K > 4096) return ze_fail(e, ZE_ERR_INVALID, "fragment path: M <= 64, N % 16, K % 32, K <= 4096");
        bf16_t *wf = nullptr, *xf = nullptr;
        const size_t mp = M <= 16 ? 16 : M <= 32 ? 32 : 64;  // the kernels read whole 16-row tiles: 1, 2 or 4 of them (dispatch_mt)
        ZE_HIP(hipMalloc((void**)&wf, ((size_t)N * K + mp * K) * sizeof(bf16_t)));
        xf = wf + (size_t)N * K;
        ze_launch_pack_fragments((const bf16_t*)w, K, N, K, wf, s);
        ze_launch_pack_fragments((const bf16_t*)a, K, M, K, xf, s);
        if (act == 5)  // the sixteen-wave one-shot kernel (qkv / o projections)
            ze_launch_gemm_oneshot(ZE_EPI_NONE, xf, wf, (const bf16_t*)bias, nullptr, 0, (bf16_t*)cmat, N, M, N, K, s);
        else
            ze_launch_gemm_frag(ZE_EPI_NONE, xf, wf, (const bf16_t*)bias, nullptr, 0, (bf16_t*)cmat, N, M, N, K, s);
        hipStreamSynchronize(s);
        hipFree(wf);
    } else if (act == 4) {  // SwiGLU epilogue on interleaved gate/up rows: C is [M, N/2]
        if (N % 32) return ze_fail(e, ZE_ERR_INVALID, "SwiGLU: N = 2 * width with width % 16 == 0");
        ze_launch_gemm(ZE_EPI_SWIGLU, (const bf16_t*)a, K, (const bf16_t*)w, K, (const bf16_t*)bias, nullptr, 0,
                       (bf16_t*)cmat, N / 2, nullptr, M, N, K, s, e->prefill_ws());
    } else if (act == 6 || act == 7) {  // the launcher of the row-streaming decode regime (7: SwiGLU, C is [M, N/2])
        if (act == 7 && N % 32) return ze_fail(e, ZE_ERR_INVALID, "SwiGLU: N = 2 * width with width % 16 == 0");
        ze_launch_gemm_wide(act == 7 ? ZE_EPI_SWIGLU : ZE_EPI_NONE, (const bf16_t*)a, K, (const bf16_t*)w, K, (const bf16_t*)bias,
                            nullptr, 0, (bf16_t*)cmat, act == 7 ? N / 2 : N, M, N, K, e->gemm_ws(), s);
    } else if (act == 10) {  // the lm_head of the row-streaming regime: fp32 output [M, N] through ze_launch_gemm_wide
        ze_launch_gemm_wide(ZE_EPI_F32, (const bf16_t*)a, K, (const bf16_t*)w, K, nullptr, nullptr, 0, (bf16_t*)cmat, N, M, N, K,
                            e->gemm_ws(), s);
    } else if (act == 8 || act == 9) {  // the eight-phase 256 x 256 kernel whatever the grid (9: SwiGLU), for its tests
        if (act == 9 && N % 32) return ze_fail(e, ZE_ERR_INVALID, "SwiGLU: N = 2 * width with width % 16 == 0");
        if (K % 64 || K < 64) return ze_fail(e, ZE_ERR_INVALID, "eight-phase kernel: K a multiple of 64");
        ze_launch_gemm_p8(act == 9 ? ZE_EPI_SWIGLU : ZE_EPI_NONE, (const bf16_t*)a, K, (const bf16_t*)w, K, (const bf16_t*)bias, nullptr, 0,
                          (bf16_t*)cmat, act == 9 ? N / 2 : N, nullptr, M, N, K, s, e->prefill_ws());
    } else if (act == 2) {  // weight-streaming mode of the batched decode step (rows = chains), for measurements
        ze_launch_gemm_stream(ZE_EPI_NONE, (const bf16_t*)a, K, (const bf16_t*)w, K, (const bf16_t*)bias, nullptr, 0,
                              (bf16_t*)cmat, N, M, N, K, e->gemm_ws(), s);
    } else {
        ze_launch_gemm(act ? ZE_EPI_GELU : ZE_EPI_NONE, (const bf16_t*)a, K, (const bf16_t*)w, K, (const bf16_t*)bias,
                       nullptr, 0, (bf16_t*)cmat, N, nullptr, M, N, K, s, e->prefill_ws());
    }
    ZE_KCHECK();
    return ZE_OK;
}

// The public GEMM launchers with the operands the engine gives them: leading dimensions of their own, the residual epilogue, the output
// row table (tests/test_gpu_gemm_operands.py).  Everything a launcher would not take is refused here, before anything is launched.
extern "C" int ze_op_gemm(ze_engine* e, int launcher, int epi, const void* a, int lda, const void* w, int ldw, const void* bias,
                          const void* r, int ldr, void* cmat, int ldc, const int32_t* c_rows, int M, int N, int K, void* stream) {
    if (!e || !a || !w || !cmat) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (launcher < 0 || launcher > 6) return ze_fail(e, ZE_ERR_INVALID, "launcher must be in [0, 6]");
    if (M <= 0 || N <= 0 || K <= 0) return ze_fail(e, ZE_ERR_INVALID, "M, N, K > 0");
    const bool frag = launcher == 5 || launcher == 6;
    bool epi_ok = epi == ZE_EPI_NONE || epi == ZE_EPI_RESIDUAL;  // (the dispatch_epi list of the launcher's kernels, ze_gemm.hip)
    if (launcher != 6) epi_ok = epi_ok || epi == ZE_EPI_SWIGLU || epi == ZE_EPI_F32 || (launcher != 5 && epi == ZE_EPI_GELU);
    if (!epi_ok) return ze_fail(e, ZE_ERR_INVALID, "the launcher has no kernel with this epilogue");
    if (epi == ZE_EPI_RESIDUAL && !r) return ze_fail(e, ZE_ERR_INVALID, "RESIDUAL needs r");
    if (epi == ZE_EPI_SWIGLU && N % 32) return ze_fail(e, ZE_ERR_INVALID, "SwiGLU: N = 2 * width with width % 16 == 0");
    if (K % 8) return ze_fail(e, ZE_ERR_INVALID, "K must be a multiple of 8");
    if (launcher == 2 && (K % 64 || K < 64)) return ze_fail(e, ZE_ERR_INVALID, "eight-phase kernel: K a multiple of 64");
    if (lda < K || ldw < K || ldc < (epi == ZE_EPI_SWIGLU ? N / 2 : N) || (epi == ZE_EPI_RESIDUAL && ldr < N))
        return ze_fail(e, ZE_ERR_INVALID, "a leading dimension is below its extent");
    if (lda % 8 || ldw % 8 || (size_t)a % 16 || (size_t)w % 16)  // (every kernel loads its operands in 16-byte row pieces)
        return ze_fail(e, ZE_ERR_INVALID, "the rows of a and w start on 16-byte boundaries");
    if (launcher >= 3 && c_rows) return ze_fail(e, ZE_ERR_INVALID, "the launcher takes no output row table");
    if (frag && (M > 64 || N % 16 || K % 32 || (launcher == 5 && K > 4096)))
        return ze_fail(e, ZE_ERR_INVALID, "fragment path: M <= 64, N % 16, K % 32, K <= 4096");
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    const bf16_t *A = (const bf16_t*)a, *W = (const bf16_t*)w, *B = (const bf16_t*)bias;
    const bf16_t* R = epi == ZE_EPI_RESIDUAL ? (const bf16_t*)r : nullptr;
    if (!R) ldr = 0;
    bf16_t* C = (bf16_t*)cmat;
    if (frag) {  // operands packed here, as ze_op_linear act 3 / 5 does
        bf16_t *wf = nullptr, *xf = nullptr;
        const size_t mp = M <= 16 ? 16 : M <= 32 ? 32 : 64;  // the kernels read whole 16-row tiles: 1, 2 or 4 of them (dispatch_mt)
        ZE_HIP(hipMalloc((void**)&wf, ((size_t)N * K + mp * K) * sizeof(bf16_t)));
        xf = wf + (size_t)N * K;
        ze_launch_pack_fragments(W, ldw, N, K, wf, s);
        ze_launch_pack_fragments(A, lda, M, K, xf, s);
        if (launcher == 6) ze_launch_gemm_oneshot(epi, xf, wf, B, R, ldr, C, ldc, M, N, K, s);
        else ze_launch_gemm_frag(epi, xf, wf, B, R, ldr, C, ldc, M, N, K, s);
        hipError_t le = hipGetLastError();
        hipStreamSynchronize(s);
        hipFree(wf);
        if (le != hipSuccess) return ze_fail(e, ZE_ERR_HIP, hipGetErrorString(le));
        return ZE_OK;
    }
    switch (launcher) {
        case 0: ze_launch_gemm(epi, A, lda, W, ldw, B, R, ldr, C, ldc, c_rows, M, N, K, s, e->prefill_ws()); break;
        case 1: ze_launch_gemm(epi, A, lda, W, ldw, B, R, ldr, C, ldc, c_rows, M, N, K, s); break;
        case 2: ze_launch_gemm_p8(epi, A, lda, W, ldw, B, R, ldr, C, ldc, c_rows, M, N, K, s, e->prefill_ws()); break;
        case 3: ze_launch_gemm_stream(epi, A, lda, W, ldw, B, R, ldr, C, ldc, M, N, K, e->gemm_ws(), s); break;
        default: ze_launch_gemm_wide(epi, A, lda, W, ldw, B, R, ldr, C, ldc, M, N, K, e->gemm_ws(), s); break;
    }
    ZE_KCHECK();
    return ZE_OK;
}

// The W4 forms of the fragment launchers on one matrix: ze_op_gemm's launchers 5 / 6 with the MXFP4 stream as W (row-major q4 / scale
// as ze_op_quantize_mxfp4 writes them, packed here by ze_launch_pack_fragments4).  tests/test_gpu_gemm4.py holds it against
// ze_op_gemm on the dequantised bf16 weights, bit for bit.
extern "C" int ze_op_gemm4(ze_engine* e, int launcher, int epi, const void* a, int lda, const void* q4, const void* scale_e8m0,
                           const void* bias, const void* r, int ldr, void* cmat, int ldc, int M, int N, int K, void* stream) {
    if (!e || !a || !q4 || !scale_e8m0 || !cmat) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (launcher != 5 && launcher != 6) return ze_fail(e, ZE_ERR_INVALID, "only launchers 5 and 6 (the fragment kernels) have an MXFP4 form");
    if (M <= 0 || N <= 0 || K <= 0) return ze_fail(e, ZE_ERR_INVALID, "M, N, K > 0");
    if (K % 32) return ze_fail(e, ZE_ERR_INVALID, "MXFP4: K must be a multiple of 32");
    bool epi_ok = epi == ZE_EPI_NONE || epi == ZE_EPI_RESIDUAL;
    if (launcher == 5) epi_ok = epi_ok || epi == ZE_EPI_SWIGLU || epi == ZE_EPI_F32;
    if (!epi_ok) return ze_fail(e, ZE_ERR_INVALID, "the launcher has no kernel with this epilogue");
    if (epi == ZE_EPI_RESIDUAL && !r) return ze_fail(e, ZE_ERR_INVALID, "RESIDUAL needs r");
    if (epi == ZE_EPI_SWIGLU && N % 32) return ze_fail(e, ZE_ERR_INVALID, "SwiGLU: N = 2 * width with width % 16 == 0");
    if (lda < K || ldc < (epi == ZE_EPI_SWIGLU ? N / 2 : N) || (epi == ZE_EPI_RESIDUAL && ldr < N))
        return ze_fail(e, ZE_ERR_INVALID, "a leading dimension is below its extent");
    if (lda % 8 || (size_t)a % 16 || (size_t)q4 % 4) return ze_fail(e, ZE_ERR_INVALID, "the rows of a start on 16-byte boundaries, q4 on a 4-byte one");
    if (M > 64 || N % 16 || (launcher == 5 && K > 4096)) return ze_fail(e, ZE_ERR_INVALID, "fragment path: M <= 64, N % 16, K % 32, K <= 4096");
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    const bf16_t *A = (const bf16_t*)a, *B = (const bf16_t*)bias;
    const bf16_t* R = epi == ZE_EPI_RESIDUAL ? (const bf16_t*)r : nullptr;
    if (!R) ldr = 0;
    bf16_t* C = (bf16_t*)cmat;
    const size_t mp = M <= 16 ? 16 : M <= 32 ? 32 : 64;  // the kernels read whole 16-row tiles: 1, 2 or 4 of them (dispatch_mt)
    const size_t codes = (size_t)N * K / 2, scales = (size_t)N * K / 32;
    uint8_t* buf = nullptr;  // activation fragments, then the codes, then the scales
    ZE_HIP(hipMalloc((void**)&buf, mp * K * sizeof(bf16_t) + codes + scales));
    bf16_t* xf = (bf16_t*)buf;
    uint8_t *wf4 = buf + mp * K * sizeof(bf16_t), *sf4 = wf4 + codes;
    ze_launch_pack_fragments(A, lda, M, K, xf, s);
    ze_launch_pack_fragments4((const uint8_t*)q4, (const uint8_t*)scale_e8m0, N, K, wf4, sf4, s);
    if (launcher == 6) ze_launch_gemm_oneshot(epi, xf, (const bf16_t*)wf4, B, R, ldr, C, ldc, M, N, K, s, nullptr, nullptr, sf4);
    else ze_launch_gemm_frag(epi, xf, (const bf16_t*)wf4, B, R, ldr, C, ldc, M, N, K, s, nullptr, nullptr, sf4);
    hipError_t le = hipGetLastError();
    hipStreamSynchronize(s);
    hipFree(buf);
    if (le != hipSuccess) return ze_fail(e, ZE_ERR_HIP, hipGetErrorString(le));
    return ZE_OK;
}

extern "C" int ze_fragment_bytes(ze_engine* e, size_t* bytes) {
    if (!e || !bytes) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    *bytes = (e->frag_ready && !e->wide_regime()) ? e->arena_f_bytes + (e->fp8_ready ? e->arena_f8_bytes : 0) + e->arena_f4_bytes : 0;
    return ZE_OK;
}

extern "C" int ze_op_token_logprob(ze_engine* e, const void* logits, int rows, int vocab, int ld, const int32_t* targets,
                                   float* out, void* stream) {
    if (!logits || !targets || !out || rows < 0 || vocab <= 0 || ld < vocab || ld % 8)
        return ze_fail(e, ZE_ERR_INVALID, "bad token_logprob arguments");
    hipSetDevice(e->device);
    ze_launch_token_logprob((const bf16_t*)logits, ld, vocab, targets, out, rows, (hipStream_t)stream);
    ZE_KCHECK();
    return ZE_OK;
}

extern "C" int ze_op_score_detail(ze_engine* e, const void* logits, int rows, int vocab, int ld, const int32_t* targets, int top_n,
                                  float* out_logprob, float* out_entropy, int32_t* out_rank, int32_t* out_top_ids,
                                  float* out_top_logprobs, void* stream) {
    if (!e || !logits || !targets || !out_logprob || rows < 0 || vocab <= 0 || ld < vocab || ld % 8)
        return ze_fail(e, ZE_ERR_INVALID, "bad score_detail arguments");
    if (top_n < 0 || top_n > ZE_MAX_TOP_LOGPROBS) return ze_fail(e, ZE_ERR_INVALID, "top_n must be in [0, 20]");
    if (!out_top_ids != !out_top_logprobs || (out_top_ids && top_n < 1))
        return ze_fail(e, ZE_ERR_INVALID, "the top arrays are both null, or both set with top_n >= 1");
    hipSetDevice(e->device);
    ze_launch_score_detail((const bf16_t*)logits, ld, vocab, targets, out_top_ids ? top_n : 0, out_logprob, out_entropy, out_rank,
                           out_top_ids, out_top_logprobs, rows, (hipStream_t)stream);
    ZE_KCHECK();
    return ZE_OK;
}

extern "C" int ze_op_rmsnorm(ze_engine* e, const void* x, const void* weight, void* y, int rows, int cols, float eps,
                             void* stream) {
    if (!e || !x || !weight || !y) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (cols % 8) return ze_fail(e, ZE_ERR_INVALID, "cols must be a multiple of 8");
    hipSetDevice(e->device);
    ze_launch_rmsnorm((const bf16_t*)x, cols, (const bf16_t*)weight, (bf16_t*)y, cols, rows, cols, eps,
                      (hipStream_t)stream);
    ZE_KCHECK();
    return ZE_OK;
}

extern "C" int ze_op_attention(ze_engine* e, const void* q, const void* k, const void* v, void* o, int T, int heads,
                               int kv_heads, int D, const int32_t* cu, int n_seg, int causal, void* stream) {
    if (!e || !q || !k || !v || !o || !cu) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (D != 80 && D != 128) return ze_fail(e, ZE_ERR_INVALID, "D must be 80 or 128");
    if (heads % kv_heads) return ze_fail(e, ZE_ERR_INVALID, "kv_heads must divide heads");
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> tiles((size_t)4 * (T / 64 + n_seg + 2));
    const int bq = ze_gemv_knobs[1] == 9 ? 64 : ZE_FA_BQ_LONG;  // (two query tiles per wave unless knob 1 = 9: the unit op covers both forms)
    const int nt = build_tiles(cu, n_seg, tiles.data(), (int)tiles.size() / 4, bq);
    if (nt < 0) return ze_fail(e, ZE_ERR_NOMEM, "tile overflow");
    int4* dt = nullptr;
    ZE_HIP(hipMalloc((void**)&dt, (size_t)std::max(nt, 1) * 16));
    ZE_HIP(hipMemcpyAsync(dt, tiles.data(), (size_t)nt * 16, hipMemcpyHostToDevice, s));
    // causal inside each segment: key j visible to query i iff j <= i (absolute row indices, offset 0)
    ze_launch_flash_attn(D, causal, (const bf16_t*)q, heads * D, D, (const bf16_t*)k, kv_heads * D, D,
                         (const bf16_t*)v, kv_heads * D, D, (bf16_t*)o, heads * D, D, dt, nt, heads, heads / kv_heads,
                         1.0f / sqrtf((float)D), 0, s, nullptr, 0, bq);
    hipError_t le = hipGetLastError();
    hipStreamSynchronize(s);
    hipFree(dt);
    if (le != hipSuccess) return ze_fail(e, ZE_ERR_HIP, hipGetErrorString(le));
    return ZE_OK;
}

// ---- K4 / K5 + K8 / K13 / K15 + K18 on their own (one entry per kernel), the launchers ze_vit_forward / ze_prefill use
// K4: rows of pixel_values gathered into WINDOW order (+ the cast to bf16 the patch embed reads), and merged rows scattered back
extern "C" int ze_op_window_gather(ze_engine* e, const float* pixel_values, const int32_t* grid_thw, int n_images, void* out_bf16,
                                   void* stream) {
    if (!e || !pixel_values || !grid_thw || !out_bf16 || n_images <= 0) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    const ze_config& c = e->cfg;
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    const int mu = c.spatial_merge_size * c.spatial_merge_size;
    const int pk = c.in_channels * c.temporal_patch_size * c.patch_size * c.patch_size;
    std::vector<int64_t> widx;
    std::vector<int32_t> cu_win;
    ze_window_index_impl(grid_thw, n_images, c.spatial_merge_size, c.window_size, c.patch_size, widx, cu_win);
    const int n = (int)widx.size() * mu;
    if (n > c.max_patches) return ze_fail(e, ZE_ERR_NOMEM, "too many patches for max_patches");
    std::vector<int> perm(n);
    for (int j = 0; j < n / mu; ++j)
        for (int u = 0; u < mu; ++u) perm[j * mu + u] = (int)widx[j] * mu + u;
    ZE_HIP(hipMemcpyAsync(e->vperm, perm.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    ZE_HIP(hipStreamSynchronize(s));  // (perm is a local)
    ze_launch_gather_cast_rows(pixel_values, pk, e->vperm, (bf16_t*)out_bf16, pk, n, s);
    ZE_KCHECK();
    return ZE_OK;
}
extern "C" int ze_op_window_scatter(ze_engine* e, const void* x_bf16, int cols, const int32_t* grid_thw, int n_images, void* out_bf16,
                                    void* stream) {
    if (!e || !x_bf16 || !grid_thw || !out_bf16 || n_images <= 0 || cols <= 0 || cols % 8) return ze_fail(e, ZE_ERR_INVALID, "bad argument (cols % 8)");
    const ze_config& c = e->cfg;
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    std::vector<int64_t> widx;
    std::vector<int32_t> cu_win;
    ze_window_index_impl(grid_thw, n_images, c.spatial_merge_size, c.window_size, c.patch_size, widx, cu_win);
    const int m = (int)widx.size();
    if (m > c.max_patches) return ze_fail(e, ZE_ERR_NOMEM, "too many rows for max_patches");
    std::vector<int> inv(m);
    for (int j = 0; j < m; ++j) inv[j] = (int)widx[j];
    ZE_HIP(hipMemcpyAsync(e->vinv, inv.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, s));
    ZE_HIP(hipStreamSynchronize(s));
    ze_launch_scatter_rows((const bf16_t*)x_bf16, cols, e->vinv, (bf16_t*)out_bf16, cols, m, cols, s);
    ZE_KCHECK();
    return ZE_OK;
}
// K5 + K8: the 2-D rotary tables of the grids (fp32, HF:...:125-134,441-446) applied to the q and k thirds of qkv [n, 3 * heads * D]
// in place, fp32 arithmetic (HF:...:160-171); rows in WINDOW order when window_order != 0 (as inside the ViT), else HF order
extern "C" int ze_op_vision_rope(ze_engine* e, void* qkv_bf16, const int32_t* grid_thw, int n_images, int window_order, void* stream) {
    if (!e || !qkv_bf16 || !grid_thw || n_images <= 0) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    const ze_config& c = e->cfg;
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    const int mu = c.spatial_merge_size * c.spatial_merge_size;
    const int hd = e->vit_head_dim, half = hd / 2, nf = half / 2;
    std::vector<int64_t> widx;
    std::vector<int32_t> cu_win, hw;
    ze_window_index_impl(grid_thw, n_images, c.spatial_merge_size, c.window_size, c.patch_size, widx, cu_win);
    ze_vision_pos_ids_impl(grid_thw, n_images, c.spatial_merge_size, hw);
    const int n = (int)widx.size() * mu;
    if (n > c.max_patches) return ze_fail(e, ZE_ERR_NOMEM, "too many patches for max_patches");
    std::vector<float> invf(nf), hc((size_t)n * half), hs((size_t)n * half);
    for (int i = 0; i < nf; ++i) invf[i] = 1.0f / powf(10000.0f, (float)(2 * i) / (float)half);
    for (int r = 0; r < n; ++r) {
        const int old = window_order ? (int)widx[r / mu] * mu + r % mu : r;
        for (int i = 0; i < nf; ++i) {
            const float fh = (float)hw[2 * old] * invf[i], fw = (float)hw[2 * old + 1] * invf[i];
            hc[(size_t)r * half + i] = cosf(fh);
            hs[(size_t)r * half + i] = sinf(fh);
            hc[(size_t)r * half + nf + i] = cosf(fw);
            hs[(size_t)r * half + nf + i] = sinf(fw);
        }
    }
    ZE_HIP(hipMemcpyAsync(e->vcos, hc.data(), hc.size() * sizeof(float), hipMemcpyHostToDevice, s));
    ZE_HIP(hipMemcpyAsync(e->vsin, hs.data(), hs.size() * sizeof(float), hipMemcpyHostToDevice, s));
    ZE_HIP(hipStreamSynchronize(s));
    ze_launch_vision_rope((bf16_t*)qkv_bf16, e->vcos, e->vsin, n, c.vit_heads, hd, s);
    ZE_KCHECK();
    return ZE_OK;
}
// K13: out[t] = embed_tokens[ids[t]], rows whose id is the image token overwritten by the feature rows in order (HF:...:1206-1215)
extern "C" int ze_op_embed_scatter(ze_engine* e, const int32_t* input_ids, int len, const void* image_embeds, int n_image_rows,
                                   void* out_bf16, void* stream) {
    if (!e || !input_ids || !out_bf16 || len <= 0) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    const ze_config& c = e->cfg;
    if (len > e->prefill_rows) return ze_fail(e, ZE_ERR_NOMEM, "more rows than the prefill workspace holds");
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    std::vector<int> src(len);
    int img = 0;
    for (int t = 0; t < len; ++t) {
        if (input_ids[t] < 0 || input_ids[t] >= c.vocab) return ze_fail(e, ZE_ERR_INVALID, "token id out of range");
        src[t] = input_ids[t] == c.image_token_id ? -1 - img++ : input_ids[t];
    }
    if (img != n_image_rows || (img > 0 && !image_embeds))
        return ze_fail(e, ZE_ERR_MISMATCH, "Image features and image tokens do not match, tokens: " + std::to_string(img) +
                                               ", features: " + std::to_string(n_image_rows));
    ZE_HIP(hipMemcpyAsync(e->tsrc, src.data(), (size_t)len * sizeof(int), hipMemcpyHostToDevice, s));
    ZE_HIP(hipStreamSynchronize(s));
    ze_launch_embed_rows(e->tsrc, e->embed, (const bf16_t*)image_embeds, (bf16_t*)out_bf16, len, c.hidden, s);
    ZE_KCHECK();
    return ZE_OK;
}
// K15 + K18: M-RoPE on the q / k parts of qkv [T, (heads + 2 kv_heads) * 128] (q in place; cos / sin rounded to bf16, products
// and sum rounded as HF's bf16 tensors round them, HF:...:557-599) and the KV append: the roped k rows and the v rows go
// into `layer`'s cache of chain `seq` at positions past .. past + T - 1 (DynamicCache.update, HF:...:667-668).  The chain's
// length is NOT changed (a unit op: ze_op_kv_read reads rows back whatever the chain's length says).
extern "C" int ze_op_mrope_kv(ze_engine* e, int seq, int layer, void* qkv_bf16, int T, const int32_t* position_ids, int past, void* stream) {
    ZE_TRY(check_seq(e, seq));
    const ze_config& c = e->cfg;
    if (!qkv_bf16 || !position_ids || T <= 0 || layer < 0 || layer >= c.layers || past < 0 || past + T > c.max_ctx || T > e->prefill_rows)
        return ze_fail(e, ZE_ERR_INVALID, "bad mrope_kv arguments");
    for (int i = 0; i < 3 * T; ++i)
        if (position_ids[i] < 0 || position_ids[i] >= e->max_pos) return ze_fail(e, ZE_ERR_INVALID, "position id out of range");
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    ZE_HIP(hipMemcpyAsync(e->tpos, position_ids, (size_t)3 * T * sizeof(int), hipMemcpyHostToDevice, s));
    ZE_HIP(hipStreamSynchronize(s));
    ze_launch_mrope_kv((bf16_t*)qkv_bf16, T, c.heads, c.kv_heads, e->head_dim, e->cosT, e->sinT, e->tpos, e->axis_of, e->kc(layer, seq),
                       e->vc(layer, seq), c.max_ctx, past, nullptr, 0, s);
    ZE_KCHECK();
    return ZE_OK;
}
// the decode-step form of the same (k_rope_kv_batch: row b = chain seqs[b] at ITS position ctx + rope_delta, K/V appended at ctx)
extern "C" int ze_op_rope_kv_decode(ze_engine* e, const int32_t* seqs, int n, int layer, void* qkv_bf16, void* stream) {
    if (!e || !seqs || !qkv_bf16 || n <= 0 || n > e->cfg.max_seqs || layer < 0 || layer >= e->cfg.layers)
        return ze_fail(e, ZE_ERR_INVALID, "bad rope_kv_decode arguments");
    const ze_config& c = e->cfg;
    for (int i = 0; i < n; ++i) {
        ZE_TRY(check_seq(e, seqs[i]));
        if (e->ctx_host[seqs[i]] + 1 > c.max_ctx) return ze_fail(e, ZE_ERR_NOMEM, "sequence exceeds max_ctx");
    }
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    ze_launch_set_ints(e->bseq, seqs, n, s);
    ze_launch_rope_kv_batch((bf16_t*)qkv_bf16, n, c.heads, c.kv_heads, e->head_dim, e->cosT, e->sinT, e->st_dev, e->bseq, e->kc(layer, 0),
                            e->vc(layer, 0), (size_t)c.kv_heads * c.max_ctx * e->head_dim, c.max_ctx, s);
    ZE_KCHECK();
    return ZE_OK;
}
// The attention of ONE batched decode step, alone: row b of qkv_bf16 [n, (heads + 2 kv_heads) x 128] is chain seqs[b]'s
// projection AFTER ze_op_rope_kv_decode (which rotated q / k and appended k, v at row ctx of the cache); the kernel of the step
// (k_attn_decode_wave_long in the row-streaming family and from 17 chains on, the fragment family's choice below) attends the
// q heads over rows 0 .. ctx of `layer` and writes out_bf16 [n, heads x 128].  Chain state is not advanced.
extern "C" int ze_op_attn_decode(ze_engine* e, const int32_t* seqs, int n, int layer, const void* qkv_bf16, void* out_bf16, void* stream) {
    if (!e || !seqs || !qkv_bf16 || !out_bf16 || n <= 0 || n > e->cfg.max_seqs || layer < 0 || layer >= e->cfg.layers)
        return ze_fail(e, ZE_ERR_INVALID, "bad attn_decode arguments");
    for (int i = 0; i < n; ++i) {
        ZE_TRY(check_seq(e, seqs[i]));
        if (e->ctx_host[seqs[i]] + 1 > e->cfg.max_ctx) return ze_fail(e, ZE_ERR_NOMEM, "sequence exceeds max_ctx");
    }
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    ze_launch_set_ints(e->bseq, seqs, n, s);
    sync_prefix(e, seqs, n, s);
    set_live_parts(e, seqs, n, 1);
    launch_batch_attention(e, ze_rows_caller(e, (const bf16_t*)qkv_bf16, (bf16_t*)out_bf16), layer, n, false, s);
    ZE_KCHECK();
    return ZE_OK;
}
// The attention of the SINGLE-CHAIN decode step, alone: the step's own launch (launch_step_attention) on the caller's row -- qkv_bf16
// [(heads + 2 kv_heads) x 128] as ze_op_rope_kv_decode / ze_op_mrope_kv left it, of which the q part is read -- over rows 0 .. ctx of
// `layer`'s cache of chain `seq`; out_bf16 [heads x 128].  Chain state is not advanced.
extern "C" int ze_op_attn_decode_single(ze_engine* e, int seq, int layer, const void* qkv_bf16, void* out_bf16, void* stream) {
    ZE_TRY(check_seq(e, seq));
    if (!qkv_bf16 || !out_bf16 || layer < 0 || layer >= e->cfg.layers) return ze_fail(e, ZE_ERR_INVALID, "bad attn_decode_single arguments");
    if (e->head_dim != 128) return ze_fail(e, ZE_ERR_INVALID, "the decode attention needs 128-wide heads");
    if (e->ctx_host[seq] + 1 > e->cfg.max_ctx) return ze_fail(e, ZE_ERR_NOMEM, "sequence exceeds max_ctx");
    hipSetDevice(e->device);
    launch_step_attention(e, layer, seq, (hipStream_t)stream, (const bf16_t*)qkv_bf16, (bf16_t*)out_bf16);
    ZE_KCHECK();
    return ZE_OK;
}
// rows [start, start + n) of `layer`'s K and V cache of chain `seq`, every kv head: out_k / out_v bf16 [kv_heads, n, 128] (device)
extern "C" int ze_op_kv_read(ze_engine* e, int seq, int layer, int start, int n, void* out_k, void* out_v, void* stream) {
    ZE_TRY(check_seq(e, seq));
    const ze_config& c = e->cfg;
    if (!out_k || !out_v || layer < 0 || layer >= c.layers || start < 0 || n <= 0 || start + n > c.max_ctx)
        return ze_fail(e, ZE_ERR_INVALID, "bad kv_read arguments");
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    const size_t row = (size_t)e->head_dim * sizeof(bf16_t);
    for (int h = 0; h < c.kv_heads; ++h) {
        ZE_HIP(hipMemcpyAsync((char*)out_k + (size_t)h * n * row, e->kc(layer, seq) + ((size_t)h * c.max_ctx + start) * e->head_dim,
                              (size_t)n * row, hipMemcpyDeviceToDevice, s));
        ZE_HIP(hipMemcpyAsync((char*)out_v + (size_t)h * n * row, e->vc(layer, seq) + ((size_t)h * c.max_ctx + start) * e->head_dim,
                              (size_t)n * row, hipMemcpyDeviceToDevice, s));
    }
    return ZE_OK;
}

// ONE launch of the single-chain decode GEMV family (ze_launch_gemv: k_gemv, bf16 or FP8 stream) on the caller's device operands,
// every epilogue and prologue reachable -- the product path calls the launcher only from ze_enqueue_decode_step / ze_prefill, with
// the model's own shapes.  epi = the ZE_GV_* code.  A shape the launcher refuses is an error, never another kernel.
// (w4 / scale4 non-null: the MXFP4 stream of ze_op_gemv4)
static int op_gemv_any(ze_engine* e, int epi, const void* w_bf16, const void* w8, const void* scale8, const void* w4, const void* scale4,
                       const void* x_bf16, const void* norm_w, float eps, const void* bias_bf16, int act8, int N, int K, void* out_bf16,
                       float* out_f32, const uint8_t* seen, float penalty, int32_t* out_token, int seq, int layer,
                       const void* embed, int token, void* embed_out, void* stream) {
    if (!e || (!w_bf16 && !w8 && !w4) || (w8 && !scale8) || (w4 && !scale4) || (!x_bf16 && !embed))
        return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (epi < ZE_GV_QKV_ROPE || epi > ZE_GV_PLAIN) return ze_fail(e, ZE_ERR_INVALID, "unknown epilogue");
    if (N < 2 || N % 2 || K < 8 || K % 8) return ze_fail(e, ZE_ERR_INVALID, "N must be even, K a multiple of 8");
    if (w4 && K % 32) return ze_fail(e, ZE_ERR_INVALID, "the MXFP4 stream needs K % 32 == 0 (one scale per 32 elements)");
    if (epi == ZE_GV_SWIGLU && N % 32) return ze_fail(e, ZE_ERR_INVALID, "SwiGLU: N = 2 * width with width % 16 == 0");
    if (epi == ZE_GV_LOGITS ? !out_f32 : !out_bf16) return ze_fail(e, ZE_ERR_INVALID, "null output");
    if (act8 && (!w8 || !norm_w)) return ze_fail(e, ZE_ERR_INVALID, "act8 goes with the FP8 stream and the norm prologue");
    if (embed && (!embed_out || token < 0)) return ze_fail(e, ZE_ERR_INVALID, "embedding prologue: embed_out and a token");
    if (out_token && epi != ZE_GV_LOGITS) return ze_fail(e, ZE_ERR_INVALID, "the folded arg-max belongs to the LOGITS epilogue");
    if (out_token && penalty != 1.0f && !seen) return ze_fail(e, ZE_ERR_INVALID, "a penalty needs the seen flags");
    const ze_config& c = e->cfg;
    if (epi == ZE_GV_QKV_ROPE) {
        ZE_TRY(check_seq(e, seq));
        if (layer < 0 || layer >= c.layers || e->head_dim != 128 || N != (c.heads + 2 * c.kv_heads) * 128)
            return ze_fail(e, ZE_ERR_INVALID, "QKV_ROPE: N = (heads + 2 kv_heads) x 128 of the engine, a layer of the engine");
        if (e->ctx_host[seq] + 1 > c.max_ctx) return ze_fail(e, ZE_ERR_NOMEM, "sequence exceeds max_ctx");
    }
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    // scratch: a chain state that carries `token` (embedding prologue), and what the arg-max reduction writes besides the token
    ze_seq_dev* st_tmp = nullptr;
    uint8_t* seen_tmp = nullptr;
    if (embed || out_token) ZE_HIP(hipMalloc((void**)&st_tmp, sizeof(ze_seq_dev) + 2 * sizeof(int) + (out_token ? (size_t)N : 0)));
    int32_t* tok_tmp = reinterpret_cast<int32_t*>(st_tmp + 1);
    int r = ZE_OK;
    const ze_seq_dev* st = epi == ZE_GV_QKV_ROPE ? e->st_dev + seq : nullptr;
    if (embed) {
        if (st) {
            if (hipMemcpyAsync(st_tmp, st, sizeof(ze_seq_dev), hipMemcpyDeviceToDevice, s) != hipSuccess) r = ze_fail(e, ZE_ERR_HIP, "hipMemcpyAsync failed");
        } else if (hipMemsetAsync(st_tmp, 0, sizeof(ze_seq_dev), s) != hipSuccess) {
            r = ze_fail(e, ZE_ERR_HIP, "hipMemsetAsync failed");
        }
        ze_launch_set_ints(&st_tmp->token, &token, 1, s);
        st = st_tmp;
    }
    ze_gemv_args a;
    memset(&a, 0, sizeof(a));
    a.W = (const bf16_t*)w_bf16;
    a.ldw = K;
    a.W8 = (const uint8_t*)w8;
    a.scale8 = (const float*)scale8;
    a.ldw8 = K;
    a.W4 = (const uint8_t*)w4;
    a.scale4 = (const uint8_t*)scale4;
    a.N = N;
    a.K = K;
    a.x = (const bf16_t*)x_bf16;
    a.norm_w = (const bf16_t*)norm_w;
    a.eps = eps;
    a.bias = (const bf16_t*)bias_bf16;
    a.out_bf16 = (bf16_t*)out_bf16;
    a.out_f32 = out_f32;
    a.D = 128;
    a.act8 = act8 ? 1 : 0;
    a.st = st;
    if (epi == ZE_GV_QKV_ROPE) {
        a.cosT = e->cosT;
        a.sinT = e->sinT;
        a.kcache = e->kc(layer, seq);
        a.vcache = e->vc(layer, seq);
        a.heads = c.heads;
        a.kv_heads = c.kv_heads;
        a.max_ctx = c.max_ctx;
    }
    a.embed = (const bf16_t*)embed;
    a.embed_out = (bf16_t*)embed_out;
    if (out_token) {  // the engine's own partial slots (created once with the engine: ze_launch_amax_init), as the decode step uses them
        a.seen = seen;
        a.penalty = penalty;
        a.amax_ws = e->damax;
    }
    if (r == ZE_OK && !ze_launch_gemv(epi, a, s))
        r = ze_fail(e, (w8 && K % 16) ? ZE_ERR_INVALID : ZE_ERR_NOMEM,
                    "shape refused by the GEMV launcher (x does not fit the LDS stage, or the FP8 stream with K % 16 != 0)");
    if (r == ZE_OK && out_token) {
        seen_tmp = reinterpret_cast<uint8_t*>(tok_tmp + 2);
        const int fresh[3] = {0, 0, 1};  // finished, n_gen, max_gen: the token lands in tok_tmp[0]
        ze_launch_set_ints(&st_tmp->finished, fresh, 3, s);
        ze_launch_sample_folded(e->damax, N, seen_tmp, st_tmp, e->eos_dev, 0, c.pad_token_id, /*ignore_eos=*/1, /*advance_ctx=*/0, tok_tmp, s);
        if (hipMemcpyAsync(out_token, tok_tmp, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess) r = ze_fail(e, ZE_ERR_HIP, "hipMemcpyAsync failed");
    }
    if (r == ZE_OK && hipGetLastError() != hipSuccess) r = ze_fail(e, ZE_ERR_HIP, "GEMV launch failed");
    if (st_tmp) {
        if (hipStreamSynchronize(s) != hipSuccess && r == ZE_OK) r = ze_fail(e, ZE_ERR_HIP, "hipStreamSynchronize failed");
        hipFree(st_tmp);
    }
    return r;
}

extern "C" int ze_op_gemv(ze_engine* e, int epi, const void* w_bf16, const void* w8, const void* scale8, const void* x_bf16,
                          const void* norm_w, float eps, const void* bias_bf16, int act8, int N, int K, void* out_bf16,
                          float* out_f32, const uint8_t* seen, float penalty, int32_t* out_token, int seq, int layer,
                          const void* embed, int token, void* embed_out, void* stream) {
    return op_gemv_any(e, epi, w_bf16, w8, scale8, nullptr, nullptr, x_bf16, norm_w, eps, bias_bf16, act8, N, K, out_bf16, out_f32, seen,
                       penalty, out_token, seq, layer, embed, token, embed_out, stream);
}

// the same launch with the MXFP4 stream as W (ze_gemv4.hip): q4 u8 [N, K / 2], scale_e8m0 u8 [N, K / 32]
extern "C" int ze_op_gemv4(ze_engine* e, int epi, const void* q4, const void* scale_e8m0, const void* x_bf16, const void* norm_w, float eps,
                           const void* bias_bf16, int N, int K, void* out_bf16, float* out_f32, const uint8_t* seen, float penalty,
                           int32_t* out_token, int seq, int layer, const void* embed, int token, void* embed_out, void* stream) {
    if (!q4 || !scale_e8m0) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    return op_gemv_any(e, epi, nullptr, nullptr, nullptr, q4, scale_e8m0, x_bf16, norm_w, eps, bias_bf16, 0, N, K, out_bf16, out_f32, seen,
                       penalty, out_token, seq, layer, embed, token, embed_out, stream);
}

// fp32 logits of n hidden rows through the lm_head pass of the prefill paths (ze_launch_logits_rows: k_logits_multi, final RMSNorm
// fused, one pass over W per eight rows).  A K the launcher refuses (eight staged rows do not fit in LDS) is ZE_ERR_NOMEM.
extern "C" int ze_op_logits_rows(ze_engine* e, const void* w_bf16, const void* norm_w, float eps, const void* x_bf16, float* out_f32,
                                 int n, int N, int K, void* stream) {
    if (!e || !w_bf16 || !norm_w || !x_bf16 || !out_f32) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (n <= 0 || N <= 0 || K < 8 || K % 8) return ze_fail(e, ZE_ERR_INVALID, "n and N positive, K a multiple of 8");
    hipSetDevice(e->device);
    std::vector<const bf16_t*> xr(n);
    std::vector<float*> lo(n);
    for (int i = 0; i < n; ++i) {
        xr[i] = (const bf16_t*)x_bf16 + (size_t)i * K;
        lo[i] = out_f32 + (size_t)i * N;
    }
    if (!ze_launch_logits_rows((const bf16_t*)w_bf16, K, N, K, (const bf16_t*)norm_w, eps, xr.data(), lo.data(), n, (hipStream_t)stream))
        return ze_fail(e, ZE_ERR_NOMEM, "shape refused by the logits-rows launcher (eight staged rows do not fit the LDS stage)");
    ZE_KCHECK();
    return ZE_OK;
}

// ================================================================== fp8 decode weights
static int quantize_linear(ze_engine* e, ze_linear& l, int rows, int cols, uint8_t*& cur8, float*& curs, hipStream_t s) {
    l.ld8 = (cols + 15) / 16 * 16;
    l.w8 = cur8;
    l.scale8 = curs;
    cur8 += (size_t)rows * l.ld8;
    curs += rows;
    ze_launch_quantize_rows(l.w, rows, cols, l.ld, l.w8, l.ld8, l.scale8, s);
    return ZE_OK;
}

extern "C" int ze_weights_quantize_fp8(ze_engine* e, void* stream) {
    if (!e) return ze_fail(e, ZE_ERR_INVALID, "null engine");
    if (e->mx4_ready) return ze_fail(e, ZE_ERR_INVALID, "the engine streams MXFP4 decode weights: the two formats exclude each other");
    if (e->fp8_ready) return ZE_OK;  // (a weight change clears the flag: ze_weights_changed)
    const ze_config& c = e->cfg;
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    const int H = c.hidden, hd = e->head_dim, nq = c.heads * hd, nqkv = nq + 2 * c.kv_heads * hd, ip = e->text_ipad;
    auto pad16 = [](int x) { return (size_t)((x + 15) / 16 * 16); };
    size_t bytes = 0, rows = 0;
    for (int li = 0; li < c.layers; ++li) {
        bytes += (size_t)nqkv * pad16(H) + (size_t)H * pad16(nq) + (size_t)2 * ip * pad16(H) + (size_t)H * pad16(ip);
        rows += (size_t)nqkv + H + 2 * ip + H;
    }
    const bool head = !c.tie_word_embeddings;  // a tied lm_head is the embedding table: it stays bf16
    if (head) {
        bytes += (size_t)c.vocab * pad16(H);
        rows += c.vocab;
    }
    if (!e->arena8) ZE_HIP(hipMalloc((void**)&e->arena8, bytes + rows * sizeof(float) + 256));  // re-quantisation reuses it
    ZE_HIP(hipMemsetAsync(e->arena8, 0, bytes + rows * sizeof(float) + 256, s));
    uint8_t* cur8 = e->arena8;
    float* curs = reinterpret_cast<float*>(e->arena8 + (bytes + 255) / 256 * 256);
    for (int li = 0; li < c.layers; ++li) {
        ze_text_layer& L = e->tl[li];
        quantize_linear(e, L.qkv, nqkv, H, cur8, curs, s);
        quantize_linear(e, L.o, H, nq, cur8, curs, s);
        quantize_linear(e, L.gate_up, 2 * ip, H, cur8, curs, s);
        quantize_linear(e, L.down, H, ip, cur8, curs, s);
    }
    if (head) {
        e->lm_head8.w = e->lm_head;
        e->lm_head8.ld = H;
        quantize_linear(e, e->lm_head8, c.vocab, H, cur8, curs, s);
    }
    ZE_KCHECK();
    ZE_HIP(hipStreamSynchronize(s));
    e->fp8_ready = true;
    e->frag_ready = false;  // the bf16 copies were replaced by the dequantised values
    ze_prefix_weights_changed(e);
    ++ze_tune_epoch;  // captured decode steps hold the bf16 streams
    return ZE_OK;
}

// ================================================================== MXFP4 decode weights
// The life cycle of the fp8 switch above, line by line, with the 4-bit stream in the fp8 stream's place; only the batch-1 GEMVs read
// it (gemv_args_of), every other path computes from the dequantised bf16 arena.
static bool mx4_takes(const ze_linear& l, int cols) { return cols % 32 == 0 && l.ld % 8 == 0; }

extern "C" int ze_weights_quantize_mxfp4(ze_engine* e, void* stream) {
    if (!e) return ze_fail(e, ZE_ERR_INVALID, "null engine");
    if (e->fp8_ready) return ze_fail(e, ZE_ERR_INVALID, "the engine streams FP8 decode weights: the two formats exclude each other");
    if (e->mx4_ready) return ZE_OK;  // (a weight change clears the flag: ze_weights_changed)
    const ze_config& c = e->cfg;
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    const int H = c.hidden, hd = e->head_dim, nq = c.heads * hd, nqkv = nq + 2 * c.kv_heads * hd, ip = e->text_ipad;
    const bool head = !c.tie_word_embeddings;  // a tied lm_head is the embedding table: it stays bf16
    if (head) {
        e->lm_head8.w = e->lm_head;
        e->lm_head8.ld = H;
    }
    // (tensor, rows, cols) in stream order; a tensor whose K is not a multiple of 32 keeps its bf16 stream
    std::vector<std::tuple<ze_linear*, int, int>> todo;
    for (int li = 0; li < c.layers; ++li) {
        ze_text_layer& L = e->tl[li];
        todo.emplace_back(&L.qkv, nqkv, H);
        todo.emplace_back(&L.o, H, nq);
        todo.emplace_back(&L.gate_up, 2 * ip, H);
        todo.emplace_back(&L.down, H, ip);
    }
    if (head) todo.emplace_back(&e->lm_head8, c.vocab, H);
    size_t codes = 0, scales = 0;
    for (auto& t : todo) {
        if (!mx4_takes(*std::get<0>(t), std::get<2>(t))) continue;
        codes += (size_t)std::get<1>(t) * (std::get<2>(t) / 2);   // rows of K / 2 bytes: a multiple of 16
        scales += (size_t)std::get<1>(t) * (std::get<2>(t) / 32);
    }
    if (!e->arena4) ZE_HIP(hipMalloc((void**)&e->arena4, codes + scales + 256));  // re-quantisation reuses it
    uint8_t* cur4 = e->arena4;
    uint8_t* curs = e->arena4 + codes;
    for (auto& t : todo) {
        ze_linear& l = *std::get<0>(t);
        const int rows = std::get<1>(t), cols = std::get<2>(t);
        if (!mx4_takes(l, cols)) continue;
        l.w4 = cur4;
        l.scale4 = curs;
        cur4 += (size_t)rows * (cols / 2);
        curs += (size_t)rows * (cols / 32);
        ze_launch_quantize_mxfp4(l.w, rows, cols, l.ld, l.w4, l.scale4, s);
    }
    ZE_KCHECK();
    ZE_HIP(hipStreamSynchronize(s));
    e->mx4_ready = true;
    e->frag_ready = false;  // the bf16 copies were replaced by the dequantised values
    ze_prefix_weights_changed(e);
    ++ze_tune_epoch;  // captured decode steps hold the bf16 streams
    return ZE_OK;
}

extern "C" int ze_op_quantize_mxfp4(ze_engine* e, void* w_bf16, int rows, int cols, void* q_out, void* scale_out, void* stream) {
    if (!e || !w_bf16 || !q_out || !scale_out || rows <= 0 || cols <= 0 || cols % 32)
        return ze_fail(e, ZE_ERR_INVALID, "bad argument (cols must be a multiple of 32)");
    if (((uintptr_t)w_bf16 | (uintptr_t)q_out) % 16) return ze_fail(e, ZE_ERR_INVALID, "w_bf16 and q_out must be 16-byte aligned");
    hipSetDevice(e->device);
    ze_launch_quantize_mxfp4((bf16_t*)w_bf16, rows, cols, cols, (uint8_t*)q_out, (uint8_t*)scale_out, (hipStream_t)stream);
    ZE_KCHECK();
    return ZE_OK;
}

extern "C" int ze_weight_format(ze_engine* e) {
    if (!e) return ze_fail(e, ZE_ERR_INVALID, "null engine");
    return e->mx4_ready ? ZE_WEIGHTS_MXFP4 : e->fp8_ready ? ZE_WEIGHTS_FP8 : ZE_WEIGHTS_BF16;
}

extern "C" int ze_set_fp8_activations(ze_engine* e, int on) {
    if (!e) return ze_fail(e, ZE_ERR_INVALID, "null engine");
    if (on && !e->fp8_ready)
        return ze_fail(e, ZE_ERR_INVALID, "fp8 activations go with fp8 weights: call ze_weights_quantize_fp8 first");
    if (e->fp8_act != (on != 0)) {
        e->fp8_act = on != 0;
        ++ze_tune_epoch;  // captured decode steps bake the choice of kernels in
        ze_prefix_weights_changed(e);   // (the passes compute other K/V rows from now on)
    }
    return ZE_OK;
}

extern "C" int ze_op_linear_mx(ze_engine* e, const void* a8, const void* sa, const void* w8, const void* sw, const void* bias,
                               void* cmat, int M, int N, int K, int swiglu, void* stream) {
    if (!e || !a8 || !sa || !w8 || !sw || !cmat || M <= 0 || N <= 0 || K <= 0)
        return ze_fail(e, ZE_ERR_INVALID, "null pointer or empty shape");
    if (K % 128 != 0 || K < 256 || (swiglu && N % 32 != 0))
        return ze_fail(e, ZE_ERR_INVALID, "K must be a multiple of 128 (>= 256); with swiglu N a multiple of 32");
    hipSetDevice(e->device);
    if (!ze_launch_gemm_mx(swiglu ? ZE_EPI_SWIGLU : ZE_EPI_NONE, (const uint8_t*)a8, K, (const float*)sa, (const uint8_t*)w8, K,
                           (const float*)sw, (const bf16_t*)bias, (bf16_t*)cmat, swiglu ? N / 2 : N, M, N, K, (hipStream_t)stream))
        return ze_fail(e, ZE_ERR_INVALID, "shape not supported by the block-scaled kernel");
    ZE_KCHECK();
    return ZE_OK;
}

extern "C" int ze_op_quantize_fp8(ze_engine* e, void* w_bf16, int rows, int cols, void* q_out, void* scale_out,
                                  void* stream) {
    if (!e || !w_bf16 || !q_out || !scale_out || rows <= 0 || cols <= 0 || cols % 16)
        return ze_fail(e, ZE_ERR_INVALID, "bad argument (cols must be a multiple of 16)");
    hipSetDevice(e->device);
    ze_launch_quantize_rows((bf16_t*)w_bf16, rows, cols, cols, (uint8_t*)q_out, cols, (float*)scale_out, (hipStream_t)stream);
    ZE_KCHECK();
    return ZE_OK;
}

extern "C" int ze_set_decode_regime(ze_engine* e, int regime) {
    if (!e || regime < -1 || regime > 1) return ze_fail(e, ZE_ERR_INVALID, "regime is -1 (by capacity), 0 (fragment kernels) or 1 (row streaming)");
    if (regime != e->decode_regime) {
        const bool was = e->wide_regime();
        e->decode_regime = regime;
        if (was != e->wide_regime()) {
            e->frag_ready = false;         // the other family's weight copies are built on its first step
            ze_prefix_weights_changed(e);  // (rows the decode steps wrote are the other family's, equal within bf16 rounding only)
        }
        ++ze_tune_epoch;  // captured batched steps bake the kernel family in
    }
    return e->wide_regime() ? 1 : 0;
}

// ================================================================== measurement
extern "C" int ze_tune(int knob, int value) {
    if (knob < 0 || knob >= 25) return ze_fail(nullptr, ZE_ERR_INVALID, "unknown knob");
    ze_gemv_knobs[knob] = value;
    ++ze_tune_epoch;  // captured decode steps bake the launch policy in: engines drop their graphs on the next use
    return ZE_OK;
}
// The numeric helpers every epilogue of the library shares (ze_common.h: f32_to_bf16 / pack_bf16x2 = v_cvt_pk_bf16_f32, silu_f =
// x * v_rcp_f32(1 + v_exp_f32(-x))), alone: out[i] = bf16(x[i]) | bf16(bf16(silu(x[i])) * y[i]) << 16, out2[i] = pack(x[i], y[i]).
extern "C" int ze_op_numeric_helpers(ze_engine* e, const float* x, const float* y, uint32_t* out, uint32_t* out2, int n, void* stream) {
    if (!e || !x || !y || !out || !out2 || n < 0) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    hipSetDevice(e->device);
    ze_launch_numeric_helpers(x, y, out, out2, n, (hipStream_t)stream);
    ZE_KCHECK();
    return ZE_OK;
}

// The image side of the engine: the front-end entry points (tile upload, Pillow-exact crop + bicubic resize, patchify, the index
// helpers of the C ABI) and the ViT forward pass.  The kernels: ze_frontend.hip, ze_attention.hip, ze_gemm.hip.
#include <math.h>
#include <string.h>

#include "ze_engine.h"

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
int build_tiles(const int32_t* cu, int n_seg, int* out /* int4 rows */, int cap_tiles, int bq) {
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
    const int bq_full = ze_knobs[ZE_KNOB_GATE_UP_FLASH] == ZE_FLASH_BQ64 ? 64 : ZE_FA_BQ_LONG;
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

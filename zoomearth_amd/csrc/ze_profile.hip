// Measurement entries: the kernels of the forward passes, alone, between HIP events on the caller's stream.  Nothing here chooses
// a launcher: every projection goes through the function the pass itself calls (ze_forward.hip: gemv_args_of, prefill_projection;
// ze_decode_batch.hip: the batch_* launches), so a profiler times what the pass runs.
#include <string.h>

#include <vector>

#include "ze_engine.h"

// `warm` warm-up launches, then `iters` launches between two events on s; avg_us = the average launch duration
template <typename F>
static int time_launches(ze_engine* e, hipStream_t s, int warm, int iters, F launch, float* avg_us) {
    hipEvent_t a = nullptr, b = nullptr;
    float ms = 0.f;
    const int r = [&]() -> int {
        ZE_HIP(hipEventCreate(&a));
        ZE_HIP(hipEventCreate(&b));
        for (int i = 0; i < warm; ++i) launch(i);
        ZE_HIP(hipEventRecord(a, s));
        for (int i = 0; i < iters; ++i) launch(i);
        ZE_HIP(hipEventRecord(b, s));
        ZE_HIP(hipEventSynchronize(b));
        ZE_HIP(hipEventElapsedTime(&ms, a, b));
        ZE_KCHECK();
        return ZE_OK;
    }();
    if (a) hipEventDestroy(a);
    if (b) hipEventDestroy(b);
    if (r == ZE_OK) *avg_us = ms * 1000.0f / (float)iters;
    return r;
}

// algorithmic bytes of a weight matrix as launch `g` streams it: bf16, the FP8 copy (1 byte per weight + one fp32 scale per row), or
// the MXFP4 copy (half a byte per weight + one scale byte per 32 weights)
static double weight_bytes(double rows, double cols, bool fp8) { return fp8 ? rows * cols + rows * 4.0 : rows * cols * 2.0; }
static double weight_bytes(double rows, double cols, const ze_gemv_args& g) {
    if (g.W4) return rows * cols * 0.5 + rows * cols / 32.0;
    return weight_bytes(rows, cols, g.W8 != nullptr);
}

// The weight-streaming kernels of the SINGLE-CHAIN decode step (chain slot 0), one kind per call, with the arguments
// ze_enqueue_decode_step gives them: a quantised engine streams its FP8 or MXFP4 copy, with FP8 activations where the step has them.
extern "C" int ze_profile_decode_kernel(ze_engine* e, int which, int iters, float* avg_us, double* bytes_per_launch,
                                        void* stream) {
    if (!e || !avg_us || !bytes_per_launch || iters <= 0) return ze_fail(e, ZE_ERR_INVALID, "bad argument");
    const ze_config& c = e->cfg;
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    const int H = c.hidden, nq = c.heads * e->head_dim, nqkv = nq + 2 * c.kv_heads * e->head_dim, ip = e->text_ipad;
    ZE_HIP(hipMemsetAsync(e->dh, 0, (size_t)H * 2, s));
    ZE_HIP(hipMemsetAsync(e->dattn, 0, (size_t)nq * 2, s));
    ZE_HIP(hipMemsetAsync(e->dact, 0, (size_t)ip * 2, s));
    double bytes = 0;
    auto launch = [&](int it) {
        const int li = it % c.layers;
        const ze_text_layer& L = e->tl[li];
        ze_gemv_args g;
        switch (which) {
            case 0:
                g = gemv_args_of(e, L.qkv, nqkv, H, e->dh);
                g.norm_w = L.in_norm; g.eps = c.rms_eps; g.bias = L.qkv.bias; g.out_bf16 = e->dq; g.st = e->st_dev; g.cosT = e->cosT;
                g.sinT = e->sinT; g.kcache = e->kc(li, 0); g.vcache = e->vc(li, 0);
                g.heads = c.heads; g.kv_heads = c.kv_heads; g.max_ctx = c.max_ctx; g.act8 = e->fp8_act ? 1 : 0;
                bytes = weight_bytes(nqkv, H, g);
                ze_launch_gemv(ZE_GV_QKV_ROPE, g, s);
                break;
            case 1:
                g = gemv_args_of(e, L.o, H, nq, e->dattn);
                g.out_bf16 = e->dh;
                bytes = weight_bytes(H, nq, g);
                ze_launch_gemv(ZE_GV_RESIDUAL, g, s);
                break;
            case 2:
                g = gemv_args_of(e, L.gate_up, 2 * ip, H, e->dh);
                g.norm_w = L.post_norm; g.eps = c.rms_eps; g.out_bf16 = e->dact; g.act8 = e->fp8_act ? 1 : 0;
                bytes = weight_bytes(2.0 * c.intermediate, H, g);
                ze_launch_gemv(ZE_GV_SWIGLU, g, s);
                break;
            case 3:
                g = gemv_args_of(e, L.down, H, ip, e->dact);
                g.out_bf16 = e->dh;
                bytes = weight_bytes(H, c.intermediate, g);
                ze_launch_gemv(ZE_GV_RESIDUAL, g, s);
                break;
            default:
                g = gemv_args_of(e, lm_head_linear(e, true), c.vocab, H, e->dh);
                g.norm_w = e->final_norm; g.eps = c.rms_eps; g.out_f32 = e->dlogits;
                bytes = weight_bytes(c.vocab, H, g);
                ze_launch_gemv(ZE_GV_LOGITS, g, s);
                break;
        }
    };
    ZE_TRY(time_launches(e, s, std::min(iters, 4), iters, launch, avg_us));
    *bytes_per_launch = bytes;
    return ZE_OK;
}

// The kernels of the BATCHED decode step (ze_decode_batch / ze_decode_burst) at n chains (slots 0..n-1, with whatever
// context they hold), one kind per call, cycling through the layers' real weights and KV caches, bracketed by HIP events
// on `stream`.  which: 0 qkv, 1 o_proj, 2 gate_up (SwiGLU), 3 down, 4 lm_head, 5 decode attention, 6 RMSNorm,
// 7 rope + KV append.  bytes_per_launch = algorithmic bytes: the weight matrix (0-4), the K/V rows of the n chains (5),
// the activation rows read + written (6, 7).
// Cases 0-6 call the step's own launch functions: on a quantised engine they stream (and count) the FP8 fragments the step streams.
extern "C" int ze_profile_batch_kernel(ze_engine* e, int which, int n, int iters, float* avg_us, double* bytes_per_launch,
                                       void* stream) {
    if (!e || !avg_us || !bytes_per_launch || iters <= 0 || n <= 0 || n > e->cfg.max_seqs || (n > 64 && !e->wide_regime()))
        return ze_fail(e, ZE_ERR_INVALID, "bad argument");
    const ze_config& c = e->cfg;
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    ZE_TRY(ensure_fragments(e, s));
    const int H = c.hidden, hd = e->head_dim, nq = c.heads * hd, nkv = c.kv_heads * hd, nqkv = nq + 2 * nkv;
    std::vector<int> seqs(n);
    double kv_bytes = 0;
    for (int i = 0; i < n; ++i) {
        seqs[i] = i;
        kv_bytes += (double)(std::min(e->ctx_host[i] + 1, c.max_ctx)) * nkv * 2 * 2;
    }
    stage_batch(e, seqs.data(), n, 1, s);  // (the row table, the hints, the mates and the grid a decode step of these chains would launch)
    const ze_step_rows rows = ze_rows_own(e);
    double bytes = 0;
    auto launch = [&](int it) {
        const int li = it % c.layers;
        switch (which) {
            case 0: bytes = weight_bytes(nqkv, H, batch_qkv(e, rows, li, n, s)); break;
            case 1: bytes = weight_bytes(H, nq, batch_o(e, rows, li, n, s)); break;
            case 2: bytes = weight_bytes(2.0 * c.intermediate, H, batch_gate_up(e, rows, li, n, s)); break;
            case 3: bytes = weight_bytes(H, c.intermediate, batch_down(e, rows, li, n, s)); break;
            case 4: bytes = weight_bytes(c.vocab, H, batch_lm_head(e, rows, li, n, s)); break;
            case 5:
                batch_attention(e, rows, li, n, s);
                bytes = kv_bytes;
                break;
            case 6:
                batch_norm(e, rows, li, n, ZE_NORM_IN, s);
                bytes = (double)n * H * 2 * 2;
                break;
            default:
                ze_launch_rope_kv_batch(e->bqkv, n, c.heads, c.kv_heads, hd, e->cosT, e->sinT, e->st_dev, rows.seq, e->kc(li, 0),
                                        e->vc(li, 0), (size_t)c.kv_heads * c.max_ctx * hd, c.max_ctx, s);
                bytes = (double)n * nqkv * 2 * 2;
                break;
        }
    };
    ZE_TRY(time_launches(e, s, std::min(iters, 4), iters, launch, avg_us));
    *bytes_per_launch = bytes;
    return ZE_OK;
}

// what the prefill profilers share: the argument check, the scratch rows, flops[which] = 2 x rows x N x K of the real shape
static int prefill_profile_setup(ze_engine* e, int rows, double flops[4]) {
    const ze_config& c = e->cfg;
    const int H = c.hidden, nq = c.heads * e->head_dim, nqkv = nq + 2 * c.kv_heads * e->head_dim;
    if (nqkv < H) return ze_fail(e, ZE_ERR_INVALID, "scratch rows too short for this shape");
    flops[ZE_PROJ_QKV] = 2.0 * rows * nqkv * H;
    flops[ZE_PROJ_O] = 2.0 * rows * H * nq;
    flops[ZE_PROJ_GATE_UP] = 2.0 * rows * 2.0 * c.intermediate * H;
    flops[ZE_PROJ_DOWN] = 2.0 * rows * H * c.intermediate;
    return ZE_OK;
}
// projection `which` of layer li (in rotation) as the pass launches it, minus the norm, its output in scratch: qkv and gate/up
// where the pass puts them, o and down into the qkv rows instead of the residual stream
static void profile_prefill_projection(ze_engine* e, int li, int which, int rows, hipStream_t s) {
    const int nqkv = (e->cfg.heads + 2 * e->cfg.kv_heads) * e->head_dim;
    const bool gate_up = which == ZE_PROJ_GATE_UP;
    prefill_projection(e, e->tl[li % e->cfg.layers], which, rows, false, gate_up ? e->ta : e->tqkv, gate_up ? e->text_ipad : nqkv, s);
}

// The projections of a PREFILL pass, one kind per call, on the pass's own operands: the engine's layer weights in rotation and the
// activation rows the last ze_prefill_batch / ze_prefill left in the workspace (normalised hidden rows, attention output, SwiGLU
// output of its last layer -- rows beyond that pass hold older passes' rows or zeros), through the launcher the pass uses
// (ze_launch_gemm: k_gemm_p8 from ~1.5 K rows on).  which: 0 qkv, 1 o_proj (+ residual), 2 gate_up (SwiGLU), 3 down (+ residual).
// Outputs go to scratch rows (the residual stream is read, never written).  flops_per_launch = 2 x rows x N x K of the real shape.
extern "C" int ze_profile_prefill_kernel(ze_engine* e, int which, int rows, int iters, float* avg_us, double* flops_per_launch,
                                         void* stream) {
    if (!e || !avg_us || !flops_per_launch || iters <= 0 || rows <= 0 || rows > e->prefill_rows || which < 0 || which > 3)
        return ze_fail(e, ZE_ERR_INVALID, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    double flops[4];
    ZE_TRY(prefill_profile_setup(e, rows, flops));
    ZE_TRY(time_launches(e, s, std::min(iters, 3), iters, [&](int it) { profile_prefill_projection(e, it, which, rows, s); }, avg_us));
    *flops_per_launch = flops[which];
    return ZE_OK;
}

// The four projections of a prefill layer in PASS ORDER (qkv, o, gate/up, down; layer after layer, as ze_prefill_batch issues them --
// minus the norm / rope / attention launches between them), every launch bracketed by its own pair of HIP events: per-projection
// averages under the clocks and cache state a pass gives them (twelve back-to-back launches of ONE projection run 5-9 % slower than
// the same kernel inside a pass: rocprofv3 of the replayed pass, profiles/r06_prefill_by_shape.csv).  Operands as
// ze_profile_prefill_kernel.  avg_us / flops: [0] qkv, [1] o, [2] gate/up, [3] down.
extern "C" int ze_profile_prefill_layer(ze_engine* e, int rows, int layers_run, float avg_us[4], double flops[4], void* stream) {
    if (!e || !avg_us || !flops || layers_run <= 0 || layers_run > 256 || rows <= 0 || rows > e->prefill_rows)
        return ze_fail(e, ZE_ERR_INVALID, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    hipSetDevice(e->device);
    ZE_TRY(prefill_profile_setup(e, rows, flops));
    std::vector<hipEvent_t> ev((size_t)layers_run * 8, nullptr);
    double sum[4] = {0, 0, 0, 0};
    const int r = [&]() -> int {
        for (auto& x : ev) ZE_HIP(hipEventCreate(&x));
        for (int li = 0; li < 2; ++li)   // warm-up
            for (int w = 0; w < 4; ++w) profile_prefill_projection(e, li, w, rows, s);
        for (int li = 0; li < layers_run; ++li)
            for (int w = 0; w < 4; ++w) {
                ZE_HIP(hipEventRecord(ev[(size_t)(li * 4 + w) * 2], s));
                profile_prefill_projection(e, li, w, rows, s);
                ZE_HIP(hipEventRecord(ev[(size_t)(li * 4 + w) * 2 + 1], s));
            }
        ZE_HIP(hipStreamSynchronize(s));
        for (int li = 0; li < layers_run; ++li)
            for (int w = 0; w < 4; ++w) {
                float ms = 0.f;
                ZE_HIP(hipEventElapsedTime(&ms, ev[(size_t)(li * 4 + w) * 2], ev[(size_t)(li * 4 + w) * 2 + 1]));
                sum[w] += ms;
            }
        ZE_KCHECK();
        return ZE_OK;
    }();
    for (auto& x : ev)
        if (x) hipEventDestroy(x);
    ZE_TRY(r);
    for (int w = 0; w < 4; ++w) avg_us[w] = (float)(sum[w] * 1000.0 / layers_run);
    return ZE_OK;
}

// Decode weight formats of the engine: the FP8 and MXFP4 quantisation of the text weights, the switches that go with them (FP8
// activations, the decode regime of the batched step) and ze_tune, the one writer of the measurement knobs (ze_knobs.h).
#include "ze_engine.h"

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
    if (knob < 0 || knob >= ZE_KNOB_COUNT) return ze_fail(nullptr, ZE_ERR_INVALID, "unknown knob");
    ze_knobs[knob] = value;
    ++ze_tune_epoch;  // captured decode steps bake the launch policy in: engines drop their graphs on the next use
    return ZE_OK;
}

// The unit ops of the C ABI (ze_op_*, ze_fragment_bytes): one kernel or launcher each on the caller's operands, for the tests and the
// tools -- nothing in the product path calls them.  (ze_op_crop_resize and ze_op_patchify, which the product path does call, are in
// ze_vision.hip; the ops of a feature unit -- beam, LoRA, spec, grammar -- are in that unit.)
#include <math.h>
#include <cmath>
#include <string.h>

#include "ze_engine.h"

// A device table for the length of one call: `words` 4-byte words are allocated and the first `n` copied from `host`, launch(table)
// enqueues on s what reads it, the stream is drained and the table freed.  The first error; `what` = the message of a failed launch.
template <typename F>
static int with_scratch_table(ze_engine* e, const void* host, size_t n, size_t words, hipStream_t s, const char* what, F launch) {
    int32_t* dev = nullptr;
    ZE_HIP(hipMalloc((void**)&dev, words * sizeof(int32_t)));
    int r = ZE_OK;
    if (hipMemcpyAsync(dev, host, n * sizeof(int32_t), hipMemcpyHostToDevice, s) != hipSuccess) r = ze_fail(e, ZE_ERR_HIP, "hipMemcpyAsync failed");
    if (r == ZE_OK) launch(dev);
    if (r == ZE_OK && hipGetLastError() != hipSuccess) r = ze_fail(e, ZE_ERR_HIP, what);
    if (hipStreamSynchronize(s) != hipSuccess && r == ZE_OK) r = ze_fail(e, ZE_ERR_HIP, "hipStreamSynchronize failed");
    hipFree(dev);
    return r;
}

// The selection alone, on caller-supplied rows (any vocab / ld, a filter and a temperature per row, no repetition penalty): the filter of
// every row and, with the entropy filters given (typical_p non-null), its band behind it
static int op_sample_select(ze_engine* e, const float* logits, int rows, int vocab, int ld, const float* temperature, const int32_t* top_k,
                            const float* top_p, const float* min_p, const float* typical_p, const float* epsilon_cutoff, const float* eta_cutoff,
                            float* out_cut, float* out_ceil, int32_t* out_kept, void* stream) {
    if (rows <= 0 || vocab <= 0 || ld < vocab) return ze_fail(e, ZE_ERR_INVALID, "rows and vocab must be positive, ld >= vocab");
    std::vector<float> table((size_t)rows * (typical_p ? 8 : 4));  // the filter table, then the entropy-filter table
    for (int r = 0; r < rows; ++r) {
        if (!(temperature[r] > 0.f)) return ze_fail(e, ZE_ERR_INVALID, "temperature must be positive");
        ZE_TRY(ze_check_filter(e, top_k[r], top_p[r], min_p[r]));
        float* f = &table[4 * (size_t)r];
        memcpy(f, &top_k[r], sizeof(int));
        f[1] = top_p[r], f[2] = min_p[r], f[3] = temperature[r];
        if (!typical_p) continue;
        ZE_TRY(ze_check_entropy_filter(e, typical_p[r], epsilon_cutoff[r], eta_cutoff[r]));
        float* g = &table[4 * ((size_t)rows + r)];
        g[0] = typical_p[r], g[1] = epsilon_cutoff[r], g[2] = eta_cutoff[r], g[3] = temperature[r];
    }
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    return with_scratch_table(e, table.data(), table.size(), table.size(), s, "selection kernel launch failed", [&](int32_t* words) {
        const float* dev = (const float*)words;
        ze_launch_sample_filter(logits, vocab, ld, nullptr, nullptr, 0, rows, 1.0f, 1.0f, dev, out_cut, out_kept, nullptr, s);
        if (typical_p)
            ze_launch_sample_band(logits, vocab, ld, nullptr, nullptr, 0, rows, 1.0f, 1.0f, dev + 4 * (size_t)rows, out_cut, out_cut, out_ceil,
                                  out_kept, nullptr, s);
    });
}

extern "C" int ze_op_sample_filter(ze_engine* e, const float* logits, int rows, int vocab, int ld, const float* temperature, const int32_t* top_k,
                                   const float* top_p, const float* min_p, float* out_cut, int32_t* out_kept, void* stream) {
    if (!e || !logits || !temperature || !top_k || !top_p || !min_p || !out_cut) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    return op_sample_select(e, logits, rows, vocab, ld, temperature, top_k, top_p, min_p, nullptr, nullptr, nullptr, out_cut, nullptr, out_kept, stream);
}

// The whole warper chain's selection (unit op: the filter of every row, then its band)
extern "C" int ze_op_sample_band(ze_engine* e, const float* logits, int rows, int vocab, int ld, const float* temperature, const int32_t* top_k,
                                 const float* top_p, const float* min_p, const float* typical_p, const float* epsilon_cutoff, const float* eta_cutoff,
                                 float* out_cut, float* out_ceil, int32_t* out_kept, void* stream) {
    if (!e || !logits || !temperature || !top_k || !top_p || !min_p || !typical_p || !epsilon_cutoff || !eta_cutoff || !out_cut || !out_ceil)
        return ze_fail(e, ZE_ERR_INVALID, "null argument");
    return op_sample_select(e, logits, rows, vocab, ld, temperature, top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff, out_cut, out_ceil,
                            out_kept, stream);
}

// One draw per caller row with a (temperature | greedy, penalty, seed, stream, index) of its own: the per-chain kernels of
// ze_sample.hip with row = slot, on tables built for the call
static int op_sample_rows(ze_engine* e, const float* logits, int rows, int vocab, int ld, const uint8_t* seen, const float* temperature,
                          const float* repetition_penalty, const uint64_t* seed, const int32_t* sample_stream, const int32_t* index,
                          const int32_t* top_k, const float* top_p, const float* min_p, const float* band_cut, const float* band_ceil,
                          int32_t* out_tokens, void* stream) {
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
    return with_scratch_table(e, host.data(), host.size(), words, s, "sampling kernel launch failed", [&](int32_t* dev) {
        ze_launch_sample_rows(logits, vocab, ld, seen, reinterpret_cast<const ze_seq_dev*>(dev + o_st), dev + o_ids, rows,
                              reinterpret_cast<const ze_chain_sampling*>(dev + o_samp), draws,
                              filters ? reinterpret_cast<const float*>(dev + o_filt) : nullptr,
                              filters || band_cut ? reinterpret_cast<float*>(dev + o_cut) : nullptr,
                              band_cut ? reinterpret_cast<float*>(dev + o_ceil) : nullptr, reinterpret_cast<float*>(dev + o_part), reinterpret_cast<float*>(dev + o_sum), out_tokens, s);
    });
}

extern "C" int ze_op_sample_rows(ze_engine* e, const float* logits, int rows, int vocab, int ld, const uint8_t* seen, const float* temperature,
                                 const float* repetition_penalty, const uint64_t* seed, const int32_t* sample_stream, const int32_t* index,
                                 const int32_t* top_k, const float* top_p, const float* min_p, int32_t* out_tokens, void* stream) {
    return op_sample_rows(e, logits, rows, vocab, ld, seen, temperature, repetition_penalty, seed, sample_stream, index, top_k, top_p,
                          min_p, nullptr, nullptr, out_tokens, stream);
}

// ... under a band per row as ze_op_sample_band (or anyone) found it: the _band draw kernels alone
extern "C" int ze_op_sample_rows_band(ze_engine* e, const float* logits, int rows, int vocab, int ld, const uint8_t* seen, const float* temperature,
                                      const float* repetition_penalty, const uint64_t* seed, const int32_t* sample_stream, const int32_t* index,
                                      const float* cut, const float* ceil, int32_t* out_tokens, void* stream) {
    if (!cut || !ceil) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    return op_sample_rows(e, logits, rows, vocab, ld, seen, temperature, repetition_penalty, seed, sample_stream, index, nullptr,
                          nullptr, nullptr, cut, ceil, out_tokens, stream);
}

// one sampling step on caller-supplied logits; `index` plays the role of the generated-token index of the draw
static int op_sample(ze_engine* e, int seq, const float* logits, float repetition_penalty, const ze_sample_opts& so, int index, int32_t* out_token,
                     hipStream_t s) {
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

extern "C" int ze_op_sample_greedy(ze_engine* e, int seq, const float* logits, float repetition_penalty, int32_t* out_token, void* stream) {
    return op_sample(e, seq, logits, repetition_penalty, ze_sample_opts{}, 0, out_token, (hipStream_t)stream);
}

extern "C" int ze_op_sample_temperature(ze_engine* e, int seq, const float* logits, float repetition_penalty, float temperature, uint64_t seed,
                                        int index, int32_t* out_token, void* stream) {
    if (!(temperature > 0.f)) return ze_fail(e, ZE_ERR_INVALID, "temperature must be positive");
    ze_sample_opts so;
    so.temperature = temperature;
    so.seed = seed;
    so.slot = seq;
    if (check_seq(e, seq) == 0) ze_attach_filters(e, so, false);
    return op_sample(e, seq, logits, repetition_penalty, so, index, out_token, (hipStream_t)stream);
}

// ================================================================== unit ops
extern "C" int ze_op_logit_adjust(ze_engine* e, const float* logits, int rows, int vocab, int ld, const uint16_t* counts, const float* presence,
                                  const float* frequency, const int32_t* eos_masked, const int32_t* bias_offsets, const int32_t* bias_ids,
                                  const float* bias_vals, float* out, void* stream) {
    if (!e || !logits || !presence || !frequency || !eos_masked || !bias_offsets || !out || out == logits)
        return ze_fail(e, ZE_ERR_INVALID, "bad logit_adjust arguments");
    if (rows < 0 || vocab <= 0 || ld < vocab) return ze_fail(e, ZE_ERR_INVALID, "rows >= 0, vocab > 0 and ld >= vocab");
    hipSetDevice(e->device);
    ze_launch_logit_adjust(logits, rows, vocab, ld, counts, presence, frequency, eos_masked, bias_offsets, bias_ids, bias_vals, e->eos_dev,
                           e->cfg.n_eos, out, (hipStream_t)stream);
    ZE_KCHECK();
    return ZE_OK;
}

extern "C" int ze_op_token_rules(ze_engine* e, const float* logits, int rows, int vocab, int ld, const int32_t* hist_ids, const int32_t* hist_offsets,
                                 const int32_t* n_context, const int32_t* no_repeat_ngram, const int32_t* ban_seqs, const int32_t* ban_offsets,
                                 const int32_t* stop_seqs, const int32_t* stop_offsets, const int32_t* min_new, float* out_rows, int32_t* out_stop,
                                 void* stream) {
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

extern "C" int ze_op_token_logprobs(ze_engine* e, const float* logits, int rows, int vocab, int ld, const int32_t* targets, int top_n,
                                    float* out_logprob, int32_t* out_top_ids, float* out_top_logprobs, void* stream) {
    if (!e || !logits || !targets || !out_logprob || rows < 0 || vocab <= 0 || ld < vocab)
        return ze_fail(e, ZE_ERR_INVALID, "bad token_logprobs arguments");
    if (top_n < 0 || top_n > ZE_MAX_TOP_LOGPROBS) return ze_fail(e, ZE_ERR_INVALID, "top_n must be in [0, 20]");
    if (top_n > 0 && (!out_top_ids || !out_top_logprobs)) return ze_fail(e, ZE_ERR_INVALID, "null top arrays");
    hipSetDevice(e->device);
    ze_launch_token_logprobs(logits, rows, vocab, ld, targets, top_n, out_logprob, out_top_ids, out_top_logprobs, (hipStream_t)stream);
    ZE_KCHECK();
    return ZE_OK;
}

// The fragment-major kernels of the batched decode step (the skinny frag kernel, or the sixteen-wave one-shot kernel of the qkv / o
// projections) on row-major operands, packed for the call: A [M, K] and W [N, K] bf16 -- or, with q4, the MXFP4 stream q4 / scale4 as
// ze_op_quantize_mxfp4 writes it.  The kernels read whole 16-row tiles, 1, 2 or 4 of them (dispatch_mt): M rounds up to 16, 32 or 64.
static int op_gemm_frag(ze_engine* e, bool oneshot, int epi, const bf16_t* A, int lda, const bf16_t* W, int ldw, const uint8_t* q4,
                        const uint8_t* scale4, const bf16_t* B, const bf16_t* R, int ldr, bf16_t* C, int ldc, int M, int N, int K, hipStream_t s) {
    const size_t mp = M <= 16 ? 16 : M <= 32 ? 32 : 64;
    const size_t xbytes = mp * K * sizeof(bf16_t), codes = (size_t)N * K / 2, scales = (size_t)N * K / 32;
    uint8_t* buf = nullptr;  // activation fragments, then the weight fragments: bf16, or the codes and then the scales
    ZE_HIP(hipMalloc((void**)&buf, xbytes + (q4 ? codes + scales : (size_t)N * K * sizeof(bf16_t))));
    bf16_t* xf = (bf16_t*)buf;
    uint8_t *wf = buf + xbytes, *sf4 = q4 ? wf + codes : nullptr;
    ze_launch_pack_fragments(A, lda, M, K, xf, s);
    if (q4) ze_launch_pack_fragments4(q4, scale4, N, K, wf, sf4, s);
    else ze_launch_pack_fragments(W, ldw, N, K, (bf16_t*)wf, s);
    if (oneshot) ze_launch_gemm_oneshot(epi, xf, (const bf16_t*)wf, B, R, ldr, C, ldc, M, N, K, s, nullptr, nullptr, sf4);
    else ze_launch_gemm_frag(epi, xf, (const bf16_t*)wf, B, R, ldr, C, ldc, M, N, K, s, nullptr, nullptr, sf4);
    hipError_t le = hipGetLastError();
    hipStreamSynchronize(s);
    hipFree(buf);
    if (le != hipSuccess) return ze_fail(e, ZE_ERR_HIP, hipGetErrorString(le));
    return ZE_OK;
}

// launcher 0 .. 6 of ze_op_gemm on operands its callers have checked
static int op_gemm_launch(ze_engine* e, int launcher, int epi, const bf16_t* A, int lda, const bf16_t* W, int ldw, const bf16_t* B, const bf16_t* R,
                          int ldr, bf16_t* C, int ldc, const int32_t* c_rows, int M, int N, int K, hipStream_t s) {
    switch (launcher) {
        case 0: ze_launch_gemm(epi, A, lda, W, ldw, B, R, ldr, C, ldc, c_rows, M, N, K, s, e->prefill_ws()); break;
        case 1: ze_launch_gemm(epi, A, lda, W, ldw, B, R, ldr, C, ldc, c_rows, M, N, K, s); break;
        case 2: ze_launch_gemm_p8(epi, A, lda, W, ldw, B, R, ldr, C, ldc, c_rows, M, N, K, s, e->prefill_ws()); break;
        case 3: ze_launch_gemm_stream(epi, A, lda, W, ldw, B, R, ldr, C, ldc, M, N, K, e->gemm_ws(), s); break;
        case 4: ze_launch_gemm_wide(epi, A, lda, W, ldw, B, R, ldr, C, ldc, M, N, K, e->gemm_ws(), s); break;
        default: return op_gemm_frag(e, launcher == 6, epi, A, lda, W, ldw, nullptr, nullptr, B, R, ldr, C, ldc, M, N, K, s);
    }
    ZE_KCHECK();
    return ZE_OK;
}

// C = act(A W^T + bias) on packed operands (lda = ldw = K): `act` is the older spelling of ze_op_gemm's (launcher, epilogue) pair.
// With a SwiGLU epilogue C is [M, N / 2]; act 10 writes fp32 and takes no bias.
extern "C" int ze_op_linear(ze_engine* e, const void* a, const void* w, const void* bias, void* cmat, int M, int N, int K, int act, void* stream) {
    static const int form[11][2] = {{0, ZE_EPI_NONE}, {0, ZE_EPI_GELU}, {3, ZE_EPI_NONE}, {5, ZE_EPI_NONE}, {0, ZE_EPI_SWIGLU}, {6, ZE_EPI_NONE},
                                    {4, ZE_EPI_NONE}, {4, ZE_EPI_SWIGLU}, {2, ZE_EPI_NONE}, {2, ZE_EPI_SWIGLU}, {4, ZE_EPI_F32}};
    if (!e || !a || !w || !cmat) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (K % 8) return ze_fail(e, ZE_ERR_INVALID, "K must be a multiple of 8");
    const bool known = act >= 0 && act <= 10;  // (any other act has always been act 1)
    const int launcher = known ? form[act][0] : 0, epi = known ? form[act][1] : ZE_EPI_GELU;
    if (launcher >= 5 && (M > 64 || N % 16 || K % 32 || K > 4096)) return ze_fail(e, ZE_ERR_INVALID, "fragment path: M <= 64, N % 16, K % 32, K <= 4096");
    if (epi == ZE_EPI_SWIGLU && N % 32) return ze_fail(e, ZE_ERR_INVALID, "SwiGLU: N = 2 * width with width % 16 == 0");
    if (launcher == 2 && (K % 64 || K < 64)) return ze_fail(e, ZE_ERR_INVALID, "eight-phase kernel: K a multiple of 64");
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    const bf16_t *A = (const bf16_t*)a, *W = (const bf16_t*)w, *B = act == 10 ? nullptr : (const bf16_t*)bias;
    const int ldc = epi == ZE_EPI_SWIGLU ? N / 2 : N;
    if (M == 1 && act == 0 && N % 2 == 0) {  // one row: the single-chain GEMV first, where it takes the shape
        ze_gemv_args g;
        memset(&g, 0, sizeof(g));
        g.W = W, g.ldw = K, g.N = N, g.K = K, g.D = 128;
        g.x = A, g.bias = B, g.out_bf16 = (bf16_t*)cmat;
        if (!ze_launch_gemv(ZE_GV_PLAIN, g, s)) return op_gemm_launch(e, 1, epi, A, K, W, K, B, nullptr, 0, (bf16_t*)cmat, ldc, nullptr, M, N, K, s);
        ZE_KCHECK();
        return ZE_OK;
    }
    return op_gemm_launch(e, launcher, epi, A, K, W, K, B, nullptr, 0, (bf16_t*)cmat, ldc, nullptr, M, N, K, s);
}

// The public GEMM launchers with the operands the engine gives them: leading dimensions of their own, the residual epilogue, the output
// row table (tests/test_gpu_gemm_operands.py).  Everything a launcher would not take is refused here, before anything is launched.
extern "C" int ze_op_gemm(ze_engine* e, int launcher, int epi, const void* a, int lda, const void* w, int ldw, const void* bias, const void* r,
                          int ldr, void* cmat, int ldc, const int32_t* c_rows, int M, int N, int K, void* stream) {
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
    const bf16_t* R = epi == ZE_EPI_RESIDUAL ? (const bf16_t*)r : nullptr;
    return op_gemm_launch(e, launcher, epi, (const bf16_t*)a, lda, (const bf16_t*)w, ldw, (const bf16_t*)bias, R, R ? ldr : 0, (bf16_t*)cmat, ldc,
                          c_rows, M, N, K, (hipStream_t)stream);
}

// The W4 forms of the fragment launchers on one matrix: ze_op_gemm's launchers 5 / 6 with the MXFP4 stream as W (row-major q4 / scale
// as ze_op_quantize_mxfp4 writes them, packed by ze_launch_pack_fragments4).  tests/test_gpu_gemm4.py holds it against
// ze_op_gemm on the dequantised bf16 weights, bit for bit.
extern "C" int ze_op_gemm4(ze_engine* e, int launcher, int epi, const void* a, int lda, const void* q4, const void* scale_e8m0, const void* bias,
                           const void* r, int ldr, void* cmat, int ldc, int M, int N, int K, void* stream) {
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
    const bf16_t* R = epi == ZE_EPI_RESIDUAL ? (const bf16_t*)r : nullptr;
    return op_gemm_frag(e, launcher == 6, epi, (const bf16_t*)a, lda, nullptr, 0, (const uint8_t*)q4, (const uint8_t*)scale_e8m0, (const bf16_t*)bias,
                        R, R ? ldr : 0, (bf16_t*)cmat, ldc, M, N, K, (hipStream_t)stream);
}

extern "C" int ze_fragment_bytes(ze_engine* e, size_t* bytes) {
    if (!e || !bytes) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    *bytes = (e->frag_ready && !e->wide_regime()) ? e->arena_f_bytes + (e->fp8_ready ? e->arena_f8_bytes : 0) + e->arena_f4_bytes : 0;
    return ZE_OK;
}

extern "C" int ze_op_token_logprob(ze_engine* e, const void* logits, int rows, int vocab, int ld, const int32_t* targets, float* out, void* stream) {
    if (!logits || !targets || !out || rows < 0 || vocab <= 0 || ld < vocab || ld % 8)
        return ze_fail(e, ZE_ERR_INVALID, "bad token_logprob arguments");
    hipSetDevice(e->device);
    ze_launch_token_logprob((const bf16_t*)logits, ld, vocab, targets, out, rows, (hipStream_t)stream);
    ZE_KCHECK();
    return ZE_OK;
}

extern "C" int ze_op_score_detail(ze_engine* e, const void* logits, int rows, int vocab, int ld, const int32_t* targets, int top_n,
                                  float* out_logprob, float* out_entropy, int32_t* out_rank, int32_t* out_top_ids, float* out_top_logprobs,
                                  void* stream) {
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

extern "C" int ze_op_rmsnorm(ze_engine* e, const void* x, const void* weight, void* y, int rows, int cols, float eps, void* stream) {
    if (!e || !x || !weight || !y) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (cols % 8) return ze_fail(e, ZE_ERR_INVALID, "cols must be a multiple of 8");
    hipSetDevice(e->device);
    ze_launch_rmsnorm((const bf16_t*)x, cols, (const bf16_t*)weight, (bf16_t*)y, cols, rows, cols, eps,
                      (hipStream_t)stream);
    ZE_KCHECK();
    return ZE_OK;
}

extern "C" int ze_op_attention(ze_engine* e, const void* q, const void* k, const void* v, void* o, int T, int heads, int kv_heads, int D,
                               const int32_t* cu, int n_seg, int causal, void* stream) {
    if (!e || !q || !k || !v || !o || !cu) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (D != 80 && D != 128) return ze_fail(e, ZE_ERR_INVALID, "D must be 80 or 128");
    if (heads % kv_heads) return ze_fail(e, ZE_ERR_INVALID, "kv_heads must divide heads");
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> tiles((size_t)4 * (T / 64 + n_seg + 2));
    const int bq = ze_knobs[ZE_KNOB_GATE_UP_FLASH] == ZE_FLASH_BQ64 ? 64 : ZE_FA_BQ_LONG;  // (two query tiles per wave unless knob 1 = 9: the unit op covers both forms)
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
extern "C" int ze_op_window_gather(ze_engine* e, const float* pixel_values, const int32_t* grid_thw, int n_images, void* out_bf16, void* stream) {
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
extern "C" int ze_op_window_scatter(ze_engine* e, const void* x_bf16, int cols, const int32_t* grid_thw, int n_images, void* out_bf16, void* stream) {
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
extern "C" int ze_op_embed_scatter(ze_engine* e, const int32_t* input_ids, int len, const void* image_embeds, int n_image_rows, void* out_bf16,
                                   void* stream) {
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
                       float* out_f32, const uint8_t* seen, float penalty, int32_t* out_token, int seq, int layer, const void* embed, int token,
                       void* embed_out, void* stream) {
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

extern "C" int ze_op_gemv(ze_engine* e, int epi, const void* w_bf16, const void* w8, const void* scale8, const void* x_bf16, const void* norm_w,
                          float eps, const void* bias_bf16, int act8, int N, int K, void* out_bf16, float* out_f32, const uint8_t* seen,
                          float penalty, int32_t* out_token, int seq, int layer, const void* embed, int token, void* embed_out, void* stream) {
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
extern "C" int ze_op_logits_rows(ze_engine* e, const void* w_bf16, const void* norm_w, float eps, const void* x_bf16, float* out_f32, int n, int N,
                                 int K, void* stream) {
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

extern "C" int ze_op_linear_mx(ze_engine* e, const void* a8, const void* sa, const void* w8, const void* sw, const void* bias, void* cmat, int M,
                               int N, int K, int swiglu, void* stream) {
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

extern "C" int ze_op_quantize_fp8(ze_engine* e, void* w_bf16, int rows, int cols, void* q_out, void* scale_out, void* stream) {
    if (!e || !w_bf16 || !q_out || !scale_out || rows <= 0 || cols <= 0 || cols % 16)
        return ze_fail(e, ZE_ERR_INVALID, "bad argument (cols must be a multiple of 16)");
    hipSetDevice(e->device);
    ze_launch_quantize_rows((bf16_t*)w_bf16, rows, cols, cols, (uint8_t*)q_out, cols, (float*)scale_out, (hipStream_t)stream);
    ZE_KCHECK();
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

// The numeric helpers every epilogue of the library shares (ze_common.h: f32_to_bf16 / pack_bf16x2 = v_cvt_pk_bf16_f32, silu_f =
// x * v_rcp_f32(1 + v_exp_f32(-x))), alone: out[i] = bf16(x[i]) | bf16(bf16(silu(x[i])) * y[i]) << 16, out2[i] = pack(x[i], y[i]).
extern "C" int ze_op_numeric_helpers(ze_engine* e, const float* x, const float* y, uint32_t* out, uint32_t* out2, int n, void* stream) {
    if (!e || !x || !y || !out || !out2 || n < 0) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    hipSetDevice(e->device);
    ze_launch_numeric_helpers(x, y, out, out2, n, (hipStream_t)stream);
    ZE_KCHECK();
    return ZE_OK;
}

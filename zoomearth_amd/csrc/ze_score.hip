// The scored-row path of a batched scoring pass (ze_score_batch, ze_forward.hip): of the pass's hidden rows only those whose
// next-token log-probability was asked for go through the final norm and the lm_head.
//   table (device int, staged with the pass's other tables): [n] rows of the pass's hidden state, then [n] target ids
//   k_rmsnorm_gather   y[r] = final norm of x[table[r]], dense rows -- the arithmetic of k_rmsnorm (ze_rmsnorm.h), the same bits
//   lm_head            ze_launch_gemm over the dense rows in chunks of the free MLP workspace, as ze_score chunks its rows:
//                      bf16 logits, K in sequence on every tile, so a row's logits do not depend on the chunk it falls into
//   k_token_logprob    fp32 log-softmax pick of the target id, a function of the row alone; where ze_score_batch_detail asks for
//                      entropy, rank or alternatives, k_score_detail (ze_score_detail.hip) in its place: the same pick and more
// Zero scored rows launch nothing.
#include "ze_engine.h"
#include "ze_rmsnorm.h"

// One wave per output row, four rows per workgroup, 16-byte loads and stores (cols % 8 == 0, rows 16-byte aligned)
__global__ void __launch_bounds__(256) k_rmsnorm_gather(const bf16_t* __restrict__ x, int ldx, const int* __restrict__ src_rows,
                                                        const bf16_t* __restrict__ w, bf16_t* __restrict__ y, int ldy, int rows,
                                                        int cols, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const bf16_t* xr = x + (size_t)src_rows[row] * ldx;
    const float inv = rms_wave_inv(xr, cols, eps, lane);
    bf16_t* yr = y + (size_t)row * ldy;
    const int nv = cols >> 3;
    for (int v = lane; v < nv; v += 64) {
        uint32_t o[4];
        rms_norm_vec(xr, w, v, inv, o);
        *reinterpret_cast<uint4*>(yr + v * 8) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

void ze_launch_rmsnorm_gather(const bf16_t* x, int ldx, const int* src_rows, const bf16_t* w, bf16_t* y, int ldy, int rows, int cols,
                              float eps, hipStream_t s) {
    if (rows <= 0) return;
    k_rmsnorm_gather<<<ze_cdiv(rows, 4), 256, 0, s>>>(x, ldx, src_rows, w, y, ldy, rows, cols, eps);
}

// rows of logits one lm_head launch of a scoring pass may write into the MLP workspace (0: not even one)
int ze_score_chunk_rows(const ze_engine* e, int rows) {
    const int ldl = (e->cfg.vocab + 7) & ~7;
    int chunk = (int)std::min<size_t>((size_t)e->prefill_rows * e->text_ipad / ldl, (size_t)rows);
    if (chunk >= 128) chunk &= ~127;
    return chunk;
}

// out[r] = log_softmax(lm_head(final_norm(e->th[rows[r]])))[targets[r]] for the n entries of e->tscore, after the pass's layers
// detail (ze_score_batch_detail): k_score_detail in k_token_logprob's place, its outputs packed as out
int ze_score_rows(ze_engine* e, int n, float* out, const ze_score_detail_out* detail, hipStream_t s) {
    if (n <= 0) return ZE_OK;
    const ze_config& c = e->cfg;
    const int H = c.hidden, ldl = (c.vocab + 7) & ~7;
    const int chunk = ze_score_chunk_rows(e, n);
    if (chunk < 1) return ze_fail(e, ZE_ERR_NOMEM, "prefill workspace too small for one row of logits");
    const int* targets = e->tscore + n;
    ze_launch_rmsnorm_gather(e->th, H, e->tscore, e->final_norm, e->ty, H, n, H, c.rms_eps, s);
    for (int r0 = 0; r0 < n; r0 += chunk) {
        const int m = std::min(chunk, n - r0);
        ze_launch_gemm(ZE_EPI_NONE, e->ty + (size_t)r0 * H, H, e->lm_head, H, nullptr, nullptr, 0, e->ta, ldl, nullptr, m, c.vocab, H, s);
        if (detail && detail->any()) {
            const ze_score_detail_out& d = *detail;
            ze_launch_score_detail(e->ta, ldl, c.vocab, targets + r0, d.top_n, out + r0, d.entropy ? d.entropy + r0 : nullptr,
                                   d.rank ? d.rank + r0 : nullptr, d.top_ids ? d.top_ids + (size_t)r0 * d.top_n : nullptr,
                                   d.top_lps ? d.top_lps + (size_t)r0 * d.top_n : nullptr, m, s);
        } else {
            ze_launch_token_logprob(e->ta, ldl, c.vocab, targets + r0, out + r0, m, s);
        }
    }
    return ZE_OK;
}

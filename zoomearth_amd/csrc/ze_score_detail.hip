// What a scored position reports beyond its log-probability (vLLM's `prompt_logprobs=N`; the per-token entropy a GRPO trainer
// logs and masks on; rank / top-1 agreement of likelihood evaluation).  One workgroup of 256 threads per row of bf16 logits
// ([rows, ld], ld % 8 == 0, as k_token_logprob takes them), every output a function of the row alone.  With l_i = float(logits[i]),
// m = max l, e_i = expf(l_i - m), tot = sum e_i and the total order "a before b" = (value descending, id ascending) of ze_logprobs.hip:
//     logprob = l[t] - m - logf(tot)                  the bits of k_token_logprob (ze_sample.hip): its maximum pass, its summation
//                                                     (ownership of the 16-byte groups, tail elements, shuffle order, (red0 + red1) +
//                                                     (red2 + red3)) and its final expression; a target outside [0, vocab) gives 0
//     entropy = logf(tot) - S / tot                   S = sum e_i * (l_i - m) over l_i > -inf, in the ownership and order of tot; every
//                                                     operation rounded to fp32 on its own (no contraction into an fma)
//     rank    = |{i : i before t}|                    0-based; -1 for a target outside the range
//     top-N   = the first N entries of the order      each with (l_i - m) - logf(tot); places the row cannot fill with finite entries
//                                                     carry (-1, -inf)
// A row without a finite maximum: entropy NaN, rank -1, every place (-1, -inf).
//
// The rows are bf16, so a row of 151,936 entries has at most 65,536 distinct values and ties at the N-th place are the normal case.
// The selection is therefore exact on the 16-bit order-preserving key of a value (-0 counts as +0, as the float comparison has it):
//   pass 1  the maximum; every thread keeps the maximum of its own elements.  tau, the N-th largest of these 256 maxima, is a lower
//           bound of the row's N-th largest value; the finite entries >= tau are the candidates.
//   pass 2  tot, S and the rank's count in one walk; the candidates' high key bytes go into a 256-bin LDS histogram, which gives the
//           byte B of the N-th largest key and the number of candidates above that bin.
//   pass 3  the low bytes of the candidates in bin B into a second histogram: T, the N-th largest key itself, and gt < N, the number
//           of entries above it.  Fewer than N candidates in all: every one of them is taken and pass 3 is skipped.
//   pass 4  the gt entries above T are appended to an LDS list (any order; ranked afterwards by counting under the total order).  The
//           entries equal to T need the N - gt lowest ids: the row is walked in chunks of 131,072 ids, a thread writes the equality
//           bits of its eight ids as one byte of an LDS bitmap, and the bitmap is scanned in id order behind a workgroup prefix sum.
// Histogram adds of a wave that all hit one bin (a row of equal values) are folded into one LDS atomic.  top_n = 0 stops after pass 2.
#include "ze_kernels.h"

// S and the entropy are stated as separately rounded fp32 operations: no multiply-add of this unit is fused
#pragma clang fp contract(off)

#define SD_CHUNK_GROUPS 16384  // 16-byte groups per bitmap chunk: one byte each

struct ze_score_detail_args {
    const bf16_t* logits;  // [rows, ld]
    int ld, vocab;
    const int* targets;  // [rows]
    int top_n;
    float* out_lp;    // [rows]
    float* out_ent;   // [rows] or null
    int* out_rank;    // [rows] or null
    int* out_ids;     // [rows, top_n] or null
    float* out_tlp;   // [rows, top_n] or null
};

// ascending key of a bf16 value: a > b as floats <=> key(a) > key(b) for non-NaN values, -0 folded onto +0
__device__ __forceinline__ uint32_t sd_key(float v) {
    uint32_t b = __float_as_uint(v) >> 16;
    if (b == 0x8000u) b = 0;
    return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}

// the eight values of 16-byte group g; group nv is the row's tail, its missing places NaN (no comparison holds for them)
__device__ __forceinline__ void sd_load8(const bf16_t* row, int g, int nv, int vocab, float v[8]) {
    if (g < nv) {
        const uint4 q = *(const uint4*)(row + (size_t)g * 8);
        const uint32_t u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) v[2 * j] = bf16lo(u[j]), v[2 * j + 1] = bf16hi(u[j]);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (g == nv && g * 8 + j < vocab) ? bf16_to_f32(row[g * 8 + j]) : __uint_as_float(0x7fc00000u);
    }
}

// h[bin] += 1 for the lanes with p; one add for the wave where they all name the same bin
__device__ __forceinline__ void sd_hist_add(int* h, bool p, int bin) {
    const unsigned long long act = __ballot(p);
    if (act == 0) return;
    const int lead = __ffsll((long long)act) - 1;
    const int b0 = __shfl(bin, lead, 64);
    if (__ballot(p && bin != b0) == 0) {
        if ((int)(threadIdx.x & 63) == lead) atomicAdd(&h[b0], (int)__popcll(act));
    } else if (p) {
        atomicAdd(&h[bin], 1);
    }
}

__device__ __forceinline__ float sd_wg_sum(float x, float* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    __syncthreads();
    if (lane == 0) red[w] = x;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ int sd_wg_sum_int(int x, int* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    __syncthreads();
    if (lane == 0) red[w] = x;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// bin (= tid) of a 256-bin histogram where the count from the top reaches `want`, given `above0` entries above the histogram:
// writes *sel = bin, *sel_above = above0 + entries in higher bins; no bin reaches it: *sel stays as it was
__device__ __forceinline__ void sd_select(const int* h, int above0, int want, int* sel, int* sel_above) {
    const int tid = threadIdx.x;
    int above = above0;
    for (int j = 255; j > tid; --j) above += h[j];
    if (above < want && want <= above + h[tid]) *sel = tid, *sel_above = above;
}

__global__ void __launch_bounds__(256) k_score_detail(const ze_score_detail_args a) {
    __shared__ float red[4];
    __shared__ int redi[4];
    __shared__ float smax[256];
    __shared__ int h1[256], h2[256];
    __shared__ __attribute__((aligned(16))) uint8_t bm[SD_CHUNK_GROUPS];
    __shared__ int gt_ids[32], eq_ids[32], wtot[4];
    __shared__ float stau;
    __shared__ int sB, sAbove, sL, sGt, n_gt, n_eq;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bf16_t* row = a.logits + (size_t)r * a.ld;
    const int vocab = a.vocab, nv = vocab / 8;
    const int t = a.targets[r];
    const bool t_ok = t >= 0 && t < vocab;
    const float lt = t_ok ? bf16_to_f32(row[t]) : __uint_as_float(0x7fc00000u);
    int N = min(a.out_ids ? a.top_n : 0, ZE_MAX_TOP_LOGPROBS);

    // ---- pass 1: the maximum, as k_token_logprob takes it
    float m = -INFINITY;
    for (int g = tid; g < nv; g += 256) {
        const uint4 q = *(const uint4*)(row + (size_t)g * 8);
        const uint32_t u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            m = fmaxf(m, bf16lo(u[j]));
            m = fmaxf(m, bf16hi(u[j]));
        }
    }
    for (int i = nv * 8 + tid; i < vocab; i += 256) m = fmaxf(m, bf16_to_f32(row[i]));
    const float tm = m;  // this thread's own
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) red[w] = m;
    smax[tid] = tm;
    h1[tid] = 0, h2[tid] = 0;
    if (tid == 0) sB = -1, sAbove = 0, sL = 0, sGt = 0, n_gt = 0, n_eq = 0, stau = -INFINITY;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const bool fin = fabsf(m) < INFINITY;
    if (!fin) N = 0;  // (uniform) nothing to select; the places are filled below

    // tau = the N-th largest of the 256 thread maxima (ranked by counting, equal maxima ordered by thread); fewer than N finite
    // maxima: -inf, every finite entry is a candidate
    if (N > 0) {
        int rk = 0;
        for (int j = 0; j < 256; ++j) rk += (smax[j] > tm || (smax[j] == tm && j < tid)) ? 1 : 0;
        if (rk == N - 1) stau = tm;
    }
    __syncthreads();
    const float tau = stau;

    // ---- pass 2: tot and S in k_token_logprob's ownership and order, the rank's count, the candidates' high bytes
    float sum = 0.f, S = 0.f;
    int before = 0;
    for (int g = tid; g < nv; g += 256) {
        float v[8];
        sd_load8(row, g, nv, vocab, v);
        bool any = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float d = v[j] - m;
            const float e = expf(d);
            sum += e;
            if (v[j] > -INFINITY) S = __fadd_rn(S, __fmul_rn(e, d));
            before += (v[j] > lt || (v[j] == lt && g * 8 + j < t)) ? 1 : 0;
            any |= v[j] >= tau && v[j] > -INFINITY;
        }
        if (N > 0 && __ballot(any) != 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) sd_hist_add(h1, v[j] >= tau && v[j] > -INFINITY, (int)(sd_key(v[j]) >> 8));
        }
    }
    for (int i = nv * 8 + tid; i < vocab; i += 256) {
        const float x = bf16_to_f32(row[i]);
        const float d = x - m;
        const float e = expf(d);
        sum += e;
        if (x > -INFINITY) S = __fadd_rn(S, __fmul_rn(e, d));
        before += (x > lt || (x == lt && i < t)) ? 1 : 0;
        if (N > 0 && x >= tau && x > -INFINITY) atomicAdd(&h1[sd_key(x) >> 8], 1);
    }
    const float tot = sd_wg_sum(sum, red);
    const float lse = logf(tot);
    if (tid == 0) a.out_lp[r] = t_ok ? lt - m - lse : 0.f;
    if (a.out_ent) {  // (uniform)
        const float Stot = sd_wg_sum(S, red);
        if (tid == 0) a.out_ent[r] = fin ? __fsub_rn(lse, __fdiv_rn(Stot, tot)) : __uint_as_float(0x7fc00000u);
    }
    if (a.out_rank) {
        const int rk = sd_wg_sum_int(before, redi);
        if (tid == 0) a.out_rank[r] = (fin && t_ok) ? rk : -1;
    }
    if (!a.out_ids || a.top_n <= 0) return;
    int* o_ids = a.out_ids + (size_t)r * a.top_n;
    float* o_tlp = a.out_tlp + (size_t)r * a.top_n;
    if (N <= 0) {  // no finite maximum
        if (tid < a.top_n) o_ids[tid] = -1, o_tlp[tid] = -INFINITY;
        return;
    }

    // ---- the byte B of the N-th largest key (the workgroup sums above ordered every add to h1 before these reads)
    sd_select(h1, 0, N, &sB, &sAbove);
    __syncthreads();
    const int B = sB;  // -1: fewer than N candidates, all of them are taken
    const int ng = nv + (vocab > nv * 8 ? 1 : 0);
    uint32_t T = 0;  // entries with a key above T are taken outright
    int need = 0;    // ... and the `need` lowest ids among the entries equal to T
    if (B >= 0) {
        // ---- pass 3: the low bytes of the candidates in bin B
        for (int g = tid; g < ng; g += 256) {
            float v[8];
            sd_load8(row, g, nv, vocab, v);
            bool any = false;
            uint32_t k[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                k[j] = sd_key(v[j]);
                any |= v[j] >= tau && v[j] > -INFINITY && (int)(k[j] >> 8) == B;
            }
            if (__ballot(any) != 0) {
#pragma unroll
                for (int j = 0; j < 8; ++j) sd_hist_add(h2, v[j] >= tau && v[j] > -INFINITY && (int)(k[j] >> 8) == B, (int)(k[j] & 255u));
            }
        }
        __syncthreads();
        sd_select(h2, sAbove, N, &sL, &sGt);
        __syncthreads();
        T = ((uint32_t)B << 8) | (uint32_t)sL;
        need = N - sGt;
    }

    // ---- pass 4: the entries above T into gt_ids; the `need` lowest ids equal to T through the bitmap, chunk by chunk
    for (int c0 = 0; c0 < ng; c0 += SD_CHUNK_GROUPS) {
        const bool scan = need > 0 && n_eq < need;  // (uniform: n_eq is written between the barriers at the end of the loop body)
        for (int gl = tid; gl < SD_CHUNK_GROUPS; gl += 256) {
            const int g = c0 + gl;
            uint32_t eq = 0;
            if (g < ng) {
                float v[8];
                sd_load8(row, g, nv, vocab, v);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const bool cand = v[j] >= tau && v[j] > -INFINITY;
                    const uint32_t k = sd_key(v[j]);
                    if (cand && (B < 0 || k > T)) {
                        const int p = atomicAdd(&n_gt, 1);
                        if (p < 32) gt_ids[p] = g * 8 + j;
                    }
                    if (cand && B >= 0 && k == T) eq |= 1u << j;
                }
            } else if (!scan) {
                break;
            }
            if (scan) bm[gl] = (uint8_t)eq;
        }
        __syncthreads();
        if (scan) {
            // thread tid owns words [16 tid, 16 tid + 16) of the chunk's 4096: ids c0 * 8 + 512 tid ...
            const uint32_t* words = reinterpret_cast<const uint32_t*>(bm) + 16 * tid;
            uint32_t wv[16];
            int cnt = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint4 x = *reinterpret_cast<const uint4*>(words + 4 * q);
                wv[4 * q] = x.x, wv[4 * q + 1] = x.y, wv[4 * q + 2] = x.z, wv[4 * q + 3] = x.w;
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) cnt += __popc(wv[q]);
            int inc = cnt;  // inclusive prefix over the wave, then the waves in order
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(inc, o, 64);
                if (lane >= o) inc += y;
            }
            if (lane == 63) wtot[w] = inc;
            __syncthreads();
            int pos = n_eq + inc - cnt;
            for (int x = 0; x < w; ++x) pos += wtot[x];
            const int chunk_tot = wtot[0] + wtot[1] + wtot[2] + wtot[3];
            if (cnt > 0 && pos < need) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    uint32_t bits = wv[q];
                    while (bits && pos < need) {
                        const int bit = __ffs((int)bits) - 1;
                        bits &= bits - 1;
                        eq_ids[pos++] = c0 * 8 + (16 * tid + q) * 32 + bit;
                    }
                }
            }
            __syncthreads();
            if (tid == 0) n_eq += chunk_tot;
            __syncthreads();
        }
    }
    __syncthreads();

    // ---- the places: the entries above T ranked by counting, the equal ones behind them in id order, the rest empty
    const int ngt = min(n_gt, 32);
    const int neq = min(n_eq, need);
    if (tid < ngt) {
        const int id = gt_ids[tid];
        const float v = bf16_to_f32(row[id]);
        int rk = 0;
        for (int j = 0; j < ngt; ++j) {
            const int oj = gt_ids[j];
            const float ov = bf16_to_f32(row[oj]);
            rk += (ov > v || (ov == v && oj < id)) ? 1 : 0;
        }
        if (rk < a.top_n) o_ids[rk] = id, o_tlp[rk] = (v - m) - lse;
    } else if (tid >= 64 && tid - 64 < neq) {
        const int k = tid - 64, id = eq_ids[k];
        if (ngt + k < a.top_n) o_ids[ngt + k] = id, o_tlp[ngt + k] = (bf16_to_f32(row[id]) - m) - lse;
    } else if (tid >= 128 && tid - 128 >= ngt + neq && tid - 128 < a.top_n) {
        o_ids[tid - 128] = -1, o_tlp[tid - 128] = -INFINITY;
    }
}

void ze_launch_score_detail(const bf16_t* logits, int ld, int vocab, const int* targets, int top_n, float* out_lp, float* out_ent,
                            int* out_rank, int* out_ids, float* out_tlp, int rows, hipStream_t s) {
    if (rows <= 0) return;
    ze_score_detail_args a{};
    a.logits = logits, a.ld = ld, a.vocab = vocab, a.targets = targets, a.top_n = top_n;
    a.out_lp = out_lp, a.out_ent = out_ent, a.out_rank = out_rank, a.out_ids = out_ids, a.out_tlp = out_tlp;
    k_score_detail<<<rows, 256, 0, s>>>(a);
}

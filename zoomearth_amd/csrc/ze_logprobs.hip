// Per-token log-probabilities of generated tokens, with the N best alternatives (replaces: vLLM's `logprobs=N` of a sampled
// token and the completion part of `old_per_token_logps`, src/train/RL/.../open_r1/trainer/grpo_trainer.py:660-683, which the
// reference obtains with one more forward pass).  For a row l of fp32 logits (the lm_head's output, before repetition penalty,
// temperature and filters):
//     logprob(t) = l[t] - max(l) - logf(sum_i expf(l[i] - max(l)))
//     top-N      = the N entries with the largest l, ties to the lower id, in (value descending, id ascending) order; places a
//                  row cannot fill with finite entries carry (id -1, logprob -inf)
// One workgroup of 256 threads per row, so the result is a function of the row alone: whichever rows share the launch, whichever
// slot the chain holds, graph or no graph.
//   pass 1: the maximum.  Thread t owns the 4-element groups t, t + 256, ... (16-byte loads where the row is 16-byte aligned, the
//           same elements in the same order where it is not); per thread, then per wave by __shfl_xor, then the four waves in
//           order.  Every thread also keeps the maximum of its own elements: the N-th largest of these 256 maxima, tau, is a
//           lower bound of the row's N-th largest value (they are 256 distinct elements and N <= 20 < 256).
//   pass 2: the sum of expf(l - max) in the same ownership and order (four lane accumulators per thread, (a0 + a1) + (a2 + a3)),
//           and every finite element >= tau goes as (value, id) into an LDS list through an LDS counter.  The append order is
//           not deterministic; the list is then ranked by counting under the total order (value desc, id asc), which is.
//   overflow: the counter's final value -- the number of finite elements >= tau, a property of the row -- decides.  More than
//           LP_CAP of them (all logits equal, a maximum duplicated thousands of times): N rounds of a workgroup arg-max over the
//           entries strictly after the previous pick in the total order.  Slow (N more passes) and correct.
#include "ze_kernels.h"

#define LP_CAP 1024

struct lp_row {
    const float* row;
    int vocab;
    bool vec;  // 16-byte loads allowed
};

__device__ __forceinline__ float4 lp_load4(const lp_row& r, int g) {
    if (r.vec) return *reinterpret_cast<const float4*>(r.row + (size_t)g * 4);
    const float* p = r.row + (size_t)g * 4;
    return make_float4(p[0], p[1], p[2], p[3]);
}

// (value desc, id asc): is a before b?
__device__ __forceinline__ bool lp_before(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

__device__ __forceinline__ float lp_wg_max(float m, float* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    __syncthreads();
    if (lane == 0) red[w] = m;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// the slow path: places [0, N) by N arg-max rounds over the finite entries after (pv, pi) in the total order
__device__ void lp_top_rounds(const lp_row& r, int N, float m, float lse, int* out_ids, float* out_lps, float* redv, int* redi) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nv = r.vocab / 4;
    float pv = INFINITY;
    int pi = -1;
    for (int k = 0; k < N; ++k) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int g = tid; g < nv; g += 256) {
            const float4 q = lp_load4(r, g);
            const float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (v[j] > -INFINITY && lp_before(pv, pi, v[j], 4 * g + j) && lp_before(v[j], 4 * g + j, bv, bi)) bv = v[j], bi = 4 * g + j;
        }
        for (int i = nv * 4 + tid; i < r.vocab; i += 256) {
            const float v = r.row[i];
            if (v > -INFINITY && lp_before(pv, pi, v, i) && lp_before(v, i, bv, bi)) bv = v, bi = i;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (lp_before(ov, oi, bv, bi)) bv = ov, bi = oi;
        }
        __syncthreads();
        if (lane == 0) redv[w] = bv, redi[w] = bi;
        __syncthreads();
        bv = redv[0], bi = redi[0];
        for (int x = 1; x < 4; ++x)
            if (lp_before(redv[x], redi[x], bv, bi)) bv = redv[x], bi = redi[x];
        const bool found = bi != 0x7fffffff;
        if (tid == 0) {
            out_ids[k] = found ? bi : -1;
            out_lps[k] = found ? bv - m - lse : -INFINITY;
        }
        if (!found) {  // (uniform) nothing is left: the remaining places are empty too
            if (tid > k && tid < N) out_ids[tid] = -1, out_lps[tid] = -INFINITY;
            return;
        }
        pv = bv, pi = bi;
    }
}

struct ze_lp_args {
    const float* logits;  // [rows, ld]
    int vocab, ld;
    // unit-op form (st == null): row r has targets[r], every row wants top_n, outputs are indexed by r with top stride top_n
    const int* targets;
    int top_n;
    // chain form: row b is chain slot seq_ids ? seq_ids[b] : slot0; want[slot] = -1 off / 0 / 1..20; the token is st[slot].token,
    // the history entry st[slot].n_gen - 1 (dropped at max_gen); outputs are the history buffers ([slots, max_gen(, 20)])
    const ze_seq_dev* st;
    const int* seq_ids;
    int slot0;
    const int* want;
    int max_gen;
    float* out_lp;
    int* out_ids;
    float* out_tlp;
};

__global__ void __launch_bounds__(256) k_token_logprobs(const ze_lp_args a) {
    __shared__ float red[4];
    __shared__ int redi[4];
    __shared__ float smax[256];
    __shared__ float cv[LP_CAP];
    __shared__ int ci[LP_CAP];
    __shared__ int cnt;
    __shared__ float stau;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int N, target;
    float* o_lp;
    int* o_ids;
    float* o_tlp;
    if (a.st) {
        const int slot = a.seq_ids ? a.seq_ids[b] : a.slot0;
        N = a.want[slot];
        if (N < 0) return;  // this chain asked for nothing (uniform: the whole workgroup leaves)
        const int idx = a.st[slot].n_gen - 1;
        if (idx < 0 || idx >= a.max_gen) return;
        target = a.st[slot].token;
        const size_t e = (size_t)slot * a.max_gen + idx;
        o_lp = a.out_lp + e;
        o_ids = a.out_ids + e * ZE_MAX_TOP_LOGPROBS;
        o_tlp = a.out_tlp + e * ZE_MAX_TOP_LOGPROBS;
        if (!a.out_ids) N = 0;  // (the setter allocates them before any chain can ask for alternatives)
    } else {
        N = a.top_n;
        target = a.targets[b];
        o_lp = a.out_lp + b;
        o_ids = a.out_ids + (size_t)b * N;
        o_tlp = a.out_tlp + (size_t)b * N;
    }
    N = min(N, ZE_MAX_TOP_LOGPROBS);
    lp_row r;
    r.row = a.logits + (size_t)b * a.ld;
    r.vocab = a.vocab;
    r.vec = (reinterpret_cast<uintptr_t>(r.row) & 15) == 0;
    const int nv = r.vocab / 4;

    // ---- pass 1: maximum (and this thread's own)
    float tm = -INFINITY;
    {
        int g = tid;
        for (; g + 768 < nv; g += 1024) {  // four loads in flight
            const float4 q0 = lp_load4(r, g), q1 = lp_load4(r, g + 256), q2 = lp_load4(r, g + 512), q3 = lp_load4(r, g + 768);
            tm = fmaxf(tm, fmaxf(fmaxf(fmaxf(q0.x, q0.y), fmaxf(q0.z, q0.w)), fmaxf(fmaxf(q1.x, q1.y), fmaxf(q1.z, q1.w))));
            tm = fmaxf(tm, fmaxf(fmaxf(fmaxf(q2.x, q2.y), fmaxf(q2.z, q2.w)), fmaxf(fmaxf(q3.x, q3.y), fmaxf(q3.z, q3.w))));
        }
        for (; g < nv; g += 256) {
            const float4 q = lp_load4(r, g);
            tm = fmaxf(tm, fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w)));
        }
        for (int i = nv * 4 + tid; i < r.vocab; i += 256) tm = fmaxf(tm, r.row[i]);
    }
    const float m = lp_wg_max(tm, red);

    // tau = the N-th largest of the 256 thread maxima (ranked by counting; equal maxima are ordered by thread)
    float tau = INFINITY;
    if (N > 0) {
        smax[tid] = tm;
        if (tid == 0) cnt = 0;
        __syncthreads();
        int rank = 0;
        for (int j = 0; j < 256; ++j) rank += lp_before(smax[j], j, tm, tid) ? 1 : 0;
        if (rank == N - 1) stau = tm;
        __syncthreads();
        tau = stau;
    }

    // ---- pass 2: sum of expf(l - m); candidates >= tau
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int g0 = tid; g0 < nv; g0 += 1024) {
        float4 q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (g0 + u * 256 < nv) q[u] = lp_load4(r, g0 + u * 256);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int g = g0 + u * 256;
            if (g < nv) {
                const float v[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
                a0 += expf(v[0] - m);
                a1 += expf(v[1] - m);
                a2 += expf(v[2] - m);
                a3 += expf(v[3] - m);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (v[j] >= tau && v[j] > -INFINITY) {
                        const int k = atomicAdd(&cnt, 1);
                        if (k < LP_CAP) cv[k] = v[j], ci[k] = 4 * g + j;
                    }
            }
        }
    }
    float sum = (a0 + a1) + (a2 + a3);
    for (int i = nv * 4 + tid; i < r.vocab; i += 256) {
        const float v = r.row[i];
        sum += expf(v - m);
        if (v >= tau && v > -INFINITY) {
            const int k = atomicAdd(&cnt, 1);
            if (k < LP_CAP) cv[k] = v, ci[k] = i;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    __syncthreads();
    if (lane == 0) red[w] = sum;
    __syncthreads();
    const float lse = logf((red[0] + red[1]) + (red[2] + red[3]));
    if (tid == 0) *o_lp = (target >= 0 && target < r.vocab) ? r.row[target] - m - lse : 0.f;
    if (N <= 0) return;

    // ---- top-N: rank the candidates by counting
    const int c = cnt;  // (the barriers above ordered every append before this read)
    if (c > LP_CAP) {
        lp_top_rounds(r, N, m, lse, o_ids, o_tlp, red, redi);
        return;
    }
    for (int i = tid; i < c; i += 256) {
        const float v = cv[i];
        const int id = ci[i];
        int rank = 0;
        for (int j = 0; j < c; ++j) rank += lp_before(cv[j], ci[j], v, id) ? 1 : 0;
        if (rank < N) o_ids[rank] = id, o_tlp[rank] = v - m - lse;
    }
    if (tid >= c && tid < N) o_ids[tid] = -1, o_tlp[tid] = -INFINITY;
}

void ze_launch_token_logprobs(const float* logits, int rows, int vocab, int ld, const int* targets, int top_n, float* out_lp,
                              int* out_ids, float* out_tlp, hipStream_t s) {
    if (rows <= 0) return;
    ze_lp_args a{};
    a.logits = logits, a.vocab = vocab, a.ld = ld, a.targets = targets, a.top_n = top_n;
    a.out_lp = out_lp, a.out_ids = out_ids, a.out_tlp = out_tlp;
    k_token_logprobs<<<rows, 256, 0, s>>>(a);
}

void ze_launch_chain_logprobs(const float* logits, int vocab, int ld, const ze_seq_dev* st, const int* seq_ids, int slot0, int n,
                              const ze_logprob_bufs& lp, int max_gen, hipStream_t s) {
    if (n <= 0) return;
    ze_lp_args a{};
    a.logits = logits, a.vocab = vocab, a.ld = ld;
    a.st = st, a.seq_ids = seq_ids, a.slot0 = slot0, a.want = lp.want, a.max_gen = max_gen;
    a.out_lp = lp.tok, a.out_ids = lp.top_ids, a.out_tlp = lp.top_lps;
    k_token_logprobs<<<n, 256, 0, s>>>(a);
}

__global__ void k_set_logprobs(int* want, int slot, int top_n) { want[slot] = top_n; }
void ze_launch_set_logprobs(int* want, int slot, int top_n, hipStream_t s) { k_set_logprobs<<<1, 1, 0, s>>>(want, slot, top_n); }

// The log-probability twin of k_gather_chain_tokens, for ONE device -> host copy: out = [n_gen, finished, top_n per chain (3n
// ints) | n rows of cap ids | n rows of cap f32 | n x cap x stride ids | n x cap x stride f32]; places beyond a chain's own top_n
// are (id -1, -inf).  stride = 0: no alternatives.
__global__ void k_gather_chain_logprobs(const ze_seq_dev* __restrict__ st, const int* __restrict__ out_tokens,
                                        const int* __restrict__ want, const float* __restrict__ tok,
                                        const int* __restrict__ top_ids, const float* __restrict__ top_lps, int max_ctx,
                                        const int* __restrict__ slots, int n, int cap, int stride, int* __restrict__ out) {
    const int c = blockIdx.y, seq = slots[c];
    const int ng = min(min(st[seq].n_gen, cap), max_ctx);
    const int tn = want[seq];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out[3 * c] = ng;
        out[3 * c + 1] = st[seq].finished;
        out[3 * c + 2] = tn;
    }
    const size_t rows = (size_t)n * cap;
    int* d_tok = out + 3 * n + (size_t)c * cap;
    float* d_lp = reinterpret_cast<float*>(out + 3 * n + rows) + (size_t)c * cap;
    int* d_ids = out + 3 * n + 2 * rows + (size_t)c * cap * stride;
    float* d_tlp = reinterpret_cast<float*>(out + 3 * n + 2 * rows + rows * stride) + (size_t)c * cap * stride;
    const size_t src = (size_t)seq * max_ctx;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < ng; i += gridDim.x * 256) {
        d_tok[i] = out_tokens[src + i];
        d_lp[i] = tok[src + i];
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < ng * stride; i += gridDim.x * 256) {
        const int t = i / stride, j = i - t * stride;
        const bool has = top_ids && j < tn;
        d_ids[i] = has ? top_ids[(src + t) * ZE_MAX_TOP_LOGPROBS + j] : -1;
        d_tlp[i] = has ? top_lps[(src + t) * ZE_MAX_TOP_LOGPROBS + j] : -INFINITY;
    }
}
void ze_launch_gather_chain_logprobs(const ze_seq_dev* st, const int* out_tokens, const ze_logprob_bufs& lp, int max_ctx,
                                     const int* slots, int n, int cap, int stride, int* out, hipStream_t s) {
    if (n > 0)
        k_gather_chain_logprobs<<<dim3(std::max(1, std::min(ze_cdiv(cap * std::max(stride, 1), 256), 32)), n), 256, 0, s>>>(
            st, out_tokens, lp.want, lp.tok, lp.top_ids, lp.top_lps, max_ctx, slots, n, cap, stride, out);
}

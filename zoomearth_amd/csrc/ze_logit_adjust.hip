// Per-chain additive logit adjustments (include/zoomearth.h, ze_seq_set_logit_adjust): a sparse bias list, presence / frequency
// penalties over the counts of the chain's GENERATED tokens, and the EOS ids masked while fewer than min_new_tokens were
// generated.  A step's raw fp32 rows l are copied into a second buffer as
//     t_i = frequency * (float)c_i ; if c_i > 0: t_i = t_i + presence ; a_i = (l_i + bias_i) - t_i ; a_eos = -inf while masked
// every operation rounded to fp32 on its own (the file is compiled without contraction: no fused multiply-add), so a row is
// bit for bit the numpy float32 restatement (tests/logit_adjust_ref.py).  The sampler reads the copy; the log-probability
// kernel keeps reading l.
//
// The work is elementwise, so the grid is 2-D: vocabulary chunks x rows, 256 threads, two 16-byte groups per thread, all
// loads of a thread issued before the first use.  (One workgroup per row, the shape of the reductions next door, is bound by a
// single workgroup's load latency: 7 % / 33 % of the traffic floor in ze_logprobs.hip.)  An output element depends on its own
// row's inputs alone -- the same bits whatever the batch, the slot, graph or eager.  The workgroup that owns a chunk applies
// the bias entries and EOS ids that fall into it after its own dense writes: no cross-workgroup races, no atomics.  A row of
// a chain without a request is copied unchanged (not even l + 0, which would turn -0 into +0).
#include <cstring>

#include "ze_kernels.h"

#pragma clang fp contract(off)

#define LA_THREADS 256
#define LA_GROUPS 2                               // 16-byte groups per thread
#define LA_CHUNK (LA_THREADS * LA_GROUPS * 4)     // elements of a row per workgroup

struct ze_la_args {
    const float* logits;  // [rows, ld]
    float* out;           // [rows, ld]
    int vocab, ld;
    const int* eos_ids;
    int n_eos;
    // counts: unit form u16 [rows, vocab] or null; chain form u16 [slots, vocab] or null (no chain has penalties yet)
    const uint16_t* counts;
    // unit form (st == null): per row r presence[r], frequency[r], eos_masked[r], bias entries bias_off[r] .. bias_off[r + 1]
    const float *presence, *frequency;
    const int *eos_masked, *bias_off;
    // bias lists: unit form flat; chain form [slots, ZE_MAX_LOGIT_BIAS]
    const int* bias_ids;
    const float* bias_vals;
    // chain form: row b is chain slot seq_ids ? seq_ids[b] : slot0; table = ZE_LA_WORDS ints per slot (ze_launch_set_logit_adjust)
    const ze_seq_dev* st;
    const int* seq_ids;
    int slot0;
    const int* table;
};

__device__ __forceinline__ float la_value(float l, float bias, unsigned c, float presence, float frequency) {
    float t = frequency * (float)c;
    if (c > 0) t = t + presence;
    return (l + bias) - t;
}

__global__ void __launch_bounds__(LA_THREADS) k_logit_adjust(const ze_la_args a) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const float* in = a.logits + (size_t)b * a.ld;
    float* out = a.out + (size_t)b * a.ld;
    float presence = 0.f, frequency = 0.f;
    bool on = true, masked = false;
    const uint16_t* cnt = nullptr;
    const int* bids = a.bias_ids;
    const float* bvals = a.bias_vals;
    int nb = 0;
    if (a.st) {
        const int slot = a.seq_ids ? a.seq_ids[b] : a.slot0;
        const int* t = a.table + (size_t)slot * ZE_LA_WORDS;
        presence = __int_as_float(t[0]);
        frequency = __int_as_float(t[1]);
        const int min_new = t[2];
        nb = min(max(t[3], 0), ZE_MAX_LOGIT_BIAS);
        on = presence != 0.f || frequency != 0.f || min_new > 0 || nb > 0;
        masked = a.st[slot].n_gen < min_new;
        if (a.counts && (presence != 0.f || frequency != 0.f)) cnt = a.counts + (size_t)slot * a.vocab;
        bids += (size_t)slot * ZE_MAX_LOGIT_BIAS;
        bvals += (size_t)slot * ZE_MAX_LOGIT_BIAS;
    } else {
        presence = a.presence[b];
        frequency = a.frequency[b];
        masked = a.eos_masked[b] != 0;
        if (a.counts) cnt = a.counts + (size_t)b * a.vocab;
        const int o0 = a.bias_off[b];
        nb = max(a.bias_off[b + 1] - o0, 0);
        bids += o0;
        bvals += o0;
        on = presence != 0.f || frequency != 0.f || masked || nb > 0;  // all off: a row without a request, copied
    }
    const int lo = blockIdx.x * LA_CHUNK, hi = min(lo + LA_CHUNK, a.vocab);
    // 16-byte groups while both rows are aligned (ld % 4 and the bases decide); the rest of the chunk one element at a time
    const bool vec = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const bool cvec = cnt && (reinterpret_cast<uintptr_t>(cnt) & 7) == 0;
    const int vend = vec ? (hi & ~3) : lo;  // lo is a multiple of 4
    float4 v[LA_GROUPS];
    uint2 q[LA_GROUPS];
#pragma unroll
    for (int u = 0; u < LA_GROUPS; ++u) {
        const int i = lo + (u * LA_THREADS + tid) * 4;
        q[u] = make_uint2(0u, 0u);
        if (i < vend) {
            v[u] = *reinterpret_cast<const float4*>(in + i);
            if (cvec)
                q[u] = *reinterpret_cast<const uint2*>(cnt + i);
            else if (cnt)
                q[u] = make_uint2((unsigned)cnt[i] | ((unsigned)cnt[i + 1] << 16), (unsigned)cnt[i + 2] | ((unsigned)cnt[i + 3] << 16));
        }
    }
#pragma unroll
    for (int u = 0; u < LA_GROUPS; ++u) {
        const int i = lo + (u * LA_THREADS + tid) * 4;
        if (i < vend) {
            float4 r = v[u];
            if (on) {
                r.x = la_value(r.x, 0.f, q[u].x & 0xffffu, presence, frequency);
                r.y = la_value(r.y, 0.f, q[u].x >> 16, presence, frequency);
                r.z = la_value(r.z, 0.f, q[u].y & 0xffffu, presence, frequency);
                r.w = la_value(r.w, 0.f, q[u].y >> 16, presence, frequency);
            }
            *reinterpret_cast<float4*>(out + i) = r;
        }
    }
    for (int i = vend + tid; i < hi; i += LA_THREADS) {
        const float l = in[i];
        out[i] = on ? la_value(l, 0.f, cnt ? cnt[i] : 0u, presence, frequency) : l;
    }
    if (!on || (nb == 0 && !masked)) return;  // (uniform: the whole workgroup leaves)
    __syncthreads();
    for (int j = tid; j < nb; j += LA_THREADS) {
        const int i = bids[j];
        if (i >= lo && i < hi) out[i] = la_value(in[i], bvals[j], cnt ? cnt[i] : 0u, presence, frequency);
    }
    if (!masked) return;
    __syncthreads();
    for (int j = tid; j < a.n_eos; j += LA_THREADS) {
        const int i = a.eos_ids[j];
        if (i >= lo && i < hi) out[i] = -INFINITY;
    }
}

static void launch(const ze_la_args& a, int rows, hipStream_t s) {
    if (rows <= 0 || a.vocab <= 0) return;
    k_logit_adjust<<<dim3(ze_cdiv(a.vocab, LA_CHUNK), rows), LA_THREADS, 0, s>>>(a);
}

void ze_launch_logit_adjust(const float* logits, int rows, int vocab, int ld, const uint16_t* counts, const float* presence,
                            const float* frequency, const int* eos_masked, const int* bias_off, const int* bias_ids,
                            const float* bias_vals, const int* eos_ids, int n_eos, float* out, hipStream_t s) {
    ze_la_args a{};
    a.logits = logits, a.out = out, a.vocab = vocab, a.ld = ld, a.eos_ids = eos_ids, a.n_eos = n_eos, a.counts = counts;
    a.presence = presence, a.frequency = frequency, a.eos_masked = eos_masked, a.bias_off = bias_off;
    a.bias_ids = bias_ids, a.bias_vals = bias_vals;
    launch(a, rows, s);
}

void ze_launch_chain_logit_adjust(const float* logits, int vocab, const ze_seq_dev* st, const int* seq_ids, int slot0, int n,
                                  const ze_logit_adjust_bufs& la, const int* eos_ids, int n_eos, float* out, hipStream_t s) {
    ze_la_args a{};
    a.logits = logits, a.out = out, a.vocab = vocab, a.ld = vocab, a.eos_ids = eos_ids, a.n_eos = n_eos, a.counts = la.counts;
    a.bias_ids = la.bias_ids, a.bias_vals = la.bias_vals;
    a.st = st, a.seq_ids = seq_ids, a.slot0 = slot0, a.table = la.table;
    launch(a, n, s);
}

// After the token of a step was accepted: the chain's count of it goes up by one (saturating), one thread per chain.  Only
// chains with a penalty keep counts.  word 4 of the slot's table = the chain had finished before this step, whose token is
// then a pad and is not counted.
__global__ void __launch_bounds__(64) k_count_tokens(const ze_seq_dev* __restrict__ st, const int* __restrict__ seq_ids, int slot0,
                                                     int n, int* __restrict__ table, uint16_t* __restrict__ counts, int vocab) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n) return;
    const int slot = seq_ids ? seq_ids[b] : slot0;
    int* t = table + (size_t)slot * ZE_LA_WORDS;
    if (__int_as_float(t[0]) == 0.f && __int_as_float(t[1]) == 0.f) return;
    if (t[4]) return;
    const ze_seq_dev c = st[slot];
    if (c.n_gen <= 0) return;
    if ((unsigned)c.token < (unsigned)vocab) {
        uint16_t* p = counts + (size_t)slot * vocab + c.token;
        const uint16_t k = *p;
        if (k < 0xffffu) *p = (uint16_t)(k + 1);
    }
    t[4] = c.finished;
}

void ze_launch_count_tokens(const ze_seq_dev* st, const int* seq_ids, int slot0, int n, const ze_logit_adjust_bufs& la, int vocab,
                            hipStream_t s) {
    if (n <= 0 || !la.counts) return;
    k_count_tokens<<<ze_cdiv(n, 64), 64, 0, s>>>(st, seq_ids, slot0, n, la.table, la.counts, vocab);
}

struct ze_la_words {
    int v[ZE_LA_WORDS];
};
__global__ void k_set_logit_adjust(int* table, int slot, ze_la_words w) {
    if (threadIdx.x < ZE_LA_WORDS) table[(size_t)slot * ZE_LA_WORDS + threadIdx.x] = w.v[threadIdx.x];
}
void ze_launch_set_logit_adjust(int* table, int slot, float presence, float frequency, int min_new_tokens, int n_bias,
                                hipStream_t s) {
    ze_la_words w{};
    std::memcpy(&w.v[0], &presence, sizeof(float));
    std::memcpy(&w.v[1], &frequency, sizeof(float));
    w.v[2] = min_new_tokens;
    w.v[3] = n_bias;
    k_set_logit_adjust<<<1, ZE_LA_WORDS, 0, s>>>(table, slot, w);
}

// Speculative decoding by prompt lookup (HF: generate(prompt_lookup_num_tokens=, max_matching_ngram_size=); vLLM: the `ngram`
// speculative method): the drafter, the accept pass, the row table of a speculative step, their unit entries and the setter.
// The step itself -- draft -> rows -> the fragment family's launches -> accept -- is enqueued by ze_decode_batch.hip (spec_burst).
//
// Drafter (normative: tests/spec_ref.py restates it).  The history of a chain is its prompt ids followed by its generated ids, n
// ids in all.  For g = max_ngram down to min_ngram with g < n: among the starts p in [0, n - g - 1] with
// history[p .. p + g) == history[n - g .. n) -- every such occurrence has at least one id behind it, and the tail itself
// (p = n - g) is not one -- the LARGEST p wins; the first g with an occurrence wins.  The draft is history[p + g .. ), at most k ids,
// cut at the end of the history and at `cap` (the rows and tokens the chain has room for).  No occurrence: length 0.
//
// Accept pass.  Row j of a chain holds the logits behind its token at position ctx + j (row 0: the chain's last token, row j: draft
// id j - 1).  For j = 0, 1, ...: the token is the arg-max of row j under the repetition penalty (score < 0 ? score * p : score / p on
// the ids seen SO FAR, the tokens of rows 0 .. j - 1 included; lowest id on ties; 0 for a row of NaN: k_argmax_partial /
// k_argmax_final_batch of ze_sample.hip -- a maximum under a total order, so the bits do not depend on how it is reduced); it is
// emitted and marked seen; the walk ends behind the last row, behind a token that is not draft id j, behind an EOS id, or when the
// chain's room is used up.  Plain C++ stores from vector lanes only; nothing waits for the host.
#include <cmath>
#include <cstring>

#include "ze_engine.h"

#define SP_THREADS 1024

// the history in its two segments
struct sp_hist {
    const int* seg0;
    int l0;
    const int* seg1;
    int l1;
    __device__ __forceinline__ int at(int i) const { return i < l0 ? seg0[i] : seg1[i - l0]; }
};

// workgroup-wide; every thread gets the same (d_start, d_len): the draft is history[d_start .. d_start + d_len)
__device__ __forceinline__ void spec_draft_wg(const sp_hist& h, int k, int gmin, int gmax, int cap, int* s_best, int* s_tail, int& d_start, int& d_len) {
    const int n = h.l0 + h.l1;
    int best = -1, hit = 0;
    for (int g = gmax; g >= gmin; --g) {
        if (g >= n) continue;  // (uniform) no earlier occurrence can exist
        if (threadIdx.x == 0) *s_best = -1;
        if ((int)threadIdx.x < g) s_tail[threadIdx.x] = h.at(n - g + threadIdx.x);
        __syncthreads();
        int mine = -1;
        for (int p = threadIdx.x; p <= n - g - 1; p += blockDim.x) {
            bool m = true;
            for (int i = 0; i < g; ++i) m = m && h.at(p + i) == s_tail[i];
            if (m) mine = p;  // (ascending: the thread's last hit is its largest)
        }
        if (mine >= 0) atomicMax(s_best, mine);
        __syncthreads();
        best = *s_best;
        __syncthreads();  // (the next g writes both again)
        if (best >= 0) {
            hit = g;
            break;
        }
    }
    d_start = d_len = 0;
    if (best < 0) return;
    d_start = best + hit;
    d_len = max(0, min(min(k, n - d_start), cap));
}

// chain form: workgroup c serves chain c of the burst's list
__global__ void __launch_bounds__(256) k_spec_draft(const ze_spec_step a) {
    __shared__ int s_best, s_tail[ZE_SP_MAX_K];
    const int c = blockIdx.x;
    const int slot = a.chains[ZE_SP_CHAIN_WORDS * c], row0 = a.chains[ZE_SP_CHAIN_WORDS * c + 1], rows = a.chains[ZE_SP_CHAIN_WORDS * c + 2];
    const int* t = a.table + (size_t)slot * ZE_SP_WORDS;
    const ze_seq_dev st = a.st[slot];
    const int k = min(t[0], rows - 1);
    if (k <= 0) {  // a chain without speculation rides the step with one row, fed its last token (a chain out of room: a dead row)
        if (threadIdx.x == 0) {
            a.row_tok[row0] = st.token;
            a.row_off[row0] = st.ctx < a.max_ctx ? 0 : -1;
            a.dlen[c] = 0;
        }
        return;
    }
    const int n_gen = min(min(max(st.n_gen, 0), st.max_gen), a.max_ctx);
    // rows 0 .. L need cache rows ctx .. ctx + L and emit up to L + 1 tokens
    const int cap = min(a.max_ctx - 1 - st.ctx, st.max_gen - st.n_gen - 1);
    const bool dead = st.finished != 0 || cap < 0;
    sp_hist h;
    h.seg0 = a.hist_ctx + (size_t)slot * a.max_ctx, h.l0 = min(max(t[3], 0), a.max_ctx);
    h.seg1 = a.out_tokens + (size_t)slot * a.max_ctx, h.l1 = n_gen;
    int d_start = 0, d_len = 0;
    if (!dead) spec_draft_wg(h, k, t[1], t[2], cap, &s_best, s_tail, d_start, d_len);
    const int j = threadIdx.x;
    if (j < rows) {
        const bool live = !dead && j <= d_len;
        a.row_tok[row0 + j] = j == 0 ? st.token : (live ? h.at(d_start + j - 1) : 0);
        a.row_off[row0 + j] = live ? j : -1;
    }
    if (j == 0) a.dlen[c] = dead ? -1 : d_len;
}

// unit form: the history of row r is hist[r * ld .. + lens[r])
__global__ void __launch_bounds__(256) k_spec_draft_rows(const int* __restrict__ hist, const int* __restrict__ lens, int ld, int k, int gmin,
                                                         int gmax, int* __restrict__ out_draft, int* __restrict__ out_len) {
    __shared__ int s_best, s_tail[ZE_SP_MAX_K];
    const int r = blockIdx.x;
    sp_hist h;
    h.seg0 = hist + (size_t)r * ld, h.l0 = min(max(lens[r], 0), ld), h.seg1 = h.seg0, h.l1 = 0;  // (one segment)
    int d_start = 0, d_len = 0;
    spec_draft_wg(h, k, gmin, gmax, k, &s_best, s_tail, d_start, d_len);
    const int j = threadIdx.x;
    if (j < k) out_draft[(size_t)r * k + j] = j < d_len ? h.at(d_start + j) : -1;
    if (j == 0) out_len[r] = d_len;
}

__device__ __forceinline__ void sp_better(float& bv, int& bi, float v, int i) {  // (`better` of ze_sample.hip)
    if (v > bv || (v == bv && i < bi)) {
        bv = v;
        bi = i;
    }
}

// The walk over the rows of one chain, workgroup-wide: lg = row 0 ([L + 1, ld]), draft[0 .. L), room >= 1 tokens may be emitted.
// s_acc receives the emitted tokens; returns their number (the same in every thread); *s_fin = an EOS id was emitted.
__device__ __forceinline__ int spec_accept_wg(const float* __restrict__ lg, int ld, int vocab, const uint8_t* __restrict__ seen, float penalty,
                                              const int* __restrict__ draft, int L, int room, const int* __restrict__ eos_ids, int n_eos,
                                              int ignore_eos, int* s_acc, int* s_fin, float* s_v, int* s_i, int* s_stop) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (threadIdx.x == 0) *s_fin = 0;
    int m = 0;
    for (int j = 0; j <= L; ++j) {
        const float* row = lg + (size_t)j * ld;
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int i = threadIdx.x; i < vocab; i += SP_THREADS) {
            float v = row[i];
            if (penalty != 1.0f) {
                bool sn = seen != nullptr && seen[i] != 0;
                for (int q = 0; q < j; ++q) sn = sn || s_acc[q] == i;  // the tokens this step has emitted already
                if (sn) v = v < 0.f ? v * penalty : v / penalty;
            }
            sp_better(bv, bi, v, i);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            sp_better(bv, bi, ov, oi);
        }
        if (lane == 0) {
            s_v[wid] = bv;
            s_i[wid] = bi;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < SP_THREADS / 64; ++w) sp_better(bv, bi, s_v[w], s_i[w]);
            int tok = bi;
            if ((unsigned)tok >= (unsigned)vocab) tok = 0;  // every logit NaN: torch.argmax gives 0
            s_acc[j] = tok;
            bool eos = false;
            if (!ignore_eos)
                for (int e = 0; e < n_eos; ++e) eos = eos || tok == eos_ids[e];
            if (eos) *s_fin = 1;
            *s_stop = (j == L || tok != draft[j] || eos || j + 1 >= room) ? 1 : 0;
        }
        __syncthreads();
        m = j + 1;
        if (*s_stop) break;  // (uniform; s_stop is next written behind the barrier of the next row)
    }
    return m;
}

#define SP_ACCEPT_SHARED                                \
    __shared__ int s_acc[ZE_SP_MAX_K + 1], s_fin, s_stop; \
    __shared__ float s_v[SP_THREADS / 64];              \
    __shared__ int s_i[SP_THREADS / 64]

// chain form: workgroup b serves chain first_chain + b of the burst's list
__global__ void __launch_bounds__(SP_THREADS) k_spec_accept(const ze_spec_step a, int first_chain) {
    SP_ACCEPT_SHARED;
    const int c = first_chain + blockIdx.x;
    const int slot = a.chains[ZE_SP_CHAIN_WORDS * c], row0 = a.chains[ZE_SP_CHAIN_WORDS * c + 1];
    const int L = a.dlen[c];
    if (L < 0) return;  // a dead chain: finished, or out of room
    const float penalty = __int_as_float(a.chains[ZE_SP_CHAIN_WORDS * c + 3]);
    uint8_t* seen = a.seen + (size_t)slot * a.vocab;
    const int m = spec_accept_wg(a.logits + (size_t)row0 * a.vocab, a.vocab, a.vocab, seen, penalty, a.row_tok + row0 + 1, L, L + 1, a.eos_ids,
                                 a.n_eos, a.ignore_eos, s_acc, &s_fin, s_v, s_i, &s_stop);
    if (threadIdx.x != 0) return;
    ze_seq_dev* st = a.st + slot;
    const int n_gen = st->n_gen;
    for (int q = 0; q < m; ++q) {
        if (n_gen + q < st->max_gen) a.out_tokens[(size_t)slot * a.max_ctx + n_gen + q] = s_acc[q];
        seen[s_acc[q]] = 1;
    }
    st->ctx += m;  // the rows behind it stay in the cache as dead rows, as after ze_seq_truncate
    st->n_gen = n_gen + m;
    st->token = s_acc[m - 1];
    if (s_fin) st->finished = 1;
    int* t = const_cast<int*>(a.table) + (size_t)slot * ZE_SP_WORDS;
    t[4] += 1;
    t[5] += L;
    t[6] += m - 1;
}

// unit form: chain c owns rows c * (k + 1) .. of logits [n * (k + 1), ld], draft[c * k ..], seen [n, vocab] or null
__global__ void __launch_bounds__(SP_THREADS) k_spec_accept_rows(const float* __restrict__ logits, int vocab, int ld, int k,
                                                                 const int* __restrict__ draft, const int* __restrict__ draft_len,
                                                                 uint8_t* __restrict__ seen, const float* __restrict__ penalty,
                                                                 const int* __restrict__ room, const int* __restrict__ eos_ids, int n_eos,
                                                                 int ignore_eos, int* __restrict__ out_tokens, int* __restrict__ out_count,
                                                                 int* __restrict__ out_finished) {
    SP_ACCEPT_SHARED;
    const int c = blockIdx.x;
    const int L = min(max(draft_len[c], 0), k);
    uint8_t* sn = seen ? seen + (size_t)c * vocab : nullptr;
    const int m = spec_accept_wg(logits + (size_t)c * (k + 1) * ld, ld, vocab, sn, sn ? penalty[c] : 1.0f, draft + (size_t)c * k, L,
                                 max(room[c], 1), eos_ids, n_eos, ignore_eos, s_acc, &s_fin, s_v, s_i, &s_stop);
    if (threadIdx.x != 0) return;
    for (int q = 0; q <= k; ++q) out_tokens[(size_t)c * (k + 1) + q] = q < m ? s_acc[q] : -1;
    if (sn)
        for (int q = 0; q < m; ++q) sn[s_acc[q]] = 1;
    out_count[c] = m;
    out_finished[c] = s_fin;
}

// ------------------------------------------------------------------ sampled mode (ze_seq_set_speculation_mode, mode 1)
// The token of row j is what the plain step's sampler gives on that row: the chain's request (greedy | temperature, seed, penalty,
// filter), the draw index n_gen + j on the chain's own stream, and the seen-set as of row j -- the chain's plus draft ids 0 .. j - 1,
// which ARE the tokens of rows 0 .. j - 1 whenever row j is reached.  Every row's inputs are therefore known before any row is drawn:
// the prepare pass lays them down as per-row shadows (ze_spec_draw), the per-chain sampling kernels of ze_sample.hip draw all rows at
// once with row = slot (ze_launch_sample_rows, as ze_op_sample_rows runs them: the same device functions as the plain step, so the
// same bits), and the walk compares tokens with the draft and commits as k_spec_accept does.

// the seen-set of row j: the chain's bytes, then draft ids 0 .. j - 1 (workgroup-wide; ids outside the vocabulary are skipped)
__device__ __forceinline__ void spec_seen_row(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int vocab, const int* __restrict__ draft,
                                              int j) {
    if ((vocab & 15) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
        for (int i = threadIdx.x; i < (vocab >> 4); i += blockDim.x) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
    } else {
        for (int i = threadIdx.x; i < vocab; i += blockDim.x) dst[i] = src[i];
    }
    __syncthreads();
    if ((int)threadIdx.x < j && (unsigned)draft[threadIdx.x] < (unsigned)vocab) dst[draft[threadIdx.x]] = 1;
}

// chain form: workgroup (j, b) lays down the shadow of row j of chain first_chain + b
__global__ void __launch_bounds__(256) k_spec_prepare(const ze_spec_step a, const ze_spec_draw d, int first_chain, int first_row, float temperature,
                                                      unsigned long long seed, const ze_chain_sampling* __restrict__ samp,
                                                      const float4* __restrict__ filt) {
    const int c = first_chain + blockIdx.y, j = blockIdx.x;
    const int slot = a.chains[ZE_SP_CHAIN_WORDS * c], row0 = a.chains[ZE_SP_CHAIN_WORDS * c + 1], rows = a.chains[ZE_SP_CHAIN_WORDS * c + 2];
    if (j >= rows) return;
    const int sh = row0 + j - first_row;
    const bool live = j <= a.dlen[c];  // (a dead chain: -1)
    // the chain's own request, else the call's values (chain_sampling_of of ze_sample.hip; the penalty was resolved by the host)
    ze_chain_sampling r{temperature, __int_as_float(a.chains[ZE_SP_CHAIN_WORDS * c + 3]), seed};
    if (samp) {
        const ze_chain_sampling own = samp[slot];
        if (own.penalty > 0.f) r = own;
    }
    if (!live) r = ze_chain_sampling{0.f, 1.0f, 0ull};  // a row the walk never reaches: the cheapest draw there is
    if (threadIdx.x == 0) {
        const ze_seq_dev cs = a.st[slot];
        ze_seq_dev st = {};
        st.n_gen = cs.n_gen + j;
        st.stream = cs.stream;
        d.samp[sh] = r;
        d.st[sh] = st;
        d.ids[sh] = sh;
        reinterpret_cast<float4*>(d.filt)[sh] = filt && live ? filt[slot] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (!live || r.penalty == 1.0f) return;  // (the sampler reads a seen-set under a penalty alone)
    spec_seen_row(a.seen + (size_t)slot * a.vocab, d.seen + (size_t)sh * a.vocab, a.vocab, a.row_tok + row0 + 1, j);
}

// unit form: the tables come from the host; row c * (k + 1) + j gets the seen-set of chain c as of row j
__global__ void __launch_bounds__(256) k_spec_prepare_rows(const uint8_t* __restrict__ seen, uint8_t* __restrict__ scratch, int vocab, int k,
                                                           const int* __restrict__ draft, const int* __restrict__ draft_len) {
    const int c = blockIdx.y, j = blockIdx.x;
    const int L = min(max(draft_len[c], 0), k);
    spec_seen_row(seen + (size_t)c * vocab, scratch + ((size_t)c * (k + 1) + j) * vocab, vocab, draft + (size_t)c * k, min(j, L));
}

// The walk over the drawn tokens of one chain (one thread): tok[0 .. L], draft[0 .. L), room >= 1 tokens may be emitted.  Returns the
// number emitted; *fin = an EOS id was emitted.
__device__ __forceinline__ int spec_walk_drawn(const int* __restrict__ tok, const int* __restrict__ draft, int L, int room,
                                               const int* __restrict__ eos_ids, int n_eos, int ignore_eos, int* fin) {
    *fin = 0;
    int m = 0;
    for (int j = 0; j <= L; ++j) {
        const int t = tok[j];
        bool eos = false;
        if (!ignore_eos)
            for (int e = 0; e < n_eos; ++e) eos = eos || t == eos_ids[e];
        if (eos) *fin = 1;
        m = j + 1;
        if (j == L || t != draft[j] || eos || j + 1 >= room) break;
    }
    return m;
}

// chain form: workgroup b (one wave, one thread at work) serves chain first_chain + b; the commit is k_spec_accept's
__global__ void __launch_bounds__(64) k_spec_accept_drawn(const ze_spec_step a, const int32_t* __restrict__ tok, int first_chain, int first_row) {
    if (threadIdx.x != 0) return;
    const int c = first_chain + blockIdx.x;
    const int slot = a.chains[ZE_SP_CHAIN_WORDS * c], row0 = a.chains[ZE_SP_CHAIN_WORDS * c + 1];
    const int L = a.dlen[c];
    if (L < 0) return;  // a dead chain: finished, or out of room
    const int32_t* mine = tok + row0 - first_row;
    int fin;
    const int m = spec_walk_drawn(mine, a.row_tok + row0 + 1, L, L + 1, a.eos_ids, a.n_eos, a.ignore_eos, &fin);
    uint8_t* seen = a.seen + (size_t)slot * a.vocab;
    ze_seq_dev* st = a.st + slot;
    const int n_gen = st->n_gen;
    for (int q = 0; q < m; ++q) {
        if (n_gen + q < st->max_gen) a.out_tokens[(size_t)slot * a.max_ctx + n_gen + q] = mine[q];
        seen[mine[q]] = 1;
    }
    st->ctx += m;
    st->n_gen = n_gen + m;
    st->token = mine[m - 1];
    if (fin) st->finished = 1;
    int* t = const_cast<int*>(a.table) + (size_t)slot * ZE_SP_WORDS;
    t[4] += 1;
    t[5] += L;
    t[6] += m - 1;
}

// unit form: the outputs of k_spec_accept_rows
__global__ void __launch_bounds__(64) k_spec_accept_drawn_rows(const int32_t* __restrict__ tok, int vocab, int k, const int* __restrict__ draft,
                                                               const int* __restrict__ draft_len, uint8_t* __restrict__ seen,
                                                               const int* __restrict__ room, const int* __restrict__ eos_ids, int n_eos,
                                                               int ignore_eos, int* __restrict__ out_tokens, int* __restrict__ out_count,
                                                               int* __restrict__ out_finished) {
    if (threadIdx.x != 0) return;
    const int c = blockIdx.x;
    const int L = min(max(draft_len[c], 0), k);
    const int32_t* mine = tok + (size_t)c * (k + 1);
    int fin;
    const int m = spec_walk_drawn(mine, draft + (size_t)c * k, L, max(room[c], 1), eos_ids, n_eos, ignore_eos, &fin);
    for (int q = 0; q <= k; ++q) out_tokens[(size_t)c * (k + 1) + q] = q < m ? mine[q] : -1;
    if (seen)
        for (int q = 0; q < m; ++q) seen[(size_t)c * vocab + mine[q]] = 1;
    out_count[c] = m;
    out_finished[c] = fin;
}

void ze_launch_spec_accept_sampled(const ze_spec_step& a, const ze_spec_draw& d, int first_chain, int first_row, int n_rows, float temperature,
                                   unsigned long long seed, bool draws, const ze_chain_sampling* samp, const float* filt, hipStream_t s) {
    const int n = a.n_chains - first_chain;
    if (n <= 0 || n_rows <= 0) return;
    k_spec_prepare<<<dim3(ZE_SP_MAX_K + 1, n), 256, 0, s>>>(a, d, first_chain, first_row, temperature, seed, samp, reinterpret_cast<const float4*>(filt));
    ze_launch_sample_rows(a.logits + (size_t)first_row * a.vocab, a.vocab, a.vocab, d.seen, d.st, d.ids, n_rows, d.samp, draws,
                          filt ? d.filt : nullptr, d.cuts, nullptr, d.part, d.sums, d.tok, s);
    k_spec_accept_drawn<<<n, 64, 0, s>>>(a, d.tok, first_chain, first_row);
}

// the rows' input embeddings (k_embed_tokens_batch with the ids of the row table)
__global__ void __launch_bounds__(256) k_spec_embed(const int* __restrict__ row_tok, int n, const bf16_t* __restrict__ embed,
                                                    bf16_t* __restrict__ out, int hidden) {
    const int nv = hidden >> 3;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * nv) return;
    const int b = (int)(i / nv), v = (int)(i % nv);
    *reinterpret_cast<uint4*>(out + (size_t)b * hidden + v * 8) = *reinterpret_cast<const uint4*>(embed + (size_t)row_tok[b] * hidden + v * 8);
}

void ze_launch_spec_draft(const ze_spec_step& a, hipStream_t s) {
    if (a.n_chains > 0) k_spec_draft<<<a.n_chains, 256, 0, s>>>(a);
}
void ze_launch_spec_accept(const ze_spec_step& a, int first_chain, hipStream_t s) {
    if (a.n_chains > first_chain) k_spec_accept<<<a.n_chains - first_chain, SP_THREADS, 0, s>>>(a, first_chain);
}
void ze_launch_spec_embed(const int* row_tok, int n, const bf16_t* embed, bf16_t* out, int hidden, hipStream_t s) {
    if (n > 0) k_spec_embed<<<(unsigned)(((size_t)n * (hidden >> 3) + 255) / 256), 256, 0, s>>>(row_tok, n, embed, out, hidden);
}

// ------------------------------------------------------------------ host
void ze_spec_free(ze_engine* e) {
    const ze_spec& q = e->spec;
    const ze_spec_draw& d = q.draw;
    void* dev[] = {q.table, q.row_seq, q.row_off, q.row_tok, q.chains, q.dlen, q.logits, q.partial, q.tickets,
                   d.samp,  d.st,      d.filt,    d.ids,     d.seen,   d.cuts, d.part,   d.sums,    d.tok};
    for (void* p : dev)
        if (p) hipFree(p);
}

static void write_spec(ze_engine* e, int seq, const ze_spec::chain_host& h, hipStream_t s) {
    ze_spec& q = e->spec;
    const bool was = q.host[seq].k > 0;
    q.host[seq] = h;
    q.pending[seq] = 0;
    q.n_spec += (int)(h.k > 0) - (int)was;
    if (!was && h.k <= 0) return;
    const int words[ZE_SP_WORDS] = {h.k, h.min_ngram, h.max_ngram, h.n_prompt, 0, 0, 0, 0};  // (the counters start at zero)
    ze_launch_set_ints(q.table + (size_t)seq * ZE_SP_WORDS, words, ZE_SP_WORDS, s);
}

void ze_spec_clear(ze_engine* e, int seq, hipStream_t s) {
    if (e->spec.on(seq)) write_spec(e, seq, ze_spec::chain_host{}, s);
}

// buffers that come with a first request, all or none (the engine stays usable without them)
struct sp_item {
    void** p;
    size_t bytes;
    bool zero;
};
static int alloc_all_or_none(ze_engine* e, const sp_item* items, int n, const char* msg) {
    void* got[16] = {};
    int k = 0;
    bool ok = true;
    for (; k < n; ++k) {
        if (hipMalloc(&got[k], items[k].bytes) != hipSuccess || (items[k].zero && hipMemset(got[k], 0, items[k].bytes) != hipSuccess)) {
            ok = false;
            break;
        }
    }
    // once per engine, and waited for: setters on other streams may write their entries at once
    if (ok && hipStreamSynchronize(nullptr) != hipSuccess) ok = false;
    if (!ok) {
        (void)hipGetLastError();
        for (void* p : got)
            if (p) hipFree(p);
        return ze_fail(e, ZE_ERR_NOMEM, msg);
    }
    for (k = 0; k < n; ++k) *items[k].p = got[k];
    return ZE_OK;
}

int ze_spec_alloc(ze_engine* e) {
    ze_spec& q = e->spec;
    const ze_config& c = e->cfg;
    if (q.table) return ZE_OK;
    if (q.host.empty()) q.host.assign(c.max_seqs, ze_spec::chain_host{}), q.pending.assign(c.max_seqs, 0);
    const int wparts = (c.max_ctx + 191) / 192;
    const sp_item items[] = {
        {(void**)&q.table, (size_t)c.max_seqs * ZE_SP_WORDS * sizeof(int), true},
        {(void**)&q.row_seq, ZE_SP_MAX_ROWS * sizeof(int), true},
        {(void**)&q.row_off, ZE_SP_MAX_ROWS * sizeof(int), true},
        {(void**)&q.row_tok, ZE_SP_MAX_ROWS * sizeof(int), true},
        {(void**)&q.chains, (size_t)ZE_SP_MAX_ROWS * ZE_SP_CHAIN_WORDS * sizeof(int), true},
        {(void**)&q.dlen, ZE_SP_MAX_ROWS * sizeof(int), true},
        {(void**)&q.logits, (size_t)ZE_SP_MAX_ROWS * c.vocab * sizeof(float), false},
        {(void**)&q.partial, (size_t)ZE_SP_MAX_ROWS * std::max(std::max(e->max_splits, 8), wparts) * c.heads * 132 * sizeof(float), false},
        {(void**)&q.tickets, (size_t)ZE_SP_MAX_ROWS * c.kv_heads * sizeof(unsigned), true},
    };
    return alloc_all_or_none(e, items, (int)(sizeof(items) / sizeof(items[0])), "hipMalloc of the speculation buffers failed");
}

// the per-row shadows of the sampled mode, with its first request
static int spec_alloc_draw(ze_engine* e) {
    ze_spec_draw& d = e->spec.draw;
    if (d.samp) return ZE_OK;
    const size_t R = ZE_SP_MAX_ROWS;
    const sp_item items[] = {
        {(void**)&d.samp, R * sizeof(ze_chain_sampling), true}, {(void**)&d.st, R * sizeof(ze_seq_dev), true},
        {(void**)&d.filt, R * 4 * sizeof(float), true},         {(void**)&d.ids, R * sizeof(int), true},
        {(void**)&d.seen, R * (size_t)e->cfg.vocab, true},      {(void**)&d.cuts, R * sizeof(float), true},
        {(void**)&d.part, R * 2 * 128 * sizeof(float), true},   {(void**)&d.sums, R * 128 * sizeof(float), true},
        {(void**)&d.tok, R * sizeof(int32_t), true},
    };
    return alloc_all_or_none(e, items, (int)(sizeof(items) / sizeof(items[0])), "hipMalloc of the sampled-speculation buffers failed");
}

static int set_speculation(ze_engine* e, int seq, int k, int min_ngram, int max_ngram, const int32_t* prompt_ids, int n_prompt, int mode,
                           void* stream) {
    ZE_TRY(check_seq(e, seq));
    if (mode != 0 && mode != 1) return ze_fail(e, ZE_ERR_INVALID, "mode must be 0 (greedy) or 1 (sampled)");
    const ze_config& c = e->cfg;
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    if (k == 0) {
        ze_spec_clear(e, seq, s);
        ZE_KCHECK();
        return ZE_OK;
    }
    if (k < 1 || k > ZE_SP_MAX_K) return ze_fail(e, ZE_ERR_INVALID, "k must be in [0, 8] (0 = off)");
    if (min_ngram < 1 || min_ngram > max_ngram || max_ngram > ZE_SP_MAX_K) return ze_fail(e, ZE_ERR_INVALID, "1 <= min_ngram <= max_ngram <= 8 violated");
    if (n_prompt < 0 || n_prompt > c.max_ctx) return ze_fail(e, ZE_ERR_INVALID, "n_prompt must be in [0, max_ctx]");
    if (n_prompt > 0 && !prompt_ids) return ze_fail(e, ZE_ERR_INVALID, "null prompt_ids");
    for (int i = 0; i < n_prompt; ++i)
        if (prompt_ids[i] < 0 || prompt_ids[i] >= c.vocab) return ze_fail(e, ZE_ERR_INVALID, "prompt token id out of range");
    if (e->wide_regime())
        return ze_fail(e, ZE_ERR_INVALID, "speculation needs the fragment kernels: this engine runs the row-streaming family (ze_set_decode_regime)");
    const ze_requests& r = e->req;
    if (mode == 0 && r.samp_host[seq].penalty > 0.f && r.samp_host[seq].temperature > 0.f)
        return ze_fail(e, ZE_ERR_INVALID, "speculation is greedy only: the chain has a sampled request (ze_seq_set_sampling)");
    if (mode == 0 && r.filt_host[seq].on()) return ze_fail(e, ZE_ERR_INVALID, "speculation is greedy only: the chain has a sampling filter");
    if (r.ent_host[seq].on())
        return ze_fail(e, ZE_ERR_INVALID, mode ? "speculation excludes an entropy filter on the same chain" : "speculation is greedy only: the chain has an entropy filter");
    if (r.la_host[seq].on()) return ze_fail(e, ZE_ERR_INVALID, "speculation excludes a logit adjust on the same chain");
    if (r.tr_host[seq].on()) return ze_fail(e, ZE_ERR_INVALID, "speculation excludes token rules on the same chain");
    if (r.gr_host[seq] >= 0) return ze_fail(e, ZE_ERR_INVALID, "speculation excludes a grammar on the same chain");
    if (r.lp_host[seq] >= 0) return ze_fail(e, ZE_ERR_INVALID, "speculation excludes log-probabilities on the same chain");
    ZE_TRY(ze_spec_alloc(e));
    if (mode == 1) ZE_TRY(spec_alloc_draw(e));
    if (!e->req.tr_ctx) {  // the context history of the token rules holds the prompt ids (a chain has rules or speculation, never both)
        int* ctx = nullptr;
        if (hipMalloc((void**)&ctx, (size_t)c.max_seqs * c.max_ctx * sizeof(int)) != hipSuccess) {
            (void)hipGetLastError();
            return ze_fail(e, ZE_ERR_NOMEM, "hipMalloc of the context history failed");
        }
        e->req.tr_ctx = ctx;
    }
    // (a copy from pageable memory has left the caller's array when the call returns, and is ordered on the stream)
    if (n_prompt > 0)
        ZE_HIP(hipMemcpyAsync(e->req.tr_ctx + (size_t)seq * c.max_ctx, prompt_ids, (size_t)n_prompt * sizeof(int), hipMemcpyHostToDevice, s));
    ze_spec::chain_host h;
    h.k = k, h.min_ngram = min_ngram, h.max_ngram = max_ngram, h.n_prompt = n_prompt, h.mode = mode;
    write_spec(e, seq, h, s);
    ZE_KCHECK();
    return ZE_OK;
}

extern "C" int ze_seq_set_speculation(ze_engine* e, int seq, int k, int min_ngram, int max_ngram, const int32_t* prompt_ids, int n_prompt,
                                      void* stream) {
    return set_speculation(e, seq, k, min_ngram, max_ngram, prompt_ids, n_prompt, 0, stream);
}

extern "C" int ze_seq_set_speculation_mode(ze_engine* e, int seq, int k, int min_ngram, int max_ngram, const int32_t* prompt_ids, int n_prompt,
                                           int mode, void* stream) {
    return set_speculation(e, seq, k, min_ngram, max_ngram, prompt_ids, n_prompt, mode, stream);
}

extern "C" int ze_chain_spec_stats(ze_engine* e, int seq, int* steps, int* drafted, int* accepted, void* stream) {
    ZE_TRY(check_seq(e, seq));
    int w[ZE_SP_WORDS] = {};
    if (e->spec.on(seq)) {
        hipSetDevice(e->device);
        hipStream_t s = (hipStream_t)stream;
        ZE_HIP(hipMemcpyAsync(w, e->spec.table + (size_t)seq * ZE_SP_WORDS, sizeof(w), hipMemcpyDeviceToHost, s));
        ZE_HIP(hipStreamSynchronize(s));
    }
    if (steps) *steps = w[4];
    if (drafted) *drafted = w[5];
    if (accepted) *accepted = w[6];
    return ZE_OK;
}

extern "C" int ze_op_spec_draft(ze_engine* e, const int32_t* hist_ids, const int32_t* hist_lens, int rows, int ld, int k, int min_ngram,
                                int max_ngram, int32_t* out_draft, int32_t* out_len, void* stream) {
    if (!e || !hist_ids || !hist_lens || !out_draft || !out_len) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (rows < 0 || ld < 1) return ze_fail(e, ZE_ERR_INVALID, "rows >= 0 and ld >= 1");
    if (k < 1 || k > ZE_SP_MAX_K) return ze_fail(e, ZE_ERR_INVALID, "k must be in [1, 8]");
    if (min_ngram < 1 || min_ngram > max_ngram || max_ngram > ZE_SP_MAX_K) return ze_fail(e, ZE_ERR_INVALID, "1 <= min_ngram <= max_ngram <= 8 violated");
    if (rows == 0) return ZE_OK;
    hipSetDevice(e->device);
    k_spec_draft_rows<<<rows, 256, 0, (hipStream_t)stream>>>(hist_ids, hist_lens, ld, k, min_ngram, max_ngram, out_draft, out_len);
    ZE_KCHECK();
    return ZE_OK;
}

extern "C" int ze_op_spec_accept(ze_engine* e, const float* logits, int n_chains, int vocab, int ld, int k, const int32_t* draft,
                                 const int32_t* draft_len, uint8_t* seen, const float* repetition_penalty, const int32_t* room, int ignore_eos,
                                 int32_t* out_tokens, int32_t* out_count, int32_t* out_finished, void* stream) {
    if (!e || !logits || !draft || !draft_len || !room || !out_tokens || !out_count || !out_finished) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (seen && !repetition_penalty) return ze_fail(e, ZE_ERR_INVALID, "a seen-set needs the penalties");
    if (n_chains < 0 || vocab <= 0 || vocab > e->cfg.vocab || ld < vocab) return ze_fail(e, ZE_ERR_INVALID, "n_chains >= 0, 0 < vocab <= the engine's and ld >= vocab");
    if (k < 1 || k > ZE_SP_MAX_K) return ze_fail(e, ZE_ERR_INVALID, "k must be in [1, 8]");
    if (n_chains == 0) return ZE_OK;
    hipSetDevice(e->device);
    k_spec_accept_rows<<<n_chains, SP_THREADS, 0, (hipStream_t)stream>>>(logits, vocab, ld, k, draft, draft_len, seen, repetition_penalty, room,
                                                                        e->eos_dev, e->cfg.n_eos, ignore_eos, out_tokens, out_count, out_finished);
    ZE_KCHECK();
    return ZE_OK;
}

// The sampled accept pass alone: the shadows of the n_chains x (k + 1) rows on tables built for the call (the requests, draw indices
// and filters by the host, the seen-sets by k_spec_prepare_rows), the per-chain sampling kernels over them, the walk.
extern "C" int ze_op_spec_accept_sampled(ze_engine* e, const float* logits, int n_chains, int vocab, int ld, int k, const int32_t* draft,
                                         const int32_t* draft_len, uint8_t* seen, const float* repetition_penalty, const int32_t* room,
                                         int ignore_eos, const float* temperature, const uint64_t* seed, const int32_t* sample_stream,
                                         const int32_t* index0, const int32_t* top_k, const float* top_p, const float* min_p,
                                         int32_t* out_tokens, int32_t* out_count, int32_t* out_finished, void* stream) {
    if (!e || !logits || !draft || !draft_len || !room || !out_tokens || !out_count || !out_finished || !temperature || !seed || !sample_stream || !index0)
        return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (seen && !repetition_penalty) return ze_fail(e, ZE_ERR_INVALID, "a seen-set needs the penalties");
    if (n_chains < 0 || vocab <= 0 || ld < vocab) return ze_fail(e, ZE_ERR_INVALID, "n_chains >= 0, vocab > 0 and ld >= vocab");
    if (k < 1 || k > ZE_SP_MAX_K) return ze_fail(e, ZE_ERR_INVALID, "k must be in [1, 8]");
    const bool filters = top_k || top_p || min_p;
    if (filters && !(top_k && top_p && min_p)) return ze_fail(e, ZE_ERR_INVALID, "top_k, top_p and min_p come together or not at all");
    if (n_chains == 0) return ZE_OK;
    const size_t rows = (size_t)n_chains * (k + 1);
    // one block of 4-byte words: requests (4 per row) | chain states (8) | filters (4) | row ids | cuts | tokens | arg-max partials
    // (256) | chunk sums (128), then the seen-sets as of every row (bytes); the host fills the words before the partials
    static_assert(sizeof(ze_chain_sampling) == 16 && sizeof(ze_seq_dev) == 32, "table strides");
    const size_t o_samp = 0, o_st = o_samp + 4 * rows, o_filt = o_st + 8 * rows, o_ids = o_filt + 4 * rows, o_cut = o_ids + rows, o_tok = o_cut + rows,
                 o_part = o_tok + rows, o_sum = o_part + 256 * rows, o_seen = o_sum + 128 * rows, words = o_seen + (seen ? (rows * vocab + 3) / 4 : 0);
    std::vector<int32_t> host(o_part, 0);
    bool draws = false;
    for (int c = 0; c < n_chains; ++c) {
        if (!(std::isfinite(temperature[c]) && temperature[c] >= 0.f)) return ze_fail(e, ZE_ERR_INVALID, "temperature must be finite and >= 0 (0 = greedy)");
        const float pen = seen ? repetition_penalty[c] : 1.0f;
        if (!(std::isfinite(pen) && pen > 0.f)) return ze_fail(e, ZE_ERR_INVALID, "repetition_penalty must be finite and > 0 (1 = off)");
        if (index0[c] < 0) return ze_fail(e, ZE_ERR_INVALID, "index0 must be >= 0");
        if (filters) ZE_TRY(ze_check_filter(e, top_k[c], top_p[c], min_p[c]));
        draws |= temperature[c] > 0.f;
        for (int j = 0; j <= k; ++j) {
            const size_t r = (size_t)c * (k + 1) + j;
            const ze_chain_sampling req{temperature[c], pen, temperature[c] > 0.f ? (unsigned long long)seed[c] : 0ull};
            memcpy(&host[o_samp + 4 * r], &req, sizeof(req));
            ze_seq_dev st;
            memset(&st, 0, sizeof(st));
            st.n_gen = index0[c] + j;
            st.stream = sample_stream[c];
            memcpy(&host[o_st + 8 * r], &st, sizeof(st));
            host[o_ids + r] = (int32_t)r;
            if (filters) {
                host[o_filt + 4 * r] = top_k[c];
                memcpy(&host[o_filt + 4 * r + 1], &top_p[c], sizeof(float));
                memcpy(&host[o_filt + 4 * r + 2], &min_p[c], sizeof(float));
            }
        }
    }
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    int32_t* dev = nullptr;
    ZE_HIP(hipMalloc((void**)&dev, words * sizeof(int32_t)));
    int r = ZE_OK;
    if (hipMemcpyAsync(dev, host.data(), host.size() * sizeof(int32_t), hipMemcpyHostToDevice, s) != hipSuccess)
        r = ze_fail(e, ZE_ERR_HIP, "hipMemcpyAsync failed");
    if (r == ZE_OK) {
        uint8_t* scratch = seen ? reinterpret_cast<uint8_t*>(dev + o_seen) : nullptr;
        if (seen) k_spec_prepare_rows<<<dim3(k + 1, n_chains), 256, 0, s>>>(seen, scratch, vocab, k, draft, draft_len);
        ze_launch_sample_rows(logits, vocab, ld, scratch, reinterpret_cast<const ze_seq_dev*>(dev + o_st), dev + o_ids, (int)rows,
                              reinterpret_cast<const ze_chain_sampling*>(dev + o_samp), draws,
                              filters ? reinterpret_cast<const float*>(dev + o_filt) : nullptr, reinterpret_cast<float*>(dev + o_cut), nullptr,
                              reinterpret_cast<float*>(dev + o_part), reinterpret_cast<float*>(dev + o_sum), dev + o_tok, s);
        k_spec_accept_drawn_rows<<<n_chains, 64, 0, s>>>(dev + o_tok, vocab, k, draft, draft_len, seen, room, e->eos_dev, e->cfg.n_eos, ignore_eos,
                                                        out_tokens, out_count, out_finished);
    }
    if (r == ZE_OK && hipGetLastError() != hipSuccess) r = ze_fail(e, ZE_ERR_HIP, "sampled accept launch failed");
    if (hipStreamSynchronize(s) != hipSuccess && r == ZE_OK) r = ze_fail(e, ZE_ERR_HIP, "hipStreamSynchronize failed");
    hipFree(dev);
    return r;
}

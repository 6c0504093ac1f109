// Per-chain token rules (include/zoomearth.h, ze_seq_set_token_rules): the rules that depend on the SEQUENCE of a chain's tokens.
//   ban pass   HF's NoRepeatNGramLogitsProcessor and NoBadWordsLogitsProcessor: -inf at every id that would complete an n-gram the
//              history (context + generated ids) already holds, and at the last id of every ban record whose first m - 1 ids are
//              the history's last m - 1.  Runs before the sampler of a step, in place on the adjusted copy of the step's rows
//              (ze_logit_adjust.hip), so -inf meets the additive terms, the EOS mask and the repetition penalty in HF's order.
//   stop pass  a whole stop record found at the tail of the GENERATED ids finishes the chain (never reaching into the context,
//              not while fewer than min_new_tokens were generated).  Runs after the step's token was accepted.
// One workgroup per chain row.  The history is streamed once, 16 bytes a thread where the segment's alignment allows; the tail
// (at most 15 ids) and the packed records sit in LDS.  A ban is an idempotent store of one constant: no atomics, no ordering,
// and a row's bits depend on its own chain alone -- the same whatever the batch, the slot, graph or eager.  The restatement is
// tests/token_rules_ref.py.
#include "ze_kernels.h"

#define TR_THREADS 256
#define TR_STOP_THREADS 64  // one thread per stop record

struct ze_tr_args {
    float* rows;  // ban pass: [n, ld], written in place
    int vocab, ld;
    // unit form (st == null): history of row r = hist[hist_off[r] .. hist_off[r + 1]), its first n_ctx[r] ids the context;
    // records of row r = list[list_off[r] .. list_off[r + 1])
    const int *hist, *hist_off, *n_ctx, *ngram, *list, *list_off, *min_new;
    int* out_stop;
    // chain form: row b is chain slot seq_ids ? seq_ids[b] : slot0; table = ZE_TR_WORDS ints per slot, lists [slots,
    // ZE_MAX_RULE_INTS], ctx [slots, max_ctx] or null, la_table = the logit-adjust table (word 2: min_new_tokens)
    ze_seq_dev* st;
    const int* seq_ids;
    int slot0;
    const int *table, *lists, *ctx, *out_tokens, *la_table;
    int max_ctx;
};

// the record thread r owns in a packed list of n ints staged in LDS: its offset (of the length word), or -1
__device__ __forceinline__ int tr_record(const int* recs, int n, int r) {
    int off = 0;
    for (int i = 0; i < r && off < n; ++i) {
        const int len = recs[off];
        if (len < 1 || len > ZE_MAX_RULE_LEN) return -1;
        off += 1 + len;
    }
    if (off >= n) return -1;
    const int len = recs[off];
    return (len >= 1 && len <= ZE_MAX_RULE_LEN && off + 1 + len <= n) ? off : -1;
}

struct tr_hist {
    const int *seg0, *seg1;  // context ids, generated ids
    int l0, l1;
    __device__ __forceinline__ int at(int i) const { return i < l0 ? seg0[i] : seg1[i - l0]; }
};

// id sits at history index j with predecessor prev: banned when the n - 1 ids before j are the history's last n - 1
__device__ __forceinline__ void tr_candidate(const tr_hist& h, const int* tail, int n, int j, int id, int prev, float* out, int vocab) {
    if (j < n - 1) return;
    if (n >= 2 && prev != tail[1]) return;
    for (int k = 2; k < n; ++k)
        if (h.at(j - k) != tail[k]) return;
    if ((unsigned)id < (unsigned)vocab) out[id] = -INFINITY;
}

__device__ __forceinline__ void tr_scan(const tr_hist& h, const int* seg, int len, int g0, const int* tail, int n, float* out, int vocab) {
    if (len <= 0) return;
    const int tid = threadIdx.x;
    const int mis = min(len, (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(seg) & 15u)) & 15u) >> 2));
    const int nv = (len - mis) >> 2;
    for (int i = tid; i < mis; i += TR_THREADS) tr_candidate(h, tail, n, g0 + i, seg[i], g0 + i > 0 ? h.at(g0 + i - 1) : -1, out, vocab);
    const int4* v = reinterpret_cast<const int4*>(seg + mis);
    for (int q = tid; q < nv; q += TR_THREADS) {
        const int4 x = v[q];
        const int j = g0 + mis + 4 * q;
        tr_candidate(h, tail, n, j, x.x, j > 0 ? h.at(j - 1) : -1, out, vocab);
        tr_candidate(h, tail, n, j + 1, x.y, x.x, out, vocab);
        tr_candidate(h, tail, n, j + 2, x.z, x.y, out, vocab);
        tr_candidate(h, tail, n, j + 3, x.w, x.z, out, vocab);
    }
    for (int i = mis + 4 * nv + tid; i < len; i += TR_THREADS)
        tr_candidate(h, tail, n, g0 + i, seg[i], g0 + i > 0 ? h.at(g0 + i - 1) : -1, out, vocab);
}

__global__ void __launch_bounds__(TR_THREADS) k_token_ban(const ze_tr_args a) {
    __shared__ int tail[ZE_MAX_RULE_LEN];       // tail[k] = history[L - k], k = 1 .. 15
    __shared__ int recs[ZE_MAX_RULE_INTS];
    const int b = blockIdx.x, tid = threadIdx.x;
    int n = 0, nbi = 0;
    const int* ban = nullptr;
    tr_hist h{nullptr, nullptr, 0, 0};
    if (a.st) {
        const int slot = a.seq_ids ? a.seq_ids[b] : a.slot0;
        const int* t = a.table + (size_t)slot * ZE_TR_WORDS;
        n = t[0], nbi = t[3];
        if (n <= 0 && nbi <= 0) return;  // (uniform: the whole workgroup leaves) a chain without bans: its row stays as it is
        const ze_seq_dev c = a.st[slot];
        if (c.finished) return;          // it emits pad whatever the row holds
        ban = a.lists + (size_t)slot * ZE_MAX_RULE_INTS;
        h.l0 = a.ctx ? min(max(t[5], 0), a.max_ctx) : 0;
        h.seg0 = a.ctx ? a.ctx + (size_t)slot * a.max_ctx : nullptr;
        h.l1 = min(min(max(c.n_gen, 0), c.max_gen), a.max_ctx);
        h.seg1 = a.out_tokens + (size_t)slot * a.max_ctx;
    } else {
        n = a.ngram[b];
        const int o = a.list_off[b];
        nbi = a.list_off[b + 1] - o;
        if (n <= 0 && nbi <= 0) return;
        ban = a.list + o;
        const int ho = a.hist_off[b], len = max(a.hist_off[b + 1] - ho, 0);
        h.l0 = min(max(a.n_ctx[b], 0), len);
        h.seg0 = a.hist + ho;
        h.l1 = len - h.l0;
        h.seg1 = h.seg0 + h.l0;
    }
    n = min(n, ZE_MAX_RULE_LEN);
    nbi = min(max(nbi, 0), ZE_MAX_RULE_INTS);
    float* out = a.rows + (size_t)b * a.ld;
    const int L = h.l0 + h.l1;
    if (tid >= 1 && tid < ZE_MAX_RULE_LEN) tail[tid] = tid <= L ? h.at(L - tid) : -1;
    for (int i = tid; i < nbi; i += TR_THREADS) recs[i] = ban[i];
    __syncthreads();
    if (tid < ZE_MAX_RULE_WORDS && nbi > 0) {
        const int off = tr_record(recs, nbi, tid);
        if (off >= 0) {
            const int m = recs[off];
            bool hit = m - 1 <= L;
            for (int k = 1; k < m && hit; ++k) hit = tail[k] == recs[off + m - k];  // record id m - 1 - k against history[L - k]
            const int id = recs[off + m];
            if (hit && (unsigned)id < (unsigned)a.vocab) out[id] = -INFINITY;
        }
    }
    if (n < 1 || L < n - 1) return;
    tr_scan(h, h.seg0, h.l0, 0, tail, n, out, a.vocab);
    tr_scan(h, h.seg1, h.l1, h.l0, tail, n, out, a.vocab);
}

__global__ void __launch_bounds__(TR_STOP_THREADS) k_token_stop(const ze_tr_args a) {
    __shared__ int recs[ZE_MAX_RULE_INTS];
    __shared__ int hit;
    const int b = blockIdx.x, tid = threadIdx.x;
    int nsi = 0, ng = 0, min_new = 0, slot = 0;
    const int *stop = nullptr, *gen = nullptr;
    if (a.st) {
        slot = a.seq_ids ? a.seq_ids[b] : a.slot0;
        nsi = a.table[(size_t)slot * ZE_TR_WORDS + 1];
        if (nsi <= 0) return;  // (uniform)
        const ze_seq_dev c = a.st[slot];
        if (c.finished) return;  // never un-finished, and its pads are no text
        stop = a.lists + (size_t)slot * ZE_MAX_RULE_INTS;
        ng = min(min(max(c.n_gen, 0), c.max_gen), a.max_ctx);
        gen = a.out_tokens + (size_t)slot * a.max_ctx;
        min_new = a.la_table[(size_t)slot * ZE_LA_WORDS + 2];
    } else {
        const int o = a.list_off[b];
        nsi = a.list_off[b + 1] - o;
        stop = a.list + o;
        const int ho = a.hist_off[b], len = max(a.hist_off[b + 1] - ho, 0), l0 = min(max(a.n_ctx[b], 0), len);
        ng = len - l0;
        gen = a.hist + ho + l0;
        min_new = a.min_new[b];
    }
    nsi = min(max(nsi, 0), ZE_MAX_RULE_INTS);
    if (tid == 0) hit = 0;
    for (int i = tid; i < nsi; i += TR_STOP_THREADS) recs[i] = stop[i];
    __syncthreads();
    if (ng >= min_new && nsi > 0) {
        const int off = tr_record(recs, nsi, tid);
        if (off >= 0) {
            const int m = recs[off];
            bool eq = m <= ng;  // the whole record inside the generated ids
            for (int i = 0; i < m && eq; ++i) eq = gen[ng - m + i] == recs[off + 1 + i];
            if (eq) hit = 1;
        }
    }
    __syncthreads();
    if (tid != 0) return;
    if (a.st) {
        if (hit) a.st[slot].finished = 1;
    } else {
        a.out_stop[b] = hit;
    }
}

void ze_launch_token_ban(float* rows, int n, int vocab, int ld, const int* hist, const int* hist_off, const int* n_ctx, const int* ngram,
                         const int* ban, const int* ban_off, hipStream_t s) {
    if (n <= 0 || vocab <= 0) return;
    ze_tr_args a{};
    a.rows = rows, a.vocab = vocab, a.ld = ld, a.hist = hist, a.hist_off = hist_off, a.n_ctx = n_ctx, a.ngram = ngram;
    a.list = ban, a.list_off = ban_off;
    k_token_ban<<<n, TR_THREADS, 0, s>>>(a);
}

void ze_launch_token_stop(int n, const int* hist, const int* hist_off, const int* n_ctx, const int* stop, const int* stop_off,
                          const int* min_new, int* out_stop, hipStream_t s) {
    if (n <= 0) return;
    ze_tr_args a{};
    a.hist = hist, a.hist_off = hist_off, a.n_ctx = n_ctx, a.list = stop, a.list_off = stop_off, a.min_new = min_new;
    a.out_stop = out_stop;
    k_token_stop<<<n, TR_STOP_THREADS, 0, s>>>(a);
}

void ze_launch_chain_token_ban(float* rows, int vocab, ze_seq_dev* st, const int* seq_ids, int slot0, int n, const ze_token_rule_bufs& tr,
                               const int* out_tokens, int max_ctx, hipStream_t s) {
    if (n <= 0 || vocab <= 0) return;
    ze_tr_args a{};
    a.rows = rows, a.vocab = vocab, a.ld = vocab, a.st = st, a.seq_ids = seq_ids, a.slot0 = slot0;
    a.table = tr.table, a.lists = tr.ban, a.ctx = tr.ctx, a.out_tokens = out_tokens, a.max_ctx = max_ctx;
    k_token_ban<<<n, TR_THREADS, 0, s>>>(a);
}

void ze_launch_chain_token_stop(ze_seq_dev* st, const int* seq_ids, int slot0, int n, const ze_token_rule_bufs& tr, const int* la_table,
                                const int* out_tokens, int max_ctx, hipStream_t s) {
    if (n <= 0) return;
    ze_tr_args a{};
    a.st = st, a.seq_ids = seq_ids, a.slot0 = slot0, a.table = tr.table, a.lists = tr.stop, a.la_table = la_table;
    a.out_tokens = out_tokens, a.max_ctx = max_ctx;
    k_token_stop<<<n, TR_STOP_THREADS, 0, s>>>(a);
}

struct ze_tr_words {
    int v[ZE_TR_WORDS];
};
__global__ void k_set_token_rules(int* table, int slot, ze_tr_words w) {
    if (threadIdx.x < ZE_TR_WORDS) table[(size_t)slot * ZE_TR_WORDS + threadIdx.x] = w.v[threadIdx.x];
}
void ze_launch_set_token_rules(int* table, int slot, int ngram, int n_stop_ints, int n_stop_words, int n_ban_ints, int n_ban_words,
                               int n_context, hipStream_t s) {
    ze_tr_words w{};
    w.v[0] = ngram, w.v[1] = n_stop_ints, w.v[2] = n_stop_words, w.v[3] = n_ban_ints, w.v[4] = n_ban_words, w.v[5] = n_context;
    k_set_token_rules<<<1, ZE_TR_WORDS, 0, s>>>(table, slot, w);
}

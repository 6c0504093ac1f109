// Guided decoding (include/zoomearth.h, ze_grammar_create / ze_seq_set_grammar): a deterministic token automaton per grammar, shared by
// the chains that use it and immutable on the device, and a (grammar, state) word per chain.
//   build     once per grammar: allow[state, word] -- bit t % 32 of word t / 32 is set when token t may follow in `state`, from
//             token_class and trans; the bits of the EOS ids come from accepting[state] (their class is never looked at).
//   mask      before the sampler of a step, in place on the adjusted copy of the step's rows (ze_logit_adjust.hip), behind the adjust
//             kernel and the ban pass: -inf wherever the bit of the chain's state is clear.  The row is not read: the pass loads
//             ceil(vocab / 8) bytes of mask per chain and stores one constant, four ids a thread (one 16-byte store where all four are
//             banned, the common case: a state allows about 1 % of the ids).  Idempotent stores, no atomics, no ordering, and a
//             row's bits depend on its own chain alone -- the same whatever the batch, the slot, graph or eager.
//   advance   after the step's token was accepted, one thread per chain: state = trans[state][token_class[token]].
// The mask is elementwise, so its grid is the one of ze_logit_adjust.hip: vocabulary chunks x rows -- one live chain still spreads
// over the CUs.  The restatement is tests/grammar_ref.py.
#include "ze_kernels.h"

#define GR_THREADS 256
#define GR_GROUPS 2                             // groups of four ids per thread
#define GR_CHUNK (GR_THREADS * GR_GROUPS * 4)   // ids of a row per workgroup (64 mask words)

struct ze_gr_args {
    float* rows;  // mask: [n, ld], written in place
    int vocab, ld;
    const int* eos_ids;
    int n_eos;
    // unit form (st == null): every row under grammar g; states[r] = the row's state (-1: a row without a grammar), tokens[r] and
    // out_states[r] for the advance
    ze_grammar_dev g;
    const int *states, *tokens;
    int* out_states;
    // chain form: row b is chain slot seq_ids ? seq_ids[b] : slot0; table = ZE_GR_WORDS ints per slot; grammars [ZE_MAX_GRAMMARS]
    ze_seq_dev* st;
    const int* seq_ids;
    int slot0, n;
    int* table;
    const ze_grammar_dev* grammars;
    const int* out_tokens;
    int max_ctx;
};

__global__ void __launch_bounds__(256) k_grammar_build(const ze_grammar_dev g, int vocab, const int* __restrict__ eos_ids, int n_eos,
                                                       uint32_t* __restrict__ allow) {
    const int w = blockIdx.x * 256 + threadIdx.x, state = blockIdx.y;
    if (w >= g.words) return;
    const int16_t* tr = g.trans + (size_t)state * g.n_classes;
    const bool acc = g.accepting[state] != 0;
    uint32_t bits = 0;
    for (int k = 0; k < 32; ++k) {
        const int t = w * 32 + k;
        if (t >= vocab) break;
        bool eos = false;
        for (int j = 0; j < n_eos; ++j) eos |= eos_ids[j] == t;
        const int cls = g.token_class[t];
        const bool ok = eos ? acc : (cls < g.n_classes && tr[cls] >= 0);
        bits |= (uint32_t)ok << k;
    }
    allow[(size_t)state * g.words + w] = bits;
}

__global__ void __launch_bounds__(GR_THREADS) k_grammar_mask(const ze_gr_args a) {
    const int b = blockIdx.y, tid = threadIdx.x;
    ze_grammar_dev g;
    int state;
    // (every exit below is uniform: the whole workgroup leaves)
    if (a.st) {
        const int slot = a.seq_ids ? a.seq_ids[b] : a.slot0;
        const int* t = a.table + (size_t)slot * ZE_GR_WORDS;
        const int id = t[0] - 1;
        if (id < 0 || id >= ZE_MAX_GRAMMARS) return;  // a chain without a grammar: its row stays as it is
        if (a.st[slot].finished) return;              // it emits pad whatever the row holds
        g = a.grammars[id];
        state = t[1];
    } else {
        g = a.g;
        state = a.states[b];
    }
    if (state < 0 || state >= g.n_states) return;
    const uint32_t* allow = g.allow + (size_t)state * g.words;
    float* out = a.rows + (size_t)b * a.ld;
    const bool vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const int lo = blockIdx.x * GR_CHUNK;
    uint32_t w[GR_GROUPS];
#pragma unroll
    for (int u = 0; u < GR_GROUPS; ++u) {
        const int i = lo + (u * GR_THREADS + tid) * 4;
        w[u] = i < a.vocab ? allow[i >> 5] : 0xffffffffu;  // (vocab <= 32 * words)
    }
#pragma unroll
    for (int u = 0; u < GR_GROUPS; ++u) {
        const int i = lo + (u * GR_THREADS + tid) * 4;
        if (i >= a.vocab) continue;
        const uint32_t nib = (w[u] >> (i & 31)) & 0xfu;  // i is a multiple of 4: its four bits share a word
        if (nib == 0u && vec && i + 3 < a.vocab) {
            *reinterpret_cast<float4*>(out + i) = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i + k < a.vocab && !((nib >> k) & 1u)) out[i + k] = -INFINITY;
        }
    }
}

// the state after `tok` in `state`, or -1 when the automaton does not allow it.  An EOS id keeps the state (allowed in an accepting one)
__device__ __forceinline__ int gr_next(const ze_grammar_dev& g, int state, int tok, int vocab, const int* eos_ids, int n_eos) {
    if ((unsigned)state >= (unsigned)g.n_states || (unsigned)tok >= (unsigned)vocab) return -1;
    for (int j = 0; j < n_eos; ++j)
        if (eos_ids[j] == tok) return g.accepting[state] ? state : -1;
    const int cls = g.token_class[tok];
    return cls < g.n_classes ? (int)g.trans[(size_t)state * g.n_classes + cls] : -1;
}

__global__ void __launch_bounds__(64) k_grammar_advance(const ze_gr_args a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.n) return;
    if (!a.st) {
        a.out_states[b] = gr_next(a.g, a.states[b], a.tokens[b], a.vocab, a.eos_ids, a.n_eos);
        return;
    }
    const int slot = a.seq_ids ? a.seq_ids[b] : a.slot0;
    int* t = a.table + (size_t)slot * ZE_GR_WORDS;
    const int id = t[0] - 1;
    if (id < 0 || id >= ZE_MAX_GRAMMARS) return;
    if (t[3]) return;  // the chain had finished before this step: its token is a pad
    const ze_seq_dev c = a.st[slot];
    if (c.n_gen <= 0) return;
    const int ng = min(min(c.n_gen, c.max_gen), a.max_ctx);
    const int tok = ng == c.n_gen ? a.out_tokens[(size_t)slot * a.max_ctx + ng - 1] : c.token;
    const int next = gr_next(a.grammars[id], t[1], tok, a.vocab, a.eos_ids, a.n_eos);
    if (next >= 0)
        t[1] = next;
    else
        t[2] = 1;  // (only when other requests banned every allowed id and the arg-max of an all -inf row fell on id 0)
    t[3] = c.finished;
}

void ze_launch_grammar_build(const ze_grammar_dev& g, int vocab, const int* eos_ids, int n_eos, uint32_t* allow, hipStream_t s) {
    if (g.n_states <= 0 || g.words <= 0) return;
    k_grammar_build<<<dim3(ze_cdiv(g.words, 256), g.n_states), 256, 0, s>>>(g, vocab, eos_ids, n_eos, allow);
}

void ze_launch_grammar_mask(float* rows, int n, int vocab, int ld, const ze_grammar_dev& g, const int* states, hipStream_t s) {
    if (n <= 0 || vocab <= 0) return;
    ze_gr_args a{};
    a.rows = rows, a.vocab = vocab, a.ld = ld, a.g = g, a.states = states;
    k_grammar_mask<<<dim3(ze_cdiv(vocab, GR_CHUNK), n), GR_THREADS, 0, s>>>(a);
}

void ze_launch_grammar_advance(int n, int vocab, const ze_grammar_dev& g, const int* states, const int* tokens, const int* eos_ids,
                               int n_eos, int* out_states, hipStream_t s) {
    if (n <= 0) return;
    ze_gr_args a{};
    a.n = n, a.vocab = vocab, a.g = g, a.states = states, a.tokens = tokens, a.eos_ids = eos_ids, a.n_eos = n_eos, a.out_states = out_states;
    k_grammar_advance<<<ze_cdiv(n, 64), 64, 0, s>>>(a);
}

void ze_launch_chain_grammar_mask(float* rows, int vocab, ze_seq_dev* st, const int* seq_ids, int slot0, int n, const ze_grammar_bufs& gr,
                                  hipStream_t s) {
    if (n <= 0 || vocab <= 0) return;
    ze_gr_args a{};
    a.rows = rows, a.vocab = vocab, a.ld = vocab, a.st = st, a.seq_ids = seq_ids, a.slot0 = slot0, a.table = gr.table, a.grammars = gr.grammars;
    k_grammar_mask<<<dim3(ze_cdiv(vocab, GR_CHUNK), n), GR_THREADS, 0, s>>>(a);
}

void ze_launch_chain_grammar_advance(ze_seq_dev* st, const int* seq_ids, int slot0, int n, const ze_grammar_bufs& gr, int vocab,
                                     const int* eos_ids, int n_eos, const int* out_tokens, int max_ctx, hipStream_t s) {
    if (n <= 0) return;
    ze_gr_args a{};
    a.n = n, a.vocab = vocab, a.eos_ids = eos_ids, a.n_eos = n_eos, a.st = st, a.seq_ids = seq_ids, a.slot0 = slot0, a.table = gr.table;
    a.grammars = gr.grammars, a.out_tokens = out_tokens, a.max_ctx = max_ctx;
    k_grammar_advance<<<ze_cdiv(n, 64), 64, 0, s>>>(a);
}

struct ze_gr_words {
    int v[ZE_GR_WORDS];
};
__global__ void k_set_grammar(int* table, int slot, ze_gr_words w) {
    if (threadIdx.x < ZE_GR_WORDS) table[(size_t)slot * ZE_GR_WORDS + threadIdx.x] = w.v[threadIdx.x];
}
void ze_launch_set_grammar(int* table, int slot, int grammar, int state, hipStream_t s) {
    ze_gr_words w{};
    w.v[0] = grammar + 1, w.v[1] = grammar >= 0 ? state : 0;  // (a request starts from a live chain that violated nothing)
    k_set_grammar<<<1, ZE_GR_WORDS, 0, s>>>(table, slot, w);
}

__global__ void k_set_grammar_desc(ze_grammar_dev* grammars, int id, ze_grammar_dev g) {
    grammars[id] = g;
}
void ze_launch_set_grammar_desc(ze_grammar_dev* grammars, int id, const ze_grammar_dev& g, hipStream_t s) {
    k_set_grammar_desc<<<1, 1, 0, s>>>(grammars, id, g);
}

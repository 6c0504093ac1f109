// ze_engine: owns the packed bf16 weight arena, the KV cache, chain state and workspaces of one GPU.
//
// HBM layout (3B config, sizes for max_seqs=4, max_ctx=4096):
//   weight arena  (one hipMalloc, ~7.5 GB bf16)   all matrices [N, K] row-major, K contiguous (the MFMA / GEMV feed)
//       ViT   : patch_embed [1280,1176]; per block qkv [3840,1280]+b, proj [1280,1280]+b,
//               gate_up [2*3424,1280]+b (gate/up rows interleaved in blocks of 16, zero padded 3420->3424),
//               down [1280,3424]+b (K zero padded); merger ln_q, mlp.0 [5120,5120]+b, mlp.2 [2048,5120]+b
//       LLM   : embed_tokens [151936,2048] (= lm_head when tied); per layer qkv [2560,2048]+b (q|k|v stacked),
//               o [2048,2048], gate_up [2*11008,2048] (interleaved), down [2048,11008]; norms
//   KV cache      [layers][max_seqs][kv_heads][max_ctx][128] bf16, K and V separate (36,864 B per cached token)
//   tables        text cos/sin bf16 [max_ctx + 512][64]; normalise LUT f32 [3][256]
//   chain state   ze_seq_dev[max_seqs], seen-set u8 [max_seqs][vocab], out tokens int32 [max_seqs][max_ctx]
//   workspaces    ViT activations for max_patches rows; prefill activations for max_ctx rows; decode vectors
#pragma once
#include <algorithm>
#include <functional>
#include <map>
#include <tuple>
#include <set>
#include <string>
#include <vector>

#include "ze_host.h"
#include "ze_kernels.h"

struct ze_linear {
    bf16_t* w = nullptr;
    bf16_t* bias = nullptr;
    int n = 0, k = 0, ld = 0;
    // fp8 decode copy (ze_weights_quantize_fp8): E4M3 bytes [n, ld8] + per-row scale exponent applied as 2^k
    uint8_t* w8 = nullptr;
    float* scale8 = nullptr;
    int ld8 = 0;
    // MXFP4 decode copy (ze_weights_quantize_mxfp4): E2M1 codes [n, k / 2] + E8M0 block scales [n, k / 32], null = none (the two
    // formats exclude each other; a tensor whose k is not a multiple of 32 keeps its bf16 stream)
    uint8_t* w4 = nullptr;
    uint8_t* scale4 = nullptr;
    // MFMA-fragment-major copy for the batched decode step (ze_launch_pack_fragments), null = none
    bf16_t* wf = nullptr;
    // qkv only, row-streaming regime: rows (and bias) permuted per head for the rope + KV-append epilogue (ze_launch_permute_qkv)
    bf16_t* wp = nullptr;
    bf16_t* bias_p = nullptr;
    // the same in FP8 (ze_launch_pack_fragments8 of w8), streamed with scale8 when the engine is quantised, null = none
    uint8_t* wf8 = nullptr;
    // the same in MXFP4 (ze_launch_pack_fragments4 of w4 / scale4): codes and fragment-major block scales, streamed by the W4 kernels
    // of the 2 .. 64-chain step on an MXFP4 engine (such a tensor then has no bf16 fragments: wf stays null), null = none
    uint8_t* wf4 = nullptr;
    uint8_t* sf4 = nullptr;
    bool has_frag() const { return wf || wf4; }
};
struct ze_vit_block {
    bf16_t *norm1 = nullptr, *norm2 = nullptr;
    ze_linear qkv, proj, gate_up, down;
};
struct ze_text_layer {
    bf16_t *in_norm = nullptr, *post_norm = nullptr;
    ze_linear qkv, o, gate_up, down;
};
// where an HF tensor lands in the packed arena
struct ze_dest {
    bf16_t* dst = nullptr;
    int rows = 0, cols = 0, ld = 0, mode = 0, offset = 0;
    int kind = 0;  // 0 matrix, 1 norm weight, 2 bias, 3 embedding / lm_head
};

// What a captured decode step was captured under: every value its launch sequence or a kernel argument depends on.  Built in one
// place, ze_step_key_of (ze_requests.hip); a request kind that changes what a step launches adds its mode here and there.
enum { ZE_STEP_SAMPLED = 0, ZE_STEP_UNSAMPLED = 1, ZE_STEP_SPEC = 2 };
struct ze_step_key {
    int n = 0;  // rows of a batched step; 0 = the single-chain step
    int kind = ZE_STEP_SAMPLED;     // batched step: with its sampler, without it (beam search), or speculative (draft .. accept)
    int n_plain = 0, n_chains = 0;  // speculative step only: the rows the sampler takes, the chains the drafter and the accept pass walk
    int n_drawn = 0, n_drawn_rows = 0;  // ... the last of those chains that speculate in sampled mode, and their rows (the step's last): the drawn accept pass
    float penalty = 0.f;
    int ignore_eos = 0;
    float temperature = 0.f;
    unsigned long long seed = 0;
    unsigned tune_epoch = 0;                   // single-chain step only (the batched graphs are flushed when the epoch changes)
    int live_parts = 0, live_parts_long = 0;   // batched step only: the attention grids' extents
    int sampling_bits = 0;                     // bit 0 = sampling filters, bit 1 = per-chain sampling table, bit 2 = ... with a draw, bit 3 = entropy filters
    int lp_mode = 0, la_mode = 0, tr_mode = 0, gr_mode = 0;
    auto tied() const {
        return std::tie(n, kind, n_plain, n_chains, n_drawn, n_drawn_rows, penalty, ignore_eos, temperature, seed, tune_epoch, live_parts, live_parts_long, sampling_bits, lp_mode, la_mode,
                        tr_mode, gr_mode);
    }
    bool operator==(const ze_step_key& o) const { return tied() == o.tied(); }
    bool operator<(const ze_step_key& o) const { return tied() < o.tied(); }
};

// Per-chain requests (ze_requests.hip: the setters, what a step launches for them, and the keys of the captured steps).  Each kind
// keeps its truth on the host, a per-slot device table written in stream order by its setter, a count of the slots that have
// one, and buffers allocated by the first request that needs them.  A step launches nothing for a kind no chain has asked for.
struct ze_requests {
    // Sampling filters (ze_seq_set_sampling_filter): filt_host is the truth, filt_dev the per-slot table the selection kernel reads
    // ((top_k bits, top_p, min_p, 0) per slot; all zero = off), written in stream order by the setter; n_filters = slots with a
    // filter.  While it is 0 no sampling launch knows about filters at all.  cut_dev: [max_seqs] cuts of a batched step (one per
    // row of the launch), then [max_seqs] for the single-chain launches (one per slot).
    struct filter_host { int top_k = 0; float top_p = 1.f, min_p = 0.f; bool on() const { return top_k > 0 || top_p < 1.f || min_p > 0.f; } };
    std::vector<filter_host> filt_host;
    int n_filters = 0;
    float *filt_dev = nullptr, *cut_dev = nullptr;
    // Entropy filters (ze_seq_set_entropy_filter: typical / epsilon / eta), kept like the sampling filters: ent_host the truth,
    // ent_dev the per-slot table the band selection reads ((typical_p, epsilon_cutoff, eta_cutoff, 0) per slot; all zero = off),
    // n_entropy = slots with one.  While it is 0 no sampling launch knows about bands at all.  ceil_dev: the ceilings, laid out as
    // cut_dev.
    struct entropy_host { float typical_p = 1.f, epsilon = 0.f, eta = 0.f; bool on() const { return typical_p < 1.f || epsilon > 0.f || eta > 0.f; } };
    std::vector<entropy_host> ent_host;
    int n_entropy = 0;
    float *ent_dev = nullptr, *ceil_dev = nullptr;
    // Sampling requests (ze_seq_set_sampling): samp_host is the truth (penalty = 0: the slot has none), samp_dev the per-slot
    // table the per-chain sampling kernels read, allocated by the first request and written in stream order by the setter;
    // n_sampling = slots with a request, n_sampled = those of them that draw (temperature > 0).  While n_sampling is 0 every
    // step launches the scalar kernels, under the graph keys it always had.
    std::vector<ze_chain_sampling> samp_host;
    int n_sampling = 0, n_sampled = 0;
    ze_chain_sampling* samp_dev = nullptr;
    // Log-probabilities of generated tokens (ze_seq_set_logprobs): lp_host is the truth (-1 off, 0 chosen token only, 1..20
    // alternatives), lp_dev the per-slot table the kernel reads, written in stream order by the setter; n_logprobs = slots with
    // a request.  While it is 0 no step launches the kernel.  History, allocated by the first request that needs it: lp_tok f32
    // [max_seqs, max_ctx]; lp_top_ids int32 / lp_top_lps f32 [max_seqs, max_ctx, 20].
    std::vector<int> lp_host;
    int n_logprobs = 0;
    int* lp_dev = nullptr;
    float* lp_tok = nullptr;
    int* lp_top_ids = nullptr;
    float* lp_top_lps = nullptr;
    // what a captured step must have been captured with: 0 = no kernel, 1 = chosen-token history only, 2 = alternatives too
    int lp_mode() const { return n_logprobs > 0 ? (lp_top_ids ? 2 : 1) : 0; }
    ze_logprob_bufs lp_bufs() const { return ze_logprob_bufs{lp_dev, lp_tok, lp_top_ids, lp_top_lps}; }
    // Logit adjustments (ze_seq_set_logit_adjust): la_host is the truth, la_dev the per-slot table the kernels read (ZE_LA_WORDS
    // ints per slot, all zero = off), written in stream order by the setter; n_adjust = slots with a request.  While it is 0 no
    // step launches anything for them.  Allocated by the first request: la_bias_ids / la_bias_vals [max_seqs, ZE_MAX_LOGIT_BIAS]
    // and la_rows f32 [max_seqs + 1, vocab], the adjusted rows the sampler reads (row b of a batched step; the last row serves
    // the single-chain launches, which share one workspace as it is); by the first request with a penalty: la_counts u16
    // [max_seqs, vocab].
    struct adjust_host {
        float presence = 0.f, frequency = 0.f;
        int min_new = 0, n_bias = 0;
        bool penalties() const { return presence != 0.f || frequency != 0.f; }
        bool on() const { return penalties() || min_new > 0 || n_bias > 0; }
    };
    std::vector<adjust_host> la_host;
    int n_adjust = 0;
    int* la_dev = nullptr;
    int* la_bias_ids = nullptr;
    float* la_bias_vals = nullptr;
    float* la_rows = nullptr;
    uint16_t* la_counts = nullptr;
    // what a captured step must have been captured with: 0 = nothing, 1 = the adjust kernel, 2 = the count kernel too
    int la_mode() const { return n_adjust > 0 ? (la_counts ? 2 : 1) : 0; }
    // (of a single-chain step, which serves one chain: nothing while THAT chain has no request -- it then reads its raw row)
    int la_mode(int seq) const { return la_host[seq].on() ? la_mode() : 0; }
    ze_logit_adjust_bufs la_bufs() const { return ze_logit_adjust_bufs{la_dev, la_bias_ids, la_bias_vals, la_counts}; }
    // Token rules (ze_seq_set_token_rules): tr_host is the truth, tr_dev the per-slot table the kernels read (ZE_TR_WORDS ints per
    // slot, all zero = off), written in stream order by the setter; n_bans / n_stops = slots with n-gram or ban records / with
    // stop records.  While both are 0 no step launches anything for them.  Allocated by the first request: tr_stop / tr_ban
    // [max_seqs, ZE_MAX_RULE_INTS] (and, with bans, the adjusted rows la_rows); by the first request with a context: tr_ctx
    // [max_seqs, max_ctx].
    struct rules_host {
        int ngram = 0, n_stop_ints = 0, n_stop_words = 0, n_ban_ints = 0, n_ban_words = 0, n_context = 0;
        bool bans() const { return ngram > 0 || n_ban_words > 0; }
        bool stops() const { return n_stop_words > 0; }
        bool on() const { return bans() || stops(); }
    };
    std::vector<rules_host> tr_host;
    int n_bans = 0, n_stops = 0;
    int *tr_dev = nullptr, *tr_stop = nullptr, *tr_ban = nullptr, *tr_ctx = nullptr;
    // what a captured step must have been captured with: bit 0 = adjusted copy + ban pass, bit 1 = stop pass, bit 2 = the
    // context history exists (a kernel argument)
    int tr_mode() const { return n_bans + n_stops > 0 ? (n_bans > 0) | (n_stops > 0) << 1 | (tr_ctx != nullptr) << 2 : 0; }
    // (of a single-chain step: by THAT chain's request)
    int tr_mode(int seq) const { return tr_host[seq].on() ? (int)tr_host[seq].bans() | (int)tr_host[seq].stops() << 1 | (tr_ctx != nullptr) << 2 : 0; }
    ze_token_rule_bufs tr_bufs() const { return ze_token_rule_bufs{tr_dev, tr_stop, tr_ban, tr_ctx}; }
    // Guided decoding (ze_grammar_create / ze_seq_set_grammar): gr_tab holds the engine's grammars -- `block` one allocation with the
    // allow bits and the three tables of a grammar, null = a free id, users = slots set to it (ze_grammar_destroy refuses while > 0);
    // gr_host is the truth per slot (the grammar id, -1 = none), gr_dev the per-slot table the kernels read (ZE_GR_WORDS ints per
    // slot, all zero = off; the state lives there alone, moved by the advance pass), gr_desc the grammars as the kernels see them;
    // n_grammar = slots with a grammar.  While it is 0 no step launches anything for them.  gr_dev and gr_desc (and the adjusted
    // rows la_rows) come with the first grammar.
    struct grammar_host {
        void* block = nullptr;
        int n_states = 0, n_classes = 0, users = 0;
    };
    grammar_host gr_tab[ZE_MAX_GRAMMARS];
    std::vector<int> gr_host;
    int n_grammar = 0;
    int* gr_dev = nullptr;
    ze_grammar_dev* gr_desc = nullptr;
    // what a captured step must have been captured with: 1 = the mask pass (on the adjusted copy) and the advance pass
    int gr_mode() const { return n_grammar > 0; }
    // (of a single-chain step: by THAT chain's request)
    int gr_mode(int seq) const { return gr_host[seq] >= 0; }
    ze_grammar_bufs gr_bufs() const { return ze_grammar_bufs{gr_dev, gr_desc}; }
};

// Prefix cache (ze_prefix.hip): a pool of K/V blocks independent of the chain slots.  data: [n_blocks][layers][kv_heads][K|V]
// [block_rows][head_dim] bf16.  Per block, host truth: the generation it was saved under (0 = never; ze_engine::prefix_generation),
// the number of the save that wrote it and of the last load that reads it.  saves / loads: the events behind the last ZE_PREFIX_RING
// calls of each kind (call number -> entry number % ring), what the stream order of ze_prefix_save / ze_prefix_load is built from;
// ids_save / ids_load: the device lists their kernels read (ids_load: a call's block ids, then its destination slots; ids_cap + max_seqs ints).
enum { ZE_PREFIX_RING = 64 };
struct ze_prefix_pool {
    int n_blocks = 0, block_rows = 0, ids_cap = 0;
    size_t block_elems = 0;
    bf16_t* data = nullptr;
    int *ids_save = nullptr, *ids_load = nullptr;
    struct call { hipEvent_t ev = nullptr; uint64_t seq = 0; };
    std::vector<call> saves, loads;
    uint64_t n_saves = 0, n_loads = 0;
    std::vector<unsigned> saved_gen;
    std::vector<uint64_t> saved_seq, read_seq;
};

// LoRA adapters (ze_lora.hip).  An adapter is a set of (A fp32 [r, cols], B fp32 [rows, r], scale) per base tensor, resident on the
// device; the active one is merged into the arena.  store: the bf16 row-major snapshot of every tensor a resident adapter names,
// taken from the arena while it held the base bits -- what every merge and restore reads; dropped by any base-weight write.
struct ze_lora_tensor {
    float *A = nullptr, *B = nullptr;
    int r = 0;
    float scale = 0.f;
};
struct ze_lora_adapter {
    bool used = false;
    std::map<std::string, ze_lora_tensor> t;  // by canonical tensor name
};
struct ze_lora {
    ze_lora_adapter ad[ZE_MAX_ADAPTERS];
    int active = -1;
    std::map<std::string, bf16_t*> store;
    size_t store_bytes = 0;
};

// Speculative decoding by prompt lookup (ze_spec.hip; the steps themselves: ze_decode_batch.hip).  host: the truth per slot (k = 0: off);
// table: the per-slot device words the drafter and the accept pass read (ZE_SP_WORDS ints: k, min_ngram, max_ngram, prompt ids, then
// the counters steps / drafted / accepted), written in stream order by the setter; n_spec = slots with a request.  While it is 0 no
// burst launches anything for it.  The prompt ids live in the context history of the token rules (ze_requests::tr_ctx: the two
// requests exclude each other per chain).  Everything below comes with the first request: the row table of a speculative step --
// row_seq / row_off / row_tok [64]: the chain slot of a row, its offset behind the chain's context (< 0: a dead row) and the id it
// is fed -- the burst's chains (ZE_SP_CHAIN_WORDS ints each: slot, first row, rows, penalty bits), their draft lengths, and the
// step's own logits rows, attention partials and tickets (a step may have more rows than the engine has slots).
// Sampled mode (ze_seq_set_speculation_mode, mode 1; chain_host::mode): the chain's rows are drawn by the per-chain sampling kernels
// of the plain step with row = slot, on per-row shadows the prepare pass lays down (ze_spec_draw below).  The shadows come with the
// first request of that mode, all or none: the scratch seen-sets are ZE_SP_MAX_ROWS x vocab bytes.
enum { ZE_SP_WORDS = 8, ZE_SP_CHAIN_WORDS = 4, ZE_SP_MAX_ROWS = 64, ZE_SP_MAX_K = 8 };
// the shadows of n rows: entry r of every table belongs to row r (ids[r] = r): the request, the chain state (stream, draw index),
// the filter, the seen-set as of that row ([n, vocab]), then the draw's workspaces (cuts n, part 2 * 128 * n, sums 128 * n) and tokens
struct ze_spec_draw {
    ze_chain_sampling* samp = nullptr;
    ze_seq_dev* st = nullptr;
    float* filt = nullptr;
    int* ids = nullptr;
    uint8_t* seen = nullptr;
    float *cuts = nullptr, *part = nullptr, *sums = nullptr;
    int32_t* tok = nullptr;
};
struct ze_spec {
    struct chain_host { int k = 0, min_ngram = 0, max_ngram = 0, n_prompt = 0, mode = 0; };
    std::vector<chain_host> host;
    std::vector<char> pending;   // the chain took part in a ze_decode_burst_begin whose _end has not read its length back yet
    int n_spec = 0;
    int* table = nullptr;
    int *row_seq = nullptr, *row_off = nullptr, *row_tok = nullptr, *chains = nullptr, *dlen = nullptr;
    float *logits = nullptr, *partial = nullptr;
    unsigned* tickets = nullptr;
    ze_spec_draw draw;           // sampled mode only (null until its first request)
    bool on(int seq) const { return !host.empty() && host[seq].k > 0; }
    bool sampled(int seq) const { return on(seq) && host[seq].mode == 1; }
};

// Beam search (ze_beam.hip): everything a beam call keeps between two forwards, device-resident, allocated by the first call (all or
// none) and grown when a call asks for more generated tokens per hypothesis than `cap`.  Rows are indexed g * B + j (group g, slot
// position j); tables marked "by slot" by the chain slot.  seqs: the call's slots; glist: the groups still stepping; gstate:
// ZE_BM_GWORDS ints per group (steps done, done word, heuristic bit, prompt rows, token budget, float bits of budget ** length_penalty);
// run_score / brank: running score and HF beam index of the hypothesis in a row; cand_*: k_beam_rows' table, B + n_eos per row;
// parent (by slot): the slot whose hypothesis moves here; seen_prev (by slot): the seen byte select overwrote; bidx (by slot) [cap]:
// the running beam indices; fin_*: the finished pool of a group (B entries, fin_order = rank -> entry); divs[n] = n ** length_penalty.
enum { ZE_BM_GWORDS = 8, ZE_BM_MAX_BEAMS = 16 };
struct ze_beam {
    int cap = 0, rows = 0;      // generated tokens a hypothesis row holds; rows (= max_seqs)
    int B = 0, groups = 0, max_new = 0;   // of the last call (ze_op_beam_finished reads with them)
    int *seqs = nullptr, *glist = nullptr, *gstate = nullptr, *brank = nullptr, *cand_tok = nullptr, *parent = nullptr, *seen_prev = nullptr;
    int *bidx = nullptr, *fin_len = nullptr, *fin_is = nullptr, *fin_order = nullptr, *fin_tok = nullptr, *fin_bidx = nullptr;
    float *run_score = nullptr, *cand_score = nullptr, *fin_score = nullptr, *divs = nullptr;
    int *u_seqs = nullptr, *u_parent = nullptr;   // ze_op_kv_reorder's own slot and parent tables (a beam call in progress keeps its own)
};

struct ze_engine {
    ze_config cfg{};
    int device = 0;
    std::string err;
    int head_dim = 128, vit_head_dim = 80, vit_ipad = 0, text_ipad = 0, max_pos = 0;

    // weights
    bf16_t* arena = nullptr;
    size_t arena_elems = 0, arena_used = 0;
    std::map<std::string, ze_dest> dests;
    std::set<std::string> loaded;
    void* staging = nullptr;
    size_t staging_bytes = 0;
    ze_lora* lora = nullptr;  // adapters and the base store (null until the first ze_lora_create)
    ze_linear patch_embed, merger0, merger2;
    bf16_t* ln_q = nullptr;
    std::vector<ze_vit_block> vb;
    bf16_t *embed = nullptr, *lm_head = nullptr, *final_norm = nullptr;
    ze_linear lm_head8;          // fp8 copy of an untied lm_head (w / ld unused)
    uint8_t* arena8 = nullptr;    // fp8 decode weights (0 until ze_weights_quantize_fp8)
    bool fp8_ready = false;
    uint8_t* arena4 = nullptr;    // MXFP4 decode weights: codes, then the block scales (0 until ze_weights_quantize_mxfp4)
    bool mx4_ready = false;       // never together with fp8_ready
    bool fp8_act = false;         // ze_set_fp8_activations: qkv / gate-up inputs quantised to E4M3 per row (needs fp8_ready)
    uint8_t* ty8p = nullptr;      // prefill with FP8 activations: the normalised rows as E4M3 bytes, row-major [rows, hidden]
    float* ty8p_scale = nullptr;  // ... and their scales (block-scaled MFMA GEMM, ze_gemm.hip: k_gemm_ring_mx)
    float* damax = nullptr;       // single-chain decode: arg-max partials of the lm_head GEMV's workgroups (count, pairs)
    uint8_t* ty8 = nullptr;       // batched decode: the normalised rows as FP8 fragments (64 rows x hidden bytes)
    float* ty8_scale = nullptr;   // ... and their per-row scales (64)
    // second, fragment-major copy of the wide decode projections (qkv, gate/up, lm_head) for batched decode: built on
    // the first batched step, rebuilt after any weight change (the 288 GB of HBM make the extra 4.2 GB free)
    bf16_t* arena_f = nullptr;
    uint8_t* arena_f8 = nullptr;  // FP8 fragment copies (fp8_ready only)
    uint8_t* arena_f4 = nullptr;  // MXFP4 fragment copies: codes, then scales, per tensor (mx4_ready, ze_tune knob 24 = 0)
    size_t arena_f_bytes = 0, arena_f8_bytes = 0, arena_f4_bytes = 0;  // what the three hold (ze_fragment_bytes)
    bool frag_w4 = false;         // the copies were built for the 4-bit stream (a change of knob 24 rebuilds them)
    bf16_t* lm_head_f = nullptr;
    bool frag_ready = false;
    bf16_t* arena_p = nullptr;        // permuted qkv rows + biases of every layer (row-streaming regime, head_dim 128)
    ze_qkv_epi* qkv_epi_dev = nullptr;  // [layers] epilogue arguments of the fused qkv launch
    // Kernel family of the batched decode step (ze_set_decode_regime): 0 = fragment kernels (at most 64 chains per step),
    // 1 = row-streaming kernels (any count), -1 = by the engine's capacity (max_seqs > 64 -> 1).  Never a function of how
    // many chains are live: a chain's tokens do not depend on the batch it happens to share.
    int decode_regime = -1;
    bool wide_regime() const { return decode_regime == 1 || (decode_regime < 0 && cfg.max_seqs > 64); }
    std::vector<ze_text_layer> tl;

    // tables
    bf16_t *cosT = nullptr, *sinT = nullptr;
    int* axis_of = nullptr;
    float* lut = nullptr;
    int* eos_dev = nullptr;

    // KV cache + chain state
    bf16_t *kcache = nullptr, *vcache = nullptr;
    ze_seq_dev* st_dev = nullptr;
    uint8_t* seen = nullptr;
    int32_t* out_tokens = nullptr;
    std::vector<int> ctx_host, delta_host;
    std::vector<int> split_host;   // round 6: the chains' split rows (ze_seq_dev::split), host truth
    // ze_seq_fork: the chain's row of dlogits holds the logits of its LAST cached row and nothing has drawn from it -- set where a
    // prefill / scoring pass (or a fork) leaves the chain, cleared by whatever draws for it, steps it or changes its rows; and the
    // token those passes pushed into the chain state (the prompt's last id)
    std::vector<char> logits_fresh;
    std::vector<int> tok_host;
    int* bmate = nullptr;          // [max_seqs] per row of the batched step: the row it shares its prefix parts with, or -1 (upload_mates)
    int live_parts_long = 0;       // 384-key parts of the batch's longest chain under its split (the pipelined attention's grid extent)
    // Shared-prefix hints, (source chain << 16) | P per chain slot.  pfx_host is the truth, kept by whatever call changes it
    // (ze_seq_copy_prefix on the admission stream, ze_seq_retire, ...); the device copy pfx_dev -- what the decode attention
    // reads -- is written by ONE stream only: the stream of the batched decode step, which pushes the words that differ from
    // pfx_pushed for ITS chains before it enqueues the step (sync_prefix, ze_seq.hip; called from ze_decode_batch.hip).  A chain state pushed from another
    // stream can therefore never bring a stale hint back.  pfx_copy_ev[seq]: recorded behind the chain's last
    // ze_seq_copy_prefix (null = none): only a chain whose copy has COMPLETED may become the holder other chains read from.
    std::vector<int> pfx_host, pfx_pushed;
    int* pfx_dev = nullptr;
    std::vector<hipEvent_t> pfx_copy_ev;
    bool prefix_hints = true;      // the hint fits its 16 + 16 bits (ze_tune knob 17 = 1: every chain reads its own rows)
    ze_requests req;  // per-chain requests (above)
    ze_spec spec;     // speculative decoding (above)
    ze_beam* beam = nullptr;  // beam search (above; null until the first beam call)
    // prefix cache: the pool (null = none) and the generation of the weights -- bumped by whatever changes what a K/V row of given
    // tokens would be (ze_prefix_weights_changed), so that a block saved under another generation is never loaded
    ze_prefix_pool* prefix_pool = nullptr;
    unsigned prefix_generation = 1;
    // captured single-chain decode step per slot, and the key it was captured under (ze_step_key_of)
    std::vector<hipGraphExec_t> graphs;
    std::vector<ze_step_key> graph_key;

    // front-end workspace
    uint8_t *fe_tmp = nullptr, *fe_img = nullptr;
    int *fe_coef = nullptr;  // device coefficient tables
    size_t fe_tmp_bytes = 0, fe_img_bytes = 0, fe_coef_ints = 0;
    int* fe_coef_host = nullptr;  // pinned
    hipEvent_t v_staged = nullptr, t_staged = nullptr;  // behind the last H2D copy out of v_host_* / t_host_ints (stage_acquire)
    hipEvent_t fe_done = nullptr;  // recorded behind the last kernel that reads the front-end workspace (any stream)
    bool fe_in_flight = false;
    // TIFF tile decode (ze_tiff.hip): the compressed bytes + chunk table of ze_tile_upload_tiff on the device, and the padded tiles of a
    // tiled file before they are placed.  Both are sized by the request and grown on demand; tiff_done is recorded behind the last kernel
    // that reads either, and the next call's copy waits for it on its own stream
    uint8_t *tiff_in = nullptr, *tiff_tiles = nullptr;
    size_t tiff_in_cap = 0, tiff_tiles_cap = 0;
    hipEvent_t tiff_done = nullptr;

    // ViT workspace
    bf16_t *vx = nullptr, *vh = nullptr, *vy = nullptr, *vqkv = nullptr, *vo = nullptr, *va = nullptr, *vz = nullptr,
           *vz2 = nullptr;
    float *vcos = nullptr, *vsin = nullptr;
    int *vperm = nullptr, *vinv = nullptr;
    int4* vtiles_win = nullptr;
    int4* vtiles_full = nullptr;
    int* v_host_ints = nullptr;   // pinned staging for perm / tiles
    float* v_host_f32 = nullptr;  // pinned staging for cos/sin
    size_t v_host_ints_cap = 0, v_host_f32_cap = 0;

    // prefill workspace
    bf16_t *th = nullptr, *ty = nullptr, *tqkv = nullptr, *to = nullptr, *ta = nullptr;
    int *tsrc = nullptr, *tpos = nullptr;
    int4* ttiles = nullptr;
    int* ttile_aux = nullptr;  // batched prefill: (chain slot, position offset) per attention tile
    int* trow_aux = nullptr;   // batched prefill: (chain slot, cache position) per row
    int* tscore = nullptr;     // scoring pass (ze_score_batch): [n] scored rows of the pass's hidden state, then their [n] target ids
    int prefill_rows = 0;
    int* t_host_ints = nullptr;  // pinned
    size_t t_host_ints_cap = 0;
    // batched host <-> device id transfers of the scheduler (ze_seq_mark_seen_batch: host -> device on the admission stream;
    // ze_chain_tokens_batch: device -> host on the decode stream): one pinned + one device buffer per direction, max_seqs x
    // max_ctx ints, allocated at first use
    int *xs_host = nullptr, *xs_dev = nullptr, *xt_host = nullptr, *xt_dev = nullptr;
    size_t xs_cap = 0, xt_cap = 0;
    int *xl_host = nullptr, *xl_dev = nullptr;  // gather scratch of ze_chain_logprobs* (pinned + device, grown on demand)
    size_t xl_cap = 0;
    hipEvent_t xs_staged = nullptr;

    // decode workspace
    bf16_t *dh = nullptr, *dq = nullptr, *dattn = nullptr, *dact = nullptr;
    float *dlogits = nullptr, *dpartial = nullptr, *dsample = nullptr;
    int max_splits = 64;
    int* d_host_ints = nullptr;  // pinned, small
    unsigned* atickets = nullptr;  // decode attention: one arrival ticket per (chain, kv head)
    unsigned bgraph_epoch = 0;  // ze_tune epoch the batched graphs were captured under (a change flushes them)
    // split-K GEMM workspace
    float* gslab = nullptr;       // split-K slabs of the weight-streaming GEMMs (ze_gemm_ws)
    size_t gslab_floats = 0;
    int gticket_cap = 0;
    ze_gemm_ws gemm_ws() const { return ze_gemm_ws{gslab, gslab_floats, gtickets, gticket_cap}; }
    unsigned* gtickets = nullptr;
    // split-K workspace of the PREFILL family (round 6: the down projection of a pass in three K slices, ze_gemm.hip ze_prefill_ksplit):
    // slabs and tickets of its own -- a prefill pass on the admission stream runs beside the decode step, which owns the ones above
    float* pslab = nullptr;
    size_t pslab_floats = 0;
    unsigned* ptickets = nullptr;
    int pticket_cap = 0;
    // (allocated on first use with the split switched on -- ze_tune knob 20 = 3: the form is not shipped, DESIGN 7i c, and 0.7 GB of
    //  slabs per engine are not reserved for it)
    ze_gemm_ws prefill_ws();
    // batched decode: activations of its own (rows = chains), so that a decode burst on one HIP stream and a prefill / ViT
    // round on another never share a buffer (the scheduler overlaps them: zoomearth_amd/scheduler.py)
    bf16_t *bh = nullptr, *by = nullptr, *bqkv = nullptr, *bo = nullptr, *ba = nullptr;
    int* bseq = nullptr;
    float *blogits = nullptr, *bpartial = nullptr, *bsample = nullptr;
    ze_seq_dev* bstate_host = nullptr;  // pinned
    std::map<ze_step_key, hipGraphExec_t> bgraphs;  // captured batched decode steps
    int live_parts = 0;  // 192-key parts the longest chain of the current batch needs (the attention grid's extent); 0 = all

    // timers
    bool timers_on = false;
    bool counted = false;  // in ze_live_engines (a create that failed half-way is destroyed uncounted)
    struct ev_pair { int phase; hipEvent_t a, b; };
    std::vector<ev_pair> ev_used;
    std::vector<ev_pair> ev_free;
    float phase_ms[5] = {0, 0, 0, 0, 0};

    bf16_t* kc(int layer, int seq) const {
        return kcache + (((size_t)layer * cfg.max_seqs + seq) * cfg.kv_heads) * (size_t)cfg.max_ctx * head_dim;
    }
    bf16_t* vc(int layer, int seq) const {
        return vcache + (((size_t)layer * cfg.max_seqs + seq) * cfg.kv_heads) * (size_t)cfg.max_ctx * head_dim;
    }
};

#define ZE_TRY(x)               \
    do {                        \
        int _r = (x);           \
        if (_r != 0) return _r; \
    } while (0)
#define ZE_KCHECK() ZE_HIP(hipGetLastError())

// engine internals used across translation units
extern unsigned ze_tune_epoch;
void ze_weights_changed(ze_engine* e);
int ze_engine_build_layout(ze_engine* e);
int ze_timer_begin(ze_engine* e, int phase, hipStream_t s);
void ze_timer_end(ze_engine* e, int handle, hipStream_t s);

template <typename T>
static int dev_alloc(ze_engine* e, T** p, size_t count, bool zero = true) {
    ZE_HIP(hipMalloc((void**)p, std::max<size_t>(count, 1) * sizeof(T)));
    if (zero) ZE_HIP(hipMemset(*p, 0, std::max<size_t>(count, 1) * sizeof(T)));
    return 0;
}
static inline int check_seq(ze_engine* e, int seq) {
    if (!e) return ze_fail(e, ZE_ERR_INVALID, "null engine");
    if (seq < 0 || seq >= e->cfg.max_seqs) return ze_fail(e, ZE_ERR_NOTFOUND, "sequence id out of range");
    return ZE_OK;
}

// ---- per-chain requests (ze_requests.hip), kept out of the library's dynamic symbols
#pragma GCC visibility push(hidden)
int ze_requests_create(ze_engine* e);  // host tables and the per-slot device tables (ze_engine_create); first error, 0 = none
void ze_requests_free(ze_engine* e);
// the slot goes to another chain (reset, truncate, copy_prefix): it never inherits a request.  Nothing is launched for a slot without one.
void ze_requests_clear(ze_engine* e, int seq, hipStream_t s);
// The rows the sampler of a step reads: the step's own while no chain of it has a request (the step then launches what it always
// did), else their adjusted copy.  seq_ids = null: the one chain `slot0`, whose row `logits` is.
const float* ze_requests_rows(ze_engine* e, const float* logits, const int* seq_ids, int slot0, int n, hipStream_t s);
// after the token of a step was accepted: log-probability entries, then token counts, then stop records, then the grammar's
// state -- each only for chains that asked (ze_requests_logprobs: the first of the three alone)
void ze_requests_logprobs(ze_engine* e, const float* logits, const int* seq_ids, int slot0, int n, hipStream_t s);
void ze_requests_after_token(ze_engine* e, const float* logits, const int* seq_ids, int slot0, int n, hipStream_t s);
int ze_check_filter(ze_engine* e, int top_k, float top_p, float min_p);
int ze_check_entropy_filter(ze_engine* e, float typical_p, float epsilon_cutoff, float eta_cutoff);
// the sampling options of a launch: see ze_requests.hip
void ze_attach_filters(ze_engine* e, ze_sample_opts& so, bool batch);
float ze_penalty_of(const ze_engine* e, const ze_gen_params* p, int seq);
ze_sample_opts ze_sample_opts_of(ze_engine* e, const ze_gen_params* p, int slot, bool batch = false);
// n = 0: the single-chain step of chain `seq`; else the batched step of n rows, of `kind` (a speculative one with its layout)
ze_step_key ze_step_key_of(const ze_engine* e, int n, int seq, float penalty, int ignore_eos, const ze_sample_opts& so,
                           int kind = ZE_STEP_SAMPLED, int n_plain = 0, int n_chains = 0, int n_drawn = 0, int n_drawn_rows = 0);

// ---- speculative decoding (ze_spec.hip)
void ze_spec_free(ze_engine* e);
int ze_spec_alloc(ze_engine* e);   // the buffers of the first request, all or none
void ze_spec_clear(ze_engine* e, int seq, hipStream_t s);   // wherever ze_requests_clear runs
// one chain per workgroup of the burst's list (`chains`: ZE_SP_CHAIN_WORDS ints each): the drafter fills the chain's rows of the row
// table, the accept pass walks them
struct ze_spec_step {
    ze_seq_dev* st;
    const int *table, *chains, *hist_ctx, *eos_ids;
    int32_t* out_tokens;
    uint8_t* seen;
    const float* logits;
    int *row_off, *row_tok, *dlen;
    int n_chains, max_ctx, vocab, n_eos, ignore_eos;
};
void ze_launch_spec_draft(const ze_spec_step& a, hipStream_t s);
void ze_launch_spec_accept(const ze_spec_step& a, int first_chain, hipStream_t s);
// The accept pass of the sampled-mode chains [first_chain, a.n_chains) of the list, whose rows are [first_row, first_row + n_rows) of
// the step: prepare (the rows' shadows) -> the per-chain sampling kernels over the rows -> the walk.  temperature / seed: the call's
// (a chain without a request of its own follows them, its penalty is in its chain words); draws: some row may have a temperature;
// samp / filt: the per-slot tables or null.
void ze_launch_spec_accept_sampled(const ze_spec_step& a, const ze_spec_draw& d, int first_chain, int first_row, int n_rows, float temperature,
                                   unsigned long long seed, bool draws, const ze_chain_sampling* samp, const float* filt, hipStream_t s);
void ze_launch_spec_embed(const int* row_tok, int n, const bf16_t* embed, bf16_t* out, int hidden, hipStream_t s);

// ---- beam search (ze_beam.hip)
void ze_beam_free(ze_engine* e);   // (ze_engine_destroy)
// one teacher-forced batched step of the chains `seqs` (ze_decode_batch.hip): the forward of ze_decode_batch on the tokens their chain
// states hold -- the cache grows by one row per chain, the logits rows stay in e->blogits, nothing is drawn
int ze_beam_forward(ze_engine* e, const int32_t* seqs, int n, int use_graph, hipStream_t s);

// ---- the launch sites of the forward passes (ze_forward.hip, ze_decode_batch.hip) that the profilers (ze_profile.hip) time: a projection's launcher is
// chosen in these functions only, so a profiler cannot launch anything but what the pass launches
enum { ZE_PROJ_QKV = 0, ZE_PROJ_O = 1, ZE_PROJ_GATE_UP = 2, ZE_PROJ_DOWN = 3 };
enum { ZE_NORM_IN = 0, ZE_NORM_POST = 1, ZE_NORM_FINAL = 2 };
// prefill: projection `which` of layer L on `rows` rows into out; norm = false: on the normalised rows the last pass left
void prefill_projection(ze_engine* e, const ze_text_layer& L, int which, int rows, bool norm, bf16_t* out, int ldo, hipStream_t s);
// single-chain decode: the cleared GEMV arguments with the weight (the FP8 copy too on a quantised engine), N, K, x and D set
ze_gemv_args gemv_args_of(const ze_engine* e, const ze_linear& lin, int N, int K, const bf16_t* x);
ze_linear lm_head_linear(const ze_engine* e, bool decode);
// The rows of one batched decode step (ze_decode_batch.hip): what its launches read or write per row that differs between the
// kinds of step.  A launch takes its rows from this struct and from nowhere else; no engine member changes while a step is enqueued.
struct ze_step_rows {
    const int* seq;      // row -> chain slot
    const int* off;      // row -> its offset behind the chain's context; null = one row per chain, at the chain's own ctx
    const int* mate;     // row -> the row it shares its prefix parts with (upload_mates); null = no pairing
    const bf16_t* q;     // the qkv rows the attention reads ...
    bf16_t* out;         // ... and the rows it writes
    float* logits;       // [rows, vocab]
    float* partial;      // attention partials
    unsigned* tickets;   // arrival tickets of the attention's merge
};
ze_step_rows ze_rows_own(const ze_engine* e);   // the engine's own step buffers: the plain step, beam, ze_decode_batch, the profiler
ze_step_rows ze_rows_spec(const ze_engine* e);  // the speculative row table (ze_spec): spec_burst, ze_op_decode_rows
ze_step_rows ze_rows_caller(const ze_engine* e, const bf16_t* q, bf16_t* out);   // the engine's chains, the caller's q / out rows: ze_op_attn_decode
// batched decode: one launch kind each for the n rows of `rows`; a projection returns whether it streamed FP8 weights
void batch_norm(ze_engine* e, const ze_step_rows& rows, int li, int n, int which, hipStream_t s);
bool batch_qkv(ze_engine* e, const ze_step_rows& rows, int li, int n, hipStream_t s);  // with the rope / KV-append launch where that is not fused
void batch_attention(ze_engine* e, const ze_step_rows& rows, int li, int n, hipStream_t s);
bool batch_o(ze_engine* e, const ze_step_rows& rows, int li, int n, hipStream_t s);
bool batch_gate_up(ze_engine* e, const ze_step_rows& rows, int li, int n, hipStream_t s);
bool batch_down(ze_engine* e, const ze_step_rows& rows, int li, int n, hipStream_t s);
bool batch_lm_head(ze_engine* e, const ze_step_rows& rows, int li, int n, hipStream_t s);
// the decode attention of a step alone (frag_out: its output in the fragment layout the o projection of family 0 reads)
void launch_batch_attention(ze_engine* e, const ze_step_rows& rows, int li, int n, bool frag_out, hipStream_t s);
// the scored-row path of a scoring pass (ze_score.hip): final norm of the n hidden rows e->tscore lists, lm_head in chunks of the
// MLP workspace, log-softmax pick of their targets into out (device f32 [n]); n = 0 launches nothing
void ze_launch_rmsnorm_gather(const bf16_t* x, int ldx, const int* src_rows, const bf16_t* w, bf16_t* y, int ldy, int rows, int cols,
                              float eps, hipStream_t s);
int ze_score_chunk_rows(const ze_engine* e, int rows);
// what a scoring pass writes per scored row beside the log-probability (ze_score_batch_detail); null members are not asked for,
// a null struct or all members null: k_token_logprob runs, as in ze_score_batch
struct ze_score_detail_out {
    int top_n = 0;
    float* entropy = nullptr;
    int* rank = nullptr;
    int* top_ids = nullptr;  // [n, top_n]
    float* top_lps = nullptr;
    bool any() const { return entropy || rank || top_ids; }
};
int ze_score_rows(ze_engine* e, int n, float* out, const ze_score_detail_out* detail, hipStream_t s);
// what a batched step sets up before its launches
int ensure_fragments(ze_engine* e, hipStream_t s);
void sync_prefix(ze_engine* e, const int32_t* seqs, int n, hipStream_t s);
void set_live_parts(ze_engine* e, const int32_t* seqs, int n, int steps);
// ... all of it for `steps` steps of the (valid) chains `seqs`: e->bseq, the prefix hints, the mates, the attention grids' extents
void stage_batch(ze_engine* e, const int32_t* seqs, int n, int steps, hipStream_t s);
// the attention tile list of n_seg segments (ze_vision.hip; ze_op_attention): the tile count, -1 when cap_tiles do not hold it
int build_tiles(const int32_t* cu, int n_seg, int* out /* int4 rows */, int cap_tiles, int bq = 64);
int stage_acquire(ze_engine* e, hipEvent_t& ev);   // wait for / record the event behind the last reader of a staging buffer (ze_forward.hip)
int stage_release(ze_engine* e, hipEvent_t& ev, hipStream_t s);
// the decode attention of the single-chain step (ze_forward.hip) on its own q / out rows, or the caller's: ze_op_attn_decode_single
void launch_step_attention(ze_engine* e, int li, int seq, hipStream_t s, const bf16_t* q_row = nullptr, bf16_t* out_row = nullptr);
// helpers of ze_forward.hip that the batched paths (ze_decode_batch.hip) share with the single-chain ones
int capture_step(ze_engine* e, const std::function<int(hipStream_t)>& enqueue, hipGraphExec_t* exec);
int first_token(ze_engine* e, int q, float pen, int ign, const ze_sample_opts& so, hipStream_t s);
int trim_at_eos(const ze_config& c, const int32_t* tokens, int n);
int xfer_reserve(ze_engine* e, int*& host, int*& dev, size_t& cap, size_t need, hipEvent_t staged, hipStream_t s);   // (ze_seq.hip)
// chain bookkeeping (ze_seq.hip) shared with ze_prefix.hip: the readers of rows >= keep of chain `seq` move to another holder; the chain state
// of `seq` goes to the device in stream order
void prefix_source_gone(ze_engine* e, int seq, int keep);
int push_state(ze_engine* e, int seq, hipStream_t s, int token, int n_gen, int finished);
// ---- prefix cache (ze_prefix.hip)
void ze_prefix_pool_free(ze_engine* e);   // (ze_engine_destroy: the device is idle)
// the K/V rows of given tokens are no longer what they were: every pool block counts as unsaved from now on
inline void ze_prefix_weights_changed(ze_engine* e) { ++e->prefix_generation; }
// an HF checkpoint key of either layout as the key of ze_engine::dests (ze_engine.hip)
std::string ze_canonical_name(const char* name);
// ---- LoRA adapters (ze_lora.hip)
void ze_lora_free(ze_engine* e);          // (ze_engine_destroy)
// the arena was written from outside the adapters (load, synthetic fill, invalidate, broadcast): its contents are the base now --
// no adapter is active and the base store is dropped; resident adapters stay
void ze_lora_base_written(ze_engine* e);
#pragma GCC visibility pop

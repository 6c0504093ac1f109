// Per-chain requests of the engine (ze_requests in ze_engine.h): the setters of the C ABI, what a decode step launches for the
// chains that asked, the sampling options of a launch, and the key of a captured step.  Host code only: the kernels live in
// ze_sample*.hip, ze_logprobs.hip, ze_logit_adjust.hip, ze_token_rules.hip and ze_grammar.hip.
#include <cmath>

#include <initializer_list>

#include "ze_engine.h"

// Buffers a request kind needs from its first use on, all of a group or none: on failure whatever this call allocated is freed,
// the HIP error is cleared and the engine is as it was.
struct lazy_buf {
    void** p;
    size_t bytes;
};
template <typename T>
static lazy_buf buf_of(T*& p, size_t count) {
    return lazy_buf{(void**)&p, count * sizeof(T)};
}
static int alloc_first_use(ze_engine* e, std::initializer_list<lazy_buf> bufs, const char* msg) {
    void* got[4] = {nullptr, nullptr, nullptr, nullptr};
    int k = 0;
    for (const lazy_buf& b : bufs) {
        if (hipMalloc(&got[k], b.bytes) != hipSuccess) {
            (void)hipGetLastError();
            while (k > 0) hipFree(got[--k]);
            return ze_fail(e, ZE_ERR_NOMEM, msg);
        }
        ++k;
    }
    k = 0;
    for (const lazy_buf& b : bufs) *b.p = got[k++];
    return ZE_OK;
}

int ze_requests_create(ze_engine* e) {
    const ze_config& c = e->cfg;
    ze_requests& q = e->req;
    int r = 0;
    auto chk = [&](int rr) {
        if (rr != 0 && r == 0) r = rr;
    };
    q.filt_host.assign(c.max_seqs, ze_requests::filter_host{});
    chk(dev_alloc(e, &q.filt_dev, (size_t)c.max_seqs * 4));
    chk(dev_alloc(e, &q.cut_dev, (size_t)c.max_seqs * 2));
    q.ent_host.assign(c.max_seqs, ze_requests::entropy_host{});
    chk(dev_alloc(e, &q.ent_dev, (size_t)c.max_seqs * 4));
    chk(dev_alloc(e, &q.ceil_dev, (size_t)c.max_seqs * 2));
    q.samp_host.assign(c.max_seqs, ze_chain_sampling{0.f, 0.f, 0ull});
    q.lp_host.assign(c.max_seqs, -1);
    chk(dev_alloc(e, &q.lp_dev, (size_t)c.max_seqs, false));
    if (q.lp_dev && hipMemset(q.lp_dev, 0xff, (size_t)c.max_seqs * sizeof(int)) != hipSuccess) chk(ZE_ERR_HIP);  // every slot -1 = off
    q.la_host.assign(c.max_seqs, ze_requests::adjust_host{});
    chk(dev_alloc(e, &q.la_dev, (size_t)c.max_seqs * ZE_LA_WORDS));  // all zero = off
    q.tr_host.assign(c.max_seqs, ze_requests::rules_host{});
    chk(dev_alloc(e, &q.tr_dev, (size_t)c.max_seqs * ZE_TR_WORDS));  // all zero = off
    q.gr_host.assign(c.max_seqs, -1);
    return r;
}

void ze_requests_free(ze_engine* e) {
    const ze_requests& q = e->req;
    void* dev[] = {q.filt_dev, q.cut_dev, q.ent_dev, q.ceil_dev, q.samp_dev, q.lp_dev, q.lp_tok, q.lp_top_ids, q.lp_top_lps, q.la_dev, q.la_bias_ids,
                   q.la_bias_vals, q.la_rows, q.la_counts, q.tr_dev, q.tr_stop, q.tr_ban, q.tr_ctx, q.gr_dev, q.gr_desc};
    for (void* p : dev)
        if (p) hipFree(p);
    for (const ze_requests::grammar_host& g : q.gr_tab)
        if (g.block) hipFree(g.block);
}

// ---- sampling filters (top-k / top-p / min-p per chain; ze_sample_filter.hip the kernel)
int ze_check_filter(ze_engine* e, int top_k, float top_p, float min_p) {
    if (top_k < 0) return ze_fail(e, ZE_ERR_INVALID, "top_k must be >= 0 (0 = off)");
    if (!(top_p > 0.f && top_p <= 1.f)) return ze_fail(e, ZE_ERR_INVALID, "top_p must be in (0, 1] (1 = off)");
    if (!(min_p >= 0.f && min_p <= 1.f)) return ze_fail(e, ZE_ERR_INVALID, "min_p must be in [0, 1] (0 = off)");
    return ZE_OK;
}

static void write_filter(ze_engine* e, int seq, int top_k, float top_p, float min_p, hipStream_t s) {
    ze_requests::filter_host& f = e->req.filt_host[seq];
    const bool was = f.on();
    f.top_k = top_k, f.top_p = top_p, f.min_p = min_p;
    e->req.n_filters += (int)f.on() - (int)was;
    // the table keeps all zeros for "off" (a zero top_p is no legal value)
    if (was || f.on()) ze_launch_set_filter(e->req.filt_dev, seq, top_k, f.on() ? top_p : 0.f, min_p, 0.f, s);
}

extern "C" int ze_seq_set_sampling_filter(ze_engine* e, int seq, int top_k, float top_p, float min_p, void* stream) {
    ZE_TRY(check_seq(e, seq));
    ZE_TRY(ze_check_filter(e, top_k, top_p, min_p));
    if ((top_k > 0 || top_p < 1.f || min_p > 0.f) && e->spec.on(seq) && !e->spec.sampled(seq)) return ze_fail(e, ZE_ERR_INVALID, "the chain speculates (ze_seq_set_speculation): greedy only, no sampling filter");
    hipSetDevice(e->device);
    write_filter(e, seq, top_k, top_p, min_p, (hipStream_t)stream);
    ZE_KCHECK();
    return ZE_OK;
}

// ---- entropy filters (typical / epsilon / eta per chain; ze_sample_band.hip the kernel)
int ze_check_entropy_filter(ze_engine* e, float typical_p, float epsilon_cutoff, float eta_cutoff) {
    if (!(typical_p > 0.f && typical_p <= 1.f)) return ze_fail(e, ZE_ERR_INVALID, "typical_p must be in (0, 1] (1 = off)");
    if (!(epsilon_cutoff >= 0.f && epsilon_cutoff < 1.f)) return ze_fail(e, ZE_ERR_INVALID, "epsilon_cutoff must be in [0, 1) (0 = off)");
    if (!(eta_cutoff >= 0.f && eta_cutoff < 1.f)) return ze_fail(e, ZE_ERR_INVALID, "eta_cutoff must be in [0, 1) (0 = off)");
    return ZE_OK;
}

static void write_entropy_filter(ze_engine* e, int seq, float typical_p, float epsilon_cutoff, float eta_cutoff, hipStream_t s) {
    ze_requests::entropy_host& f = e->req.ent_host[seq];
    const bool was = f.on();
    f.typical_p = typical_p, f.epsilon = epsilon_cutoff + 0.f, f.eta = eta_cutoff + 0.f;
    e->req.n_entropy += (int)f.on() - (int)was;
    // the table keeps all zeros for "off" (a zero typical_p is no legal value)
    if (was || f.on()) ze_launch_set_entropy_filter(e->req.ent_dev, seq, f.on() ? typical_p : 0.f, f.epsilon, f.eta, 0.f, s);
}

extern "C" int ze_seq_set_entropy_filter(ze_engine* e, int seq, float typical_p, float epsilon_cutoff, float eta_cutoff, void* stream) {
    ZE_TRY(check_seq(e, seq));
    ZE_TRY(ze_check_entropy_filter(e, typical_p, epsilon_cutoff, eta_cutoff));
    if ((typical_p < 1.f || epsilon_cutoff > 0.f || eta_cutoff > 0.f) && e->spec.on(seq))
        return ze_fail(e, ZE_ERR_INVALID, "the chain speculates (ze_seq_set_speculation): greedy only, no entropy filter");
    hipSetDevice(e->device);
    write_entropy_filter(e, seq, typical_p, epsilon_cutoff, eta_cutoff, (hipStream_t)stream);
    ZE_KCHECK();
    return ZE_OK;
}

// ---- sampling requests (greedy | temperature, seed, repetition penalty per chain; the per-chain kernels of ze_sample.hip read samp_dev)
static void write_sampling(ze_engine* e, int seq, const ze_chain_sampling& v, hipStream_t s) {
    ze_chain_sampling& h = e->req.samp_host[seq];
    const bool was = h.penalty > 0.f, on = v.penalty > 0.f;
    e->req.n_sampling += (int)on - (int)was;
    e->req.n_sampled += (int)(on && v.temperature > 0.f) - (int)(was && h.temperature > 0.f);
    h = v;
    if (was || on) ze_launch_set_sampling(e->req.samp_dev, seq, v, s);
}
static void clear_sampling(ze_engine* e, int seq, hipStream_t s) {
    if (e->req.samp_host[seq].penalty > 0.f) write_sampling(e, seq, ze_chain_sampling{0.f, 0.f, 0ull}, s);
}

extern "C" int ze_seq_set_sampling(ze_engine* e, int seq, int mode, float temperature, uint64_t seed, float repetition_penalty,
                                   void* stream) {
    ZE_TRY(check_seq(e, seq));
    if (mode < -1 || mode > 1) return ze_fail(e, ZE_ERR_INVALID, "mode must be -1 (clear), 0 (greedy) or 1 (temperature sampling)");
    if (mode == 1 && !(std::isfinite(temperature) && temperature > 0.f))
        return ze_fail(e, ZE_ERR_INVALID, "temperature must be finite and > 0");
    if (mode >= 0 && !(std::isfinite(repetition_penalty) && repetition_penalty > 0.f))
        return ze_fail(e, ZE_ERR_INVALID, "repetition_penalty must be finite and > 0 (1 = off)");
    if (mode == 1 && e->spec.on(seq) && !e->spec.sampled(seq)) return ze_fail(e, ZE_ERR_INVALID, "the chain speculates (ze_seq_set_speculation): greedy only");
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    if (mode >= 0 && !e->req.samp_dev) {
        const size_t entries = (size_t)e->cfg.max_seqs;
        ze_chain_sampling* t = nullptr;
        ZE_TRY(alloc_first_use(e, {buf_of(t, entries)}, "hipMalloc of the sampling-request table failed"));
        // all zero = no request.  Once per engine, and waited for: setters on other streams may write their entries at once
        if (hipMemset(t, 0, entries * sizeof(ze_chain_sampling)) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) {
            (void)hipGetLastError();
            hipFree(t);
            return ze_fail(e, ZE_ERR_HIP, "hipMemset of the sampling-request table failed");
        }
        e->req.samp_dev = t;
    }
    if (mode < 0)
        clear_sampling(e, seq, s);
    else
        write_sampling(e, seq, ze_chain_sampling{mode == 1 ? temperature : 0.f, repetition_penalty, mode == 1 ? (unsigned long long)seed : 0ull}, s);
    ZE_KCHECK();
    return ZE_OK;
}

// ---- log-probabilities of generated tokens (ze_logprobs.hip the kernel)
static void write_logprobs(ze_engine* e, int seq, int top_n, hipStream_t s) {
    const int was = e->req.lp_host[seq];
    if (was == top_n) return;
    e->req.lp_host[seq] = top_n;
    e->req.n_logprobs += (int)(top_n >= 0) - (int)(was >= 0);
    ze_launch_set_logprobs(e->req.lp_dev, seq, top_n, s);
}

extern "C" int ze_seq_set_logprobs(ze_engine* e, int seq, int top_n, void* stream) {
    ZE_TRY(check_seq(e, seq));
    if (top_n < -1 || top_n > ZE_MAX_TOP_LOGPROBS) return ze_fail(e, ZE_ERR_INVALID, "top_n must be in [-1, 20] (-1 = off)");
    if (top_n >= 0 && e->spec.on(seq)) return ze_fail(e, ZE_ERR_INVALID, "the chain speculates (ze_seq_set_speculation): no log-probabilities");
    hipSetDevice(e->device);
    ze_requests& q = e->req;
    const size_t entries = (size_t)e->cfg.max_seqs * e->cfg.max_ctx;
    if (top_n >= 0 && !q.lp_tok) ZE_TRY(alloc_first_use(e, {buf_of(q.lp_tok, entries)}, "hipMalloc of the log-probability history failed"));
    if (top_n >= 1 && !q.lp_top_ids)
        ZE_TRY(alloc_first_use(e, {buf_of(q.lp_top_ids, entries * ZE_MAX_TOP_LOGPROBS), buf_of(q.lp_top_lps, entries * ZE_MAX_TOP_LOGPROBS)},
                               "hipMalloc of the top-logprobs history failed"));
    write_logprobs(e, seq, top_n, (hipStream_t)stream);
    ZE_KCHECK();
    return ZE_OK;
}

// (only while some chain of the engine has a request -- without one the step launches what it always did)
void ze_requests_logprobs(ze_engine* e, const float* logits, const int* seq_ids, int slot0, int n, hipStream_t s) {
    if (e->req.n_logprobs > 0)
        ze_launch_chain_logprobs(logits, e->cfg.vocab, e->cfg.vocab, e->st_dev, seq_ids, slot0, n, e->req.lp_bufs(), e->cfg.max_ctx, s);
}

// ---- logit adjustments (ze_logit_adjust.hip the kernels)
static void write_adjust(ze_engine* e, int seq, const ze_requests::adjust_host& h, const int32_t* ids, const float* vals, hipStream_t s) {
    ze_requests& q = e->req;
    const bool was = q.la_host[seq].on();
    q.la_host[seq] = h;
    q.n_adjust += (int)h.on() - (int)was;
    if (!was && !h.on()) return;
    if (h.n_bias > 0) {  // the list travels as kernel arguments, 128 words a launch
        ze_launch_set_ints(q.la_bias_ids + (size_t)seq * ZE_MAX_LOGIT_BIAS, ids, h.n_bias, s);
        ze_launch_set_ints(reinterpret_cast<int*>(q.la_bias_vals + (size_t)seq * ZE_MAX_LOGIT_BIAS), reinterpret_cast<const int*>(vals),
                           h.n_bias, s);
    }
    // (also the word that remembers a finished chain: every request starts from a live chain with zero counts)
    ze_launch_set_logit_adjust(q.la_dev, seq, h.presence, h.frequency, h.min_new, h.n_bias, s);
}

// the adjusted rows and the bias lists, on first use (a logit-adjust request, or token rules with bans)
static int ensure_adjusted_rows(ze_engine* e) {
    ze_requests& q = e->req;
    if (q.la_rows) return ZE_OK;
    const ze_config& c = e->cfg;
    return alloc_first_use(e, {buf_of(q.la_bias_ids, (size_t)c.max_seqs * ZE_MAX_LOGIT_BIAS), buf_of(q.la_bias_vals, (size_t)c.max_seqs * ZE_MAX_LOGIT_BIAS),
                               buf_of(q.la_rows, ((size_t)c.max_seqs + 1) * c.vocab)},
                           "hipMalloc of the adjusted-row buffer failed");
}

extern "C" int ze_seq_set_logit_adjust(ze_engine* e, int seq, float presence_penalty, float frequency_penalty, int min_new_tokens,
                                       const int32_t* bias_ids, const float* bias_vals, int n_bias, void* stream) {
    ZE_TRY(check_seq(e, seq));
    const ze_config& c = e->cfg;
    if (!std::isfinite(presence_penalty) || !std::isfinite(frequency_penalty))
        return ze_fail(e, ZE_ERR_INVALID, "presence_penalty and frequency_penalty must be finite (0 = off)");
    if (min_new_tokens < 0) return ze_fail(e, ZE_ERR_INVALID, "min_new_tokens must be >= 0 (0 = off)");
    if (n_bias < 0 || n_bias > ZE_MAX_LOGIT_BIAS) return ze_fail(e, ZE_ERR_INVALID, "n_bias must be in [0, 512]");
    if (n_bias > 0 && (!bias_ids || !bias_vals)) return ze_fail(e, ZE_ERR_INVALID, "null bias arrays");
    for (int i = 0; i < n_bias; ++i) {
        if (bias_ids[i] < 0 || bias_ids[i] >= c.vocab) return ze_fail(e, ZE_ERR_INVALID, "bias token id out of range");
        if (std::isnan(bias_vals[i]) || bias_vals[i] == INFINITY)
            return ze_fail(e, ZE_ERR_INVALID, "a bias must be finite or -inf (-inf = the token is banned)");
    }
    if (n_bias > 1) {
        std::vector<int32_t> sorted(bias_ids, bias_ids + n_bias);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return ze_fail(e, ZE_ERR_INVALID, "duplicate bias token id");
    }
    ze_requests::adjust_host h;
    h.presence = presence_penalty + 0.f;  // (-0 -> +0: "no penalty" has one spelling)
    h.frequency = frequency_penalty + 0.f;
    h.min_new = min_new_tokens;
    h.n_bias = n_bias;
    if (h.on() && e->spec.on(seq)) return ze_fail(e, ZE_ERR_INVALID, "the chain speculates (ze_seq_set_speculation): no logit adjust");
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    ze_requests& q = e->req;
    if (h.on()) ZE_TRY(ensure_adjusted_rows(e));
    if (h.penalties() && !q.la_counts)
        ZE_TRY(alloc_first_use(e, {buf_of(q.la_counts, (size_t)c.max_seqs * c.vocab)}, "hipMalloc of the token counts failed"));
    if (h.penalties()) ZE_HIP(hipMemsetAsync(q.la_counts + (size_t)seq * c.vocab, 0, (size_t)c.vocab * sizeof(uint16_t), s));
    write_adjust(e, seq, h, bias_ids, bias_vals, s);
    ZE_KCHECK();
    return ZE_OK;
}

// A chain with bans (token rules) or a grammar counts as adjusted: the ban pass and the grammar's mask pass write -inf into its
// copy behind the adjust kernel, which leaves the row of an all-zero request untouched.
const float* ze_requests_rows(ze_engine* e, const float* logits, const int* seq_ids, int slot0, int n, hipStream_t s) {
    const ze_requests& q = e->req;
    const bool bans = seq_ids ? q.n_bans > 0 : q.tr_host[slot0].bans();
    const bool guided = seq_ids ? q.n_grammar > 0 : q.gr_host[slot0] >= 0;
    if (!bans && !guided && (seq_ids ? q.n_adjust == 0 : !q.la_host[slot0].on())) return logits;
    float* out = seq_ids ? q.la_rows : q.la_rows + (size_t)e->cfg.max_seqs * e->cfg.vocab;
    ze_launch_chain_logit_adjust(logits, e->cfg.vocab, e->st_dev, seq_ids, slot0, n, q.la_bufs(), e->eos_dev, e->cfg.n_eos, out, s);
    if (bans) ze_launch_chain_token_ban(out, e->cfg.vocab, e->st_dev, seq_ids, slot0, n, q.tr_bufs(), e->out_tokens, e->cfg.max_ctx, s);
    if (guided) ze_launch_chain_grammar_mask(out, e->cfg.vocab, e->st_dev, seq_ids, slot0, n, q.gr_bufs(), s);
    return out;
}

// ---- token rules (ze_token_rules.hip the kernels)
static void write_rules(ze_engine* e, int seq, const ze_requests::rules_host& h, const int32_t* stop, const int32_t* ban, hipStream_t s) {
    ze_requests& q = e->req;
    const ze_requests::rules_host was = q.tr_host[seq];
    q.tr_host[seq] = h;
    q.n_bans += (int)h.bans() - (int)was.bans();
    q.n_stops += (int)h.stops() - (int)was.stops();
    if (!was.on() && !h.on()) return;
    // the lists travel as kernel arguments, 128 words a launch
    if (h.n_stop_ints > 0) ze_launch_set_ints(q.tr_stop + (size_t)seq * ZE_MAX_RULE_INTS, stop, h.n_stop_ints, s);
    if (h.n_ban_ints > 0) ze_launch_set_ints(q.tr_ban + (size_t)seq * ZE_MAX_RULE_INTS, ban, h.n_ban_ints, s);
    ze_launch_set_token_rules(q.tr_dev, seq, h.ngram, h.n_stop_ints, h.n_stop_words, h.n_ban_ints, h.n_ban_words, h.n_context, s);
}

// ints of a packed list of n_words records (len, id0 .. id(len-1), ...), or -1 with the message set
static int check_records(ze_engine* e, const int32_t* seqs, int n_words, const char* what) {
    const auto bad = [&](const char* why) {
        ze_fail(e, ZE_ERR_INVALID, (std::string(what) + ": " + why).c_str());
        return -1;
    };
    if (n_words < 0 || n_words > ZE_MAX_RULE_WORDS) return bad("at most 64 records");
    if (n_words > 0 && !seqs) return bad("null list");
    int off = 0;
    for (int w = 0; w < n_words; ++w) {
        if (off >= ZE_MAX_RULE_INTS) return bad("a packed list holds at most 1024 ints");
        const int len = seqs[off];
        if (len < 1 || len > ZE_MAX_RULE_LEN) return bad("a record holds 1 to 16 token ids");
        if (off + 1 + len > ZE_MAX_RULE_INTS) return bad("a packed list holds at most 1024 ints");
        for (int i = 0; i < len; ++i)
            if (seqs[off + 1 + i] < 0 || seqs[off + 1 + i] >= e->cfg.vocab) return bad("token id out of range");
        off += 1 + len;
    }
    return off;
}

extern "C" int ze_seq_set_token_rules(ze_engine* e, int seq, int no_repeat_ngram, const int32_t* stop_seqs, int n_stop_words,
                                      const int32_t* ban_seqs, int n_ban_words, const int32_t* context_ids, int n_context, void* stream) {
    ZE_TRY(check_seq(e, seq));
    const ze_config& c = e->cfg;
    if (no_repeat_ngram < 0 || no_repeat_ngram > ZE_MAX_RULE_LEN) return ze_fail(e, ZE_ERR_INVALID, "no_repeat_ngram must be in [0, 16] (0 = off)");
    const int stop_ints = check_records(e, stop_seqs, n_stop_words, "stop_seqs");
    if (stop_ints < 0) return ZE_ERR_INVALID;
    const int ban_ints = check_records(e, ban_seqs, n_ban_words, "ban_seqs");
    if (ban_ints < 0) return ZE_ERR_INVALID;
    if (n_context < 0 || n_context > c.max_ctx) return ze_fail(e, ZE_ERR_INVALID, "n_context must be in [0, max_ctx]");
    if (n_context > 0 && !context_ids) return ze_fail(e, ZE_ERR_INVALID, "null context_ids");
    for (int i = 0; i < n_context; ++i)
        if (context_ids[i] < 0 || context_ids[i] >= c.vocab) return ze_fail(e, ZE_ERR_INVALID, "context token id out of range");
    ze_requests::rules_host h;
    h.ngram = no_repeat_ngram, h.n_stop_ints = stop_ints, h.n_stop_words = n_stop_words, h.n_ban_ints = ban_ints, h.n_ban_words = n_ban_words;
    h.n_context = h.bans() ? n_context : 0;  // (stop records never look at the context)
    if (h.on() && e->spec.on(seq)) return ze_fail(e, ZE_ERR_INVALID, "the chain speculates (ze_seq_set_speculation): no token rules");
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    ze_requests& q = e->req;
    if (h.bans()) ZE_TRY(ensure_adjusted_rows(e));
    if (h.on() && !q.tr_stop)
        ZE_TRY(alloc_first_use(e, {buf_of(q.tr_stop, (size_t)c.max_seqs * ZE_MAX_RULE_INTS), buf_of(q.tr_ban, (size_t)c.max_seqs * ZE_MAX_RULE_INTS)},
                               "hipMalloc of the token-rule lists failed"));
    if (h.n_context > 0 && !q.tr_ctx)
        ZE_TRY(alloc_first_use(e, {buf_of(q.tr_ctx, (size_t)c.max_seqs * c.max_ctx)}, "hipMalloc of the context history failed"));
    // (a copy from pageable memory has left the caller's array when the call returns, and is ordered on the stream)
    if (h.n_context > 0)
        ZE_HIP(hipMemcpyAsync(q.tr_ctx + (size_t)seq * c.max_ctx, context_ids, (size_t)h.n_context * sizeof(int), hipMemcpyHostToDevice, s));
    write_rules(e, seq, h, stop_seqs, ban_seqs, s);
    ZE_KCHECK();
    return ZE_OK;
}

// ---- guided decoding (ze_grammar.hip the kernels)
static void write_grammar(ze_engine* e, int seq, int grammar, int state, hipStream_t s) {
    ze_requests& q = e->req;
    const int was = q.gr_host[seq];
    if (was < 0 && grammar < 0) return;
    if (was >= 0) q.gr_tab[was].users -= 1;
    if (grammar >= 0) q.gr_tab[grammar].users += 1;
    q.gr_host[seq] = grammar;
    q.n_grammar += (int)(grammar >= 0) - (int)(was >= 0);
    ze_launch_set_grammar(q.gr_dev, seq, grammar, state, s);
}

static int check_grammar(ze_engine* e, int grammar) {
    if (!e) return ze_fail(e, ZE_ERR_INVALID, "null engine");
    if (grammar < 0 || grammar >= ZE_MAX_GRAMMARS || !e->req.gr_tab[grammar].block) return ze_fail(e, ZE_ERR_NOTFOUND, "no such grammar");
    return ZE_OK;
}

// the grammar as the kernels see it: four tables in one allocation, the 4-byte words first
static ze_grammar_dev grammar_layout(void* block, int vocab, int n_states, int n_classes) {
    ze_grammar_dev g;
    g.n_states = n_states, g.n_classes = n_classes, g.words = ze_cdiv(vocab, 32);
    char* p = (char*)block;
    g.allow = (const uint32_t*)p;
    p += (size_t)n_states * g.words * sizeof(uint32_t);
    g.trans = (const int16_t*)p;
    p += (size_t)n_states * n_classes * sizeof(int16_t);
    g.token_class = (const uint16_t*)p;
    p += (size_t)vocab * sizeof(uint16_t);
    g.accepting = (const uint8_t*)p;
    return g;
}
static size_t grammar_bytes(int vocab, int n_states, int n_classes) {
    return (size_t)n_states * ze_cdiv(vocab, 32) * sizeof(uint32_t) + (size_t)n_states * n_classes * sizeof(int16_t) +
           (size_t)vocab * sizeof(uint16_t) + (size_t)n_states;
}

extern "C" int ze_grammar_create(ze_engine* e, const uint16_t* token_class, int n_classes, const int16_t* trans, int n_states,
                                 const uint8_t* accepting, int* out_grammar, void* stream) {
    if (!e) return ze_fail(e, ZE_ERR_INVALID, "null engine");
    if (!token_class || !trans || !accepting || !out_grammar) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    const ze_config& c = e->cfg;
    if (n_states < 1 || n_states > ZE_MAX_GRAMMAR_STATES) return ze_fail(e, ZE_ERR_INVALID, "n_states must be in [1, 2048]");
    if (n_classes < 1 || n_classes > ZE_MAX_GRAMMAR_CLASSES) return ze_fail(e, ZE_ERR_INVALID, "n_classes must be in [1, 4096]");
    const auto is_eos = [&](int t) {
        for (int k = 0; k < c.n_eos; ++k)
            if (c.eos_token_ids[k] == t) return true;
        return false;
    };
    std::vector<uint8_t> used(n_classes, 0);  // classes some token other than an EOS id has
    for (int t = 0; t < c.vocab; ++t) {
        if (is_eos(t)) continue;  // (its class is never looked at)
        if (token_class[t] >= n_classes) return ze_fail(e, ZE_ERR_INVALID, "token class out of range");
        used[token_class[t]] = 1;
    }
    for (int st = 0; st < n_states; ++st) {
        bool open = accepting[st] != 0;
        for (int k = 0; k < n_classes; ++k) {
            const int to = trans[(size_t)st * n_classes + k];
            if (to < -1 || to >= n_states) return ze_fail(e, ZE_ERR_INVALID, "transition outside [-1, n_states)");
            open |= to >= 0 && used[k];
        }
        if (!open) return ze_fail(e, ZE_ERR_INVALID, "a state that is not accepting allows no token (dead end)");
    }
    ze_requests& q = e->req;
    int id = 0;
    while (id < ZE_MAX_GRAMMARS && q.gr_tab[id].block) ++id;
    if (id == ZE_MAX_GRAMMARS) return ze_fail(e, ZE_ERR_INVALID, "an engine holds at most 16 grammars");
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    if (!q.gr_dev) {
        ZE_TRY(ensure_adjusted_rows(e));
        int* table = nullptr;
        ze_grammar_dev* desc = nullptr;
        const size_t entries = (size_t)c.max_seqs * ZE_GR_WORDS;
        ZE_TRY(alloc_first_use(e, {buf_of(table, entries), buf_of(desc, (size_t)ZE_MAX_GRAMMARS)}, "hipMalloc of the grammar tables failed"));
        // all zero = no grammar.  Once per engine, and waited for: setters on other streams may write their entries at once
        if (hipMemset(table, 0, entries * sizeof(int)) != hipSuccess || hipMemset(desc, 0, ZE_MAX_GRAMMARS * sizeof(ze_grammar_dev)) != hipSuccess ||
            hipStreamSynchronize(nullptr) != hipSuccess) {
            (void)hipGetLastError();
            hipFree(table);
            hipFree(desc);
            return ze_fail(e, ZE_ERR_HIP, "hipMemset of the grammar tables failed");
        }
        q.gr_dev = table, q.gr_desc = desc;
    }
    void* block = nullptr;
    if (hipMalloc(&block, grammar_bytes(c.vocab, n_states, n_classes)) != hipSuccess) {
        (void)hipGetLastError();
        return ze_fail(e, ZE_ERR_NOMEM, "hipMalloc of the grammar failed");
    }
    const ze_grammar_dev g = grammar_layout(block, c.vocab, n_states, n_classes);
    // (a copy from pageable memory has left the caller's array when the call returns, and is ordered on the stream)
    bool ok = hipMemcpyAsync((void*)g.trans, trans, (size_t)n_states * n_classes * sizeof(int16_t), hipMemcpyHostToDevice, s) == hipSuccess &&
              hipMemcpyAsync((void*)g.token_class, token_class, (size_t)c.vocab * sizeof(uint16_t), hipMemcpyHostToDevice, s) == hipSuccess &&
              hipMemcpyAsync((void*)g.accepting, accepting, (size_t)n_states, hipMemcpyHostToDevice, s) == hipSuccess;
    if (ok) {
        ze_launch_grammar_build(g, c.vocab, e->eos_dev, c.n_eos, (uint32_t*)g.allow, s);
        ze_launch_set_grammar_desc(q.gr_desc, id, g, s);
        ok = hipGetLastError() == hipSuccess;
    }
    // off the step path: the grammar is complete before any stream may use it
    if (hipStreamSynchronize(s) != hipSuccess) ok = false;
    if (!ok) {
        (void)hipGetLastError();
        hipFree(block);
        return ze_fail(e, ZE_ERR_HIP, "building the grammar on the device failed");
    }
    q.gr_tab[id].block = block, q.gr_tab[id].n_states = n_states, q.gr_tab[id].n_classes = n_classes, q.gr_tab[id].users = 0;
    *out_grammar = id;
    return ZE_OK;
}

extern "C" int ze_grammar_destroy(ze_engine* e, int grammar) {
    ZE_TRY(check_grammar(e, grammar));
    ze_requests::grammar_host& g = e->req.gr_tab[grammar];
    if (g.users > 0) return ze_fail(e, ZE_ERR_INVALID, "the grammar is still set on a chain");
    hipSetDevice(e->device);
    ZE_HIP(hipDeviceSynchronize());  // steps of chains that used it may still be in flight
    ze_launch_set_grammar_desc(e->req.gr_desc, grammar, ze_grammar_dev{}, nullptr);
    ZE_HIP(hipStreamSynchronize(nullptr));
    ZE_HIP(hipFree(g.block));
    g = ze_requests::grammar_host{};
    return ZE_OK;
}

extern "C" int ze_seq_set_grammar(ze_engine* e, int seq, int grammar, int state, void* stream) {
    ZE_TRY(check_seq(e, seq));
    if (grammar < -1) return ze_fail(e, ZE_ERR_INVALID, "grammar must be an id or -1 (clear)");
    if (grammar >= 0) {
        ZE_TRY(check_grammar(e, grammar));
        if (state < 0 || state >= e->req.gr_tab[grammar].n_states) return ze_fail(e, ZE_ERR_INVALID, "state outside the grammar");
    }
    if (grammar >= 0 && e->spec.on(seq)) return ze_fail(e, ZE_ERR_INVALID, "the chain speculates (ze_seq_set_speculation): no grammar");
    hipSetDevice(e->device);
    write_grammar(e, seq, grammar, state, (hipStream_t)stream);
    ZE_KCHECK();
    return ZE_OK;
}

extern "C" int ze_chain_grammar_state(ze_engine* e, int seq, int* state, int* violated, void* stream) {
    ZE_TRY(check_seq(e, seq));
    if (!state || !violated) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    *state = -1, *violated = 0;
    if (e->req.gr_host[seq] < 0) return ZE_OK;  // no grammar: state -1
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    int w[ZE_GR_WORDS];
    ZE_HIP(hipMemcpyAsync(w, e->req.gr_dev + (size_t)seq * ZE_GR_WORDS, sizeof(w), hipMemcpyDeviceToHost, s));
    ZE_HIP(hipStreamSynchronize(s));
    *state = w[1], *violated = w[2];
    return ZE_OK;
}

extern "C" int ze_op_grammar_mask(ze_engine* e, int grammar, const float* logits, int rows, int vocab, int ld, const int32_t* states, float* out,
                                  void* stream) {
    ZE_TRY(check_grammar(e, grammar));
    if (!logits || !states || !out || out == logits) return ze_fail(e, ZE_ERR_INVALID, "bad grammar_mask arguments");
    if (rows < 0 || vocab <= 0 || vocab > e->cfg.vocab || ld < vocab) return ze_fail(e, ZE_ERR_INVALID, "rows >= 0, 0 < vocab <= the engine's and ld >= vocab");
    if (rows == 0) return ZE_OK;
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    const ze_requests::grammar_host& h = e->req.gr_tab[grammar];
    ZE_HIP(hipMemcpy2DAsync(out, (size_t)ld * sizeof(float), logits, (size_t)ld * sizeof(float), (size_t)vocab * sizeof(float), rows,
                            hipMemcpyDeviceToDevice, s));
    ze_launch_grammar_mask(out, rows, vocab, ld, grammar_layout(h.block, e->cfg.vocab, h.n_states, h.n_classes), states, s);
    ZE_KCHECK();
    return ZE_OK;
}

extern "C" int ze_op_grammar_advance(ze_engine* e, int grammar, const int32_t* states, const int32_t* tokens, int rows, int32_t* out_states,
                                     void* stream) {
    ZE_TRY(check_grammar(e, grammar));
    if (!states || !tokens || !out_states || rows < 0) return ze_fail(e, ZE_ERR_INVALID, "bad grammar_advance arguments");
    hipSetDevice(e->device);
    const ze_requests::grammar_host& h = e->req.gr_tab[grammar];
    ze_launch_grammar_advance(rows, e->cfg.vocab, grammar_layout(h.block, e->cfg.vocab, h.n_states, h.n_classes), states, tokens, e->eos_dev,
                              e->cfg.n_eos, out_states, (hipStream_t)stream);
    ZE_KCHECK();
    return ZE_OK;
}

// ---- all kinds together
void ze_requests_clear(ze_engine* e, int seq, hipStream_t s) {
    const ze_requests& q = e->req;
    if (q.filt_host[seq].on()) write_filter(e, seq, 0, 1.f, 0.f, s);
    if (q.ent_host[seq].on()) write_entropy_filter(e, seq, 1.f, 0.f, 0.f, s);
    clear_sampling(e, seq, s);
    write_logprobs(e, seq, -1, s);
    if (q.la_host[seq].on()) write_adjust(e, seq, ze_requests::adjust_host{}, nullptr, nullptr, s);
    if (q.tr_host[seq].on()) write_rules(e, seq, ze_requests::rules_host{}, nullptr, nullptr, s);
    if (q.gr_host[seq] >= 0) write_grammar(e, seq, -1, 0, s);
    ze_spec_clear(e, seq, s);
}

void ze_requests_after_token(ze_engine* e, const float* logits, const int* seq_ids, int slot0, int n, hipStream_t s) {
    const ze_requests& q = e->req;
    ze_requests_logprobs(e, logits, seq_ids, slot0, n, s);
    if (seq_ids ? q.n_adjust > 0 : q.la_host[slot0].on()) ze_launch_count_tokens(e->st_dev, seq_ids, slot0, n, q.la_bufs(), e->cfg.vocab, s);
    // a stop record at the tail of the generated ids finishes its chain
    if (seq_ids ? q.n_stops > 0 : q.tr_host[slot0].stops())
        ze_launch_chain_token_stop(e->st_dev, seq_ids, slot0, n, q.tr_bufs(), q.la_dev, e->out_tokens, e->cfg.max_ctx, s);
    // the accepted token moves the chain's automaton on (last: it remembers whether the step finished the chain)
    if (seq_ids ? q.n_grammar > 0 : q.gr_host[slot0] >= 0)
        ze_launch_chain_grammar_advance(e->st_dev, seq_ids, slot0, n, q.gr_bufs(), e->cfg.vocab, e->eos_dev, e->cfg.n_eos, e->out_tokens,
                                        e->cfg.max_ctx, s);
}

// ---- the sampling options of a launch
// A sampled launch learns about filters only while some chain of the engine has one: with none set it is today's launch
// sequence.  `batch`: the cuts of a batched step (one per row) -- otherwise the slot's own word.
void ze_attach_filters(ze_engine* e, ze_sample_opts& so, bool batch) {
    const ze_requests& q = e->req;
    if (!so.draws() || q.n_filters + q.n_entropy == 0) return;
    const size_t at = batch ? 0 : (size_t)e->cfg.max_seqs + so.slot;
    so.cuts = q.cut_dev + at;
    if (q.n_filters > 0) so.filt = q.filt_dev;
    if (q.n_entropy > 0) {  // (the band selection starts from the filter's cut, or from -inf while no chain has a filter)
        so.ent = q.ent_dev;
        so.ceils = q.ceil_dev + at;
    }
}

// The repetition penalty a single-chain launch runs with: the chain's own while it has a sampling request, else the call's
float ze_penalty_of(const ze_engine* e, const ze_gen_params* p, int seq) {
    if (e->req.samp_host[seq].penalty > 0.f) return e->req.samp_host[seq].penalty;
    return p->repetition_penalty > 0.f ? p->repetition_penalty : 1.0f;
}

// A single-chain launch serves one known chain: its request (ze_seq_set_sampling) is resolved here, on the host, and the scalar
// kernels run with the chain's own values.  `batch`: the call's values stay the launch's defaults, and the per-slot table joins
// them while some chain of the engine has a request -- with none it is today's launch sequence.
ze_sample_opts ze_sample_opts_of(ze_engine* e, const ze_gen_params* p, int slot, bool batch) {
    ze_sample_opts so;
    const ze_chain_sampling& req = e->req.samp_host[slot];
    if (!batch && req.penalty > 0.f) {
        so.temperature = req.temperature;
        so.seed = req.temperature > 0.f ? req.seed : 0ull;
    } else if (p->do_sample && p->temperature > 0.f) {
        so.temperature = p->temperature;
        so.seed = p->seed;
    }
    if (batch && e->req.n_sampling > 0) {
        so.samp = e->req.samp_dev;
        so.samp_draws = e->req.n_sampled > 0;
    }
    so.slot = slot;
    ze_attach_filters(e, so, batch);
    return so;
}

// The key of a captured step: the effective values of the launch (a new request re-captures), and per request kind what the step
// launches for it -- of a single-chain step by THAT chain's request, of a batched step by the engine's.  Never a request's values.
ze_step_key ze_step_key_of(const ze_engine* e, int n, int seq, float penalty, int ignore_eos, const ze_sample_opts& so, int kind, int n_plain,
                           int n_chains, int n_drawn, int n_drawn_rows) {
    const ze_requests& q = e->req;
    ze_step_key k;
    k.n = n;
    k.kind = kind;
    k.n_plain = n_plain;
    k.n_chains = n_chains;
    k.n_drawn = n_drawn;
    k.n_drawn_rows = n_drawn_rows;
    k.penalty = penalty;
    k.ignore_eos = ignore_eos;
    k.temperature = so.temperature;
    k.seed = so.seed;
    k.tune_epoch = n ? 0u : ze_tune_epoch;
    k.live_parts = n ? e->live_parts : 0;
    k.live_parts_long = n ? e->live_parts_long : 0;
    k.sampling_bits = (int)(so.filt != nullptr) | (int)(so.samp != nullptr) << 1 | (int)so.samp_draws << 2 | (int)(so.ent != nullptr) << 3;
    k.lp_mode = q.lp_mode();
    k.la_mode = n ? q.la_mode() : q.la_mode(seq);
    k.tr_mode = n ? q.tr_mode() : q.tr_mode(seq);
    k.gr_mode = n ? q.gr_mode() : q.gr_mode(seq);
    return k;
}

// Chain state of the engine: the shared-prefix hints and their device words, the chain state pushed to the device, every ze_seq_*
// entry (reset, retire, truncate, copy_prefix, fork, ...), the seen-set marks and the id transfer scratch they share with ze_requests.hip.
#include <string.h>

#include "ze_engine.h"

// ================================================================== chains
// ---- shared-prefix hints (ze_engine::pfx_host / pfx_dev; the ownership rule is stated in ze_engine.h)
static void set_prefix_hint(ze_engine* e, int seq, int value) { e->pfx_host[seq] = value; }
// the K/V rows chain `d` copied (ze_seq_copy_prefix) have landed: nothing recorded, or the event behind the copy is over
static bool prefix_copy_done(ze_engine* e, int d) {
    hipEvent_t ev = e->pfx_copy_ev[d];
    return !ev || hipEventQuery(ev) == hipSuccess;
}
// rows below `keep` of chain `seq` are about to change (or the chain is over): chains that read their prefix from it move to
// the one among them with the longest prefix WHOSE COPY HAS LANDED (its own rows hold the same bits), which goes back to reading
// its own rows; readers it does not cover -- and all of them when no copy has landed yet -- go back to their own rows as well
// (a chain joins a decode step only behind its own prefill pass, so its own rows are always good by then)
void prefix_source_gone(ze_engine* e, int seq, int keep) {
    int leader = -1, lead_p = 0;
    const int n = (int)e->pfx_host.size();
    for (int d = 0; d < n; ++d) {
        const int h = e->pfx_host[d];
        if (h != 0 && (h >> 16) == seq && (h & 0xffff) > keep && (h & 0xffff) > lead_p && prefix_copy_done(e, d))
            leader = d, lead_p = h & 0xffff;
    }
    for (int d = 0; d < n; ++d) {
        const int h = e->pfx_host[d];
        if (h == 0 || (h >> 16) != seq || (h & 0xffff) <= keep) continue;
        const int p = h & 0xffff;
        set_prefix_hint(e, d, (leader < 0 || d == leader || p > lead_p) ? 0 : ((leader << 16) | p));
    }
}
// Before a batched decode step is enqueued on `s`: the device words of ITS chains follow the host's (the one place pfx_dev is
// written, on the one stream that reads it)
void sync_prefix(ze_engine* e, const int32_t* seqs, int n, hipStream_t s) {
    int idx[64], val[64], m = 0;
    for (int i = 0; i < n; ++i) {
        const int q = seqs[i];
        const int want = (e->prefix_hints && ze_knobs[ZE_KNOB_NO_PREFIX_HINTS] != ZE_KNOB_ON) ? e->pfx_host[q] : 0;
        if (e->pfx_pushed[q] == want) continue;
        e->pfx_pushed[q] = want;
        idx[m] = q, val[m] = want;
        if (++m == 64) ze_launch_scatter_ints(e->pfx_dev, idx, val, m, s), m = 0;
    }
    if (m) ze_launch_scatter_ints(e->pfx_dev, idx, val, m, s);
}

int push_state(ze_engine* e, int seq, hipStream_t s, int token, int n_gen, int finished) {
    ze_seq_dev st;
    memset(&st, 0, sizeof(st));
    st.ctx = e->ctx_host[seq];
    st.rope_delta = e->delta_host[seq];
    st.token = token;
    st.finished = finished;
    st.n_gen = n_gen;
    st.max_gen = e->cfg.max_ctx;
    st.split = e->split_host[seq];
    static_assert(sizeof(ze_seq_dev) == 8 * sizeof(int), "chain state is eight ints");
    ze_launch_set_ints(reinterpret_cast<int*>(e->st_dev + seq), reinterpret_cast<const int*>(&st), 8, s);
    return ZE_OK;
}

extern "C" int ze_seq_reset(ze_engine* e, int seq, void* stream) {
    ZE_TRY(check_seq(e, seq));
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    e->ctx_host[seq] = 0;
    e->delta_host[seq] = 0;
    e->split_host[seq] = 0;
    e->logits_fresh[seq] = 0;
    prefix_source_gone(e, seq, 0);
    e->pfx_host[seq] = 0;
    ZE_HIP(hipMemsetAsync(e->seen + (size_t)seq * e->cfg.vocab, 0, e->cfg.vocab, s));
    ze_requests_clear(e, seq, s);
    return push_state(e, seq, s, 0, 0, 0);
}

// The chain in `seq` is over and its slot may be given to another chain: no decode step ENQUEUED after this call reads a prefix
// from it (the step pushes the changed hints on its own stream first: sync_prefix).  The caller orders the call behind the
// steps already in flight that may still read the slot's rows -- a scheduler calls it between bursts -- before it lets anything
// overwrite them.  `stream` is unused since round 4 (kept for the ABI): hints are host state until a decode step picks them up.
extern "C" int ze_seq_retire(ze_engine* e, int seq, void* stream) {
    (void)stream;
    ZE_TRY(check_seq(e, seq));
    prefix_source_gone(e, seq, 0);
    set_prefix_hint(e, seq, 0);
    return ZE_OK;
}

// Declares that the first `rows` cached tokens of `seq` hold the same bits as the source chain's (the caller's knowledge: a
// prefix it wrote to both; ze_seq_copy_prefix records this by itself).  rows = 0 clears.  Also the measurement hook of
// bench.py / tools/pmc_kernel.py: the decode attention timed with the sharing the question stream has.
extern "C" int ze_seq_set_prefix_hint(ze_engine* e, int seq, int src_seq, int rows, void* stream) {
    (void)stream;
    ZE_TRY(check_seq(e, seq));
    if (rows <= 0 || src_seq == seq) {
        set_prefix_hint(e, seq, 0);
        return ZE_OK;
    }
    ZE_TRY(check_seq(e, src_seq));
    if (rows > e->ctx_host[seq] || rows > e->ctx_host[src_seq] || rows >= 65536 || !e->prefix_hints)
        return ze_fail(e, ZE_ERR_INVALID, "prefix hint: rows exceed a chain's context (or hints are switched off)");
    set_prefix_hint(e, seq, (src_seq << 16) | rows);
    return ZE_OK;
}

// (source chain << 16) | rows: where the decode attention reads the first rows of `seq` from; 0 = its own cache
// Measurement / test entry: declares row `rows` the chain's split row (what prefilling tokens with an image block does by itself,
// note_split) -- for chains built from text ids that stand in for image prompts (tools/pmc_kernel.py, bench.py's annex, tests).
extern "C" int ze_seq_set_split(ze_engine* e, int seq, int rows, void* stream) {
    ZE_TRY(check_seq(e, seq));
    if (rows < 0 || rows > e->ctx_host[seq] || rows >= 65536) return ze_fail(e, ZE_ERR_INVALID, "split row out of range");
    hipSetDevice(e->device);
    e->split_host[seq] = rows;
    ze_launch_set_ints(&(e->st_dev + seq)->split, &rows, 1, (hipStream_t)stream);
    return ZE_OK;
}

extern "C" int ze_seq_prefix_hint(ze_engine* e, int seq) {
    if (check_seq(e, seq) != 0) return ZE_ERR_NOTFOUND;
    return e->pfx_host[seq];
}

extern "C" int ze_seq_truncate(ze_engine* e, int seq, int keep_len, void* stream) {
    ZE_TRY(check_seq(e, seq));
    if (keep_len < 0 || keep_len > e->ctx_host[seq]) return ze_fail(e, ZE_ERR_INVALID, "keep_len out of range");
    hipSetDevice(e->device);
    e->ctx_host[seq] = keep_len;
    e->logits_fresh[seq] = 0;
    if (keep_len < e->split_host[seq]) e->split_host[seq] = 0;   // (the image block itself is cut: the rest is a chain without one)
    prefix_source_gone(e, seq, keep_len);   // rows from keep_len on will be rewritten
    if ((e->pfx_host[seq] & 0xffff) > keep_len) e->pfx_host[seq] = 0;
    // the seen-set belongs to the dropped continuation: the caller re-marks the (new) prompt
    ZE_HIP(hipMemsetAsync(e->seen + (size_t)seq * e->cfg.vocab, 0, e->cfg.vocab, (hipStream_t)stream));
    ze_requests_clear(e, seq, (hipStream_t)stream);
    return push_state(e, seq, (hipStream_t)stream, 0, 0, 0);
}

extern "C" int ze_seq_copy_prefix(ze_engine* e, int dst_seq, int src_seq, int n_tokens, void* stream) {
    ZE_TRY(check_seq(e, dst_seq));
    ZE_TRY(check_seq(e, src_seq));
    if (dst_seq == src_seq) return ze_fail(e, ZE_ERR_INVALID, "source and destination chain are the same");
    if (n_tokens <= 0 || n_tokens > e->ctx_host[src_seq]) return ze_fail(e, ZE_ERR_INVALID, "n_tokens exceeds the source chain's context");
    const ze_config& c = e->cfg;
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t head_stride = (size_t)c.max_ctx * e->head_dim, seq_stride = (size_t)c.kv_heads * head_stride;
    ze_launch_kv_copy_prefix(e->kcache, e->vcache, (size_t)c.max_seqs * seq_stride, seq_stride, head_stride, c.layers, c.kv_heads,
                             e->head_dim, src_seq, dst_seq, n_tokens, s);
    ZE_KCHECK();
    e->ctx_host[dst_seq] = n_tokens;
    e->delta_host[dst_seq] = 0;
    e->logits_fresh[dst_seq] = 0;
    // the split row travels with the rows: the copy holds the source's first image block iff it reaches past its end (the same
    // tokens, the same split -- however a chain came by its rows)
    e->split_host[dst_seq] = (e->split_host[src_seq] > 0 && e->split_host[src_seq] <= n_tokens) ? e->split_host[src_seq] : 0;
    prefix_source_gone(e, dst_seq, 0);
    if (!e->pfx_copy_ev[dst_seq]) ZE_HIP(hipEventCreateWithFlags(&e->pfx_copy_ev[dst_seq], hipEventDisableTiming));
    ZE_HIP(hipEventRecord(e->pfx_copy_ev[dst_seq], s));  // (a holder other chains may be pointed at only once this is over)
    // the copy stays (the prefill attention of a later pass reads the chain's own rows); the decode attention reads the
    // source's -- or the source's own source, when that one covers these rows
    {
        int src = src_seq;
        const int hs = e->pfx_host[src_seq];
        if (hs != 0 && (hs & 0xffff) >= n_tokens) src = hs >> 16;
        e->pfx_host[dst_seq] = (e->prefix_hints && n_tokens < 65536 && src != dst_seq) ? ((src << 16) | n_tokens) : 0;
    }
    ZE_HIP(hipMemsetAsync(e->seen + (size_t)dst_seq * c.vocab, 0, c.vocab, s));
    ze_requests_clear(e, dst_seq, s);
    return push_state(e, dst_seq, s, 0, 0, 0);
}

// The whole chain `src_seq`, n times (include/zoomearth.h): validation first -- after an error nothing was enqueued or changed --
// then the destination table, ONE launch of k_kv_fork (ze_fork.hip: K/V rows, logits row, seen-set), and per destination the host
// state ze_seq_copy_prefix keeps, with the rope delta and the prompt's last id handed on (no prefill follows).
extern "C" int ze_seq_fork(ze_engine* e, int src_seq, const int32_t* dst_seqs, int n, void* stream) {
    ZE_TRY(check_seq(e, src_seq));
    if (!dst_seqs || n <= 0) return ze_fail(e, ZE_ERR_INVALID, "fork needs a table of n > 0 destination chains");
    for (int i = 0; i < n; ++i) {
        ZE_TRY(check_seq(e, dst_seqs[i]));
        if (dst_seqs[i] == src_seq) return ze_fail(e, ZE_ERR_INVALID, "source and destination chain are the same");
        for (int j = 0; j < i; ++j)
            if (dst_seqs[j] == dst_seqs[i]) return ze_fail(e, ZE_ERR_INVALID, "a destination chain appears twice");
    }
    const int rows = e->ctx_host[src_seq];
    if (rows <= 0) return ze_fail(e, ZE_ERR_INVALID, "the source chain is empty");
    if (!e->logits_fresh[src_seq])
        return ze_fail(e, ZE_ERR_INVALID, "the source chain's logits are not those of its last row (it drew, stepped or changed since its prefill)");
    if (n > e->prefill_rows) return ze_fail(e, ZE_ERR_NOMEM, "more destinations than the id buffer holds");
    const ze_config& c = e->cfg;
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    // the destination slots travel as kernel arguments into the prefill's id buffer, in stream order behind whatever still reads it
    // (ze_seq_mark_seen's way: no allocation, no staging buffer to wait for)
    ze_launch_set_ints(e->tsrc, dst_seqs, n, s);
    const size_t head_stride = (size_t)c.max_ctx * e->head_dim, seq_stride = (size_t)c.kv_heads * head_stride;
    ze_launch_kv_fork(e->kcache, e->vcache, (size_t)c.max_seqs * seq_stride, seq_stride, head_stride, c.layers, c.kv_heads, e->head_dim,
                      src_seq, e->tsrc, n, rows, e->dlogits, e->seen, c.vocab, s);
    ZE_KCHECK();
    // the decode attention reads the prompt from the source -- or the source's own holder, when that one covers the rows (the rule
    // of ze_seq_copy_prefix): one copy of the prompt is streamed for all siblings
    // (looked up per destination, behind prefix_source_gone: a destination that WAS the source's holder is none afterwards)
    for (int i = 0; i < n; ++i) {
        const int d = dst_seqs[i];
        e->ctx_host[d] = rows;
        e->delta_host[d] = e->delta_host[src_seq];
        e->split_host[d] = e->split_host[src_seq];
        e->tok_host[d] = e->tok_host[src_seq];
        e->logits_fresh[d] = 1;
        prefix_source_gone(e, d, 0);
        if (!e->pfx_copy_ev[d]) ZE_HIP(hipEventCreateWithFlags(&e->pfx_copy_ev[d], hipEventDisableTiming));
        ZE_HIP(hipEventRecord(e->pfx_copy_ev[d], s));  // (a holder other chains may be pointed at only once this is over)
        const int hs = e->pfx_host[src_seq];
        const int holder = (hs != 0 && (hs & 0xffff) >= rows) ? (hs >> 16) : src_seq;
        e->pfx_host[d] = (e->prefix_hints && rows < 65536 && holder != d) ? ((holder << 16) | rows) : 0;
        ze_requests_clear(e, d, s);
        ZE_TRY(push_state(e, d, s, e->tok_host[d], 0, 0));
    }
    return ZE_OK;
}

extern "C" int ze_seq_len(ze_engine* e, int seq) {
    if (check_seq(e, seq) != 0) return ZE_ERR_NOTFOUND;
    return e->ctx_host[seq];
}

extern "C" int ze_seq_mark_seen(ze_engine* e, int seq, const int32_t* ids, int n, void* stream) {
    ZE_TRY(check_seq(e, seq));
    if (n < 0 || (n > 0 && !ids)) return ze_fail(e, ZE_ERR_INVALID, "bad ids");
    if ((size_t)n > e->t_host_ints_cap) return ze_fail(e, ZE_ERR_NOMEM, "too many ids");
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= e->cfg.vocab) return ze_fail(e, ZE_ERR_INVALID, "token id out of range");
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    // the ids travel as kernel arguments (128 per launch) into the prefill's id buffer, in stream order behind whatever still
    // reads it: no pinned staging buffer to wait for -- the stream synchronisation this call used to begin with made the
    // scheduler wait for its whole prefill pass once per request (2.1 ms per call on the real entry point)
    ze_launch_set_ints(e->tsrc, ids, n, s);
    ze_launch_mark_seen(e->seen + (size_t)seq * e->cfg.vocab, e->tsrc, n, s);
    ZE_KCHECK();
    return ZE_OK;
}

// pinned + device scratch of the batched id transfers, sized by the REQUEST and grown on demand (max_seqs x max_ctx ints per
// direction were ~100 MB four times over at 768 slots x 32 K context, for calls that move a few hundred KB): `need` ints, rounded up
// to the next power of two from 64 Ki ints on.  Growing waits for the work that may still read the old block (the caller's stream and
// the block's staging event), frees it, and allocates anew; a failed device allocation frees the pinned half it had just obtained.
int xfer_reserve(ze_engine* e, int*& host, int*& dev, size_t& cap, size_t need, hipEvent_t staged, hipStream_t s) {
    if (need <= cap) return ZE_OK;
    size_t want = (size_t)64 << 10;
    while (want < need) want <<= 1;
    if (cap) {
        if (staged) ZE_HIP(hipEventSynchronize(staged));
        ZE_HIP(hipStreamSynchronize(s));
        hipHostFree(host);
        hipFree(dev);
        host = dev = nullptr;
        cap = 0;
    }
    int *h = nullptr, *d = nullptr;
    ZE_HIP(hipHostMalloc((void**)&h, want * sizeof(int)));
    if (hipMalloc((void**)&d, want * sizeof(int)) != hipSuccess) {
        hipHostFree(h);
        return ze_fail(e, ZE_ERR_NOMEM, "hipMalloc of the id transfer scratch failed");
    }
    host = h;
    dev = d;
    cap = want;
    return ZE_OK;
}

// ze_seq_mark_seen for the n chains of a prefill pass at once: ONE host -> device copy and ONE launch instead of ~10 launches per
// chain (the scheduler's thread spent 1.4 ms per chain in the single-chain call on a busy GPU: 1.8 s per lane of the 15-s stream)
extern "C" int ze_seq_mark_seen_batch(ze_engine* e, const int32_t* seqs, const int32_t* counts, int n, const int32_t* ids, void* stream) {
    if (!e || n < 0 || (n > 0 && (!seqs || !counts))) return ze_fail(e, ZE_ERR_INVALID, "bad arguments");
    if (n == 0) return ZE_OK;
    if (n > e->cfg.max_seqs) return ze_fail(e, ZE_ERR_INVALID, "more chains than slots");
    size_t total = 0;
    int max_count = 0;
    for (int i = 0; i < n; ++i) {
        ZE_TRY(check_seq(e, seqs[i]));
        if (counts[i] < 0 || counts[i] > e->cfg.max_ctx) return ze_fail(e, ZE_ERR_INVALID, "bad id count");
        total += (size_t)counts[i];
        max_count = std::max(max_count, counts[i]);
    }
    if (total > 0 && !ids) return ze_fail(e, ZE_ERR_INVALID, "bad ids");
    for (size_t i = 0; i < total; ++i)
        if (ids[i] < 0 || ids[i] >= e->cfg.vocab) return ze_fail(e, ZE_ERR_INVALID, "token id out of range");
    if (total == 0) return ZE_OK;
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    // (the event is recorded BEHIND the kernel that reads the device block -- ADVICE r5: behind the copy alone, a second call on
    //  another stream could have overwritten xs_dev under the first call's kernel; acquire waits for that kernel now)
    ZE_TRY(stage_acquire(e, e->xs_staged));
    ZE_TRY(xfer_reserve(e, e->xs_host, e->xs_dev, e->xs_cap, (size_t)(2 * n + 1) + total, e->xs_staged, s));
    int* h = e->xs_host;
    h[0] = 0;
    for (int i = 0; i < n; ++i) {
        h[i + 1] = h[i] + counts[i];
        h[n + 1 + i] = seqs[i];
    }
    memcpy(h + 2 * n + 1, ids, total * sizeof(int));
    ZE_HIP(hipMemcpyAsync(e->xs_dev, h, ((size_t)(2 * n + 1) + total) * sizeof(int), hipMemcpyHostToDevice, s));
    ze_launch_mark_seen_batch(e->seen, e->cfg.vocab, e->xs_dev, e->xs_dev + 2 * n + 1, n, max_count, s);
    ZE_KCHECK();
    ZE_TRY(stage_release(e, e->xs_staged, s));
    return ZE_OK;
}

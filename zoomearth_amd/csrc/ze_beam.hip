// Beam search on the device (include/zoomearth.h: ze_beam_search, ze_op_beam_step, ze_op_kv_reorder).
// replaces: GenerationMixin._beam_search with do_sample = False (HF:generation/utils.py:3208-3560) -- log_softmax + processors + running
// scores (:3388-3420), _get_top_k_continuations (:3077-3129), _get_running_beams_for_next_iteration (:3131-3151),
// _update_finished_beams (:3153-3204), _check_early_stop_heuristic (:3008-3052), _beam_search_has_unfinished_sequences (:3055-3075)
// and the cache reorder (:3477-3489) -- per group (one prompt), i.e. HF at batch size 1.
//
// Between two forwards a step is three launches on the burst's stream, one behind the other:
//   k_beam_rows     one workgroup per beam row, three passes over the row: maximum, sum of expf(l - max), then the row's B best non-EOS
//                   (score, token) and its n_eos EOS scores, score = penalised log-probability + the beam's running score
//   k_beam_select   one workgroup per group: total order over the B * (B + n_eos) candidates (score descending, then flat index
//                   beam * vocab + token ascending), the finished pool, the stop conditions, the slot assignment, the chain states
//   k_beam_reorder  every slot whose hypothesis comes from another slot takes that slot's generated K/V rows, generated ids, beam
//                   indices and seen-set
// Hazards.  The slot assignment (k_beam_select) lets a surviving parent keep one child in its own slot, so a slot that k_beam_reorder
// reads is never one it writes.  What k_beam_select itself writes into a slot that k_beam_reorder reads lies outside what is copied:
// the new id and beam index at position n (the copy takes [0, n)), and the new id's seen byte, whose earlier value it keeps in
// seen_prev so that the copy hands a sibling the parent's set as it was.
#include "ze_engine.h"

#include <cmath>
#include <cstring>

struct ze_beam_args {
    ze_seq_dev* st;
    uint8_t* seen;
    int32_t* out_tokens;
    const int* eos_ids;
    const int *seqs, *glist;
    int *gstate, *brank, *cand_tok, *parent, *seen_prev, *bidx, *fin_len, *fin_is, *fin_order, *fin_tok, *fin_bidx;
    float *run_score, *cand_score, *fin_score;
    const float* divs;
    int B, n_eos, vocab, seen_stride, max_ctx, cap, early;
    float penalty, length_penalty;
};

enum { BM_N = 0, BM_DONE = 1, BM_HEUR = 2, BM_PROMPT = 3, BM_MAXNEW = 4, BM_NEVER_DIV = 5 };

// (score descending, index ascending): the one order every comparison of a step is made under
__device__ __forceinline__ bool bm_better(float s, int i, float os, int oi) { return s > os || (s == os && i < oi); }

__device__ __forceinline__ float bm_score(float l, float m, float logz, bool seen, float penalty, float run) {
    float lp = (l - m) - logz;
    if (seen) lp = lp < 0.f ? lp * penalty : lp / penalty;   // (HF runs the processors on the log-probabilities: :3389)
    return lp + run;
}

// the workgroup's best (score, index) under bm_better; every thread returns it
__device__ __forceinline__ void bm_reduce_best(float& s, int& i, float* rs, int* ri) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float os = __shfl_xor(s, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (bm_better(os, oi, s, i)) s = os, i = oi;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) rs[threadIdx.x >> 6] = s, ri[threadIdx.x >> 6] = i;
    __syncthreads();
    s = rs[0], i = ri[0];
    for (int w = 1; w < 4; ++w)
        if (bm_better(rs[w], ri[w], s, i)) s = rs[w], i = ri[w];
}

// logits: fp32 rows of `ld` floats; by_slot: row of a beam = its chain slot (the logits a prefill / fork left), else its place in the
// step (glist order).  vec: ld % 4 == 0 and a 16-byte aligned base -- the row goes in float4 pieces.
__global__ void __launch_bounds__(256) k_beam_rows(const ze_beam_args a, const float* __restrict__ logits, int ld, int by_slot, int vec) {
    __shared__ float rs[4];
    __shared__ int ri[4];
    const int B = a.B, lg = blockIdx.x / B, j = blockIdx.x % B, g = a.glist[lg], row = g * B + j, tid = threadIdx.x;
    if (a.gstate[g * ZE_BM_GWORDS + BM_DONE]) return;
    const int slot = a.seqs[row], vocab = a.vocab;
    const float* lr = logits + (size_t)(by_slot ? slot : lg * B + j) * ld;
    const uint8_t* sn = a.seen + (size_t)slot * a.seen_stride;
    const bool pen = a.penalty != 1.0f;
    const float run = a.run_score[row];
    const int nv = vec ? vocab / 4 : 0;
    // ---- pass 1: the maximum
    float m = -INFINITY;
    for (int q = tid; q < nv; q += 256) {
        const float4 v = reinterpret_cast<const float4*>(lr)[q];
        m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    }
    for (int i = nv * 4 + tid; i < vocab; i += 256) m = fmaxf(m, lr[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((tid & 63) == 0) rs[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(rs[0], rs[1]), fmaxf(rs[2], rs[3]));
    __syncthreads();
    // ---- pass 2: the sum, in a fixed order (a thread's own pieces in order, the wave's tree, the four waves)
    float sum = 0.f;
    for (int q = tid; q < nv; q += 256) {
        const float4 v = reinterpret_cast<const float4*>(lr)[q];
        sum += expf(v.x - m);
        sum += expf(v.y - m);
        sum += expf(v.z - m);
        sum += expf(v.w - m);
    }
    for (int i = nv * 4 + tid; i < vocab; i += 256) sum += expf(lr[i] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((tid & 63) == 0) rs[tid >> 6] = sum;
    __syncthreads();
    const float logz = logf((rs[0] + rs[1]) + (rs[2] + rs[3]));
    __syncthreads();
    int eos[ZE_MAX_EOS];
#pragma unroll
    for (int k = 0; k < ZE_MAX_EOS; ++k) eos[k] = k < a.n_eos ? a.eos_ids[k] : -1;
    const int width = B + a.n_eos;
    float* cs = a.cand_score + (size_t)row * width;
    int* ct = a.cand_tok + (size_t)row * width;
    // ---- pass 3, the last over the row: every thread keeps the B best of its own non-EOS tokens, best first, in LDS columns of
    // its own ([place][thread]: no bank conflicts); then B rounds take the best head among the threads' lists.  The total order
    // makes the result independent of who held what.
    __shared__ float l_s[ZE_BM_MAX_BEAMS][256];
    __shared__ int l_i[ZE_BM_MAX_BEAMS][256];
    int cnt = 0;
    auto take = [&](float l, int i) {
        bool stop = false;
#pragma unroll
        for (int k2 = 0; k2 < ZE_MAX_EOS; ++k2) stop = stop || i == eos[k2];
        if (stop) return;
        const float s = bm_score(l, m, logz, pen && sn[i], a.penalty, run);
        if (!(s == s)) return;   // (a NaN compares with nothing: never a candidate)
        if (cnt == B && !bm_better(s, i, l_s[B - 1][tid], l_i[B - 1][tid])) return;
        int pos = cnt < B ? cnt++ : B - 1;
        for (; pos > 0 && bm_better(s, i, l_s[pos - 1][tid], l_i[pos - 1][tid]); --pos)
            l_s[pos][tid] = l_s[pos - 1][tid], l_i[pos][tid] = l_i[pos - 1][tid];
        l_s[pos][tid] = s, l_i[pos][tid] = i;
    };
    for (int q = tid; q < nv; q += 256) {
        const float4 v = reinterpret_cast<const float4*>(lr)[q];
        take(v.x, 4 * q), take(v.y, 4 * q + 1), take(v.z, 4 * q + 2), take(v.w, 4 * q + 3);
    }
    for (int i = nv * 4 + tid; i < vocab; i += 256) take(lr[i], i);
    int head = 0;
    for (int k = 0; k < B; ++k) {
        float bs = head < cnt ? l_s[head][tid] : -INFINITY;
        int bi = head < cnt ? l_i[head][tid] : 0x7fffffff;
        const int mine = bi;
        bm_reduce_best(bs, bi, rs, ri);
        const bool none = bi == 0x7fffffff;   // fewer than k + 1 non-EOS tokens in the row
        if (tid == 0) cs[k] = none ? -INFINITY : bs, ct[k] = none ? -1 : bi;
        if (none) {
            for (int r = k + 1 + tid; r < B; r += 256) cs[r] = -INFINITY, ct[r] = -1;
            break;
        }
        if (mine == bi) ++head;   // (token ids are distinct: one thread held the winner)
    }
    if (tid < a.n_eos) {
        const int t = eos[tid];
        const bool ok = t >= 0 && t < vocab;
        cs[B + tid] = ok ? bm_score(lr[t], m, logz, pen && sn[t], a.penalty, run) : -INFINITY;
        ct[B + tid] = ok ? t : -1;
    }
}

enum { BM_MAX_CAND = ZE_BM_MAX_BEAMS * (ZE_BM_MAX_BEAMS + ZE_MAX_EOS) };

__global__ void __launch_bounds__(256) k_beam_select(const ze_beam_args a) {
    __shared__ float c_score[BM_MAX_CAND];
    __shared__ int c_flat[BM_MAX_CAND], c_tok[BM_MAX_CAND], c_ord[BM_MAX_CAND];
    __shared__ unsigned char c_row[BM_MAX_CAND], c_beam[BM_MAX_CAND], c_eos[BM_MAX_CAND];
    // what thread 0 decides: run_c[k] the candidate that becomes running beam k, child_at[j] the running beam that lives in slot
    // position j, nf_* the new finished entries (pool entry, candidate, score)
    __shared__ int run_c[ZE_BM_MAX_BEAMS], child_at[ZE_BM_MAX_BEAMS], nf_entry[ZE_BM_MAX_BEAMS], nf_cand[ZE_BM_MAX_BEAMS], n_newfin, n_old_s, last_s;
    __shared__ float nf_score[ZE_BM_MAX_BEAMS];
    const int B = a.B, g = a.glist[blockIdx.x], tid = threadIdx.x, width = B + a.n_eos, nc = B * width;
    int* gs = a.gstate + g * ZE_BM_GWORDS;
    if (gs[BM_DONE]) {   // (between two reads of the done words a finished group rides along: every hypothesis stays where it is)
        if (tid < B) a.parent[a.seqs[g * B + tid]] = a.seqs[g * B + tid];
        return;
    }
    for (int c = tid; c < nc; c += 256) {
        const int j = c / width, k = c % width, tok = a.cand_tok[(size_t)(g * B + j) * width + k];
        const int beam = a.brank[g * B + j];
        c_row[c] = j, c_beam[c] = beam, c_eos[c] = k >= B, c_tok[c] = tok;
        c_score[c] = tok >= 0 ? a.cand_score[(size_t)(g * B + j) * width + k] : -INFINITY;
        c_flat[c] = tok >= 0 ? beam * a.vocab + tok : 0x7fffffff - c;   // (an empty entry: behind every real one, still distinct)
    }
    __syncthreads();
    for (int c = tid; c < nc; c += 256) {
        int rank = 0;
        const float s = c_score[c];
        const int f = c_flat[c];
        const bool real = c_tok[c] >= 0;
        for (int o = 0; o < nc; ++o) {
            const bool oreal = c_tok[o] >= 0;
            // real entries first; among them the total order (a NaN score, which compares with nothing, would break it: the engine's
            // logits have none)
            if (o != c && (oreal != real ? oreal : bm_better(c_score[o], c_flat[o], s, f))) ++rank;
        }
        c_ord[rank] = c;
    }
    __syncthreads();
    if (tid == 0) {
        const int n = gs[BM_N], max_new = gs[BM_MAXNEW];
        const bool last = n + 1 >= max_new;   // MaxLengthCriteria: every candidate of this step hits a stopping criterion (:3438)
        int n_run = 0, n_fc = 0, fc[ZE_BM_MAX_BEAMS];
        for (int r = 0; r < nc; ++r) {
            const int c = c_ord[r];
            if (c_tok[c] < 0) break;
            const bool hit = c_eos[c] || last;
            if (r < B && hit) fc[n_fc++] = c;                        // did_top_num_beams_just_finished (:3178)
            if ((last || !c_eos[c]) && n_run < B) run_c[n_run++] = c;   // (:3145-3147; at the last step every candidate is masked alike)
            if (r >= B && n_run == B) break;
        }
        for (int k = n_run; k < B; ++k) run_c[k] = run_c[0];   // (unreachable: the host checks vocab - n_eos >= B)
        // ---- slot assignment: a parent keeps its first child, the other children take the childless slots in ascending order
        bool has_child[ZE_BM_MAX_BEAMS];
        int slot_of[ZE_BM_MAX_BEAMS];
        for (int j = 0; j < B; ++j) has_child[j] = false;
        for (int k = 0; k < B; ++k) {
            const int pj = c_row[run_c[k]];
            slot_of[k] = has_child[pj] ? -1 : pj;
            has_child[pj] = true;
        }
        int fr = 0;
        for (int k = 0; k < B; ++k) {
            if (slot_of[k] >= 0) continue;
            while (has_child[fr]) ++fr;
            slot_of[k] = fr++;
        }
        for (int k = 0; k < B; ++k) child_at[slot_of[k]] = k;
        // ---- the finished pool (:3153-3204): entries by rank through fin_order, new entries behind equal old ones
        float* fsc = a.fin_score + g * B;
        int *fis = a.fin_is + g * B, *ford = a.fin_order + g * B;
        bool all_fin = true;
        for (int r = 0; r < B; ++r) all_fin = all_fin && fis[ford[r]];
        const bool admit = gs[BM_HEUR] && !(all_fin && a.early == 1);   // (:3184-3187)
        float ms[2 * ZE_BM_MAX_BEAMS];
        int me[2 * ZE_BM_MAX_BEAMS], mn = B;   // me >= 0: a pool entry; < 0: new candidate fc[-me - 1]
        for (int r = 0; r < B; ++r) ms[r] = fsc[ford[r]], me[r] = ford[r];
        for (int f = 0; admit && f < n_fc; ++f) {
            const float s = c_score[fc[f]] / a.divs[n + 1];   // (:3182)
            int pos = mn;
            while (pos > 0 && ms[pos - 1] < s) --pos;
            for (int r = mn; r > pos; --r) ms[r] = ms[r - 1], me[r] = me[r - 1];
            ms[pos] = s, me[pos] = -f - 1, ++mn;
        }
        int freed[ZE_BM_MAX_BEAMS], n_freed = 0, nn = 0;
        for (int r = B; r < mn; ++r)
            if (me[r] >= 0) freed[n_freed++] = me[r];
        for (int r = 0; r < B; ++r) {
            if (me[r] < 0) {
                const int entry = freed[nn];
                nf_entry[nn] = entry, nf_cand[nn] = fc[-me[r] - 1], nf_score[nn] = ms[r], ++nn;
                me[r] = entry;
                fis[entry] = 1;
                fsc[entry] = ms[r];
            }
            ford[r] = me[r];
        }
        n_newfin = nn, n_old_s = n, last_s = last;
        // ---- the stop conditions (:3491-3508), at the new length n + 1
        all_fin = true;
        float worst = INFINITY;
        for (int r = 0; r < B; ++r) all_fin = all_fin && fis[ford[r]], worst = fminf(worst, fsc[ford[r]]);
        const float div = (a.early == 2 && a.length_penalty > 0.f) ? __int_as_float(gs[BM_NEVER_DIV]) : a.divs[n + 1];
        const float best_run = (c_score[run_c[0]] + (last ? -1.0e9f : 0.f)) / div;
        bool improve = false;
        for (int r = 0; r < B; ++r) improve = improve || best_run > (fis[ford[r]] ? worst : -1.0e9f);
        const int heur = gs[BM_HEUR] && improve;
        gs[BM_HEUR] = heur;
        gs[BM_N] = n + 1;
        gs[BM_DONE] = !heur || (all_fin && a.early == 1) || last;
    }
    __syncthreads();
    const int n = n_old_s;
    // ---- the new finished hypotheses: the parent's ids and beam indices, then the candidate's own
    for (int f = 0; f < n_newfin; ++f) {
        const int c = nf_cand[f], src = a.seqs[g * B + c_row[c]];
        int* ft = a.fin_tok + (size_t)(g * B + nf_entry[f]) * a.cap;
        int* fb = a.fin_bidx + (size_t)(g * B + nf_entry[f]) * a.cap;
        for (int i = tid; i < n; i += 256) ft[i] = a.out_tokens[(size_t)src * a.max_ctx + i], fb[i] = a.bidx[(size_t)src * a.cap + i];
        if (tid == 0) ft[n] = c_tok[c], fb[n] = c_beam[c], a.fin_len[g * B + nf_entry[f]] = n + 1;
    }
    __syncthreads();   // (the rows read above are the ones written below, at position n only -- which nothing above reads)
    if (tid < B) {
        const int j = tid, k = child_at[j], c = run_c[k], slot = a.seqs[g * B + j], pslot = a.seqs[g * B + c_row[c]], tok = c_tok[c];
        a.parent[slot] = pslot;
        a.brank[g * B + j] = k;
        a.run_score[g * B + j] = c_score[c] + (last_s ? -1.0e9f : 0.f);
        a.bidx[(size_t)slot * a.cap + n] = c_beam[c];
        a.out_tokens[(size_t)slot * a.max_ctx + n] = tok;
        a.st[slot].token = tok;
        a.st[slot].n_gen = n + 1;
        if (pslot == slot) {
            uint8_t* sn = a.seen + (size_t)slot * a.seen_stride;
            a.seen_prev[slot] = sn[tok];
            sn[tok] = 1;
        }
    }
}

// blockIdx.z: a row of the step (beam call: glist order; unit call, glist null: z names seqs[z] itself); blockIdx.y < kv_runs: one
// (layer, kv head, K|V) run, rows [row0, end) of it in 16-byte pieces, as k_kv_fork cuts it; kv_runs: the generated ids and the beam
// indices; kv_runs + 1: the seen-set.  A slot whose hypothesis stays (parent == slot) leaves at once.
__global__ void __launch_bounds__(256) k_beam_reorder(const ze_beam_args a, bf16_t* __restrict__ kcache, bf16_t* __restrict__ vcache,
                                                      size_t layer_stride, size_t seq_stride, size_t head_stride, int kv_heads, int kv_runs,
                                                      int pieces_per_row, int unit_row0, int unit_rows) {
    const int z = blockIdx.z, y = blockIdx.y, first = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
    const int g = a.glist ? a.glist[z / a.B] : 0, slot = a.seqs[a.glist ? g * a.B + z % a.B : z], src = a.parent[slot];
    if (src == slot) return;
    const int* gs = a.gstate + g * ZE_BM_GWORDS;
    if (y < kv_runs) {
        const int row0 = a.glist ? gs[BM_PROMPT] : unit_row0;
        const int end = a.glist ? min(a.st[slot].ctx, a.max_ctx) : unit_row0 + unit_rows;
        if (end <= row0) return;
        const int which = y & 1, kvh = (y >> 1) % kv_heads, layer = (y >> 1) / kv_heads;
        bf16_t* base = (which ? vcache : kcache) + (size_t)layer * layer_stride + (size_t)kvh * head_stride;
        const uint4* s = reinterpret_cast<const uint4*>(base + (size_t)src * seq_stride) + (size_t)row0 * pieces_per_row;
        uint4* d = reinterpret_cast<uint4*>(base + (size_t)slot * seq_stride) + (size_t)row0 * pieces_per_row;
        const int n_vec = (end - row0) * pieces_per_row;
        for (int i = first; i < n_vec; i += step) d[i] = s[i];
        return;
    }
    if (y == kv_runs) {   // positions [0, n): position n is the slot's own (k_beam_select)
        const int n = gs[BM_N] - 1;
        for (int i = first; i < n; i += step) {
            a.out_tokens[(size_t)slot * a.max_ctx + i] = a.out_tokens[(size_t)src * a.max_ctx + i];
            a.bidx[(size_t)slot * a.cap + i] = a.bidx[(size_t)src * a.cap + i];
        }
        return;
    }
    // the parent's set as it was before k_beam_select marked the id of the child it keeps, then this slot's own new id
    const int ptok = a.st[src].token, tok = a.st[slot].token;
    const uint8_t pprev = (uint8_t)a.seen_prev[src];
    const uint8_t* sp = a.seen + (size_t)src * a.seen_stride;
    uint8_t* dp = a.seen + (size_t)slot * a.seen_stride;
    if (a.seen_stride % 16 == 0) {
        for (int i = first; i < a.seen_stride / 16; i += step) {
            uint4 v = reinterpret_cast<const uint4*>(sp)[i];
            uint8_t* b = reinterpret_cast<uint8_t*>(&v);
            if (ptok >> 4 == i) b[ptok & 15] = pprev;
            if (tok >> 4 == i) b[tok & 15] = 1;
            reinterpret_cast<uint4*>(dp)[i] = v;
        }
        return;
    }
    for (int i = first; i < a.seen_stride; i += step) dp[i] = i == tok ? 1 : (i == ptok ? pprev : sp[i]);
}

// a group's tables as a call finds them: beam 0 runs at 0, the others at -1e9 (:3332-3334), an empty finished pool
__global__ void k_beam_init(const ze_beam_args a) {
    const int g = blockIdx.x, j = threadIdx.x;
    if (j >= a.B) return;
    a.run_score[g * a.B + j] = j == 0 ? 0.f : -1.0e9f;
    a.brank[g * a.B + j] = j;
    a.fin_score[g * a.B + j] = -1.0e9f;
    a.fin_is[g * a.B + j] = 0;
    a.fin_len[g * a.B + j] = 0;
    a.fin_order[g * a.B + j] = j;
    a.parent[a.seqs[g * a.B + j]] = a.seqs[g * a.B + j];
}

// ================================================================== host side
void ze_beam_free(ze_engine* e) {
    ze_beam* b = e->beam;
    if (!b) return;
    void* dev[] = {b->u_seqs, b->u_parent, b->seqs, b->glist, b->gstate, b->brank, b->cand_tok, b->parent, b->seen_prev, b->bidx, b->fin_len, b->fin_is,
                   b->fin_order, b->fin_tok, b->fin_bidx, b->run_score, b->cand_score, b->fin_score, b->divs};
    for (void* p : dev)
        if (p) hipFree(p);
    delete b;
    e->beam = nullptr;
}

// the buffers of a call whose hypotheses hold up to `need` generated tokens: all or none (after ZE_ERR_NOMEM the engine has no beam
// buffers and is usable as before)
static int beam_alloc(ze_engine* e, int need) {
    if (e->beam && e->beam->cap >= need) return ZE_OK;
    ze_beam_free(e);
    ze_beam* b = new ze_beam();
    e->beam = b;
    const size_t rows = (size_t)e->cfg.max_seqs, width = ZE_BM_MAX_BEAMS + ZE_MAX_EOS;
    b->rows = (int)rows, b->cap = need;
    bool ok = true;
    auto get = [&](auto** p, size_t count) {
        if (ok && hipMalloc((void**)p, std::max<size_t>(count, 1) * 4) != hipSuccess) ok = false, *p = nullptr, (void)hipGetLastError();
    };
    get(&b->seqs, rows), get(&b->glist, rows), get(&b->gstate, rows * ZE_BM_GWORDS), get(&b->brank, rows), get(&b->cand_tok, rows * width);
    get(&b->parent, rows), get(&b->seen_prev, rows), get(&b->bidx, rows * need), get(&b->fin_len, rows), get(&b->fin_is, rows);
    get(&b->fin_order, rows), get(&b->fin_tok, rows * need), get(&b->fin_bidx, rows * need), get(&b->run_score, rows);
    get(&b->cand_score, rows * width), get(&b->fin_score, rows), get(&b->divs, (size_t)need + 1);
    get(&b->u_seqs, rows), get(&b->u_parent, rows);
    if (!ok) {
        ze_beam_free(e);
        return ze_fail(e, ZE_ERR_NOMEM, "beam search: the device allocation of the beam tables failed");
    }
    return ZE_OK;
}

static ze_beam_args beam_args(ze_engine* e, const ze_beam_params* p, int vocab) {
    const ze_beam* b = e->beam;
    ze_beam_args a;
    a.st = e->st_dev, a.seen = e->seen, a.out_tokens = e->out_tokens, a.eos_ids = e->eos_dev;
    a.seqs = b->seqs, a.glist = b->glist;
    a.gstate = b->gstate, a.brank = b->brank, a.cand_tok = b->cand_tok, a.parent = b->parent, a.seen_prev = b->seen_prev, a.bidx = b->bidx;
    a.fin_len = b->fin_len, a.fin_is = b->fin_is, a.fin_order = b->fin_order, a.fin_tok = b->fin_tok, a.fin_bidx = b->fin_bidx;
    a.run_score = b->run_score, a.cand_score = b->cand_score, a.fin_score = b->fin_score, a.divs = b->divs;
    a.B = p->num_beams, a.n_eos = e->cfg.n_eos, a.vocab = vocab, a.seen_stride = e->cfg.vocab, a.max_ctx = e->cfg.max_ctx, a.cap = b->cap;
    a.early = p->early_stopping;
    a.penalty = p->repetition_penalty > 0.f ? p->repetition_penalty : 1.0f;
    a.length_penalty = p->length_penalty;
    return a;
}

// The x-extent of k_beam_reorder, by ze_kv_fork_blocks' reasoning: about 2048 blocks of 256 threads in all and no more, shared by
// the runs of every row of the step (a row that stays leaves at once, so the budget is spent on the rows that move: at most all).
static int reorder_blocks(int runs, int rows, int n_vec) { return ze_kv_fork_blocks(std::max(1, runs * rows), n_vec); }

// the three launches of a step over the n_live groups of glist; gen_rows: the generated K/V rows a moving slot may hold
static void beam_step(ze_engine* e, const ze_beam_args& a, int n_live, const float* logits, int ld, int by_slot, int gen_rows, hipStream_t s) {
    const ze_config& c = e->cfg;
    const int vec = ld % 4 == 0 && reinterpret_cast<uintptr_t>(logits) % 16 == 0;
    k_beam_rows<<<n_live * a.B, 256, 0, s>>>(a, logits, ld, by_slot, vec);
    k_beam_select<<<n_live, 256, 0, s>>>(a);
    const size_t head_stride = (size_t)c.max_ctx * e->head_dim, seq_stride = (size_t)c.kv_heads * head_stride;
    const int ppr = e->head_dim * 2 / 16, runs = c.layers * c.kv_heads * 2;
    const int gx = reorder_blocks(runs + 2, n_live * a.B, std::max(gen_rows * ppr, c.vocab / 16));
    k_beam_reorder<<<dim3(gx, runs + 2, n_live * a.B), 256, 0, s>>>(a, e->kcache, e->vcache, (size_t)c.max_seqs * seq_stride, seq_stride,
                                                                   head_stride, c.kv_heads, runs, ppr, 0, 0);
}

// (the checks themselves are host-only code: ze_index.cpp, where a stand-alone sanitizer build runs them)
static int beam_check_params(ze_engine* e, const int32_t* seqs, int groups, const ze_beam_params* p) {
    if (!e || !seqs || !p) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    const char* why = "";
    const int r = ze_beam_check_impl(seqs, groups, p->num_beams, p->num_return_sequences, p->max_new_tokens, p->early_stopping,
                                     p->length_penalty, p->repetition_penalty, e->cfg.max_seqs, e->cfg.max_ctx, &why);
    return r == 0 ? ZE_OK : ze_fail(e, r, why);
}

// the finished pools of the last call, by rank, to host arrays (any may be NULL); waits for the stream
static int beam_read_finished(ze_engine* e, int groups, int n_ret, int max_new, int32_t* out_tokens, int32_t* out_len, float* out_scores,
                              int32_t* out_bidx, int32_t* out_is, hipStream_t s) {
    const ze_beam* b = e->beam;
    const int B = b->B, n = groups * B, cap = b->cap;
    std::vector<int> len(n), is(n), ord(n), tok((size_t)n * cap), bix((size_t)n * cap);
    std::vector<float> sc(n);
    ZE_HIP(hipMemcpyAsync(len.data(), b->fin_len, n * sizeof(int), hipMemcpyDeviceToHost, s));
    ZE_HIP(hipMemcpyAsync(is.data(), b->fin_is, n * sizeof(int), hipMemcpyDeviceToHost, s));
    ZE_HIP(hipMemcpyAsync(ord.data(), b->fin_order, n * sizeof(int), hipMemcpyDeviceToHost, s));
    ZE_HIP(hipMemcpyAsync(sc.data(), b->fin_score, n * sizeof(float), hipMemcpyDeviceToHost, s));
    ZE_HIP(hipMemcpyAsync(tok.data(), b->fin_tok, (size_t)n * cap * sizeof(int), hipMemcpyDeviceToHost, s));
    ZE_HIP(hipMemcpyAsync(bix.data(), b->fin_bidx, (size_t)n * cap * sizeof(int), hipMemcpyDeviceToHost, s));
    ZE_HIP(hipStreamSynchronize(s));
    for (int g = 0; g < groups; ++g)
        for (int r = 0; r < n_ret; ++r) {
            const int o = g * n_ret + r, en = g * B + ord[g * B + r], m = std::min(len[en], max_new);
            if (out_len) out_len[o] = m;
            if (out_scores) out_scores[o] = sc[en];
            if (out_is) out_is[o] = is[en];
            for (int i = 0; i < max_new; ++i) {
                if (out_tokens) out_tokens[(size_t)o * max_new + i] = i < m ? tok[(size_t)en * cap + i] : e->cfg.pad_token_id;
                // (HF stores the beam index with the batch offset: :3125-3127)
                if (out_bidx) out_bidx[(size_t)o * max_new + i] = i < m ? bix[(size_t)en * cap + i] + g * B : -1;
            }
        }
    return ZE_OK;
}

// divs[n] = float(n ** length_penalty), the divisor HF computes in Python floats (:3048, :3182)
static void upload_divs(ze_engine* e, float length_penalty, int max_new, hipStream_t s) {
    std::vector<float> divs;
    ze_beam_divs_impl(length_penalty, max_new, divs);
    std::vector<int> bits(max_new + 1);
    memcpy(bits.data(), divs.data(), bits.size() * sizeof(float));
    ze_launch_set_ints(reinterpret_cast<int*>(e->beam->divs), bits.data(), max_new + 1, s);
}

// group words of a call: nothing generated, not done, heuristic open, the prompt's rows, the token budget and budget ** length_penalty
static void upload_groups(ze_engine* e, const int32_t* seqs, int groups, const ze_beam_params* p, const std::vector<int>& budget, hipStream_t s) {
    const int B = p->num_beams;
    std::vector<int> gw((size_t)groups * ZE_BM_GWORDS, 0), all(groups);
    for (int g = 0; g < groups; ++g) {
        int* w = &gw[(size_t)g * ZE_BM_GWORDS];
        const float nd = (float)std::pow((double)budget[g], (double)p->length_penalty);
        w[BM_HEUR] = 1, w[BM_PROMPT] = e->ctx_host[seqs[g * B]], w[BM_MAXNEW] = budget[g];
        memcpy(&w[BM_NEVER_DIV], &nd, sizeof(float));
        all[g] = g;
    }
    ze_launch_set_ints(e->beam->seqs, seqs, groups * B, s);
    ze_launch_set_ints(e->beam->glist, all.data(), groups, s);
    ze_launch_set_ints(e->beam->gstate, gw.data(), (int)gw.size(), s);
    e->beam->B = B, e->beam->groups = groups, e->beam->max_new = p->max_new_tokens;
}

extern "C" int ze_op_beam_step(ze_engine* e, const int32_t* seqs, int groups, const ze_beam_params* p, int begin, const float* logits,
                               int vocab, int ld, int32_t* out_parent, int32_t* out_token, float* out_score, int32_t* out_rank,
                               int32_t* out_done, void* stream) {
    ZE_TRY(beam_check_params(e, seqs, groups, p));
    const ze_config& c = e->cfg;
    if (!logits || vocab < 1 || vocab > c.vocab || ld < vocab) return ze_fail(e, ZE_ERR_INVALID, "beam step: logits NULL, vocab outside [1, the engine's] or ld < vocab");
    if (vocab - c.n_eos < p->num_beams) return ze_fail(e, ZE_ERR_INVALID, "beam step: fewer than num_beams non-EOS tokens");
    const int B = p->num_beams, n = groups * B;
    if (!begin && (!e->beam || e->beam->B != B || e->beam->groups != groups || e->beam->max_new != p->max_new_tokens))
        return ze_fail(e, ZE_ERR_INVALID, "beam step: begin = 0 continues the call that began with the same groups, num_beams and max_new_tokens");
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    ZE_TRY(beam_alloc(e, p->max_new_tokens));
    const ze_beam_args a = beam_args(e, p, vocab);
    int gen_rows = 0;
    for (int g = 0; g < groups; ++g) gen_rows = std::max(gen_rows, e->ctx_host[seqs[g * B]]);
    if (begin) {
        upload_groups(e, seqs, groups, p, std::vector<int>(groups, p->max_new_tokens), s);
        upload_divs(e, p->length_penalty, p->max_new_tokens, s);
        k_beam_init<<<groups, 64, 0, s>>>(a);
    }
    beam_step(e, a, groups, logits, ld, 0, gen_rows, s);
    ZE_KCHECK();
    std::vector<int> par(c.max_seqs), rank(n), gw((size_t)groups * ZE_BM_GWORDS);
    std::vector<float> sc(n);
    std::vector<ze_seq_dev> st(c.max_seqs);
    ZE_HIP(hipMemcpyAsync(par.data(), e->beam->parent, c.max_seqs * sizeof(int), hipMemcpyDeviceToHost, s));
    ZE_HIP(hipMemcpyAsync(rank.data(), e->beam->brank, n * sizeof(int), hipMemcpyDeviceToHost, s));
    ZE_HIP(hipMemcpyAsync(gw.data(), e->beam->gstate, gw.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    ZE_HIP(hipMemcpyAsync(sc.data(), e->beam->run_score, n * sizeof(float), hipMemcpyDeviceToHost, s));
    ZE_HIP(hipMemcpyAsync(st.data(), e->st_dev, c.max_seqs * sizeof(ze_seq_dev), hipMemcpyDeviceToHost, s));
    ZE_HIP(hipStreamSynchronize(s));
    for (int g = 0; g < groups; ++g) {
        if (out_done) out_done[g] = gw[(size_t)g * ZE_BM_GWORDS + BM_DONE];
        for (int j = 0; j < B; ++j) {
            const int r = g * B + j;
            int pj = -1;
            for (int k = 0; k < B; ++k)
                if (seqs[g * B + k] == par[seqs[r]]) pj = k;
            if (out_parent) out_parent[r] = pj;
            if (out_token) out_token[r] = st[seqs[r]].token;
            if (out_score) out_score[r] = sc[r];
            if (out_rank) out_rank[r] = rank[r];
        }
    }
    return ZE_OK;
}

extern "C" int ze_op_beam_finished(ze_engine* e, int groups, int32_t* out_tokens, int32_t* out_len, float* out_scores, int32_t* out_beam_indices,
                                   int32_t* out_finished, void* stream) {
    if (!e || !e->beam || e->beam->groups != groups || groups <= 0) return ze_fail(e, ZE_ERR_INVALID, "no beam call of that many groups to read");
    hipSetDevice(e->device);
    return beam_read_finished(e, groups, e->beam->B, e->beam->max_new, out_tokens, out_len, out_scores, out_beam_indices, out_finished,
                              (hipStream_t)stream);
}

extern "C" int ze_op_kv_reorder(ze_engine* e, const int32_t* src_seqs, const int32_t* dst_seqs, int n, int row0, int rows, void* stream) {
    if (!e) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    const ze_config& c = e->cfg;
    {
        const char* why = "";
        const int r = ze_kv_reorder_check_impl(src_seqs, dst_seqs, n, row0, rows, c.max_seqs, c.max_ctx, &why);
        if (r != 0) return ze_fail(e, r, why);
    }
    if (n == 0 || rows == 0) return ZE_OK;
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    ZE_TRY(beam_alloc(e, 1));
    ze_beam_params p{};
    p.num_beams = 1;
    ze_beam_args a = beam_args(e, &p, c.vocab);
    // (tables of its own: a beam call in progress -- ze_op_beam_step with begin = 0 to follow -- keeps its slots and parents)
    a.glist = nullptr, a.seqs = e->beam->u_seqs, a.parent = e->beam->u_parent;
    ze_launch_set_ints(e->beam->u_seqs, dst_seqs, n, s);
    ze_launch_scatter_ints(e->beam->u_parent, dst_seqs, src_seqs, n, s);
    const size_t head_stride = (size_t)c.max_ctx * e->head_dim, seq_stride = (size_t)c.kv_heads * head_stride;
    const int ppr = e->head_dim * 2 / 16, runs = c.layers * c.kv_heads * 2;
    k_beam_reorder<<<dim3(reorder_blocks(runs, n, rows * ppr), runs, n), 256, 0, s>>>(a, e->kcache, e->vcache, (size_t)c.max_seqs * seq_stride,
                                                                                    seq_stride, head_stride, c.kv_heads, runs, ppr, row0, rows);
    ZE_KCHECK();
    for (int i = 0; i < n; ++i) e->logits_fresh[dst_seqs[i]] = 0;
    return ZE_OK;
}

// a per-chain request the beam step does not serve (include/zoomearth.h), by name; null = none
static const char* beam_refused_request(const ze_engine* e, int q) {
    const ze_requests& r = e->req;
    if (r.samp_host[q].penalty > 0.f) return "a sampling request (ze_seq_set_sampling)";
    if (r.filt_host[q].on()) return "a sampling filter";
    if (r.ent_host[q].on()) return "an entropy filter";
    if (r.lp_host[q] >= 0) return "a log-probability request";
    if (r.la_host[q].on()) return "a logit adjustment";
    if (r.tr_host[q].on()) return "token rules";
    if (r.gr_host[q] >= 0) return "a grammar";
    if (e->spec.on(q)) return "speculation";
    return nullptr;
}

extern "C" int ze_beam_search(ze_engine* e, const int32_t* seqs, int groups, const ze_beam_params* p, int32_t* out_tokens, int32_t* out_len,
                              float* out_scores, int32_t* out_beam_indices, void* stream) {
    ZE_TRY(beam_check_params(e, seqs, groups, p));
    if (!out_tokens || !out_len) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    const ze_config& c = e->cfg;
    const int B = p->num_beams, n = groups * B;
    if (c.vocab - c.n_eos < B) return ze_fail(e, ZE_ERR_INVALID, "beam search: fewer than num_beams non-EOS tokens");
    if (n > 64 && !e->wide_regime())
        return ze_fail(e, ZE_ERR_INVALID, "beam search: more than 64 rows in a step of an engine pinned to the fragment kernels (ze_set_decode_regime)");
    std::vector<int> budget(groups);
    for (int i = 0; i < n; ++i) {
        const char* what = beam_refused_request(e, seqs[i]);
        if (what) return ze_fail(e, ZE_ERR_INVALID, std::string("beam search: a slot of the call has ") + what + ", which a beam step does not serve");
    }
    for (int g = 0; g < groups; ++g) {
        const int src = seqs[g * B];
        if (e->ctx_host[src] <= 0) return ze_fail(e, ZE_ERR_INVALID, "beam search: the first slot of a group holds no prefilled prompt");
        if (!e->logits_fresh[src])
            return ze_fail(e, ZE_ERR_INVALID, "beam search: the first slot of a group drew, stepped or changed since its prefill (the ze_seq_fork source contract)");
        if (e->ctx_host[src] >= c.max_ctx) return ze_fail(e, ZE_ERR_NOMEM, "beam search: the prompt fills max_ctx");
        if (B - 1 > e->prefill_rows) return ze_fail(e, ZE_ERR_NOMEM, "more destinations than the id buffer holds");
        // token t is fed back as cache row prompt + t - 1: a group stops where max_ctx does
        budget[g] = std::min(p->max_new_tokens, c.max_ctx - e->ctx_host[src]);
    }
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    ZE_TRY(ensure_fragments(e, s));
    ZE_TRY(beam_alloc(e, p->max_new_tokens));
    // (the one step of ze_seq_fork that can fail behind its checks, done for every destination before the first fork)
    for (int g = 0; g < groups; ++g)
        for (int j = 1; j < B; ++j)
            if (!e->pfx_copy_ev[seqs[g * B + j]]) ZE_HIP(hipEventCreateWithFlags(&e->pfx_copy_ev[seqs[g * B + j]], hipEventDisableTiming));
    // ---- nothing was enqueued or changed up to here
    for (int g = 0; g < groups && B > 1; ++g) ZE_TRY(ze_seq_fork(e, seqs[g * B], seqs + g * B + 1, B - 1, stream));
    const ze_beam_args a = beam_args(e, p, c.vocab);
    upload_groups(e, seqs, groups, p, budget, s);
    upload_divs(e, p->length_penalty, p->max_new_tokens, s);
    k_beam_init<<<groups, 64, 0, s>>>(a);
    // step 0 ranks the logits rows the prefill (and the fork) left per slot; no cache row is generated yet
    for (int i = 0; i < n; ++i) e->logits_fresh[seqs[i]] = 0;
    beam_step(e, a, groups, e->dlogits, c.vocab, 1, 0, s);
    ZE_KCHECK();
    std::vector<int> live(groups), gw((size_t)groups * ZE_BM_GWORDS);
    std::vector<char> done(groups, 0);
    for (int g = 0; g < groups; ++g) live[g] = g;
    const int sync_every = std::max(1, p->sync_every);
    const int td = ze_timer_begin(e, 3, s);
    const int ran = [&]() -> int {
    for (int t = 1; t < p->max_new_tokens; ++t) {
        // a group whose budget is spent is done on the device too (the last step's stop); the others' done words are read every
        // sync_every steps
        if (t % sync_every == 0) {
            ZE_HIP(hipMemcpyAsync(gw.data(), e->beam->gstate, gw.size() * sizeof(int), hipMemcpyDeviceToHost, s));
            ZE_HIP(hipStreamSynchronize(s));
            for (int g = 0; g < groups; ++g) done[g] = done[g] || gw[(size_t)g * ZE_BM_GWORDS + BM_DONE];
        }
        std::vector<int> still;
        ze_beam_live_impl(live, done, budget, t, still);
        if (still.size() != live.size() && !still.empty()) ze_launch_set_ints(e->beam->glist, still.data(), (int)still.size(), s);
        live.swap(still);
        if (live.empty()) break;
        std::vector<int> rows;
        for (int g : live) rows.insert(rows.end(), seqs + g * B, seqs + (g + 1) * B);
        ZE_TRY(ze_beam_forward(e, rows.data(), (int)rows.size(), p->use_graph, s));
        beam_step(e, a, (int)live.size(), e->blogits, c.vocab, 0, t, s);
        ZE_KCHECK();
    }
    return ZE_OK;
    }();
    ze_timer_end(e, td, s);   // (also behind a step that failed)
    ZE_TRY(ran);
    return beam_read_finished(e, groups, p->num_return_sequences, p->max_new_tokens, out_tokens, out_len, out_scores, out_beam_indices, nullptr, s);
}

// Measurement entry (tools/bench_beam_search.py): HIP-event time per launch of ONE beam kernel -- which = 0 k_beam_rows, 1
// k_beam_select, 2 k_beam_reorder -- on `groups` groups of B beams in slots 0 .. groups * B - 1, logits device f32 [groups * B, vocab].
// The reorder is timed at its widest: every slot but a group's first takes the first one's `gen_rows` generated rows.  The slots'
// chain states are overwritten: an engine used for this serves nothing else.
extern "C" int ze_profile_beam_kernel(ze_engine* e, int which, int groups, int B, int gen_rows, const float* logits, int iters, float* out_us,
                                      void* stream) {
    if (!e || !logits || !out_us || which < 0 || which > 2 || iters < 1 || gen_rows < 0) return ze_fail(e, ZE_ERR_INVALID, "bad profile arguments");
    const ze_config& c = e->cfg;
    ze_beam_params p{};
    p.num_beams = B, p.num_return_sequences = 1, p.max_new_tokens = std::min(c.max_ctx, iters + 8), p.length_penalty = 1.0f, p.early_stopping = 2;
    p.repetition_penalty = 1.0f;
    std::vector<int> seqs(std::max(0, groups * B));
    for (size_t i = 0; i < seqs.size(); ++i) seqs[i] = (int)i;
    ZE_TRY(beam_check_params(e, seqs.data(), groups, &p));
    if (gen_rows + 1 > c.max_ctx || c.vocab - c.n_eos < B) return ze_fail(e, ZE_ERR_INVALID, "profile: rows or beams out of range");
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    ZE_TRY(beam_alloc(e, p.max_new_tokens));
    const ze_beam_args a = beam_args(e, &p, c.vocab);
    const int n = groups * B;
    for (int q : seqs) e->ctx_host[q] = 0, e->logits_fresh[q] = 0;
    upload_groups(e, seqs.data(), groups, &p, std::vector<int>(groups, p.max_new_tokens), s);
    upload_divs(e, p.length_penalty, p.max_new_tokens, s);
    k_beam_init<<<groups, 64, 0, s>>>(a);
    const int vec = c.vocab % 4 == 0 && reinterpret_cast<uintptr_t>(logits) % 16 == 0;
    k_beam_rows<<<n, 256, 0, s>>>(a, logits, c.vocab, 0, vec);
    const size_t head_stride = (size_t)c.max_ctx * e->head_dim, seq_stride = (size_t)c.kv_heads * head_stride;
    const int ppr = e->head_dim * 2 / 16, runs = c.layers * c.kv_heads * 2;
    const int gx = reorder_blocks(runs + 2, n, std::max(gen_rows * ppr, c.vocab / 16));
    hipEvent_t t0, t1;
    ZE_HIP(hipEventCreate(&t0));
    ZE_HIP(hipEventCreate(&t1));
    auto launch = [&]() {
        if (which == 0) k_beam_rows<<<n, 256, 0, s>>>(a, logits, c.vocab, 0, vec);
        if (which == 1) k_beam_select<<<groups, 256, 0, s>>>(a);
        if (which == 2)
            k_beam_reorder<<<dim3(gx, runs + 2, n), 256, 0, s>>>(a, e->kcache, e->vcache, (size_t)c.max_seqs * seq_stride, seq_stride, head_stride,
                                                                c.kv_heads, runs, ppr, 0, 0);
    };
    if (which == 2) {   // one select for the tokens and the step count, then the widest parent table and the rows to move
        k_beam_select<<<groups, 256, 0, s>>>(a);
        std::vector<int> par(n);
        for (int i = 0; i < n; ++i) {
            par[i] = i / B * B;
            ze_launch_set_ints(&(e->st_dev + i)->ctx, &gen_rows, 1, s);
        }
        ze_launch_set_ints(e->beam->parent, par.data(), n, s);   // (slots 0 .. n - 1: the table by slot is the table by row)
    }
    launch();
    ZE_HIP(hipEventRecord(t0, s));
    for (int i = 0; i < iters; ++i) launch();
    ZE_HIP(hipEventRecord(t1, s));
    ZE_HIP(hipEventSynchronize(t1));
    float ms = 0.f;
    ZE_HIP(hipEventElapsedTime(&ms, t0, t1));
    hipEventDestroy(t0);
    hipEventDestroy(t1);
    ZE_KCHECK();
    *out_us = ms * 1000.f / iters;
    return ZE_OK;
}

// Top-k / top-p / min-p sampling filters (HF:generation/logits_process.py TopKLogitsWarper, TopPLogitsWarper,
// MinPLogitsWarper, in the order of HF:generation/utils.py:_get_logits_processor: temperature -> top-k -> top-p -> min-p).
// Each of the three keeps "everything at or above a value", so the filter of a chain is ONE fp32 cut per step:
// token i survives iff z_i >= cut, z_i = score_i / T (score = repetition-penalised fp32 logit, the value the draw uses).
// k_sample_filter finds that cut; the draw (ze_sample.hip) treats z_i < cut as e_i = 0 and keeps its summation order.
//
// Definitions (restated in tests/sampling_filters_ref.py):
//   key(z)  order-preserving 32-bit integer of z (-0 counts as +0, NaN sorts below -inf)
//   e_i     = expf(z_i - z_max)  (fp32; not finite or negative -> 0)
//   w_i     = (uint64) rintf(e_i * 2^40): the MASS of a token, integer fixed point.  e_i * 2^40 is exact in fp32, the
//             sum of 151,936 such values stays below 2^58, and integer adds commute -- whatever order the atomics land in
//   top-k   key_k = key of the k-th largest z (k < vocab; ties at that value all survive); M = sum of w over key >= key_k
//   top-p   target = ceil((double)top_p * (double)M); token i survives iff  sum of w_j over key_j > key_i  <  target
//           (equal scores live or die together; the arg-max has nothing above it and always survives)
//   min-p   e_i >= min_p  (fp32 compare; the ratio to the top probability needs no normalisation)
//   cut     = smallest z among the survivors of all three, kept = their number
//
// One workgroup of 1024 threads per chain (grid.x = chain): the cut is a function of the chain's own row -- no partials
// shared between workgroups, no floating-point atomics, nothing that depends on the grid.  Radix select on key(z) in
// 11 + 11 + 10 bits with LDS histograms of (count u32, mass u64) filled by LDS integer atomics:
//   pass 0  z_max                      pass 1  level-1 histogram of the whole row (kept for both selects)
//   top-k   level 1 from pass 1, two more passes that touch only the tokens under the chosen prefix
//   top-p   level 1 from pass 1 again (buckets below key_k's dropped, its own bucket cut to what survives), two more passes
//   last    survivors' count and minimum (min-p applied here)
// A select that is off costs no pass; a chain without any filter writes cut = -inf and leaves.
#include "ze_kernels.h"
#include "ze_sample_select.h"
#include <cstring>

__global__ void __launch_bounds__(FILT_THREADS) k_sample_filter(const float* __restrict__ logits, int vocab, int ld,
                                                                const uint8_t* __restrict__ seen_base,
                                                                const int* __restrict__ seq_ids, int slot0, float penalty,
                                                                float temperature, const float4* __restrict__ filt,
                                                                float* __restrict__ out_cut, int* __restrict__ out_kept,
                                                                const ze_chain_sampling* __restrict__ samp) {
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63;
    const int slot = seq_ids ? seq_ids[b] : slot0 + b;
    const float4 fp = filt[slot];
    int top_k = __float_as_int(fp.x);
    const float top_p = fp.y, min_p = fp.z;
    if (fp.w > 0.f) temperature = fp.w;  // the unit op: a temperature per row
    if (samp) {  // per-chain sampling requests (ze_seq_set_sampling): the slot's own temperature and penalty; uniform per workgroup
        const ze_chain_sampling r = samp[slot];
        if (r.penalty > 0.f) temperature = r.temperature, penalty = r.penalty;
    }
    const bool greedy = !(temperature > 0.f);  // (only a per-chain row: the scalar launch exists for sampled steps alone)
    if (top_k >= vocab) top_k = 0;
    const bool has_k = top_k > 0, has_p = top_p < 1.0f, has_m = min_p > 0.f;
    if (greedy || (!has_k && !has_p && !has_m)) {
        if (t == 0) {
            out_cut[b] = -INFINITY;
            if (out_kept) out_kept[b] = vocab;
        }
        return;
    }
    const float* lg = logits + (size_t)b * ld;
    const uint8_t* seen = seen_base ? seen_base + (seq_ids ? (size_t)slot * vocab : 0) : nullptr;
    const bool vec = (vocab & 3) == 0 && (reinterpret_cast<uintptr_t>(lg) & 15) == 0 &&
                     (!seen || (reinterpret_cast<uintptr_t>(seen) & 3) == 0);

    __shared__ unsigned h1c[FILT_BUCKETS], h2c[FILT_BUCKETS];
    __shared__ unsigned long long h1m[FILT_BUCKETS], h2m[FILT_BUCKETS];
    __shared__ unsigned sWc[FILT_THREADS / 64];
    __shared__ unsigned long long sWm[FILT_THREADS / 64];
    __shared__ filt_sel sel;
    __shared__ unsigned sKeyMax, sKeyMin, sKept;

    for (int i = t; i < FILT_BUCKETS; i += FILT_THREADS) h1c[i] = 0u, h1m[i] = 0ull;
    if (t == 0) sKeyMax = 0u, sKeyMin = 0xffffffffu, sKept = 0u;
    __syncthreads();

    // pass 0: z_max (through the key: an integer maximum)
    {
        unsigned km = 0u;
        filt_foreach(lg, seen, penalty, temperature, vocab, vec, [&](int, float z) { km = max(km, filt_key(z)); });
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) km = max(km, (unsigned)__shfl_xor((int)km, off, 64));
        if (lane == 0) atomicMax(&sKeyMax, km);
    }
    __syncthreads();
    const float zmax = filt_unkey(sKeyMax);

    unsigned key_cut = 0u;  // survivors of top-k and top-p: key >= key_cut
    if (has_k || has_p) {
        // pass 1: the whole row by the top 11 bits
        filt_foreach(lg, seen, penalty, temperature, vocab, vec, [&](int, float z) {
            const unsigned k = filt_key(z);
            atomicAdd(&h1c[k >> 21], 1u);
            const unsigned long long w = filt_mass(filt_e(z, zmax));
            if (w) atomicAdd(&h1m[k >> 21], w);
        });
        __syncthreads();
        int floor_b = -1;
        unsigned floor_cnt = 0u;
        unsigned long long floor_mass = 0ull, m_surv = 0ull;
        for (int which = 0; which < 2; ++which) {  // 0: top-k (by count), 1: top-p (by mass, over the survivors of top-k)
            if (which == 0 ? !has_k : !has_p) continue;
            const bool by_mass = which == 1;
            unsigned long long target;
            if (!by_mass) {
                target = (unsigned long long)top_k;
            } else {
                if (!has_k) {  // total mass of the row
                    filt_scan(h1c, h1m, true, ~0ull, -1, 0u, 0ull, sWc, sWm, &sel);
                    m_surv = sel.mass_total;
                    __syncthreads();
                }
                target = (unsigned long long)ceil((double)top_p * (double)m_surv);
            }
            filt_scan(h1c, h1m, by_mass, target, floor_b, floor_cnt, floor_mass, sWc, sWm, &sel);
            if (!sel.found) {
                __syncthreads();
                continue;  // nothing crosses (an all -inf row): this select keeps everything it was given
            }
            unsigned prefix = (unsigned)sel.bucket;
            unsigned long long above_w = by_mass ? sel.mass_above : (unsigned long long)sel.cnt_above;
            unsigned long long above_m = sel.mass_above;
            unsigned above_c = sel.cnt_above;
            const unsigned l1_c = sel.cnt_above;  // what lies above the level-1 bucket
            const unsigned long long l1_m = sel.mass_above;
            __syncthreads();
            const unsigned key_floor = key_cut;
#pragma unroll 1
            for (int level = 1; level < 3; ++level) {  // 11 more bits, then the last 10
                const int shift = level == 1 ? 10 : 0, pshift = level == 1 ? 21 : 10;
                const unsigned mask = level == 1 ? 0x7ffu : 0x3ffu;
                for (int i = t; i < FILT_BUCKETS; i += FILT_THREADS) h2c[i] = 0u, h2m[i] = 0ull;
                __syncthreads();
                filt_foreach(lg, seen, penalty, temperature, vocab, vec, [&](int, float z) {
                    const unsigned k = filt_key(z);
                    if ((k >> pshift) == prefix && k >= key_floor) {
                        atomicAdd(&h2c[(k >> shift) & mask], 1u);
                        const unsigned long long w = filt_mass(filt_e(z, zmax));
                        if (w) atomicAdd(&h2m[(k >> shift) & mask], w);
                    }
                });
                __syncthreads();
                filt_scan(h2c, h2m, by_mass, target - above_w, -1, 0u, 0ull, sWc, sWm, &sel);
                // (the crossing is inside the prefix by construction; `found` can only fail on an empty histogram)
                const int bk = sel.found ? sel.bucket : 0;
                prefix = (prefix << (level == 1 ? 11 : 10)) | (unsigned)bk;
                above_w += by_mass ? sel.mass_above : (unsigned long long)sel.cnt_above;
                above_m += sel.mass_above;
                above_c += sel.cnt_above;
                if (level == 2) {
                    above_m += sel.mass_in;  // tokens AT the cut survive, ties and all
                    above_c += sel.cnt_in;
                }
                __syncthreads();
            }
            key_cut = prefix;
            if (!by_mass) {  // what top-p starts from: the survivors' mass, and the level-1 histogram cut at key_k
                m_surv = above_m;
                floor_b = (int)(key_cut >> 21);
                floor_cnt = above_c - l1_c;
                floor_mass = above_m - l1_m;
            }
        }
    }

    // last pass: the survivors (min-p joins here)
    {
        unsigned cnt = 0u, kmin = 0xffffffffu;
        filt_foreach(lg, seen, penalty, temperature, vocab, vec, [&](int, float z) {
            const unsigned k = filt_key(z);
            if (k >= key_cut && (!has_m || filt_e(z, zmax) >= min_p)) {
                cnt += 1u;
                kmin = min(kmin, k);
            }
        });
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            cnt += (unsigned)__shfl_xor((int)cnt, off, 64);
            kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, off, 64));
        }
        if (lane == 0) {
            atomicAdd(&sKept, cnt);
            atomicMin(&sKeyMin, kmin);
        }
    }
    __syncthreads();
    if (t == 0) {
        // (no survivor at all -- a row of NaN: no cut)
        out_cut[b] = sKept ? filt_unkey(sKeyMin) : -INFINITY;
        if (out_kept) out_kept[b] = sKept ? (int)sKept : vocab;
    }
}

void ze_launch_sample_filter(const float* logits, int vocab, int ld, const uint8_t* seen_base, const int* seq_ids, int slot0,
                             int n, float penalty, float temperature, const float* filt, float* out_cut, int* out_kept,
                             const ze_chain_sampling* samp, hipStream_t s) {
    if (n <= 0) return;
    k_sample_filter<<<n, FILT_THREADS, 0, s>>>(logits, vocab, ld, seen_base, seq_ids, slot0, penalty, temperature,
                                               reinterpret_cast<const float4*>(filt), out_cut, out_kept, samp);
}

// filt[slot] = (top_k bits, top_p, min_p, temperature of the row or 0): the values travel as kernel arguments
__global__ void k_set_filter(float4* filt, int slot, float4 v) { filt[slot] = v; }
void ze_launch_set_filter(float* filt, int slot, int top_k, float top_p, float min_p, float temperature, hipStream_t s) {
    float kbits;
    std::memcpy(&kbits, &top_k, sizeof(kbits));
    k_set_filter<<<1, 1, 0, s>>>(reinterpret_cast<float4*>(filt), slot, make_float4(kbits, top_p, min_p, temperature));
}

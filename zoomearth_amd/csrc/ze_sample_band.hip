// Typical-p / epsilon / eta sampling cutoffs (HF:generation/logits_process.py TypicalLogitsWarper, EpsilonLogitsWarper,
// EtaLogitsWarper, each with min_tokens_to_keep = 1, in the order of HF:generation/utils.py:_get_logits_processor: ... -> min-p ->
// typical -> epsilon -> eta).  After a softmax -log p_i - H is monotone in z_i, so the typical set is an INTERVAL of z, and epsilon
// and eta are thresholds on p_i: with the cut of ze_sample_filter.hip the whole warper chain of a chain is one fp32 BAND
// [cut, ceil] per step.  k_sample_band runs after k_sample_filter, reads its cut (or starts from -inf) and writes the band; the
// draw (ze_sample.hip, the _band kernels) treats z_i < cut or z_i > ceil as e_i = 0 and keeps its summation order.
//
// Definitions (include/zoomearth.h; restated in tests/entropy_filters_ref.py), with z, e, w and key() of ze_sample_filter.hip:
//   S        the survivors so far: key(z_i) in [key(cut), key(top)], top = the largest surviving z (the row maximum at first)
//   u_i      = (uint64) rintf(e_i * (z_max - z_i) * 2^40), 0 where e_i is 0
//   H(S)     = log(M * 2^-40) + U / M  in float64 from the two integers M = sum w, U = sum u over S: a function of the row alone
//   typical  s_i = |((z_max - z_i) + lm) - Hf| in fp32, lm = fp32(log(M * 2^-40)), Hf = fp32(H); target = ceil((double)typical_p *
//            (double)M); token i survives iff  sum of w_j over s_j < s_i  <  target (equal s live or die together).  Every fp32
//            step of s is monotone in z, so the survivors are the tokens of S with z in [lo, hi], their smallest and largest z
//   epsilon  over the band's survivors, mass M2: keep w_i >= ceil((double)eps * (double)M2), and the largest-z survivor
//   eta      H3, M3 over what epsilon left: thr = min(eta, sqrt(eta) * exp(-H3)) in float64; keep w_i >= ceil(thr * (double)M3),
//            and the largest-z survivor
//   cut      = smallest surviving z, ceil = hi when typical ran (+inf otherwise), kept = the survivors' number
//
// One workgroup of 1024 threads per chain (grid.x = chain), nothing shared between workgroups, no floating-point atomics.  Passes
// over the row (each stage that is off costs none; a chain without any of the three leaves at once):
//   always   z_max; the survey of S (count, M, U)
//   typical  radix select on ~key(s) in 11 + 11 + 10 bits by mass (LDS histograms of (count u32, mass u64), LDS integer atomics;
//            the last two passes touch only the tokens under the chosen prefix); the survey of the band
//   epsilon  one survey          eta  one survey
#include "ze_kernels.h"
#include "ze_sample_select.h"

struct band_acc {
    unsigned cnt, kmin, kmax, pad;
    unsigned long long m, u;
};

__device__ __forceinline__ unsigned long long band_wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, off, 64), hi = __shfl_xor((unsigned)(v >> 32), off, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

__device__ __forceinline__ unsigned long long band_u(float e, float d) {
    return e > 0.f ? (unsigned long long)rintf(e * d * 1099511627776.0f) : 0ull;
}

// the tokens with key(z) in [klo, ktop] that pred(key, z, w) accepts: count, smallest and largest key, M and U (integer sums: exact
// in any order)
template <class P>
__device__ __forceinline__ band_acc band_survey(const float* __restrict__ lg, const uint8_t* __restrict__ seen, float penalty,
                                                float temperature, int vocab, bool vec, float zmax, unsigned klo, unsigned ktop,
                                                band_acc* acc, P pred) {
    if (threadIdx.x == 0) *acc = band_acc{0u, 0xffffffffu, 0u, 0u, 0ull, 0ull};
    __syncthreads();
    unsigned cnt = 0u, kmin = 0xffffffffu, kmax = 0u;
    unsigned long long m = 0ull, u = 0ull;
    filt_foreach(lg, seen, penalty, temperature, vocab, vec, [&](int, float z) {
        const unsigned k = filt_key(z);
        if (k < klo || k > ktop) return;
        const float e = filt_e(z, zmax);
        const unsigned long long w = filt_mass(e);
        if (!pred(k, z, w)) return;
        cnt += 1u;
        kmin = min(kmin, k);
        kmax = max(kmax, k);
        m += w;
        u += band_u(e, zmax - z);
    });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cnt += (unsigned)__shfl_xor((int)cnt, off, 64);
        kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, off, 64));
        kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, off, 64));
    }
    m = band_wave_sum(m);
    u = band_wave_sum(u);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&acc->cnt, cnt);
        atomicMin(&acc->kmin, kmin);
        atomicMax(&acc->kmax, kmax);
        atomicAdd(&acc->m, m);
        atomicAdd(&acc->u, u);
    }
    __syncthreads();
    const band_acc r = *acc;
    __syncthreads();
    return r;
}

__device__ __forceinline__ double band_entropy(unsigned long long m, unsigned long long u) {
    return log((double)m * 9.094947017729282e-13) + (double)u / (double)m;  // 2^-40
}

__global__ void __launch_bounds__(FILT_THREADS) k_sample_band(const float* __restrict__ logits, int vocab, int ld,
                                                              const uint8_t* __restrict__ seen_base,
                                                              const int* __restrict__ seq_ids, int slot0, float penalty,
                                                              float temperature, const float4* __restrict__ ent,
                                                              const float* in_cut, float* out_cut, float* __restrict__ out_ceil,
                                                              int* __restrict__ out_kept,
                                                              const ze_chain_sampling* __restrict__ samp) {
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63;
    const int slot = seq_ids ? seq_ids[b] : slot0 + b;
    const float4 ep = ent[slot];
    const float typ = ep.x, eps = ep.y, eta = ep.z;
    if (ep.w > 0.f) temperature = ep.w;  // the unit op: a temperature per row
    if (samp) {  // per-chain sampling requests (ze_seq_set_sampling): the slot's own temperature and penalty; uniform per workgroup
        const ze_chain_sampling r = samp[slot];
        if (r.penalty > 0.f) temperature = r.temperature, penalty = r.penalty;
    }
    const bool greedy = !(temperature > 0.f);
    const bool has_t = typ > 0.f && typ < 1.f, has_e = eps > 0.f && eps < 1.f, has_h = eta > 0.f && eta < 1.f;
    const float cut0 = in_cut ? in_cut[b] : -INFINITY;  // (in_cut may be out_cut: read by every thread before thread 0 writes)
    if (greedy || (!has_t && !has_e && !has_h)) {
        if (t == 0) {
            out_cut[b] = cut0;
            out_ceil[b] = INFINITY;
            if (out_kept && !in_cut) out_kept[b] = vocab;
        }
        return;
    }
    const float* lg = logits + (size_t)b * ld;
    const uint8_t* seen = seen_base ? seen_base + (seq_ids ? (size_t)slot * vocab : 0) : nullptr;
    const bool vec = (vocab & 3) == 0 && (reinterpret_cast<uintptr_t>(lg) & 15) == 0 &&
                     (!seen || (reinterpret_cast<uintptr_t>(seen) & 3) == 0);

    __shared__ unsigned hc[FILT_BUCKETS];
    __shared__ unsigned long long hm[FILT_BUCKETS];
    __shared__ unsigned sWc[FILT_THREADS / 64];
    __shared__ unsigned long long sWm[FILT_THREADS / 64];
    __shared__ filt_sel sel;
    __shared__ band_acc acc;
    __shared__ unsigned sKeyMax;

    if (t == 0) sKeyMax = 0u;
    __syncthreads();
    // z_max of the row (through the key: an integer maximum)
    {
        unsigned km = 0u;
        filt_foreach(lg, seen, penalty, temperature, vocab, vec, [&](int, float z) { km = max(km, filt_key(z)); });
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) km = max(km, (unsigned)__shfl_xor((int)km, off, 64));
        if (lane == 0) atomicMax(&sKeyMax, km);
    }
    __syncthreads();
    const float zmax = filt_unkey(sKeyMax);

    unsigned klo = filt_key(cut0), ktop = sKeyMax;  // (a NaN score has key 0, below key(-inf): never a survivor)
    if (klo < 0x007fffffu) klo = 0x007fffffu;
    const auto all = [](unsigned, float, unsigned long long) { return true; };
    band_acc S = band_survey(lg, seen, penalty, temperature, vocab, vec, zmax, klo, ktop, &acc, all);
    bool ceiling = false;
    if (S.m == 0ull) {  // no mass at all (a row without a finite score): no band
        if (t == 0) {
            out_cut[b] = cut0;
            out_ceil[b] = INFINITY;
            if (out_kept) out_kept[b] = S.cnt ? (int)S.cnt : vocab;
        }
        return;
    }

    if (has_t) {
        const double lmd = log((double)S.m * 9.094947017729282e-13);
        const float lm = (float)lmd, Hf = (float)(lmd + (double)S.u / (double)S.m);
        const auto skey = [=](float z) { return ~filt_key(fabsf(((zmax - z) + lm) - Hf)); };  // larger = more typical
        const unsigned long long target = (unsigned long long)ceil((double)typ * (double)S.m);
        unsigned prefix = 0u;
        unsigned long long above = 0ull;
        bool found = true;
#pragma unroll 1
        for (int level = 0; level < 3 && found; ++level) {  // 11 + 11 + 10 bits
            const int shift = level == 0 ? 21 : level == 1 ? 10 : 0, pshift = level == 1 ? 21 : 10;
            const unsigned mask = level == 2 ? 0x3ffu : 0x7ffu;
            for (int i = t; i < FILT_BUCKETS; i += FILT_THREADS) hc[i] = 0u, hm[i] = 0ull;
            __syncthreads();
            filt_foreach(lg, seen, penalty, temperature, vocab, vec, [&](int, float z) {
                const unsigned k = filt_key(z);
                if (k < klo || k > ktop) return;
                const unsigned sk = skey(z);
                if (level > 0 && (sk >> pshift) != prefix) return;
                atomicAdd(&hc[(sk >> shift) & mask], 1u);
                const unsigned long long w = filt_mass(filt_e(z, zmax));
                if (w) atomicAdd(&hm[(sk >> shift) & mask], w);
            });
            __syncthreads();
            filt_scan(hc, hm, true, target - above, -1, 0u, 0ull, sWc, sWm, &sel);
            found = sel.found != 0;  // (1 <= target <= M: the crossing exists, and lies under the prefix by construction)
            prefix = (prefix << (level == 2 ? 10 : 11)) | (unsigned)(found ? sel.bucket : 0);
            above += sel.mass_above;
            __syncthreads();
        }
        if (found) {
            const unsigned scut = prefix;
            S = band_survey(lg, seen, penalty, temperature, vocab, vec, zmax, klo, ktop, &acc,
                            [=](unsigned, float z, unsigned long long) { return skey(z) >= scut; });
            klo = S.kmin, ktop = S.kmax;
            ceiling = true;
        }
    }
    if (has_e) {
        const unsigned long long thr = (unsigned long long)ceil((double)eps * (double)S.m);
        const unsigned top = ktop;
        S = band_survey(lg, seen, penalty, temperature, vocab, vec, zmax, klo, ktop, &acc,
                        [=](unsigned k, float, unsigned long long w) { return w >= thr || k == top; });
        klo = S.kmin;
    }
    if (has_h) {
        const double thr_p = fmin((double)eta, sqrt((double)eta) * exp(-band_entropy(S.m, S.u)));
        const unsigned long long thr = (unsigned long long)ceil(thr_p * (double)S.m);
        const unsigned top = ktop;
        S = band_survey(lg, seen, penalty, temperature, vocab, vec, zmax, klo, ktop, &acc,
                        [=](unsigned k, float, unsigned long long w) { return w >= thr || k == top; });
        klo = S.kmin;
    }
    if (t == 0) {
        out_cut[b] = filt_unkey(klo);
        out_ceil[b] = ceiling ? filt_unkey(ktop) : INFINITY;
        if (out_kept) out_kept[b] = (int)S.cnt;
    }
}

void ze_launch_sample_band(const float* logits, int vocab, int ld, const uint8_t* seen_base, const int* seq_ids, int slot0, int n,
                           float penalty, float temperature, const float* ent, const float* in_cut, float* out_cut, float* out_ceil,
                           int* out_kept, const ze_chain_sampling* samp, hipStream_t s) {
    if (n <= 0) return;
    k_sample_band<<<n, FILT_THREADS, 0, s>>>(logits, vocab, ld, seen_base, seq_ids, slot0, penalty, temperature,
                                             reinterpret_cast<const float4*>(ent), in_cut, out_cut, out_ceil, out_kept, samp);
}

// ent[slot] = (typical_p, epsilon_cutoff, eta_cutoff, temperature of the row or 0): the values travel as kernel arguments
__global__ void k_set_entropy_filter(float4* ent, int slot, float4 v) { ent[slot] = v; }
void ze_launch_set_entropy_filter(float* ent, int slot, float typical_p, float epsilon_cutoff, float eta_cutoff, float temperature,
                                  hipStream_t s) {
    k_set_entropy_filter<<<1, 1, 0, s>>>(reinterpret_cast<float4*>(ent), slot, make_float4(typical_p, epsilon_cutoff, eta_cutoff, temperature));
}

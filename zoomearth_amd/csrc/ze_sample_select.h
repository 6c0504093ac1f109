// What the selection kernels of the sampling filters share (ze_sample_filter.hip: the cut of top-k / top-p / min-p;
// ze_sample_band.hip: the band of typical / epsilon / eta): the order-preserving key of a score, the integer mass of a token, the
// walk over a chain's row as the draw reads it, and the scan of a 2048-bucket LDS histogram of (count, mass) for the bucket where
// a running weight crosses a target.  One workgroup of FILT_THREADS threads per chain.
#pragma once
#include "ze_kernels.h"

#define FILT_THREADS 1024
#define FILT_BUCKETS 2048

__device__ __forceinline__ unsigned filt_key(float z) {
    if (!(z == z)) return 0u;
    const unsigned u = __float_as_uint(z + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float filt_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ float filt_e(float z, float zmax) {
    const float e = expf(z - zmax);
    return (e >= 0.f && e <= 1.f) ? e : 0.f;
}
__device__ __forceinline__ unsigned long long filt_mass(float e) { return (unsigned long long)rintf(e * 1099511627776.0f); }

// f(i, z) for every token of the row, z = score / T as the draw computes it; 16-byte loads when the row allows
template <class F>
__device__ __forceinline__ void filt_foreach(const float* __restrict__ lg, const uint8_t* __restrict__ seen, float penalty,
                                             float temperature, int vocab, bool vec, F f) {
    const bool pen = seen != nullptr && penalty != 1.0f;
    if (vec) {
        const int n4 = vocab >> 2;
#pragma unroll 2
        for (int g = threadIdx.x; g < n4; g += FILT_THREADS) {
            const float4 q = reinterpret_cast<const float4*>(lg)[g];
            const unsigned sn = pen ? reinterpret_cast<const unsigned*>(seen)[g] : 0u;
            float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float x = v[j];
                if ((sn >> (8 * j)) & 0xffu) x = x < 0.f ? x * penalty : x / penalty;
                f(4 * g + j, x / temperature);
            }
        }
    } else {
#pragma unroll 4
        for (int i = threadIdx.x; i < vocab; i += FILT_THREADS) {
            float x = lg[i];
            if (pen && seen[i]) x = x < 0.f ? x * penalty : x / penalty;
            f(i, x / temperature);
        }
    }
}

struct filt_sel {
    int found, bucket;
    unsigned cnt_above, cnt_in;
    unsigned long long mass_above, mass_in, mass_total;
};

// Walks the FILT_BUCKETS buckets from the top and finds the one where the running weight crosses `target`:
// above < target <= above + in (weight = count, or mass when by_mass).  Buckets below `floor_b` count as empty and bucket
// floor_b carries floor_mass / floor_cnt instead of its own (floor_b < 0: none).  Integer prefix sums: exact in any order.
static __device__ void filt_scan(const unsigned* __restrict__ hc, const unsigned long long* __restrict__ hm, bool by_mass,
                          unsigned long long target, int floor_b, unsigned floor_cnt, unsigned long long floor_mass,
                          unsigned* sWc, unsigned long long* sWm, filt_sel* out) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int b_hi = FILT_BUCKETS - 1 - 2 * t, b_lo = b_hi - 1;
    unsigned c[2];
    unsigned long long m[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int b = j ? b_lo : b_hi;
        c[j] = hc[b];
        m[j] = hm[b];
        if (b < floor_b) c[j] = 0u, m[j] = 0ull;
        if (b == floor_b) c[j] = floor_cnt, m[j] = floor_mass;
    }
    unsigned ic = c[0] + c[1];
    unsigned long long im = m[0] + m[1];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned oc = __shfl_up(ic, off, 64);
        const unsigned lo = __shfl_up((unsigned)im, off, 64), hi = __shfl_up((unsigned)(im >> 32), off, 64);
        if (lane >= off) {
            ic += oc;
            im += ((unsigned long long)hi << 32) | lo;
        }
    }
    if (t == 0) out->found = 0;
    if (lane == 63) {
        sWc[w] = ic;
        sWm[w] = im;
    }
    __syncthreads();
    unsigned pc = 0;
    unsigned long long pm = 0, tm = 0;
    for (int k = 0; k < FILT_THREADS / 64; ++k) {
        if (k < w) pc += sWc[k], pm += sWm[k];
        tm += sWm[k];
    }
    unsigned ec = pc + ic - (c[0] + c[1]);
    unsigned long long em = pm + im - (m[0] + m[1]);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const unsigned long long above = by_mass ? em : (unsigned long long)ec, in = by_mass ? m[j] : (unsigned long long)c[j];
        if (above < target && target <= above + in) {  // one bucket at most
            out->found = 1;
            out->bucket = j ? b_lo : b_hi;
            out->cnt_above = ec;
            out->cnt_in = c[j];
            out->mass_above = em;
            out->mass_in = m[j];
        }
        ec += c[j];
        em += m[j];
    }
    if (t == 0) out->mass_total = tm;
    __syncthreads();
}

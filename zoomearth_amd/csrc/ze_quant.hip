// FP8 (OCP E4M3, the fp8 of gfx950) weight quantisation for the decode weight stream (BASELINE.json configs[4]).
// One workgroup per weight row: amax -> scale 2^k with k the smallest integer such that amax / 2^k <= 448 ->
// q = cvt_fp8(w / 2^k) (exact division, round to nearest even by v_cvt_pk_fp8_f32) -> the bf16 row is overwritten
// with q * 2^k, which bf16 represents exactly.  The prefill / ViT GEMMs and the batched-decode GEMMs keep reading the
// bf16 arena, the batch-1 decode GEMVs stream the fp8 copy (half the bytes) and dequantise in registers: both
// compute with IDENTICAL weight values.  Restated in numpy by oracle/fp8.py.  (The MXFP4 quantiser follows the fp8 one below.)
#include "ze_kernels.h"

typedef float f32x2_t __attribute__((ext_vector_type(2)));

__global__ void __launch_bounds__(256) k_quantize_rows(bf16_t* __restrict__ w, int cols, int ld,
                                                       uint8_t* __restrict__ q, int ld8, float* __restrict__ scale) {
    bf16_t* row = w + (size_t)blockIdx.x * ld;
    uint8_t* qrow = q + (size_t)blockIdx.x * ld8;
    const int tid = threadIdx.x;
    float amax = 0.f;
    for (int i = tid; i < cols; i += 256) amax = fmaxf(amax, fabsf(bf16_to_f32(row[i])));
    amax = wave_max(amax);
    __shared__ float red[4];
    if ((tid & 63) == 0) red[tid >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    int k = 0;
    if (amax > 0.f) {
        int e;
        const float m = frexpf(amax / 448.0f, &e);  // amax / 448 = m * 2^e, m in [0.5, 1)
        k = (m == 0.5f) ? e - 1 : e;
    }
    const float s = ldexpf(1.0f, k), inv = ldexpf(1.0f, -k);
    if (tid == 0) scale[blockIdx.x] = s;
    for (int i = tid * 2; i < ld8; i += 512) {  // two elements per thread-step (one cvt_pk), zero beyond cols
        const float a = i < cols ? bf16_to_f32(row[i]) * inv : 0.f;
        const float b = i + 1 < cols ? bf16_to_f32(row[i + 1]) * inv : 0.f;
        const int packed = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
        *reinterpret_cast<uint16_t*>(qrow + i) = (uint16_t)(packed & 0xffff);
        const f32x2_t back = __builtin_amdgcn_cvt_pk_f32_fp8(packed, false);
        if (i < cols) row[i] = f32_to_bf16(back.x * s);
        if (i + 1 < cols) row[i + 1] = f32_to_bf16(back.y * s);
    }
}

void ze_launch_quantize_rows(bf16_t* w, int rows, int cols, int ld, uint8_t* q, int ld8, float* scale, hipStream_t s) {
    if (rows <= 0) return;
    k_quantize_rows<<<rows, 256, 0, s>>>(w, cols, ld, q, ld8, scale);
}

// ---------------------------------------------------------------------------------------------------------------- MXFP4
// OCP MXFP4 weight quantisation for the 4-bit decode stream (ze_gemv4.hip; reduced precision, opt-in).  A row is cut into blocks of
// 32 consecutive k; per block amax = max |w|, e = floor(log2(amax)) - 2 clamped to [-125, 125] -- the range in which every
// code * 2^e, from 0.5 * 2^-125 to 6 * 2^125, is a normal bf16 -- and e = 0 for an all-zero block; the scale byte is e + 127 (E8M0).
// An element is w / 2^e rounded to the nearest of {0, 0.5, 1, 1.5, 2, 3, 4, 6} (E2M1), ties to the even code, magnitudes above 6
// saturate, the sign is kept (-0 is code 8).  q [rows, cols / 2] holds the even k in the low nibble; the bf16 row is overwritten
// with code * 2^e, which bf16 holds exactly.  Integer and exponent arithmetic on the bf16 bits only: floor(log2) is the exponent
// field, rounding is seven comparisons of the magnitude bits with the bits of the tie points 2^e * {0.25, 0.75, 1.25, 1.75, 2.5,
// 3.5, 5} (a tie goes up exactly where the upper code is even), so tests/mxfp4_ref.py reproduces every bit in numpy.  Inf and NaN
// magnitudes are above every tie point: they saturate to 6 * 2^125.
// bf16 bits of m * 2^E with E the biased exponent (<= 0: the subnormal form) and m the 7 mantissa bits below an implicit one
__device__ __forceinline__ uint32_t mx4_bits(int E, uint32_t m) { return E > 0 ? ((uint32_t)E << 7) | m : (0x80u | m) >> (1 - E); }

__global__ void __launch_bounds__(256) k_quantize_mxfp4(bf16_t* __restrict__ w, int rows, int cols, int ld, uint8_t* __restrict__ q,
                                                        uint8_t* __restrict__ scale) {
    const int bpr = cols >> 5;  // blocks per row
    const long long blk = (long long)blockIdx.x * 256 + threadIdx.x;
    if (blk >= (long long)rows * bpr) return;
    const int r = (int)(blk / bpr), b = (int)(blk % bpr);
    uint4* src = reinterpret_cast<uint4*>(w + (size_t)r * ld + (size_t)b * 32);
    uint4 v[4];
    uint32_t amax = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[i] = src[i];
        const uint32_t u[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) amax = max(amax, max(u[j] & 0x7fffu, (u[j] >> 16) & 0x7fffu));
    }
    int e = 0;
    if (amax) e = min(max((int)(amax >> 7) - 127 - 2, -125), 125);
    const int E = e + 127;
    // tie points: code goes up at "above" (t0, t2, t4, t6) or at "at or above" (t1, t3, t5)
    const uint32_t t0 = mx4_bits(E - 2, 0x00), t1 = mx4_bits(E - 1, 0x40), t2 = mx4_bits(E, 0x20), t3 = mx4_bits(E, 0x60),
                   t4 = mx4_bits(E + 1, 0x20), t5 = mx4_bits(E + 1, 0x60), t6 = mx4_bits(E + 2, 0x20);
    auto quant = [&](uint32_t h, uint32_t& back) {  // h: 16 bf16 bits -> the 4-bit code, back: bf16 bits of code * 2^e
        const uint32_t a = h & 0x7fffu, sgn = h >> 15;
        const uint32_t c = (a > t0) + (a >= t1) + (a > t2) + (a >= t3) + (a > t4) + (a >= t5) + (a > t6);
        // code c = (exponent field c >> 1, mantissa bit c & 1): 1 is 0.5 (the subnormal), c >= 2 is 1.m * 2^((c >> 1) - 1)
        const uint32_t mag = c == 0 ? 0u : c == 1 ? (uint32_t)(E - 1) << 7 : ((uint32_t)(E + (int)(c >> 1) - 1) << 7) | ((c & 1u) << 6);
        back = (sgn << 15) | mag;
        return (sgn << 3) | c;
    };
    uint32_t qw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t u[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
        uint32_t packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t lo, hi;
            const uint32_t cl = quant(u[j] & 0xffffu, lo), ch = quant(u[j] >> 16, hi);
            packed |= (cl | (ch << 4)) << (8 * j);
            u[j] = lo | (hi << 16);
        }
        qw[i] = packed;
        src[i] = make_uint4(u[0], u[1], u[2], u[3]);
    }
    *reinterpret_cast<uint4*>(q + ((size_t)r * bpr + b) * 16) = make_uint4(qw[0], qw[1], qw[2], qw[3]);
    scale[(size_t)r * bpr + b] = (uint8_t)E;
}

// Row-major MXFP4 (q [n, k / 2], scale [n, k / 32]) -> the fragment-major copy the W4 kernels of the batched decode step stream
// (ze_gemm.hip, ze_gemm_oneshot.hip; the layout is written down in zoomearth.h next to the format, restated by tests/gemm4_ref.py).
// One wave per 16 x 32 fragment (nb, ks), as k_pack_fragments8: lane = fq * 16 + fr moves the four bytes q[row][16 ks + 4 fq .. + 3]
// -- its 8 codes, nibble order untouched -- to codes[((nb S + ks) * 64 + lane) * 4], and the lanes fq == 0 move the row's scale byte of
// block ks to scales[(nb S + ks) * 16 + fr].  rope_dim: the row permutation of k_pack_fragments (qkv), for codes and scales alike.
__global__ void __launch_bounds__(256) k_pack_fragments4(const uint8_t* __restrict__ q, const uint8_t* __restrict__ scale, int n, int k,
                                                         uint8_t* __restrict__ Wf, uint8_t* __restrict__ Sf, int rope_dim) {
    const size_t frag = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int ns = k >> 5;
    if (frag >= (size_t)(n >> 4) * ns) return;
    const int lane = threadIdx.x & 63, nb = (int)(frag / ns), ks = (int)(frag % ns);
    int row = nb * 16 + (lane & 15);
    if (rope_dim > 0) {
        const int bph = rope_dim >> 4, h = nb / bph, j = nb % bph, r = lane & 15;
        row = h * rope_dim + (r < 8 ? 8 * j + r : (rope_dim >> 1) + 8 * j + (r - 8));
    }
    const uint32_t v = *reinterpret_cast<const uint32_t*>(q + (size_t)row * (k >> 1) + ks * 16 + (lane >> 4) * 4);
    *reinterpret_cast<uint32_t*>(Wf + (frag * 64 + lane) * 4) = v;
    if (lane < 16) Sf[frag * 16 + lane] = scale[(size_t)row * ns + ks];
}
// n % 16 == 0 and k % 32 == 0 (the callers check)
void ze_launch_pack_fragments4(const uint8_t* q4, const uint8_t* scale, int n, int k, uint8_t* Wf4, uint8_t* Sf4, hipStream_t s, int rope_dim) {
    const size_t frags = (size_t)(n >> 4) * (k >> 5);
    if (frags == 0) return;
    k_pack_fragments4<<<(unsigned)((frags + 3) / 4), 256, 0, s>>>(q4, scale, n, k, Wf4, Sf4, rope_dim);
}

// cols % 32 == 0, ld % 8 == 0 and w 16-byte aligned (the callers check): a thread owns one block
void ze_launch_quantize_mxfp4(bf16_t* w, int rows, int cols, int ld, uint8_t* q, uint8_t* scale, hipStream_t s) {
    if (rows <= 0 || cols <= 0) return;
    const long long blocks = (long long)rows * (cols >> 5);
    k_quantize_mxfp4<<<(unsigned)((blocks + 255) / 256), 256, 0, s>>>(w, rows, cols, ld, q, scale);
}

// The wave-per-row RMSNorm's arithmetic, written once: k_rmsnorm (ze_elementwise.hip) and the gathering norm of the scoring pass
// (ze_score.hip: k_rmsnorm_gather) call these two functions, so that a row comes out as the same bits from either.
//   y = w * bf16(x * rsqrt(mean(x^2) + eps)), the cast to bf16 BEFORE the weight multiply (HF's Qwen2RMSNorm).
// One wave per row; lane l owns the 16-byte vectors l, l + 64, ...; the sum of squares goes lane partials in vector order, then
// the xor butterfly of wave_sum -- a function of the row alone.
#pragma once
#include "ze_common.h"

// rsqrt(mean(x^2) + eps) of the row at xr (cols % 8 == 0), in every lane of the wave
__device__ __forceinline__ float rms_wave_inv(const bf16_t* __restrict__ xr, int cols, float eps, int lane) {
    float ss = 0.f;
    const int nv = cols >> 3;
    for (int v = lane; v < nv; v += 64) {
        const uint4 q = *reinterpret_cast<const uint4*>(xr + v * 8);
        const uint32_t u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a = bf16lo(u[j]), b = bf16hi(u[j]);
            ss += a * a + b * b;
        }
    }
    ss = wave_sum(ss);
    return rsqrtf(ss / (float)cols + eps);
}

// the eight normalised, weighted elements of vector v of the row, as four packed bf16 pairs
__device__ __forceinline__ void rms_norm_vec(const bf16_t* __restrict__ xr, const bf16_t* __restrict__ w, int v, float inv,
                                             uint32_t (&o)[4]) {
    const uint4 q = *reinterpret_cast<const uint4*>(xr + v * 8);
    const uint4 g = *reinterpret_cast<const uint4*>(w + v * 8);
    const uint32_t u[4] = {q.x, q.y, q.z, q.w};
    const uint32_t gw[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float a = bf16_round(bf16lo(u[j]) * inv) * bf16lo(gw[j]);
        const float b = bf16_round(bf16hi(u[j]) * inv) * bf16hi(gw[j]);
        o[j] = pack_bf16x2(a, b);
    }
}

// MXFP4 (OCP: E2M1 codes, one E8M0 scale per 32 elements along K) instantiations of the decode weight-streaming kernel: the
// shape policy of the fp8 stream, 2048-element chunks -- a lane's 16-B load is exactly one scale block -- and the dequantised
// pair code * 2^e straight out of v_cvt_scalef32_pk_f32_fp4 (ze_quant.hip, tests/mxfp4_ref.py).  Reduced precision, opt-in.
#include "ze_gemv_kernel.h"

bool ze_launch_gemv4(int epi, const ze_gemv_args& a, hipStream_t s) {
    if (a.K % 32) return false;
    if ((size_t)((a.K + 2047) / 2048 + 1) * 4096 + 128 > 60000) return false;  // x (and the zero chunk) must fit the LDS stage
    // Shape policy.  A chunk is 2048 elements, so the decoder's K = 2048 .. 3584 rows are one or two chunks: a trip is as many chunks
    // as the row has (a trip past the row's end would convert and multiply the zero chunk).  At one chunk a wave takes ONE row pair
    // whatever N: two pairs make hipcc unroll the pair-set loop to 185 VGPRs (2 waves per SIMD against the family's 4) and measured
    // 9.46 us against 8.62 on the 3B gate/up.  Long K (the down projection) splits K over the four waves as the family does.
    const bool long_k = a.K > 4096;
    const bool many_rows = a.N >= 8192 && ze_knobs[ZE_KNOB_GATE_UP_FLASH] != ZE_GATE_UP_ONE_PAIR;  // (knob 1 = 2: one pair per wave, as for the fp8 stream)
    const bool wide_one = many_rows && ze_knobs[ZE_KNOB_GATE_UP_FLASH] == ZE_GATE_UP_TWO_PAIRS;      // (knob 1 = 1: the measured-and-rejected two pairs at one chunk)
    const bool one_chunk = a.K <= 2048;
#define ZE_GV4(EPI, P1, PM1, P2, PM2)                                                   \
    if (one_chunk) {                                                                    \
        if (wide_one) launch_gemv_cfg<EPI, PM1, 1, 1, 4>(a, s);                         \
        else launch_gemv_cfg<EPI, P1, 1, 1, 4>(a, s);                                   \
    } else {                                                                            \
        if (many_rows) launch_gemv_cfg<EPI, PM2, 1, 2, 4>(a, s);                        \
        else launch_gemv_cfg<EPI, P2, 1, 2, 4>(a, s);                                   \
    }
    switch (epi) {
        case ZE_GV_QKV_ROPE: ZE_GV4(ZE_GV_QKV_ROPE, 1, 1, 1, 1) break;
        case ZE_GV_SWIGLU: ZE_GV4(ZE_GV_SWIGLU, 1, 2, 1, 2) break;
        case ZE_GV_RESIDUAL:
            if (long_k) launch_gemv_cfg<ZE_GV_RESIDUAL, 2, 4, 2, 4>(a, s);
            else ZE_GV4(ZE_GV_RESIDUAL, 1, 1, 1, 1)
            break;
        case ZE_GV_LOGITS: ZE_GV4(ZE_GV_LOGITS, 1, 2, 1, 2) break;
        default:
            if (long_k) launch_gemv_cfg<ZE_GV_PLAIN, 2, 4, 2, 4>(a, s);
            else ZE_GV4(ZE_GV_PLAIN, 1, 1, 1, 1)
            break;
    }
#undef ZE_GV4
    return true;
}

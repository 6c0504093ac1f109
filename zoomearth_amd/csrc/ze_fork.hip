// Fork of a prefilled chain (ze_seq_fork): the source's cached K/V rows, its last-position logits row and its repetition-penalty set
// go to n destination slots in ONE launch.  Every 16-byte piece of the source is loaded once and stored n times -- one read and n
// writes where n launches of k_kv_copy_prefix read the source n times.
#include "ze_kernels.h"

#include <algorithm>

// blockIdx.y < kv_runs: (layer, kv head, K|V) picks one contiguous run of the cache (n_vec 16-byte pieces from the chain's row 0), as
// in k_kv_copy_prefix; blockIdx.y == kv_runs: the fp32 logits row (vocab floats); kv_runs + 1: the seen-set (vocab bytes).
// blockIdx.x strides over the run's pieces.  dst[0 .. n): the destination slots, a device table written in stream order in front of
// the launch.  vec_rows = 0: vocab is no multiple of 16, the two rows go element by element.
__global__ void __launch_bounds__(256) k_kv_fork(bf16_t* __restrict__ kcache, bf16_t* __restrict__ vcache, size_t layer_stride,
                                                 size_t seq_stride, size_t head_stride, int kv_heads, int kv_runs, int src,
                                                 const int* __restrict__ dst, int n, int n_vec, float* __restrict__ logits,
                                                 uint8_t* __restrict__ seen, int vocab, int vec_rows) {
    const int y = blockIdx.y, first = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
    if (y < kv_runs) {
        const int which = y & 1, kvh = (y >> 1) % kv_heads, layer = (y >> 1) / kv_heads;
        bf16_t* base = (which ? vcache : kcache) + (size_t)layer * layer_stride + (size_t)kvh * head_stride;
        const uint4* s = reinterpret_cast<const uint4*>(base + (size_t)src * seq_stride);
        for (int i = first; i < n_vec; i += step) {
            const uint4 v = s[i];
            for (int k = 0; k < n; ++k) reinterpret_cast<uint4*>(base + (size_t)dst[k] * seq_stride)[i] = v;
        }
        return;
    }
    const bool lg = y == kv_runs;
    if (vec_rows) {
        // (vocab % 16 == 0: both rows start on 16-byte boundaries in every slot)
        const int pieces = lg ? vocab / 4 : vocab / 16;
        char* base = lg ? reinterpret_cast<char*>(logits) : reinterpret_cast<char*>(seen);
        const size_t row_bytes = lg ? (size_t)vocab * sizeof(float) : (size_t)vocab;
        const uint4* s = reinterpret_cast<const uint4*>(base + (size_t)src * row_bytes);
        for (int i = first; i < pieces; i += step) {
            const uint4 v = s[i];
            for (int k = 0; k < n; ++k) reinterpret_cast<uint4*>(base + (size_t)dst[k] * row_bytes)[i] = v;
        }
        return;
    }
    for (int i = first; i < vocab; i += step) {
        if (lg) {
            const float v = logits[(size_t)src * vocab + i];
            for (int k = 0; k < n; ++k) logits[(size_t)dst[k] * vocab + i] = v;
        } else {
            const uint8_t v = seen[(size_t)src * vocab + i];
            for (int k = 0; k < n; ++k) seen[(size_t)dst[k] * vocab + i] = v;
        }
    }
}

// The x-extent: k_kv_copy_prefix caps it at 8 blocks per run, sized for a 347-row prefix; a fork copies a whole prompt (800 - 1300
// rows = 12,800 - 20,800 pieces per run at head_dim 128).  A streaming kernel wants about 8 blocks of 256 threads per CU and no more
// (256 CUs: ~2048 blocks, grid-stride the rest), so the runs share that budget: 14 blocks per run for the 3B model's 144 runs, at
// most 16 for a model with fewer.
int ze_kv_fork_blocks(int runs, int n_vec) { return std::max(1, std::min({16, 2048 / std::max(1, runs), (n_vec + 255) / 256})); }

void ze_launch_kv_fork(bf16_t* kcache, bf16_t* vcache, size_t layer_stride, size_t seq_stride, size_t head_stride, int layers, int kv_heads,
                       int D, int src, const int* dst_dev, int n, int n_tokens, float* logits, uint8_t* seen, int vocab, hipStream_t s) {
    if (n <= 0 || n_tokens <= 0) return;
    const int n_vec = n_tokens * D * 2 / 16, runs = layers * kv_heads * 2;
    // (the two vocabulary rows are at most as long as a run of a few hundred tokens: the same x-extent serves them)
    const int gx = ze_kv_fork_blocks(runs + 2, std::max(n_vec, vocab / 4));
    k_kv_fork<<<dim3(gx, runs + 2), 256, 0, s>>>(kcache, vcache, layer_stride, seq_stride, head_stride, kv_heads, runs, src, dst_dev, n, n_vec,
                                                 logits, seen, vocab, vocab % 16 == 0 ? 1 : 0);
}

// TIFF tile decode on the device: LZW and PackBits chunks (strips or tiles) of an 8-bit RGB file, the horizontal predictor, and the
// placement of padded tiles.  The state machines are in ze_tiff_codec.h (shared with the sanitizer program of tests/tiff_san); this
// unit holds the three kernels, the scratch they need and the two C-ABI entries.
//
// One wave decodes one chunk: the code stream of a chunk is serial, a tile has thousands of chunks.  The wave's scalar side runs the
// state machine, its 64 lanes perform each emit as a byte copy inside the chunk's own output.
#include "ze_engine.h"
#include "ze_tiff_codec.h"

namespace {

struct tiff_args {
    const uint8_t* bytes;   // the concatenated chunks, each on a 16-byte boundary
    uint64_t n_bytes;       // a multiple of 16
    const int32_t* table;   // [n_chunks, ZT_TABLE_INTS]
    uint8_t* rgb;           // u8 [h, w, 3]
    uint8_t* tiles;         // tiled: [n_chunks, chunk_h, chunk_w, 3] padded tiles
    int32_t* status;        // [n_chunks]
    int h, w, tiled, chunk_w, chunk_h, predictor;
};

// The chunk's table row in scalar registers; false (and its status written) when the row does not fit.
__device__ __forceinline__ bool chunk_row(const tiff_args& a, int chunk, zt_chunk& t) {
    const int32_t* r = a.table + (size_t)chunk * ZT_TABLE_INTS;
    t.off = __builtin_amdgcn_readfirstlane(r[0]), t.len = __builtin_amdgcn_readfirstlane(r[1]);
    t.x0 = __builtin_amdgcn_readfirstlane(r[2]), t.y0 = __builtin_amdgcn_readfirstlane(r[3]);
    t.w = __builtin_amdgcn_readfirstlane(r[4]), t.h = __builtin_amdgcn_readfirstlane(r[5]);
    t.sw = __builtin_amdgcn_readfirstlane(r[6]), t.sh = __builtin_amdgcn_readfirstlane(r[7]);
    return zt_chunk_ok(t, a.n_bytes, a.h, a.w, a.tiled, a.chunk_w, a.chunk_h) != 0;
}
__device__ __forceinline__ uint8_t* chunk_out(const tiff_args& a, int chunk, const zt_chunk& t) {
    return a.tiled ? a.tiles + (size_t)chunk * a.chunk_w * a.chunk_h * 3 : a.rgb + (size_t)t.y0 * a.w * 3;
}

// 16 KB of LDS (the string table) per wave, one wave per workgroup: up to ten chunks in flight per CU (160 KB).
__global__ __launch_bounds__(64) void k_tiff_lzw(tiff_args a) {
    __shared__ uint32_t table[ZT_LZW_CODES];
    const int chunk = blockIdx.x, lane = threadIdx.x;
    zt_chunk t;
    if (!chunk_row(a, chunk, t)) {
        if (lane == 0) a.status[chunk] = ZT_BAD_TABLE;
        return;
    }
    uint8_t* out = chunk_out(a, chunk, t);
    zt_lzw s;
    zt_lzw_init(s, a.bytes + t.off, (uint32_t)t.len, (uint32_t)t.sw * (uint32_t)t.sh * 3u);
    // out[0, fenced) is known to have reached memory: a copy whose source ends below it needs no wait
    uint32_t fenced = 0;
    zt_emit e;
    while (zt_lzw_step(s, table, e)) {
        if (e.kind == ZT_EMIT_FILL) {  // a literal: one byte
            if (lane == 0) out[e.dst] = (uint8_t)e.value;
            continue;
        }
        const uint32_t d = e.dst - e.src;  // >= 1: the source starts before the destination
        const uint32_t reach = e.len < d ? e.len : d;
        if (e.src + reach > fenced) {
            // the source bytes were stored by other lanes of this wave: their stores complete (release) before any lane loads (acquire)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            fenced = e.dst;
        }
        if (d >= e.len) {
            for (uint32_t i = lane; i < e.len; i += 64) out[e.dst + i] = out[e.src + i];
        } else {  // the source runs into the destination (KwKwK): every read stays below dst
            for (uint32_t i = lane; i < e.len; i += 64) out[e.dst + i] = out[e.src + i % d];
        }
    }
    if (lane == 0) a.status[chunk] = s.status;
}

__global__ __launch_bounds__(64) void k_tiff_packbits(tiff_args a) {
    const int chunk = blockIdx.x, lane = threadIdx.x;
    zt_chunk t;
    if (!chunk_row(a, chunk, t)) {
        if (lane == 0) a.status[chunk] = ZT_BAD_TABLE;
        return;
    }
    uint8_t* out = chunk_out(a, chunk, t);
    const uint8_t* in = a.bytes + t.off;
    zt_packbits s;
    zt_packbits_init(s, in, (uint32_t)t.len, (uint32_t)t.sw * (uint32_t)t.sh * 3u);
    zt_emit e;
    while (zt_packbits_step(s, e)) {  // at most 128 bytes per emit
        for (uint32_t i = lane; i < e.len; i += 64) out[e.dst + i] = e.kind == ZT_EMIT_FILL ? (uint8_t)e.value : in[e.src + i];
    }
    if (lane == 0) a.status[chunk] = s.status;
}

__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(v, o);
        if (lane >= o) v += up;
    }
    return v;
}

// Predictor 2 and the placement of tiles: one wave (one workgroup) per stored row of a chunk, the rows of a chunk strided over grid.y
// (UNPREDICT_MAX_GRID_Y at the most: a chunk of more rows than that gives each wave several).  The row's running sum mod 256 per channel
// is a wave scan over 64 pixels at a time with a carry between the pieces (R and G share a word: 64 x 255 stays below 2^16).  Strips
// are summed in place; a tile's row goes from the padded tile to its clipped place in the image (predictor 1: a copy).
constexpr int UNPREDICT_MAX_GRID_Y = 4096;
__global__ __launch_bounds__(64) void k_tiff_unpredict(tiff_args a) {
    const int chunk = blockIdx.x, lane = threadIdx.x;
    zt_chunk t;
    if (!chunk_row(a, chunk, t) || __builtin_amdgcn_readfirstlane(a.status[chunk]) != ZT_OK) return;
    const int x0 = t.x0, y0 = t.y0, cw = t.w, ch = t.h;
    for (int row = blockIdx.y; row < ch; row += gridDim.y) {  // (the padding rows of an edge tile land nowhere)
        const uint8_t* src = a.tiled ? a.tiles + ((size_t)chunk * a.chunk_h + row) * a.chunk_w * 3 : a.rgb + (size_t)(y0 + row) * a.w * 3;
        uint8_t* dst = a.rgb + ((size_t)(y0 + row) * a.w + x0) * 3;
        uint32_t carry_rg = 0, carry_b = 0;
        for (int base = 0; base < cw; base += 64) {  // the pixels right of cw are padding: nothing left of them depends on them
            const int p = base + lane;
            uint32_t r = 0, g = 0, b = 0;
            if (p < cw) r = src[p * 3], g = src[p * 3 + 1], b = src[p * 3 + 2];
            if (a.predictor == 2) {
                const uint32_t rg = wave_inclusive_sum(r | (g << 16), lane) + carry_rg;
                const uint32_t bb = wave_inclusive_sum(b, lane) + carry_b;
                r = rg & 255u, g = (rg >> 16) & 255u, b = bb & 255u;
                carry_rg = __shfl(rg, 63) & 0x00ff00ffu;
                carry_b = __shfl(bb, 63) & 255u;
            }
            if (p < cw) dst[p * 3] = (uint8_t)r, dst[p * 3 + 1] = (uint8_t)g, dst[p * 3 + 2] = (uint8_t)b;
        }
    }
}

int grow(ze_engine* e, uint8_t*& p, size_t& cap, size_t need, const char* what) {
    if (need <= cap) return ZE_OK;
    if (e->tiff_done) ZE_HIP(hipEventSynchronize(e->tiff_done));  // the last reader of the old buffer
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    const size_t want = (need + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
    if (hipMalloc((void**)&p, want) != hipSuccess) {
        p = nullptr;
        (void)hipGetLastError();
        return ze_fail(e, ZE_ERR_NOMEM, what);
    }
    cap = want;
    return ZE_OK;
}

int check_shape(ze_engine* e, size_t n_bytes, int n_chunks, int h, int w, int compression, int predictor, int tiled, int chunk_w, int chunk_h) {
    if (n_bytes == 0 || n_bytes % ZT_INPUT_ALIGN != 0 || n_chunks <= 0 || h <= 0 || w <= 0 || chunk_w <= 0 || chunk_h <= 0)
        return ze_fail(e, ZE_ERR_INVALID, "tiff decode: empty image, no chunks, or an input size that is no multiple of 16");
    if (compression != ZT_COMPRESSION_LZW && compression != ZT_COMPRESSION_PACKBITS)
        return ze_fail(e, ZE_ERR_INVALID, "tiff decode: compression is neither 5 (LZW) nor 32773 (PackBits)");
    if (predictor != 1 && predictor != 2) return ze_fail(e, ZE_ERR_INVALID, "tiff decode: predictor is neither 1 nor 2");
    if ((tiled != 0 && tiled != 1) || (!tiled && chunk_w != w)) return ze_fail(e, ZE_ERR_INVALID, "tiff decode: strips are as wide as the image");
    if ((uint64_t)chunk_w * (uint64_t)chunk_h * 3u > ZT_MAX_CHUNK_OUT) return ze_fail(e, ZE_ERR_INVALID, "tiff decode: a chunk stores more than 1 MiB");
    if ((uint64_t)n_chunks * (uint64_t)chunk_w * (uint64_t)chunk_h * 3u > ((uint64_t)1 << 33))
        return ze_fail(e, ZE_ERR_INVALID, "tiff decode: more chunks than any image has");
    return ZE_OK;
}

// the kernels on device operands; tiff_done is recorded behind them
int launch(ze_engine* e, tiff_args a, int n_chunks, int compression, hipStream_t s) {
    if (a.tiled) {
        ZE_TRY(grow(e, e->tiff_tiles, e->tiff_tiles_cap, (size_t)n_chunks * a.chunk_w * a.chunk_h * 3, "hipMalloc of the padded tiles failed"));
        a.tiles = e->tiff_tiles;
    }
    if (compression == ZT_COMPRESSION_LZW)
        k_tiff_lzw<<<n_chunks, 64, 0, s>>>(a);
    else
        k_tiff_packbits<<<n_chunks, 64, 0, s>>>(a);
    ZE_KCHECK();
    if (a.tiled || a.predictor == 2) {
        k_tiff_unpredict<<<dim3(n_chunks, std::min(a.chunk_h, UNPREDICT_MAX_GRID_Y)), 64, 0, s>>>(a);
        ZE_KCHECK();
    }
    if (!e->tiff_done) ZE_HIP(hipEventCreateWithFlags(&e->tiff_done, hipEventDisableTiming));
    ZE_HIP(hipEventRecord(e->tiff_done, s));
    return ZE_OK;
}

}  // namespace

extern "C" int ze_op_tiff_decode(ze_engine* e, const uint8_t* dev_bytes, size_t n_bytes, const int32_t* dev_table, int n_chunks, int h, int w,
                                 int compression, int predictor, int tiled, int chunk_w, int chunk_h, uint8_t* dev_rgb, int32_t* dev_status,
                                 void* stream) {
    if (!e || !dev_bytes || !dev_table || !dev_rgb || !dev_status) return ze_fail(e, ZE_ERR_INVALID, "tiff decode: null argument");
    if ((uintptr_t)dev_bytes % ZT_INPUT_ALIGN != 0) return ze_fail(e, ZE_ERR_INVALID, "tiff decode: the input is not 16-byte aligned");
    ZE_TRY(check_shape(e, n_bytes, n_chunks, h, w, compression, predictor, tiled, chunk_w, chunk_h));
    (void)hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    if (e->tiff_done) ZE_HIP(hipStreamWaitEvent(s, e->tiff_done, 0));  // the padded tiles of the call before, on whatever stream
    tiff_args a{dev_bytes, (uint64_t)n_bytes, dev_table, dev_rgb, nullptr, dev_status, h, w, tiled, chunk_w, chunk_h, predictor};
    return launch(e, a, n_chunks, compression, s);
}

extern "C" int ze_tile_upload_tiff(ze_engine* e, const uint8_t* host_bytes, size_t n_bytes, const int32_t* host_table, int n_chunks, int h,
                                   int w, int compression, int predictor, int tiled, int chunk_w, int chunk_h, uint8_t* dev_rgb,
                                   int32_t* dev_status, void* stream) {
    if (!e || !host_bytes || !host_table || !dev_rgb || !dev_status) return ze_fail(e, ZE_ERR_INVALID, "tile_upload_tiff: null argument");
    ZE_TRY(check_shape(e, n_bytes, n_chunks, h, w, compression, predictor, tiled, chunk_w, chunk_h));
    (void)hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t table_bytes = (size_t)n_chunks * ZT_TABLE_INTS * sizeof(int32_t);
    ZE_TRY(grow(e, e->tiff_in, e->tiff_in_cap, n_bytes + table_bytes, "hipMalloc of the compressed tile failed"));
    if (e->tiff_done) ZE_HIP(hipStreamWaitEvent(s, e->tiff_done, 0));  // the kernels of the tile before still read the staging
    ZE_HIP(hipMemcpyAsync(e->tiff_in, host_bytes, n_bytes, hipMemcpyHostToDevice, s));
    ZE_HIP(hipMemcpyAsync(e->tiff_in + n_bytes, host_table, table_bytes, hipMemcpyHostToDevice, s));
    tiff_args a{e->tiff_in, (uint64_t)n_bytes, (const int32_t*)(e->tiff_in + n_bytes), dev_rgb, nullptr, dev_status, h, w, tiled, chunk_w, chunk_h,
                predictor};
    return launch(e, a, n_chunks, compression, s);
}

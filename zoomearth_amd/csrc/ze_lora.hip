// LoRA adapters (ze_lora_*): a low-rank delta merged into the live weight arena.  No forward kernel knows about adapters: an active
// adapter IS the arena's contents, W' = bf16(W + scale * B @ A) per adapted tensor, computed from a bf16 snapshot of the base tensor
// (the base store) so that every switch is ONE pass per tensor -- never unmerge-then-merge, whose rounding would not return the
// base bits.
//
// The arithmetic of one element is fixed (LoRA): fp32, k ascending, products and sums rounded separately (no fused
// multiply-add), one bf16 round-to-nearest-even at the end -- numpy float32 reproduces it bit for bit (tests/lora_ref.py).
#include "ze_engine.h"

#include <string.h>

#include <algorithm>
#include <memory>

__device__ __forceinline__ int lora_map_row(int r, int mode, int offset) {  // = map_row of k_pack_rows (ze_elementwise.hip)
    return mode == 0 ? offset + r : (r >> 4) * 32 + (r & 15) + offset;
}

// One tensor per launch.  A work item is a tile of LORA_ROWS rows x 256 * VEC columns: a thread owns VEC consecutive columns of
// every row of the tile.  The tile's B rows are staged in LDS (read back as broadcasts); A[k, col .. col + VEC) is loaded once per k
// -- coalesced, 32 bytes per lane with VEC = 8 -- and reused across the tile's rows, so A traffic (L2-resident: r x cols floats) is
// r / LORA_ROWS of the weight stream.  VEC = 8: 16-byte loads of base and 16-byte stores into the arena; VEC = 1: the scalar form
// for cols % 8 != 0 or pointers / leading dimensions off the 16-byte grid.  r = 0 copies the base bits (the restore).
enum { LORA_ROWS = 16 };

template <int VEC>
__global__ void __launch_bounds__(256) k_lora_merge(const bf16_t* __restrict__ base, int rows, int cols, const float* __restrict__ A,
                                                    const float* __restrict__ B, int r, float scale, bf16_t* __restrict__ dst, int ld,
                                                    int mode, int offset) {
    // (built with -ffp-contract=off, csrc/Makefile: the products and sums below stay separate instructions)
    __shared__ float Bs[LORA_ROWS * ZE_LORA_MAX_RANK];
    const int col_tiles = (cols + 256 * VEC - 1) / (256 * VEC), row_tiles = (rows + LORA_ROWS - 1) / LORA_ROWS;
    const int items = col_tiles * row_tiles;
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        // (consecutive items share a row tile: its B rows stay in L2 while the column tiles pass)
        const int rt = item / col_tiles, ct = item - rt * col_tiles;
        const int row0 = rt * LORA_ROWS, nr = min(LORA_ROWS, rows - row0);
        const int col = (ct * 256 + threadIdx.x) * VEC;
        __syncthreads();  // the previous item's readers of Bs
        for (int i = threadIdx.x; i < nr * r; i += 256) Bs[i] = B[(size_t)row0 * r + i];
        __syncthreads();
        if (col >= cols) continue;
        float acc[LORA_ROWS][VEC];
#pragma unroll
        for (int i = 0; i < LORA_ROWS; ++i)
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc[i][j] = 0.0f;
        for (int k = 0; k < r; ++k) {
            float a[VEC];
            if (VEC == 8) {
                const float4 a0 = *reinterpret_cast<const float4*>(A + (size_t)k * cols + col);
                const float4 a1 = *reinterpret_cast<const float4*>(A + (size_t)k * cols + col + 4);
                a[0] = a0.x, a[1] = a0.y, a[2] = a0.z, a[3] = a0.w;
                a[4 % VEC] = a1.x, a[5 % VEC] = a1.y, a[6 % VEC] = a1.z, a[7 % VEC] = a1.w;
            } else {
                a[0] = A[(size_t)k * cols + col];
            }
#pragma unroll
            for (int i = 0; i < LORA_ROWS; ++i) {
                const float b = Bs[i * r + k];  // (rows >= nr read stale LDS: their sums are never stored)
#pragma unroll
                for (int j = 0; j < VEC; ++j) acc[i][j] = __fadd_rn(acc[i][j], __fmul_rn(b, a[j]));
            }
        }
#pragma unroll
        for (int i = 0; i < LORA_ROWS; ++i) {
            if (i >= nr) continue;
            const size_t src = (size_t)(row0 + i) * cols + col, out = (size_t)lora_map_row(row0 + i, mode, offset) * ld + col;
            if (VEC == 8) {
                uint4 w = *reinterpret_cast<const uint4*>(base + src);
                if (r > 0) {
                    uint32_t* p = reinterpret_cast<uint32_t*>(&w);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        p[j] = pack_bf16x2(__fadd_rn(bf16lo(p[j]), __fmul_rn(scale, acc[i][(2 * j) % VEC])),
                                           __fadd_rn(bf16hi(p[j]), __fmul_rn(scale, acc[i][(2 * j + 1) % VEC])));
                }
                *reinterpret_cast<uint4*>(dst + out) = w;
            } else {
                const bf16_t w = base[src];
                dst[out] = r > 0 ? f32_to_bf16(__fadd_rn(bf16_to_f32(w), __fmul_rn(scale, acc[i][0]))) : w;
            }
        }
    }
}

// The inverse of k_pack_rows for bf16: the tensor's rows out of the arena, through the row map, into a row-major rows x cols store.
// A thread moves VEC consecutive columns (16 bytes with VEC = 8).
template <int VEC>
__global__ void __launch_bounds__(256) k_lora_snapshot(const bf16_t* __restrict__ arena, int ld, int mode, int offset,
                                                       bf16_t* __restrict__ store, int rows, int cols) {
    const int per_row = (cols + VEC - 1) / VEC;
    const size_t n = (size_t)rows * per_row;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int row = (int)(i / per_row), col = (int)(i - (size_t)row * per_row) * VEC;
        const size_t src = (size_t)lora_map_row(row, mode, offset) * ld + col, out = (size_t)row * cols + col;
        if (VEC == 8)
            *reinterpret_cast<uint4*>(store + out) = *reinterpret_cast<const uint4*>(arena + src);
        else
            store[out] = arena[src];
    }
}

// about 8 workgroups of 256 per CU (256 CUs), grid-stride beyond that: the extent of the repo's other streaming kernels (ze_fork.hip)
static unsigned lora_grid(size_t work_items) { return (unsigned)std::max<size_t>(1, std::min<size_t>(2048, work_items)); }
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static void ze_launch_lora_merge(const bf16_t* base, int rows, int cols, const float* A, const float* B, int r, float scale, bf16_t* dst, int ld,
                          int mode, int offset, hipStream_t s) {
    if (rows <= 0 || cols <= 0) return;
    const bool vec = cols % 8 == 0 && ld % 8 == 0 && aligned16(base) && aligned16(dst) && (r == 0 || aligned16(A));
    const int row_tiles = (rows + LORA_ROWS - 1) / LORA_ROWS;
    if (vec)
        k_lora_merge<8><<<lora_grid((size_t)row_tiles * ((cols + 2047) / 2048)), 256, 0, s>>>(base, rows, cols, A, B, r, scale, dst, ld, mode, offset);
    else
        k_lora_merge<1><<<lora_grid((size_t)row_tiles * ((cols + 255) / 256)), 256, 0, s>>>(base, rows, cols, A, B, r, scale, dst, ld, mode, offset);
}

static void ze_launch_lora_snapshot(const bf16_t* arena, int ld, int mode, int offset, bf16_t* store, int rows, int cols, hipStream_t s) {
    if (rows <= 0 || cols <= 0) return;
    if (cols % 8 == 0 && ld % 8 == 0 && aligned16(arena) && aligned16(store))
        k_lora_snapshot<8><<<lora_grid(((size_t)rows * (cols / 8) + 255) / 256), 256, 0, s>>>(arena, ld, mode, offset, store, rows, cols);
    else
        k_lora_snapshot<1><<<lora_grid(((size_t)rows * cols + 255) / 256), 256, 0, s>>>(arena, ld, mode, offset, store, rows, cols);
}

// ================================================================== the adapters
// Invariant: while adapter X is active, every tensor X names is in the base store, and every tensor X does not name holds its base
// bits in the arena.  So a tensor that is not yet in the store can always be snapshotted from the arena.
static void free_tensor(ze_lora_tensor& t) {
    if (t.A) hipFree(t.A);
    if (t.B) hipFree(t.B);
    t.A = t.B = nullptr;
}

static void drop_store(ze_lora* l) {
    for (auto& kv : l->store)
        if (kv.second) hipFree(kv.second);
    l->store.clear();
    l->store_bytes = 0;
}

void ze_lora_base_written(ze_engine* e) {
    if (!e || !e->lora) return;
    e->lora->active = -1;
    drop_store(e->lora);
}

void ze_lora_free(ze_engine* e) {
    if (!e->lora) return;
    for (auto& ad : e->lora->ad)
        for (auto& kv : ad.t) free_tensor(kv.second);
    drop_store(e->lora);
    delete e->lora;
    e->lora = nullptr;
}

static int check_adapter(ze_engine* e, int adapter) {
    if (!e) return ze_fail(e, ZE_ERR_INVALID, "null engine");
    if (adapter < 0 || adapter >= ZE_MAX_ADAPTERS || !e->lora || !e->lora->ad[adapter].used)
        return ze_fail(e, ZE_ERR_NOTFOUND, "no such adapter");
    return ZE_OK;
}

extern "C" int ze_lora_create(ze_engine* e, int* adapter) {
    if (!e || !adapter) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (!e->lora) e->lora = new ze_lora;
    for (int i = 0; i < ZE_MAX_ADAPTERS; ++i)
        if (!e->lora->ad[i].used) {
            e->lora->ad[i].used = true;
            *adapter = i;
            return ZE_OK;
        }
    return ze_fail(e, ZE_ERR_NOMEM, "the engine already holds ZE_MAX_ADAPTERS adapters");
}

// fp16 / bf16 / fp32 -> fp32, exactly
static void to_f32(const void* src, int dtype, size_t n, float* out) {
    if (dtype == ZE_F32) {
        memcpy(out, src, n * sizeof(float));
    } else if (dtype == ZE_BF16) {
        const uint16_t* p = (const uint16_t*)src;
        for (size_t i = 0; i < n; ++i) {
            const uint32_t u = (uint32_t)p[i] << 16;
            memcpy(out + i, &u, 4);
        }
    } else {
        const uint16_t* p = (const uint16_t*)src;
        for (size_t i = 0; i < n; ++i) {
            const uint32_t h = p[i], sign = (h & 0x8000u) << 16, ex = (h >> 10) & 31u, man = h & 1023u;
            uint32_t u;
            if (ex == 31) {
                u = sign | 0x7f800000u | (man << 13);
            } else if (ex != 0) {
                u = sign | ((ex + 112u) << 23) | (man << 13);
            } else if (man == 0) {
                u = sign;
            } else {  // subnormal half: man * 2^-24
                int sh = 0;
                uint32_t m = man;
                while (!(m & 1024u)) m <<= 1, ++sh;
                u = sign | ((uint32_t)(113 - sh) << 23) | ((m & 1023u) << 13);
            }
            memcpy(out + i, &u, 4);
        }
    }
}

extern "C" int ze_lora_add(ze_engine* e, int adapter, const char* name, int dtype, int r, float scale, const void* host_A,
                           const void* host_B) {
    ZE_TRY(check_adapter(e, adapter));
    if (!name || !host_A || !host_B) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (dtype != ZE_F32 && dtype != ZE_F16 && dtype != ZE_BF16) return ze_fail(e, ZE_ERR_INVALID, "bad dtype");
    if (r < 1 || r > ZE_LORA_MAX_RANK) return ze_fail(e, ZE_ERR_INVALID, std::string("LoRA rank out of range [1, 128] for ") + name);
    if (e->lora->active == adapter) return ze_fail(e, ZE_ERR_INVALID, "the adapter is active: deactivate it before adding to it");
    const std::string cn = ze_canonical_name(name);
    auto it = e->dests.find(cn);
    if (it == e->dests.end() && cn != "lm_head.weight") return ze_fail(e, ZE_ERR_NOTFOUND, std::string("unknown weight: ") + name);
    // (a tied lm_head has no entry of its own)
    if (it == e->dests.end() || it->second.kind != 0)
        return ze_fail(e, ZE_ERR_INVALID, std::string("LoRA adapts projection matrices only (not embeddings, lm_head, norms or biases): ") + name);
    const ze_dest& d = it->second;
    ze_lora_adapter& ad = e->lora->ad[adapter];
    if (ad.t.count(cn)) return ze_fail(e, ZE_ERR_INVALID, std::string("the adapter already has a delta for ") + name);
    hipSetDevice(e->device);
    const size_t na = (size_t)r * d.cols, nb = (size_t)d.rows * r;
    std::unique_ptr<float[]> host(new float[std::max(na, nb)]);
    ze_lora_tensor t;
    t.r = r, t.scale = scale;
    auto upload = [&](const void* src, size_t n, float** dev) {
        to_f32(src, dtype, n, host.get());
        return hipMalloc((void**)dev, n * sizeof(float)) == hipSuccess &&
               hipMemcpy(*dev, host.get(), n * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    };
    if (!upload(host_A, na, &t.A) || !upload(host_B, nb, &t.B)) {
        hipGetLastError();
        free_tensor(t);
        return ze_fail(e, ZE_ERR_NOMEM, "LoRA: the device allocation failed");
    }
    ad.t[cn] = t;
    return ZE_OK;
}

extern "C" int ze_lora_destroy(ze_engine* e, int adapter) {
    ZE_TRY(check_adapter(e, adapter));
    if (e->lora->active == adapter) return ze_fail(e, ZE_ERR_INVALID, "the adapter is active: activate another one (or -1) first");
    hipSetDevice(e->device);
    ze_lora_adapter& ad = e->lora->ad[adapter];
    for (auto& kv : ad.t) free_tensor(kv.second);
    ad.t.clear();
    ad.used = false;
    return ZE_OK;
}

extern "C" int ze_lora_activate(ze_engine* e, int adapter, void* stream) {
    if (!e) return ze_fail(e, ZE_ERR_INVALID, "null engine");
    if (adapter != -1) ZE_TRY(check_adapter(e, adapter));
    ze_lora* l = e->lora;
    if (!l || adapter == l->active) return ZE_OK;
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    // what is not in the base store yet holds its base bits in the arena (the invariant above)
    for (const auto& ad : l->ad)
        for (const auto& kv : ad.t) {
            if (!ad.used || l->store.count(kv.first)) continue;
            const ze_dest& d = e->dests.at(kv.first);
            bf16_t* p = nullptr;
            const size_t bytes = (size_t)d.rows * d.cols * sizeof(bf16_t);
            if (hipMalloc((void**)&p, bytes) != hipSuccess) {
                hipGetLastError();
                return ze_fail(e, ZE_ERR_NOMEM, "LoRA: the base store allocation failed");
            }
            l->store[kv.first] = p;
            l->store_bytes += bytes;
            ze_launch_lora_snapshot(d.dst, d.ld, d.mode, d.offset, p, d.rows, d.cols, s);
        }
    static const std::map<std::string, ze_lora_tensor> none;
    const auto& was = l->active >= 0 ? l->ad[l->active].t : none;
    const auto& now = adapter >= 0 ? l->ad[adapter].t : none;
    for (const auto& kv : was)
        if (!now.count(kv.first)) {
            const ze_dest& d = e->dests.at(kv.first);
            ze_launch_lora_merge(l->store.at(kv.first), d.rows, d.cols, nullptr, nullptr, 0, 0.f, d.dst, d.ld, d.mode, d.offset, s);
        }
    for (const auto& kv : now) {
        const ze_dest& d = e->dests.at(kv.first);
        const ze_lora_tensor& t = kv.second;
        ze_launch_lora_merge(l->store.at(kv.first), d.rows, d.cols, t.A, t.B, t.r, t.scale, d.dst, d.ld, d.mode, d.offset, s);
    }
    l->active = adapter;
    ze_weights_changed(e);
    ZE_KCHECK();
    ZE_HIP(hipStreamSynchronize(s));
    return ZE_OK;
}

extern "C" int ze_lora_info(ze_engine* e, int* active, int* n_resident, size_t* base_store_bytes) {
    if (!e) return ze_fail(e, ZE_ERR_INVALID, "null engine");
    const ze_lora* l = e->lora;
    int n = 0;
    if (l)
        for (const auto& ad : l->ad) n += ad.used;
    if (active) *active = l ? l->active : -1;
    if (n_resident) *n_resident = n;
    if (base_store_bytes) *base_store_bytes = l ? l->store_bytes : 0;
    return ZE_OK;
}

extern "C" int ze_op_lora_merge(ze_engine* e, const void* base_bf16, int rows, int cols, const float* A, const float* B, int r, float scale,
                                void* dst_bf16, int ld, int mode, int offset, void* stream) {
    if (!e || !base_bf16 || !dst_bf16) return ze_fail(e, ZE_ERR_INVALID, "null argument");
    if (rows <= 0 || cols <= 0 || ld < cols || offset < 0 || (mode != 0 && mode != 1))
        return ze_fail(e, ZE_ERR_INVALID, "lora merge: rows, cols > 0, ld >= cols, offset >= 0, mode 0 or 1");
    if (r < 0 || r > ZE_LORA_MAX_RANK || (r > 0 && (!A || !B))) return ze_fail(e, ZE_ERR_INVALID, "lora merge: 0 <= r <= 128, A and B for r > 0");
    hipSetDevice(e->device);
    ze_launch_lora_merge((const bf16_t*)base_bf16, rows, cols, A, B, r, scale, (bf16_t*)dst_bf16, ld, mode, offset, (hipStream_t)stream);
    ZE_KCHECK();
    return ZE_OK;
}

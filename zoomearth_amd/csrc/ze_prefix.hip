// Prefix cache (ze_prefix_*): a pool of K/V blocks that outlives the chains whose rows it holds.  A block is `block_rows` consecutive
// cached rows of one chain for every layer and KV head, K and V both; WHAT a block holds is the caller's knowledge (keys, allocation
// and eviction live in zoomearth_amd/prefix_cache.py) -- the engine stores and returns bits, orders the copies between streams and
// knows which blocks were saved under the weights it has now.
//
// Pool layout: [n_blocks][layers][kv_heads][K|V][block_rows][head_dim] bf16.  One (layer, kv head, K|V) run of a block is block_rows *
// head_dim * 2 bytes in a row here AND in the slot cache ([layers][max_seqs][kv_heads][max_ctx][head_dim]: consecutive rows of one
// head are consecutive bytes), so both kernels move whole 16-byte pieces and a wave's 64 lanes touch 1 KiB in a row on either side.
#include "ze_engine.h"

#include <algorithm>

// Both kernels: blockIdx.y = (layer, kv head, K|V) picks the run, as in k_kv_fork; blockIdx.x strides over the pieces of that run of
// ALL the call's blocks (piece i of the slot side belongs to block ids[i / ppr], ppr = pieces per run of one block).

// rows [row0, row0 + nb * block_rows) of chain `seq` -> the nb blocks ids[0 .. nb): n_vec = nb * ppr pieces per run
__global__ void __launch_bounds__(256) k_kv_save(const bf16_t* __restrict__ kcache, const bf16_t* __restrict__ vcache, size_t layer_stride,
                                                 size_t seq_stride, size_t head_stride, int kv_heads, int seq, int piece0,
                                                 uint4* __restrict__ pool, const int* __restrict__ ids, int ppr, int n_vec) {
    const int y = blockIdx.y, runs = gridDim.y, step = gridDim.x * 256;
    const int which = y & 1, kvh = (y >> 1) % kv_heads, layer = (y >> 1) / kv_heads;
    const bf16_t* base = (which ? vcache : kcache) + (size_t)layer * layer_stride + (size_t)seq * seq_stride + (size_t)kvh * head_stride;
    const uint4* s = reinterpret_cast<const uint4*>(base) + piece0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_vec; i += step) {
        const int j = i / ppr, w = i - j * ppr;
        pool[((size_t)ids[j] * runs + y) * ppr + w] = s[i];
    }
}

// the first n_vec pieces per run of the blocks ids[0 .. ) -> rows from 0 on of the n chains dst[0 .. n): every piece is loaded once
// and stored n times; n_vec may end inside the last block, whose remaining rows are not touched in any destination
__global__ void __launch_bounds__(256) k_kv_load(bf16_t* __restrict__ kcache, bf16_t* __restrict__ vcache, size_t layer_stride,
                                                 size_t seq_stride, size_t head_stride, int kv_heads, const uint4* __restrict__ pool,
                                                 const int* __restrict__ ids, const int* __restrict__ dst, int n, int ppr, int n_vec) {
    const int y = blockIdx.y, runs = gridDim.y, step = gridDim.x * 256;
    const int which = y & 1, kvh = (y >> 1) % kv_heads, layer = (y >> 1) / kv_heads;
    bf16_t* base = (which ? vcache : kcache) + (size_t)layer * layer_stride + (size_t)kvh * head_stride;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_vec; i += step) {
        const int j = i / ppr, w = i - j * ppr;
        const uint4 v = pool[((size_t)ids[j] * runs + y) * ppr + w];
        for (int k = 0; k < n; ++k) reinterpret_cast<uint4*>(base + (size_t)dst[k] * seq_stride)[i] = v;
    }
}

// (the x-extent is k_kv_fork's: the runs share about 2048 workgroups, at most 16 each)
void ze_launch_kv_save(const bf16_t* kcache, const bf16_t* vcache, size_t layer_stride, size_t seq_stride, size_t head_stride, int layers,
                       int kv_heads, int D, int seq, int row0, bf16_t* pool, const int* ids_dev, int nb, int block_rows, hipStream_t s) {
    if (nb <= 0) return;
    const int per_row = D * 2 / 16, ppr = block_rows * per_row, n_vec = nb * ppr, runs = layers * kv_heads * 2;
    k_kv_save<<<dim3(ze_kv_fork_blocks(runs, n_vec), runs), 256, 0, s>>>(kcache, vcache, layer_stride, seq_stride, head_stride, kv_heads, seq,
                                                                         row0 * per_row, reinterpret_cast<uint4*>(pool), ids_dev, ppr, n_vec);
}

void ze_launch_kv_load(bf16_t* kcache, bf16_t* vcache, size_t layer_stride, size_t seq_stride, size_t head_stride, int layers, int kv_heads,
                       int D, const bf16_t* pool, const int* ids_dev, int block_rows, const int* dst_dev, int n, int n_rows, hipStream_t s) {
    if (n <= 0 || n_rows <= 0) return;
    const int per_row = D * 2 / 16, ppr = block_rows * per_row, n_vec = n_rows * per_row, runs = layers * kv_heads * 2;
    k_kv_load<<<dim3(ze_kv_fork_blocks(runs, n_vec), runs), 256, 0, s>>>(kcache, vcache, layer_stride, seq_stride, head_stride, kv_heads,
                                                                         reinterpret_cast<const uint4*>(pool), ids_dev, dst_dev, n, ppr, n_vec);
}

// ================================================================== the pool
// Stream order.  Saves and loads are numbered; the last ZE_PREFIX_RING calls of each kind keep an event recorded behind their kernel
// (an entry is reused only once its event is over, so a call that has left the ring has completed).  Every save waits for the save
// before it and every load for the load before it -- each kind has ONE device id list, and the chain of waits makes "the latest" stand
// for "all": a load then waits for the latest save among its blocks, a save for the latest load that reads one of its blocks.
static hipEvent_t ring_event(const std::vector<ze_prefix_pool::call>& ring, uint64_t seq) {
    if (seq == 0) return nullptr;
    const ze_prefix_pool::call& c = ring[seq % ring.size()];
    return c.seq == seq ? c.ev : nullptr;
}
static void ring_wait(const std::vector<ze_prefix_pool::call>& ring, uint64_t seq, hipStream_t s) {
    if (hipEvent_t ev = ring_event(ring, seq)) hipStreamWaitEvent(s, ev, 0);
}
static int ring_record(ze_engine* e, std::vector<ze_prefix_pool::call>& ring, uint64_t seq, hipStream_t s) {
    ze_prefix_pool::call& c = ring[seq % ring.size()];
    if (c.seq != 0) ZE_HIP(hipEventSynchronize(c.ev));  // (the call ZE_PREFIX_RING calls ago: over long since)
    c.seq = seq;
    ZE_HIP(hipEventRecord(c.ev, s));
    return ZE_OK;
}

static void pool_free(ze_prefix_pool* p) {
    if (!p) return;
    for (auto* ring : {&p->saves, &p->loads})
        for (auto& c : *ring)
            if (c.ev) hipEventDestroy(c.ev);
    if (p->data) hipFree(p->data);
    if (p->ids_save) hipFree(p->ids_save);
    if (p->ids_load) hipFree(p->ids_load);
    delete p;
}

void ze_prefix_pool_free(ze_engine* e) {
    pool_free(e->prefix_pool);
    e->prefix_pool = nullptr;
}

extern "C" int ze_prefix_pool_create(ze_engine* e, int n_blocks, int block_rows) {
    if (!e) return ze_fail(e, ZE_ERR_INVALID, "null engine");
    if (e->prefix_pool) return ze_fail(e, ZE_ERR_INVALID, "the engine already has a prefix pool");
    const ze_config& c = e->cfg;
    if (n_blocks <= 0 || block_rows <= 0 || block_rows % 8 || block_rows > c.max_ctx)
        return ze_fail(e, ZE_ERR_INVALID, "prefix pool: n_blocks > 0, block_rows a multiple of 8 and at most max_ctx");
    hipSetDevice(e->device);
    ze_prefix_pool* p = new ze_prefix_pool;
    p->n_blocks = n_blocks, p->block_rows = block_rows;
    p->block_elems = (size_t)c.layers * c.kv_heads * 2 * block_rows * e->head_dim;
    p->ids_cap = (c.max_ctx + block_rows - 1) / block_rows;
    bool ok = hipMalloc((void**)&p->data, p->block_elems * (size_t)n_blocks * sizeof(bf16_t)) == hipSuccess &&
              hipMalloc((void**)&p->ids_save, (size_t)p->ids_cap * sizeof(int)) == hipSuccess &&
              hipMalloc((void**)&p->ids_load, (size_t)(p->ids_cap + c.max_seqs) * sizeof(int)) == hipSuccess;
    p->saves.resize(ZE_PREFIX_RING), p->loads.resize(ZE_PREFIX_RING);
    for (auto* ring : {&p->saves, &p->loads})
        for (auto& call : *ring) ok = ok && hipEventCreateWithFlags(&call.ev, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        hipGetLastError();  // (the engine stays usable: the failure is not left behind for the next kernel check)
        pool_free(p);
        return ze_fail(e, ZE_ERR_NOMEM, "prefix pool: the device allocation failed");
    }
    p->saved_gen.assign(n_blocks, 0), p->saved_seq.assign(n_blocks, 0), p->read_seq.assign(n_blocks, 0);
    e->prefix_pool = p;
    return ZE_OK;
}

extern "C" int ze_prefix_pool_destroy(ze_engine* e) {
    if (!e) return ze_fail(e, ZE_ERR_INVALID, "null engine");
    if (!e->prefix_pool) return ZE_OK;
    hipSetDevice(e->device);
    for (auto* ring : {&e->prefix_pool->saves, &e->prefix_pool->loads})   // nothing may still read or write the pool
        for (auto& c : *ring)
            if (c.seq != 0) hipEventSynchronize(c.ev);
    ze_prefix_pool_free(e);
    return ZE_OK;
}

extern "C" int ze_prefix_pool_info(ze_engine* e, int* n_blocks, int* block_rows, unsigned* generation) {
    if (!e) return ze_fail(e, ZE_ERR_INVALID, "null engine");
    const ze_prefix_pool* p = e->prefix_pool;
    if (n_blocks) *n_blocks = p ? p->n_blocks : 0;
    if (block_rows) *block_rows = p ? p->block_rows : 0;
    if (generation) *generation = e->prefix_generation;
    return ZE_OK;
}

extern "C" int ze_prefix_save(ze_engine* e, int seq, int row0, const int32_t* blocks, int n, void* stream) {
    if (!e) return ze_fail(e, ZE_ERR_INVALID, "null engine");
    ze_prefix_pool* p = e->prefix_pool;
    if (!p) return ze_fail(e, ZE_ERR_INVALID, "the engine has no prefix pool");
    if (!blocks || n <= 0) return ze_fail(e, ZE_ERR_INVALID, "prefix save needs a list of n > 0 blocks");
    ZE_TRY(check_seq(e, seq));
    for (int i = 0; i < n; ++i)
        if (blocks[i] < 0 || blocks[i] >= p->n_blocks) return ze_fail(e, ZE_ERR_NOTFOUND, "prefix block id out of range");
    if (row0 < 0 || row0 % p->block_rows) return ze_fail(e, ZE_ERR_INVALID, "row0 is not a multiple of block_rows");
    if ((long long)row0 + (long long)n * p->block_rows > e->ctx_host[seq])
        return ze_fail(e, ZE_ERR_INVALID, "prefix save: the rows reach past the chain's context");
    {
        std::vector<int32_t> sorted(blocks, blocks + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return ze_fail(e, ZE_ERR_INVALID, "a prefix block appears twice");
    }
    const ze_config& c = e->cfg;
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    uint64_t readers = 0;
    for (int i = 0; i < n; ++i) readers = std::max(readers, p->read_seq[blocks[i]]);
    ring_wait(p->saves, p->n_saves, s);   // the id list, and any earlier save into these blocks
    ring_wait(p->loads, readers, s);      // the loads still reading them
    ze_launch_set_ints(p->ids_save, blocks, n, s);
    const size_t head_stride = (size_t)c.max_ctx * e->head_dim, seq_stride = (size_t)c.kv_heads * head_stride;
    ze_launch_kv_save(e->kcache, e->vcache, (size_t)c.max_seqs * seq_stride, seq_stride, head_stride, c.layers, c.kv_heads, e->head_dim, seq,
                      row0, p->data, p->ids_save, n, p->block_rows, s);
    ZE_KCHECK();
    ZE_TRY(ring_record(e, p->saves, ++p->n_saves, s));
    for (int i = 0; i < n; ++i) p->saved_gen[blocks[i]] = e->prefix_generation, p->saved_seq[blocks[i]] = p->n_saves;
    return ZE_OK;
}

extern "C" int ze_prefix_load(ze_engine* e, const int32_t* blocks, int n_blocks, int n_rows, int split_row, const int32_t* dst_seqs, int n,
                              void* stream) {
    if (!e) return ze_fail(e, ZE_ERR_INVALID, "null engine");
    ze_prefix_pool* p = e->prefix_pool;
    if (!p) return ze_fail(e, ZE_ERR_INVALID, "the engine has no prefix pool");
    if (!blocks || n_blocks <= 0 || !dst_seqs || n <= 0) return ze_fail(e, ZE_ERR_INVALID, "prefix load needs n_blocks > 0 blocks and n > 0 destination chains");
    for (int i = 0; i < n; ++i) {
        ZE_TRY(check_seq(e, dst_seqs[i]));
        for (int j = 0; j < i; ++j)
            if (dst_seqs[j] == dst_seqs[i]) return ze_fail(e, ZE_ERR_INVALID, "a destination chain appears twice");
    }
    for (int i = 0; i < n_blocks; ++i)
        if (blocks[i] < 0 || blocks[i] >= p->n_blocks) return ze_fail(e, ZE_ERR_NOTFOUND, "prefix block id out of range");
    const long long cap = (long long)n_blocks * p->block_rows;
    if (n_rows <= 0 || n_rows > cap || n_rows <= cap - p->block_rows || n_rows > e->cfg.max_ctx)
        return ze_fail(e, ZE_ERR_INVALID, "prefix load: n_rows must end inside the last block (and within max_ctx)");
    if (split_row < 0 || split_row > n_rows || split_row >= 65536) return ze_fail(e, ZE_ERR_INVALID, "split row out of range");
    uint64_t writer = 0;
    for (int i = 0; i < n_blocks; ++i) {
        if (p->saved_gen[blocks[i]] != e->prefix_generation)
            return ze_fail(e, ZE_ERR_INVALID, "a prefix block was not saved under the engine's current weights");
        writer = std::max(writer, p->saved_seq[blocks[i]]);
    }
    const ze_config& c = e->cfg;
    hipSetDevice(e->device);
    hipStream_t s = (hipStream_t)stream;
    ring_wait(p->loads, p->n_loads, s);   // the id list
    ring_wait(p->saves, writer, s);       // the saves that wrote these blocks
    // (block ids, then destination slots, as ONE table: one ze_launch_set_ints for both)
    std::vector<int> table(blocks, blocks + n_blocks);
    table.insert(table.end(), dst_seqs, dst_seqs + n);
    ze_launch_set_ints(p->ids_load, table.data(), n_blocks + n, s);
    const size_t head_stride = (size_t)c.max_ctx * e->head_dim, seq_stride = (size_t)c.kv_heads * head_stride;
    ze_launch_kv_load(e->kcache, e->vcache, (size_t)c.max_seqs * seq_stride, seq_stride, head_stride, c.layers, c.kv_heads, e->head_dim,
                      p->data, p->ids_load, p->block_rows, p->ids_load + n_blocks, n, n_rows, s);
    ZE_KCHECK();
    ZE_TRY(ring_record(e, p->loads, ++p->n_loads, s));
    for (int i = 0; i < n_blocks; ++i) p->read_seq[blocks[i]] = p->n_loads;
    // the destinations: dst_seqs[0] as a prefill of these rows leaves a chain, the others as ze_seq_copy_prefix from it does
    const int first = dst_seqs[0];
    for (int i = 0; i < n; ++i) {
        const int d = dst_seqs[i];
        e->ctx_host[d] = n_rows;
        e->delta_host[d] = 0;
        e->logits_fresh[d] = 0;
        e->split_host[d] = split_row;
        prefix_source_gone(e, d, 0);
        if (!e->pfx_copy_ev[d]) ZE_HIP(hipEventCreateWithFlags(&e->pfx_copy_ev[d], hipEventDisableTiming));
        ZE_HIP(hipEventRecord(e->pfx_copy_ev[d], s));  // (a holder other chains may be pointed at only once this is over)
        e->pfx_host[d] = (i > 0 && e->prefix_hints && n_rows < 65536) ? ((first << 16) | n_rows) : 0;
        ZE_HIP(hipMemsetAsync(e->seen + (size_t)d * c.vocab, 0, c.vocab, s));
        ze_requests_clear(e, d, s);
        ZE_TRY(push_state(e, d, s, 0, 0, 0));
    }
    return ZE_OK;
}

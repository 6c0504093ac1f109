// Stand-alone CPU program over zoomearth_amd/csrc/ze_tiff_codec.h -- the state machines the device kernels run -- for AddressSanitizer
// and UBSan (g++ -fsanitize=address,undefined; run directly).  It decodes a file of chunks
//     u32 count, then per chunk: u32 compression, u32 input bytes, u32 output bytes, the input
// and writes per chunk: i32 status, the output buffer (output bytes long, whatever the status).  Every input lives in a heap block of
// exactly its size, so a read past the chunk is the sanitizer's to report; every output lies between guard bytes that are checked
// here.  The emits are performed with the byte loop of the kernels' copy: out[dst + i] = out[src + i mod (dst - src)].
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ze_tiff_codec.h"

static const size_t GUARD = 64;

static int decode(uint32_t compression, const uint8_t* in, uint32_t in_len, uint8_t* out, uint32_t out_len) {
    zt_emit e;
    uint64_t passes = 0;
    if (compression == ZT_COMPRESSION_LZW) {
        std::vector<uint32_t> table(ZT_LZW_CODES, 0xffffffffu);
        zt_lzw s;
        zt_lzw_init(s, in, in_len, out_len);
        while (zt_lzw_step(s, table.data(), e)) {
            if (++passes > (uint64_t)in_len + 1) return -100;  // more emits than input bytes: the loop bound is broken
            if (e.dst + e.len > out_len || (e.kind == ZT_EMIT_COPY && e.src >= e.dst)) return -101;
            const uint32_t d = e.dst - e.src;
            for (uint32_t i = 0; i < e.len; ++i) out[e.dst + i] = e.kind == ZT_EMIT_FILL ? (uint8_t)e.value : out[e.src + i % d];
        }
        return s.status;
    }
    if (compression == ZT_COMPRESSION_PACKBITS) {
        zt_packbits s;
        zt_packbits_init(s, in, in_len, out_len);
        while (zt_packbits_step(s, e)) {
            if (++passes > (uint64_t)in_len + 1) return -100;
            if (e.dst + e.len > out_len || (e.kind == ZT_EMIT_INPUT && e.src + e.len > in_len)) return -101;
            for (uint32_t i = 0; i < e.len; ++i) out[e.dst + i] = e.kind == ZT_EMIT_FILL ? (uint8_t)e.value : in[e.src + i];
        }
        return s.status;
    }
    return -102;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    uint32_t count = 0;
    if (fread(&count, 4, 1, fi) != 1) return 2;
    for (uint32_t c = 0; c < count; ++c) {
        uint32_t head[3];
        if (fread(head, 4, 3, fi) != 3) return 2;
        const uint32_t in_len = head[1], out_len = head[2];
        uint8_t* in = (uint8_t*)malloc(in_len ? in_len : 1);
        if (in_len && fread(in, 1, in_len, fi) != in_len) return 2;
        uint8_t* buf = (uint8_t*)malloc(out_len + 2 * GUARD);
        memset(buf, 0xA5, out_len + 2 * GUARD);
        const int32_t status = decode(head[0], in, in_len, buf + GUARD, out_len);
        for (size_t i = 0; i < GUARD; ++i)
            if (buf[i] != 0xA5 || buf[GUARD + out_len + i] != 0xA5) {
                fprintf(stderr, "chunk %u: a guard byte changed\n", c);
                return 3;
            }
        if (status < 0) {
            fprintf(stderr, "chunk %u: decoder invariant %d broken\n", c, status);
            return 4;
        }
        fwrite(&status, 4, 1, fo);
        fwrite(buf + GUARD, 1, out_len, fo);
        free(buf);
        free(in);
    }
    fclose(fi);
    if (fclose(fo) != 0) return 2;
    printf("tiff codec ok: %u chunks\n", count);
    return 0;
}

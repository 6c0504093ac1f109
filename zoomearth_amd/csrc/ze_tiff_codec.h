// TIFF LZW (compression 5) and PackBits (32773): the per-code state machines, for host and device.
//
// One chunk (a strip or a tile) is `in_len` compressed bytes that decode to exactly `out_len` bytes.  A step function consumes input and
// returns ONE emit -- "copy `len` bytes that the chunk's own output already holds at `src`", "write `len` bytes of `value`" or "copy `len`
// bytes of the input at `src`" -- and the caller performs it at `dst`: k_tiff_lzw / k_tiff_packbits (ze_tiff.hip) with the 64 lanes of a
// wave, the sanitizer program of tests/tiff_san with a byte loop.  Everything that decides what is read and written is here: the bit
// reader, the code-width rule, the table update, every bound and the status of the chunk.
//
// Bounds: the reader never takes a byte at or past in_len; an emit never passes out_len (dst + len <= out_len, checked before it is
// returned) and its source lies inside [0, dst) of the output or inside [0, in_len) of the input; every pass of a step's loop consumes at
// least 8 bits of input, so a chunk takes at most in_len passes whatever its bytes are.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define ZT_HD __host__ __device__ __forceinline__
#else
#define ZT_HD inline
#endif
// a wave-uniform value read through a vector path (LDS, a global load) goes back to a scalar register on the device
#if defined(__HIP_DEVICE_COMPILE__)
#define ZT_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define ZT_UNIFORM(x) ((uint32_t)(x))
#endif

// the status word of a chunk: 0, or its first defect
enum {
    ZT_OK = 0,            // decoded exactly out_len bytes
    ZT_IN_EXHAUSTED = 1,  // the input ended before the output was full
    ZT_BAD_CODE = 2,      // LZW: a code above the next free code (or a table code where only a literal can stand)
    ZT_OUT_OVERRUN = 3,   // the next string / run would pass the end of the chunk's output
    ZT_OUT_SHORT = 4,     // LZW: EOI before the output was full
    ZT_BAD_TABLE = 5      // the chunk's row of the chunk table does not fit the image, the input buffer or the limits below
};
enum { ZT_EMIT_COPY = 0, ZT_EMIT_FILL = 1, ZT_EMIT_INPUT = 2 };

#define ZT_COMPRESSION_LZW 5
#define ZT_COMPRESSION_PACKBITS 32773
// the LZW table packs (offset << 12 | length) of a string inside the chunk's output into one word: 4096 words = 16 KB of LDS per wave.
// A string is at most 3839 bytes (entry k is at most k - 256 long), an offset stays below 2^20.
#define ZT_MAX_CHUNK_OUT (1u << 20)
#define ZT_LZW_CODES 4096
#define ZT_INPUT_ALIGN 16  // a chunk's bytes start on a 16-byte boundary of the input buffer, which is a multiple of 16 long

struct zt_emit {
    uint32_t kind, dst, src, len, value;
};

// ---- input: a byte reader over [0, len) that fetches 16 aligned bytes at a time
struct zt_bytes {
    const uint8_t* in;
    uint32_t len, pos;
    uint64_t lo, hi;  // the 16 bytes at wbase (two words, not an array: the state stays in registers)
    uint32_t wbase;
};
ZT_HD void zt_bytes_init(zt_bytes& b, const uint8_t* in, uint32_t len) {
    b.in = in;
    b.len = len;
    b.pos = 0;
    b.wbase = 0xffffffffu;
    b.lo = b.hi = 0;
}
// the byte at `pos` (pos < len is the caller's to have checked)
ZT_HD uint32_t zt_byte_at(zt_bytes& b, uint32_t pos) {
    const uint32_t base = pos & ~15u;
    if (base != b.wbase) {
#if defined(__HIP_DEVICE_COMPILE__)
        // the piece may reach past len, never past the 16-byte multiple the buffer is long (ZT_INPUT_ALIGN; checked with the table row)
        const uint4 v = *(const uint4*)(b.in + base);
        b.lo = (uint64_t)ZT_UNIFORM(v.x) | ((uint64_t)ZT_UNIFORM(v.y) << 32);
        b.hi = (uint64_t)ZT_UNIFORM(v.z) | ((uint64_t)ZT_UNIFORM(v.w) << 32);
#else
        const uint32_t n = b.len - base < 16 ? b.len - base : 16;  // the host reads the chunk's own bytes only (the sanitizer's bound)
        uint8_t w[16] = {0};
        memcpy(w, b.in + base, n);
        b.lo = b.hi = 0;
        for (int i = 0; i < 8; ++i) b.lo |= (uint64_t)w[i] << (8 * i), b.hi |= (uint64_t)w[8 + i] << (8 * i);
#endif
        b.wbase = base;
    }
    const uint32_t k = pos & 15u;
    return (uint32_t)((k < 8 ? b.lo : b.hi) >> ((k & 7u) * 8u)) & 255u;
}

// ---- LZW (TIFF 6.0: MSB-first codes, ClearCode 256, EOI 257, first free code 258, 9 .. 12 bits, the width rises one code early)
struct zt_lzw {
    zt_bytes b;
    uint32_t bits, nbits;          // the bit buffer: the low nbits of `bits` are the next bits of the stream, MSB first
    uint32_t out_pos, out_len;
    uint32_t width, next;          // the code width and the next free code (4096 = the table is full: nothing more is added)
    uint32_t prev_off, prev_len;   // the string of the previous code, inside the output
    uint32_t have_prev;            // 0 at the start and behind a ClearCode: the next code is a literal and adds no entry
    int status;
};
ZT_HD void zt_lzw_init(zt_lzw& s, const uint8_t* in, uint32_t in_len, uint32_t out_len) {
    zt_bytes_init(s.b, in, in_len);
    s.bits = s.nbits = 0;
    s.out_pos = 0;
    s.out_len = out_len;
    s.width = 9;
    s.next = 258;
    s.prev_off = s.prev_len = s.have_prev = 0;
    s.status = ZT_OK;
}
// The next code, or -1 when fewer than `width` bits are left.
ZT_HD int zt_lzw_code(zt_lzw& s) {
    while (s.nbits < s.width) {  // at most two passes: width <= 12
        if (s.b.pos >= s.b.len) return -1;
        s.bits = ((s.bits << 8) | zt_byte_at(s.b, s.b.pos)) & 0xfffffu;  // nbits < 12 before, at most 19 bits behind
        s.b.pos++;
        s.nbits += 8;
    }
    s.nbits -= s.width;
    return (int)((s.bits >> s.nbits) & ((1u << s.width) - 1u));
}
// One emit of the stream into `e` (returns 1), or the end of the chunk (returns 0, s.status says how).  `table`: ZT_LZW_CODES words
// that belong to this chunk alone (LDS on the device); entries below 258 are never touched.
ZT_HD int zt_lzw_step(zt_lzw& s, uint32_t* table, zt_emit& e) {
    for (;;) {  // every pass takes `width` >= 9 bits of input or ends the chunk
        if (s.out_pos == s.out_len) {
            s.status = ZT_OK;  // full: libtiff stops here too, with or without an EOI behind
            return 0;
        }
        const int code = zt_lzw_code(s);
        if (code < 0) {
            s.status = ZT_IN_EXHAUSTED;
            return 0;
        }
        if (code == 257) {
            s.status = ZT_OUT_SHORT;
            return 0;
        }
        if (code == 256) {
            s.width = 9;
            s.next = 258;
            s.have_prev = 0;
            continue;
        }
        uint32_t src = 0, len = 1;
        if (code >= 258) {
            if (!s.have_prev || (uint32_t)code > s.next) {
                s.status = ZT_BAD_CODE;  // (code == next is the KwKwK case; with a full table next is 4096, above every code)
                return 0;
            }
            if ((uint32_t)code < s.next) {
                const uint32_t t = ZT_UNIFORM(table[code]);
                src = t >> 12;
                len = t & 4095u;
            } else {  // KwKwK: the previous string and its own first byte -- the source runs into the destination
                src = s.prev_off;
                len = s.prev_len + 1;
            }
        }
        if (len > s.out_len - s.out_pos) {
            s.status = ZT_OUT_OVERRUN;
            return 0;
        }
        if (s.have_prev && s.next < ZT_LZW_CODES) {
            // the new string: the previous one and the first byte of this one, which is written right behind it
            table[s.next] = (s.prev_off << 12) | (s.prev_len + 1);
            s.next++;
            if (s.next + 1 >= (1u << s.width) && s.width < 12) s.width++;  // 9 -> 10 when the next free code reaches 511, ...
        }
        e.kind = code < 256 ? ZT_EMIT_FILL : ZT_EMIT_COPY;
        e.dst = s.out_pos;
        e.src = src;
        e.len = len;
        e.value = (uint32_t)code & 255u;
        s.prev_off = s.out_pos;
        s.prev_len = len;
        s.have_prev = 1;
        s.out_pos += len;
        return 1;
    }
}

// ---- PackBits: n in 0 .. 127 copies n + 1 input bytes, n in -127 .. -1 repeats the next byte 1 - n times, -128 does nothing
struct zt_packbits {
    zt_bytes b;
    uint32_t out_pos, out_len;
    int status;
};
ZT_HD void zt_packbits_init(zt_packbits& s, const uint8_t* in, uint32_t in_len, uint32_t out_len) {
    zt_bytes_init(s.b, in, in_len);
    s.out_pos = 0;
    s.out_len = out_len;
    s.status = ZT_OK;
}
ZT_HD int zt_packbits_step(zt_packbits& s, zt_emit& e) {
    for (;;) {  // every pass takes at least one byte of input or ends the chunk
        if (s.out_pos == s.out_len) {
            s.status = ZT_OK;
            return 0;
        }
        if (s.b.pos >= s.b.len) {
            s.status = ZT_IN_EXHAUSTED;
            return 0;
        }
        const uint32_t n = zt_byte_at(s.b, s.b.pos);
        s.b.pos++;
        if (n == 128) continue;
        const uint32_t len = n < 128 ? n + 1 : 257 - n;
        const uint32_t need = n < 128 ? len : 1;
        if (need > s.b.len - s.b.pos) {
            s.status = ZT_IN_EXHAUSTED;
            return 0;
        }
        if (len > s.out_len - s.out_pos) {
            s.status = ZT_OUT_OVERRUN;
            return 0;
        }
        e.dst = s.out_pos;
        e.len = len;
        if (n < 128) {
            e.kind = ZT_EMIT_INPUT;
            e.src = s.b.pos;
            e.value = 0;
        } else {
            e.kind = ZT_EMIT_FILL;
            e.src = 0;
            e.value = zt_byte_at(s.b, s.b.pos);
        }
        s.b.pos += need;
        s.out_pos += len;
        return 1;
    }
}

// ---- the chunk table: 8 int32 per chunk
// {input offset, input bytes, x0, y0, w, h of the destination rectangle, stored w, stored h}.  Strips (tiled = 0) decode in place: full
// width, stored = destination.  Tiles are stored at the tile size chunk_w x chunk_h, edge tiles padded, and clipped when placed.
#define ZT_TABLE_INTS 8
struct zt_chunk {
    int32_t off, len, x0, y0, w, h, sw, sh;
};
ZT_HD int zt_chunk_ok(const zt_chunk& t, uint64_t n_bytes, int h, int w, int tiled, int chunk_w, int chunk_h) {
    const int64_t off = t.off, len = t.len;
    const int x0 = t.x0, y0 = t.y0, cw = t.w, ch = t.h, sw = t.sw, sh = t.sh;
    if (off < 0 || len <= 0 || off % ZT_INPUT_ALIGN != 0 || (uint64_t)(off + len) > n_bytes) return 0;
    if (x0 < 0 || y0 < 0 || cw < 1 || ch < 1 || cw > w - x0 || ch > h - y0) return 0;
    if (tiled) {
        if (sw != chunk_w || sh != chunk_h || cw > sw || ch > sh) return 0;
    } else {
        if (x0 != 0 || cw != w || sw != w || sh != ch || sh > chunk_h) return 0;
    }
    return (uint64_t)sw * (uint64_t)sh * 3u <= ZT_MAX_CHUNK_OUT;
}

// The measurement knobs of ze_tune (include/zoomearth.h holds the table that describes them: one row per enumerator, same numbers).
// A knob at 0 is the shipped default; the named values below are the alternatives the launch rules compare against.
#pragma once

enum ze_knob {
    ZE_KNOB_GEMV_DOWN = 0,          // ZE_DOWN_*
    ZE_KNOB_GATE_UP_FLASH = 1,      // ZE_GATE_UP_* (single-chain gate/up GEMV) and ZE_FLASH_* (prefill / ViT flash attention)
    ZE_KNOB_GEMV_GRID_CAP = 2,      // a grid size
    ZE_KNOB_RING32_FROM = 3,        // a row count
    ZE_KNOB_P8_LAUNCH = 4,          // ZE_P8_*
    ZE_KNOB_SKINNY = 5,             // ZE_SKINNY_*
    ZE_KNOB_GEMM_STAGING = 6,       // ZE_STAGING_*
    ZE_KNOB_GEMM_TILE = 7,          // ZE_TILE_*
    ZE_KNOB_BATCH_ATTN = 8,         // ZE_ATTN_*
    ZE_KNOB_O_SKINNY = 9,           // ZE_KNOB_ON
    ZE_KNOB_BF16_FRAGMENTS = 10,    // ZE_KNOB_ON
    ZE_KNOB_RING_ATTN_PART = 11,    // keys per part
    ZE_KNOB_PREFILL_BF16_GEMM = 12, // ZE_KNOB_ON
    ZE_KNOB_WIDE_DECODE = 13,       // ZE_WIDE_*
    ZE_KNOB_SEPARATE_ARGMAX = 14,   // ZE_KNOB_ON
    ZE_KNOB_WIDE_TILES = 15,        // ZE_WT_*
    ZE_KNOB_ATTN_ROTATION = 16,     // step | shift << 4
    ZE_KNOB_NO_PREFIX_HINTS = 17,   // ZE_KNOB_ON
    ZE_KNOB_KSTEP32 = 18,           // ZE_KNOB_ON
    ZE_KNOB_TALL_RING = 19,         // ZE_TALL_PLAIN_RING
    ZE_KNOB_PREFILL_KSPLIT = 20,    // ZE_PREFILL_KSPLIT_3
    ZE_KNOB_P8_WALK = 21,           // ZE_KNOB_ON: the column walk; > 1: R << 8 | C blocks
    ZE_KNOB_MROPE_Q_IN_PLACE = 22,  // ZE_KNOB_ON
    ZE_KNOB_ATTN_SPLIT = 23,        // ZE_SPLIT_*
    ZE_KNOB_MX4_BF16_FRAGMENTS = 24,  // ZE_KNOB_ON
    ZE_KNOB_COUNT = 25
};
extern int ze_knobs[ZE_KNOB_COUNT];  // defined in ze_gemv.hip, written by ze_tune (ze_weights.hip) alone

enum { ZE_KNOB_ON = 1 };  // the one alternative of a two-way knob
enum { ZE_DOWN_TWO_PAIRS = 1, ZE_DOWN_FOUR_CHUNKS = 2, ZE_DOWN_NO_KSPLIT = 3 };
enum { ZE_GATE_UP_TWO_PAIRS = 1, ZE_GATE_UP_ONE_PAIR = 2, ZE_FLASH_REG_STAGED = 7, ZE_FLASH_BQ64 = 9 };
enum { ZE_P8_TILE_PER_WG = 1, ZE_P8_PERSISTENT = 2 };
enum { ZE_SKINNY_OFF = 1, ZE_SKINNY_GRID32 = 2 };
enum { ZE_STAGING_REGISTERS = 1, ZE_STAGING_RING = 2 };
enum { ZE_TILE_REG_ONLY = 3, ZE_TILE_256 = 4, ZE_TILE_128X256 = 6, ZE_TILE_P8 = 8, ZE_TILE_P8_PER_TILE = 9, ZE_TILE_PLAIN_EPILOGUE = 10 };
enum { ZE_ATTN_SLICE = 1, ZE_ATTN_RING = 2, ZE_ATTN_PLAIN_GRID = 3, ZE_ATTN_PART192 = 4 };
enum { ZE_WIDE_STREAM = 1, ZE_WIDE_QKV_PAIR = 2, ZE_WIDE_TILES_257 = 3, ZE_WIDE_NO_TALL = 4 };
enum { ZE_WT_WSTREAM = 1, ZE_WT_WSTREAM_TILES = 4, ZE_WT_BLOCKS_256 = 5, ZE_WT_ONE_LAUNCH = 6, ZE_WT_NO_TWO_ROW_TILES = 7,
       ZE_WT_WSTREAM_385_512 = 8, ZE_WT_PLAIN = 9 };
enum { ZE_TALL_PLAIN_RING = 4, ZE_PREFILL_KSPLIT_3 = 3 };
enum { ZE_SPLIT_ROWS = 2, ZE_SPLIT_PAIRED = 3 };

// segs_class.h -- the one classification of a segment of the segmented sort
// (misort_local_sort_segments) by its length, and the layout of the header the
// count kernel fills.  Included by the host (runtime.cpp: misort_segment_class,
// the launch loop) and by the kernels (segs.hip, segs_tile.h): one definition.
//
// A segment of len keys is sorted as a block of 2^class keys, the rest of the
// block all-ones:
//   len == 0                  -1: nothing to do;
//   1 <= len <= 2^tile_log2   max(ceil_log2(len), 5): the row tile's LR (a tile
//                             of 2^LT keys holds 2^(LT - LR) segments of the
//                             class; up to 32 keys are one lane's registers);
//   longer                    ceil_log2(len): the k of the padded blocks.
// For every len >= 2 this is rows_plan(len, key_bytes)'s path and block.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MISORT_HD __host__ __device__
#else
#define MISORT_HD
#endif

namespace misort {

constexpr int SEG_LR_MIN = 5;     // ROWS_LR_MIN (kernels.h)
constexpr int SEG_CLASSES = 64;   // classes 0..63; 5..62 occur

// log2 of the largest SORT tile: KT<K>::LT of bitonic.h (asserted in segs_tile.h)
MISORT_HD constexpr int seg_tile_log2(int key_bytes) { return key_bytes == 4 ? 15 : 13; }

MISORT_HD inline int segment_class(int64_t len, int key_bytes) {
    if (len <= 0) return -1;
    int cl = len > 1 ? 64 - __builtin_clzll((unsigned long long)(len - 1)) : 0;  // ceil_log2
    if (cl > 62) cl = 62;
    if (len <= ((int64_t)1 << seg_tile_log2(key_bytes)) && cl < SEG_LR_MIN) cl = SEG_LR_MIN;
    return cl;
}

// The header: 64-bit words at the start of the context's segment buffer, zeroed
// before the count kernel.  The class lists (32-bit segment indices, class after
// class) follow at SEG_LIST_BYTES.
enum SegHeader : int {
    SEG_H_COUNT = 0,                        // [class] segments of the class
    SEG_H_KEYS = SEG_CLASSES,               // [class] keys in them
    SEG_H_FIRST = 2 * SEG_CLASSES,          // offsets[0]
    SEG_H_LAST = SEG_H_FIRST + 1,           // offsets[nseg]
    SEG_H_BAD = SEG_H_FIRST + 2,            // malformed segments
    SEG_H_BAD_AT = SEG_H_FIRST + 3,         // ~(the first malformed index); 0: none
    SEG_H_FETCH = SEG_H_FIRST + 4,          // words the host reads
    SEG_H_CURSOR = SEG_H_FETCH,             // [class] next free slot of the class's list (host: its base)
    SEG_H_WORDS = SEG_H_CURSOR + SEG_CLASSES
};
constexpr int SEG_LIST_BYTES = 2048;
static_assert(SEG_H_WORDS * 8 <= SEG_LIST_BYTES, "the lists start after the header");

}  // namespace misort

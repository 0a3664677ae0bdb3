// topk_segs_plan.h -- what the segmented top-k (topk_segs.hip) does with a
// segment of a given length, host only: the runtime decides from it after the
// count kernel and misort_topk_segments_plan reports it.
//
// A segment's class is segment_class(len, 8) of segs_class.h (the records are 8
// bytes): -1 for an empty one, 5..13 up to the tile's 2^13 keys, ceil_log2(len)
// above.  Per class:
//   -1        nothing runs: the fill kernel writes the whole row;
//   5..13     ONE pass, keys -> outputs, a block of 2^class virtual records per
//             segment, m_out = min(len, k) real results (the fill writes the rest);
//   c >= 14   the passes of topk_plan(2^c, k): the segment is cut as a row of
//             2^c keys, P = 2^(c - 13) pieces of the tile, the keys past len
//             virtual.  Only the first pass knows of segments; the last writes
//             the outputs of segment list[r].
// Refused: k outside 1..2^13, a class >= 32 (a length above 2^31: a position
// must stay below 2^31, the fill index 0xFFFFFFFF is never real), and k > 2^10
// with any class >= 14 (topk_plan.h says why).
#pragma once
#include "segs_class.h"
#include "topk_plan.h"

namespace misort {

constexpr int64_t TOPK_SEGS_K_MAX = (int64_t)1 << TOPK_LT;  // a segment's results come from one tile
constexpr int TOPK_SEGS_CLASS_END = 32;  // class 32 holds the lengths 2^31 + 1 .. 2^32

enum TopkSegsRefusal : int {
    TOPK_SEGS_OK = 0,
    TOPK_SEGS_BAD_K = 1,      // k outside 1 .. 2^13
    TOPK_SEGS_TOO_LONG = 2,   // a segment longer than 2^31 keys
    TOPK_SEGS_K_LONG = 3      // k > 2^10 with a segment longer than 2^13 keys
};

inline bool topk_segs_k_ok(int64_t k) { return k >= 1 && k <= TOPK_SEGS_K_MAX; }

// Whether a non-empty class (cls = segment_class(len, 8), -1 for no segment) goes with k.
inline TopkSegsRefusal topk_segs_class_refusal(int cls, int64_t k) {
    if (!topk_segs_k_ok(k)) return TOPK_SEGS_BAD_K;
    if (cls >= TOPK_SEGS_CLASS_END) return TOPK_SEGS_TOO_LONG;
    if (cls > TOPK_LT && k > TOPK_K_LONG_MAX) return TOPK_SEGS_K_LONG;
    return TOPK_SEGS_OK;
}

// The passes of one class (cls >= 5) as topk_plan gives them for a row of 2^cls
// keys; up to max are written, the count is returned (-1: refused).
inline int topk_segs_class_plan(int cls, int64_t k, TopkPass* out, int max) {
    if (cls < SEG_LR_MIN || topk_segs_class_refusal(cls, k) != TOPK_SEGS_OK) return -1;
    if (cls <= TOPK_LT) {
        // one block per segment; k may exceed the block: min(len, k) results are real
        if (max > 0) out[0] = TopkPass{(int64_t)1 << cls, cls, 1, k};
        return 1;
    }
    return topk_plan((int64_t)1 << cls, k, out, max);
}

// The passes of one segment of len keys: 0 for an empty one, one for len <= 2^13
// (m_in = len, m_out = min(len, k)), else the class's; -1 for a refused (len, k).
inline int topk_segs_plan(int64_t len, int64_t k, TopkPass* out, int max) {
    if (len < 0) return -1;
    const int cls = segment_class(len, 8);
    if (topk_segs_class_refusal(cls, k) != TOPK_SEGS_OK) return -1;
    if (cls < 0) return 0;
    const int np = topk_segs_class_plan(cls, k, out, max);
    if (np == 1 && cls <= TOPK_LT && max > 0) out[0].m_in = len, out[0].m_out = len < k ? len : k;
    return np;
}

}  // namespace misort

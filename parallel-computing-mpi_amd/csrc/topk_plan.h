// topk_plan.h -- the pass plan of the row-wise top-k (topk.hip), host only: the
// runtime runs it and misort_topk_plan reports it.
//
// A pass cuts every row of m_in records into npieces blocks of 2^lr virtual
// records, sorts every block in an LDS tile and keeps the first k records of
// each: m_out = npieces k records per row.  The first pass reads the caller's
// keys (m_in = cols), the later ones the candidates of the pass before.
//   m_in <= 2^13:  one block per row, lr = max(ceil_log2(m_in), 5): the LAST pass
//                  (m_out = k), which splits the records into the outputs;
//   else:          lr = 13, npieces = ceil(m_in / 2^13), candidates out.
// k <= 2^10 when cols > 2^13, so a pass over m_in > 2^13 records leaves
// ceil(m_in / 2^13) k <= m_in / 8 + 2^10 < m_in of them: the plan ends.  The
// longest one, cols = 2^31 with k = 2^10, has 7 passes (2^31, 2^28, 2^25, 2^22,
// 2^19, 2^16, 2^13 records); cols = 2^20 has 4, cols = 2^17 with k = 64 has 2.
#pragma once
#include <stdint.h>

namespace misort {

constexpr int TOPK_LT = 13;          // log2 records of the tile (the u64 SORT tile)
constexpr int TOPK_LR_MIN = 5;       // a block is at least a lane's 32 records
constexpr int64_t TOPK_COLS_MAX = (int64_t)1 << 31;  // a column index stays below 2^31
constexpr int64_t TOPK_K_LONG_MAX = (int64_t)1 << 10;  // k of rows longer than the tile
constexpr int TOPK_MAX_PASSES = 8;   // no plan is longer (see above)

struct TopkPass {
    int64_t m_in;     // records of a row the pass reads
    int lr;           // log2 virtual records of a block
    int64_t npieces;  // blocks of a row
    int64_t m_out;    // records of a row it leaves: npieces k
};

inline bool topk_shape_ok(int64_t cols, int64_t k) {
    return k >= 1 && k <= cols && cols <= TOPK_COLS_MAX && (cols <= ((int64_t)1 << TOPK_LT) || k <= TOPK_K_LONG_MAX);
}

// Writes up to max passes and returns the count, or -1 for a shape top-k does not take.
inline int topk_plan(int64_t cols, int64_t k, TopkPass* out, int max) {
    if (!topk_shape_ok(cols, k)) return -1;
    int n = 0;
    for (int64_t m = cols;; ++n) {
        TopkPass p;
        p.m_in = m;
        if (m <= ((int64_t)1 << TOPK_LT)) {
            int lr = TOPK_LR_MIN;
            while (((int64_t)1 << lr) < m) ++lr;
            p.lr = lr, p.npieces = 1;
        } else {
            p.lr = TOPK_LT, p.npieces = (m + ((int64_t)1 << TOPK_LT) - 1) >> TOPK_LT;
        }
        p.m_out = p.npieces * k;
        if (n < max) out[n] = p;
        if (p.npieces == 1) return n + 1;
        m = p.m_out;
    }
}

}  // namespace misort

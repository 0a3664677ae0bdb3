// rows_tile.h -- the row-wise SORT tile: every row of a row-major rows x cols
// array sorted on its own, cols <= 2^LT, in one HBM read and one write per key.
//
// Built on the SORT tile of bitonic.h.  In the flip formulation every aligned
// 2^m block of a tile is ascending after level m, so a tile that STOPS after
// level LR holds 2^(LT - LR) sorted blocks of 2^LR keys: one row each.  One
// level more would merge neighbouring rows.
//
// Index mapping: LR = max(ceil_log2(cols), ROWS_LR_MIN), a tile holds
// R = 2^(LT - LR) rows, and virtual key v of tile j is row j R + (v >> LR),
// column v & (2^LR - 1).  It reads in[row cols + col] when col < cols and
// row < rows, else the all-ones sentinel; a sentinel suffix of a 2^LR block can
// only move upwards inside its block (no compare-exchange of levels 1..LR
// leaves the block), so the first cols keys of the sorted block are the sorted
// row and only those are stored.  64-bit index arithmetic throughout.
//
// Levels 1..5 sort a lane's 32 consecutive keys in registers, u32 levels
// 6..min(LR, WAVE_LEVELS) run in the wave, the rest as LDS phases in the pad()
// layout with lds_range_w's barrier rule.  The top levels stay network phases
// (the shipped tile's merge-level top is not used here).  One tile per
// workgroup: a workgroup has read all its rows into LDS before it stores any
// and tiles own disjoint rows, so out == in is safe.
//
// Included by one translation unit per key type (rows_u32.hip, rows_u64.hip).
#pragma once
#include "bitonic.h"

namespace misort {

namespace {

// flags: bit 0 = 16-byte vector accesses (both pointers 16-byte aligned and
// cols a multiple of the vector: every vector lies inside one row, aligned);
// bit 1 = f64 keys (u64 only): ord_of_f64 on the real keys after the loads,
// f64_of_ord in the stores -- the sentinels stay all-ones.
constexpr int ROWS_VEC = 1, ROWS_F64 = 2;

template <typename K, int LT, int LR>
__global__ __launch_bounds__((TileGeo<K, LT>::NT), (TileGeo<K, LT>::WAVES_PER_EU)) void k_sort_rows(
    const K* in, K* out, int64_t rows, int64_t cols, int64_t tile0, int flags) {
    typedef TileGeo<K, LT> G;
    typedef typename KT<K>::vec vec_t;
    static_assert(LR >= ROWS_LR_MIN && LR <= LT, "a row block is a lane's 32 keys .. the tile");
    constexpr int CM = (1 << LR) - 1;
    __shared__ __attribute__((aligned(16))) K s[lds_words(G::T)];
    const int t = threadIdx.x;
    const int64_t row0 = (tile0 + blockIdx.x) << (LT - LR);  // the tile's first row
    const bool vec = flags & ROWS_VEC;
    const bool f64 = sizeof(K) == 8 && (flags & ROWS_F64);
    // every virtual key real and every vector aligned: no bounds checks
    const bool full = vec && cols == (int64_t)(CM + 1) && row0 + (1 << (LT - LR)) <= rows;
    K pre[G::LOADS][G::V];
#pragma unroll
    for (int k = 0; k < G::LOADS; ++k) {
        const int e = place<K, LT>(k, t);
        const int64_t r = row0 + (e >> LR);
        const int c = e & CM;
        const K* src = in + (r * cols + c);
        if (full) {
            const vec_t x = __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(src));
#pragma unroll
            for (int j = 0; j < G::V; ++j) pre[k][j] = f64 ? (K)ord_of_f64((uint64_t)x[j]) : x[j];
        } else if (vec) {
            const bool real = r < rows && c < cols;  // cols % V == 0: the whole vector or none of it
            vec_t x = {};
            if (real) x = *reinterpret_cast<const vec_t*>(src);
#pragma unroll
            for (int j = 0; j < G::V; ++j)
                pre[k][j] = !real ? KT<K>::MAX : f64 ? (K)ord_of_f64((uint64_t)x[j]) : x[j];
        } else {
#pragma unroll
            for (int j = 0; j < G::V; ++j) {
                const bool real = r < rows && c + j < cols;
                K x = KT<K>::MAX;
                if (real) x = src[j];
                pre[k][j] = real && f64 ? (K)ord_of_f64((uint64_t)x) : x;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < G::LOADS; ++k) {
        const int e = place<K, LT>(k, t);
#pragma unroll
        for (int j = 0; j < G::V; ++j) s[pad(e + j)] = pre[k][j];
    }
    __syncthreads();
    // levels the registers (and, u32, the wave) finish
    constexpr int DONE = sizeof(K) == 4 ? (LR < WAVE_LEVELS ? LR : WAVE_LEVELS) : 5;
    {
        K x[32];
        const int a0 = pad(t << 5);
#pragma unroll
        for (int c = 0; c < 32; ++c) x[c] = s[a0 + c];
        sort32_regs<K>(x);
        if constexpr (sizeof(K) == 4) wave_levels<6, DONE>(x, t & 63);
        // each lane rewrites only the keys it read
#pragma unroll
        for (int c = 0; c < 32; ++c) s[a0 + c] = x[c];
    }
    if constexpr (DONE < LR) {
        // level DONE + 1 <= WAVE_BITS stays inside the wave; the last phase of
        // level LR ends with a workgroup barrier (lds_range_w, NEXT_HI = -1)
        static_assert(DONE + 1 <= WAVE_BITS, "the first LDS level is wave-local");
        wave_sync();
        sort_levels_w<K, DONE + 1, LR>(s, t);
    } else {
        __syncthreads();  // the stores read other lanes' keys
    }
#pragma unroll
    for (int k = 0; k < G::LOADS; ++k) {
        const int e = place<K, LT>(k, t);
        const int64_t r = row0 + (e >> LR);
        const int c = e & CM;
        K* dst = out + (r * cols + c);
        K x[G::V];
#pragma unroll
        for (int j = 0; j < G::V; ++j) {
            x[j] = s[pad(e + j)];
            if (f64) x[j] = (K)f64_of_ord((uint64_t)x[j]);  // never stored where it is a sentinel
        }
        if (vec) {
            if (full || (r < rows && c < cols)) {
                vec_t v;
#pragma unroll
                for (int j = 0; j < G::V; ++j) v[j] = x[j];
                if (full) __builtin_nontemporal_store(v, reinterpret_cast<vec_t*>(dst));
                else *reinterpret_cast<vec_t*>(dst) = v;
            }
        } else {
#pragma unroll
            for (int j = 0; j < G::V; ++j)
                if (r < rows && c + j < cols) dst[j] = x[j];
        }
    }
}

template <typename K, int LT, int LR>
void launch_rows(const K* in, K* out, int64_t rows, int64_t cols, int flags, hipStream_t s) {
    const int64_t ntiles = (rows + (1 << (LT - LR)) - 1) >> (LT - LR);
    constexpr int64_t MAX_GRID = 0x7FFFFFFF;
    for (int64_t t0 = 0; t0 < ntiles; t0 += MAX_GRID) {
        const int64_t g = ntiles - t0 < MAX_GRID ? ntiles - t0 : MAX_GRID;
        k_sort_rows<K, LT, LR><<<dim3((unsigned)g), dim3(TileGeo<K, LT>::NT), 0, s>>>(in, out, rows, cols, t0, flags);
    }
}

// u32: the 2^14 tile (512 lanes, two workgroups per CU) up to LR = 14, the
// 2^15 tile (1024 lanes) for LR = 15 alone; u64: the 2^13 tile.
template <typename K>
bool launch_rows_lr(int lr, const K* in, K* out, int64_t rows, int64_t cols, int flags, hipStream_t s) {
    constexpr int LT = sizeof(K) == 4 ? SORT_LT_MERGE : KT<K>::LT;
    switch (lr) {
#define MISORT_ROWS_CASE(LR_) \
    case LR_:                 \
        if constexpr (LR_ <= LT) launch_rows<K, LT, LR_>(in, out, rows, cols, flags, s); \
        return LR_ <= LT
        MISORT_ROWS_CASE(5);
        MISORT_ROWS_CASE(6);
        MISORT_ROWS_CASE(7);
        MISORT_ROWS_CASE(8);
        MISORT_ROWS_CASE(9);
        MISORT_ROWS_CASE(10);
        MISORT_ROWS_CASE(11);
        MISORT_ROWS_CASE(12);
        MISORT_ROWS_CASE(13);
        MISORT_ROWS_CASE(14);
#undef MISORT_ROWS_CASE
    case 15:
        if constexpr (sizeof(K) == 4) launch_rows<K, SORT_LT_U32, 15>(in, out, rows, cols, flags, s);
        return sizeof(K) == 4;
    default:
        return false;
    }
}

}  // namespace

template <typename K>
hipError_t sort_rows_tile(const K* in, K* out, int64_t rows, int64_t cols, bool f64, hipStream_t s,
                          LaunchHook* hook) {
    if (rows <= 0 || cols <= 0) return hipSuccess;
    if ((sizeof(K) == 4 && f64) || cols > ((int64_t)1 << KT<K>::LT)) return hipErrorInvalidValue;
    const int cl = ceil_log2(cols);
    const int lr = cl < ROWS_LR_MIN ? ROWS_LR_MIN : cl;
    const bool aligned = (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
    HookScope hs(hook, KIND_TILE_SORT, 2.0 * (double)rows * (double)cols * sizeof(K), s);
    // a row is a whole shipped tile: the SORT pass over rows * cols keys is the
    // row sort (u32 2^14: its merge-level top; f64 keys would need a sweep after it)
    // MISORT_ROWS_SHIPPED=0 keeps such rows on the row tile (read per call: a probe's A/B)
    const char* knob = getenv("MISORT_ROWS_SHIPPED");
    const bool shipped = (lr == KT<K>::LT || (sizeof(K) == 4 && lr == SORT_LT_MERGE)) && !(knob && atoi(knob) == 0);
    if (aligned && !f64 && cols == ((int64_t)1 << lr) && shipped) {
        launch_sort<K>(in, out, rows * cols, false, s, lr);
        return hipGetLastError();
    }
    const int flags = (aligned && cols % KT<K>::V == 0 ? ROWS_VEC : 0) | (f64 ? ROWS_F64 : 0);
    if (!launch_rows_lr<K>(lr, in, out, rows, cols, flags, s)) return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace misort

// segs_tile.h -- the segment SORT tile: the row tile of rows_tile.h with another
// front.  One launch sorts the segments of ONE class LR (segs_class.h): their
// lengths lie in (2^(LR-1), 2^LR] (LR = 5: 1..32), a tile of 2^LT keys holds
// R = 2^(LT - LR) of them and runs the network's levels 1..LR only.
//
// Index mapping: row r of tile j is segment list[j R + r] of the class's list;
// virtual key v of the tile is row v >> LR, column v & (2^LR - 1), and reads
// in[begin + col] when col < len, else the all-ones sentinel (a row past the
// class's count has len 0).  As in the row tile a sentinel suffix only moves
// upwards inside its block, so the first len keys of the sorted block are the
// sorted segment and only those are stored, to out[begin + col].
//
// The tile's R (begin, len) pairs are staged in LDS by its first R lanes (two
// dependent loads each: the list entry, then the two offsets) before the key
// loads; loads and stores read them from there (reading the offsets per load
// and store instead took 1.0-2.1x the time: profiles/segments/stage_ab.jsonl).
// Segments start anywhere: element accesses throughout.  ord_of_f64 is applied
// to real keys only (the mapped all-ones padding would be the smallest key).
//
// Levels, LDS layout and barrier rule are the row tile's (sort32_regs,
// wave_levels, sort_levels_w).  One tile per workgroup: a workgroup has read
// all its segments into LDS before it stores any, and validated offsets make
// the segments disjoint, so out == in is safe.
//
// Included by one translation unit per key type (segs_u32.hip, segs_u64.hip).
#pragma once
#include "bitonic.h"
#include "segs_class.h"

namespace misort {

namespace {

static_assert(seg_tile_log2(4) == KT<uint32_t>::LT && seg_tile_log2(8) == KT<uint64_t>::LT,
              "segs_class.h knows the largest SORT tiles");
static_assert(SEG_LR_MIN == ROWS_LR_MIN, "segs_class.h knows the shortest row block");

constexpr int SEGS_F64 = 2;  // flags: f64 keys (u64 only), as ROWS_F64

template <typename K, int LT, int LR>
__global__ __launch_bounds__((TileGeo<K, LT>::NT), (TileGeo<K, LT>::WAVES_PER_EU)) void k_sort_segs(
    const K* in, K* out, const int64_t* __restrict__ off, const uint32_t* __restrict__ list, int64_t count,
    int flags) {
    typedef TileGeo<K, LT> G;
    static_assert(LR >= SEG_LR_MIN && LR <= LT, "a segment block is a lane's 32 keys .. the tile");
    constexpr int CM = (1 << LR) - 1;
    constexpr int R = 1 << (LT - LR);
    static_assert(R <= G::NT, "one lane stages one segment");
    __shared__ __attribute__((aligned(16))) K s[lds_words(G::T)];
    __shared__ int64_t seg_begin[R];
    __shared__ int seg_len[R];
    const int t = threadIdx.x;
    const bool f64 = sizeof(K) == 8 && (flags & SEGS_F64);
    if (t < R) {
        // (begin, len) of the tile's row t from the offsets; a row past the class's count is empty
        const int64_t j = (int64_t)blockIdx.x * R + t;
        int64_t b = 0, l = 0;
        if (j < count) {
            const int64_t g = list[j];
            b = off[g];
            l = off[g + 1] - b;
        }
        seg_begin[t] = b;
        seg_len[t] = (int)(l < CM + 1 ? l : CM + 1);  // the class holds no longer one
    }
    __syncthreads();
    K pre[G::LOADS][G::V];
#pragma unroll
    for (int k = 0; k < G::LOADS; ++k) {
        const int e = place<K, LT>(k, t);
        const int r = e >> LR, c = e & CM;
        const int len = seg_len[r];
        const K* src = in + (seg_begin[r] + c);
#pragma unroll
        for (int j = 0; j < G::V; ++j) {
            const bool real = c + j < len;
            K x = KT<K>::MAX;
            if (real) x = src[j];
            pre[k][j] = real && f64 ? (K)ord_of_f64((uint64_t)x) : x;
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
        const int r = e >> LR, c = e & CM;
        const int len = seg_len[r];
        K* dst = out + (seg_begin[r] + c);
#pragma unroll
        for (int j = 0; j < G::V; ++j) {
            K x = s[pad(e + j)];
            if (f64) x = (K)f64_of_ord((uint64_t)x);  // never stored where it is a sentinel
            if (c + j < len) dst[j] = x;
        }
    }
}

template <typename K, int LT, int LR>
void launch_segs(const K* in, K* out, const int64_t* off, const uint32_t* list, int64_t count, int flags,
                 hipStream_t s) {
    // count <= 2^31 - 1 segments: the grid fits one launch
    const int64_t ntiles = (count + (1 << (LT - LR)) - 1) >> (LT - LR);
    k_sort_segs<K, LT, LR><<<dim3((unsigned)ntiles), dim3(TileGeo<K, LT>::NT), 0, s>>>(in, out, off, list, count, flags);
}

// The tiles of launch_rows_lr (rows_tile.h): u32 the 2^14 tile up to LR = 14,
// the 2^15 tile for LR = 15 alone; u64 the 2^13 tile.
template <typename K>
bool launch_segs_lr(int lr, const K* in, K* out, const int64_t* off, const uint32_t* list, int64_t count, int flags,
                    hipStream_t s) {
    constexpr int LT = sizeof(K) == 4 ? SORT_LT_MERGE : KT<K>::LT;
    switch (lr) {
#define MISORT_SEGS_CASE(LR_) \
    case LR_:                 \
        if constexpr (LR_ <= LT) launch_segs<K, LT, LR_>(in, out, off, list, count, flags, s); \
        return LR_ <= LT
        MISORT_SEGS_CASE(5);
        MISORT_SEGS_CASE(6);
        MISORT_SEGS_CASE(7);
        MISORT_SEGS_CASE(8);
        MISORT_SEGS_CASE(9);
        MISORT_SEGS_CASE(10);
        MISORT_SEGS_CASE(11);
        MISORT_SEGS_CASE(12);
        MISORT_SEGS_CASE(13);
        MISORT_SEGS_CASE(14);
#undef MISORT_SEGS_CASE
    case 15:
        if constexpr (sizeof(K) == 4) launch_segs<K, SORT_LT_U32, 15>(in, out, off, list, count, flags, s);
        return sizeof(K) == 4;
    default:
        return false;
    }
}

}  // namespace

template <typename K>
hipError_t sort_segs_tile(const K* in, K* out, const int64_t* off, const uint32_t* list, int64_t count, int lr,
                          int64_t keys, bool f64, hipStream_t s, LaunchHook* hook) {
    if (count <= 0) return hipSuccess;
    if ((sizeof(K) == 4 && f64) || !in || !out || !off || !list || count > 0x7FFFFFFF) return hipErrorInvalidValue;
    HookScope hs(hook, KIND_TILE_SORT, 2.0 * (double)keys * sizeof(K), s);
    if (!launch_segs_lr<K>(lr, in, out, off, list, count, f64 ? SEGS_F64 : 0, s)) return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace misort

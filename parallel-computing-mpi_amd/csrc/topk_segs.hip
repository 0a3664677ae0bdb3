// topk_segs.hip -- segmented top-k (gfx950): the k smallest or largest keys of
// every segment [off[i], off[i + 1]) of a caller's array of 32-bit keys, sorted,
// with their positions inside the segment, into row i of nseg x k outputs.
//
// The order and the maps are those of topk.hip: both directions sort ASCENDING
// records T(key) << 32 | position, T = K for the smallest keys (K the identity,
// or ord_of_f32), T = ~K for the largest.  The segments come from the class
// lists of the segmented sorts (segs.hip, segs_class.h with 8-byte keys).
//
//   k_topk_segs<LR, RECS_IN, SPLIT>  the body of k_topk on the front of
//                  k_sort_segs_pairs: TileGeo<uint64_t, 13>, the pad() layout,
//                  sort32_regs, levels 6..LR as sort_levels_w's LDS phases and
//                  its barrier rule, a lane's slot 4 consecutive records.
//     keys -> outputs (SPLIT, LR = 5..13: one class up to the tile).  Row r of
//                  tile j is segment list[j R + r], R = 2^(13 - LR); the tile's
//                  first R lanes stage (begin, len, segment) in LDS; a row past
//                  the class's count has len 0.  Slots j < min(len, k) go to
//                  out[segment k + j].
//     keys -> candidates (LR = 13, one class c >= 14): every segment of the class
//                  is P = 2^(c - 13) pieces of 2^13 keys; tile b is piece
//                  b & (P - 1) of list entry b >> (c - 13); the position of
//                  record e is piece << 13 | e, real below len.  The first k
//                  records of the sorted piece go to cand[b k + j], all-ones
//                  where the piece has fewer real ones.  A piece at or past len
//                  leaves as a whole workgroup before any barrier and writes its
//                  k all-ones candidates only.  Afterwards the class is `count`
//                  uniform rows of P k candidate records: topk_pass takes over.
//     records -> outputs (RECS_IN, SPLIT, LR = 5..13: the last pass of a long
//                  class).  Row r has m candidate records, its first k go to
//                  out[list[r] k + j]; len > 2^13 >= k, so all k are real.
//   k_topk_segs_fill  the shape of the offset sweeps (256 lanes, a capped grid
//                  that strides, 64-bit indices): slots [len, k) of every row
//                  with len < k get the index 0xFFFFFFFF and the fill key, the
//                  unmapped all-ones record.  It reads only the offsets and
//                  writes slots no tile writes: no order against the tiles.
//
// Sentinels: a virtual record at or past its segment's length is the all-ones
// record.  T is applied to real keys only.  A position is below 2^31, so no
// real record equals the sentinel: sentinels are strictly the largest records
// of a block, and a tile stores only the first min(len, k) of a block that has
// len real records -- no sentinel is ever stored by a tile.
//
// Aliasing: none.  A tile writes row `segment` while other tiles still read
// their keys: no output may overlap the keys or the offsets (the runtime
// refuses it).
//
// No kernel waits on another workgroup and none has an atomic.
#include "bitonic.h"
#include "segs_class.h"
#include "topk_segs_plan.h"

namespace misort {

namespace {

static_assert(seg_tile_log2(8) == KT<uint64_t>::LT, "segs_class.h knows the u64 SORT tile");
static_assert(TOPK_LT == KT<uint64_t>::LT, "the plan cuts segments into tiles of the u64 SORT tile");
static_assert(SEG_LR_MIN == ROWS_LR_MIN && TOPK_LR_MIN == ROWS_LR_MIN, "one shortest block");

constexpr int TS_LT = KT<uint64_t>::LT;
constexpr int TS_NT = 256;            // the fill: the sweeps of segs.hip
constexpr int TS_MAX_GRID = 1 << 20;  // SEGS_MAX_GRID
// flags: bit 0 = f32 keys, bit 1 = the largest keys (T = ~K)
constexpr int TS_F32 = 1, TS_LARGEST = 2;

struct TopkSegsArgs {
    const uint32_t* keys_in;       // source KEYS
    const uint64_t* recs_in;       // source RECS: count rows of m records
    uint64_t* recs_out;            // sink candidates
    uint32_t *keys_out, *idx_out;  // sink SPLIT
    const int64_t* off;
    const uint32_t* list;
    int64_t count, m, k, tile0;
    int piece_log2;  // keys -> candidates: c - 13
    int flags;
};

// tk_map / tk_unmap of topk.hip
__device__ __forceinline__ uint32_t ts_map(uint32_t x, bool f32, bool largest) {
    const uint32_t o = f32 ? ord_of_f32(x) : x;
    return largest ? ~o : o;
}
__device__ __forceinline__ uint32_t ts_unmap(uint32_t t, bool f32, bool largest) {
    const uint32_t o = largest ? ~t : t;
    return f32 ? f32_of_ord(o) : o;
}

template <int LR, bool RECS_IN, bool SPLIT>
__global__ __launch_bounds__((TileGeo<uint64_t, TS_LT>::NT), (TileGeo<uint64_t, TS_LT>::WAVES_PER_EU)) void
k_topk_segs(TopkSegsArgs a) {
    typedef uint64_t K;
    constexpr int LT = TS_LT;
    typedef TileGeo<K, LT> G;
    static_assert(LR >= SEG_LR_MIN && LR <= LT, "a segment block is a lane's 32 records .. the tile");
    static_assert(SPLIT || (LR == LT && !RECS_IN), "candidates come from pieces of the tile, out of keys");
    constexpr int W = 4;
    constexpr int LOADS = 32 / W;
    constexpr int CM = (1 << LR) - 1;
    constexpr int R = SPLIT ? 1 << (LT - LR) : 1;
    static_assert(R <= G::NT, "one lane stages one segment");
    __shared__ __attribute__((aligned(16))) K s[lds_words(G::T)];
    __shared__ int64_t seg_begin[R];  // SPLIT: the row's first key (KEYS) or record (RECS)
    __shared__ int seg_len[R];        //        its keys or records, 0 past the count
    __shared__ uint32_t seg_at[R];    //        the segment: its row of the outputs
    const int t = threadIdx.x;
    const int64_t tile = a.tile0 + blockIdx.x;
    const bool f32 = a.flags & TS_F32;
    const bool largest = a.flags & TS_LARGEST;
    const int64_t kk = a.k;
    // keys -> candidates: the piece's first position, the segment's begin and length (wave-uniform)
    [[maybe_unused]] int64_t p_begin = 0, p_len = 0, p_rec0 = 0;
    if constexpr (SPLIT) {
        if (t < R) {
            const int64_t j = tile * R + t;
            int64_t b = 0, l = 0;
            uint32_t g = 0;
            if (j < a.count) {
                g = a.list[j];
                if constexpr (RECS_IN) {
                    b = j * a.m, l = a.m;
                } else {
                    b = a.off[g];
                    l = a.off[g + 1] - b;
                }
            }
            seg_begin[t] = b;
            seg_len[t] = (int)(l < 0 ? 0 : l < CM + 1 ? l : CM + 1);  // the class holds no longer one
            seg_at[t] = g;
        }
        __syncthreads();
    } else {
        const int64_t entry = tile >> a.piece_log2;
        const int64_t piece = tile - (entry << a.piece_log2);
        const int64_t g = a.list[entry];
        p_begin = a.off[g];
        p_len = a.off[g + 1] - p_begin;
        p_rec0 = piece << LT;
        if (p_rec0 >= p_len) {
            // nothing real in this piece: the whole workgroup leaves, before any barrier
            for (int64_t j = t; j < kk; j += G::NT) a.recs_out[tile * kk + j] = ~(K)0;
            return;
        }
    }
    K pre[LOADS][W];
#pragma unroll
    for (int k = 0; k < LOADS; ++k) {
        const int e = (k * G::NT + t) * W;
        if constexpr (SPLIT) {
            const int r = e >> LR, c = e & CM;
            const int len = seg_len[r];
            const int64_t at = seg_begin[r] + c;
#pragma unroll
            for (int j = 0; j < W; ++j) {
                K x = ~(K)0;
                if (c + j < len) {
                    if constexpr (RECS_IN) x = a.recs_in[at + j];
                    else x = (K)ts_map(a.keys_in[at + j], f32, largest) << 32 | (uint32_t)(c + j);
                }
                pre[k][j] = x;
            }
        } else {
            const int64_t p = p_rec0 + e;
#pragma unroll
            for (int j = 0; j < W; ++j) {
                K x = ~(K)0;
                if (p + j < p_len) x = (K)ts_map(a.keys_in[p_begin + p + j], f32, largest) << 32 | (uint32_t)(p + j);
                pre[k][j] = x;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < LOADS; ++k) {
        const int e = (k * G::NT + t) * W;
#pragma unroll
        for (int j = 0; j < W; ++j) s[pad(e + j)] = pre[k][j];
    }
    __syncthreads();
    {
        K x[32];
        const int a0 = pad(t << 5);
#pragma unroll
        for (int c = 0; c < 32; ++c) x[c] = s[a0 + c];
        sort32_regs<K>(x);
        // each lane rewrites only the records it read
#pragma unroll
        for (int c = 0; c < 32; ++c) s[a0 + c] = x[c];
    }
    if constexpr (5 < LR) {
        // level 6 stays inside the wave; the last phase of level LR ends with a
        // workgroup barrier (lds_range_w, NEXT_HI = -1)
        wave_sync();
        sort_levels_w<K, 6, LR>(s, t);
    } else {
        __syncthreads();  // the stores read other lanes' records
    }
#pragma unroll
    for (int k = 0; k < LOADS; ++k) {
        const int e = (k * G::NT + t) * W;
        const int j0 = e & CM;
        if constexpr (SPLIT) {
            const int r = e >> LR;
            // the first min(len, k) records of the block are real: never a sentinel
            const int64_t lim = seg_len[r] < kk ? seg_len[r] : kk;
            if (j0 >= lim) continue;
            const int64_t off = (int64_t)seg_at[r] * kk + j0;
#pragma unroll
            for (int j = 0; j < W; ++j)
                if (j0 + j < lim) {
                    const K rec = s[pad(e + j)];
                    if (a.keys_out) a.keys_out[off + j] = ts_unmap((uint32_t)(rec >> 32), f32, largest);
                    a.idx_out[off + j] = (uint32_t)rec;
                }
        } else {
            if (j0 >= kk) continue;
            const int64_t off = tile * kk + j0;  // tile = entry P + piece
#pragma unroll
            for (int j = 0; j < W; ++j)
                if (j0 + j < kk) a.recs_out[off + j] = s[pad(e + j)];
        }
    }
}

template <int LR, bool RECS_IN, bool SPLIT>
void launch_topk_segs(TopkSegsArgs a, int64_t ntiles, hipStream_t s) {
    constexpr int64_t MAX_GRID = 0x7FFFFFFF;
    for (int64_t t0 = 0; t0 < ntiles; t0 += MAX_GRID) {
        const int64_t g = ntiles - t0 < MAX_GRID ? ntiles - t0 : MAX_GRID;
        a.tile0 = t0;
        k_topk_segs<LR, RECS_IN, SPLIT><<<dim3((unsigned)g), dim3(TileGeo<uint64_t, TS_LT>::NT), 0, s>>>(a);
    }
}

template <bool RECS_IN>
bool launch_topk_segs_split(int lr, const TopkSegsArgs& a, int64_t ntiles, hipStream_t s) {
    switch (lr) {
#define MISORT_TOPK_SEGS_CASE(LR_) \
    case LR_:                      \
        launch_topk_segs<LR_, RECS_IN, true>(a, ntiles, s); \
        return true
        MISORT_TOPK_SEGS_CASE(5);
        MISORT_TOPK_SEGS_CASE(6);
        MISORT_TOPK_SEGS_CASE(7);
        MISORT_TOPK_SEGS_CASE(8);
        MISORT_TOPK_SEGS_CASE(9);
        MISORT_TOPK_SEGS_CASE(10);
        MISORT_TOPK_SEGS_CASE(11);
        MISORT_TOPK_SEGS_CASE(12);
        MISORT_TOPK_SEGS_CASE(13);
#undef MISORT_TOPK_SEGS_CASE
    default:
        return false;
    }
}

// A workgroup takes 256 consecutive segments at a time: a lane reads one
// length, then the lanes together write the rows that are short, a row after a
// row.  A workgroup with no short row writes nothing.
__global__ __launch_bounds__(TS_NT) void k_topk_segs_fill(const int64_t* __restrict__ off, int64_t nseg, int64_t k,
                                                          uint32_t* keys_out, uint32_t* idx_out, uint32_t fill_key) {
    __shared__ int lens[TS_NT];
    __shared__ int any_short;
    const int t = threadIdx.x;
    const int64_t ngroups = (nseg + TS_NT - 1) / TS_NT;
    for (int64_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {  // a uniform trip count
        if (t == 0) any_short = 0;
        __syncthreads();
        const int64_t i = grp * TS_NT + t;
        int64_t l = k;  // past nseg: nothing to fill
        if (i < nseg) l = off[i + 1] - off[i];
        l = l < 0 ? 0 : l < k ? l : k;  // k <= 2^13
        lens[t] = (int)l;
        if (l < k) any_short = 1;  // every writer writes 1
        __syncthreads();
        if (any_short) {
            for (int r = 0; r < TS_NT; ++r) {
                const int64_t row = (grp * TS_NT + r) * k;
                for (int64_t j = lens[r] + t; j < k; j += TS_NT) {
                    if (keys_out) keys_out[row + j] = fill_key;
                    idx_out[row + j] = 0xFFFFFFFFu;
                }
            }
        }
        __syncthreads();  // the next trip rewrites lens and any_short
    }
}

}  // namespace

hipError_t topk_segs_tile(const uint32_t* keys_in, uint32_t* keys_out, uint32_t* idx_out, const int64_t* off,
                          const uint32_t* list, int64_t count, int lr, int64_t keys, int64_t k, bool f32,
                          bool largest, hipStream_t s, LaunchHook* hook) {
    if (count <= 0 || k <= 0) return hipSuccess;
    if (!keys_in || !idx_out || !off || !list || count > 0x7FFFFFFF || !topk_segs_k_ok(k)) return hipErrorInvalidValue;
    TopkSegsArgs a = {};
    a.keys_in = keys_in, a.keys_out = keys_out, a.idx_out = idx_out, a.off = off, a.list = list;
    a.count = count, a.k = k;
    a.flags = (f32 ? TS_F32 : 0) | (largest ? TS_LARGEST : 0);
    const int64_t ntiles = (count + (1 << (TS_LT - lr)) - 1) >> (TS_LT - lr);
    // the keys read once; at most min(len, k) results per segment written
    const double out = (keys_out ? 8.0 : 4.0) * (double)(keys < count * k ? keys : count * k);
    HookScope hs(hook, KIND_TILE_SORT, 4.0 * (double)keys + out, s);
    if (!launch_topk_segs_split<false>(lr, a, ntiles, s)) return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t topk_segs_pieces(const uint32_t* keys_in, uint64_t* cand, const int64_t* off, const uint32_t* list,
                            int64_t count, int cls, int64_t keys, int64_t k, bool f32, bool largest, hipStream_t s,
                            LaunchHook* hook) {
    if (count <= 0 || k <= 0) return hipSuccess;
    if (!keys_in || !cand || !off || !list || count > 0x7FFFFFFF || cls <= TS_LT || cls >= TOPK_SEGS_CLASS_END ||
        k > TOPK_K_LONG_MAX)
        return hipErrorInvalidValue;
    TopkSegsArgs a = {};
    a.keys_in = keys_in, a.recs_out = cand, a.off = off, a.list = list;
    a.count = count, a.k = k, a.piece_log2 = cls - TS_LT;
    a.flags = (f32 ? TS_F32 : 0) | (largest ? TS_LARGEST : 0);
    const int64_t ntiles = count << (cls - TS_LT);  // count < 2^31, cls - 13 <= 18
    HookScope hs(hook, KIND_TILE_SORT, 4.0 * (double)keys + 8.0 * (double)ntiles * (double)k, s);
    launch_topk_segs<TS_LT, false, false>(a, ntiles, s);
    return hipGetLastError();
}

hipError_t topk_segs_last(const TopkPass& p, const uint64_t* recs_in, uint32_t* keys_out, uint32_t* idx_out,
                          const uint32_t* list, int64_t count, int64_t k, bool f32, bool largest, hipStream_t s,
                          LaunchHook* hook) {
    if (count <= 0 || k <= 0) return hipSuccess;
    if (!recs_in || !idx_out || !list || count > 0x7FFFFFFF || p.npieces != 1 || p.lr < SEG_LR_MIN || p.lr > TS_LT ||
        p.m_in > ((int64_t)1 << p.lr) || k > p.m_in)
        return hipErrorInvalidValue;
    TopkSegsArgs a = {};
    a.recs_in = recs_in, a.keys_out = keys_out, a.idx_out = idx_out, a.list = list;
    a.count = count, a.m = p.m_in, a.k = k;
    a.flags = (f32 ? TS_F32 : 0) | (largest ? TS_LARGEST : 0);
    const int64_t ntiles = (count + (1 << (TS_LT - p.lr)) - 1) >> (TS_LT - p.lr);
    const double bytes = 8.0 * (double)count * (double)p.m_in + (keys_out ? 8.0 : 4.0) * (double)count * (double)k;
    HookScope hs(hook, KIND_TILE_SORT, bytes, s);
    if (!launch_topk_segs_split<true>(p.lr, a, ntiles, s)) return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t topk_segs_fill(const int64_t* off, int64_t nseg, int64_t k, uint32_t* keys_out, uint32_t* idx_out,
                          bool f32, bool largest, hipStream_t s, LaunchHook* hook) {
    if (nseg <= 0 || k <= 0) return hipSuccess;
    if (!off || !idx_out || !topk_segs_k_ok(k)) return hipErrorInvalidValue;
    // the unmapped all-ones key: the last key of the direction's order
    const uint32_t fill_key = largest ? (f32 ? 0xFFFFFFFFu : 0u) : (f32 ? 0x7FFFFFFFu : 0xFFFFFFFFu);
    HookScope hs(hook, KIND_OTHER, 8.0 * (double)(nseg + 1), s);  // the offsets; what it writes depends on them
    const int64_t g = (nseg + TS_NT - 1) / TS_NT;
    k_topk_segs_fill<<<(unsigned)(g > TS_MAX_GRID ? TS_MAX_GRID : g), TS_NT, 0, s>>>(off, nseg, k, keys_out, idx_out,
                                                                                   fill_key);
    return hipGetLastError();
}

}  // namespace misort

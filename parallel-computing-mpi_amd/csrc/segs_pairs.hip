// segs_pairs.hip -- the segmented key-value sort's kernels (gfx950): every
// segment [off[i], off[i + 1]) of a caller's (32-bit key, 32-bit value) arrays
// sorted on its own by (key, value).  The offset sweeps, the classes and the
// class lists are those of the keys-only segmented sort (segs.hip,
// segs_class.h) with 8-byte keys: what is sorted is the u64 record
// K(key) << 32 | value of rows_pairs.hip, K the identity or ord_of_f32.
//
//   k_sort_segs_pairs<LR>  one class LR = 5..13: the body of k_sort_rows_pairs on
//                  the front of k_sort_segs.  TileGeo<uint64_t, 13>, the pad()
//                  layout, sort32_regs, levels 6..LR as sort_levels_w's LDS
//                  phases and its barrier rule.  Row r of tile j is segment
//                  list[j R + r], R = 2^(13 - LR); the tile's R (begin, len)
//                  pairs are staged in LDS by its first R lanes (segs_tile.h
//                  says why); a row past the class's count has len 0.  The
//                  records are formed in registers as the tile loads (value c,
//                  the position inside the segment, where there is no value
//                  array: the stable argsort of the segment) and split again as
//                  it stores, so they never exist in HBM.  Segments start
//                  anywhere: element accesses throughout.
//   k_pad_segs_pairs, k_unpad_segs_pairs  the long classes (k > 13), one k at a
//                  time, in the shape of k_pad_segs / k_unpad_segs: 256 lanes, a
//                  capped grid that strides, 64-bit indices, one 16-byte vector
//                  (two records) of the padded buffer per lane and trip.  Block r
//                  of the padded buffer gets the records of segment list[r] and
//                  all-ones above its length; the first len records of block r go
//                  back, split, to begin + c.
//
// Sentinels: a virtual record at or past its segment's length is the all-ones
// RECORD.  K is applied to real keys only -- ord_of_f32 of the all-ones pattern
// would be 0, the smallest key.  A real record can equal the sentinel (u32 key
// 0xFFFFFFFF or f32 pattern 0x7FFFFFFF, with value 0xFFFFFFFF); the per-block
// argument of rows_tile.h covers it: no compare-exchange of levels 1..LR (or of
// the 2^k-key block sort) leaves its block, the block ends up ascending, and the
// all-ones records after the first len positions are equal to any real one
// among them bit for bit, so the first len records are the sorted segment
// whichever of the equal records they are.
//
// Aliasing: one tile per workgroup; a workgroup has read all its segments of
// both input arrays into LDS before it stores any, and validated offsets make
// the segments disjoint, so an output may be exactly an input.  A long class's
// pad sweep has read all its segments before its sort starts.
//
// No kernel waits on another workgroup and none has an atomic.
#include "bitonic.h"
#include "segs_class.h"

namespace misort {

namespace {

static_assert(seg_tile_log2(8) == KT<uint64_t>::LT, "segs_class.h knows the u64 SORT tile");
static_assert(SEG_LR_MIN == ROWS_LR_MIN, "segs_class.h knows the shortest row block");

constexpr int SP_LT = KT<uint64_t>::LT;
constexpr int SP_NT = 256;             // the sweeps of segs.hip
constexpr int SP_MAX_GRID = 1 << 20;   // SEGS_MAX_GRID
typedef uint64_t rec2_t __attribute__((ext_vector_type(2)));

// rp_rec of rows_pairs.hip
__device__ __forceinline__ uint64_t sp_rec(uint32_t k, uint32_t v, bool f32) {
    return (uint64_t)(f32 ? ord_of_f32(k) : k) << 32 | v;
}

template <int LR>
__global__ __launch_bounds__((TileGeo<uint64_t, SP_LT>::NT), (TileGeo<uint64_t, SP_LT>::WAVES_PER_EU)) void
k_sort_segs_pairs(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out,
                  const int64_t* __restrict__ off, const uint32_t* __restrict__ list, int64_t count, int f32) {
    typedef uint64_t K;
    constexpr int LT = SP_LT;
    typedef TileGeo<K, LT> G;
    static_assert(LR >= SEG_LR_MIN && LR <= LT, "a segment block is a lane's 32 records .. the tile");
    constexpr int CM = (1 << LR) - 1;
    constexpr int R = 1 << (LT - LR);
    static_assert(R <= G::NT, "one lane stages one segment");
    __shared__ __attribute__((aligned(16))) K s[lds_words(G::T)];
    __shared__ int64_t seg_begin[R];
    __shared__ int seg_len[R];
    const int t = threadIdx.x;
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
        seg_len[t] = (int)(l < 0 ? 0 : l < CM + 1 ? l : CM + 1);  // the class holds no longer one
    }
    __syncthreads();
    K pre[G::LOADS][G::V];
#pragma unroll
    for (int k = 0; k < G::LOADS; ++k) {
        const int e = place<K, LT>(k, t);
        const int r = e >> LR, c = e & CM;
        const int len = seg_len[r];
        const int64_t at = seg_begin[r] + c;
#pragma unroll
        for (int j = 0; j < G::V; ++j) {
            K x = ~(K)0;
            if (c + j < len) x = sp_rec(keys_in[at + j], vals_in ? vals_in[at + j] : (uint32_t)(c + j), f32);
            pre[k][j] = x;
        }
    }
#pragma unroll
    for (int k = 0; k < G::LOADS; ++k) {
        const int e = place<K, LT>(k, t);
#pragma unroll
        for (int j = 0; j < G::V; ++j) s[pad(e + j)] = pre[k][j];
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
    for (int k = 0; k < G::LOADS; ++k) {
        const int e = place<K, LT>(k, t);
        const int r = e >> LR, c = e & CM;
        const int len = seg_len[r];
        const int64_t at = seg_begin[r] + c;
#pragma unroll
        for (int j = 0; j < G::V; ++j) {
            const K rec = s[pad(e + j)];
            const uint32_t o = (uint32_t)(rec >> 32);
            if (c + j < len) {  // never stored where it is a sentinel
                if (keys_out) keys_out[at + j] = f32 ? f32_of_ord(o) : o;
                vals_out[at + j] = (uint32_t)rec;
            }
        }
    }
}

template <int LR>
void launch_segs_pairs(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out,
                       const int64_t* off, const uint32_t* list, int64_t count, bool f32, hipStream_t s) {
    // count <= 2^31 - 1 segments: the grid fits one launch
    const int64_t ntiles = (count + (1 << (SP_LT - LR)) - 1) >> (SP_LT - LR);
    k_sort_segs_pairs<LR><<<dim3((unsigned)ntiles), dim3(TileGeo<uint64_t, SP_LT>::NT), 0, s>>>(
        keys_in, vals_in, keys_out, vals_out, off, list, count, f32 ? 1 : 0);
}

template <bool FLT>
__global__ __launch_bounds__(SP_NT) void k_pad_segs_pairs(const uint32_t* keys_in, const uint32_t* vals_in,
                                                          const int64_t* __restrict__ off,
                                                          const uint32_t* __restrict__ list,
                                                          uint64_t* __restrict__ padded, int64_t count, int k) {
    const int64_t nq = (count << k) / 2, cm = ((int64_t)1 << k) - 1;
    const int64_t stride = (int64_t)gridDim.x * SP_NT;
    for (int64_t q = (int64_t)blockIdx.x * SP_NT + threadIdx.x; q < nq; q += stride) {
        const int64_t p = q * 2, r = p >> k, c = p & cm;
        const int64_t g = list[r];
        const int64_t b = off[g], len = off[g + 1] - b;
        rec2_t v;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            uint64_t x = ~(uint64_t)0;
            // real keys only; the position inside the segment where there is no value array
            if (c + j < len) x = sp_rec(keys_in[b + c + j], vals_in ? vals_in[b + c + j] : (uint32_t)(c + j), FLT);
            v[j] = x;
        }
        reinterpret_cast<rec2_t*>(padded)[q] = v;
    }
}

template <bool FLT>
__global__ __launch_bounds__(SP_NT) void k_unpad_segs_pairs(const uint64_t* __restrict__ padded, uint32_t* keys_out,
                                                            uint32_t* vals_out, const int64_t* __restrict__ off,
                                                            const uint32_t* __restrict__ list, int64_t count, int k) {
    const int64_t nq = (count << k) / 2, cm = ((int64_t)1 << k) - 1;
    const int64_t stride = (int64_t)gridDim.x * SP_NT;
    for (int64_t q = (int64_t)blockIdx.x * SP_NT + threadIdx.x; q < nq; q += stride) {
        const int64_t p = q * 2, r = p >> k, c = p & cm;
        const int64_t g = list[r];
        const int64_t b = off[g], len = off[g + 1] - b;
        if (c >= len) continue;  // padding only: not read
        const rec2_t v = reinterpret_cast<const rec2_t*>(padded)[q];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t o = (uint32_t)(v[j] >> 32);
            if (c + j < len) {  // never stored where it is padding
                if (keys_out) keys_out[b + c + j] = FLT ? f32_of_ord(o) : o;
                vals_out[b + c + j] = (uint32_t)v[j];
            }
        }
    }
}

// segs_grid of segs.hip
unsigned sp_grid(int64_t nq) {
    const int64_t g = (nq + SP_NT - 1) / SP_NT;
    return (unsigned)(g < 1 ? 1 : g > SP_MAX_GRID ? SP_MAX_GRID : g);
}

// k >= 1 keeps a block a whole number of vectors
bool sp_args_ok(const void* user, const void* padded, const int64_t* off, const uint32_t* list, int64_t count,
                int k) {
    if (!user || !padded || !off || !list || !aligned16(padded)) return false;
    return k >= 1 && k <= 58 && count <= (INT64_MAX >> k) / 8;
}

}  // namespace

hipError_t sort_segs_pairs_tile(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out,
                                uint32_t* vals_out, const int64_t* off, const uint32_t* list, int64_t count, int lr,
                                int64_t keys, bool f32, hipStream_t s, LaunchHook* hook) {
    if (count <= 0) return hipSuccess;
    if (!keys_in || !vals_out || !off || !list || count > 0x7FFFFFFF) return hipErrorInvalidValue;
    const double arrays = 2.0 + (vals_in ? 1.0 : 0.0) + (keys_out ? 1.0 : 0.0);
    HookScope hs(hook, KIND_TILE_SORT, arrays * 4.0 * (double)keys, s);
    switch (lr) {
#define MISORT_SEGS_PAIRS_CASE(LR_) \
    case LR_:                       \
        launch_segs_pairs<LR_>(keys_in, vals_in, keys_out, vals_out, off, list, count, f32, s); \
        break
        MISORT_SEGS_PAIRS_CASE(5);
        MISORT_SEGS_PAIRS_CASE(6);
        MISORT_SEGS_PAIRS_CASE(7);
        MISORT_SEGS_PAIRS_CASE(8);
        MISORT_SEGS_PAIRS_CASE(9);
        MISORT_SEGS_PAIRS_CASE(10);
        MISORT_SEGS_PAIRS_CASE(11);
        MISORT_SEGS_PAIRS_CASE(12);
        MISORT_SEGS_PAIRS_CASE(13);
#undef MISORT_SEGS_PAIRS_CASE
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t pad_segs_pairs(const uint32_t* keys_in, const uint32_t* vals_in, const int64_t* off, const uint32_t* list,
                          int64_t count, int64_t keys, uint64_t* padded, int k, bool f32, hipStream_t s,
                          LaunchHook* hook) {
    if (count <= 0) return hipSuccess;
    if (!sp_args_ok(keys_in, padded, off, list, count, k)) return hipErrorInvalidValue;
    const double bytes = (vals_in ? 8.0 : 4.0) * (double)keys + 8.0 * (double)count * (double)((int64_t)1 << k);
    HookScope hs(hook, KIND_OTHER, bytes, s);
    const unsigned g = sp_grid((count << k) / 2);
    if (f32) k_pad_segs_pairs<true><<<g, SP_NT, 0, s>>>(keys_in, vals_in, off, list, padded, count, k);
    else k_pad_segs_pairs<false><<<g, SP_NT, 0, s>>>(keys_in, vals_in, off, list, padded, count, k);
    return hipGetLastError();
}

hipError_t unpad_segs_pairs(const uint64_t* padded, uint32_t* keys_out, uint32_t* vals_out, const int64_t* off,
                            const uint32_t* list, int64_t count, int64_t keys, int k, bool f32, hipStream_t s,
                            LaunchHook* hook) {
    if (count <= 0) return hipSuccess;
    if (!sp_args_ok(vals_out, padded, off, list, count, k)) return hipErrorInvalidValue;
    const double bytes = (keys_out ? 16.0 : 12.0) * (double)keys;
    HookScope hs(hook, KIND_OTHER, bytes, s);
    const unsigned g = sp_grid((count << k) / 2);
    if (f32) k_unpad_segs_pairs<true><<<g, SP_NT, 0, s>>>(padded, keys_out, vals_out, off, list, count, k);
    else k_unpad_segs_pairs<false><<<g, SP_NT, 0, s>>>(padded, keys_out, vals_out, off, list, count, k);
    return hipGetLastError();
}

}  // namespace misort

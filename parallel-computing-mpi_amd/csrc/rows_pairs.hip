// rows_pairs.hip -- the row-wise key-value SORT tile (gfx950): every row of a
// row-major rows x cols array of (32-bit key, 32-bit value) pairs sorted on its
// own by (key, value), cols <= 2^13, in one HBM read and one write per array
// element and no scratch.
//
// It is the u64 row tile of rows_tile.h with another load and store: the same
// TileGeo<uint64_t, 13>, LR = max(ceil_log2(cols), ROWS_LR_MIN), 2^(13 - LR)
// rows per tile, the same pad layout, sort32_regs, levels 6..LR as
// sort_levels_w's LDS phases and the same barrier rule; a lane's slots are
// place()'s, or twice as wide (W below).  What the network sorts is the record
// K(key) << 32 | value of pairs.hip, K the identity or ord_of_f32; it is formed
// in registers as the tile loads (value c where there is no value array: the
// stable argsort of the row) and split again as the tile stores, so the records
// never exist in HBM.
//
// Sentinels: a virtual element outside its row, or past the last row, is the
// all-ones RECORD.  K is applied to real keys only -- ord_of_f32 of the all-ones
// pattern would be 0, the smallest key.  A real record can equal the sentinel
// (u32 key 0xFFFFFFFF or f32 pattern 0x7FFFFFFF, with value 0xFFFFFFFF); the
// per-block argument of rows_tile.h covers it: no compare-exchange of levels
// 1..LR leaves a 2^LR block, the block ends up ascending, and the cols - real
// all-ones records after the first cols positions are equal to any real one
// among them bit for bit, so the first cols records are the sorted row
// whichever of the equal records they are.
//
// Aliasing: one tile per workgroup; a workgroup has read all its rows of both
// input arrays into LDS before it stores any, and tiles own disjoint rows, so
// an output may be exactly an input.
#include "bitonic.h"

namespace misort {

namespace {

// W: the consecutive records of a lane's slot, slot k of lane t = virtual records
// (k NT + t) W ..: 2 is the u64 tile's own placement (8-byte accesses on the
// 32-bit arrays), 4 makes every access 16 bytes.  Measured at 2^27 pairs, the
// two kernels alternated (profiles/rows_pairs/access_width_ab.jsonl): W = 4 takes
// 0.79-0.94 of W = 2's time for the argsort and 0.79-0.93 with values, at every
// row length from 64 to 2^13, so it runs wherever it can.
// flags: bit 0 = W-element accesses (every array in use aligned to 4 W bytes and
// cols a multiple of W, so every slot lies inside one row, aligned; W = 4 is
// launched only so), else element accesses; bit 1 = f32 keys: ord_of_f32 on
// the real keys after the loads, f32_of_ord in the stores -- the sentinels
// stay all-ones.
constexpr int RP_VEC = 1, RP_F32 = 2;
constexpr int RP_LT = KT<uint64_t>::LT;

__device__ __forceinline__ uint64_t rp_rec(uint32_t k, uint32_t v, bool f32) {
    return (uint64_t)(f32 ? ord_of_f32(k) : k) << 32 | v;
}

template <int LR, int W>
__global__ __launch_bounds__((TileGeo<uint64_t, RP_LT>::NT), (TileGeo<uint64_t, RP_LT>::WAVES_PER_EU)) void
k_sort_rows_pairs(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out,
                  int64_t rows, int64_t cols, int64_t tile0, int flags) {
    typedef uint64_t K;
    constexpr int LT = RP_LT;
    typedef TileGeo<K, LT> G;
    static_assert(LR >= ROWS_LR_MIN && LR <= LT && (W == 2 || W == 4), "a row block is a lane's 32 records .. the tile");
    typedef uint32_t u32xw __attribute__((ext_vector_type(W)));
    constexpr int LOADS = 32 / W;
    constexpr int CM = (1 << LR) - 1;
    __shared__ __attribute__((aligned(16))) K s[lds_words(G::T)];
    const int t = threadIdx.x;
    const int64_t row0 = (tile0 + blockIdx.x) << (LT - LR);  // the tile's first row
    const bool vec = flags & RP_VEC;
    const bool f32 = flags & RP_F32;
    // every virtual record real and every slot aligned: no bounds checks
    const bool full = vec && cols == (int64_t)(CM + 1) && row0 + (1 << (LT - LR)) <= rows;
    K pre[LOADS][W];
#pragma unroll
    for (int k = 0; k < LOADS; ++k) {
        const int e = (k * G::NT + t) * W;
        const int64_t r = row0 + (e >> LR);
        const int c = e & CM;
        const int64_t off = r * cols + c;
        if (full) {
            const u32xw x = __builtin_nontemporal_load(reinterpret_cast<const u32xw*>(keys_in + off));
            u32xw v;
#pragma unroll
            for (int j = 0; j < W; ++j) v[j] = (uint32_t)(c + j);
            if (vals_in) v = __builtin_nontemporal_load(reinterpret_cast<const u32xw*>(vals_in + off));
#pragma unroll
            for (int j = 0; j < W; ++j) pre[k][j] = rp_rec(x[j], v[j], f32);
        } else if (vec) {
            const bool real = r < rows && c < cols;  // cols % W == 0: the whole slot or none of it
            u32xw x = {}, v;
#pragma unroll
            for (int j = 0; j < W; ++j) v[j] = (uint32_t)(c + j);
            if (real) {
                x = *reinterpret_cast<const u32xw*>(keys_in + off);
                if (vals_in) v = *reinterpret_cast<const u32xw*>(vals_in + off);
            }
#pragma unroll
            for (int j = 0; j < W; ++j) pre[k][j] = real ? rp_rec(x[j], v[j], f32) : ~(K)0;
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const bool real = r < rows && c + j < cols;
                K x = ~(K)0;
                if (real) x = rp_rec(keys_in[off + j], vals_in ? vals_in[off + j] : (uint32_t)(c + j), f32);
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
        const int64_t r = row0 + (e >> LR);
        const int c = e & CM;
        const int64_t off = r * cols + c;
        u32xw x, v;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const K rec = s[pad(e + j)];
            const uint32_t o = (uint32_t)(rec >> 32);
            x[j] = f32 ? f32_of_ord(o) : o;  // never stored where it is a sentinel
            v[j] = (uint32_t)rec;
        }
        if (full) {
            if (keys_out) __builtin_nontemporal_store(x, reinterpret_cast<u32xw*>(keys_out + off));
            __builtin_nontemporal_store(v, reinterpret_cast<u32xw*>(vals_out + off));
        } else if (vec) {
            if (r < rows && c < cols) {
                if (keys_out) *reinterpret_cast<u32xw*>(keys_out + off) = x;
                *reinterpret_cast<u32xw*>(vals_out + off) = v;
            }
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j)
                if (r < rows && c + j < cols) {
                    if (keys_out) keys_out[off + j] = x[j];
                    vals_out[off + j] = v[j];
                }
        }
    }
}

template <int LR, int W>
void launch_rows_pairs(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out,
                       int64_t rows, int64_t cols, int flags, hipStream_t s) {
    const int64_t ntiles = (rows + (1 << (RP_LT - LR)) - 1) >> (RP_LT - LR);
    constexpr int64_t MAX_GRID = 0x7FFFFFFF;
    for (int64_t t0 = 0; t0 < ntiles; t0 += MAX_GRID) {
        const int64_t g = ntiles - t0 < MAX_GRID ? ntiles - t0 : MAX_GRID;
        k_sort_rows_pairs<LR, W><<<dim3((unsigned)g), dim3(TileGeo<uint64_t, RP_LT>::NT), 0, s>>>(
            keys_in, vals_in, keys_out, vals_out, rows, cols, t0, flags);
    }
}

}  // namespace

hipError_t sort_rows_pairs_tile(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out,
                                uint32_t* vals_out, int64_t rows, int64_t cols, bool f32, hipStream_t s,
                                LaunchHook* hook) {
    if (rows <= 0 || cols <= 0) return hipSuccess;
    if (!keys_in || !vals_out || cols > ((int64_t)1 << RP_LT)) return hipErrorInvalidValue;
    const int cl = ceil_log2(cols);
    const int lr = cl < ROWS_LR_MIN ? ROWS_LR_MIN : cl;
    const bool vec = aligned8(keys_in) && aligned8(vals_in) && aligned8(keys_out) && aligned8(vals_out) && cols % 2 == 0;
    const int flags = (vec ? RP_VEC : 0) | (f32 ? RP_F32 : 0);
    // four elements per slot where every access can be 16 bytes (then vec holds too);
    // MISORT_ROWS_PAIRS_W=2 keeps such calls on the 8-byte kernel (read per call: a probe's A/B)
    const char* knob = getenv("MISORT_ROWS_PAIRS_W");
    const bool w4 = aligned16(keys_in) && aligned16(vals_in) && aligned16(keys_out) && aligned16(vals_out) &&
                    cols % 4 == 0 && !(knob && atoi(knob) == 2);
    const double arrays = 2.0 + (vals_in ? 1.0 : 0.0) + (keys_out ? 1.0 : 0.0);
    HookScope hs(hook, KIND_TILE_SORT, arrays * 4.0 * (double)rows * (double)cols, s);
    switch (lr) {
#define MISORT_ROWS_PAIRS_CASE(LR_) \
    case LR_:                       \
        if (w4) launch_rows_pairs<LR_, 4>(keys_in, vals_in, keys_out, vals_out, rows, cols, flags, s); \
        else launch_rows_pairs<LR_, 2>(keys_in, vals_in, keys_out, vals_out, rows, cols, flags, s); \
        break
        MISORT_ROWS_PAIRS_CASE(5);
        MISORT_ROWS_PAIRS_CASE(6);
        MISORT_ROWS_PAIRS_CASE(7);
        MISORT_ROWS_PAIRS_CASE(8);
        MISORT_ROWS_PAIRS_CASE(9);
        MISORT_ROWS_PAIRS_CASE(10);
        MISORT_ROWS_PAIRS_CASE(11);
        MISORT_ROWS_PAIRS_CASE(12);
        MISORT_ROWS_PAIRS_CASE(13);
#undef MISORT_ROWS_PAIRS_CASE
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace misort

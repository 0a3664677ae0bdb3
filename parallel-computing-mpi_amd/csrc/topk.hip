// topk.hip -- row-wise top-k (gfx950): the k smallest or largest keys of every
// row of a row-major rows x cols array of 32-bit keys, sorted, with their
// columns, without sorting the rows.
//
// Both directions sort ASCENDING records T(key) << 32 | column with the u64
// network of bitonic.h: T = K for the smallest keys (K the identity, or
// ord_of_f32), T = ~K for the largest.  The first k records of a row are then
// its k best keys, best first (descending key for largest), equal keys in
// ascending column order in both directions.  No descending network exists.
//
// One tile kernel, k_topk, runs over BLOCKS of 2^LR virtual records.  It is the
// row tile of rows_pairs.hip -- TileGeo<uint64_t, 13>, 2^(13 - LR) blocks per
// tile, the pad layout, sort32_regs, levels 6..LR as sort_levels_w's LDS phases,
// the same barrier rule, a lane's slot 4 consecutive records -- with two sources
// and two sinks.  Global block b is piece b % npieces of row b / npieces, its
// virtual record e is record (piece << LR | e) of the row (LR < 13 only with
// npieces == 1: a block is a row).
//   source KEYS  the record of column c is formed in registers from
//                keys_in[row cols + c], T on real keys only;
//   source RECS  record i of a row of m candidate records;
//   sink RECS    the first k records of every block go to
//                recs_out[(row npieces + piece) k + j]: the block's candidates;
//   sink SPLIT   (npieces == 1, the last pass) keys_out[row k + j] = unT of the
//                high half (null keys_out: none), idx_out[row k + j] = the low.
// A sorted block holds the k smallest records of its piece, and a row's k
// smallest records are among the k smallest of its pieces, so a pass KEYS ->
// RECS over pieces of 2^13 leaves npieces k candidates per row, RECS -> RECS
// passes shrink them while they are more than a tile, and a pass -> SPLIT over
// one block per row ends it (topk_plan.h; rows up to 2^13: KEYS -> SPLIT alone).
// The records of a row are distinct (their columns are), so the result does
// not depend on how the row was cut.
//
// Sentinels: a virtual record past its row (column >= cols, or record >= m), or
// of a row >= rows, is the all-ones record; so is what sink RECS writes where a
// block has fewer than k real records (the block is ascending, they come
// last).  cols <= 2^31, so the low half of a real record is below 2^31 and NO
// real record equals the sentinel: sentinels are strictly the largest records
// of every block, and since k <= cols real records exist in a row none of them
// is among the first k of the row's last pass -- no sentinel reaches an output.
// The case that needs the low half: the largest direction on the u32 key 0, or
// on the f32 pattern 0xFFFFFFFF whose K is 0.  T is all-ones there, the record's
// high half equals the sentinel's, and only the column (< 2^31 <= 0xFFFFFFFF)
// keeps the record below it.
//
// Aliasing: none.  Sink SPLIT writes row k + j while other tiles still read
// their rows, so an output must not overlap the input (the runtime refuses it).
#include "bitonic.h"
#include "topk_plan.h"

namespace misort {

namespace {

// flags: bit 0 = 16-byte loads of the keys (keys_in 16-byte aligned and cols a
// multiple of 4, so every slot lies inside one row, aligned: RP_VEC's rule),
// else element loads; bit 1 = f32 keys (ord_of_f32 on real keys, f32_of_ord in
// sink SPLIT); bit 2 = the largest keys (T = ~K); bit 3 = 16-byte stores of sink
// SPLIT (the outputs in use 16-byte aligned and k a multiple of 4).
constexpr int TK_VEC = 1, TK_F32 = 2, TK_LARGEST = 4, TK_VEC_OUT = 8;
constexpr int TK_LT = KT<uint64_t>::LT;
static_assert(TK_LT == TOPK_LT, "the plan cuts rows into tiles of the u64 SORT tile");
static_assert(ROWS_LR_MIN == TOPK_LR_MIN, "the plan's shortest block is the row tile's");

struct TopkArgs {
    const uint32_t* keys_in;   // source KEYS
    const uint64_t* recs_in;   // source RECS
    uint64_t* recs_out;        // sink RECS
    uint32_t *keys_out, *idx_out;  // sink SPLIT
    int64_t rows, m, k, npieces, tile0;
    int flags;
};

__device__ __forceinline__ uint32_t tk_map(uint32_t x, bool f32, bool largest) {
    const uint32_t o = f32 ? ord_of_f32(x) : x;
    return largest ? ~o : o;
}
__device__ __forceinline__ uint32_t tk_unmap(uint32_t t, bool f32, bool largest) {
    const uint32_t o = largest ? ~t : t;
    return f32 ? f32_of_ord(o) : o;
}

template <int LR, bool RECS_IN, bool SPLIT>
__global__ __launch_bounds__((TileGeo<uint64_t, TK_LT>::NT), (TileGeo<uint64_t, TK_LT>::WAVES_PER_EU)) void
k_topk(TopkArgs a) {
    typedef uint64_t K;
    constexpr int LT = TK_LT;
    typedef TileGeo<K, LT> G;
    static_assert(LR >= ROWS_LR_MIN && LR <= LT, "a block is a lane's 32 records .. the tile");
    constexpr int W = 4;
    typedef uint32_t u32xw __attribute__((ext_vector_type(W)));
    constexpr int LOADS = 32 / W;
    constexpr int CM = (1 << LR) - 1;
    __shared__ __attribute__((aligned(16))) K s[lds_words(G::T)];
    const int t = threadIdx.x;
    const int64_t tile = a.tile0 + blockIdx.x;
    // LR == LT: the tile is one block, a piece of a row; else its blocks are whole rows
    int64_t row0, piece;
    if constexpr (LR == LT) {
        row0 = tile / a.npieces;
        piece = tile - row0 * a.npieces;
    } else {
        row0 = tile << (LT - LR);
        piece = 0;
    }
    const int64_t rec0 = piece << LR;  // the block's first record in its row (LR < LT: 0)
    const int64_t rows = a.rows, m = a.m;
    const bool vec = a.flags & TK_VEC;
    const bool f32 = a.flags & TK_F32;
    const bool largest = a.flags & TK_LARGEST;
    K pre[LOADS][W];
#pragma unroll
    for (int k = 0; k < LOADS; ++k) {
        const int e = (k * G::NT + t) * W;
        const int64_t r = row0 + (e >> LR);
        const int64_t c = rec0 + (e & CM);
        const int64_t off = r * m + c;
        if constexpr (RECS_IN) {
#pragma unroll
            for (int j = 0; j < W; ++j) {
                K x = ~(K)0;
                if (r < rows && c + j < m) x = a.recs_in[off + j];
                pre[k][j] = x;
            }
        } else if (vec) {
            const bool real = r < rows && c < m;  // cols % W == 0: the whole slot or none of it
            u32xw x = {};
            if (real) x = __builtin_nontemporal_load(reinterpret_cast<const u32xw*>(a.keys_in + off));
#pragma unroll
            for (int j = 0; j < W; ++j)
                pre[k][j] = real ? (K)tk_map(x[j], f32, largest) << 32 | (uint32_t)(c + j) : ~(K)0;
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j) {
                K x = ~(K)0;
                if (r < rows && c + j < m) x = (K)tk_map(a.keys_in[off + j], f32, largest) << 32 | (uint32_t)(c + j);
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
    // the first k records of every block: slots at or past k have nothing to store
    const int64_t kk = a.k;
#pragma unroll
    for (int k = 0; k < LOADS; ++k) {
        const int e = (k * G::NT + t) * W;
        const int64_t r = row0 + (e >> LR);
        const int j0 = e & CM;
        if (r >= rows || j0 >= kk) continue;
        if constexpr (SPLIT) {
            const int64_t off = r * kk + j0;
            u32xw x, v;
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const K rec = s[pad(e + j)];
                x[j] = tk_unmap((uint32_t)(rec >> 32), f32, largest);  // never stored where it is a sentinel
                v[j] = (uint32_t)rec;
            }
            if (a.flags & TK_VEC_OUT) {  // k % W == 0: the whole slot is below k
                if (a.keys_out) *reinterpret_cast<u32xw*>(a.keys_out + off) = x;
                *reinterpret_cast<u32xw*>(a.idx_out + off) = v;
            } else {
#pragma unroll
                for (int j = 0; j < W; ++j)
                    if (j0 + j < kk) {
                        if (a.keys_out) a.keys_out[off + j] = x[j];
                        a.idx_out[off + j] = v[j];
                    }
            }
        } else {
            const int64_t off = (r * a.npieces + piece) * kk + j0;
#pragma unroll
            for (int j = 0; j < W; ++j)
                if (j0 + j < kk) a.recs_out[off + j] = s[pad(e + j)];
        }
    }
}

template <int LR, bool RECS_IN, bool SPLIT>
void launch_topk(TopkArgs a, int64_t ntiles, hipStream_t s) {
    constexpr int64_t MAX_GRID = 0x7FFFFFFF;
    for (int64_t t0 = 0; t0 < ntiles; t0 += MAX_GRID) {
        const int64_t g = ntiles - t0 < MAX_GRID ? ntiles - t0 : MAX_GRID;
        a.tile0 = t0;
        k_topk<LR, RECS_IN, SPLIT><<<dim3((unsigned)g), dim3(TileGeo<uint64_t, TK_LT>::NT), 0, s>>>(a);
    }
}

template <bool RECS_IN>
bool launch_topk_split(int lr, const TopkArgs& a, int64_t ntiles, hipStream_t s) {
    switch (lr) {
#define MISORT_TOPK_CASE(LR_) \
    case LR_:                 \
        launch_topk<LR_, RECS_IN, true>(a, ntiles, s); \
        return true
        MISORT_TOPK_CASE(5);
        MISORT_TOPK_CASE(6);
        MISORT_TOPK_CASE(7);
        MISORT_TOPK_CASE(8);
        MISORT_TOPK_CASE(9);
        MISORT_TOPK_CASE(10);
        MISORT_TOPK_CASE(11);
        MISORT_TOPK_CASE(12);
        MISORT_TOPK_CASE(13);
#undef MISORT_TOPK_CASE
    default:
        return false;
    }
}

}  // namespace

hipError_t topk_pass(const TopkPass& p, const uint32_t* keys_in, const uint64_t* recs_in, uint64_t* recs_out,
                     uint32_t* keys_out, uint32_t* idx_out, int64_t rows, int64_t k, bool f32, bool largest,
                     hipStream_t s, LaunchHook* hook) {
    if (rows <= 0 || k <= 0) return hipSuccess;
    const bool split = p.npieces == 1;  // the plan's last pass
    if (p.lr < ROWS_LR_MIN || p.lr > TK_LT || p.npieces < 1 || (p.lr < TK_LT && !split) ||
        p.m_in > (p.npieces << p.lr) || k > p.m_in || k > ((int64_t)1 << p.lr) || (keys_in != nullptr) == (recs_in != nullptr) ||
        (split ? !idx_out : !recs_out))
        return hipErrorInvalidValue;
    TopkArgs a;
    a.keys_in = keys_in, a.recs_in = recs_in, a.recs_out = recs_out, a.keys_out = keys_out, a.idx_out = idx_out;
    a.rows = rows, a.m = p.m_in, a.k = k, a.npieces = p.npieces, a.tile0 = 0;
    a.flags = (keys_in && aligned16(keys_in) && p.m_in % 4 == 0 ? TK_VEC : 0) | (f32 ? TK_F32 : 0) |
              (largest ? TK_LARGEST : 0) |
              (split && aligned16(keys_out) && aligned16(idx_out) && k % 4 == 0 ? TK_VEC_OUT : 0);
    const int64_t ntiles =
        p.lr == TK_LT ? rows * p.npieces : (rows + (1 << (TK_LT - p.lr)) - 1) >> (TK_LT - p.lr);
    const double in_bytes = (keys_in ? 4.0 : 8.0) * (double)rows * (double)p.m_in;
    const double out_bytes = split ? (keys_out ? 8.0 : 4.0) * (double)rows * (double)k : 8.0 * (double)rows * (double)p.m_out;
    HookScope hs(hook, KIND_TILE_SORT, in_bytes + out_bytes, s);
    bool ok = true;
    if (!split) {
        if (recs_in) launch_topk<TK_LT, true, false>(a, ntiles, s);
        else launch_topk<TK_LT, false, false>(a, ntiles, s);
    } else {
        ok = recs_in ? launch_topk_split<true>(p.lr, a, ntiles, s) : launch_topk_split<false>(p.lr, a, ntiles, s);
    }
    if (!ok) return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace misort

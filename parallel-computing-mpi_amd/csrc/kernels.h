// kernels.h -- internal launch interface of the gfx950 bitonic kernels
// (kernels.hip).  Not part of the public C-ABI (include/misort.h).
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>

namespace misort {

// IEEE double bits <-> order-preserving u64 (negative: all bits flipped; else
// the sign bit set), so every kernel compares unsigned integers.
__device__ __forceinline__ uint64_t ord_of_f64(uint64_t b) {
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ uint64_t f64_of_ord(uint64_t o) {
    return (o >> 63) ? (o & 0x7FFFFFFFFFFFFFFFull) : ~o;
}
// The same on 32 bits: IEEE float bits <-> order-preserving u32 (the f32 keys
// of the key-value sorts).
__device__ __forceinline__ uint32_t ord_of_f32(uint32_t b) { return (b >> 31) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ uint32_t f32_of_ord(uint32_t o) { return (o >> 31) ? (o & 0x7FFFFFFFu) : ~o; }

// Kernel families, used for per-launch profiling (HIP events) and reporting.
enum Kind : int {
    KIND_TILE_SORT = 0,   // levels 1..LT inside one LDS tile
    KIND_GLOBAL = 1,      // retired (round 3): network ROWS pass
    KIND_TILE_MERGE = 2,  // retired (round 3): network in-tile merge pass
    KIND_MERGE_SPLIT = 3, // compare-split merge (keep lowest/highest n)
    KIND_OTHER = 4,       // f64 transform, fills, checks
    KIND_SPAN = 5,        // retired (round 3): network SPAN pass
    KIND_WIDE = 6,        // retired (round 3): network wide ROWS pass
    KIND_RUNS = 7,        // one merge level: runs of 2^hi keys -> runs of 2^(hi+1)
    KIND_EXCHANGE = 8,    // compare-split exchange leg (samples, RCCL send/recv, codec); not a kernel
    KIND_RUNSK = 9,       // R merge levels in one pass: runs of 2^hi -> 2^(hi+R), 2^R-way (runsk.hip)
    KIND_RUNSK_KERNEL = 10,  // the k_mergek launch of a KIND_RUNSK pass alone (nested in it)
    KIND_MERGE_SPLIT_TAIL = 11,  // in-place compare-split of a small bracket; bytes: an UPPER bound
                                 // (2 na + min(na, nb) keys: the device finds the window it rewrites)
    KIND_COUNT = 12
};

// Per-launch hook: called before and after every kernel launch of a sort with
// the kernel kind and its algorithmic HBM bytes (each key read once and
// written once).  nullptr = no profiling.
//
// A hook that binds() times the local sort's passes by events the kernels
// carry themselves (hipExtLaunchKernelGGL start/stop: the dispatch's own
// timestamps, no marker packets between the kernels): bind() hands out the
// events for the next launch (either may be null); kernel_kind >= 0 records
// that launch, pass_kind >= 0 the pass it ends (from the end of this sort's
// previous pass; bind_reset() starts a sort), both -1 binds a tick (the stop
// of the launch before a recorded one, where the hook times a launch from the
// previous one's end).
struct LaunchHook {
    virtual void before(Kind k, double bytes, hipStream_t s) = 0;
    virtual void after(Kind k, hipStream_t s) = 0;
    virtual bool binds() const { return false; }
    virtual void bind_reset() {}
    virtual bool bind(int kernel_kind, int pass_kind, double bytes, hipEvent_t* start, hipEvent_t* stop) {
        (void)kernel_kind, (void)pass_kind, (void)bytes;
        *start = *stop = nullptr;
        return false;
    }
    virtual ~LaunchHook() = default;
};

// The hook's record of kind k around the launches of a scope (null hook: nothing).
struct HookScope {
    LaunchHook* h;
    Kind k;
    hipStream_t s;
    HookScope(LaunchHook* h_, Kind k_, double bytes, hipStream_t s_) : h(h_), k(k_), s(s_) {
        if (h) h->before(k, bytes, s);
    }
    ~HookScope() {
        if (h) h->after(k, s);
    }
};

// Host helpers the launchers share.  A null pointer is aligned: it is not accessed.
inline bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// The smallest k with 2^k >= n, capped at 62 (n may come from a caller: no shift past the sign bit).
inline int ceil_log2(int64_t n) {
    int k = 0;
    while (k < 62 && ((int64_t)1 << k) < n) ++k;
    return k;
}

// A kernel launch carrying timing events (either may be null), or a plain one.
template <typename F, typename... Args>
inline void launch_timed(F kernel, dim3 grid, dim3 block, uint32_t shmem, hipStream_t s, hipEvent_t start,
                         hipEvent_t stop, Args... args) {
    if (start || stop) hipExtLaunchKernelGGL(kernel, grid, block, shmem, s, start, stop, 0u, args...);
    else kernel<<<grid, block, shmem, s>>>(args...);
}

// Chunked first/last pass of a local sort, for host staging that overlaps the
// PCIe copies with the sort (misort_sort_host).  The SORT pass runs chunk by
// chunk; before chunk [k0, k1) is read, before_first(k0, k1, s) makes stream s
// wait for those input keys.  If after_last is set, the final pass (a
// contiguous-tile MERGE or SORT pass) also runs chunk by chunk and
// after_last(k0, k1, s) is called once output keys [k0, k1) are enqueued.
// `chunk` is a multiple of the SORT tile.
struct StageIO {
    int64_t chunk = 0;
    std::function<int(int64_t, int64_t, hipStream_t)> before_first;
    std::function<int(int64_t, int64_t, hipStream_t)> after_last;
};

// Local ascending sort of n keys: in -> out (in == out allowed).
// K = uint32_t or uint64_t.  ord_in: the input holds IEEE doubles that are
// mapped to order-preserving u64 on load (K must be uint64_t); the output
// then stays in that ordered form.  scratch (n keys, distinct from in and out,
// or nullptr) lets the passes ping-pong between two buffers instead of
// rewriting `out` in place (copy-shaped HBM traffic).
// ord_out (K = uint64_t): the output is mapped back to IEEE double bits --
// by the last pass's stores when it is a multi-way pass, else by one more
// sweep (small sorts).
// block_log2 > 0 (the row sort's long rows): n is a multiple of 2^block_log2
// and every aligned 2^block_log2-key block is sorted on its own -- the passes
// are those of a 2^block_log2-key sort, run over all n keys (io must be null).
template <typename K>
hipError_t local_sort(const K* in, K* out, int64_t n, bool ord_in, K* scratch, hipStream_t s,
                      LaunchHook* hook, const StageIO* io = nullptr, bool ord_out = false, int block_log2 = 0);

// One HBM pass of a plan's shape over n keys (kind KIND_TILE_SORT, KIND_RUNS
// or KIND_RUNSK; hi, R as in the plan): probes and tests.
template <typename K>
hipError_t run_pass(const K* in, K* out, int64_t n, int kind, int hi, int R, int flip, hipStream_t s);

// Compare-split merge (device half of psort.cc:116-164): out[0..na) = the na
// smallest (keep_max=0) or largest (keep_max=1) keys of A U B, ascending.
// scratch must hold ceil(na/2048)+1 int64 co-ranks.
// ord_out (K = uint64_t): out gets IEEE double bits (the sort's last stage over f64 keys).
template <typename K>
hipError_t merge_split(const K* a, int64_t na, const K* b, int64_t nb, K* out,
                       int keep_max, int64_t* scratch, hipStream_t s, LaunchHook* hook, bool ord_out = false);

// The same compare-split IN PLACE when b touches one end of a: only the
// affected window of a (found on the device: keep-min, a's keys after b[0];
// keep-max, a's keys up to b[nb-1]) is staged into `stage` (same offsets) and
// merged back; O(window + nb) instead of O(na).  scratch holds
// ceil(na/2048) + 6 int64.
template <typename K>
hipError_t merge_split_tail(K* a, int64_t na, const K* b, int64_t nb, int keep_max, K* stage, int64_t* scratch,
                            hipStream_t s, LaunchHook* hook);

// Full merge of two ascending runs: out[0..na+nb) (A first on ties; for pure
// keys the result equals std::sort of the concatenation).  scratch holds
// ceil((na+nb)/2048)+1 int64 co-ranks.
template <typename K>
hipError_t merge_full(const K* a, int64_t na, const K* b, int64_t nb, K* out, int64_t* scratch, hipStream_t s,
                      LaunchHook* hook);

// One merge level of the local sort (runs.hip): src holds ascending runs of
// 2^lw keys (the last may be short), dst gets the ascending runs of 2^(lw+1).
// Only output keys [o0, o1) are written (o0 a multiple of 4096, o1 of 4096 or
// n; o1 <= 0 means n): the chunked last pass of host staging.  src != dst.
// hook: a binding hook times the level's merge launch as a KIND_RUNS pass.
template <typename K>
hipError_t merge_level(const K* src, K* dst, int64_t n, int lw, hipStream_t s, int64_t o0 = 0, int64_t o1 = 0,
                       LaunchHook* hook = nullptr);

// Fence stride of the multi-way passes (log2 keys).
constexpr int MERGEK_FENCE_LOG2 = 7;  // runsk_fg6.hip: 6 (fence stride 256 measured equal to 128, profiles/r02)
// log2 keys of the u32 SORT tiles (bitonic.h).  15: 1024 lanes, one
// workgroup per CU, all 15 levels as the bitonic network.  14: 512 lanes, two
// workgroups per CU, levels 11..14 as in-LDS merge levels (SORT_MERGE_F).
// The plan picks per size (sort_tile_u32); u32 multi-way passes take runs of
// 2^14 and up.
constexpr int SORT_LT_U32 = 15, SORT_LT_MERGE = 14;

// The multi-way merge passes (runsk.hip) are built once per fence stride; each
// build exports this one handle.
struct MergekBuild {
    int fence_log2;  // a fence every 2^fence_log2 keys of a run
    // lk merge levels in one HBM pass (u32 and u64, lk = 1..4): src holds
    // ascending runs of 2^lw keys, dst gets ascending runs of 2^(lw+lk) (2^lk-way
    // merge of each group of runs; the last group may be short).  Chunks are cut
    // at fences: `phase` selects which of two per-stream fence buffers holds this
    // pass's fences; gather = build them from src first (the pass after a
    // non-multi-way pass); lk_next > 0 = write the fences of the next multi-way
    // pass (runs of 2^(lw+lk), groups of 2^lk_next) into the other buffer.
    // u32: SORT_LT_MERGE <= lw, lw + lk <= 30.  u64: 128-bit fences (key << 64 |
    // run/position tag), 13 <= lw, lw + lk <= 29.  src != dst; buffers 16-byte
    // aligned.  ord_out (u64 only): the pass is the sort's last (lk_next = 0) and
    // writes IEEE double bits (f64_of_ord in its stores: no separate sweep).
    hipError_t (*levelk_u32)(const uint32_t* src, uint32_t* dst, int64_t n, int lw, int lk, hipStream_t s, int phase,
                             bool gather, int lk_next, LaunchHook* hook, bool ord_out);
    hipError_t (*levelk_u64)(const uint64_t* src, uint64_t* dst, int64_t n, int lw, int lk, hipStream_t s, int phase,
                             bool gather, int lk_next, LaunchHook* hook, bool ord_out);
    // The per-stream fence buffer `phase` of a pass over n keys (the one
    // merge_levelk reads with that phase), for a SORT pass that writes the first
    // pass's fences itself; null on allocation failure.
    void* (*fence_buffer)(int64_t n, int key_bytes, int phase, hipStream_t s);
    // 1 if a pass on stream s rejected a chunk since the last call (the stream
    // is synchronised), else 0; negative on a HIP error.
    int (*take_error)(hipStream_t s);
    // Frees the fence and planning scratch kept for stream s on the current device.
    void (*release)(hipStream_t s);

    hipError_t merge_levelk(const uint32_t* src, uint32_t* dst, int64_t n, int lw, int lk, hipStream_t s, int phase,
                            bool gather, int lk_next, LaunchHook* hook = nullptr, bool ord_out = false) const {
        return levelk_u32(src, dst, n, lw, lk, s, phase, gather, lk_next, hook, ord_out);
    }
    hipError_t merge_levelk(const uint64_t* src, uint64_t* dst, int64_t n, int lw, int lk, hipStream_t s, int phase,
                            bool gather, int lk_next, LaunchHook* hook = nullptr, bool ord_out = false) const {
        return levelk_u64(src, dst, n, lw, lk, s, phase, gather, lk_next, hook, ord_out);
    }
};
// The build for a fence stride, and every build's stride (runsk.hip, runsk_fg6.hip).
const MergekBuild& mergek_build(int fence_log2);
constexpr int MERGEK_BUILDS[2] = {MERGEK_FENCE_LOG2, 6};
// The fence stride (log2 keys) the local sort of n keys uses: 6 (runsk_fg6)
// from 2^MISORT_FENCE_FG6_MIN keys (u32: never by default, u64: 29), else MERGEK_FENCE_LOG2.
int mergek_fence_log2(int64_t n, int key_bytes);
int merge_levelk_lw_min(int key_bytes);   // shortest input runs (log2) of a multi-way pass
int merge_levelk_lwk_max(int key_bytes);  // largest output runs (log2)

// psort.cc:88-101 lower_bound on a sorted device run: *d_out = first i with
// x <= a[i], or n.
template <typename K>
hipError_t lower_bound(const K* a, int64_t n, K x, int64_t* d_out, hipStream_t s);

// lb[v] / ub[v] = first index with a[i] >= vals[v] / a[i] > vals[v] in a
// sorted run (device arrays of nv entries).
template <typename K>
hipError_t bounds(const K* a, int64_t n, const K* vals, int nv, int64_t* lb, int64_t* ub, hipStream_t s);

// Local descents a[i] > a[i+1] (psort.cc:497-501), compared as T
// (uint32_t, uint64_t or double); result added to *count (device u64).
template <typename T>
hipError_t count_descents(const T* a, int64_t n, unsigned long long* count, hipStream_t s);

// out[c] = a[min(c*stride, n-1)] for c in [0, count): the splitter samples of a
// sorted block used to bracket the compare-split crossing point.
template <typename K>
hipError_t gather_samples(const K* a, int64_t n, int64_t stride, K* out, int64_t count, hipStream_t s);

// The compare-split bracket on the device: from the partners' samples (sa of
// the keep-min side's na keys, sb of the keep-max side's nb keys, as
// gather_samples takes them) run[0..1] = {send offset, k} of this rank's
// message (keep_max: its bottom k keys; else its top k of nloc).
template <typename K>
hipError_t exchange_count(const K* sa, int64_t na, const K* sb, int64_t nb, int keep_max, int64_t nloc,
                          int64_t* run, hipStream_t s);

// IEEE double bits <-> order-preserving u64, in place.
hipError_t f64_to_ord(uint64_t* a, int64_t n, hipStream_t s);
hipError_t ord_to_f64(uint64_t* a, int64_t n, hipStream_t s);
hipError_t ord_to_f64_copy(const uint64_t* a, uint64_t* b, int64_t n, hipStream_t s);  // b = f64 bits of a

// Key-value records of the pair sort (pairs.hip): rec[i] = K(keys[i]) << 32 | v,
// v = vals[i], or val_base + (uint32_t)i when vals is null; K is the identity
// (u32 keys) or, f32, the 32-bit form of ord_of_f64.  unzip_pairs is the
// inverse; a null `keys` writes the values only.  rec is 16-byte aligned; the
// caller's arrays need 4-byte alignment only (16-byte aligned ones take the
// vector kernel).  Records of KIND_OTHER with the bytes moved.
hipError_t zip_pairs(const uint32_t* keys, const uint32_t* vals, uint32_t val_base, uint64_t* rec, int64_t n,
                     bool f32, hipStream_t s, LaunchHook* hook);
hipError_t unzip_pairs(const uint64_t* rec, uint32_t* keys, uint32_t* vals, int64_t n, bool f32, hipStream_t s,
                       LaunchHook* hook);

// The three kernels around the two u64 sorts of the 64-bit key-value sort
// (pairs.hip; K = ord_of_f64 for f64 keys, else the identity; n <= 2^32):
//   zip_lo64     rec[i] = lo(K(keys[i])) << 32 | i;
//   gather_hi64  rec[j] = hi(K(keys[s1[j] & 0xFFFFFFFF])) << 32 | j, s1 the sorted
//                records of zip_lo64 (rec != s1);
//   emit64       for output t, with j = s2[t] & 0xFFFFFFFF (s2: the sorted records
//                of gather_hi64), r = s1[j], i = (uint32_t)r: keys_out[t] (if
//                keys_out) = the key rebuilt from hi(s2[t]) and hi(r); vals_out[t]
//                = vals_in[i] (val_bytes 4 or 8), or the u32 index i when vals_in
//                is null (val_bytes 4).
// rec, s1, s2 are 16-byte aligned; the caller's arrays need element alignment
// only.  Records of KIND_OTHER: 16n, 24n and 16n + written bytes + gathered values.
hipError_t zip_lo64(const uint64_t* keys, uint64_t* rec, int64_t n, bool f64, hipStream_t s, LaunchHook* hook);
hipError_t gather_hi64(const uint64_t* s1, const uint64_t* keys, uint64_t* rec, int64_t n, bool f64, hipStream_t s,
                       LaunchHook* hook);
hipError_t emit64(const uint64_t* s2, const uint64_t* s1, const void* vals_in, int val_bytes, uint64_t* keys_out,
                  void* vals_out, int64_t n, bool f64, hipStream_t s, LaunchHook* hook);

// Row-wise sort (rows_tile.h, rows.hip): every row of a row-major rows x cols
// array ascending, on its own.
//   sort_rows_tile  cols <= 2^tile_log2: one SORT pass, 2^(LT - LR) rows of
//                   2^LR >= cols virtual keys per LDS tile (in == out allowed;
//                   element alignment).  f64 (K = uint64_t): IEEE double bits in
//                   and out.  One KIND_TILE_SORT record of 2 rows cols keys.
//   pad_rows        pad[r << k | c] = K(in[r cols + c]) for c < cols, all-ones
//                   for cols <= c < 2^k (K = ord_of_f64 for f64 keys);
//   unpad_rows      out[r cols + c] = unK(pad[r << k | c]) for c < cols.
// pad is 16-byte aligned, 2^k >= 16 bytes of keys; the caller's arrays need
// element alignment only.  The two sweeps are one pair of kernels for keys and
// for the pairs below (rows.hip; rows_io.h says what a slot reads and writes).  Records of KIND_OTHER, each counted as
// (rows cols + rows 2^k) keys (unpad skips the vectors that hold padding only).
template <typename K>
hipError_t sort_rows_tile(const K* in, K* out, int64_t rows, int64_t cols, bool f64, hipStream_t s,
                          LaunchHook* hook);
hipError_t pad_rows(const void* in, void* pad, int64_t rows, int64_t cols, int k, int key_bytes, bool f64,
                    hipStream_t s, LaunchHook* hook);
hipError_t unpad_rows(const void* pad, void* out, int64_t rows, int64_t cols, int k, int key_bytes, bool f64,
                      hipStream_t s, LaunchHook* hook);
// Row-wise key-value sort of 32-bit keys with 32-bit values (rows_pairs.hip,
// rows.hip): every row ascending by the record K(key) << 32 | value, K the
// identity or (f32) ord_of_f32.  vals_in null: the value of (r, c) is c;
// keys_out null: no keys are written.  An output may be exactly an input.
//   sort_rows_pairs_tile  cols <= 2^13: the u64 row tile with the record formed
//                   in registers as the tile loads and split as it stores.  One
//                   KIND_TILE_SORT record of the bytes of the arrays in use
//                   (4 rows cols each).  Element alignment; 16-byte accesses
//                   when every array in use is 16-byte aligned and cols is a
//                   multiple of 4, 8-byte ones when 8-byte aligned and cols even.
//   pad_rows_pairs  pad[r << k | c] = the record of (r, c) for c < cols,
//                   all-ones for cols <= c < 2^k;
//   unpad_rows_pairs  keys_out / vals_out[r cols + c] from pad[r << k | c], c < cols.
// pad is 16-byte aligned, k >= 1.  Records of KIND_OTHER: pad counts the caller's
// arrays it reads and rows 2^k records, unpad rows cols records and the arrays
// it writes.
hipError_t sort_rows_pairs_tile(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out,
                                uint32_t* vals_out, int64_t rows, int64_t cols, bool f32, hipStream_t s,
                                LaunchHook* hook);
hipError_t pad_rows_pairs(const uint32_t* keys_in, const uint32_t* vals_in, uint64_t* pad, int64_t rows, int64_t cols,
                          int k, bool f32, hipStream_t s, LaunchHook* hook);
hipError_t unpad_rows_pairs(const uint64_t* pad, uint32_t* keys_out, uint32_t* vals_out, int64_t rows, int64_t cols,
                            int k, bool f32, hipStream_t s, LaunchHook* hook);
// How a row sort of `cols` keys runs (host only): *path 0 = sort_rows_tile
// (*block_log2 = LR, *tile_log2 = LT, one KIND_TILE_SORT record), 1 = padded
// blocks (*block_log2 = ceil_log2(cols), the passes of plan_passes(2^block_log2)).
// Records as plan_passes; returns the count.
int rows_plan(int64_t cols, int key_bytes, int* path, int* tile_log2, int* block_log2, int* out, int max);
// Rows shorter than 2^ROWS_LR_MIN keys are sorted as 2^ROWS_LR_MIN virtual keys
// (one lane's registers).
constexpr int ROWS_LR_MIN = 5;

// Row-wise top-k of 32-bit keys (topk.hip): one pass of the plan of topk_plan.h
// over every row.  It sorts blocks of 2^p.lr ascending records T(key) << 32 |
// column in the u64 row tile (T = K or, largest, ~K; K the identity or, f32,
// ord_of_f32) and keeps the first k of each.  Exactly one source: keys_in (the
// caller's rows x p.m_in keys; the records are formed in registers) or recs_in
// (rows x p.m_in candidate records).  p.npieces > 1: the candidates go to
// recs_out[(row p.npieces + piece) k + j]; p.npieces == 1, the last pass:
// keys_out (may be null) / idx_out[row k + j].  No output may overlap an input.
// Element alignment; 16-byte key loads when keys_in is 16-byte aligned and
// p.m_in a multiple of 4.  One KIND_TILE_SORT record of the bytes read and written.
struct TopkPass;
hipError_t topk_pass(const TopkPass& p, const uint32_t* keys_in, const uint64_t* recs_in, uint64_t* recs_out,
                     uint32_t* keys_out, uint32_t* idx_out, int64_t rows, int64_t k, bool f32, bool largest,
                     hipStream_t s, LaunchHook* hook);

// Segmented sort (segs.hip, segs_tile.h): segment i of a caller's array is
// [off[i], off[i + 1]), off a device array of nseg + 1 int64; its class is
// segment_class(len) of segs_class.h, which also lays out the header.
//   seg_count       validates and classifies every segment into the zeroed
//                   header hdr (SEG_H_WORDS 64-bit words); reads only off[0..nseg];
//   seg_scatter     writes every non-empty segment's index into its class's
//                   list: cursor[class] (64-bit words, the host's list bases) is
//                   advanced; `listed` is the lists' total length;
//   sort_segs_tile  one class lr <= tile_log2: the `count` segments of `list`,
//                   2^(LT - lr) per LDS tile, levels 1..lr (in == out allowed).
//                   One KIND_TILE_SORT record of 2 `keys` keys;
//   pad_segs        one class k > tile_log2: pad[r << k | c] = K(in[begin + c])
//                   for c < len of segment list[r], all-ones above;
//   unpad_segs      out[begin + c] = unK(pad[r << k | c]) for c < len.
// pad is 16-byte aligned; the caller's arrays need element alignment only.
// Count, scatter, pad and unpad are records of KIND_OTHER with the bytes moved
// (`keys`: the class's key total).
hipError_t seg_count(const int64_t* off, int64_t nseg, int64_t n, int key_bytes, void* hdr, hipStream_t s,
                     LaunchHook* hook);
hipError_t seg_scatter(const int64_t* off, int64_t nseg, int key_bytes, void* cursor, uint32_t* lists,
                       int64_t listed, hipStream_t s, LaunchHook* hook);
template <typename K>
hipError_t sort_segs_tile(const K* in, K* out, const int64_t* off, const uint32_t* list, int64_t count, int lr,
                          int64_t keys, bool f64, hipStream_t s, LaunchHook* hook);
hipError_t pad_segs(const void* in, const int64_t* off, const uint32_t* list, int64_t count, int64_t keys, void* pad,
                    int k, int key_bytes, bool f64, hipStream_t s, LaunchHook* hook);
hipError_t unpad_segs(const void* pad, void* out, const int64_t* off, const uint32_t* list, int64_t count,
                      int64_t keys, int k, int key_bytes, bool f64, hipStream_t s, LaunchHook* hook);

// Segmented key-value sort of 32-bit keys with 32-bit values (segs_pairs.hip):
// every segment ascending by the record K(key) << 32 | value, K the identity or
// (f32) ord_of_f32.  The offset sweeps, the classes and the lists are the ones
// above with key_bytes = 8.  vals_in null: the value of element begin + c is c;
// keys_out null: no keys are written.  An output may be exactly an input.
//   sort_segs_pairs_tile  one class lr = 5..13: the `count` segments of `list`,
//                   2^(13 - lr) per u64 LDS tile, the record formed in registers
//                   as the tile loads and split as it stores.  One KIND_TILE_SORT
//                   record of the bytes of the arrays in use (4 `keys` each);
//   pad_segs_pairs  one class k > 13: pad[r << k | c] = the record of element
//                   begin + c for c < len of segment list[r], all-ones above;
//   unpad_segs_pairs  keys_out / vals_out[begin + c] from pad[r << k | c], c < len.
// pad is 16-byte aligned; the caller's arrays need 4-byte alignment only.
// Records of KIND_OTHER: pad counts the caller's arrays it reads and count 2^k
// records, unpad `keys` records and the arrays it writes.
hipError_t sort_segs_pairs_tile(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out,
                                uint32_t* vals_out, const int64_t* off, const uint32_t* list, int64_t count, int lr,
                                int64_t keys, bool f32, hipStream_t s, LaunchHook* hook);
hipError_t pad_segs_pairs(const uint32_t* keys_in, const uint32_t* vals_in, const int64_t* off, const uint32_t* list,
                          int64_t count, int64_t keys, uint64_t* pad, int k, bool f32, hipStream_t s,
                          LaunchHook* hook);
hipError_t unpad_segs_pairs(const uint64_t* pad, uint32_t* keys_out, uint32_t* vals_out, const int64_t* off,
                            const uint32_t* list, int64_t count, int64_t keys, int k, bool f32, hipStream_t s,
                            LaunchHook* hook);

// Segmented top-k of 32-bit keys (topk_segs.hip): the k best keys of every
// segment and their positions inside it, into row `segment` of nseg x k outputs;
// records, maps and order as topk_pass, classes and lists as the segmented
// sorts with key_bytes = 8 (topk_segs_plan.h says what runs per class).
//   topk_segs_tile    one class lr = 5..13, keys -> outputs: the `count` segments
//                     of `list`, 2^(13 - lr) per LDS tile; slots j < min(len, k)
//                     of a row are written.  One KIND_TILE_SORT record;
//   topk_segs_pieces  one class cls >= 14, keys -> candidates: cand[(r P + piece)
//                     k + j], P = 2^(cls - 13), r the segment's place in `list`:
//                     `count` uniform rows of P k records for topk_pass (k <=
//                     2^10).  One KIND_TILE_SORT record;
//   topk_segs_last    a long class's last pass p (p.npieces == 1), records ->
//                     outputs: row r of `count` rows of p.m_in records goes to
//                     row list[r] of the outputs.  One KIND_TILE_SORT record;
//   topk_segs_fill    slots [len, k) of every row with len < k: the index
//                     0xFFFFFFFF and (keys_out given) the fill key, the unmapped
//                     all-ones key.  Reads only off[0..nseg].  One KIND_OTHER record.
// keys_out may be null.  No output may overlap an input.  Element alignment.
hipError_t topk_segs_tile(const uint32_t* keys_in, uint32_t* keys_out, uint32_t* idx_out, const int64_t* off,
                          const uint32_t* list, int64_t count, int lr, int64_t keys, int64_t k, bool f32,
                          bool largest, hipStream_t s, LaunchHook* hook);
hipError_t topk_segs_pieces(const uint32_t* keys_in, uint64_t* cand, const int64_t* off, const uint32_t* list,
                            int64_t count, int cls, int64_t keys, int64_t k, bool f32, bool largest, hipStream_t s,
                            LaunchHook* hook);
hipError_t topk_segs_last(const TopkPass& p, const uint64_t* recs_in, uint32_t* keys_out, uint32_t* idx_out,
                          const uint32_t* list, int64_t count, int64_t k, bool f32, bool largest, hipStream_t s,
                          LaunchHook* hook);
hipError_t topk_segs_fill(const int64_t* off, int64_t nseg, int64_t k, uint32_t* keys_out, uint32_t* idx_out,
                          bool f32, bool largest, hipStream_t s, LaunchHook* hook);

// Counter-based SplitMix64 keys for global indices [g0, g0+n) (bench/test input).
hipError_t fill_splitmix_u32(uint32_t* out, int64_t n, uint64_t seed, int64_t g0, hipStream_t s);
hipError_t fill_splitmix_u64(uint64_t* out, int64_t n, uint64_t seed, int64_t g0, hipStream_t s);

// Lossless delta coding of a sorted run (codec.hip), for the compare-split
// exchange: blocks of 1024 keys, first key + gaps packed at the block's width.
// codec_encode writes the stream to `out` (<= codec_max_words(n) u32 words)
// and sizes[0..1] = {coded words, raw words} (device int64); scratch holds
// codec_scratch_bytes(n) bytes.  codec_encode_dev does the same for the run
// base + run[0] of run[1] keys, both device int64, run[1] <= n_max.
// codec_decode restores the n keys.
int64_t codec_blocks(int64_t n);
size_t codec_scratch_bytes(int64_t n);
int64_t codec_max_words(int64_t n, int key_bytes);
template <typename K>
hipError_t codec_encode(const K* keys, int64_t n, uint32_t* out, void* scratch, size_t scratch_bytes,
                        int64_t* sizes, hipStream_t s);
template <typename K>
hipError_t codec_encode_dev(const K* base, const int64_t* run, int64_t n_max, uint32_t* out, void* scratch,
                            size_t scratch_bytes, int64_t* sizes, hipStream_t s);
template <typename K>
hipError_t codec_decode(const uint32_t* in, int64_t n, K* keys, hipStream_t s);

// Tile geometry per key type (exported for documentation/tests).
int tile_log2(int key_bytes);

// The HBM pass plan local_sort runs for n keys of key_bytes (4 or 8): writes
// up to max passes as 4 ints each (kind, hi, R, flip) and returns the count.
int plan_passes(int64_t n, int key_bytes, int* out, int max);

}  // namespace misort

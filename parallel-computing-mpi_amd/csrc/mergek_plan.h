// mergek_plan.h -- the host side of a multi-way merge pass (runsk.hip) as plain
// C++17: the chunk shapes, the group geometry, the environment knobs and
// plan_pass(), which turns (n, lw, depth, knobs) into every decision, count and
// workspace offset merge_pass launches with.  No HIP include: mergek_plan_dump.cpp
// builds it with the host compiler alone and prints the plans
// (tests/test_runsk_model.py).
//
// Included once per fence stride, inside that build's anonymous namespace, with
// MISORT_RUNSK_FGL (log2 of the stride) defined and <stdint.h>, <stddef.h> and
// <stdlib.h> included before it; hence no include guard.
#ifdef __HIPCC__
#define MERGEK_HD __device__ __host__
#else
#define MERGEK_HD
#endif

constexpr int FG_LOG2 = MISORT_RUNSK_FGL;
constexpr int64_t FG = (int64_t)1 << FG_LOG2;  // fence stride (keys)
typedef unsigned __int128 u128;

// The first fence merge levels of a pass as LDS merge levels (k_fence_merge)
// when the pass has at least FENCE_MERGE_MIN_BLOCKS sub-groups; else ranks by
// binary searches (k_fence_lds), which can split a sub-group over several
// blocks.  Measured (profiles/r03/ab3): 2^30 u32 66.5 -> 67.0 Gkeys/s, 2^26
// 61.5 -> 62.1; at 2^24 (64 and 16 sub-groups) the merge was slower.
constexpr int64_t FENCE_MERGE_MIN_BLOCKS = 128;

// Per key type: the fence type (key bits above 32 bits of run and position),
// the chunk workgroup (NT lanes x IT keys: CAP keys a chunk at most), the
// workgroups per CU the LDS tile allows, and the largest fence sub-group
// merged in LDS (64 KiB).
template <typename KEY>
struct KTr;
// u32, 2..8-way passes: 512 lanes x 18 outputs, 8960-key chunks (the largest
// the 18-output level layout fits: CAP + 4 (G + QA) <= 9216; 8192 before: 2^24
// +1.5 %, 2^28 +0.8 %, profiles/r04/chunk32), four workgroups per CU; 22
// outputs per lane at three per CU measured slower (profiles/r06/plan/fg6_ab.txt).
// 16-way passes: larger chunks.  A chunk holds FM * FG = CAP - K * FG keys on
// average, so at K = 16 a quarter of an 8192-key chunk's lanes idle.  Round
// 4: 22 outputs per lane (CAP 10752, three workgroups per CU) measured 2^30
// 68.9 -> 69.8 Gkeys/s; 20 or 24 per lane were slower -- an EVEN half (IT / 2
// = 10 or 12) puts the lanes' chain pointers, IT / 2 apart, on a few banks.
// Round 6: 26 outputs per lane (IT / 2 = 13, odd) and the LDS sized by the
// larger of the segments and the level outputs (not their sum): CAP 12864,
// the largest the 26-output level layout holds (CAP + 8 (G + QA) <= 512 * 26),
// still three workgroups per CU (53.4 KB); 2^30 k_mergek 2154 -> 2049 us,
// 81.6 -> 84.4 Gkeys/s, 2^28 82.2 -> 84.6 (profiles/r06/mergek/it26_ab.txt);
// 768 or 640 lanes at two workgroups per CU were slower (nt_ab.txt).  Load rows
// of 128 keys (the descriptor holds 8 bytes per row; 64 -> 128 halved it:
// 2^30 pass 2569 -> 2547 us, profiles/r05/plan/rw_ab.txt).
template <>
struct KTr<uint32_t> {
    typedef uint64_t F;
    static constexpr int NT = 512, IT = 18, CAP = 8960, WG_PER_CU = 4;
    static constexpr int IT16 = 26, CAP16 = 12864, WG16 = 3;
    // the chunk shape of a pass of lk levels
    static constexpr bool big(int lk) { return lk == 4; }
    static constexpr int it(int lk) { return big(lk) ? IT16 : IT; }
    // (k_fence_counts keeps 8-bit per-chunk counts: at most 255 + K fences of FG
    // keys a chunk, a bound only the 64-key build can reach)
    static constexpr int cap16() { return CAP16 < (255 + 16) * FG ? CAP16 : (255 + 16) * (int)FG; }
    static constexpr int cap(int lk) { return big(lk) ? cap16() : CAP; }
    static constexpr int wg(int lk) { return big(lk) ? WG16 : WG_PER_CU; }
    static constexpr int FL_LDS = 13;                // 8192 fences = 64 KiB
    // runs >= the smaller SORT tile (SORT_LT_MERGE, kernels.h); 32-bit row offsets
    static constexpr int LW_MIN = 14, LWK_MAX = 30;
};
// The u64 chunk shape: 18 outputs per lane and the largest capacity whose
// level layout fits 512 x 18 slots (CAP + 8 (G + QA) <= 9216): 8832 keys
// (69 fences of 128) instead of 8192 measured 2^29 u64 35.4 -> 36.5-36.7
// Gkeys/s, k_mergek 2.46 -> 2.33 ms per pass, 2^26 +2.2 %; 9216 keys at 20 per
// lane was slower (profiles/r04/chunk64).  The 64-key build (runsk_fg6.hip)
// takes 8896 (139 fences of 64): k_mergek -5 us per 2^29 pass
// (profiles/r05/mergek/cap_ab.txt).
template <>
struct KTr<uint64_t> {
    typedef u128 F;
    static constexpr int NT = 512, IT = 18, WG_PER_CU = 2;
    static constexpr int CAP = FG_LOG2 == 6 ? 8896 : 8832;  // ~69 KiB of keys: two tiles per CU, 4 waves per SIMD
    static constexpr int FL_LDS = 12;    // 4096 fences = 64 KiB
    static constexpr int LW_MIN = 13, LWK_MAX = 29;  // runs >= the u64 SORT tile; 32-bit row offsets
    static constexpr int it(int) { return IT; }
    static constexpr int cap(int) { return CAP; }
    static constexpr int wg(int) { return WG_PER_CU; }
};

// Every sequence an in-LDS merge reads is followed by G words of MAX
// (sentinels), so a merge chain needs no end checks: it reads at most IT words
// past an exhausted sequence.  Each level places its pairs' outputs at lane
// boundaries past the previous pair's sentinels (no lane straddles two pairs).
constexpr int PAD = 4;  // keys below the tile: a co-rank probe may read index -1

constexpr int SCAN_NT_MAX = 256;      // chunks per fence-count block (SCAN_NT below)
constexpr int SCAN_NT = SCAN_NT_MAX;  // chunks per block of the fence-count scan
// block totals a fused descriptor kernel scans in LDS itself (k_chunk_desc, PLAN)
constexpr int PLAN_SCAN_MAX = 2048;

template <typename KEY, int LK>
struct Shape {
    typedef KTr<KEY> T;
    // the merge chain of the in-LDS levels: two keys per read (u32), one (u64)
    static constexpr int CH = sizeof(KEY) == 4 ? 1 : 0;
    static constexpr int NT = T::NT, IT = T::it(LK), CAP = T::cap(LK);
    static constexpr int MAXR = CAP / 2;  // co-rank range bound: min(LA, LB) <= CAP / 2
    // zero words below the A sequences (co_rank without its i == lo test; the
    // two-key chain): the last of the G words after a sequence holds the next
    // one's, so G exceeds the keys a chain reads past a sequence (IT for the
    // two-key chain, IT + 1 for the one-key chain)
    static constexpr bool ZW = CH == 1;
    static constexpr int G = IT + 1;
    static constexpr int QA = IT;  // level outputs start at lane boundaries
    static_assert(IT % 2 == 0, "outputs stored as aligned pairs");
    // LDS slot of segment q (o = its first chunk position)
    MERGEK_HD static int seg(int o, int q) { return o + q * G; }
    static constexpr int K = 1 << LK, LKS = LK;
    static constexpr int FM = CAP / (int)FG - K;   // fences per chunk, worst case (plan_pass cuts at more)
    static constexpr int RW = LK == 4 ? 128 : (LK == 3 || NT % 256) ? 128 : 256;  // load row: RW keys of one segment
    static constexpr int NR = NT / RW;             // row parts: waves [p*RW/64, (p+1)*RW/64) load part p
    // load slots per lane: enough rows for CAP keys in K segments
    static constexpr int LS_ROWS = ((CAP + RW - 1) / RW + K + NR - 1) / NR;
    static constexpr int LS = ((IT + 1) & ~1) <= LS_ROWS ? LS_ROWS : ((IT + 1) & ~1);
    static constexpr int NROWS = LS * NR;           // lane slot j of part p holds row j * NR + p
    // the tile holds the chunk's segments with their sentinels (CAP + K G) and
    // every level's outputs (<= NT IT slots by the level layout, + G sentinels)
    static constexpr int NB_EXT = CAP + K * G > NT * IT + G ? CAP + K * G : NT * IT + G;
    static constexpr int LDS_KEYS = PAD + NB_EXT + 16;
    static_assert(FM > 0 && FM < 256 && SCAN_NT_MAX * FM < 65536,
                  "fence stride vs chunk (k_fence_counts keeps 8-bit counts and 16-bit block prefixes)");
    static_assert(CAP <= (NROWS - K) * RW, "segment rows: ceil(l_r / RW) summed over K segments");
    static_assert(CAP + (K / 2) * (G + QA) <= NT * IT, "level layout: pairs at lane boundaries");
    static_assert(LDS_KEYS < 65536, "LDS key index of a row fits 16 bits");
};

// A chunk's descriptor (k_chunk_desc writes it, k_mergek reads it; see there).
template <typename KEY, int LK>
struct alignas(128) Desc {  // whole 128-byte lines: a chunk's entries never share a line with another's
    int64_t gbase, out0;
    int o[Shape<KEY, LK>::K + 1];           // chunk position of segment r; o[K] = chunk length
    uint32_t off[Shape<KEY, LK>::NROWS];  // byte offset of the row's first key from the group base
    uint32_t la[Shape<KEY, LK>::NROWS];   // real keys of the row (0..RW) | LDS slot of its first key << 16
};

// Group geometry of the pass: groups of K runs of W keys; run r of group g
// starts at g*KW + r*W and holds clamp(n - start, 0, W) keys.
struct Geo {
    int64_t n;
    int lw, lk, fm;
    int64_t nfull;  // full groups
    int64_t kf;     // chunks per full group
    MERGEK_HD int K() const { return 1 << lk; }
    MERGEK_HD int64_t W() const { return (int64_t)1 << lw; }
    MERGEK_HD int64_t base(int64_t g) const { return g << (lw + lk); }
    MERGEK_HD int64_t run_len(int64_t g, int r) const {
        const int64_t rest = n - (base(g) + r * W());
        return rest <= 0 ? 0 : (rest < W() ? rest : W());
    }
    MERGEK_HD int64_t nfences(int64_t g) const {
        const int64_t glen = (n - base(g)) < K() * W() ? n - base(g) : K() * W();
        return (glen + FG - 1) >> FG_LOG2;
    }
    // a group's fences and chunks are < 2^31: a 32-bit division
    MERGEK_HD int64_t nchunks(int64_t g) const {
        return g < nfull ? kf : (int64_t)((uint32_t)(nfences(g) + fm - 1) / (uint32_t)fm);
    }
    // bounds slot of chunk t of group g (each group has nchunks + 1 slots)
    MERGEK_HD int64_t slot(int64_t g, int64_t t) const {
        return g < nfull ? g * (kf + 1) + t : nfull * (kf + 1) + t;
    }
};

// fm = 0: the worst-case bound, (fm + K) * FG <= CAP
template <typename KEY>
Geo make_geo(int64_t n, int lw, int lk, int fm = 0) {
    Geo geo{n, lw, lk, fm > 0 ? fm : KTr<KEY>::cap(lk) / (int)FG - (1 << lk), 0, 0};
    geo.nfull = n >> (lw + lk);
    geo.kf = ((((int64_t)1 << (lw + lk)) >> FG_LOG2) + geo.fm - 1) / geo.fm;
    return geo;
}

inline int64_t chunks_of(const Geo& geo) {
    const bool tail = (geo.nfull << (geo.lw + geo.lk)) < geo.n;
    return geo.nfull * geo.kf + (tail ? geo.nchunks(geo.nfull) : 0);
}

// The passes' environment knobs, read once per process (per build).
inline int env_int(const char* k, int dflt) {
    const char* e = getenv(k);
    return e ? atoi(e) : dflt;
}
struct MergekKnobs {
    // MISORT_PLAN_FUSE: 1 (default) = bounds inside k_chunk_desc below 4096
    // chunks, 2 = at every size, 0 = never (profiles/r03/ab_plan: 2^24 u32 43.1
    // -> 43.9 Gkeys/s; at 2^26, 9362 chunks, 65.2 -> 65.0)
    int plan_fuse = env_int("MISORT_PLAN_FUSE", 1);
    // MISORT_PLAN_SCAN: 1 (default) = a fused descriptor kernel scans the
    // fence-count block totals itself when they fit PLAN_SCAN_MAX, 0 = never
    int plan_scan = env_int("MISORT_PLAN_SCAN", 1);
    // MISORT_FENCE_RANK_MAX: fused passes whose runs hold <= 2^this fences rank
    // them and count them in one launch (k_fence_rank); 0 = never
    int rank_max = env_int("MISORT_FENCE_RANK_MAX", 14);
    // MISORT_FENCE_NEST_MIN: log2 fences from which a pass nests (FENCE_NEST_LEVELS); 0 = never
    int nest_min = env_int("MISORT_FENCE_NEST_MIN", 21);
    // MISORT_FC_SLICES_MAX (tests): the block count from which the coalesced form counts
    int64_t slices_max = getenv("MISORT_FC_SLICES_MAX") ? atoll(getenv("MISORT_FC_SLICES_MAX")) : 256;
    // MISORT_MK_FM_ADD: the capacity split's added fences (split_fm_add); -1 (default) = per key type and K
    int fm_add = env_int("MISORT_MK_FM_ADD", -1);
    // MISORT_MK_PROBE: k_mergek's probe launches after every pass (launch_mergek)
    bool probe = env_int("MISORT_MK_PROBE", 0) != 0;
};
inline const MergekKnobs& mergek_knobs() {
    static const MergekKnobs k;
    return k;
}

// The capacity split's fences per chunk above the worst-case bound (plan_pass).
// A chunk's size is FM * FG plus 2K window offsets of up to FG each, which
// nearly cancel on spread keys (sigma ~ FG sqrt(2K / 12), 1.6 FG at K = 16):
// 9 fences more at K = 16 (4.6 sigma of headroom with 128-key fences) and 3 at
// K = 8 (4.3 sigma) keep splits to about one per few 2^30 passes on spread
// keys -- a split's serial latency (k_split_desc) and its halves' merge sit on
// the pass's critical path, so rarer splits beat fuller chunks here: 12 fences
// more (2.8 sigma, ~0.3 % of chunks) measured slower than none at 2^28
// (profiles/r06/mergek/split_ab.txt).  (env MISORT_MK_FM_ADD: one value
// for every unfused pass, 0 = off), clamped so a half chunk still fits --
// ceil(fm / 2) + K fences of FG keys <= CAP -- and fm <= 255 (k_fence_counts'
// 8-bit counts).
template <typename KEY, int LK>
int split_fm_add(const MergekKnobs& kn) {
    // u64: equal kernel time, +25 us of split overhead per 2^29 pass (split_ab.txt): off
    const int want = kn.fm_add >= 0 ? kn.fm_add : sizeof(KEY) == 8 ? 0 : LK == 4 ? 9 : LK == 3 ? 3 : 0;
    const int K = 1 << LK, cap = KTr<KEY>::cap(LK), fm0 = cap / (int)FG - K;
    int fm = fm0 + (want > 0 ? want : 0);
    while (fm > fm0 && ((fm + 1) / 2 + K) * (int)FG > cap) --fm;
    if (fm > 255) fm = 255;
    return fm > fm0 ? fm - fm0 : 0;
}

// A group whose fence count lies just above a multiple of fm ends in a nearly
// empty chunk (2^30 u32 pass 1: 2048 fences a group, fm 93 -> 23 chunks, the
// last of 2 fences): up to FM_BALANCE fences more per chunk when that saves
// the group a chunk, within the split's bound (halves fit, 8-bit counts), and
// only where that chunk is >= 1/BAL_NC_MAX of the group's: 2^30 +0.35 %; on
// every pass (+1 fence a chunk, more splits for 1 chunk in 250) 2^27 -1 %
// (profiles/r06/mergek/balance_ab.txt).
constexpr int FM_BALANCE = 3, BAL_NC_MAX = 32;
template <typename KEY, int LK>
int balance_fm(int fm, int64_t gf) {
    const int K = 1 << LK, cap = KTr<KEY>::cap(LK);
    const int64_t nc = gf / fm;
    if (nc < 1 || nc > BAL_NC_MAX || nc * fm == gf) return fm;
    const int fm2 = (int)((gf + nc - 1) / nc);
    return fm2 <= fm + FM_BALANCE && fm2 <= 255 && ((fm2 + 1) / 2 + K) * (int)FG <= cap ? fm2 : fm;
}

// The fence merge levels of a u32 pass as one multi-way merge pass over the
// fences themselves (u64 keys, depth 1) once at least FENCE_NEST_LEVELS of
// them would run as global 2-way merge levels and the pass has at least
// 2^MISORT_FENCE_NEST_MIN fences (env; 0 = never): one HBM sweep of the fence
// array instead of one per level.  Measured (profiles/r05/plan/nest_ab.txt):
// 2^30 u32 passes 3 and 4 (2^23 fences) -30 us each, +0.6 %; at 2^22 fences
// (2^29 keys) the nested pass's ~600 chunks underfilled the chip: +5 us, so the
// threshold was 2^23.  Round 6: with the nested pass's own planning in one
// k_fence_rank launch, 2^21 measured 2^28 +0.5 %, 2^29 +0.6 %, 2^30 equal
// (profiles/r06/plan/nest_ab.txt).
constexpr int FENCE_NEST_LEVELS = 3;
// passes of fewer chunks fuse their planning (MISORT_PLAN_FUSE = 1)
constexpr int64_t FUSE_MAX_CHUNKS = 4096;
// planning kernel shapes by size (measured crossovers, profiles/r02/s3b-s3i):
// k_bounds' line probe from 2^17 searches, 16 descriptors per workgroup from 2^14 chunks
constexpr int64_t LINE_MIN = 1 << 17, DC16_MIN = 1 << 14;

inline size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }
// One fence buffer of a pass over n keys (MergekBuild::fence_buffer sizes the SORT
// pass's with it, so the buffer never moves between the two).
inline size_t fence_buffer_bytes(int64_t n, size_t fence_size) {
    return round256((size_t)((n + FG - 1) >> FG_LOG2) * fence_size);
}

// Everything merge_pass decides before it launches.
struct PassPlan {
    Geo geo;     // with the final fm (after the capacity split's add and the balance)
    bool fuse;   // bounds (and, nbs > 0, the block-total scan) inside k_chunk_desc
    bool split;  // capacity split: fm above the worst-case bound, over-full chunks cut in two
    bool rank;   // k_fence_rank orders and counts the fences in one launch
    bool nest;   // the global fence merge levels as one nested pass of nest_lk levels (depth 1)
    bool tail, line, slices;  // a short last group; k_bounds' line probe; k_fence_counts<SLICES>
    // fence order: a levels in LDS (k_fence_merge if fmerge, else k_fence_lds with
    // each of the nb0 sub-groups over fsplit blocks), then `left` global levels
    bool fmerge;
    int wf_log2, a, left, nest_lk, fsplit;
    int cpb, nbs, dc;  // chunks per fence-count block; blocks k_chunk_desc scans (0: k_scan_totals); descriptors per workgroup
    int64_t nchunks, nslots, nf, nbk, nb0;
    // Workspace.  Fence set (scratch set 2 * depth): the two fence buffers of fb
    // bytes, kept across the passes of a sort.  Planning set (2 * depth + 1), per
    // pass, its parts in this order (bytes[], off[]): merged fences and merge temp
    // (fb each), bounds, fence counts, their block totals, descriptors (one per
    // chunk, and with the split two per listed chunk -- at most every chunk), the
    // split's list [count, chunks...].
    enum Part { P_M, P_T, P_BOUNDS, P_CNT, P_BSUM, P_DESC, P_OVF, NPARTS };
    size_t fb, bytes[NPARTS], off[NPARTS];
    size_t fence_bytes, plan_bytes;
    int fence_set, plan_set;
};

// false: more than 2^31 chunks or bounds slots (the kernels divide them in 32 bits).
template <typename KEY, int LK>
bool plan_pass(int64_t n, int lw, int depth, const MergekKnobs& kn, PassPlan& p) {
    typedef Shape<KEY, LK> S;
    p = PassPlan{};
    Geo geo = make_geo<KEY>(n, lw, LK);
    p.fuse = kn.plan_fuse == 2 || (kn.plan_fuse == 1 && chunks_of(geo) < FUSE_MAX_CHUNKS);
    // Capacity split (unfused passes): chunks cut every fm merged fences, fm
    // above the worst-case bound by split_fm_add -- sized for a typical chunk,
    // whose K window offsets nearly cancel -- and the rare chunk that exceeds
    // CAP cut in two at its middle fence (k_chunk_desc lists it, k_split_desc cuts
    // it, k_mergek's extra workgroups run the halves).  A half holds at most
    // ceil(fm / 2) + K fences' worth of keys, so fm stays within 2 (CAP / FG - K)
    // (and 8-bit counts).
    const int fma = p.fuse ? 0 : split_fm_add<KEY, LK>(kn);
    if (fma > 0) geo = make_geo<KEY>(n, lw, LK, balance_fm<KEY, LK>(geo.fm + fma, ((int64_t)1 << (lw + LK)) >> FG_LOG2));
    p.geo = geo;
    p.split = fma > 0;
    p.tail = (geo.nfull << (lw + LK)) < n;
    p.nchunks = chunks_of(geo);
    p.nslots = geo.nfull * (geo.kf + 1) + (p.tail ? geo.nchunks(geo.nfull) + 1 : 0);
    p.nf = (n + FG - 1) >> FG_LOG2;
    if (p.nchunks >= ((int64_t)1 << 31) || p.nslots >= ((int64_t)1 << 31)) return false;
    // chunks per fence-count block: SCAN_NT, or fewer (down to 32) while that
    // leaves under 128 blocks -- a small sort's few blocks walked long slices
    p.cpb = SCAN_NT;
    while (p.cpb > 32 && (p.nchunks + p.cpb - 1) / p.cpb < 128) p.cpb /= 2;
    p.nbk = (p.nchunks + p.cpb - 1) / p.cpb;
    p.wf_log2 = lw - FG_LOG2;  // fences per run = 2^wf_log2
    p.rank = p.fuse && p.wf_log2 <= kn.rank_max;
    if (!p.rank) {
        // the group's fences into total order: the first a levels in LDS
        // (sub-groups of 2^a runs, <= 64 KiB of fences), the other LK - a as
        // fence merge levels (runs of >= 2^FL fences) or one nested pass
        constexpr int FL = KTr<KEY>::FL_LDS;
        p.a = p.wf_log2 >= FL ? 0 : (FL - p.wf_log2 < LK ? FL - p.wf_log2 : LK);
        p.left = LK - p.a;
        const int sg = p.wf_log2 + p.a;  // log2 fences of a sub-group
        p.nest = sizeof(KEY) == 4 && depth == 0 && kn.nest_min > 0 && p.left >= FENCE_NEST_LEVELS &&
                 p.nf >= ((int64_t)1 << kn.nest_min) && sg >= KTr<uint64_t>::LW_MIN &&
                 sg + p.left <= KTr<uint64_t>::LWK_MAX;
        p.nest_lk = p.nest ? p.left : 0;
        p.nb0 = (p.nf + ((int64_t)1 << sg) - 1) >> sg;
        p.fmerge = p.nb0 >= FENCE_MERGE_MIN_BLOCKS;
        // k_fence_lds: >= 512 blocks where the sub-groups are few (each loads its whole sub-group)
        p.fsplit = 1;
        while (p.fsplit < 8 && p.nb0 * p.fsplit < 512 && ((int64_t)1 << sg) / (p.fsplit * 2) >= 1024) p.fsplit *= 2;
    }
    // few blocks: per-lane slices; many: coalesced atomics (k_fence_counts)
    p.slices = p.nbk < kn.slices_max;
    p.line = (p.nslots << LK) >= LINE_MIN;
    p.nbs = !p.rank && p.fuse && kn.plan_scan && p.nbk * S::K <= PLAN_SCAN_MAX ? (int)p.nbk : 0;
    p.dc = p.nchunks >= DC16_MIN ? 16 : 4;
    p.fb = fence_buffer_bytes(n, sizeof(typename KTr<KEY>::F));
    p.bytes[PassPlan::P_M] = p.bytes[PassPlan::P_T] = p.fb;
    p.bytes[PassPlan::P_BOUNDS] = round256((size_t)p.nslots * S::K * 8);
    p.bytes[PassPlan::P_CNT] = round256((size_t)p.nbk * p.cpb * S::K * 4);
    p.bytes[PassPlan::P_BSUM] = round256((size_t)p.nbk * S::K * 4);
    p.bytes[PassPlan::P_DESC] = round256((size_t)p.nchunks * sizeof(Desc<KEY, LK>) * (p.split ? 3 : 1));
    p.bytes[PassPlan::P_OVF] = p.split ? round256((size_t)(p.nchunks + 1) * 4) : 0;
    size_t end = 0;
    for (int i = 0; i < PassPlan::NPARTS; end += p.bytes[i++]) p.off[i] = end;
    p.fence_bytes = 2 * p.fb;
    p.plan_bytes = end + 256;
    p.fence_set = 2 * depth;
    p.plan_set = 2 * depth + 1;
    return true;
}

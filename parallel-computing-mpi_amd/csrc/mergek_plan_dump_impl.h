// mergek_plan_dump_impl.h -- mergek_plan_dump.cpp's printing for one fence
// stride: included inside a namespace with MISORT_RUNSK_FGL defined, like
// mergek_plan.h itself (no include guard).
#include "mergek_plan.h"

template <typename KEY, int LK>
int dump_shape() {
    typedef Shape<KEY, LK> S;
    printf("{\"FG_LOG2\": %d, \"K\": %d, \"FM\": %d, \"RW\": %d, \"NR\": %d, \"LS\": %d, \"NROWS\": %d, \"G\": %d, "
           "\"NB_EXT\": %d, \"LDS_KEYS\": %d, \"CAP\": %d, \"IT\": %d, \"NT\": %d, \"LW_MIN\": %d, \"LWK_MAX\": %d, "
           "\"fence_bytes\": %zu, \"desc_bytes\": %zu}\n",
           FG_LOG2, S::K, S::FM, S::RW, S::NR, S::LS, S::NROWS, S::G, S::NB_EXT, S::LDS_KEYS, S::CAP, S::IT, S::NT,
           KTr<KEY>::LW_MIN, KTr<KEY>::LWK_MAX, sizeof(typename KTr<KEY>::F), sizeof(Desc<KEY, LK>));
    return 0;
}

template <typename KEY, int LK>
int dump_plan(int64_t n, int lw, int depth) {
    if (n <= 0 || lw < KTr<KEY>::LW_MIN || lw + LK > KTr<KEY>::LWK_MAX || depth < 0 || depth > 1) return 2;
    PassPlan p;
    if (!plan_pass<KEY, LK>(n, lw, depth, mergek_knobs(), p)) {
        printf("{\"ok\": false}\n");
        return 0;
    }
    const Geo& g = p.geo;
    printf("{\"ok\": true, \"n\": %lld, \"lw\": %d, \"lk\": %d, \"fm\": %d, \"fm_worst\": %d, \"nfull\": %lld, \"kf\": %lld, ",
           (long long)g.n, g.lw, g.lk, g.fm, Shape<KEY, LK>::FM, (long long)g.nfull, (long long)g.kf);
    printf("\"fuse\": %d, \"split\": %d, \"rank\": %d, \"nest\": %d, \"tail\": %d, \"line\": %d, \"slices\": %d, "
           "\"fmerge\": %d, \"wf_log2\": %d, \"a\": %d, \"left\": %d, \"nest_lk\": %d, \"fsplit\": %d, \"cpb\": %d, "
           "\"nbs\": %d, \"dc\": %d, ",
           p.fuse, p.split, p.rank, p.nest, p.tail, p.line, p.slices, p.fmerge, p.wf_log2, p.a, p.left, p.nest_lk,
           p.fsplit, p.cpb, p.nbs, p.dc);
    printf("\"nchunks\": %lld, \"nslots\": %lld, \"nf\": %lld, \"nbk\": %lld, \"nb0\": %lld, ", (long long)p.nchunks,
           (long long)p.nslots, (long long)p.nf, (long long)p.nbk, (long long)p.nb0);
    // the planning set's parts in layout order, then the two sets
    static const char* const part[PassPlan::NPARTS] = {"M", "T", "bounds", "cnt", "bsum", "desc", "ovf"};
    printf("\"parts\": [");
    for (int i = 0; i < PassPlan::NPARTS; ++i)
        printf("%s{\"name\": \"%s\", \"off\": %zu, \"bytes\": %zu}", i ? ", " : "", part[i], p.off[i], p.bytes[i]);
    printf("], \"fb\": %zu, \"fence_bytes\": %zu, \"plan_bytes\": %zu, \"fence_set\": %d, \"plan_set\": %d, "
           "\"fence_buffer_fb\": %zu}\n",
           p.fb, p.fence_bytes, p.plan_bytes, p.fence_set, p.plan_set,
           fence_buffer_bytes(n, sizeof(KEY) == 8 ? sizeof(u128) : sizeof(uint64_t)));  // as MergekBuild::fence_buffer
    return 0;
}

template <typename KEY>
int dump_key(int lk, bool shape, int64_t n, int lw, int depth) {
    switch (lk) {
        case 1: return shape ? dump_shape<KEY, 1>() : dump_plan<KEY, 1>(n, lw, depth);
        case 2: return shape ? dump_shape<KEY, 2>() : dump_plan<KEY, 2>(n, lw, depth);
        case 3: return shape ? dump_shape<KEY, 3>() : dump_plan<KEY, 3>(n, lw, depth);
        case 4: return shape ? dump_shape<KEY, 4>() : dump_plan<KEY, 4>(n, lw, depth);
    }
    return 2;
}

inline int dump(int argc, char** argv) {
    const bool shape = argc == 4;
    const int kb = atoi(argv[shape ? 1 : 4]), lk = atoi(argv[shape ? 2 : 3]);
    const int lw = shape ? 0 : atoi(argv[2]), depth = argc == 7 ? atoi(argv[6]) : 0;
    for (const char* a = shape ? "" : argv[1]; a; a = strchr(a, ',') ? strchr(a, ',') + 1 : nullptr) {
        const int64_t n = atoll(a);
        const int rc = kb == 4   ? dump_key<uint32_t>(lk, shape, n, lw, depth)
                       : kb == 8 ? dump_key<uint64_t>(lk, shape, n, lw, depth)
                                 : 2;
        if (rc) return rc;
    }
    return 0;
}

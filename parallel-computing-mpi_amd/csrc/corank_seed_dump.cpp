// corank_seed_dump.cpp -- the host model of the in-LDS co-rank search: runs
// corank_seed.h (the kernels' own search arithmetic, host compiler only) over
// every diagonal of the pairs it is given and prints one JSON line
// (tests/test_corank_seed_model.py):
//   corank_seed_dump key_bytes it la lb npairs file [maxr maxt]
// file: npairs pairs, each la sorted keys (A) then lb sorted keys (B), raw
// little-endian words of key_bytes.  Lane l searches diagonal min(l * it, la +
// lb), as a lane of `it` outputs does; 64 consecutive lanes are a wave, which
// votes on the fallback.  maxr, maxt: the level's uniform bounds (default: this
// pair's min(la, lb) and la + lb).  The keys lie as they do in LDS: a zero
// word below A (4-byte keys), sentinels after A and after B.
// Output: the level's window and step bounds; per pair the split of every
// lane, the probes every lane made and one fallback flag per wave; bad_probes:
// probes outside [A0 - 1, A0 + la) x [B0, B0 + lb] -- always 0.  Exit status 2 on bad arguments.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "corank_seed.h"

namespace {
using namespace misort;

constexpr int MAXR = 1 << 16;  // pairs of up to 2^17 keys

template <typename KEY>
int run(int it, int la, int lb, int npairs, FILE* f, int maxr, int maxt) {
    constexpr int KB = (int)sizeof(KEY);
    constexpr int PH = corank::phase_full(KB), PHS = corank::phase_seed(KB);
    constexpr int STEP0 = corank::floor_pow2(MAXR + PH), SEED0 = corank::seed_step0(2 * MAXR, PHS);
    const int tot = la + lb, G = it + 1, A0 = 1, B0 = A0 + la + G;
    const corank::Level L = corank::level(maxr, maxt, KB);
    std::vector<KEY> s((size_t)B0 + lb + G);
    const int lanes = (tot + it - 1) / it + 1;
    printf("{\"key_bytes\": %d, \"it\": %d, \"la\": %d, \"lb\": %d, \"w\": %d, \"top_seed\": %d, \"top_full\": %d, "
           "\"reach\": %d, \"seeded\": %s, \"lanes\": %d, \"pairs\": [",
           KB, it, la, lb, L.w, L.top_seed, L.top_full, L.reach, L.seeded ? "true" : "false", lanes);
    long bad = 0;
    std::vector<int> split(lanes), steps(lanes), fb;
    for (int p = 0; p < npairs; ++p) {
        for (auto& k : s) k = (KEY) ~(KEY)0;
        s[0] = 0;
        if (fread(s.data() + A0, KB, la, f) != (size_t)la || fread(s.data() + B0, KB, lb, f) != (size_t)lb) return 2;
        fb.clear();
        for (int w0 = 0; w0 < lanes; w0 += 64) {
            const int w1 = w0 + 64 < lanes ? w0 + 64 : lanes;
            bool any = false;
            for (int pass = 0; pass < 2; ++pass) {  // 0: seeded, 1: the wave's full search
                if (pass == 0 && !L.seeded) {
                    any = true;  // the level runs the full search alone (no fallback reported)
                    continue;
                }
                if (pass == 1 && !any) break;
                for (int l = w0; l < w1; ++l) {
                    const int d = l * it < tot ? l * it : tot;
                    const int lo = d - lb > 0 ? d - lb : 0, hi = d < la ? d : la;
                    int n = 0;
                    auto ok = [&](int i) {
                        ++n;
                        const int ai = A0 - 1 + i, bi = B0 + d - i;
                        if (ai < A0 - 1 || ai >= A0 + la || bi < B0 || bi > B0 + lb) ++bad;
                        return s[ai] <= s[bi];
                    };
                    int x;
                    if (pass == 0) {
                        bool failed;
                        x = corank::seeded<SEED0, 0, false>(0, la, lb, d, lo, hi, PHS ? l & PHS : 0, L, failed, ok);
                        any |= failed;
                        steps[l] = 0;
                    } else {
                        x = corank::full<STEP0, 0>(0, lo, hi, PH ? l & 31 : 0, L, ok);
                    }
                    split[l] = corank::split_of<0>(x, 0, lo);
                    steps[l] += n;
                }
            }
            fb.push_back(L.seeded && any);
        }
        printf("%s{\"splits\": [", p ? ", " : "");
        for (int l = 0; l < lanes; ++l) printf("%s%d", l ? "," : "", split[l]);
        printf("], \"steps\": [");
        for (int l = 0; l < lanes; ++l) printf("%s%d", l ? "," : "", steps[l]);
        printf("], \"fallback\": [");
        for (size_t g = 0; g < fb.size(); ++g) printf("%s%d", g ? "," : "", (int)fb[g]);
        printf("]}");
    }
    printf("], \"bad_probes\": %ld}\n", bad);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 7 && argc != 9) {
        fprintf(stderr, "usage: %s key_bytes it la lb npairs file [maxr maxt]\n", argv[0]);
        return 2;
    }
    const int kb = atoi(argv[1]), it = atoi(argv[2]), la = atoi(argv[3]), lb = atoi(argv[4]), np = atoi(argv[5]);
    const int maxr = argc == 9 ? atoi(argv[7]) : (la < lb ? la : lb), maxt = argc == 9 ? atoi(argv[8]) : la + lb;
    if ((kb != 4 && kb != 8) || it < 1 || la < 0 || lb < 0 || np < 0 || la > MAXR || lb > MAXR ||
        maxr < (la < lb ? la : lb) || maxt < la + lb || maxr > MAXR || maxt > 2 * MAXR)
        return 2;
    FILE* f = fopen(argv[6], "rb");
    if (!f) return 2;
    const int rc = kb == 4 ? run<uint32_t>(it, la, lb, np, f, maxr, maxt) : run<uint64_t>(it, la, lb, np, f, maxr, maxt);
    fclose(f);
    return rc;
}

// net_r4_dump.cpp -- the host model of the SORT tiles' in-register stages on
// 4-byte keys: runs net_r4.h (the kernels' own schedule, host compiler only)
// over every register image it is given (tests/test_net_r4_model.py):
//   net_r4_dump top cnt flip file [out]
// file: images of 32 keys each, raw little-endian u32, register 0 first.
// For every image the stage list (top, cnt, flip) runs twice: fused into
// radix-4 steps (stages_r4) and one stage at a time (stages_r2).
// Output: per image two lines of 32 hexadecimal keys, "r4 ..." and "r2 ...";
// with `out`, the same as raw u32 instead (per image 32 fused keys, then the 32
// reference keys) and one summary line on stdout.  Exit status 2 on bad
// arguments or a file that is no whole number of images.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "net_r4.h"

namespace {
using namespace misort;

typedef void (*stages_fn)(uint32_t (&)[32]);
struct Shape {
    stages_fn r4, r2;
};

template <int TOP, int CNT, bool FLIP>
constexpr Shape shape() {
    return Shape{&net_r4::stages_r4<TOP, CNT, FLIP>, &net_r4::stages_r2<TOP, CNT, FLIP>};
}
template <int TOP, int CNT>
Shape pick_flip(bool flip) {
    return flip ? shape<TOP, CNT, true>() : shape<TOP, CNT, false>();
}
template <int TOP>
Shape pick_cnt(int cnt, bool flip) {
    switch (cnt) {
    case 1: return pick_flip<TOP, 1>(flip);
    case 2: if constexpr (TOP >= 1) return pick_flip<TOP, 2>(flip); break;
    case 3: if constexpr (TOP >= 2) return pick_flip<TOP, 3>(flip); break;
    case 4: if constexpr (TOP >= 3) return pick_flip<TOP, 4>(flip); break;
    case 5: if constexpr (TOP >= 4) return pick_flip<TOP, 5>(flip); break;
    }
    return Shape{nullptr, nullptr};
}
Shape pick(int top, int cnt, bool flip) {
    switch (top) {
    case 0: return pick_cnt<0>(cnt, flip);
    case 1: return pick_cnt<1>(cnt, flip);
    case 2: return pick_cnt<2>(cnt, flip);
    case 3: return pick_cnt<3>(cnt, flip);
    case 4: return pick_cnt<4>(cnt, flip);
    }
    return Shape{nullptr, nullptr};
}

void print_line(const char* tag, const uint32_t (&v)[32]) {
    fputs(tag, stdout);
    for (int c = 0; c < 32; ++c) printf(" %08x", v[c]);
    fputc('\n', stdout);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 5 && argc != 6) {
        fprintf(stderr, "usage: %s top cnt flip file [out]\n", argv[0]);
        return 2;
    }
    const int top = atoi(argv[1]), cnt = atoi(argv[2]), flip = atoi(argv[3]);
    if (top < 0 || top > 4 || cnt < 1 || cnt > top + 1 || (flip != 0 && flip != 1)) return 2;
    const Shape sh = pick(top, cnt, flip != 0);
    if (!sh.r4) return 2;
    FILE* f = fopen(argv[4], "rb");
    if (!f) return 2;
    FILE* o = argc == 6 ? fopen(argv[5], "wb") : nullptr;
    if (argc == 6 && !o) {
        fclose(f);
        return 2;
    }
    long images = 0, differ = 0;
    int rc = 0;
    uint32_t in[32], a[32], b[32];
    for (;;) {
        const size_t got = fread(in, sizeof(uint32_t), 32, f);
        if (got == 0) break;
        if (got != 32) {
            rc = 2;
            break;
        }
        memcpy(a, in, sizeof a);
        memcpy(b, in, sizeof b);
        sh.r4(a);
        sh.r2(b);
        ++images;
        differ += memcmp(a, b, sizeof a) != 0;
        if (o) {
            if (fwrite(a, sizeof(uint32_t), 32, o) != 32 || fwrite(b, sizeof(uint32_t), 32, o) != 32) {
                rc = 2;
                break;
            }
        } else {
            print_line("r4", a);
            print_line("r2", b);
        }
    }
    fclose(f);
    if (o) {
        if (fclose(o) != 0) rc = 2;
        printf("{\"top\": %d, \"cnt\": %d, \"flip\": %d, \"images\": %ld, \"differ\": %ld}\n", top, cnt, flip, images,
               differ);
    }
    return rc;
}

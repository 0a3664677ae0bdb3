// net_r4.h -- the in-register stages of the bitonic network on 32 four-byte
// keys, two stages at a time: plain C++17 for host and device, so
// net_r4_dump.cpp (host compiler alone) runs the very schedule the kernels run
// (tests/test_net_r4_model.py).
//
// Two consecutive stages at strides 2s and s act on the 4-tuples (a, b, c, d)
// = registers (i, i + s, i + 2s, i + 3s):
//   stage 2s:  a' = min(a, c), c' = max(a, c), b' = min(b, d), d' = max(b, d)
//   stage s:   o0 = min(a', b'), o1 = max(a', b'), o2 = min(c', d'), o3 = max(c', d')
// 8 two-input min/max per 4 keys.  With three-input ops (v_min3_u32,
// v_med3_u32, v_max3_u32: full rate on gfx950) the same outputs take 6:
//   bl = min(b, d), bh = max(b, d)
//   o0 = min3(a, c, bl), o1 = med3(a, c, bl), o2 = med3(a, c, bh), o3 = max3(a, c, bh)
// o0 and o3 hold for any input.  o1 = max(min(a, c), bl) needs bl <= max(a, c),
// o2 = min(max(a, c), bh) needs bh >= min(a, c).  A 0-1 image violates one of
// them only as 0101 or 1010, so they hold whenever (a, b, c, d) is
// cyclic-bitonic -- and every 4-tuple a pair of half-cleaner stages sees is a
// strided subsequence of a bitonic block.  min, max and med3 commute with
// monotone maps, so agreement on the 0-1 images of the valid inputs is
// agreement on all of them (the tests enumerate those images).
//
// The flip stage of a level (i <-> i ^ m, m = 2^(TOP+1) - 1) and the stage
// after it obey the same algebra with c = v[i ^ m], d = v[(i + s) ^ m]: both
// halves of the block are ascending, so a <= b and d <= c, which gives both
// conditions; the outputs go to i, i + s, (i + s) ^ m, i ^ m in that order.
//
// A stage list (TOP, CNT, FLIP) -- register bits TOP .. TOP-CNT+1, the first a
// flip when FLIP -- is walked as pairs from the top; an odd count leaves the
// lowest stage a plain compare-exchange.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NET_R4_HD __host__ __device__ __forceinline__
#else
#define NET_R4_HD inline
#endif

// Build switch (tools/build_variant.sh): MISORT_NET_R4 0 = the 4-byte register
// stages one at a time (reg_stages_c, bitonic.h), two-input min/max alone.
#ifndef MISORT_NET_R4
#define MISORT_NET_R4 1
#endif

namespace misort {
namespace net_r4 {

NET_R4_HD uint32_t min2(uint32_t a, uint32_t b) { return a < b ? a : b; }
NET_R4_HD uint32_t max2(uint32_t a, uint32_t b) { return a < b ? b : a; }
// (the compiler keeps min(min(a, b), c) as two instructions: asm, as merge4 in
// lds_merge.h)
NET_R4_HD uint32_t min3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;
    asm("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
#else
    return min2(min2(a, b), c);
#endif
}
NET_R4_HD uint32_t max3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;
    asm("v_max3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
#else
    return max2(max2(a, b), c);
#endif
}
NET_R4_HD uint32_t med3(uint32_t a, uint32_t b, uint32_t c) {
    return max2(min2(a, b), min2(max2(a, b), c));  // v_med3_u32
}

NET_R4_HD void cx(uint32_t& a, uint32_t& b) {
    const uint32_t lo = min2(a, b), hi = max2(a, b);
    a = lo;
    b = hi;
}

// The radix-4 step: (a, c) and (b, d) compare-exchanged, then (a, b) and
// (c, d), for (a, b, c, d) cyclic-bitonic (see above).
NET_R4_HD void cx4(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
    const uint32_t bl = min2(b, d), bh = max2(b, d);
    const uint32_t o0 = min3(a, c, bl), o1 = med3(a, c, bl), o2 = med3(a, c, bh), o3 = max3(a, c, bh);
    a = o0;
    b = o1;
    c = o2;
    d = o3;
}

// partner of register c at stage r (flip: the mirror inside the 2^(r+1) block)
constexpr int partner(int c, int r, bool flip) { return flip ? (c ^ ((2 << r) - 1)) : (c | (1 << r)); }

// The reference schedule: one stage at a time, two-input min/max.
template <int TOP, int CNT, bool FLIP>
NET_R4_HD void stages_r2(uint32_t (&v)[32]) {
    static_assert(TOP >= 0 && TOP <= 4 && CNT >= 1 && CNT <= TOP + 1, "register bits 4..0");
#if defined(__clang__)
#pragma unroll
#endif
    for (int r = TOP; r > TOP - CNT; --r) {
#if defined(__clang__)
#pragma unroll
#endif
        for (int c = 0; c < 32; ++c)
            if (!(c & (1 << r))) cx(v[c], v[partner(c, r, FLIP && r == TOP)]);
    }
}

// The fused schedule: stages (r, r - 1) as radix-4 steps from the top.
template <int TOP, int CNT, bool FLIP>
NET_R4_HD void stages_r4(uint32_t (&v)[32]) {
    static_assert(TOP >= 0 && TOP <= 4 && CNT >= 1 && CNT <= TOP + 1, "register bits 4..0");
#if defined(__clang__)
#pragma unroll
#endif
    for (int r = TOP; r > TOP - CNT; r -= 2) {
        const bool fl = FLIP && r == TOP;
        if (r - 1 > TOP - CNT) {
            const int s = 1 << (r - 1);
#if defined(__clang__)
#pragma unroll
#endif
            for (int c = 0; c < 32; ++c) {
                if (c & (3 << (r - 1))) continue;
                // flip: c's partner is the upper one of the stage-s pair
                const int ic = partner(c, r, fl), id = partner(c + s, r, fl);
                cx4(v[c], v[c + s], v[ic], v[id]);
                if (fl) {
                    const uint32_t t = v[ic];
                    v[ic] = v[id];
                    v[id] = t;
                }
            }
        } else {
#if defined(__clang__)
#pragma unroll
#endif
            for (int c = 0; c < 32; ++c)
                if (!(c & (1 << r))) cx(v[c], v[partner(c, r, fl)]);
        }
    }
}

}  // namespace net_r4
}  // namespace misort

// corank_seed.h -- the index arithmetic of the in-LDS merge-path (co-rank)
// search (lds_merge.h), as plain C++17 for host and device: the seed, the
// window, the step schedule, the clamps, the failure test and the choice of
// the fallback.  The key loads go through a callable, so corank_seed_dump.cpp
// (host compiler alone) runs the very search the kernels run
// (tests/test_corank_seed_model.py).
//
// The search.  The split of diagonal d of merge(A, B) is the largest i in
// [lo, hi] = [max(0, d - LB), min(d, LA)] with A[i - 1] <= B[d - i] (true at
// lo).  The full search lifts i from lo by power-of-two steps covering hi - lo:
// log2 of the shorter sequence, 10 to 13 steps in a 16-way chunk.  When the
// two sequences hold keys drawn alike -- any iid input, inside a chunk or a
// tile: only ranks matter -- the split is hypergeometric around
// g = d LA / (LA + LB) with sigma <= sqrt(LA + LB) / 4.  The seeded search
// lifts from max(lo, g - W) by the steps covering 2 W, 7 or 8 of them, W about
// sqrt(T) of the level's largest pair T = LA + LB (uniform over the wave, as
// the step count must be).  It takes no phase: seeded lanes start about IT / 2
// words apart, on distinct banks already (the full search's 31-word phase
// measured slower here, the u32 tile above all).  Its answer is the full search's unless it
// sits at its lower start (above lo) or at its full reach (below hi): then the
// lane reports failure, and when any lane of a wave does, the whole wave runs
// the full search, at that level and (sticky) at the rest of its chunk or tile.
#pragma once

#if defined(__HIPCC__)
#define CORANK_HD __host__ __device__ __forceinline__
#else
#define CORANK_HD inline
#endif

// Build switches (tools/build_variant.sh): MISORT_CR_SEED 0 = the full search
// alone at 4-byte keys, MISORT_CR_SEED64 the same at 8-byte keys; MISORT_CR_WQ:
// the window in quarters of the root of T; MISORT_CR_PH: a phase mask for the
// seeded search at 4-byte keys (2^k - 1; the full search's is 31; default none).
#ifndef MISORT_CR_SEED
#define MISORT_CR_SEED 1
#endif
#ifndef MISORT_CR_SEED64
#define MISORT_CR_SEED64 1
#endif
#ifndef MISORT_CR_WQ
#define MISORT_CR_WQ 4
#endif
#ifndef MISORT_CR_PH
#define MISORT_CR_PH 0
#endif

namespace misort {
namespace corank {

static_assert((MISORT_CR_PH & (MISORT_CR_PH + 1)) == 0 && MISORT_CR_PH >= 0 && MISORT_CR_PH <= 31, "phase mask");
static_assert(MISORT_CR_WQ >= 1, "window");

// The phases of a key size: the full search's (lds_merge.h: 31 at 4-byte keys,
// none at 8-byte keys) and the seeded search's.
constexpr int phase_full(int key_bytes) { return key_bytes == 4 ? 31 : 0; }
constexpr int phase_seed(int key_bytes) { return key_bytes == 4 ? MISORT_CR_PH : 0; }
constexpr bool seed_built(int key_bytes) { return key_bytes == 4 ? MISORT_CR_SEED != 0 : MISORT_CR_SEED64 != 0; }

// clamp(t, lo, hi), lo <= hi
CORANK_HD int med3(int t, int lo, int hi) {
#if defined(__HIP_DEVICE_COMPILE__)
    int j;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(j) : "v"(t), "v"(lo), "v"(hi));
    return j;
#else
    return t < lo ? lo : (t > hi ? hi : t);
#endif
}

// the largest power of two <= n (n >= 1): the first step of a lifting search
// whose steps, 2^j <= n, sum to >= n
constexpr int floor_pow2(int n) { return 1 << (31 - __builtin_clz((unsigned)n)); }

// The window of a level whose largest pair holds maxt keys: about sqrt(maxt),
// in quarters (MISORT_CR_WQ).  Integer shifts alone -- on the device this is
// scalar work, once per level: from w0 = 2^ceil(e / 2) >= sqrt(t), e = bits of
// t, one Newton step whose division is a shift, (w0 + t / w0) / 2, lands in
// [sqrt(t) - 1, 1.25 sqrt(t)]; at least 1 (seeded() relies on a window >= 1).
constexpr int root(int t) {
    const int e = t > 0 ? 32 - __builtin_clz((unsigned)t) : 0, k = (e + 1) >> 1;
    const int w = ((1 << k) + (t >> k)) >> 1;
    return w > 1 ? w : 1;
}
constexpr int window(int maxt) { return (root(maxt) * MISORT_CR_WQ + 3) >> 2; }
// a compile-time bound on the seeded search's first step, for pairs of <= maxt
// keys (root() is monotone over the powers of two it is asked at here)
constexpr int seed_step0(int maxt, int ph) { return floor_pow2((2 * window(maxt) + ph) | 1); }

// What a level's searches share (uniform over the workgroup): the bounds the
// steps are skipped by, the seeded search's reach and whether it runs at all
// (only when it saves a step).
struct Level {
    int top_full;  // full search: steps 2^j <= maxr + its phase
    int top_seed;  // seeded search: steps 2^j <= 2 W + its phase
    int reach;     // the seeded steps' sum
    int w;
    bool seeded;
};
// maxr: the level's longest co-rank range (min(LA, LB) over its pairs); maxt:
// its largest pair
constexpr Level level(int maxr, int maxt, int key_bytes) {
    Level L{};
    L.top_full = maxr + phase_full(key_bytes);
    L.w = window(maxt);
    L.top_seed = 2 * L.w + phase_seed(key_bytes);
    const int s = floor_pow2(L.top_seed | 1);
    L.reach = 2 * s - 1;
    L.seeded = seed_built(key_bytes) && s < floor_pow2(L.top_full | 1);
    return L;
}

// The expected split of diagonal d: d LA / (LA + LB) by a float reciprocal
// (d LA < 2^31 here; EQ: LA == LB by the shape).  The device's reciprocal is
// an approximation (1 ulp), so host and device may differ by one at exact
// quotients: the search's answer does not depend on the guess, only which
// groups at a window's very edge fall back.
template <bool EQ>
CORANK_HD int guess(int d, int LA, int LB) {
    if constexpr (EQ) {
        return d >> 1;
    } else {
#if defined(__HIP_DEVICE_COMPILE__)
        // LA + LB = 0: d = 0, 0 * inf = NaN, which converts to 0
        return (int)((float)d * (float)LA * __builtin_amdgcn_rcpf((float)(LA + LB)));
#else
        return LA + LB > 0 ? (int)((float)d * (float)LA * (1.0f / (float)(LA + LB))) : 0;
#endif
    }
}

// The lifting search on positions x = x0 + (i << UL) (UL = 0: indices; the
// zero-word form of lds_merge.h runs on byte addresses of A): from x, the steps
// 2^j <= top from STEP0 down, every probe clamped into [xlo, xhi]; ok(x) loads
// and compares.  No data-dependent branches: `top` is uniform.
template <int STEP0, int UL, typename Probe>
CORANK_HD int lift(int x, int xlo, int xhi, int top, Probe&& ok) {
#if defined(__clang__)
#pragma unroll
#endif
    for (int step = STEP0; step >= 1; step >>= 1) {
        if (step > top) continue;  // uniform
        const int j = med3(x + (step << UL), xlo, xhi);
        x = ok(j) ? j : x;
    }
    return x;
}

// The full search: from lo less the lane's phase ph (positions <= lo count as
// true: ok() must hold at xlo, by a zero word below A or a test of its own).
template <int STEP0, int UL, typename Probe>
CORANK_HD int full(int x0, int lo, int hi, int ph, const Level& L, Probe&& ok) {
    return lift<STEP0, UL>(x0 + ((lo - ph) << UL), x0 + (lo << UL), x0 + (hi << UL), L.top_full, ok);
}

// The seeded search: from max(lo, g - W) less the phase.  failed: the result
// sits at the start while that is above lo (nothing proves the start's own
// predicate), or at the full reach while below hi (nothing bounds it above).
// Otherwise a probe held at the result and failed one past it, or the result
// is a clamp the full search would have stopped at too.
template <int STEP0, int UL, bool EQ, typename Probe>
CORANK_HD int seeded(int x0, int LA, int LB, int d, int lo, int hi, int ph, const Level& L, bool& failed, Probe&& ok) {
    // lo <= g <= hi (d <= LA + LB; the float quotient is off by far less than
    // the window, which is >= 1): the start stays within [lo, hi - 1] or at lo
    const int g = guess<EQ>(d, LA, LB);
    const int st = g - L.w > lo ? g - L.w : lo;
    const int xlo = x0 + (lo << UL), xhi = x0 + (hi << UL);
    const int xs = x0 + ((st - ph) << UL);
    const int x = lift<STEP0, UL>(xs, xlo, xhi, L.top_seed, ok);
    failed = (x == xs && xs > xlo) | (x == xs + (L.reach << UL) && x < xhi);
    return x;
}

// position -> split (a phased search may end below lo: every probe failed)
template <int UL>
CORANK_HD int split_of(int x, int x0, int lo) {
    const int i = (x - x0) >> UL;
    return i > lo ? i : lo;
}

}  // namespace corank
}  // namespace misort

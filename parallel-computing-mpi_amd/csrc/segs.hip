// segs.hip -- the segmented sort's offset sweeps and its long-segment path
// (gfx950).  Segment i of a caller's array is [off[i], off[i + 1]); the class of
// a segment is segment_class(len) of segs_class.h.
//
//   k_seg_count    one lane per segment and trip: validates it (0 <= off[i] <= off[i + 1]
//                  <= n), classifies it and accumulates, per class, the segment
//                  count and the key total; records off[0], off[nseg], the
//                  malformed count and the first malformed index.  Reads only
//                  off[0 .. nseg].  The host reads the header once and turns
//                  the counts into the bases of the class lists.
//   k_seg_scatter  one lane per segment and trip: writes each non-empty segment's index
//                  into its class's list.  The order inside a class is whatever
//                  the atomics give; the output does not depend on it.
// Both aggregate in LDS and issue one global atomic per workgroup and class.
//
//   k_pad_segs     the long classes (k > tile_log2), one k at a time: block r of
//                  the padded buffer gets the keys of segment list[r] (f64:
//                  ord_of_f64 of them) and all-ones above its length;
//   k_unpad_segs   the first len keys of block r go back to out + begin.
// Between them the passes of a 2^k-key local sort run over the count 2^k keys
// (sort_row_blocks, runtime.cpp), as for the long rows of rows.hip, whose shape
// the two sweeps have: 256 lanes, a capped grid that strides, 64-bit indices,
// one 16-byte vector of the padded buffer per lane and trip, element accesses on
// the caller's side (a segment starts anywhere).
//
// No kernel waits on another workgroup; the only global atomics are the adds
// (and the one max) of the two offset sweeps.
#include "kernels.h"
#include "segs_class.h"

namespace misort {

namespace {

constexpr int SEGS_NT = 256;
constexpr int SEGS_MAX_GRID = 1 << 20;  // the sweeps of rows.hip
typedef unsigned long long u64_t;

// Both offset sweeps: a workgroup takes SEGS_ITER trips of 256 consecutive
// segments and keeps SEGS_COPIES LDS counters per class, chosen by the lane, so
// that the lanes of a wave that meet in one class (all of them, for uniform
// lengths) spread over eight LDS addresses, and 2048 segments share one global
// atomic per class.
constexpr int SEGS_ITER = 8, SEGS_COPIES = 8, SEGS_SLOTS = SEG_CLASSES * SEGS_COPIES;

__global__ __launch_bounds__(SEGS_NT) void k_seg_count(const int64_t* __restrict__ off, int64_t nseg, int64_t n,
                                                       int key_bytes, u64_t* __restrict__ hdr) {
    __shared__ unsigned cnt[SEGS_SLOTS];
    __shared__ u64_t keys[SEGS_SLOTS];
    __shared__ unsigned bad;
    __shared__ u64_t bad_at;
    const int t = threadIdx.x;
    for (int i = t; i < SEGS_SLOTS; i += SEGS_NT) {
        cnt[i] = 0;
        keys[i] = 0;
    }
    if (t == 0) {
        bad = 0;
        bad_at = 0;
    }
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * (SEGS_NT * SEGS_ITER) + t;
#pragma unroll
    for (int it = 0; it < SEGS_ITER; ++it) {
        const int64_t i = i0 + it * SEGS_NT;
        if (i >= nseg) break;
        const int64_t b = off[i], e = off[i + 1];
        if (i == 0) hdr[SEG_H_FIRST] = (u64_t)b;
        if (i == nseg - 1) hdr[SEG_H_LAST] = (u64_t)e;
        if (b < 0 || e < b || e > n) {
            atomicAdd(&bad, 1u);
            atomicMax(&bad_at, ~(u64_t)i);  // the largest complement: the first index
        } else {
            const int c = segment_class(e - b, key_bytes);
            if (c >= 0) {
                const int slot = c * SEGS_COPIES + (t & (SEGS_COPIES - 1));
                atomicAdd(&cnt[slot], 1u);
                atomicAdd(&keys[slot], (u64_t)(e - b));
            }
        }
    }
    __syncthreads();
    if (t < SEG_CLASSES) {
        u64_t segs = 0, total = 0;
#pragma unroll
        for (int j = 0; j < SEGS_COPIES; ++j) {
            segs += cnt[t * SEGS_COPIES + j];
            total += keys[t * SEGS_COPIES + j];
        }
        if (segs) {
            atomicAdd(&hdr[SEG_H_COUNT + t], segs);
            atomicAdd(&hdr[SEG_H_KEYS + t], total);
        }
    } else if (t == SEG_CLASSES && bad) {
        atomicAdd(&hdr[SEG_H_BAD], (u64_t)bad);
        atomicMax(&hdr[SEG_H_BAD_AT], bad_at);
    }
}

// The offsets were validated by k_seg_count: every length is in [0, n].
__global__ __launch_bounds__(SEGS_NT) void k_seg_scatter(const int64_t* __restrict__ off, int64_t nseg,
                                                         int key_bytes, u64_t* __restrict__ cursor,
                                                         uint32_t* __restrict__ lists, int64_t listed) {
    __shared__ unsigned cnt[SEGS_SLOTS];
    __shared__ u64_t base[SEGS_SLOTS];
    const int t = threadIdx.x;
    for (int i = t; i < SEGS_SLOTS; i += SEGS_NT) cnt[i] = 0;
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * (SEGS_NT * SEGS_ITER) + t;
    int slot[SEGS_ITER];
    unsigned rank[SEGS_ITER];  // among the workgroup's segments of the slot
#pragma unroll
    for (int it = 0; it < SEGS_ITER; ++it) {
        const int64_t i = i0 + it * SEGS_NT;
        slot[it] = -1;
        rank[it] = 0;
        if (i < nseg) {
            const int c = segment_class(off[i + 1] - off[i], key_bytes);
            if (c >= 0) {
                slot[it] = c * SEGS_COPIES + (t & (SEGS_COPIES - 1));
                rank[it] = atomicAdd(&cnt[slot[it]], 1u);
            }
        }
    }
    __syncthreads();
    if (t < SEG_CLASSES) {
        u64_t before[SEGS_COPIES], total = 0;
#pragma unroll
        for (int j = 0; j < SEGS_COPIES; ++j) {
            before[j] = total;
            total += cnt[t * SEGS_COPIES + j];
        }
        if (total) {
            const u64_t b = atomicAdd(&cursor[t], total);
#pragma unroll
            for (int j = 0; j < SEGS_COPIES; ++j) base[t * SEGS_COPIES + j] = b + before[j];
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < SEGS_ITER; ++it) {
        if (slot[it] < 0) continue;
        const u64_t at = base[slot[it]] + rank[it];
        // (listed: the host's total; offsets a caller changed since the count cannot overrun the lists)
        if (at < (u64_t)listed) lists[at] = (uint32_t)(i0 + it * SEGS_NT);
    }
}

template <typename K, bool FLT>
__global__ __launch_bounds__(SEGS_NT) void k_pad_segs(const K* in, const int64_t* __restrict__ off,
                                                      const uint32_t* __restrict__ list, K* __restrict__ padded,
                                                      int64_t count, int k) {
    constexpr int W = 16 / (int)sizeof(K);
    typedef K vec_t __attribute__((ext_vector_type(W)));
    const int64_t nq = (count << k) / W, cm = ((int64_t)1 << k) - 1;
    const int64_t stride = (int64_t)gridDim.x * SEGS_NT;
    for (int64_t q = (int64_t)blockIdx.x * SEGS_NT + threadIdx.x; q < nq; q += stride) {
        const int64_t p = q * W, r = p >> k, c = p & cm;
        const int64_t g = list[r];
        const int64_t b = off[g], len = off[g + 1] - b;
        vec_t v;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            K x = ~(K)0;
            if (c + j < len) {
                x = in[b + c + j];
                if constexpr (FLT) x = (K)ord_of_f64((uint64_t)x);  // real keys only
            }
            v[j] = x;
        }
        reinterpret_cast<vec_t*>(padded)[q] = v;
    }
}

template <typename K, bool FLT>
__global__ __launch_bounds__(SEGS_NT) void k_unpad_segs(const K* __restrict__ padded, K* out,
                                                        const int64_t* __restrict__ off,
                                                        const uint32_t* __restrict__ list, int64_t count, int k) {
    constexpr int W = 16 / (int)sizeof(K);
    typedef K vec_t __attribute__((ext_vector_type(W)));
    const int64_t nq = (count << k) / W, cm = ((int64_t)1 << k) - 1;
    const int64_t stride = (int64_t)gridDim.x * SEGS_NT;
    for (int64_t q = (int64_t)blockIdx.x * SEGS_NT + threadIdx.x; q < nq; q += stride) {
        const int64_t p = q * W, r = p >> k, c = p & cm;
        const int64_t g = list[r];
        const int64_t b = off[g], len = off[g + 1] - b;
        if (c >= len) continue;  // padding only: not read
        const vec_t v = reinterpret_cast<const vec_t*>(padded)[q];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            K x = v[j];
            if constexpr (FLT) x = (K)f64_of_ord((uint64_t)x);  // never stored where it is padding
            if (c + j < len) out[b + c + j] = x;
        }
    }
}

unsigned segs_grid(int64_t nq) {
    const int64_t g = (nq + SEGS_NT - 1) / SEGS_NT;
    return (unsigned)(g < 1 ? 1 : g > SEGS_MAX_GRID ? SEGS_MAX_GRID : g);
}

// k >= 2 keeps a block a whole number of vectors
bool segs_args_ok(const void* user, const void* padded, const int64_t* off, const uint32_t* list, int64_t count, int k,
                  int key_bytes, bool f64) {
    if (!user || !padded || !off || !list || !aligned16(padded) || (key_bytes != 4 && key_bytes != 8) ||
        (f64 && key_bytes != 8))
        return false;
    return k >= 2 && k <= 58 && count <= (INT64_MAX >> k) / key_bytes;
}

double segs_bytes(int64_t count, int64_t keys, int k, int key_bytes) {
    return ((double)keys + (double)count * (double)((int64_t)1 << k)) * key_bytes;
}

}  // namespace

hipError_t seg_count(const int64_t* off, int64_t nseg, int64_t n, int key_bytes, void* hdr, hipStream_t s,
                     LaunchHook* hook) {
    if (nseg <= 0) return hipSuccess;
    if (!off || !hdr || nseg > 0x7FFFFFFF || n < 0 || (key_bytes != 4 && key_bytes != 8)) return hipErrorInvalidValue;
    HookScope hs(hook, KIND_OTHER, ((double)nseg + 1) * 8.0, s);
    const unsigned g = (unsigned)((nseg + SEGS_NT * SEGS_ITER - 1) / (SEGS_NT * SEGS_ITER));
    k_seg_count<<<g, SEGS_NT, 0, s>>>(off, nseg, n, key_bytes, (u64_t*)hdr);
    return hipGetLastError();
}

hipError_t seg_scatter(const int64_t* off, int64_t nseg, int key_bytes, void* cursor, uint32_t* lists,
                       int64_t listed, hipStream_t s, LaunchHook* hook) {
    if (nseg <= 0 || listed <= 0) return hipSuccess;
    if (!off || !cursor || !lists || nseg > 0x7FFFFFFF || (key_bytes != 4 && key_bytes != 8))
        return hipErrorInvalidValue;
    HookScope hs(hook, KIND_OTHER, ((double)nseg + 1) * 8.0 + (double)listed * 4.0, s);
    const unsigned g = (unsigned)((nseg + SEGS_NT * SEGS_ITER - 1) / (SEGS_NT * SEGS_ITER));
    k_seg_scatter<<<g, SEGS_NT, 0, s>>>(off, nseg, key_bytes, (u64_t*)cursor, lists, listed);
    return hipGetLastError();
}

hipError_t pad_segs(const void* in, const int64_t* off, const uint32_t* list, int64_t count, int64_t keys,
                    void* padded, int k, int key_bytes, bool f64, hipStream_t s, LaunchHook* hook) {
    if (count <= 0) return hipSuccess;
    if (!segs_args_ok(in, padded, off, list, count, k, key_bytes, f64)) return hipErrorInvalidValue;
    HookScope hs(hook, KIND_OTHER, segs_bytes(count, keys, k, key_bytes), s);
    const unsigned g = segs_grid((count << k) / (16 / key_bytes));
    if (key_bytes == 4)
        k_pad_segs<uint32_t, false><<<g, SEGS_NT, 0, s>>>((const uint32_t*)in, off, list, (uint32_t*)padded, count, k);
    else if (f64)
        k_pad_segs<uint64_t, true><<<g, SEGS_NT, 0, s>>>((const uint64_t*)in, off, list, (uint64_t*)padded, count, k);
    else
        k_pad_segs<uint64_t, false><<<g, SEGS_NT, 0, s>>>((const uint64_t*)in, off, list, (uint64_t*)padded, count, k);
    return hipGetLastError();
}

hipError_t unpad_segs(const void* padded, void* out, const int64_t* off, const uint32_t* list, int64_t count,
                      int64_t keys, int k, int key_bytes, bool f64, hipStream_t s, LaunchHook* hook) {
    if (count <= 0) return hipSuccess;
    if (!segs_args_ok(out, padded, off, list, count, k, key_bytes, f64)) return hipErrorInvalidValue;
    HookScope hs(hook, KIND_OTHER, segs_bytes(count, keys, k, key_bytes), s);
    const unsigned g = segs_grid((count << k) / (16 / key_bytes));
    if (key_bytes == 4)
        k_unpad_segs<uint32_t, false><<<g, SEGS_NT, 0, s>>>((const uint32_t*)padded, (uint32_t*)out, off, list, count, k);
    else if (f64)
        k_unpad_segs<uint64_t, true><<<g, SEGS_NT, 0, s>>>((const uint64_t*)padded, (uint64_t*)out, off, list, count, k);
    else
        k_unpad_segs<uint64_t, false><<<g, SEGS_NT, 0, s>>>((const uint64_t*)padded, (uint64_t*)out, off, list, count, k);
    return hipGetLastError();
}

}  // namespace misort

// pairs.hip -- the streaming and gather kernels of the key-value sorts (gfx950).
//
// 32-bit keys: a pair (32-bit key, 32-bit value) travels through the u64 sort
// as the record (K(key) << 32) | value, whose unsigned order is "by key, then by
// value".  zip_pairs builds the records, unzip_pairs takes them apart again; the
// sort between them is the unchanged u64 path.  K is the identity for u32 keys
// and the 32-bit form of ord_of_f64 for f32 keys.
//
// 64-bit keys (second half of the file): two such sorts, least-significant half
// of K(key) first, with zip_lo64, gather_hi64 and emit64 around them.
//
// All kernels are HBM-bound: 256 lanes, a capped grid (2048 workgroups for the
// 32-bit kernels, PAIRS64_MAX_GRID for the 64-bit ones) that strides over the
// rest, 64-bit indices, no LDS.  A lane takes four consecutive
// elements per trip: 16-byte accesses on the record arrays, and four
// independent loads in flight where it gathers.  The caller's arrays are only
// known to be element-aligned (a slice t[1:] is a legal argument), so a launcher
// takes the vector kernel only when every caller pointer it streams is 16-byte
// aligned, else the same kernel with element-sized accesses on the caller's
// side (no peeled head).  The record buffers are the context's own and always
// 16-byte aligned.
#include "kernels.h"

namespace misort {

namespace {

constexpr int PAIRS_NT = 256, PAIRS_MAX_GRID = 2048;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

// K = ord_of_f32 / f32_of_ord (kernels.h) for f32 keys.
template <bool F32>
__device__ __forceinline__ uint64_t rec_of(uint32_t k, uint32_t v) {
    return (uint64_t)(F32 ? ord_of_f32(k) : k) << 32 | v;
}
template <bool F32>
__device__ __forceinline__ uint32_t key_of(uint64_t r) {
    const uint32_t o = (uint32_t)(r >> 32);
    return F32 ? f32_of_ord(o) : o;
}

// Four u32 at p + 4 q: one 16-byte access (VEC: p is 16-byte aligned) or four 4-byte ones.
template <bool VEC>
__device__ __forceinline__ u32x4 load4(const uint32_t* __restrict__ p, int64_t q) {
    if constexpr (VEC) return ((const u32x4*)p)[q];
    const uint32_t* e = p + 4 * q;
    return u32x4{e[0], e[1], e[2], e[3]};
}
template <bool VEC>
__device__ __forceinline__ void store4(uint32_t* __restrict__ p, int64_t q, u32x4 x) {
    if constexpr (VEC) {
        ((u32x4*)p)[q] = x;
    } else {
        uint32_t* e = p + 4 * q;
        e[0] = x.x, e[1] = x.y, e[2] = x.z, e[3] = x.w;
    }
}

// rec[i] = K(keys[i]) << 32 | (vals ? vals[i] : val_base + i).  The last n % 4
// pairs are the scalar tail, taken by the first lanes of the grid.
template <bool VEC, bool F32>
__global__ __launch_bounds__(PAIRS_NT) void k_zip_pairs(const uint32_t* __restrict__ keys,
                                                        const uint32_t* __restrict__ vals, uint32_t val_base,
                                                        uint64_t* __restrict__ rec, int64_t n) {
    const int64_t nq = n >> 2;
    const int64_t t0 = (int64_t)blockIdx.x * PAIRS_NT + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * PAIRS_NT;
    u64x2* __restrict__ r2 = (u64x2*)rec;
    for (int64_t q = t0; q < nq; q += stride) {
        const u32x4 k = load4<VEC>(keys, q);
        u32x4 v;
        if (vals) {
            v = load4<VEC>(vals, q);
        } else {
            const uint32_t b = val_base + (uint32_t)(q << 2);
            v = u32x4{b, b + 1u, b + 2u, b + 3u};
        }
        r2[2 * q] = u64x2{rec_of<F32>(k.x, v.x), rec_of<F32>(k.y, v.y)};
        r2[2 * q + 1] = u64x2{rec_of<F32>(k.z, v.z), rec_of<F32>(k.w, v.w)};
    }
    const int64_t i = (nq << 2) + t0;
    if (i < n) rec[i] = rec_of<F32>(keys[i], vals ? vals[i] : val_base + (uint32_t)i);
}

// The inverse: keys[i] (if keys) and vals[i] from rec[i].
template <bool VEC, bool F32>
__global__ __launch_bounds__(PAIRS_NT) void k_unzip_pairs(const uint64_t* __restrict__ rec,
                                                          uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                          int64_t n) {
    const int64_t nq = n >> 2;
    const int64_t t0 = (int64_t)blockIdx.x * PAIRS_NT + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * PAIRS_NT;
    const u64x2* __restrict__ r2 = (const u64x2*)rec;
    for (int64_t q = t0; q < nq; q += stride) {
        const u64x2 a = r2[2 * q], b = r2[2 * q + 1];
        if (keys) store4<VEC>(keys, q, u32x4{key_of<F32>(a.x), key_of<F32>(a.y), key_of<F32>(b.x), key_of<F32>(b.y)});
        store4<VEC>(vals, q, u32x4{(uint32_t)a.x, (uint32_t)a.y, (uint32_t)b.x, (uint32_t)b.y});
    }
    const int64_t i = (nq << 2) + t0;
    if (i < n) {
        const uint64_t r = rec[i];
        if (keys) keys[i] = key_of<F32>(r);
        vals[i] = (uint32_t)r;
    }
}

// One lane per four pairs, at least one workgroup (the tail of n < 4).
unsigned pairs_grid(int64_t n) {
    const int64_t g = ((n >> 2) + PAIRS_NT - 1) / PAIRS_NT;
    return (unsigned)(g < 1 ? 1 : g > PAIRS_MAX_GRID ? PAIRS_MAX_GRID : g);
}

}  // namespace

hipError_t zip_pairs(const uint32_t* keys, const uint32_t* vals, uint32_t val_base, uint64_t* rec, int64_t n,
                     bool f32, hipStream_t s, LaunchHook* hook) {
    if (n <= 0) return hipSuccess;
    if (!aligned16(rec)) return hipErrorInvalidValue;
    const bool vec = aligned16(keys) && aligned16(vals);  // a null vals is not read
    HookScope os(hook, KIND_OTHER, (double)n * (vals ? 16.0 : 12.0), s);
    const unsigned g = pairs_grid(n);
    if (vec && f32) k_zip_pairs<true, true><<<g, PAIRS_NT, 0, s>>>(keys, vals, val_base, rec, n);
    else if (vec) k_zip_pairs<true, false><<<g, PAIRS_NT, 0, s>>>(keys, vals, val_base, rec, n);
    else if (f32) k_zip_pairs<false, true><<<g, PAIRS_NT, 0, s>>>(keys, vals, val_base, rec, n);
    else k_zip_pairs<false, false><<<g, PAIRS_NT, 0, s>>>(keys, vals, val_base, rec, n);
    return hipGetLastError();
}

hipError_t unzip_pairs(const uint64_t* rec, uint32_t* keys, uint32_t* vals, int64_t n, bool f32, hipStream_t s,
                       LaunchHook* hook) {
    if (n <= 0) return hipSuccess;
    if (!aligned16(rec) || !vals) return hipErrorInvalidValue;
    const bool vec = aligned16(keys) && aligned16(vals);  // a null keys is not written
    HookScope os(hook, KIND_OTHER, (double)n * (keys ? 16.0 : 12.0), s);
    const unsigned g = pairs_grid(n);
    if (vec && f32) k_unzip_pairs<true, true><<<g, PAIRS_NT, 0, s>>>(rec, keys, vals, n);
    else if (vec) k_unzip_pairs<true, false><<<g, PAIRS_NT, 0, s>>>(rec, keys, vals, n);
    else if (f32) k_unzip_pairs<false, true><<<g, PAIRS_NT, 0, s>>>(rec, keys, vals, n);
    else k_unzip_pairs<false, false><<<g, PAIRS_NT, 0, s>>>(rec, keys, vals, n);
    return hipGetLastError();
}

// ------------------------------------------------------------- 64-bit keys
//
// The stable argsort of 64-bit keys as two sorts of distinct u64 records, least
// significant half first (K = ord_of_f64 for f64 keys, the identity for u64):
//   zip_lo64     rec1[i] = lo(K(keys[i])) << 32 | i              -> sorted: S1
//   gather_hi64  rec2[j] = hi(K(keys[S1[j] & M])) << 32 | j       -> sorted: S2
//   emit64       t -> j = S2[t] & M, r = S1[j], i = r & M: index i, value
//                vals[i], key unK(hi(S2[t]) << 32 | r >> 32)
// (M = 2^32 - 1).  j is the rank in (lo, i) order, so S2 is in (hi, lo, i)
// order: by key, equal keys in input order.  The gathers (the keys in
// gather_hi64; S1 and the values in emit64) are element-sized random reads;
// everything else streams.

namespace {

// The grid cap of these three kernels: one trip per lane up to 2^30 elements,
// grid-stride beyond.  Measured at 2^28 against the 2048 of the 32-bit
// kernels (alternating builds on one MI355X, profiles/pairs64/grid_cap_ab.jsonl):
// zip_lo 0.71-0.74 against 0.79-0.84 ms, gather_hi 6.1-6.95 against 6.5-7.4
// (each 6 % under its neighbour in time), emit 6.5 against 6.96; caps of 32768
// and 65536 workgroups match it except in emit (6.7).
constexpr int PAIRS64_MAX_GRID = 1 << 20;

unsigned pairs64_grid(int64_t n) {
    const int64_t g = ((n >> 2) + PAIRS_NT - 1) / PAIRS_NT;
    return (unsigned)(g < 1 ? 1 : g > PAIRS64_MAX_GRID ? PAIRS64_MAX_GRID : g);
}

template <bool F64>
__device__ __forceinline__ uint64_t ord64(uint64_t k) { return F64 ? ord_of_f64(k) : k; }
template <bool F64>
__device__ __forceinline__ uint64_t lo_rec(uint64_t k, uint32_t i) { return ord64<F64>(k) << 32 | i; }
template <bool F64>
__device__ __forceinline__ uint64_t hi_rec(uint64_t k, uint32_t j) {
    return (ord64<F64>(k) & 0xFFFFFFFF00000000ull) | j;
}
// The key of output t from its two records: hi from S2[t], lo from S1[j].
template <bool F64>
__device__ __forceinline__ uint64_t key_of2(uint64_t t, uint64_t r) {
    const uint64_t o = (t & 0xFFFFFFFF00000000ull) | (r >> 32);
    return F64 ? f64_of_ord(o) : o;
}

// Two u64 at p + 2 h: one 16-byte access (VEC: p is 16-byte aligned) or two 8-byte ones.
template <bool VEC>
__device__ __forceinline__ u64x2 load2(const uint64_t* __restrict__ p, int64_t h) {
    if constexpr (VEC) return ((const u64x2*)p)[h];
    return u64x2{p[2 * h], p[2 * h + 1]};
}
template <bool VEC>
__device__ __forceinline__ void store2(uint64_t* __restrict__ p, int64_t h, u64x2 x) {
    if constexpr (VEC) ((u64x2*)p)[h] = x;
    else p[2 * h] = x.x, p[2 * h + 1] = x.y;
}

template <bool VEC, bool F64>
__global__ __launch_bounds__(PAIRS_NT) void k_zip_lo(const uint64_t* __restrict__ keys, uint64_t* __restrict__ rec,
                                                     int64_t n) {
    const int64_t nq = n >> 2;
    const int64_t t0 = (int64_t)blockIdx.x * PAIRS_NT + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * PAIRS_NT;
    u64x2* __restrict__ r2 = (u64x2*)rec;
    for (int64_t q = t0; q < nq; q += stride) {
        const u64x2 a = load2<VEC>(keys, 2 * q), b = load2<VEC>(keys, 2 * q + 1);
        const uint32_t i = (uint32_t)(q << 2);
        r2[2 * q] = u64x2{lo_rec<F64>(a.x, i), lo_rec<F64>(a.y, i + 1u)};
        r2[2 * q + 1] = u64x2{lo_rec<F64>(b.x, i + 2u), lo_rec<F64>(b.y, i + 3u)};
    }
    const int64_t i = (nq << 2) + t0;
    if (i < n) rec[i] = lo_rec<F64>(keys[i], (uint32_t)i);
}

// s1 holds a permutation of the indices 0..n-1 in its low halves: every gather is in bounds.
template <bool F64>
__global__ __launch_bounds__(PAIRS_NT) void k_gather_hi(const uint64_t* __restrict__ s1,
                                                        const uint64_t* __restrict__ keys,
                                                        uint64_t* __restrict__ rec, int64_t n) {
    const int64_t nq = n >> 2;
    const int64_t t0 = (int64_t)blockIdx.x * PAIRS_NT + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * PAIRS_NT;
    const u64x2* __restrict__ s2 = (const u64x2*)s1;
    u64x2* __restrict__ r2 = (u64x2*)rec;
    for (int64_t q = t0; q < nq; q += stride) {
        const u64x2 a = s2[2 * q], b = s2[2 * q + 1];
        const uint64_t k0 = keys[(uint32_t)a.x], k1 = keys[(uint32_t)a.y];  // four loads in flight
        const uint64_t k2 = keys[(uint32_t)b.x], k3 = keys[(uint32_t)b.y];
        const uint32_t j = (uint32_t)(q << 2);
        r2[2 * q] = u64x2{hi_rec<F64>(k0, j), hi_rec<F64>(k1, j + 1u)};
        r2[2 * q + 1] = u64x2{hi_rec<F64>(k2, j + 2u), hi_rec<F64>(k3, j + 3u)};
    }
    const int64_t j = (nq << 2) + t0;
    if (j < n) rec[j] = hi_rec<F64>(keys[(uint32_t)s1[j]], (uint32_t)j);
}

// VB: bytes of a value, 0 = no values, the indices are the output (u32).
// keys_out may be null.  The low halves of s2 and s1 are permutations of 0..n-1.
template <bool VEC, bool F64, int VB>
__global__ __launch_bounds__(PAIRS_NT) void k_emit(const uint64_t* __restrict__ s2, const uint64_t* __restrict__ s1,
                                                   const void* __restrict__ vals_in, uint64_t* __restrict__ keys_out,
                                                   void* __restrict__ vals_out, int64_t n) {
    const int64_t nq = n >> 2;
    const int64_t t0 = (int64_t)blockIdx.x * PAIRS_NT + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * PAIRS_NT;
    const u64x2* __restrict__ sv = (const u64x2*)s2;
    for (int64_t q = t0; q < nq; q += stride) {
        const u64x2 a = sv[2 * q], b = sv[2 * q + 1];
        const uint64_t r0 = s1[(uint32_t)a.x], r1 = s1[(uint32_t)a.y];  // four loads in flight
        const uint64_t r2 = s1[(uint32_t)b.x], r3 = s1[(uint32_t)b.y];
        if (keys_out) {
            store2<VEC>(keys_out, 2 * q, u64x2{key_of2<F64>(a.x, r0), key_of2<F64>(a.y, r1)});
            store2<VEC>(keys_out, 2 * q + 1, u64x2{key_of2<F64>(b.x, r2), key_of2<F64>(b.y, r3)});
        }
        const uint32_t i0 = (uint32_t)r0, i1 = (uint32_t)r1, i2 = (uint32_t)r2, i3 = (uint32_t)r3;
        if constexpr (VB == 0) {
            store4<VEC>((uint32_t*)vals_out, q, u32x4{i0, i1, i2, i3});
        } else if constexpr (VB == 4) {
            const uint32_t* __restrict__ v = (const uint32_t*)vals_in;
            store4<VEC>((uint32_t*)vals_out, q, u32x4{v[i0], v[i1], v[i2], v[i3]});
        } else {
            const uint64_t* __restrict__ v = (const uint64_t*)vals_in;
            const uint64_t v0 = v[i0], v1 = v[i1], v2 = v[i2], v3 = v[i3];
            store2<VEC>((uint64_t*)vals_out, 2 * q, u64x2{v0, v1});
            store2<VEC>((uint64_t*)vals_out, 2 * q + 1, u64x2{v2, v3});
        }
    }
    const int64_t t = (nq << 2) + t0;
    if (t < n) {
        const uint64_t x = s2[t], r = s1[(uint32_t)x];
        const uint32_t i = (uint32_t)r;
        if (keys_out) keys_out[t] = key_of2<F64>(x, r);
        if constexpr (VB == 0) ((uint32_t*)vals_out)[t] = i;
        else if constexpr (VB == 4) ((uint32_t*)vals_out)[t] = ((const uint32_t*)vals_in)[i];
        else ((uint64_t*)vals_out)[t] = ((const uint64_t*)vals_in)[i];
    }
}

template <bool VEC, bool F64>
void launch_emit(int vb, unsigned g, hipStream_t s, const uint64_t* s2, const uint64_t* s1, const void* vals_in,
                 uint64_t* keys_out, void* vals_out, int64_t n) {
    if (vb == 0) k_emit<VEC, F64, 0><<<g, PAIRS_NT, 0, s>>>(s2, s1, vals_in, keys_out, vals_out, n);
    else if (vb == 4) k_emit<VEC, F64, 4><<<g, PAIRS_NT, 0, s>>>(s2, s1, vals_in, keys_out, vals_out, n);
    else k_emit<VEC, F64, 8><<<g, PAIRS_NT, 0, s>>>(s2, s1, vals_in, keys_out, vals_out, n);
}

}  // namespace

hipError_t zip_lo64(const uint64_t* keys, uint64_t* rec, int64_t n, bool f64, hipStream_t s, LaunchHook* hook) {
    if (n <= 0) return hipSuccess;
    if (!aligned16(rec) || !keys || n > ((int64_t)1 << 32)) return hipErrorInvalidValue;
    const bool vec = aligned16(keys);
    HookScope os(hook, KIND_OTHER, (double)n * 16.0, s);
    const unsigned g = pairs64_grid(n);
    if (vec && f64) k_zip_lo<true, true><<<g, PAIRS_NT, 0, s>>>(keys, rec, n);
    else if (vec) k_zip_lo<true, false><<<g, PAIRS_NT, 0, s>>>(keys, rec, n);
    else if (f64) k_zip_lo<false, true><<<g, PAIRS_NT, 0, s>>>(keys, rec, n);
    else k_zip_lo<false, false><<<g, PAIRS_NT, 0, s>>>(keys, rec, n);
    return hipGetLastError();
}

hipError_t gather_hi64(const uint64_t* s1, const uint64_t* keys, uint64_t* rec, int64_t n, bool f64, hipStream_t s,
                       LaunchHook* hook) {
    if (n <= 0) return hipSuccess;
    if (!aligned16(s1) || !aligned16(rec) || s1 == rec || !keys || n > ((int64_t)1 << 32))
        return hipErrorInvalidValue;
    HookScope os(hook, KIND_OTHER, (double)n * 24.0, s);
    const unsigned g = pairs64_grid(n);
    if (f64) k_gather_hi<true><<<g, PAIRS_NT, 0, s>>>(s1, keys, rec, n);
    else k_gather_hi<false><<<g, PAIRS_NT, 0, s>>>(s1, keys, rec, n);
    return hipGetLastError();
}

hipError_t emit64(const uint64_t* s2, const uint64_t* s1, const void* vals_in, int val_bytes, uint64_t* keys_out,
                  void* vals_out, int64_t n, bool f64, hipStream_t s, LaunchHook* hook) {
    if (n <= 0) return hipSuccess;
    if (!aligned16(s2) || !aligned16(s1) || !vals_out || n > ((int64_t)1 << 32)) return hipErrorInvalidValue;
    if (vals_in ? (val_bytes != 4 && val_bytes != 8) : val_bytes != 4) return hipErrorInvalidValue;
    const int vb = vals_in ? val_bytes : 0;
    const bool vec = aligned16(keys_out) && aligned16(vals_out);  // a null keys_out is not written
    HookScope os(hook, KIND_OTHER, (double)n * (16.0 + (keys_out ? 8.0 : 0.0) + (vb ? 2.0 * vb : 4.0)), s);
    const unsigned g = pairs64_grid(n);
    if (vec && f64) launch_emit<true, true>(vb, g, s, s2, s1, vals_in, keys_out, vals_out, n);
    else if (vec) launch_emit<true, false>(vb, g, s, s2, s1, vals_in, keys_out, vals_out, n);
    else if (f64) launch_emit<false, true>(vb, g, s, s2, s1, vals_in, keys_out, vals_out, n);
    else launch_emit<false, false>(vb, g, s, s2, s1, vals_in, keys_out, vals_out, n);
    return hipGetLastError();
}

}  // namespace misort

// pairs.hip -- the two streaming kernels of the key-value sort (gfx950).
//
// A pair (32-bit key, 32-bit value) travels through the u64 sort as the record
// (K(key) << 32) | value, whose unsigned order is "by key, then by value".
// zip_pairs builds the records, unzip_pairs takes them apart again; the sort
// between them is the unchanged u64 path.  K is the identity for u32 keys and
// the 32-bit form of ord_of_f64 for f32 keys.
//
// Both kernels are pure HBM streaming: 256 lanes, a grid capped at 2048
// workgroups that strides over the rest, 64-bit indices, no LDS.  A lane takes
// four consecutive pairs per trip: one 16-byte access per key and value array
// and two per record array.  The caller's arrays are only known to be 4-byte
// aligned (a slice t[1:] is a legal argument), so the launcher takes the
// vector kernel only when every caller pointer it touches is 16-byte aligned,
// else the same kernel with 4-byte accesses on the caller's side (no peeled
// head).  The record buffer is the context's own and always 16-byte aligned.
#include "kernels.h"

namespace misort {

namespace {

constexpr int PAIRS_NT = 256, PAIRS_MAX_GRID = 2048;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

// IEEE float bits <-> order-preserving u32 (ord_of_f64 / f64_of_ord on 32 bits).
__device__ __forceinline__ uint32_t ord_of_f32(uint32_t b) { return (b >> 31) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ uint32_t f32_of_ord(uint32_t o) { return (o >> 31) ? (o & 0x7FFFFFFFu) : ~o; }

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

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct OtherScope {  // the launch's KIND_OTHER record
    LaunchHook* h;
    hipStream_t s;
    OtherScope(LaunchHook* h_, double bytes, hipStream_t s_) : h(h_), s(s_) {
        if (h) h->before(KIND_OTHER, bytes, s);
    }
    ~OtherScope() {
        if (h) h->after(KIND_OTHER, s);
    }
};

}  // namespace

hipError_t zip_pairs(const uint32_t* keys, const uint32_t* vals, uint32_t val_base, uint64_t* rec, int64_t n,
                     bool f32, hipStream_t s, LaunchHook* hook) {
    if (n <= 0) return hipSuccess;
    if (!aligned16(rec)) return hipErrorInvalidValue;
    const bool vec = aligned16(keys) && aligned16(vals);  // a null vals is not read
    OtherScope os(hook, (double)n * (vals ? 16.0 : 12.0), s);
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
    OtherScope os(hook, (double)n * (keys ? 16.0 : 12.0), s);
    const unsigned g = pairs_grid(n);
    if (vec && f32) k_unzip_pairs<true, true><<<g, PAIRS_NT, 0, s>>>(rec, keys, vals, n);
    else if (vec) k_unzip_pairs<true, false><<<g, PAIRS_NT, 0, s>>>(rec, keys, vals, n);
    else if (f32) k_unzip_pairs<false, true><<<g, PAIRS_NT, 0, s>>>(rec, keys, vals, n);
    else k_unzip_pairs<false, false><<<g, PAIRS_NT, 0, s>>>(rec, keys, vals, n);
    return hipGetLastError();
}

}  // namespace misort

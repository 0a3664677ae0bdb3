// rows.hip -- the long-row path of the row-wise sort (gfx950) and its plan.
//
// A row longer than the largest SORT tile is sorted as a block of 2^k keys,
// k = ceil_log2(cols): pad_rows copies every row to the start of its block and
// fills the rest with all-ones, the passes of a 2^k-key local sort run over
// the rows * 2^k keys (local_sort's block_log2: every pass merges its groups of
// runs on their own, so every aligned block is sorted), and unpad_rows writes
// the first cols keys of every block back.  The all-ones suffix of a block
// sorts to its end, whatever real keys equal it.
//
// f64 keys are mapped to ordered u64 HERE, in the two kernels, and the sort
// between them runs on plain u64: the SORT tile's own f64 load would map the
// raw all-ones padding (a negative NaN pattern) to 0, the smallest key.
//
// Both kernels are HBM-bound and shaped like pairs.hip's: 256 lanes, a capped
// grid that strides over the rest, 64-bit indices, one 16-byte vector of the
// padded buffer per lane and trip.  The padded buffer is the context's own and
// 16-byte aligned; the caller's array is only known to be element-aligned, so
// the launchers take the vector kernel when it is 16-byte aligned and cols is a
// multiple of the vector (every vector then lies inside one row), else element
// accesses on the caller's side.
//
// The key-value rows (second pair of kernels) take the same path on u64
// records: pad_rows_pairs zips keys and values into the padded buffer,
// unpad_rows_pairs splits the sorted records into the two outputs.
#include "kernels.h"

namespace misort {

namespace {

constexpr int ROWS_NT = 256;
// one trip per lane up to 2^28 vectors, as the 64-bit pair kernels (pairs.hip)
constexpr int ROWS_MAX_GRID = 1 << 20;

template <typename K>
struct RowVec {
    static constexpr int V = 16 / (int)sizeof(K);
    typedef K type __attribute__((ext_vector_type(V)));
};

template <typename K, bool VEC, bool F64>
__global__ __launch_bounds__(ROWS_NT) void k_pad_rows(const K* __restrict__ in, K* __restrict__ padded, int64_t rows,
                                                      int64_t cols, int k) {
    constexpr int V = RowVec<K>::V;
    typedef typename RowVec<K>::type vec_t;
    const int64_t nq = (rows << k) / V, cm = ((int64_t)1 << k) - 1;
    const int64_t stride = (int64_t)gridDim.x * ROWS_NT;
    for (int64_t q = (int64_t)blockIdx.x * ROWS_NT + threadIdx.x; q < nq; q += stride) {
        const int64_t p = q * V, r = p >> k, c = p & cm;
        const K* src = in + (r * cols + c);
        vec_t x = {};
        if constexpr (VEC) {
            // cols % V == 0: the whole vector is real or none of it
            if (c < cols) x = *reinterpret_cast<const vec_t*>(src);
#pragma unroll
            for (int j = 0; j < V; ++j) x[j] = c >= cols ? ~(K)0 : F64 ? (K)ord_of_f64((uint64_t)x[j]) : x[j];
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                K y = ~(K)0;
                if (c + j < cols) y = F64 ? (K)ord_of_f64((uint64_t)src[j]) : src[j];
                x[j] = y;
            }
        }
        reinterpret_cast<vec_t*>(padded)[q] = x;
    }
}

template <typename K, bool VEC, bool F64>
__global__ __launch_bounds__(ROWS_NT) void k_unpad_rows(const K* __restrict__ padded, K* __restrict__ out,
                                                        int64_t rows, int64_t cols, int k) {
    constexpr int V = RowVec<K>::V;
    typedef typename RowVec<K>::type vec_t;
    const int64_t nq = (rows << k) / V, cm = ((int64_t)1 << k) - 1;
    const int64_t stride = (int64_t)gridDim.x * ROWS_NT;
    for (int64_t q = (int64_t)blockIdx.x * ROWS_NT + threadIdx.x; q < nq; q += stride) {
        const int64_t p = q * V, r = p >> k, c = p & cm;
        if (c >= cols) continue;  // padding only: not read
        vec_t x = reinterpret_cast<const vec_t*>(padded)[q];
        if constexpr (F64) {
#pragma unroll
            for (int j = 0; j < V; ++j) x[j] = (K)f64_of_ord((uint64_t)x[j]);
        }
        K* dst = out + (r * cols + c);
        if constexpr (VEC) {
            *reinterpret_cast<vec_t*>(dst) = x;
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (c + j < cols) dst[j] = x[j];
        }
    }
}

unsigned rows_grid(int64_t nq) {
    const int64_t g = (nq + ROWS_NT - 1) / ROWS_NT;
    return (unsigned)(g < 1 ? 1 : g > ROWS_MAX_GRID ? ROWS_MAX_GRID : g);
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

// the arguments both kernels share; k >= 2 keeps a block a whole number of vectors
bool rows_args_ok(const void* user, const void* padded, int64_t rows, int64_t cols, int k, int key_bytes, bool f64) {
    if (!user || !padded || !aligned16(padded) || (key_bytes != 4 && key_bytes != 8) || (f64 && key_bytes != 8))
        return false;
    return k >= 2 && k <= 62 && cols <= ((int64_t)1 << k) && rows <= (INT64_MAX >> k) / key_bytes;
}

double rows_bytes(int64_t rows, int64_t cols, int k, int key_bytes) {
    return ((double)rows * (double)cols + (double)rows * (double)((int64_t)1 << k)) * key_bytes;
}

template <typename K, bool PAD>
void launch_rows_copy(const void* src, void* dst, int64_t rows, int64_t cols, int k, bool vec, bool f64,
                      hipStream_t s) {
    const unsigned g = rows_grid((rows << k) / RowVec<K>::V);
    const K* a = (const K*)src;
    K* b = (K*)dst;
#define MISORT_ROWS_LAUNCH(VEC_, F64_)                                                      \
    do {                                                                                    \
        if constexpr (PAD) k_pad_rows<K, VEC_, F64_><<<g, ROWS_NT, 0, s>>>(a, b, rows, cols, k); \
        else k_unpad_rows<K, VEC_, F64_><<<g, ROWS_NT, 0, s>>>(a, b, rows, cols, k);        \
    } while (0)
    if constexpr (sizeof(K) == 8) {
        if (vec && f64) MISORT_ROWS_LAUNCH(true, true);
        else if (vec) MISORT_ROWS_LAUNCH(true, false);
        else if (f64) MISORT_ROWS_LAUNCH(false, true);
        else MISORT_ROWS_LAUNCH(false, false);
    } else {
        (void)f64;
        if (vec) MISORT_ROWS_LAUNCH(true, false);
        else MISORT_ROWS_LAUNCH(false, false);
    }
#undef MISORT_ROWS_LAUNCH
}

// ---- key-value rows: the zip fused into the pad sweep, the unzip into the unpad
//
// The padded buffer holds the records K(key) << 32 | value of pairs.hip (K the
// identity or ord_of_f32, applied to real keys only: the padding is the all-ones
// record).  One 16-byte vector of the padded buffer = two records per lane and
// trip; the caller's 32-bit arrays take 8-byte accesses (VEC: every array in use
// 8-byte aligned and cols even, so both elements lie inside one row) or element
// accesses.  vals null: the value of (r, c) is c.  keys null (unpad): values only.
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <bool VEC, bool F32>
__global__ __launch_bounds__(ROWS_NT) void k_pad_rows_pairs(const uint32_t* __restrict__ keys,
                                                            const uint32_t* __restrict__ vals,
                                                            uint64_t* __restrict__ padded, int64_t rows, int64_t cols,
                                                            int k) {
    typedef RowVec<uint64_t>::type vec_t;
    const int64_t nq = (rows << k) / 2, cm = ((int64_t)1 << k) - 1;
    const int64_t stride = (int64_t)gridDim.x * ROWS_NT;
    for (int64_t q = (int64_t)blockIdx.x * ROWS_NT + threadIdx.x; q < nq; q += stride) {
        const int64_t p = q * 2, r = p >> k, c = p & cm;
        const int64_t off = r * cols + c;
        vec_t x = {~(uint64_t)0, ~(uint64_t)0};
        if constexpr (VEC) {
            // cols even: both elements are real or neither
            if (c < cols) {
                const u32x2 kk = *reinterpret_cast<const u32x2*>(keys + off);
                u32x2 vv = {(uint32_t)c, (uint32_t)c + 1u};
                if (vals) vv = *reinterpret_cast<const u32x2*>(vals + off);
#pragma unroll
                for (int j = 0; j < 2; ++j) x[j] = (uint64_t)(F32 ? ord_of_f32(kk[j]) : kk[j]) << 32 | vv[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (c + j < cols) {
                    const uint32_t kk = keys[off + j], vv = vals ? vals[off + j] : (uint32_t)(c + j);
                    x[j] = (uint64_t)(F32 ? ord_of_f32(kk) : kk) << 32 | vv;
                }
        }
        reinterpret_cast<vec_t*>(padded)[q] = x;
    }
}

template <bool VEC, bool F32>
__global__ __launch_bounds__(ROWS_NT) void k_unpad_rows_pairs(const uint64_t* __restrict__ padded,
                                                              uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                              int64_t rows, int64_t cols, int k) {
    typedef RowVec<uint64_t>::type vec_t;
    const int64_t nq = (rows << k) / 2, cm = ((int64_t)1 << k) - 1;
    const int64_t stride = (int64_t)gridDim.x * ROWS_NT;
    for (int64_t q = (int64_t)blockIdx.x * ROWS_NT + threadIdx.x; q < nq; q += stride) {
        const int64_t p = q * 2, r = p >> k, c = p & cm;
        if (c >= cols) continue;  // padding only: not read
        const vec_t x = reinterpret_cast<const vec_t*>(padded)[q];
        const int64_t off = r * cols + c;
        u32x2 kk, vv;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t o = (uint32_t)(x[j] >> 32);
            kk[j] = F32 ? f32_of_ord(o) : o;  // never stored where it is padding
            vv[j] = (uint32_t)x[j];
        }
        if constexpr (VEC) {
            if (keys) *reinterpret_cast<u32x2*>(keys + off) = kk;
            *reinterpret_cast<u32x2*>(vals + off) = vv;
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (c + j < cols) {
                    if (keys) keys[off + j] = kk[j];
                    vals[off + j] = vv[j];
                }
        }
    }
}

bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }  // a null array is not accessed

// k >= 1 keeps a block a whole number of 16-byte vectors
bool rows_pairs_args_ok(const void* padded, int64_t rows, int64_t cols, int k) {
    return padded && aligned16(padded) && k >= 1 && k <= 60 && cols <= ((int64_t)1 << k) &&
           rows <= (INT64_MAX >> k) / 8;
}

}  // namespace

hipError_t pad_rows_pairs(const uint32_t* keys_in, const uint32_t* vals_in, uint64_t* padded, int64_t rows,
                          int64_t cols, int k, bool f32, hipStream_t s, LaunchHook* hook) {
    if (rows <= 0 || cols <= 0) return hipSuccess;
    if (!keys_in || !rows_pairs_args_ok(padded, rows, cols, k)) return hipErrorInvalidValue;
    if (!vals_in && cols > ((int64_t)1 << 32)) return hipErrorInvalidValue;  // a 32-bit value holds 2^32 columns
    const bool vec = aligned8(keys_in) && aligned8(vals_in) && cols % 2 == 0;
    const double n = (double)rows * (double)cols;
    OtherScope os(hook, n * (vals_in ? 8.0 : 4.0) + (double)rows * (double)((int64_t)1 << k) * 8.0, s);
    const unsigned g = rows_grid((rows << k) / 2);
    if (vec && f32) k_pad_rows_pairs<true, true><<<g, ROWS_NT, 0, s>>>(keys_in, vals_in, padded, rows, cols, k);
    else if (vec) k_pad_rows_pairs<true, false><<<g, ROWS_NT, 0, s>>>(keys_in, vals_in, padded, rows, cols, k);
    else if (f32) k_pad_rows_pairs<false, true><<<g, ROWS_NT, 0, s>>>(keys_in, vals_in, padded, rows, cols, k);
    else k_pad_rows_pairs<false, false><<<g, ROWS_NT, 0, s>>>(keys_in, vals_in, padded, rows, cols, k);
    return hipGetLastError();
}

hipError_t unpad_rows_pairs(const uint64_t* padded, uint32_t* keys_out, uint32_t* vals_out, int64_t rows,
                            int64_t cols, int k, bool f32, hipStream_t s, LaunchHook* hook) {
    if (rows <= 0 || cols <= 0) return hipSuccess;
    if (!vals_out || !rows_pairs_args_ok(padded, rows, cols, k)) return hipErrorInvalidValue;
    const bool vec = aligned8(keys_out) && aligned8(vals_out) && cols % 2 == 0;
    const double n = (double)rows * (double)cols;
    OtherScope os(hook, n * 8.0 + n * (keys_out ? 8.0 : 4.0), s);
    const unsigned g = rows_grid((rows << k) / 2);
    if (vec && f32) k_unpad_rows_pairs<true, true><<<g, ROWS_NT, 0, s>>>(padded, keys_out, vals_out, rows, cols, k);
    else if (vec) k_unpad_rows_pairs<true, false><<<g, ROWS_NT, 0, s>>>(padded, keys_out, vals_out, rows, cols, k);
    else if (f32) k_unpad_rows_pairs<false, true><<<g, ROWS_NT, 0, s>>>(padded, keys_out, vals_out, rows, cols, k);
    else k_unpad_rows_pairs<false, false><<<g, ROWS_NT, 0, s>>>(padded, keys_out, vals_out, rows, cols, k);
    return hipGetLastError();
}

hipError_t pad_rows(const void* in, void* padded, int64_t rows, int64_t cols, int k, int key_bytes, bool f64,
                    hipStream_t s, LaunchHook* hook) {
    if (rows <= 0 || cols <= 0) return hipSuccess;
    if (!rows_args_ok(in, padded, rows, cols, k, key_bytes, f64)) return hipErrorInvalidValue;
    const bool vec = aligned16(in) && cols % (16 / key_bytes) == 0;
    OtherScope os(hook, rows_bytes(rows, cols, k, key_bytes), s);
    if (key_bytes == 4) launch_rows_copy<uint32_t, true>(in, padded, rows, cols, k, vec, false, s);
    else launch_rows_copy<uint64_t, true>(in, padded, rows, cols, k, vec, f64, s);
    return hipGetLastError();
}

hipError_t unpad_rows(const void* padded, void* out, int64_t rows, int64_t cols, int k, int key_bytes, bool f64,
                      hipStream_t s, LaunchHook* hook) {
    if (rows <= 0 || cols <= 0) return hipSuccess;
    if (!rows_args_ok(out, padded, rows, cols, k, key_bytes, f64)) return hipErrorInvalidValue;
    const bool vec = aligned16(out) && cols % (16 / key_bytes) == 0;
    OtherScope os(hook, rows_bytes(rows, cols, k, key_bytes), s);
    if (key_bytes == 4) launch_rows_copy<uint32_t, false>(padded, out, rows, cols, k, vec, false, s);
    else launch_rows_copy<uint64_t, false>(padded, out, rows, cols, k, vec, f64, s);
    return hipGetLastError();
}

int rows_plan(int64_t cols, int key_bytes, int* path, int* tile, int* block, int* out, int max) {
    const int lt = tile_log2(key_bytes);
    int k = 0;
    while (k < 62 && ((int64_t)1 << k) < cols) ++k;
    if (cols <= ((int64_t)1 << lt)) {
        // one SORT pass: 2^(tile - block) rows per tile, levels 1..block
        const int lr = k < ROWS_LR_MIN ? ROWS_LR_MIN : k;
        *path = 0;
        *block = lr;
        *tile = key_bytes == 4 && lr < SORT_LT_U32 ? SORT_LT_MERGE : lt;
        if (max > 0) {
            out[0] = KIND_TILE_SORT;
            out[1] = *tile - 1;
            out[2] = out[3] = 0;
        }
        return 1;
    }
    *path = 1;
    *block = k;
    int first[4] = {KIND_TILE_SORT, lt - 1, 0, 0};
    const int np = plan_passes((int64_t)1 << k, key_bytes, max > 0 ? out : first, max > 0 ? max : 1);
    *tile = (max > 0 ? out[1] : first[1]) + 1;
    return np;
}

}  // namespace misort

// rows.hip -- the long-row path of the row-wise sort (gfx950) and its plan.
//
// A row longer than the largest SORT tile is sorted as a block of 2^k records,
// k = ceil_log2(cols): the pad sweep copies every row to the start of its block
// and fills the rest with all-ones, the passes of a 2^k-key local sort run over
// the rows * 2^k records (local_sort's block_log2: every pass merges its groups
// of runs on their own, so every aligned block is sorted), and the unpad sweep
// writes the first cols records of every block back.  The all-ones suffix of a
// block sorts to its end, whatever real records equal it.
//
// A record is what the I/O policies of rows_io.h make of the caller's arrays:
// the key (u32, u64, or ord_of_f64 of an f64 key), or K(key) << 32 | value of a
// key-value pair -- the zip is fused into the pad sweep, the unzip into the
// unpad.  The keys are mapped HERE, in the two sweeps, and the sort between
// them runs on plain u32 or u64: the SORT tile's own f64 load would map the raw
// all-ones padding (a negative NaN pattern) to 0, the smallest key.
//
// Both kernels are HBM-bound and shaped like pairs.hip's: 256 lanes, a capped
// grid that strides over the rest, 64-bit indices, one 16-byte vector of the
// padded buffer per lane and trip: IO::W records, W keys or two pairs.  The
// padded buffer is the context's own and 16-byte aligned; the caller's arrays
// are only known to be element-aligned, so the launchers take the VEC kernel
// when every array in use is aligned to the policy's W-wide access (16 bytes
// for keys, 8 for the 32-bit arrays of pairs) and cols is a multiple of W
// (every slot then lies inside one row), else element accesses on the caller's
// side.
#include <type_traits>

#include "rows_io.h"

namespace misort {

namespace {

constexpr int ROWS_NT = 256;
// one trip per lane up to 2^28 vectors, as the 64-bit pair kernels (pairs.hip)
constexpr int ROWS_MAX_GRID = 1 << 20;

// VEC, and the policy's FLT, are compile-time: as runtime flags of one kernel the
// pad sweep of an argsort's element accesses took 1.10 of the specialised
// kernel's time (profiles/rows_fold/tile_fold_form1_runtime_flags.jsonl).
template <typename IO, bool VEC>
__global__ __launch_bounds__(ROWS_NT) void k_pad_rows(IO io, typename IO::rec_t* __restrict__ padded, int64_t rows,
                                                      int64_t cols, int k) {
    typedef typename IO::rec_t K;
    constexpr int W = IO::W;
    static_assert(W * sizeof(K) == 16, "a slot is one vector of the padded buffer");
    typedef K vec_t __attribute__((ext_vector_type(W)));
    const int64_t nq = (rows << k) / W, cm = ((int64_t)1 << k) - 1;
    const int64_t stride = (int64_t)gridDim.x * ROWS_NT;
    for (int64_t q = (int64_t)blockIdx.x * ROWS_NT + threadIdx.x; q < nq; q += stride) {
        const int64_t p = q * W, r = p >> k, c = p & cm;
        const int64_t off = r * cols + c;
        K x[W];
#pragma unroll
        for (int j = 0; j < W; ++j) x[j] = ~(K)0;
        if constexpr (VEC) {
            // cols % W == 0: the whole slot is real or none of it
            if (c < cols) {
                io.load(off, (uint32_t)c, x);
#pragma unroll
                for (int j = 0; j < W; ++j) x[j] = IO::map(x[j]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j)
                if (c + j < cols) x[j] = IO::map(io.load1(off + j, (uint32_t)(c + j)));
        }
        vec_t v;
#pragma unroll
        for (int j = 0; j < W; ++j) v[j] = x[j];
        reinterpret_cast<vec_t*>(padded)[q] = v;
    }
}

template <typename IO, bool VEC>
__global__ __launch_bounds__(ROWS_NT) void k_unpad_rows(const typename IO::rec_t* __restrict__ padded, IO io,
                                                        int64_t rows, int64_t cols, int k) {
    typedef typename IO::rec_t K;
    constexpr int W = IO::W;
    static_assert(W * sizeof(K) == 16, "a slot is one vector of the padded buffer");
    typedef K vec_t __attribute__((ext_vector_type(W)));
    const int64_t nq = (rows << k) / W, cm = ((int64_t)1 << k) - 1;
    const int64_t stride = (int64_t)gridDim.x * ROWS_NT;
    for (int64_t q = (int64_t)blockIdx.x * ROWS_NT + threadIdx.x; q < nq; q += stride) {
        const int64_t p = q * W, r = p >> k, c = p & cm;
        if (c >= cols) continue;  // padding only: not read
        const vec_t v = reinterpret_cast<const vec_t*>(padded)[q];
        const int64_t off = r * cols + c;
        K x[W];
#pragma unroll
        for (int j = 0; j < W; ++j) x[j] = IO::unmap(v[j]);  // never stored where it is padding
        if constexpr (VEC) {
            io.store(off, x);
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j)
                if (c + j < cols) io.store1(off + j, x[j]);
        }
    }
}

unsigned rows_grid(int64_t nq) {
    const int64_t g = (nq + ROWS_NT - 1) / ROWS_NT;
    return (unsigned)(g < 1 ? 1 : g > ROWS_MAX_GRID ? ROWS_MAX_GRID : g);
}

// The pad sweep into `padded`, or, where it is const, the unpad sweep out of it.
template <typename IO, typename P>
hipError_t launch_sweep(const IO& io, bool vec, P* padded, int64_t rows, int64_t cols, int k, hipStream_t s) {
    typedef typename IO::rec_t K;
    const unsigned g = rows_grid((rows << k) / IO::W);
    if constexpr (std::is_const_v<P>) {
        const K* p = (const K*)padded;
        if (vec) k_unpad_rows<IO, true><<<g, ROWS_NT, 0, s>>>(p, io, rows, cols, k);
        else k_unpad_rows<IO, false><<<g, ROWS_NT, 0, s>>>(p, io, rows, cols, k);
    } else {
        K* p = (K*)padded;
        if (vec) k_pad_rows<IO, true><<<g, ROWS_NT, 0, s>>>(io, p, rows, cols, k);
        else k_pad_rows<IO, false><<<g, ROWS_NT, 0, s>>>(io, p, rows, cols, k);
    }
    return hipGetLastError();
}

// the arguments both keys sweeps share; k >= 2 keeps a block a whole number of vectors
bool rows_args_ok(const void* user, const void* padded, int64_t rows, int64_t cols, int k, int key_bytes, bool f64) {
    if (!user || !padded || !aligned16(padded) || (key_bytes != 4 && key_bytes != 8) || (f64 && key_bytes != 8))
        return false;
    return k >= 2 && k <= 62 && cols <= ((int64_t)1 << k) && rows <= (INT64_MAX >> k) / key_bytes;
}

double rows_bytes(int64_t rows, int64_t cols, int k, int key_bytes) {
    return ((double)rows * (double)cols + (double)rows * (double)((int64_t)1 << k)) * key_bytes;
}

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
    HookScope hs(hook, KIND_OTHER, n * (vals_in ? 8.0 : 4.0) + (double)rows * (double)((int64_t)1 << k) * 8.0, s);
    if (f32) return launch_sweep(RowPairsIO<true>{keys_in, vals_in, nullptr, nullptr}, vec, padded, rows, cols, k, s);
    return launch_sweep(RowPairsIO<false>{keys_in, vals_in, nullptr, nullptr}, vec, padded, rows, cols, k, s);
}

hipError_t unpad_rows_pairs(const uint64_t* padded, uint32_t* keys_out, uint32_t* vals_out, int64_t rows,
                            int64_t cols, int k, bool f32, hipStream_t s, LaunchHook* hook) {
    if (rows <= 0 || cols <= 0) return hipSuccess;
    if (!vals_out || !rows_pairs_args_ok(padded, rows, cols, k)) return hipErrorInvalidValue;
    const bool vec = aligned8(keys_out) && aligned8(vals_out) && cols % 2 == 0;
    const double n = (double)rows * (double)cols;
    HookScope hs(hook, KIND_OTHER, n * 8.0 + n * (keys_out ? 8.0 : 4.0), s);
    if (f32) return launch_sweep(RowPairsIO<true>{nullptr, nullptr, keys_out, vals_out}, vec, padded, rows, cols, k, s);
    return launch_sweep(RowPairsIO<false>{nullptr, nullptr, keys_out, vals_out}, vec, padded, rows, cols, k, s);
}

hipError_t pad_rows(const void* in, void* padded, int64_t rows, int64_t cols, int k, int key_bytes, bool f64,
                    hipStream_t s, LaunchHook* hook) {
    if (rows <= 0 || cols <= 0) return hipSuccess;
    if (!rows_args_ok(in, padded, rows, cols, k, key_bytes, f64)) return hipErrorInvalidValue;
    const bool vec = aligned16(in) && cols % (16 / key_bytes) == 0;
    HookScope hs(hook, KIND_OTHER, rows_bytes(rows, cols, k, key_bytes), s);
    if (key_bytes == 4)
        return launch_sweep(RowKeysIO<uint32_t, false>{(const uint32_t*)in, nullptr}, vec, padded, rows, cols, k,
                            s);
    const uint64_t* in64 = (const uint64_t*)in;
    if (f64) return launch_sweep(RowKeysIO<uint64_t, true>{in64, nullptr}, vec, padded, rows, cols, k, s);
    return launch_sweep(RowKeysIO<uint64_t, false>{in64, nullptr}, vec, padded, rows, cols, k, s);
}

hipError_t unpad_rows(const void* padded, void* out, int64_t rows, int64_t cols, int k, int key_bytes, bool f64,
                      hipStream_t s, LaunchHook* hook) {
    if (rows <= 0 || cols <= 0) return hipSuccess;
    if (!rows_args_ok(out, padded, rows, cols, k, key_bytes, f64)) return hipErrorInvalidValue;
    const bool vec = aligned16(out) && cols % (16 / key_bytes) == 0;
    HookScope hs(hook, KIND_OTHER, rows_bytes(rows, cols, k, key_bytes), s);
    if (key_bytes == 4)
        return launch_sweep(RowKeysIO<uint32_t, false>{nullptr, (uint32_t*)out}, vec, padded, rows, cols, k, s);
    uint64_t* out64 = (uint64_t*)out;
    if (f64) return launch_sweep(RowKeysIO<uint64_t, true>{nullptr, out64}, vec, padded, rows, cols, k, s);
    return launch_sweep(RowKeysIO<uint64_t, false>{nullptr, out64}, vec, padded, rows, cols, k, s);
}

int rows_plan(int64_t cols, int key_bytes, int* path, int* tile, int* block, int* out, int max) {
    const int lt = tile_log2(key_bytes);
    const int k = ceil_log2(cols);
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

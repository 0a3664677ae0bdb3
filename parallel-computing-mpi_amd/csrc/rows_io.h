// rows_io.h -- what one slot of the pad and unpad sweeps of the long-row path
// (rows.hip) reads and writes on the caller's side.
//
// A sweep works on records of the policy's rec_t (u32 or u64): one 16-byte
// vector of the padded buffer is W records.  It hands a policy the element
// offset r cols + c of a slot of W consecutive columns of one row.  load/store
// move the slot as
// W raw records (the sweep takes them where every array in use is aligned to
// the W-wide access and cols is a multiple of W, so every slot lies inside one
// row, aligned), load1/store1 one element otherwise.  map/unmap take a raw
// record to the one that sorts and back; FLT: the keys are IEEE floats, ordered
// through ord_of_f64 or ord_of_f32.  The sweeps map real records only: mapped,
// the all-ones padding would be a small key.  Passed to the kernels by value.
//
// The row tiles (rows_tile.h, rows_pairs.hip) do not use these policies: folded
// onto one kernel over them, the tiles measured slower (profiles/rows_fold).
#pragma once
#include "kernels.h"

namespace misort {

namespace {

// Keys alone: the record is the key, W keys are one 16-byte vector.  FLT (u64
// only): IEEE double bits in the arrays.
template <typename K, bool FLT>
struct RowKeysIO {
    static_assert(!FLT || sizeof(K) == 8, "float keys of the keys-only sorts are f64");
    typedef K rec_t;
    static constexpr int W = 16 / (int)sizeof(K);
    typedef K vec_t __attribute__((ext_vector_type(W)));
    const K* in;
    K* out;

    __device__ __forceinline__ void load(int64_t off, uint32_t, K (&x)[W]) const {
        const vec_t v = *reinterpret_cast<const vec_t*>(in + off);
#pragma unroll
        for (int j = 0; j < W; ++j) x[j] = v[j];
    }
    __device__ __forceinline__ K load1(int64_t off, uint32_t) const { return in[off]; }
    static __device__ __forceinline__ K map(K x) {
        if constexpr (FLT) return (K)ord_of_f64(x);
        else return x;
    }
    static __device__ __forceinline__ K unmap(K r) {
        if constexpr (FLT) return (K)f64_of_ord(r);
        else return r;
    }
    __device__ __forceinline__ void store(int64_t off, const K (&x)[W]) const {
        vec_t v;
#pragma unroll
        for (int j = 0; j < W; ++j) v[j] = x[j];
        *reinterpret_cast<vec_t*>(out + off) = v;
    }
    __device__ __forceinline__ void store1(int64_t off, K x) const { out[off] = x; }
};

// (32-bit key, 32-bit value) pairs: the raw record is key << 32 | value, the
// mapped one K(key) << 32 | value of pairs.hip, K the identity or (FLT)
// ord_of_f32; records exist in registers and in the padded buffer only.  Two
// pairs are one vector of the padded buffer: 8-byte accesses on the 32-bit
// arrays.  vals_in null: the value of column c is the low 32 bits of c (the
// stable argsort of the row; c reaches 2^32 - 1).  keys_out null: values only.
template <bool FLT>
struct RowPairsIO {
    typedef uint64_t rec_t;
    static constexpr int W = 2;
    typedef uint32_t vec_t __attribute__((ext_vector_type(W)));
    const uint32_t *keys_in, *vals_in;
    uint32_t *keys_out, *vals_out;

    __device__ __forceinline__ void load(int64_t off, uint32_t c, uint64_t (&x)[W]) const {
        const vec_t k = *reinterpret_cast<const vec_t*>(keys_in + off);
        vec_t v = {c, c + 1u};
        if (vals_in) v = *reinterpret_cast<const vec_t*>(vals_in + off);
#pragma unroll
        for (int j = 0; j < W; ++j) x[j] = (uint64_t)k[j] << 32 | v[j];
    }
    __device__ __forceinline__ uint64_t load1(int64_t off, uint32_t c) const {
        return (uint64_t)keys_in[off] << 32 | (vals_in ? vals_in[off] : c);
    }
    static __device__ __forceinline__ uint64_t map(uint64_t x) {
        if constexpr (FLT) return (uint64_t)ord_of_f32((uint32_t)(x >> 32)) << 32 | (uint32_t)x;
        else return x;
    }
    static __device__ __forceinline__ uint64_t unmap(uint64_t r) {
        if constexpr (FLT) return (uint64_t)f32_of_ord((uint32_t)(r >> 32)) << 32 | (uint32_t)r;
        else return r;
    }
    __device__ __forceinline__ void store(int64_t off, const uint64_t (&x)[W]) const {
        const vec_t k = {(uint32_t)(x[0] >> 32), (uint32_t)(x[1] >> 32)}, v = {(uint32_t)x[0], (uint32_t)x[1]};
        if (keys_out) *reinterpret_cast<vec_t*>(keys_out + off) = k;
        *reinterpret_cast<vec_t*>(vals_out + off) = v;
    }
    __device__ __forceinline__ void store1(int64_t off, uint64_t x) const {
        if (keys_out) keys_out[off] = (uint32_t)(x >> 32);
        vals_out[off] = (uint32_t)x;
    }
};

}  // namespace

}  // namespace misort

/*
 * misort.h -- C-ABI of the MI355X-native bitonic sort (libmisort.so).
 *
 * Drop-in boundary for the hot path of masrul/Parallel-Computing-MPI's
 * Parallel-Sorting/src/psort.cc.  The reference has no FFI: its swappable unit
 * is the C++ function
 *
 *     double* parallel_bitonic_sort(double* buffer, int& loc_buf_size,
 *                                   int max_size);              // psort.cc:167
 *
 * driven by the globals numprocs/myid of MPI_COMM_WORLD (psort.cc:107,535-536),
 * with compare_split_{max,min} (psort.cc:116-164) exchanging whole blocks over
 * MPI_Sendrecv.  Here ranks are GPUs (one process per GPU), the communicator is
 * RCCL over xGMI, and keys live in HBM.  All entry points are extern "C", take
 * plain pointers and sizes, return 0 on success or a negative MISORT_E_* code
 * (message via misort_last_error()), and never throw.  A context is not
 * thread-safe; use one per thread/GPU.  Nor is it stream-safe: a context's
 * scratch buffers are shared by all its calls, whatever stream they are given.
 * Calls on one stream need nothing, they run in the order they were made.
 * Calls on different streams of one context must be ordered by the caller, with
 * an event or a wait, so that one has finished on the device before the next
 * starts; unordered calls on two streams of one context are undefined.
 *
 * Device pointers are HIP device addresses on the context's GPU.  `stream` is a
 * hipStream_t (NULL = the context's own stream); calls are asynchronous on it
 * unless stated otherwise: a call may be queued behind work that has not run
 * yet, every step of it (kernels, copies, conversions) is ordered on `stream`,
 * and what follows it on `stream` sees its result.  A call that grows one of
 * the context's scratch buffers (the first of its size) may wait for the device.
 */
#ifndef MISORT_H
#define MISORT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MISORT_VERSION 1

/* Key types.  F64 keys are IEEE doubles compared as doubles (psort.cc sorts
 * double); they are sorted as order-preserving 64-bit patterns, so results are
 * bit-exact with the reference except for mixtures of -0.0/+0.0 or NaNs, whose
 * relative order std::sort leaves unspecified.  Documented deviation, measured
 * against the compiled reference (tests/golden/make_golden_f64zero.py, 1000
 * zeros of each sign among 4002 doubles, P = 1, 2, 4, 8): the reference writes
 * its zeros in an introsort-dependent sign order (487-515 sign changes), this
 * library writes -0.0 before +0.0 within each rank's block; every position is
 * equal as a double and every non-zero position is bit-exact
 * (tests/test_gpu_parity.py::test_f64_signed_zeros_vs_reference). */
/* MISORT_F32 keys are accepted by the 32-bit key-value entry points only
 * (misort_local_sort_pairs, misort_parallel_sort_pairs); every other entry
 * point, misort_local_sort_pairs64 included, answers MISORT_E_INVALID for it
 * (64-bit keys with a payload, MISORT_U64 and MISORT_F64, go through
 * misort_local_sort_pairs64).  Their order is the total order of
 * the mapped 32-bit patterns (sign set: all bits inverted; else the sign bit
 * set): -0.0 sorts before +0.0, negative NaNs sort first and positive NaNs
 * last, and every output key is bit-identical to an input key. */
enum misort_dtype { MISORT_U32 = 0, MISORT_U64 = 1, MISORT_F64 = 2, MISORT_F32 = 3 };

enum misort_status {
    MISORT_OK = 0,
    MISORT_E_INVALID = -1,   /* bad argument */
    MISORT_E_NOT_POW2 = -2,  /* psort.cc:168-172 "bitonic sort requires 2^d processors" */
    MISORT_E_HIP = -3,       /* HIP runtime error */
    MISORT_E_RCCL = -4,      /* RCCL error */
    MISORT_E_NO_COMM = -5,   /* communicator not initialised */
    MISORT_E_CAPACITY = -6,  /* a partner block exceeds max_size (MPI_Sendrecv truncation) */
    MISORT_E_INTERNAL = -7   /* a merge pass rejected its own chunk bounds (a planning bug: the
                                output is incomplete); reported by the call itself where it
                                syncs (misort_sort_host), else at the next host sync of the
                                same stream: misort_synchronize for the context's own stream,
                                misort_check_sort for the stream it is given (a sort on a
                                caller's stream is reported there, not by misort_synchronize) */
};

/* Kernel families reported by the per-launch profiler. */
enum misort_kernel_kind {
    MISORT_K_TILE_SORT = 0,   /* levels 1..LT in one LDS tile            */
    MISORT_K_GLOBAL = 1,      /* retired (round 3): network ROWS pass    */
    MISORT_K_TILE_MERGE = 2,  /* retired (round 3): network merge pass   */
    MISORT_K_MERGE_SPLIT = 3, /* device compare-split (psort.cc:116-164) */
    MISORT_K_OTHER = 4,
    MISORT_K_SPAN = 5,        /* retired (round 3): network SPAN pass    */
    MISORT_K_WIDE = 6,        /* retired (round 3): network wide pass    */
    MISORT_K_RUN_MERGE = 7,   /* one merge level: runs 2^hi -> 2^(hi+1)  */
    MISORT_K_EXCHANGE = 8,    /* compare-split exchange leg (splitter samples, RCCL
                                 send/recv, codec), device time between events */
    MISORT_K_RUN_MERGE4 = 9,  /* a multi-way pass: lk merge levels, runs 2^hi -> 2^(hi+lk) */
    MISORT_K_RUN_MERGEK_KERNEL = 10, /* the merge kernel of a multi-way pass alone (its planning
                                        kernels excluded; nested in MISORT_K_RUN_MERGE4) */
    MISORT_K_MERGE_SPLIT_TAIL = 11  /* in-place compare-split of a small bracket
                                       (misort_merge_split_tail); its bytes are an UPPER bound,
                                       2 nblock + min(nblock, nrecv) keys: the device finds the
                                       window it rewrites */
};

typedef struct misort_ctx misort_ctx;

int misort_version(void);
const char* misort_last_error(void);

/* Context on HIP device `device`: selects it, creates a non-blocking stream and
 * grows scratch buffers on demand.  Replaces MPI_Init's per-process setup. */
int misort_create(int device, misort_ctx** out);
int misort_destroy(misort_ctx* ctx);
/* hipStream_t of the context (as void*). */
void* misort_stream(misort_ctx* ctx);
/* Waits for the context's own stream (not a caller's stream) and reports a
 * merge pass's rejected chunk on it (MISORT_E_INTERNAL).  With a communicator,
 * a wait that follows transport calls is bounded by MISORT_TIMEOUT_S (default
 * 120 s; a deadline aborts the communicator, MISORT_E_RCCL); a wait on local
 * work only is not. */
int misort_synchronize(misort_ctx* ctx);

/* ---- communicator (replaces MPI_COMM_WORLD, psort.cc:107,535-536) -------- */
#define MISORT_UNIQUE_ID_BYTES 128
/* Rank 0 creates the id (ncclGetUniqueId) and ships it to all ranks by any
 * host channel (MPI_Bcast, torch.distributed, a file). */
int misort_get_unique_id(void* id /* MISORT_UNIQUE_ID_BYTES */);
/* Collective over all nranks processes: ncclCommInitRank. nranks must be a
 * power of two (else MISORT_E_NOT_POW2, the reference's abort condition). */
int misort_comm_init(misort_ctx* ctx, int nranks, int rank, const void* id);
/* In-process rank group: P ranks as P threads of one process, each with its own
 * context (on the same or different GPUs).  The exchange is a device-to-device
 * copy ordered by HIP events; the schedule, sizes and merge-split path are the
 * same as over RCCL.  Used to run the P-rank path on one GPU (tests) and to
 * drive several GPUs from one process. */
typedef struct misort_group misort_group;
int misort_group_create(int nranks, misort_group** out);
int misort_group_destroy(misort_group* g);
int misort_comm_init_group(misort_ctx* ctx, misort_group* g, int rank);
int misort_comm_size(misort_ctx* ctx);  /* numprocs */
int misort_comm_rank(misort_ctx* ctx);  /* myid */
/* psort.cc:182-196 stage schedule of `rank` in a `p`-rank hypercube: partner
 * and keep-max flag per stage (arrays of >= 64 entries); returns the stage
 * count d(d+1)/2 or a negative status.  Pure host logic. */
int misort_bitonic_schedule(int p, int rank, int* partner, int* keep_max);
/* psort.cc:556-562 block size of `rank` for n keys over p ranks. */
int64_t misort_block_size(int64_t n, int p, int rank);

/* ---- the hot path ------------------------------------------------------- */

/* psort.cc:167 parallel_bitonic_sort over the context's communicator (a
 * single rank without misort_comm_init).  d_keys holds loc_size keys of this
 * rank's block (capacity >= loc_size); on return it holds the rank's block of
 * the result -- the same block the reference leaves in its returned buffer,
 * including the reference's output for uneven blocks.  max_size bounds every
 * rank's block (psort.cc:557, the MPI_Sendrecv receive capacity); it is checked
 * collectively (every rank against the smallest max_size, so all ranks fail
 * together), and max_size <= 0 means the largest block.  Steps: local sort
 * (psort.cc:175) then d(d+1)/2 rounds of RCCL send/recv with the partner plus a
 * device merge-split.  At P = 1 everything is enqueued on `stream`; at P > 1
 * the host waits on the stream at the start (size exchange) and once per
 * stage: the exchange count k is computed on the device from the swapped
 * splitter samples, the encoder takes it from device memory, and the ranks'
 * (coded, raw) message sizes -- which carry k -- are exchanged from device
 * memory; the host reads them once to size the RCCL send/recv.  Without the
 * codec (MISORT_COMPRESS=0) k is computed on the host: two waits per stage. */
int misort_parallel_bitonic_sort(misort_ctx* ctx, int dtype, void* d_keys, int64_t loc_size,
                                 int64_t max_size, void* stream);
/* Same, out of place: d_in is left unchanged, d_out receives the block
 * (d_in == d_out allowed).
 *
 * Buffer contract (both forms).  The arrays need element alignment only (4
 * bytes for u32, 8 for u64 / f64): the local sort of an array that is not
 * 16-byte aligned goes through an aligned buffer of the context (see
 * misort_local_sort); the stages after it (splitter samples, codec,
 * merge-split, the f64 back-conversion) use scalar or alignment-tolerant
 * accesses.  Exactly the loc_size keys of the block are written: with a
 * capacity larger than the block, [loc_size, capacity) is left unchanged, as is
 * everything outside the array; the out-of-place form leaves d_in unchanged.
 *
 * Exchange volume: before each compare-split the partners swap splitter
 * samples (every S-th key, S = max(256, n/32768)) and both derive the same
 * lower bound of the merge-path crossing point, so each side sends only the
 * keys that can cross (the min side its top k, the max side its bottom k)
 * instead of the whole block.  The kept multisets -- hence the bytes of the
 * result -- are exactly those of the reference's whole-block MPI_Sendrecv.
 * MISORT_FULL_EXCHANGE=1 (or misort_set_full_exchange) restores whole-block
 * exchange. */
int misort_parallel_bitonic_sort_oop(misort_ctx* ctx, int dtype, const void* d_in, void* d_out,
                                     int64_t loc_size, int64_t max_size, void* stream);

/* psort.cc:175 local ascending sort of n keys on one GPU, d_in -> d_out.
 *
 * Buffer contract.  Exactly d_out[0, n) is written; d_in is left unchanged
 * unless it is d_out.  d_in == d_out sorts in place; any other overlap of
 * [d_in, d_in + n) and [d_out, d_out + n) is MISORT_E_INVALID, checked by
 * address range before anything is launched (the passes of one sort read and
 * write both arrays from different workgroups).
 *
 * Alignment: the element's (4 bytes for u32, 8 for u64 / f64).  The kernels of
 * the sort that take 16-byte vector accesses through a caller's pointer are the
 * SORT tile (loads of d_in, stores of its output), the 2-way merge pass (stores
 * of full tiles) and the multi-way merge pass (stores of whole vectors; its
 * bounds search also loads aligned lines, behind an alignment test).  Their
 * loads of the runs they merge, the partition and fence kernels and the f64
 * back-conversion sweep are scalar.  None of the vector kernels is handed a
 * pointer that is not 16-byte aligned: such a d_out is sorted into a buffer the
 * context keeps (n keys, grown on demand) and copied out on `stream`; such a
 * d_in is first copied into the destination and sorted in place there.  16-byte
 * aligned arrays launch exactly what they launched before this rule existed. */
int misort_local_sort(misort_ctx* ctx, int dtype, const void* d_in, void* d_out, int64_t n,
                      void* stream);

/* ---- key-value sort (extension; the reference sorts bare keys) -------------- */

/* Key-value sort on one GPU, 32-bit keys.  key_dtype MISORT_U32 or MISORT_F32
 * (MISORT_U64 / MISORT_F64: MISORT_E_INVALID here, see misort_local_sort_pairs64
 * below); values are u32.
 * Output: the n pairs ascending by (key, value), values compared unsigned.
 * d_vals_in == NULL: the value of element i is i, so d_vals_out is the STABLE
 * argsort of the keys (n <= 2^32).  d_keys_out == NULL: values only.
 * Outputs may alias the corresponding inputs.  Asynchronous on `stream`.
 *
 * The pairs are sorted as 64-bit records (key << 32) | value through the path
 * of misort_local_sort(MISORT_U64): the context keeps a record buffer and the
 * sort's ping-pong buffer, 16 bytes per pair on top of the caller's arrays.
 * The key and value arrays need 4-byte alignment only; 16-byte aligned ones
 * take the faster vector kernels. */
int misort_local_sort_pairs(misort_ctx* ctx, int key_dtype, const void* d_keys_in, const void* d_vals_in,
                            void* d_keys_out, void* d_vals_out, int64_t n, void* stream);

/* Key-value sort on one GPU, 64-bit keys.  key_dtype MISORT_U64 or MISORT_F64
 * (anything else: MISORT_E_INVALID); val_bytes is 4 or 8, values are opaque
 * bit patterns.  Output: the n pairs ascending by key, EQUAL KEYS IN INPUT
 * ORDER: a stable sort by key.  This differs from misort_local_sort_pairs'
 * "(key, value)" order, because here the value is not part of a compared
 * record: a 64-bit key leaves no room for it in the u64 records the sort moves,
 * so the records carry the element's index and the values are gathered by it
 * at the end.  f64 keys sort as misort_local_sort(MISORT_F64) sorts them:
 * -0.0 before +0.0, negative NaNs first, positive NaNs last, and every output
 * key is bit-identical to an input key (NaN payloads included).
 * d_vals_in == NULL: d_vals_out receives n u32 indices, the stable argsort of
 * the keys; val_bytes must then be 4.  d_keys_out == NULL: values or indices
 * only.  0 <= n <= 2^32 (n == 0 launches nothing and looks at no pointer); d_keys_in and d_vals_out
 * must be non-null for n > 0.  Asynchronous on `stream`.
 *
 * How: K(key), the order-preserving 64-bit pattern, is sorted as two halves,
 * least significant first, each as distinct u64 records (half << 32 | 32-bit
 * tag) through the path of misort_local_sort(MISORT_U64): first
 * (lo(K) << 32 | i), then (hi(K) << 32 | rank of the first sort); a last
 * kernel follows the two tags back to i and writes index, key and value.
 * Scratch: two record buffers and the sort's ping-pong buffer, 24 bytes per
 * pair on top of the caller's arrays, kept by the context.
 *
 * Aliasing: d_keys_out may be d_keys_in (the keys are last read before the
 * second sort).  No output may overlap d_vals_in (the last kernel gathers from
 * it while it writes), and d_keys_out must not overlap d_vals_out: both are
 * checked by address range, MISORT_E_INVALID.  Keys need 8-byte alignment,
 * values and indices their element's; 16-byte aligned arrays take the faster
 * vector kernels. */
int misort_local_sort_pairs64(misort_ctx* ctx, int key_dtype, const void* d_keys_in, const void* d_vals_in,
                              int val_bytes, void* d_keys_out, void* d_vals_out, int64_t n, void* stream);

/* misort_local_sort_pairs over the context's communicator, 32-bit keys only
 * (there is no multi-rank sort of 64-bit keys with a payload: MISORT_U64 and
 * MISORT_F64 are MISORT_E_INVALID here).  Hypercube schedule, bracketed coded
 * exchange, relay: the records travel as MISORT_U64 keys through the path of
 * misort_parallel_bitonic_sort.  Rank r ends with pairs [r*loc, (r+1)*loc) of
 * the global (key, value) order.  Every rank must pass the same loc_size:
 * checked collectively, all ranks return MISORT_E_INVALID together otherwise
 * (with unequal blocks psort.cc's compare-split keeps a rank's own count, so
 * records would be duplicated or lost: tolerable for bare keys as the
 * reference's documented defect, not for payloads).  d_vals_in == NULL: the
 * value is the global index rank*loc + i (nranks*loc <= 2^32).  max_size as in
 * misort_parallel_bitonic_sort.  Not asynchronous: at P > 1 the host waits on
 * `stream` as misort_parallel_bitonic_sort does, and a caller must not rely on
 * its returning early at P = 1. */
int misort_parallel_sort_pairs(misort_ctx* ctx, int key_dtype, const void* d_keys_in, const void* d_vals_in,
                               void* d_keys_out, void* d_vals_out, int64_t loc_size, int64_t max_size,
                               void* stream);

/* ---- row-wise sort (extension; the reference sorts one array) ---------------- */

/* Sorts every row of a row-major rows x cols array ascending, independently:
 * d_out[r*cols .. r*cols+cols) = sorted d_in[r*cols .. r*cols+cols).
 * dtype MISORT_U32, MISORT_U64 or MISORT_F64 (MISORT_F32: MISORT_E_INVALID); f64
 * keys sort as misort_local_sort(MISORT_F64) sorts them: -0.0 before +0.0,
 * negative NaNs first, positive NaNs last.  Every output key is bit-identical
 * to an input key.  Rows are contiguous, row stride cols.  The arrays need
 * element alignment only (a view one element into its storage, odd cols);
 * 16-byte aligned ones whose cols is a multiple of 16 bytes of keys take the
 * vector kernels.  d_out == d_in is allowed; any other overlap of the two
 * rows*cols ranges is MISORT_E_INVALID, checked by address range before
 * anything is launched.  rows == 0 or cols == 0 launches nothing and looks at
 * no pointer; cols == 1 is a copy (nothing when in place).  MISORT_E_INVALID for
 * negative sizes, a null context, or a null array with rows*cols > 0.
 * Asynchronous on `stream`; a merge pass's rejected chunk (MISORT_E_INTERNAL)
 * is reported by misort_synchronize, as for misort_local_sort.
 *
 * How (misort_rows_plan tells which):
 *   cols <= 2^misort_tile_log2 (u32 2^15, u64/f64 2^13): ONE pass, one HBM read
 *     and one write per key.  A SORT tile of 2^LT keys holds 2^(LT-LR) rows
 *     padded virtually to 2^LR >= cols keys (LR >= 5: a row of up to 32 keys is
 *     one lane's registers) and runs the network's levels 1..LR only.  No
 *     scratch.
 *   longer rows: every row is copied to a block of 2^k keys, k = ceil_log2(cols),
 *     filled up with all-ones; the passes of a 2^k-key misort_local_sort run
 *     over all rows*2^k keys, sorting every block on its own; the first cols
 *     keys of every block are copied out.  Scratch kept by the context and
 *     grown on demand: two buffers of rows*2^k keys, up to 4x the input's
 *     bytes; just above a power of two the sort does up to 2x the work of
 *     rows*cols keys. */
int misort_local_sort_rows(misort_ctx* ctx, int dtype, const void* d_in, void* d_out,
                           int64_t rows, int64_t cols, void* stream);

/* Row-wise key-value sort, 32-bit keys: every row of the row-major rows x cols
 * arrays d_keys_in / d_vals_in is sorted on its own, ascending by (key, value),
 * values compared unsigned: exactly the order of misort_local_sort_pairs, row by
 * row.  key_dtype MISORT_U32 or MISORT_F32 (anything else: MISORT_E_INVALID;
 * 64-bit keys would need 128-bit records); values are 32-bit patterns.  f32
 * keys sort in the total order of their bit patterns: -0.0 before +0.0,
 * negative NaNs first, positive NaNs last; every output key is bit-identical to
 * an input key.
 * d_vals_in == NULL: the value of element (r, c) is c, so d_vals_out holds the
 * STABLE row-wise argsort, equal keys in column order (cols <= 2^32).
 * d_keys_out == NULL: no keys are written.  d_keys_in and d_vals_out are
 * required when rows*cols > 0.  rows == 0 or cols == 0 launches nothing and
 * looks at no pointer; cols == 1 copies keys and values (argsort: zeros).
 * MISORT_E_INVALID for negative sizes and a null context (checked first).
 * The arrays need 4-byte alignment only; when every array in use is 16-byte
 * aligned and cols is a multiple of 4 the one-pass kernel takes 16-byte
 * accesses, when 8-byte aligned and cols is even 8-byte ones.  Asynchronous on
 * `stream`; a merge pass's rejected chunk (MISORT_E_INTERNAL) is reported by
 * misort_synchronize, as for misort_local_sort.
 *
 * Aliasing: d_keys_out == d_keys_in and d_vals_out == d_vals_in (the same base
 * pointer) sort in place.  Any other overlap among the four rows*cols*4-byte
 * ranges, the two outputs with each other included, is MISORT_E_INVALID,
 * checked by address range before anything is launched.
 *
 * How (misort_rows_plan(cols, 8) tells which: the pairs travel as the u64
 * records (K(key) << 32) | value of misort_local_sort_pairs):
 *   cols <= 2^13: ONE pass of the u64 row tile of misort_local_sort_rows.  The
 *     record is formed in registers as the tile loads and split as it stores,
 *     so each array element is read once and written once and no record ever
 *     lies in HBM.  No scratch.
 *   longer rows: the padded blocks of misort_local_sort_rows on records.  The
 *     pad sweep forms the records (all-ones above cols), the passes of a
 *     2^k-key u64 sort, k = ceil_log2(cols), run over all rows*2^k records, the
 *     unpad sweep splits the first cols records of every block into the two
 *     outputs.  Scratch kept by the context and grown on demand: two buffers
 *     of rows*2^k*8 bytes. */
int misort_local_sort_rows_pairs(misort_ctx* ctx, int key_dtype,
                                 const void* d_keys_in, const void* d_vals_in,
                                 void* d_keys_out, void* d_vals_out,
                                 int64_t rows, int64_t cols, void* stream);

/* Host only, no device: how a row sort of `cols` keys of key_bytes (4 or 8) runs.
 * *path = 0: in one SORT pass (rows packed into LDS tiles); 1: padded blocks + merge passes.
 * *tile_log2: the SORT tile; *block_log2: log2 of the padded row length;
 * passes: as misort_plan.  Returns the number of passes or a negative status. */
int misort_rows_plan(int64_t cols, int key_bytes, int* path, int* tile_log2, int* block_log2,
                     int* passes, int max_passes);

/* ---- segmented sort (extension) ---------------------------------------------- */

/* Sorts variable-length segments of one array, each ascending on its own.
 * d_offsets is a DEVICE array of nseg + 1 int64 values; segment i is the keys
 * [d_offsets[i], d_offsets[i+1]) of d_in.  Well formed means 0 <= d_offsets[0],
 * d_offsets[i] <= d_offsets[i+1] and d_offsets[nseg] <= n; empty segments are
 * allowed.  dtype MISORT_U32, MISORT_U64 or MISORT_F64 (MISORT_F32:
 * MISORT_E_INVALID); f64 keys sort as misort_local_sort(MISORT_F64) sorts them:
 * -0.0 before +0.0, negative NaNs first, positive NaNs last.  Every output key
 * is bit-identical to an input key.
 *
 * Written range: exactly d_out[0, n).  With d_out != d_in the keys outside
 * [d_offsets[0], d_offsets[nseg]) are copied from d_in, so d_out is a complete
 * result and d_in is left unchanged; in place (d_out == d_in) those keys are not
 * touched.  Any other overlap of the two n-key ranges, and any overlap of d_out
 * with the nseg + 1 offsets, is MISORT_E_INVALID, checked by address range
 * before anything is launched.  The key arrays need element alignment only
 * (segments start anywhere: every access to them is an element access); the
 * offsets need 8-byte alignment.  0 <= nseg <= 2^31 - 1.  n == 0 launches
 * nothing and looks at no pointer; nseg == 0 launches no kernel and looks at no
 * key pointer except for the copy of all n keys when d_out != d_in.
 * MISORT_E_INVALID for a null context (checked first), negative sizes, and a
 * null array that would be read or written.
 *
 * ONE HOST WAIT PER CALL.  A count kernel reads d_offsets[0 .. nseg] (nothing
 * else), validates every segment, and counts segments and keys per class
 * (misort_segment_class) into a small header; the host waits for it and reads
 * the header once (with a communicator the wait is bounded as in
 * misort_synchronize), so that every later launch is sized exactly: a second
 * sweep writes each class's segment list, then one launch per non-empty class.
 * Everything after the wait is asynchronous on `stream`.  Because of the wait
 * the call CANNOT BE CAPTURED IN A GRAPH, and work queued on `stream` before it
 * is waited for.  Malformed offsets are refused there: MISORT_E_INVALID, the
 * message names the first malformed index i (the pair d_offsets[i],
 * d_offsets[i+1]), before any kernel that touches a key is launched: d_out is
 * unchanged.  A merge pass's rejected chunk (MISORT_E_INTERNAL) is reported by
 * misort_synchronize, as for misort_local_sort.
 *
 * How: segments up to 2^misort_tile_log2 keys go through the row tile of
 * misort_local_sort_rows, one launch per class LR = 5 .. tile_log2: a tile holds
 * 2^(LT-LR) segments of lengths in (2^(LR-1), 2^LR] (LR = 5: 1 .. 32), one HBM
 * read and one write per key, no scratch.  Longer segments go class by class,
 * k = ceil_log2(length), through the padded blocks of the long rows: gathered
 * into blocks of 2^k keys filled up with all-ones, sorted by the passes of a
 * 2^k-key misort_local_sort, the first `length` keys of every block written
 * back.  Scratch kept by the context: 4 bytes per segment plus a 2 KiB header,
 * and for the long classes two buffers of max over k (count_k * 2^k) keys. */
int misort_local_sort_segments(misort_ctx* ctx, int dtype, const void* d_in, void* d_out, int64_t n,
                               const int64_t* d_offsets, int64_t nseg, void* stream);

/* Host only, no device: the class of a segment of `len` keys of key_bytes (4 or
 * 8).  -1 for len == 0 (nothing to sort; also the status of a negative len or a
 * bad key_bytes); for 1 <= len <= 2^misort_tile_log2(key_bytes) the row tile's
 * LR = max(ceil_log2(len), 5); for longer segments ceil_log2(len), the k of the
 * padded blocks.  For every len >= 2 it is misort_rows_plan(len, key_bytes)'s
 * path and block size.  The kernels classify with the same function. */
int misort_segment_class(int64_t len, int key_bytes);

/* psort.cc:377-490 parallel_quick_sort (the reference binary's shipped sort,
 * called at psort.cc:647-648): d rounds of median-of-medians pivoting over
 * shrinking hypercube sub-groups, RCCL send/recv with the partner, device merge.
 * Per-rank output sizes are data-dependent, exactly as in the reference:
 * *out_size receives this rank's count; MISORT_E_CAPACITY if it exceeds
 * out_capacity (the reference allocates (loc+1)*P).  d_in is not modified and
 * needs element alignment only (its local sort copies a d_in that is not
 * 16-byte aligned into the context's run buffer first, as misort_local_sort
 * does).  Not asynchronous: at P > 1 the host waits on `stream` several times
 * in every round (the median, the pivot's position and the partner's count are
 * read back), and a caller must not rely on its returning early at P = 1. */
int misort_parallel_quick_sort(misort_ctx* ctx, int dtype, const void* d_in, int64_t loc_size,
                               void* d_out, int64_t out_capacity, int64_t* out_size, void* stream);

/* psort.cc:203-375 parallel_sample_native_sort / parallel_sample_bitonic_sort,
 * redesigned for RCCL over xGMI: local sort, all-gathered regular samples,
 * (key, rank, position) splitters, ONE all-to-all-v (every GPU pair on its
 * own link), a device merge tree, and a rebalancing all-to-all-v into the
 * reference block layout.  Same contract as misort_parallel_bitonic_sort_oop
 * (d_out receives loc_size keys: the globally sorted sequence in the callers'
 * block sizes); d_in != d_out.  The reference's versions are not well defined
 * (an uninitialised splitter at :318, MPI_INT used for doubles at :224/:269),
 * so parity is anchored on the sorted sequence, not on their per-rank sizes.
 * d_in needs element alignment only (handled as in misort_parallel_quick_sort).
 * Not asynchronous: at P > 1 the host waits on `stream` (block sizes, samples
 * and the all-to-all-v counts are read back), and a caller must not rely on its
 * returning early at P = 1. */
int misort_parallel_sample_sort(misort_ctx* ctx, int dtype, const void* d_in, void* d_out,
                                int64_t loc_size, int64_t max_size, void* stream);

/* Device half of compare_split_{max,min} (psort.cc:116-164) without the
 * exchange: d_out[0..nloc) = the nloc largest (keep_max=1) or smallest
 * (keep_max=0) keys of the sorted blocks local U recv, ascending.
 * Exactly d_out[0, nloc) is written; d_local and d_recv are left unchanged.
 * d_out must overlap neither of them (MISORT_E_INVALID, checked by address
 * range: a merge tile reads keys another tile may already have written).  The
 * arrays need element alignment only: the partition and merge kernels take
 * scalar accesses. */
int misort_merge_split(misort_ctx* ctx, int dtype, const void* d_local, int64_t nloc,
                       const void* d_recv, int64_t nrecv, void* d_out, int keep_max,
                       void* stream);

/* The same keep-n merge IN PLACE (psort.cc:116-164, the result replaces
 * d_block): the path a hypercube stage takes when the partner's bracket k is
 * small (k <= nblock / MISORT_TAIL_DIV, default 8): only the end of the block
 * that the nrecv received keys reach is rewritten, staged through the context's
 * work buffer.  d_recv must not overlap d_block (MISORT_E_INVALID).  Nothing
 * outside d_block[0, nblock) is written and d_recv is left unchanged; the
 * arrays need element alignment only (scalar accesses).  Exposed
 * so the path is testable on its own (extension; the reference merges the
 * whole block every stage). */
int misort_merge_split_tail(misort_ctx* ctx, int dtype, void* d_block, int64_t nblock,
                            const void* d_recv, int64_t nrecv, int keep_max, void* stream);

/* psort.cc:497-520 check_sort: local descents of this rank's block plus the
 * boundary descent against rank-1's last key, summed over the communicator.
 * Synchronous; *errors is valid on every rank.  d_keys is only read and needs
 * element alignment only (the counting kernel takes scalar loads); every
 * position i with d_keys[i] > d_keys[i+1] counts exactly once (f64: compared as
 * doubles, so a NaN on either side is no descent). */
int misort_check_sort(misort_ctx* ctx, int dtype, const void* d_keys, int64_t n,
                      int64_t* errors, void* stream);

/* Host-buffer convenience path: h_in -> pinned staging -> device -> sort ->
 * host h_out (this rank's block, parallel sort over the communicator).
 * Synchronous. */
int misort_sort_host(misort_ctx* ctx, int dtype, const void* h_in, void* h_out, int64_t loc_size,
                     int64_t max_size);

/* ---- synthetic input ------------------------------------------------------ */
/* Counter-based SplitMix64 keys of global indices [g0, g0+n):
 * key_g = mix(seed + (g+1)*0x9E3779B97F4A7C15), u32 = top 32 bits. */
int misort_fill_splitmix(misort_ctx* ctx, int dtype, void* d_out, int64_t n, uint64_t seed,
                         int64_t g0, void* stream);

int misort_set_full_exchange(misort_ctx* ctx, int on);

/* Relay each compare-split exchange through the other GPUs (P > 2; default on,
 * env MISORT_RELAY=0 turns it off): every message is cut into P parts, 2 go
 * over the pair's own xGMI link, P-2 take two hops through the other GPUs, so
 * all P-1 links of every GPU carry the stage.  Bytes delivered are identical. */
int misort_set_relay(misort_ctx* ctx, int on);

/* Delta-code the keys of each compare-split message (default on; env
 * MISORT_COMPRESS=0 turns it off).  The k keys one side sends are a sorted
 * run: blocks of 1024 keys travel as first key + gaps packed at the block's
 * bit width (lossless; ~4x smaller for 2^27 uniform u32 keys per rank).  A
 * side whose coded message would not be smaller sends it raw; the receiver
 * tells them apart by size.  Replaces the raw MPI_Sendrecv payload of
 * psort.cc:122-123 / 146-147; the kept keys are unchanged. */
int misort_set_compress(misort_ctx* ctx, int on);

/* Tooling: encode a sorted device run of n keys with the exchange codec,
 * then decode it (into `decoded` if non-null); average ms of each over
 * `reps` launches (HIP events) and the coded size in bytes. */
int misort_codec_probe(misort_ctx* ctx, int dtype, const void* keys, int64_t n, int reps, float* enc_ms,
                       float* dec_ms, int64_t* coded_bytes, void* decoded);

/* Bytes the exchanges since the last call would have moved uncoded (sent +
 * received; the coded bytes are misort_exchange_stats' `bytes`).  Resets. */
int misort_exchange_raw_bytes(misort_ctx* ctx, int64_t* raw_bytes);
/* Host logic of the bracketed exchange (pure functions, no GPU):
 * samples of a sorted block of n keys are keys[min(c*S, n-1)], c = 0..count-1,
 * S = misort_sample_stride(n), count = misort_sample_count(n).
 * misort_exchange_count returns k, the keys each partner sends (the keep-min
 * side its top k, the keep-max side its bottom k), given both sample sets; -1
 * means whole blocks (an empty side).  u64/f64 samples are order-preserving
 * u64 patterns. */
int64_t misort_sample_stride(int64_t n);
int64_t misort_sample_count(int64_t n);
int64_t misort_exchange_count(int dtype, const void* samples_min, int64_t n_min,
                              const void* samples_max, int64_t n_max);
/* Exchange volume since the last call (then reset): compare-split stages,
 * bytes sent+received, and the bytes a whole-block exchange would have moved. */
int misort_exchange_stats(misort_ctx* ctx, int64_t* stages, int64_t* bytes, int64_t* full_bytes);

/* ---- per-launch profiling (HIP events around every kernel launch) ---------- */
int misort_profile_enable(misort_ctx* ctx, int on);
/* Reset accumulated figures. */
int misort_profile_reset(misort_ctx* ctx);
/* Synchronises the stream(s) used, then reports for one kernel kind: launches,
 * summed device time (ms) and summed algorithmic HBM bytes. */
int misort_profile_read(misort_ctx* ctx, int kind, int64_t* launches, double* total_ms,
                        double* bytes);

/* Per hypercube stage of misort_parallel_bitonic_sort (stage 0 .. d(d+1)/2-1,
 * the order of psort.cc:184-185), summed over the profiled sorts: number of
 * sorts, exchange-leg device time (ms), merge-split kernel time (ms) and the
 * bytes this rank sent plus received in the stage. */
int misort_profile_stage(misort_ctx* ctx, int stage, int64_t* count, double* exchange_ms,
                         double* merge_ms, double* exchange_bytes);

/* Every profiled record since the last reset, in completion order (a
 * multi-way pass after the k_mergek launch nested in it): kind, device ms and
 * algorithmic bytes.  Fills up to `max` entries; returns the number recorded
 * (at most 2^20 are kept).  For per-pass roofline figures. */
int misort_profile_trace(misort_ctx* ctx, int max, int* kinds, double* ms, double* bytes);

/* log2 of the LARGEST SORT tile (keys) for a key width of 4 or 8 bytes: every
 * plan's tiles divide it.  The tile a given size actually uses is chosen per
 * size (u32: 2^14 or 2^15); it is the first pass of misort_plan (hi + 1). */
int misort_tile_log2(int key_bytes);

/* The HBM pass plan of a local sort of n keys (key_bytes 4 or 8), for tools
 * and tests: writes up to max_passes entries of 4 ints (kind as
 * misort_kernel_kind, hi, R, flip) and returns the number of passes (or a
 * negative status).  Host-only; no device is touched. */
int misort_plan(int64_t n, int key_bytes, int* passes, int max_passes);

/* Tooling: average device time (ms, HIP events on the context stream) of ONE
 * HBM pass of the given shape (kind MISORT_K_TILE_SORT, MISORT_K_RUN_MERGE or
 * MISORT_K_RUN_MERGE4; hi/R as misort_plan reports them) over n keys,
 * alternating in -> out and out -> in for `reps` launches.  A merge pass
 * assumes ascending runs of 2^hi keys; other input is scrambled, not sorted. */
int misort_pass_probe(misort_ctx* ctx, int dtype, const void* in, void* out, int64_t n, int kind,
                      int hi, int r, int flip, int reps, float* ms);

#ifdef __cplusplus
}
#endif
#endif

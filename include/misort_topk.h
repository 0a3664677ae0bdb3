/*
 * misort_topk.h -- row-wise top-k, an extension header of libmisort.so's C-ABI.
 *
 * Why a header of its own: tests/stream_order.py holds every `void* stream`
 * prototype of misort.h against a fixed table of cases, and this entry point
 * arrived without a case in that table.  Its stream-order contract is pinned
 * by tests/test_gpu_topk.py instead, with the same procedure
 * (behind_pending_work).  A later change can fold this header into misort.h
 * together with a table case.  Everything misort.h says about contexts,
 * streams, status codes and misort_last_error() holds here.
 */
#ifndef MISORT_TOPK_H
#define MISORT_TOPK_H
#include "misort.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Row-wise top-k, 32-bit keys: for every row of the row-major rows x cols array
 * d_keys_in, the k smallest (largest == 0) or largest (largest != 0) keys and
 * their columns: what torch.topk(dim=-1, sorted=True) returns, without sorting
 * the rows.  key_dtype MISORT_U32 or MISORT_F32 (anything else:
 * MISORT_E_INVALID).  f32 keys are compared in the total order of their mapped
 * bit patterns (sign set: all bits inverted; else the sign bit set), as in
 * misort_local_sort_rows_pairs.  For largest that is: positive NaNs first, then
 * +inf ... +0.0, -0.0 ... -inf, then negative NaNs; for smallest the reverse.
 * Every output key is bit-identical to an input key.
 *
 * Outputs: rows x k, row-major and contiguous.  d_idx_out holds the columns as
 * u32 and is required; d_keys_out holds the keys and may be NULL (indices
 * only).  Each row is SORTED, best first: ascending keys for smallest,
 * descending keys for largest.  Equal keys come out in ascending column order
 * in both directions, and of equal keys at the cut the lowest columns are kept.
 *
 * Sizes: 1 <= k <= cols and cols <= 2^31; k <= 2^10 when cols > 2^13 (a larger
 * k of long rows is MISORT_E_INVALID: sort the rows with
 * misort_local_sort_rows_pairs and take the first k columns).  rows == 0
 * launches nothing and looks at no pointer; so does k == 0 with rows, cols >= 0.
 * MISORT_E_INVALID for negative sizes, k > cols, a null context (checked
 * first), and a null d_keys_in or d_idx_out.
 *
 * Overlap: NO output may overlap the input or the other output (in place is
 * meaningless here): MISORT_E_INVALID, checked by address range before anything
 * is launched.  The input is left unchanged, and exactly rows*k elements of
 * each output are written.  The arrays need 4-byte alignment only; a 16-byte
 * aligned d_keys_in with cols a multiple of 4 is read with 16-byte loads.
 *
 * Asynchronous on `stream`, with no host wait: every launch is on `stream`.  A
 * call that grows the context's scratch may wait for the device, as misort.h
 * says for all calls.
 *
 * How (misort_topk_plan tells the passes): both directions sort ascending u64
 * records T(key) << 32 | column, T the mapped key for smallest and its
 * complement for largest, in the u64 row tile of misort_local_sort_rows_pairs;
 * the records are formed in registers and never sorted as a whole row.
 *   cols <= 2^13: ONE pass.  A tile of 2^13 records holds 2^(13-LR) rows padded
 *     virtually to 2^LR >= cols records, LR >= 5; the first k records of every
 *     row are split into the outputs.  No scratch.
 *   longer rows: the first pass sorts every piece of 2^13 keys of a row in one
 *     tile and writes its first k records: npieces*k candidates per row,
 *     npieces = ceil(cols / 2^13).  While a row has more than 2^13 candidates, a
 *     pass of the same shape over the candidates follows; the last pass sorts
 *     one block per row and splits its first k records into the outputs.  The
 *     input is read once; no merge pass runs.  Scratch, kept by the context
 *     (the buffers of the long-row sorts) and grown on demand: two candidate
 *     buffers of at most rows*npieces*k*8 bytes, about 1/4 of the input's bytes
 *     at the most. */
int misort_local_topk_rows(misort_ctx* ctx, int key_dtype, const void* d_keys_in,
                           void* d_keys_out, void* d_idx_out, int64_t rows, int64_t cols,
                           int64_t k, int largest, void* stream);

/* Host only, no device: the passes misort_local_topk_rows runs for rows of
 * `cols` keys and `k`.  Writes up to max_passes passes (`passes` may be NULL when
 * max_passes is 0) as 4 ints each:
 *   m_in     records of a row the pass reads (the first pass: cols; 2^31 is
 *            stored as its unsigned 32-bit pattern);
 *   LR       log2 virtual records of a block, 5..13;
 *   npieces  blocks per row, ceil(m_in / 2^LR); 1 in the last pass only;
 *   m_out    records of a row the pass leaves, npieces*k (the last pass: k).
 * Returns the number of passes (at most 7), or MISORT_E_INVALID for a (cols, k)
 * that misort_local_topk_rows refuses, k == 0 included. */
int misort_topk_plan(int64_t cols, int64_t k, int* passes, int max_passes);  /* host only */

#ifdef __cplusplus
}
#endif
#endif /* MISORT_TOPK_H */

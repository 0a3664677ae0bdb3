/*
 * misort_topk_segments.h -- segmented top-k, an extension header of
 * libmisort.so's C-ABI.
 *
 * Why a header of its own: tests/stream_order.py holds every `void* stream`
 * prototype of misort.h against a fixed table of cases, and this entry point
 * arrived without a case in that table (the situation misort_topk.h and
 * misort_segments_pairs.h describe).  Its stream-order contract is pinned by
 * tests/test_gpu_topk_segments.py instead, with the same procedure
 * (behind_pending_work).  A later change can fold this header into misort.h
 * together with a table case.  Everything misort.h says about contexts,
 * streams, status codes and misort_last_error() holds here.
 */
#ifndef MISORT_TOPK_SEGMENTS_H
#define MISORT_TOPK_SEGMENTS_H
#include "misort.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Segmented top-k, 32-bit keys: for every segment of d_keys_in the k smallest
 * (largest == 0) or largest (largest != 0) keys and their positions inside the
 * segment, without sorting the segments.  d_offsets is a DEVICE array of
 * nseg + 1 int64 values, exactly that of misort_local_sort_segments: segment i
 * is the keys [d_offsets[i], d_offsets[i+1]) of the n-key array; well formed
 * means 0 <= d_offsets[0], d_offsets[i] <= d_offsets[i+1] and d_offsets[nseg]
 * <= n; empty segments are allowed and keys outside the segments are ignored.
 * key_dtype MISORT_U32 or MISORT_F32 (anything else: MISORT_E_INVALID).
 *
 * Order: that of misort_local_topk_rows.  Both directions sort ascending
 * records T(key) << 32 | position, T = K for smallest and T = ~K for largest, K
 * the identity or (f32) the order-preserving pattern (sign set: all bits
 * inverted; else the sign bit set).  Each row is SORTED, best first; equal keys
 * come out in ascending position order in both directions, and of equal keys at
 * the cut the lowest positions are kept.  Every real output key is
 * bit-identical to an input key.
 *
 * Outputs: nseg x k, row-major and dense; row i belongs to segment i.
 * d_idx_out is required and holds u32 positions inside the segment (the
 * positions misort_local_sort_segments_pairs' argsort returns); d_keys_out
 * holds the keys and may be NULL.  Exactly nseg*k elements of each output in
 * use are written.
 *
 * Segments shorter than k, empty ones included: slots j >= len of the row hold
 * the unmapped all-ones record.  The index there is 0xFFFFFFFF (-1 in int32
 * storage); a real position is below 2^31, so this index is never real and
 * marks absence.  The key there is the last key of the direction's order:
 *
 *     key type   direction   fill key
 *     u32        smallest    0xFFFFFFFF
 *     u32        largest     0
 *     f32        smallest    pattern 0x7FFFFFFF
 *     f32        largest     pattern 0xFFFFFFFF
 *
 * A real key may equal the fill key; only the index tells.
 *
 * Sizes: 0 <= nseg <= 2^31 - 1, 0 <= n <= INT64_MAX >> 5, 1 <= k <= 2^13;
 * k <= 2^10 if any segment is longer than 2^13 keys, and no segment may be
 * longer than 2^31 keys.  The last two are known only after the count kernel:
 * they are refused there, at the call's one host wait, together with malformed
 * offsets (MISORT_E_INVALID, "nothing was written").  k == 0 or nseg == 0
 * launches nothing and looks at no pointer.  n == 0 with nseg > 0 is a normal
 * call: the offsets are validated (all zero) and every row is filled;
 * d_keys_in may be NULL then.  MISORT_E_INVALID for a null context (checked
 * first), negative sizes, k > 2^13, and a null d_idx_out, d_offsets or (n > 0)
 * d_keys_in.
 *
 * Overlap and alignment: NO output may overlap d_keys_in, d_offsets or the
 * other output: MISORT_E_INVALID, checked by address range before anything is
 * launched.  The inputs are left unchanged.  The key and index arrays need
 * 4-byte alignment, the offsets 8-byte alignment.
 *
 * ONE HOST WAIT PER CALL, the one of misort_local_sort_segments: a count kernel
 * reads d_offsets[0 .. nseg] (nothing else), validates every segment and counts
 * the segments per class (misort_segment_class with key_bytes 8); the host waits
 * for it and reads its header once, so that every later launch is sized
 * exactly.  Everything after the wait is asynchronous on `stream`; every launch
 * is on `stream`.  Because of the wait the call CANNOT BE CAPTURED IN A GRAPH,
 * and work queued on `stream` before it is waited for.
 *
 * How (misort_topk_segments_plan tells the passes of one segment): a fill
 * kernel writes the slots [len, k) of the rows of short segments.  Segments up
 * to 2^13 keys go through the u64 record tile, one launch per class LR = 5..13,
 * 2^(13-LR) segments per tile: the records are formed in registers and the
 * first min(len, k) of every sorted block are split into the row.  Longer
 * segments go class by class, c = ceil_log2(len): every piece of 2^13 keys is
 * sorted in one tile and leaves its first k records, 2^(c-13)*k candidates per
 * segment; from there the passes of misort_local_topk_rows for rows of 2^c
 * keys run over the class, and the last one writes row `segment`.  The keys are
 * read once and no merge pass runs.  Scratch kept by the context: 4 bytes per
 * segment plus a 2 KiB header, and for the long classes two candidate buffers
 * of at most max over c (count_c * 2^(c-13) * k) * 8 bytes. */
int misort_local_topk_segments(misort_ctx* ctx, int key_dtype, const void* d_keys_in,
                               void* d_keys_out, void* d_idx_out, int64_t n,
                               const int64_t* d_offsets, int64_t nseg,
                               int64_t k, int largest, void* stream);

/* Host only, no device: the passes misort_local_topk_segments runs for one
 * segment of `len` keys and `k`.  Writes up to max_passes passes (`passes` may
 * be NULL when max_passes is 0) as 4 ints each (m_in, LR, npieces, m_out), as
 * misort_topk_plan does:
 *   len == 0      0 passes (the fill alone);
 *   len <= 2^13   one pass: m_in = len, LR = max(ceil_log2(len), 5), npieces = 1,
 *                 m_out = min(len, k);
 *   longer        the passes of misort_topk_plan(2^ceil_log2(len), k).
 * Returns the number of passes, or MISORT_E_INVALID for a (len, k) that
 * misort_local_topk_segments refuses: k outside 1 .. 2^13, len < 0 or above
 * 2^31, k > 2^10 with len > 2^13. */
int misort_topk_segments_plan(int64_t len, int64_t k, int* passes, int max_passes);  /* host only */

#ifdef __cplusplus
}
#endif
#endif /* MISORT_TOPK_SEGMENTS_H */

/*
 * misort_segments_pairs.h -- segmented key-value sort and argsort, an extension
 * header of libmisort.so's C-ABI.
 *
 * Why a header of its own: tests/stream_order.py holds every `void* stream`
 * prototype of misort.h against a fixed table of cases, and this entry point
 * arrived without a case in that table (the situation misort_topk.h describes).
 * Its stream-order contract is pinned by tests/test_gpu_segments_pairs.py
 * instead, with the same procedure (behind_pending_work).  A later change can
 * fold this header into misort.h together with a table case.  Everything
 * misort.h says about contexts, streams, status codes and misort_last_error()
 * holds here.
 */
#ifndef MISORT_SEGMENTS_PAIRS_H
#define MISORT_SEGMENTS_PAIRS_H
#include "misort.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sorts variable-length segments of (32-bit key, 32-bit value) pairs, each
 * segment on its own by (key, value).  d_offsets is a DEVICE array of nseg + 1
 * int64 values; segment i is the elements [d_offsets[i], d_offsets[i+1]) of
 * the n-element arrays.  Well formed means 0 <= d_offsets[0], d_offsets[i] <=
 * d_offsets[i+1] and d_offsets[nseg] <= n, as for misort_local_sort_segments;
 * empty segments are allowed; 0 <= nseg <= 2^31 - 1, and n is bounded as there.
 * key_dtype MISORT_U32 or MISORT_F32 (anything else: MISORT_E_INVALID).  f32
 * keys are compared in the total order of their mapped bit patterns (sign set:
 * all bits inverted; else the sign bit set), exactly as in
 * misort_local_sort_rows_pairs: negative NaNs first, -inf ... -0.0, +0.0 ...
 * +inf, positive NaNs last.  Values are 32 bits and compare as unsigned; equal
 * keys come out in ascending value order.  Every output key is bit-identical
 * to an input key.
 *
 * Argsort mode, d_vals_in == NULL: the value of element d_offsets[i] + c is c,
 * its position INSIDE ITS SEGMENT, so d_vals_out holds the stable argsort of
 * every segment: d_keys_in[d_offsets[i] + idx] gathers the sorted segment, and
 * on uniform offsets the result is misort_local_sort_rows_pairs' argsort.  A
 * segment longer than 2^32 keys is MISORT_E_INVALID in this mode (a 32-bit
 * value holds 2^32 positions); the host decides it from the class counts,
 * before anything is written.
 *
 * Arrays: d_keys_in and d_vals_out are required; d_keys_out may be NULL (values
 * or indices only).  In place is allowed: d_keys_out == d_keys_in and
 * d_vals_out == d_vals_in, independently.  Any other overlap among the four
 * n-element arrays, and any overlap of an output with the (nseg + 1) * 8 bytes
 * of offsets, is MISORT_E_INVALID, checked by address range before anything is
 * launched.  The 32-bit arrays need 4-byte alignment only (segments start
 * anywhere: every access to them is an element access); the offsets need
 * 8-byte alignment.
 *
 * Written range: the segments' elements of every output given, and, out of
 * place, the fringes: the elements outside [d_offsets[0], d_offsets[nseg]) are
 * copied to the outputs that have an input, that is d_keys_out from d_keys_in
 * when d_keys_out is given and differs from d_keys_in, and d_vals_out from
 * d_vals_in when d_vals_in is given and differs from d_vals_out.  In argsort
 * mode the fringe of d_vals_out is NOT written.  In place the fringes are not
 * touched.  Inputs that are not outputs are left unchanged.
 *
 * n == 0 launches nothing and looks at no pointer; nseg == 0 does only the
 * fringe copies (all n elements).  MISORT_E_INVALID for a null context (checked
 * first), negative sizes, and a null array that would be read or written.
 *
 * ONE HOST WAIT PER CALL, the one of misort_local_sort_segments.  A count
 * kernel reads d_offsets[0 .. nseg] (nothing else), validates every segment and
 * counts segments and elements per class (misort_segment_class with key_bytes
 * 8) into a small header; the host waits for it and reads the header once (with
 * a communicator the wait is bounded as in misort_synchronize), so that every
 * later launch is sized exactly.  Everything after the wait is asynchronous on
 * `stream`.  Because of the wait the call CANNOT BE CAPTURED IN A GRAPH, and
 * work queued on `stream` before it is waited for.  Malformed offsets are
 * refused there: MISORT_E_INVALID, misort_last_error() names their count and
 * the first malformed index i (the pair d_offsets[i], d_offsets[i+1]), before
 * any key or value is read or written and before the fringe copies: the
 * outputs are unchanged.  A merge pass's rejected chunk (MISORT_E_INTERNAL) is
 * reported by misort_synchronize, as for misort_local_sort.
 *
 * How: what is sorted is the u64 record (K(key) << 32) | value of
 * misort_local_sort_pairs, so the classes are those of 8-byte keys.  Segments
 * up to 2^13 elements go through the u64 row tile of
 * misort_local_sort_rows_pairs, one launch per class LR = 5 .. 13: a tile holds
 * 2^(13-LR) segments of lengths in (2^(LR-1), 2^LR] (LR = 5: 1 .. 32); the
 * record is formed in registers as the tile loads and split as it stores, so
 * every array element is read once and written once, no record lies in HBM and
 * no scratch is used.  Longer segments go class by class, k = ceil_log2(length),
 * through padded blocks: a pad sweep forms the records of the class's segments
 * in blocks of 2^k (all-ones above the length), the passes of a 2^k-key u64
 * misort_local_sort run over the blocks, an unpad sweep splits the first
 * `length` records of every block into the outputs.  Scratch kept by the
 * context: 4 bytes per segment plus a 2 KiB header, and for the long classes two
 * buffers of max over k (count_k * 2^k) * 8 bytes. */
int misort_local_sort_segments_pairs(misort_ctx* ctx, int key_dtype,
                                     const void* d_keys_in, const void* d_vals_in,
                                     void* d_keys_out, void* d_vals_out, int64_t n,
                                     const int64_t* d_offsets, int64_t nseg, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MISORT_SEGMENTS_PAIRS_H */

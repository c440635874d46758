/*
 * recblr_filters.h — C-ABI of catalogue filters for the MI355X (gfx950) RecBLR
 * encoder: full-sort top-k and ranks over the items that a per-row allow-bitmap
 * keeps (in stock, sold in the caller's region, on the category page), not
 * over the whole item table.  Part of the product library (libdmrecblr.so,
 * RB_ABI_VERSION of recblr_hip.h); same conventions as recblr_hip.h: raw
 * device pointers, int64 sizes, a hipStream_t passed as void*, nothing
 * allocates or synchronises, arguments are checked before any HIP call, 0 /
 * RB_EINVAL / hipError_t returns, rb_last_error_string() for the message.
 * Plain C declarations, one per ';' — the Python binding
 * (datamining_recblr_amd/_lib.py) parses this header as it parses
 * recblr_hip.h.  Defined in csrc/capi.hip; kernels in csrc/item_scores.hip.
 *
 * Filters: allow [F, words] int32 contiguous, words = ceil(V / 32), F >= 1.
 * Bit i of word w of filter f is set iff filter f allows item 32 w + i (bit 31
 * is the int32's sign bit); bits at or beyond V are ignored.  The kernels walk
 * the item table in tiles of 32 items, so tile t of the items is word t of a
 * filter: one word load per (row, tile), ANDed into the tile's pass mask —
 * no per-item lookup, and a sparse filter means less selection work.
 *
 * allow_rows [B] int64, or NULL: the filter that row b selects.  NULL selects
 * filter 0 for every row.  -1 selects no filter (every item allowed: the
 * unfiltered call's result, bit for bit).  A value outside [-1, F) selects
 * nothing.  The filter and word indices are clamped for the load and the
 * result masked: nothing is dereferenced out of range whatever allow_rows
 * holds, and no value of it is an error.
 */
#ifndef RECBLR_FILTERS_H
#define RECBLR_FILTERS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* rb_item_topk over the items that row b's filter allows: everything else —
 * first_item, exclude, the NaN rule, the (score descending, item id ascending)
 * order, the id -1 / score -inf tail, the bit-identical scores, the
 * determinism — is rb_item_topk's, and so are its argument checks.  A row
 * that selects nothing returns k times (-1, -inf).  Workspace:
 * rb_item_topk_workspace(B, V, d, k). */
int rb_item_topk_allowed(const float* seq, const float* items, int64_t B, int64_t V, int64_t d,
                         int64_t k, int64_t first_item, const int64_t* exclude, int64_t E,
                         int64_t* ids, float* scores, void* workspace, int64_t workspace_bytes,
                         void* stream, const int32_t* allow, int64_t F, int64_t words,
                         const int64_t* allow_rows);

/* rb_item_rank over the items that row b's filter allows: n_greater / n_equal
 * count allowed items only.  A target that its row's filter does not allow
 * gives -1, -1, as an out-of-range target does.  Workspace:
 * rb_item_rank_workspace(B, V, d). */
int rb_item_rank_allowed(const float* seq, const float* items, const int64_t* target, int64_t B,
                         int64_t V, int64_t d, int64_t first_item, int64_t* n_greater,
                         int64_t* n_equal, void* workspace, int64_t workspace_bytes,
                         void* stream, const int32_t* allow, int64_t F, int64_t words,
                         const int64_t* allow_rows);

#ifdef __cplusplus
}
#endif

#endif /* RECBLR_FILTERS_H */

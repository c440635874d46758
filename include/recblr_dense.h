/*
 * recblr_dense.h — C-ABI of the all-position ("dense") training loss of the
 * MI355X (gfx950) RecBLR encoder.  Part of the product library
 * (libdmrecblr.so, RB_ABI_VERSION of recblr_hip.h); same conventions as
 * recblr_hip.h: raw device pointers, int64 sizes, a hipStream_t passed as
 * void*, nothing allocates or synchronises, 0 / RB_EINVAL / hipError_t
 * returns, rb_last_error_string() for the message.  Plain C declarations, one
 * per ';' — the Python binding (datamining_recblr_amd/_lib.py) parses this
 * header as it parses recblr_hip.h.  Defined in csrc/capi.hip.
 *
 * The encoder is causal and its pow2 pad prefix depends only on L, so row t
 * of a packed sequence (RecBLR.forward_all) holds what the reference computes
 * for the prefix sample items[:t+1] -> items[t+1] (RecBLR.py:75-102 on
 * RecBole's augmented rows).  These entry points score every packed row
 * against the item table in row chunks, with rows that carry no target
 * ignored: replaces nn.CrossEntropyLoss(ignore_index=-1) on logits that are
 * never stored.
 */
#ifndef RECBLR_DENSE_H
#define RECBLR_DENSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Per-row training targets of the packed rows (rb_pack_plan's layout: ids
 * [ntok], seq_offsets [B+1], order [B]; pos_items [B] in batch-row order):
 * for row r = seq_offsets[s] + t of packed sequence s,
 *   targets[r] = ids[r + 1]                 when r + 1 < seq_offsets[s+1],
 *              = pos_items[order[s]]        at the sequence's last row,
 * and targets[r] = -1 for ntok <= r < m_pad (the loss's padding rows) and for
 * any row whose offsets / order entry is out of range (every index is checked
 * before it is used).  One launch, every row written once.  All device int64. */
int rb_next_item_targets(const int64_t* ids, const int64_t* seq_offsets, const int64_t* order,
                         const int64_t* pos_items, int64_t B, int64_t ntok, int64_t m_pad,
                         int64_t* targets, void* stream);

/* The "rows" variants of rb_item_ce_fwd_h / rb_item_ce_probs_h /
 * rb_item_ce_probs_h_both (recblr_hip.h; same kernels, same arguments) for one
 * row chunk of a larger call:
 *   target in [0, V)  a live row;
 *   target == -1      an ignored row: nothing added to the loss, its P row
 *                     exactly 0.0 in both layouts, 0 in both group maxima;
 *                     lse is still written.  Its seq row must be finite
 *                     (padding rows are zeros);
 *   any other target  NaN loss, as rb_item_ce_fwd_h.
 * inv_n in (0, 1]: 1 / (live rows of the whole call) — the normaliser in place
 * of 1 / B.  The forward writes loss[0] = inv_n * sum over the chunk's live
 * rows of (lse - target score), added to the value loss[0] holds when
 * accumulate = 1 (the chunks of one call, in stream order: a fixed order).
 * Workspace: rb_item_ce_workspace(B, V, d). */
int rb_item_ce_fwd_h_rows(const void* seq_img, const int* seq_exp, const void* item_img,
                          const int* item_exp, const int64_t* target, int64_t B, int64_t V,
                          int64_t d, float inv_n, int accumulate, float* lse, float* loss,
                          void* workspace, int64_t workspace_bytes, void* stream);

int rb_item_ce_probs_h_rows(const void* seq_img, const int* seq_exp, const void* item_img,
                            const int* item_exp, const int64_t* target, const float* lse,
                            const float* dloss, float inv_n, int64_t B, int64_t V, int64_t d,
                            int64_t item_offset, float* probs, int64_t ld, void* stream);

int rb_item_ce_probs_h_both_rows(const void* seq_img, const int* seq_exp, const void* item_img,
                                 const int* item_exp, const int64_t* target, const float* lse,
                                 const float* dloss, float inv_n, int64_t B, int64_t V, int64_t d,
                                 int64_t item_offset, float* probs, int64_t ld, float* probs_t,
                                 int64_t ldt, float* row_group_max, float* item_group_max,
                                 void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RECBLR_DENSE_H */

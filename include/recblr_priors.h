/*
 * recblr_priors.h — C-ABI of score priors for the MI355X (gfx950) RecBLR
 * encoder: full-sort top-k and ranks over model score + weight * prior[item]
 * (a promotion, a recency or margin boost, a popularity damping, a per-market
 * prior), still without the [B, V] score matrix.  Part of the product library
 * (libdmrecblr.so, RB_ABI_VERSION of recblr_hip.h); same conventions as
 * recblr_hip.h: raw device pointers, int64 sizes, a hipStream_t passed as
 * void*, nothing allocates or synchronises, arguments are checked before any
 * HIP call, 0 / RB_EINVAL / hipError_t returns, rb_last_error_string() for the
 * message.  Plain C declarations, one per ';' — the Python binding
 * (datamining_recblr_amd/_lib.py) parses this header as it parses
 * recblr_hip.h.  Defined in csrc/capi.hip; kernels in csrc/item_scores.hip.
 *
 * Priors: prior [P, V] fp32 contiguous, P >= 1: P per-item vectors.
 * prior_rows [B] int64, or NULL: the vector that row b takes.  NULL: vector 0
 * for every row.  -1: no prior for that row (the result of the call without a
 * prior, bit for bit).  A value outside [-1, P): the row selects nothing (its
 * rank is -1, -1).  The vector and item indices are clamped for the load and
 * the value used only where it applies: nothing is dereferenced out of range
 * whatever prior_rows holds, and no value of it is an error.
 * prior_weight [B] fp32, or NULL (1 for every row): the row's strength w_b.
 *
 * The adjusted score of row b and item v is
 *     adj(b, v) = score(b, v)                            (prior_rows[b] == -1)
 *     adj(b, v) = score(b, v) + (w_b * prior[p_b, v])    otherwise
 * with score rb_item_scores' bits, the product rounded to fp32 and then the sum
 * (two roundings, no fused multiply-add), so it is reproducible in any fp32
 * arithmetic.  Every rule of rb_item_topk / rb_item_rank then applies to adj:
 * the order is (adj descending, item id ascending), a NaN adj is never selected
 * or counted, an item may be selected with adj = -inf, and the scores returned
 * are adjusted scores.
 */
#ifndef RECBLR_PRIORS_H
#define RECBLR_PRIORS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace bytes of rb_item_topk_prior (0 for arguments it rejects): enough
 * with or without groups (rb_item_topk_grouped_workspace's figure). */
int64_t rb_item_topk_prior_workspace(int64_t B, int64_t V, int64_t d, int64_t k);

/* rb_item_topk_grouped over adjusted scores.  allow NULL: no filter (F, words
 * and allow_rows are then ignored); groups NULL: no cap (max_per_group is then
 * ignored).  Everything else — first_item, exclude, the filter, the cap, the
 * id -1 / score -inf tail, the determinism, the argument checks — is that
 * call's. */
int rb_item_topk_prior(const float* seq, const float* items, int64_t B, int64_t V, int64_t d,
                       int64_t k, int64_t first_item, const int64_t* exclude, int64_t E,
                       int64_t* ids, float* scores, void* workspace, int64_t workspace_bytes,
                       void* stream, const int32_t* allow, int64_t F, int64_t words,
                       const int64_t* allow_rows, const int32_t* groups, int64_t max_per_group,
                       const float* prior, int64_t P, const int64_t* prior_rows,
                       const float* prior_weight);

/* rb_item_rank_allowed over adjusted scores (allow NULL: no filter): n_greater
 * / n_equal count the items whose adj is greater than / equal to the target's
 * adj.  The target's score is rb_item_rank's, adjusted as above; a target whose
 * adj is NaN gives -1, -1, as an out-of-range target does.  Workspace:
 * rb_item_rank_workspace(B, V, d). */
int rb_item_rank_prior(const float* seq, const float* items, const int64_t* target, int64_t B,
                       int64_t V, int64_t d, int64_t first_item, int64_t* n_greater,
                       int64_t* n_equal, void* workspace, int64_t workspace_bytes, void* stream,
                       const int32_t* allow, int64_t F, int64_t words, const int64_t* allow_rows,
                       const float* prior, int64_t P, const int64_t* prior_rows,
                       const float* prior_weight);

#ifdef __cplusplus
}
#endif

#endif /* RECBLR_PRIORS_H */

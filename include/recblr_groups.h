/*
 * recblr_groups.h — C-ABI of diversity caps for the MI355X (gfx950) RecBLR
 * encoder: full-sort top-k with at most m items of one group (brand, seller,
 * category, series) in a row's list.  Part of the product library
 * (libdmrecblr.so, RB_ABI_VERSION of recblr_hip.h); same conventions as
 * recblr_hip.h: raw device pointers, int64 sizes, a hipStream_t passed as
 * void*, nothing allocates or synchronises, arguments are checked before any
 * HIP call, 0 / RB_EINVAL / hipError_t returns, rb_last_error_string() for the
 * message.  Plain C declarations, one per ';' — the Python binding
 * (datamining_recblr_amd/_lib.py) parses this header as it parses
 * recblr_hip.h.  Defined in csrc/capi.hip; kernels in csrc/item_scores.hip.
 *
 * Groups: groups [V] int32 contiguous, one id per item.  -1: the item is never
 * capped.  Otherwise an id in [0, RB_GROUP_ID_MAX]: the kernel keeps a group
 * per list entry in 16 bits of LDS.  The values are the caller's contract and
 * are not read on the host: an id outside that range is taken modulo 65536
 * (nothing is dereferenced by it).
 *
 * The result is that of a walk: the row's selectable items (rb_item_topk's
 * rules: first_item, exclude, the allow-bitmap if given, never NaN) in
 * rb_item_topk's order (score descending, item id ascending), taking an item
 * unless max_per_group items of its group were taken, until k are taken.
 */
#ifndef RECBLR_GROUPS_H
#define RECBLR_GROUPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RB_GROUP_ID_MAX 65534

/* Workspace bytes of rb_item_topk_grouped (0 for arguments it rejects): the
 * candidate lists of rb_item_topk_workspace and each entry's group. */
int64_t rb_item_topk_grouped_workspace(int64_t B, int64_t V, int64_t d, int64_t k);

/* rb_item_topk under a cap of max_per_group (>= 1) items per group; allow
 * NULL: no filter (F, words and allow_rows are then ignored), otherwise the
 * allow-bitmaps of recblr_filters.h.  Everything else — the tie order, the id
 * -1 / score -inf tail where fewer than k are taken, the bit-identical scores,
 * the determinism, the argument checks — is rb_item_topk's.  A cap of k or
 * more, or groups that are all distinct or all -1, give rb_item_topk's (or
 * rb_item_topk_allowed's) result bit for bit. */
int rb_item_topk_grouped(const float* seq, const float* items, int64_t B, int64_t V, int64_t d,
                         int64_t k, int64_t first_item, const int64_t* exclude, int64_t E,
                         int64_t* ids, float* scores, void* workspace, int64_t workspace_bytes,
                         void* stream, const int32_t* allow, int64_t F, int64_t words,
                         const int64_t* allow_rows, const int32_t* groups,
                         int64_t max_per_group);

#ifdef __cplusplus
}
#endif

#endif /* RECBLR_GROUPS_H */

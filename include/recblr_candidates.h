/*
 * recblr_candidates.h — C-ABI of candidate-list scoring for the MI355X
 * (gfx950) RecBLR encoder: each row's representation against a list of chosen
 * item ids instead of the whole item table (reranking, sampled evaluation).
 * Part of the product library (libdmrecblr.so, RB_ABI_VERSION of
 * recblr_hip.h); same conventions as recblr_hip.h: raw device pointers, int64
 * sizes, a hipStream_t passed as void*, nothing allocates or synchronises,
 * arguments are checked before any HIP call, 0 / RB_EINVAL / hipError_t
 * returns, rb_last_error_string() for the message.  Plain C declarations, one
 * per ';' — the Python binding (datamining_recblr_amd/_lib.py) parses this
 * header as it parses recblr_hip.h.  Defined in csrc/capi.hip; kernels in
 * csrc/candidates.hip.
 *
 * Common to the three: h [B, d] fp32 (row stride ldh >= d, ldh % 4 == 0),
 * table [V, d] fp32 contiguous, both 16-B aligned; d a multiple of 4 in
 * [4, 512]; 1 <= V < 2^31; cand [B, C] int64 contiguous.  B == 0 succeeds and
 * does nothing.  An id is clamped for its loads and the result masked: no id
 * is ever dereferenced out of range.
 *
 * The score of a (row, id) pair is a pure function of the d floats of h_b and
 * the d floats of table[id]: the same bits wherever the id stands in the
 * list, whatever B and C are, whichever of the three entry points computes
 * it.  Two table rows of equal contents tie exactly.
 */
#ifndef RECBLR_CANDIDATES_H
#define RECBLR_CANDIDATES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* scores[b, c] = h_b . table[cand[b, c]]; -inf for an id outside [0, V) (so -1
 * pads a ragged list).  scores [B, C] fp32 contiguous.  C >= 1, B * C < 2^37.
 * The grid runs over the flattened B * C pairs. */
int rb_candidate_scores(const float* h, int64_t ldh, const float* table, const int64_t* cand,
                        int64_t B, int64_t C, int64_t d, int64_t V, float* scores,
                        void* stream);

/* Per row the k best of its list, in one launch: over the distinct ids of
 * cand[b] that lie in [first_item, V), are not listed in exclude[b] ([B, E]
 * int64 contiguous, NULL with E = 0; entries outside [0, V) are ignored,
 * duplicates allowed) and whose score is not NaN, ordered by (score
 * descending, id ascending) — rb_item_topk's order.  A repeated candidate id
 * appears once.  ids [B, k] int64, scores [B, k] fp32; where fewer than k
 * survive the tail holds id -1, score -inf.  A score of -0 is returned as +0.
 * 1 <= C <= 4096, 0 <= E <= 4096, 1 <= k < 2^31, 0 <= first_item <= V,
 * B < 2^31.  One 256-thread workgroup per row; LDS 8 * pow2(C) + 4 * E bytes
 * (at most 48 KB). */
int rb_candidate_topk(const float* h, int64_t ldh, const float* table, const int64_t* cand,
                      int64_t B, int64_t C, int64_t d, int64_t V, int64_t first_item, int64_t k,
                      const int64_t* exclude, int64_t E, int64_t* ids, float* scores,
                      void* stream);

/* Per row, over the entries of cand[b] that lie in [first_item, V), differ
 * from target[b] and have a non-NaN score: n_greater[b] = how many score
 * strictly above h_b . table[target[b]], n_equal[b] = how many score exactly
 * equal to it.  Entries count as listed (a repeated id counts each time).  A
 * target outside [first_item, V) gives -1, -1.  target, n_greater, n_equal [B]
 * int64.  Integer sums: deterministic.  C >= 1 with no upper limit beyond B *
 * ceil(C / 1024) < 2^31; 0 <= first_item <= V. */
int rb_candidate_ranks(const float* h, int64_t ldh, const float* table, const int64_t* target,
                       const int64_t* cand, int64_t B, int64_t C, int64_t d, int64_t V,
                       int64_t first_item, int64_t* n_greater, int64_t* n_equal, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RECBLR_CANDIDATES_H */

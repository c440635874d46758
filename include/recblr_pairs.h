/*
 * recblr_pairs.h — C-ABI of the sampled pairwise (BPR) loss of all-position
 * training of the MI355X (gfx950) RecBLR encoder.  Part of the product
 * library (libdmrecblr.so, RB_ABI_VERSION of recblr_hip.h); same conventions
 * as recblr_hip.h: raw device pointers, int64 sizes, a hipStream_t passed as
 * void*, nothing allocates or synchronises, arguments are checked before any
 * HIP call, 0 / RB_EINVAL / hipError_t returns, rb_last_error_string() for
 * the message.  Plain C declarations, one per ';' — the Python binding
 * (datamining_recblr_amd/_lib.py) parses this header as it parses
 * recblr_hip.h.  Defined in csrc/capi.hip; kernels in csrc/pair_loss.hip,
 * csrc/shared_softmax.hip and csrc/embedding.hip.
 *
 * Every packed row (RecBLR.forward_all, recblr_dense.h) is scored against its
 * target and n sampled negatives only: (2 + n) rows of d floats per position
 * instead of a sweep over the item table.
 */
#ifndef RECBLR_PAIRS_H
#define RECBLR_PAIRS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Negative sampling.  item_seq [B, L] (row stride seq_rs) right-padded rows,
 * lengths [B] (clamped to [1, L]), pos_items [B]; all device int64.  The seen
 * set of row b is item_seq[b, :len_b] and pos_items[b] — the row's window,
 * not the user's whole history.  The negative of (b, t, j), j < n_neg, is
 * uniform over [first_item, V) minus that set:
 *   attempt a = 0 .. 15 takes word a % 4 of Philox4x32-10(counter = (b, t, j,
 *   a / 4), key = seed) and maps it to first_item + mulhi(word, V -
 *   first_item); the first attempt that is not seen wins; after 16 rejections
 *   the ids above the 16th candidate are walked upward, cyclically through
 *   [first_item, V), to the first unseen one; -1 when every id is seen.
 * offsets [B + 1] and inv [B] given (rb_pack_plan's layout): every position
 * t < len_b writes neg[(offsets[inv[b]] + t) * n_neg + j] — packed order, rows
 * < ntok — and the rows [ntok, m_pad) are filled with -1.  Both NULL (ntok =
 * m_pad = B): only t = len_b - 1 is drawn, into row b; these are exactly the
 * dense call's rows at each sequence's last position.  A pure function of its
 * arguments; no atomics.  Needs 1 <= n_neg <= 256, 0 <= first_item < V < 2^31,
 * L <= 8191; an index outside its range writes nothing. */
int rb_sample_negatives(const int64_t* item_seq, int64_t seq_rs, const int64_t* lengths,
                        const int64_t* pos_items, const int64_t* offsets, const int64_t* inv,
                        int64_t B, int64_t L, int64_t n_neg, int64_t first_item, int64_t V,
                        uint64_t seed, int64_t ntok, int64_t m_pad, int64_t* neg, void* stream);

/* rb_sample_negatives with a proposal other than the uniform one: alias [V -
 * first_item] int64 (device, 8-B aligned) is an alias table over the bins i =
 * id - first_item, one word per bin: the low 32 bits an unsigned threshold,
 * the high 32 bits the bin's alias (an alias past the table is read as its
 * last bin).  Everything else is rb_sample_negatives': the seen set, the 16
 * attempts, the walk upward from the 16th candidate, -1, both layouts.  Only
 * the candidate of attempt a differs, and an attempt takes two Philox words:
 *   (u, v) = words (2 (a % 2), 2 (a % 2) + 1) of Philox4x32-10(counter = (b, t,
 *   j, a / 2), key = seed);  i = mulhi(u, V - first_item);  the candidate is
 *   first_item + (v < threshold[i] ? i : alias[i]).
 * The table is only read (one 8-byte load per attempt).  kernels.
 * negative_sampler builds it (Vose's method) together with the exact
 * probability of every id under this rule. */
int rb_sample_negatives_alias(const int64_t* item_seq, int64_t seq_rs, const int64_t* lengths,
                              const int64_t* pos_items, const int64_t* offsets,
                              const int64_t* inv, int64_t B, int64_t L, int64_t n_neg,
                              int64_t first_item, int64_t V, uint64_t seed, int64_t ntok,
                              int64_t m_pad, const int64_t* alias, int64_t* neg, void* stream);

/* Bytes of rb_pair_loss_fwd's workspace for M rows (0 for M <= 0). */
int64_t rb_pair_loss_workspace(int64_t M);

/* h [M, d] (row stride ldh), table [V, d], pos [M] (rb_next_item_targets: -1
 * an ignored row), neg [M, n_neg] (-1 an ignored pair).  For every live pair
 *   x = h_r . table[pos_r] - h_r . table[neg_rj]    -> diff [M, n_neg] (0 when ignored)
 *   l = -log(gamma + sigmoid(x))
 * loss[0] = sum l / max(n_live, 1), n_live[0] = live pairs (device scalars,
 * no host sync); the sum runs over per-workgroup partials in workgroup order.
 * An id outside [-1, V) gives a NaN loss (it is never dereferenced).  d a
 * multiple of 4 up to 512; h, table 16-B aligned with ldh % 4 == 0. */
int rb_pair_loss_fwd(const float* h, int64_t ldh, const float* table, const int64_t* pos,
                     const int64_t* neg, int64_t M, int64_t d, int64_t V, int64_t n_neg,
                     float gamma, float* diff, float* loss, int64_t* n_live, void* workspace,
                     int64_t workspace_bytes, void* stream);

/* With c_rj = dloss[0] / max(n_live[0], 1) * (-s (1 - s) / (gamma + s)), s =
 * sigmoid(diff_rj), and c_rj = 0 for an ignored pair:
 *   dh [M, d] (contiguous)  dh_r = sum_j c_rj (table[pos_r] - table[neg_rj])
 *   coef [(1 + n_neg) * M]  [ sum_j c_rj | -c_r0 | -c_r1 | ... ], one block of M
 *                           per id column: position p = k * M + r of the ids
 *                           [pos | neg_0 | neg_1 ...] has the gradient row
 *                           coef[p] * h_r (rb_embedding_bwd_apply_scaled). */
int rb_pair_loss_bwd(const float* table, const int64_t* pos, const int64_t* neg,
                     const float* diff, const float* dloss, const int64_t* n_live, int64_t M,
                     int64_t d, int64_t V, int64_t n_neg, float gamma, float* dh, float* coef,
                     void* stream);

/* rb_embedding_bwd_apply (recblr_hip.h; same plan, same workspace, same sums)
 * with position p's gradient row read as coef[p] * src[p mod src_rows] (src
 * [src_rows, d], row stride src_ld) instead of grad[p]: the M gradient rows are
 * never stored.  Bitwise rb_embedding_bwd_apply on the materialised rows. */
int rb_embedding_bwd_apply_scaled(const float* src, int64_t src_ld, int64_t src_rows,
                                  const float* coef, int64_t M, int64_t d, int64_t V,
                                  int64_t padding_idx, float* dweight, void* workspace,
                                  int64_t workspace_bytes, void* stream);

/* ---- sampled softmax with negatives shared per sequence (csrc/shared_softmax.hip) ----
 * h [M, d] (row stride ldh) packed rows, table [V, d], target [M]
 * (rb_next_item_targets: -1 an ignored row), neg [B, n_neg] one list per batch
 * row (-1 a dead column), offsets [B + 1] / order [B] (rb_pack_plan's layout:
 * packed sequence s is batch row b = order[s] at rows offsets[s] ..
 * offsets[s + 1]).  For row r of sequence s
 *   z0 = h_r . table[target_r],  z_j = h_r . table[neg[b, j]] + shift  (live columns)
 *   lse[r] = logsumexp(z0, z_j ...),  z0 -> z0[r]     (written for ignored rows too)
 * loss[0] = sum over the live rows of (lse[r] - z0[r]) / max(n_live, 1),
 * n_live[0] = live rows (device scalars, no host sync); the sum runs over
 * per-workgroup partials in workgroup order.  An id outside [-1, V) gives a NaN
 * loss (it is never dereferenced).  A plan entry with rows outside [0, M), no
 * rows, or a batch row outside [0, B) is skipped.  max_len >= 1: an upper
 * estimate of the longest sequence; it sizes the grid and the workspace only
 * (longer sequences are still covered).  d a multiple of 16 in [16, 224],
 * 1 <= n_neg <= 256; h, table 16-B aligned with ldh % 4 == 0. */
int64_t rb_shared_softmax_workspace(int64_t B, int64_t max_len);

int rb_shared_softmax_fwd(const float* h, int64_t ldh, const float* table,
                          const int64_t* target, const int64_t* neg, const int64_t* offsets,
                          const int64_t* order, int64_t M, int64_t B, int64_t d, int64_t V,
                          int64_t n_neg, int64_t max_len, float shift, float* lse, float* z0,
                          float* loss, int64_t* n_live, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* With scale = dloss[0] / max(n_live[0], 1) and p_rj = exp(z_j - lse[r]) (0 for
 * a dead column or an ignored row), for the rows the plan covers:
 *   dh [M, d] (contiguous)   dh_r = scale (sum_j p_rj table[neg[b, j]] - q_r table[target_r]),
 *                            q_r = sum_j p_rj = 1 - p_r0
 *   coef [M]                 -scale q_r: the target's gradient row is coef[r] * h_r
 *                            (rb_embedding_bwd_apply_scaled over the ids target)
 *   dneg [B, n_neg, d]       scale sum_{r in s} p_rj h_r, summed over the sequence's
 *                            rows in order (rb_embedding_bwd_apply over the ids neg)
 * Rows and lists no plan entry covers are not written. */
int rb_shared_softmax_bwd(const float* h, int64_t ldh, const float* table,
                          const int64_t* target, const int64_t* neg, const int64_t* offsets,
                          const int64_t* order, const float* lse, const float* dloss,
                          const int64_t* n_live, int64_t M, int64_t B, int64_t d, int64_t V,
                          int64_t n_neg, int64_t max_len, float shift, float* dh, float* coef,
                          float* dneg, void* stream);

/* The same two with a per-item correction of the proposal: item_shift [V]
 * (device fp32, finite at every id a list holds), and a live column of id j
 * scores
 *   z_j = (h_r . table[j] + shift) + item_shift[j]
 * in that order; z0 is unshifted as above.  With negatives drawn with
 * probability q_j each, shift = -log(n_neg) and item_shift[j] = -log(q_j) make
 * sum_j exp(z_j) an estimate of the full softmax's sum.  A dead column or an id
 * outside [0, V) reads nothing of item_shift.  Everything else, the sums'
 * orders included, is rb_shared_softmax_fwd / _bwd's; item_shift has no
 * gradient. */
int rb_shared_softmax_fwd_items(const float* h, int64_t ldh, const float* table,
                                const int64_t* target, const int64_t* neg,
                                const int64_t* offsets, const int64_t* order, int64_t M,
                                int64_t B, int64_t d, int64_t V, int64_t n_neg, int64_t max_len,
                                float shift, const float* item_shift, float* lse, float* z0,
                                float* loss, int64_t* n_live, void* workspace,
                                int64_t workspace_bytes, void* stream);

int rb_shared_softmax_bwd_items(const float* h, int64_t ldh, const float* table,
                                const int64_t* target, const int64_t* neg,
                                const int64_t* offsets, const int64_t* order, const float* lse,
                                const float* dloss, const int64_t* n_live, int64_t M, int64_t B,
                                int64_t d, int64_t V, int64_t n_neg, int64_t max_len, float shift,
                                const float* item_shift, float* dh, float* coef, float* dneg,
                                void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RECBLR_PAIRS_H */

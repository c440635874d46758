/* recblr_session.h — stateful session inference (libdmrecblr_session.so).
 *
 * rb_session_step advances the whole RecBLR encoder by one event per session
 * slot in one launch, rb_session_append by up to 16 consecutive events per
 * slot; rb_session_capture reads a layer's session state off its forward
 * over stored histories; rb_session_record keeps the ring of the last item
 * ids a slot consumed; rb_session_transfer parks a slot's whole state as one
 * row of words and resumes it (python: datamining_recblr_amd/session.py).  Its own
 * library, beside the product library, as the probe and experimental
 * libraries are ("Stateful sessions").  Same conventions as the
 * boundary (include/recblr_hip.h): raw device pointers, int status (0 = ok,
 * RB_EINVAL = -1 for a bad argument, checked before any HIP call),
 * rb_session_last_error_string() for the message, stream as void*. */
#ifndef RECBLR_SESSION_H
#define RECBLR_SESSION_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RB_SESSION_MAX_LAYERS 8
/* slots per workgroup (the M of the fp32 MFMA tile) */
#define RB_SESSION_TILE 16
/* the LDS of one gfx950 compute unit: the step kernel's budget */
#define RB_SESSION_MAX_LDS 163840
/* row status written by rb_session_step and rb_session_append */
#define RB_SESSION_NO_EVENT 0
#define RB_SESSION_STEPPED 1
#define RB_SESSION_BAD_ITEM (-1)
#define RB_SESSION_BAD_SLOT (-2)
/* row status written by rb_session_transfer (with RB_SESSION_BAD_SLOT) */
#define RB_SESSION_MOVED 2
#define RB_SESSION_BAD_BLOB (-3)
/* the number the blob format below carries in its tag */
#define RB_SESSION_BLOB_FORMAT 1

/* One RecurrentLayer (RecBLR.py:124-145): its parameters (host struct of
 * device pointers, fp32, contiguous, 16-byte aligned) and the per-slot state
 * it carries for N slots. */
typedef struct {
  const float* w_in;      /* [2H, d]  behavior_modeling.input.weight */
  const float* conv_w;    /* [H, K]   conv1d.weight (unused with disable_conv1d) */
  const float* conv_b;    /* [H]      conv1d.bias   (unused with disable_conv1d) */
  const float* w_gate;    /* [2H, H]  gates.weight */
  const float* b_gate;    /* [2H]     gates.bias */
  const float* lam;       /* [H]      Lambda */
  const float* w_out;     /* [d, H]   output.weight */
  const float* ln_w;      /* [d]      layer_norm */
  const float* ln_b;      /* [d] */
  const float* w1;        /* [4d, d]  ffn.w_1 (the six ffn pointers unused with disable_ffn) */
  const float* b1;        /* [4d] */
  const float* w2;        /* [d, 4d]  ffn.w_2 */
  const float* b2;        /* [d] */
  const float* ffn_ln_w;  /* [d]      ffn.layer_norm */
  const float* ffn_ln_b;  /* [d] */
  const float* h0;        /* [H] state of a slot with count == 0 (the pad-prefix state,
                             rb_pad_prefix_fwd); NULL = zeros */
  float* h;               /* [N, H]       recurrent state, read when count > 0, written */
  float* conv_state;      /* [N, K-1, H]  the last K-1 pre-conv rows, oldest first; zeros
                             are read when count == 0 (unused with disable_conv1d or K == 1) */
} rb_session_layer;

/* ABI version of the session library (the product ABI it pairs with). */
int rb_session_version(void);
const char* rb_session_last_error_string(void);

/* Dynamic LDS bytes the step kernel needs for (d, H); rb_session_step refuses
 * shapes whose need exceeds the CU's 160 KiB. */
int64_t rb_session_lds_bytes(int64_t d, int64_t H);

/* One encoder step (RecBLR.py:75-84 at a single position; eval mode) for B
 * rows in one launch.  Row b carries item items[b] for slot slots[b] (slots
 * NULL: slot b); slots must be unique.  For an item v in [1, V):
 *   x = LN(emb[v]); per layer: xz = x W_in^T, u | z = xz; xc = silu(conv_b +
 *   sum_j conv_w[:, j] u_hist[j]) over the K-1 stored rows and u, history
 *   shifted; r | i = xc W_g^T + b_g; alpha = exp(-softplus(Lambda) sigmoid(r));
 *   beta = sqrt(1 - alpha^2 + 1e-8) sigmoid(i); h = alpha h + beta xc;
 *   x = LN((silu(z) h) W_out^T + x); x = LN(w_2 silu(w_1 x + b_1) + b_2 + x)
 *   (no conv with disable_conv1d, no FFN with disable_ffn; FFN width 4d);
 *   out[slot] = x; count[slot] += 1.
 * Item 0 is "no event": nothing of the slot is touched.  An item outside
 * [0, V) or a slot outside [0, N) is never dereferenced: the row is masked
 * and its state left alone.  y [B, d] (optional) receives the row's out
 * (the stored one for a row that did not step; zeros for a bad slot) and
 * status [B] int32 (optional) one of RB_SESSION_*.
 * emb [V, d]; ln_w, ln_b [d] the embedding LayerNorm; eps for every
 * LayerNorm; count [N] int64; out [N, d].  d and H multiples of 16, K in
 * [1, 8], n_layers in [1, RB_SESSION_MAX_LAYERS].  One workgroup owns
 * RB_SESSION_TILE consecutive rows through every layer; a row's arithmetic
 * does not depend on the other rows of the call. */
int rb_session_step(const rb_session_layer* layers, int64_t n_layers, const float* emb,
                    const float* ln_w, const float* ln_b, float eps, const int64_t* items,
                    const int64_t* slots, int64_t* count, float* out, float* y,
                    int32_t* status, int64_t B, int64_t N, int64_t V, int64_t d, int64_t H,
                    int64_t K, int disable_conv1d, int disable_ffn, void* stream);

/* Up to T consecutive events per row in one launch.  items [B, T] int64,
 * row-major, right-padded: row b's events are the n_b entries before its
 * first 0 (entries after it are ignored).  T is 1, 2, 4, 8 or 16; a workgroup
 * owns 16 / T consecutive rows, tile row r being event r % T of call row
 * r / T.  Row b's slot (slots as for the step: unique, NULL = slot b) is left
 * as n_b successive rb_session_step calls with items[b, 0 .. n_b) would
 * leave it, bit for bit: h, conv_state, out, and count += n_b; the state is
 * written once, after the last event.  y [B, d] (optional) receives the
 * slot's out afterwards (the stored one when n_b == 0; zeros for a bad
 * slot), y_all [B, T, d] (optional) the output after each event, zeros at
 * positions >= n_b and for masked rows, status [B] (optional)
 * RB_SESSION_STEPPED when n_b >= 1, NO_EVENT when items[b, 0] == 0, BAD_SLOT
 * for a slot outside [0, N), BAD_ITEM when any of the n_b events lies outside
 * [0, V).  A BAD_ITEM row is masked as a whole: nothing of its slot is
 * touched.  Every id is range-checked before an address is formed from it.
 * The other arguments and their limits are rb_session_step's; y_all 16-byte
 * aligned when given. */
int rb_session_append(const rb_session_layer* layers, int64_t n_layers, const float* emb,
                      const float* ln_w, const float* ln_b, float eps, const int64_t* items,
                      const int64_t* slots, int64_t* count, float* out, float* y, float* y_all,
                      int32_t* status, int64_t B, int64_t T, int64_t N, int64_t V, int64_t d,
                      int64_t H, int64_t K, int disable_conv1d, int disable_ffn, void* stream);

/* The state of one layer after each of B packed sequences' last position,
 * read off that layer's forward (one launch per layer; python:
 * session.prefill(method="forward")).  Sequence b occupies rows
 * seq_offsets[b] .. seq_offsets[b+1] of the packed activations and has
 * n = seq_offsets[b+1] - seq_offsets[b] positions; for n >= 1:
 *   h[slots[b]] = the carry of tile j = (n - 1) / RB_TILE advanced by the
 *   steps 16 j .. n - 1 of rb_gate_scan_fwd's recurrence: r | i = rg + gate_b;
 *   alpha = exp(-softplus(lam) sigmoid(r)); beta = sqrt(1 - alpha^2 + 1e-8)
 *   sigmoid(i); h = alpha h + beta xc;
 *   conv_state[slots[b], k] = the u row at position n - (K - 1) + k for k in
 *   [0, K - 1), oldest first; zeros for a position before the sequence start.
 * u [ntok, H] the pre-conv rows (the x half of the in-projection), xc
 * [ntok, H] the conv + SiLU output (xc == u with disable_conv1d), rg
 * [ntok, 2H] the gates GEMM's output without its bias; u_rs, xc_rs, rg_rs
 * their row strides in floats; lam [H]; gate_b [2H]; carries
 * [B, ceil(L / RB_TILE), H] as rb_gate_scan_fwd(_last) wrote them for the
 * same B, L and seq_offsets; seq_offsets [B + 1]; slots [B], unique; h
 * [N, H]; conv_state [N, K - 1, H], NULL only when K == 1 or xc == u (then
 * no history is written).  A sequence with n < 1, with more tiles than
 * carries holds (n > RB_TILE ceil(L / RB_TILE)) or with a slot outside
 * [0, N) is skipped before any address is formed from it; the other
 * slots of h and conv_state are not written.  H a positive multiple of 4,
 * strides multiples of 4, pointers 16-byte aligned, K in [1, 8]. */
int rb_session_capture(const float* u, int64_t u_rs, const float* xc, int64_t xc_rs,
                       const float* rg, int64_t rg_rs, const float* lam, const float* gate_b,
                       const float* carries, const int64_t* seq_offsets, const int64_t* slots,
                       float* h, float* conv_state, int64_t B, int64_t L, int64_t N, int64_t H,
                       int64_t K, void* stream);

/* The item ring: ring [N, S] int64 holds per slot the last min(count, S) item
 * ids the encoder kernels consumed, event e of a slot since its reset (e from
 * 0: count before the event) at ring[slot, e % S]; entries never written hold
 * what the caller initialised them to (python: -1).  The ring has no counter
 * of its own: count [N] is read, never written, so this kernel MUST be
 * launched on the same stream BEFORE the rb_session_step / rb_session_append
 * launches that consume the same items (they advance count), once per call
 * over the call's whole matrix.
 * items [B, W] int64, row-major, right-padded with 0: the matrix whose
 * RB_SESSION_TILE-column chunks the caller feeds to rb_session_append one
 * launch each (W = 1: the items of one rb_session_step).  W may be 0 (items
 * may then be NULL): nothing is recorded and only seen is written.  slots as
 * for the step (unique; NULL = slot b).  What is recorded is the encoder
 * kernels' own masking rule, restated per row from items, slots, N and V
 * alone.  Cut the row into chunks of RB_SESSION_TILE columns; a chunk's
 * events are its entries before its first 0; if any of them lies outside
 * [0, V) the chunk contributes nothing (the launch's BAD_ITEM), otherwise its
 * events are recorded in order; a slot outside [0, N) records nothing.  With
 * the row's recorded events numbered j = 0 .. n - 1, event j goes to
 * ring[slot, (count[slot] + j) % S]; when n > S only the last S are written,
 * and every ring entry is written at most once per launch (two passes over
 * the row: count, then write), so no result rests on the order of two stores.
 * seen [B, S] (optional): row b receives the slot's ring as it stands after
 * this call's events, in ring order, built from the old ring values and the
 * call's events (the launch's own stores are not read back); all -1 for a
 * slot outside [0, N).  It is the exclusion list rb_item_topk takes.
 * Every id and slot is range-checked before an address is formed from it.
 * One wave per call row; no atomics, LDS or scratch.  B, N, S, V >= 1,
 * W >= 0, all < 2^31. */
int rb_session_record(const int64_t* items, int64_t B, int64_t W, const int64_t* slots,
                      const int64_t* count, int64_t* ring, int64_t* seen,
                      int64_t N, int64_t S, int64_t V, void* stream);

/* Parked sessions.  A slot's whole state leaves the session state as one row
 * of 4-byte words (a blob row; python: a row of an int32 [B, W] tensor) and
 * comes back later, into any slot of a state of the same shape.  Everything is
 * copied bit for bit, nothing is converted.  The row, W = row_words words:
 *   word 0          the tag: the caller's 32-bit fingerprint of the format
 *                   number (RB_SESSION_BLOB_FORMAT) and the model shape, never
 *                   0 (python: SessionState.blob_tag); 0 marks an invalid row
 *   word 1          0 (reserved)
 *   words 2-3       count[slot], int64, low word first
 *   next d          out[slot]
 *   per layer, in   h[slot] (H words), then conv_state[slot] ((K - 1) H words,
 *   order           oldest row first; absent without has_conv or with K == 1)
 *   next 2 S        the item ring ring[slot, 0 .. S) in ring order (raw
 *                   positions), int64 each, low word first; absent with S == 0
 *   pad             zeros up to a multiple of 4 words
 * rb_session_blob_words returns W (RB_EINVAL for d or H outside [1, 2^20], K
 * outside [1, 8], n_layers outside [1, 8] or S outside [0, 2^31)).  The
 * format holds for every d and H; rb_session_transfer takes multiples of 4. */
int64_t rb_session_blob_words(int64_t d, int64_t H, int64_t K, int64_t n_layers, int64_t S,
                              int has_conv);

/* Park, resume or exchange B sessions in one launch.  Call row b names slot
 * slots[b] (slots NULL: slot b; slots unique, as for the step).  Of each
 * rb_session_layer only h, conv_state and h0 are read: the weight pointers
 * may be NULL.  ring [N, S] is the item ring (NULL with S == 0).
 *   blob_out given (park): the slot's state is written to row b of blob_out
 *   [B, row_words] in the format above, with `tag` in word 0.  A slot outside
 *   [0, N) gives an all-zero row and status RB_SESSION_BAD_SLOT.
 *   blob_in given (resume): row b of blob_in is checked as a whole: word 0
 *   must equal tag, count must be >= 0 and every ring entry must lie in
 *   [-1, V).  A row that passes replaces the slot's h, conv_state, count, out
 *   and ring (status RB_SESSION_MOVED); a row that fails leaves the slot
 *   untouched (status RB_SESSION_BAD_BLOB).
 *   both (exchange): the old state goes out and the new one comes in; each
 *   element's old value is read before the same thread writes its new one,
 *   so row b of blob_out is the state before the call whatever blob_in holds
 *   (a rejected row still parks the old state).  blob_in and blob_out must
 *   not overlap.
 *   release != 0 (blob_in NULL): after the export the slot is left as a reset
 *   leaves it: h = h0 (zeros when h0 is NULL), conv_state 0, count 0, out 0,
 *   ring -1.  release with blob_in, and neither blob without release, are
 *   argument errors.
 * status [B] int32 (optional): RB_SESSION_MOVED for a row that was parked,
 * released or resumed, RB_SESSION_BAD_SLOT, or RB_SESSION_BAD_BLOB (a bad
 * slot wins: its blob row is not examined).
 * The kernel's rules: every slot is range-checked before an address is formed
 * from it; a row's validity is decided (from blob_in's header and all of its
 * ring) before the first store to its slot; every branch on slot or validity
 * is wave-uniform;
 * no atomics and no scratch; no location is written twice in a launch; no
 * other slot is written.  One workgroup of 256 threads per call row (a row is
 * 12 to a few thousand words: up to a few 16-byte sweeps of the workgroup).
 * The float parts move in 16-byte accesses, so d and H are multiples of 4,
 * out, h, conv_state, h0 and both blobs 16-byte aligned and row_words a
 * multiple of 4 (it must equal rb_session_blob_words); the ring and count
 * move in 8-byte accesses, as a ring row is only 8-byte aligned when S is odd.
 * Status and argument checks come before any HIP call.  B, N, V >= 1, S >= 0,
 * all < 2^31; K in [1, 8]; n_layers in [1, RB_SESSION_MAX_LAYERS]. */
int rb_session_transfer(const rb_session_layer* layers, int64_t n_layers, int64_t* count,
                        float* out, int64_t* ring, const int64_t* slots,
                        const int32_t* blob_in, int32_t* blob_out, int32_t* status,
                        int tag, int release, int64_t B, int64_t N, int64_t V, int64_t d,
                        int64_t H, int64_t K, int64_t S, int has_conv, int64_t row_words,
                        void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RECBLR_SESSION_H */

"""Scoring sequence representations against the whole item table.

RecBLR.calculate_loss with loss_type "CE" (RecBLR.py:100-102) multiplies the
[B, d] sequence representations by the [V, d] item table and applies
nn.CrossEntropyLoss; full_sort_predict (RecBLR.py:114-122) returns the same
[B, V] score matrix, which RecBole's evaluator (and run_with_unseen.py:229-265)
reduces to the rank of each row's target item.  Here both run on the MFMA
kernels of csrc/item_scores.hip without materialising [B, V] — the training
CE on the f16 pipe with two-part split operands (fp32-level accuracy,
RECBLR_CE_PIPE), ranking and scores on the fp32 pipe:

  * item_cross_entropy: forward computes the per-row log-sum-exp tile by
    tile; backward recomputes the logits and forms dseq = P W and
    ditems = P^T seq from P = softmax - onehot in registers;
  * item_cross_entropy_rows: the same loss over many rows (every position
    of the packed batch, RecBLR.calculate_loss_dense) in row chunks, rows
    with target -1 ignored; at most one chunk's P is ever stored;
  * pair_loss: the sampled pairwise (BPR) loss of many rows against each
    row's target and its sampled negatives only (csrc/pair_loss.hip;
    RecBLR.calculate_loss_pairs) — no sweep over the table at all;
  * shared_softmax_loss: the sampled softmax of the packed rows against each
    row's target and n negatives shared by the rows of a sequence
    (csrc/shared_softmax.hip; RecBLR.calculate_loss_sampled) — one small
    fp32 MFMA product per sequence;
  * target_ranks: per row, the number of items scoring above / equal to the
    target, from which Hit@k, MRR@k and NDCG@k follow exactly;
  * full_sort_scores: the score matrix itself when a caller needs it;
  * top_items: each row's k best items (a recommendation list), with
    seen-item exclusion, selected inside the scoring kernel;
  * item_filters: catalogue filters as bitmaps (ItemFilters), which top_items
    and target_ranks take per row (allow, allow_rows): one filter word per
    32-item tile of the sweep, ANDed into the tile's pass mask.

And against chosen items only (csrc/candidates.hip: a 16-lane group per (row,
id), no [B, C, d] gather, no sweep over the table):

  * candidate_scores: [B, C] scores of each row's own candidate ids;
  * top_candidates: a row's candidate list ordered by the model (reranking),
    scored, filtered, sorted and written by one launch; order_candidates is
    its selection rule alone, in torch ops;
  * candidate_ranks: the target's rank among a row's sampled negatives.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import kernels, linear
from .linear import _timed

__all__ = ["item_cross_entropy", "item_cross_entropy_rows", "full_sort_scores", "target_ranks", "rank_metrics",
           "top_items", "supported", "pair_loss", "pair_loss_reference", "shared_softmax_loss",
           "shared_softmax_reference", "candidate_scores",
           "order_candidates", "top_candidates", "candidate_ranks", "ItemFilters", "item_filters",
           "ItemGroups", "item_groups", "ItemPriors", "item_priors", "log_popularity"]


def supported(seq: torch.Tensor, table: torch.Tensor) -> bool:
    return (seq.is_cuda and seq.dtype == torch.float32 and table.dtype == torch.float32
            and seq.dim() == 2 and seq.shape[-1] in kernels.ITEM_DIMS)


# Backward strategy: "slices" writes the logits' gradient P one item slice at
# a time (rb_item_ce_probs, at most PROBS_SLICE_BYTES) and runs dseq += P W,
# ditems = P^T seq as library GEMMs; "fused" (rb_item_ce_bwd) recomputes the
# logits inside the MFMA kernels (fp32 pipe) and needs no [B, V] buffer at all;
# its forward runs on the fp32 pipe as well, whatever CE_PIPE says.
def _env_choice(name: str, default: str, allowed: tuple) -> str:
    """An environment switch checked at import: a value outside `allowed`
    raises instead of silently selecting another path."""
    v = os.environ.get(name, default)
    if v not in allowed:
        raise ValueError(f"{name}={v!r}: expected one of {allowed}")
    return v


CE_BACKWARD = _env_choice("RECBLR_CE_BACKWARD", "slices", ("slices", "fused"))
PROBS_SLICE_BYTES = 1 << 30
# Logits pipe of the CE forward and of the sliced backward's P: "f16" (two-part
# split operands on the f16 MFMA, fp32-level accuracy; default) or "f32".
CE_PIPE = _env_choice("RECBLR_CE_PIPE", "f16", ("f16", "f32"))
# The backward's two products dseq = P W, ditems = P^T seq: "f16" (default:
# P written in both layouts, both products on the f16x3 weight-gradient
# kernel, _bwd_f16) or "torch" (hipBLASLt fp32 on P, sliced).  Measured and
# removed: an f16 variant running ditems as the NT kernel on P^T (2.2x
# slower: 42 row tiles with K = 2048 and online row scales that P^T's rows
# outgrow; profiles/r03_ce_grads_probe.log), and rb_item_ce_bwd_h (round 4:
# each product inside a kernel that recomputes the logits, P never stored —
# equal step time, profiles/r04_ce_bench_*.log; in git history up to round 4).
CE_GRADS = _env_choice("RECBLR_CE_GRADS", "f16", ("f16", "torch"))


def set_ce_grads(mode: str) -> str:
    """Set the backward's product strategy (bench A/B); returns the previous one."""
    global CE_GRADS
    if mode not in ("f16", "torch"):
        raise ValueError(mode)
    prev, CE_GRADS = CE_GRADS, mode
    return prev


# rb_gemm_tn_h's largest N and K (include/recblr_hip.h); ditems runs with N =
# the item count rounded up to 256
GEMM_TN_MAX_N = 65536


def _tn_splits8(dev, nt: int, div: int = 1) -> int:
    """linear._tn_splits(dev, nt) // div rounded down to a multiple of 8
    (rb_gemm_tn_h takes row splits in multiples of 8), at least 8."""
    return max(8, linear._tn_splits(dev, nt) // div // 8 * 8)


def _f16_grads_ok(seq, table, rows: int | None = None) -> bool:
    """The logits' input gradients as f16x3 GEMMs (_f16_products): B a multiple
    of 256 (the weight-gradient kernel's N; its row splits), d of 128, both
    layouts of P within twice PROBS_SLICE_BYTES, the padded item count within
    the weight-gradient kernel's N limit.  rows: P's row count B when it is not
    seq's (_ItemCERows: one chunk)."""
    B, d = seq.shape
    if rows is not None:
        B = rows
    V = table.shape[0]
    return (CE_GRADS == "f16" and linear.gemm_format() == "f16x3" and B % 256 == 0
            and d % 128 == 0 and table.stride(1) == 1 and table.data_ptr() % 16 == 0
            and 8 * B * V <= 2 * PROBS_SLICE_BYTES
            and (V + 255) // 256 * 256 <= GEMM_TN_MAX_N)


# RECBLR_CE_ROUND_SPLITS=0: the item-table product's split count as round 5
# chose it (a multiple of 8; A/B)
_ROUND_SPLITS = _env_choice("RECBLR_CE_ROUND_SPLITS", "1", ("0", "1")) == "1"


def _round_splits(dev, nt: int, rows: int) -> int:
    """Split count for a weight-gradient product of nt one-per-CU tiles over
    `rows` rows: the fewest (launch rounds x 32-row steps per workgroup, + 3
    steps of fixed cost); the smallest such count (fewer partials to sum).
    The item table's product at B = 2,048: 42 tiles x 6 splits in one round
    instead of 8 splits in 1.3."""
    n = linear._num_cus(dev)
    best, best_cost = 1, None
    for s in range(1, max(1, rows // 32) + 1):
        cost = -(-nt * s // n) * (-(-(-(-rows // s)) // 32) + 3)
        if best_cost is None or cost < best_cost:
            best, best_cost = s, cost
    return best


def _group_max(x: torch.Tensor) -> torch.Tensor:
    """max |x| over each 32-row group of a [n, c] tensor (a partial last group
    too): the weight-gradient kernel's operand scale."""
    m = x.abs().amax(1)
    return F.pad(m, (0, (-m.numel()) % 32)).view(-1, 32).amax(1)


def _batch_splits(dev, nt: int, rows: int) -> int:
    """_round_splits, or round 5's count under RECBLR_CE_ROUND_SPLITS=0."""
    if _ROUND_SPLITS:
        return _round_splits(dev, nt, rows)
    return max(8, min(_tn_splits8(dev, nt), rows // 256 // 8 * 8))


def _f16_products(probs, rows, rmax, table, tmax, want_seq, want_items, splits):
    """(drows [n, d], dtable [V, d]) from probs = (P [n, Vp], P^T [V, n], bmax,
    gmax) of one rb_item_ce_probs_h_both* pass, both as the f16x3
    weight-gradient GEMM (rb_gemm_tn_h, fixed-order row-chunk partials, a
    column sum): dtable = P^T rows reduced over P's rows, drows = P table over
    P^T's item rows — no library GEMM.  rmax / tmax: the 32-row group maxima of
    rows / table (None: computed here); splits(dev, nt, n): the split count of
    the table's product."""
    p, pt, bmax, gmax = probs
    n, d = rows.shape
    V = table.shape[0]
    fl = 2 * n * V * d
    drows = dtable = None
    if want_items:
        Vp = p.shape[1]
        S1 = splits(rows.device, (Vp // 256) * (d // 128), n)
        if rmax is None:
            rmax = kernels.group_absmax(rows)
        parts = _timed("gemm", fl, kernels.gemm_tn_h, p, rows, bmax, rmax, S1)
        dtable = kernels.colsum(parts.view(S1, -1)).view(Vp, d)[:V]
    if want_seq:
        S2 = _tn_splits8(rows.device, (n // 256) * (d // 128), div=2)
        if tmax is None:
            tmax = kernels.group_absmax(table)
        parts = _timed("gemm", fl, kernels.gemm_tn_h, pt, table, gmax, tmax, S2)
        drows = kernels.colsum(parts.view(S2, -1)).view(n, d)
    return drows, dtable


def _bwd_f16(seq, table, target, lse, dloss, want_seq, want_items, split):
    """The logits' gradient in both layouts from one pass
    (rb_item_ce_probs_h_both) and both input gradients from it (_f16_products)."""
    s_seq, s_tab = split
    probs = kernels.item_ce_probs_h_both(s_seq, s_tab, target, lse, dloss, pad_to=256)
    return _f16_products(probs, seq, s_seq.gmax, table, s_tab.gmax, want_seq, want_items,
                         _batch_splits)


def _bwd_slices(seq, table, target, lse, dloss, want_seq, want_items, split=None):
    B, d = seq.shape
    V = table.shape[0]
    vc = max(32, min(V, PROBS_SLICE_BYTES // (4 * B)))
    dseq = dtable = None
    if want_items:
        dtable = torch.empty_like(table)
    for v0 in range(0, V, vc):
        rows = table[v0:v0 + vc]
        if split is not None:   # the forward's split images: bit-identical logits
            s_seq, s_tab = split
            p = kernels.item_ce_probs_h(s_seq, s_tab.rows(v0, v0 + vc), target, lse, dloss,
                                        item_offset=v0)
        else:
            p = kernels.item_ce_probs(seq, rows, target, lse, dloss, item_offset=v0)
        fl = 2 * B * rows.shape[0] * d
        if want_seq:   # slices accumulate in a fixed order
            dseq = (_timed("gemm", fl, torch.mm, p, rows) if dseq is None
                    else _timed("gemm", fl, dseq.addmm_, p, rows))
        if want_items:
            _timed("gemm", fl, torch.mm, p.t(), seq, out=dtable[v0:v0 + vc])
    return dseq, dtable


class _ItemCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, seq, table, target):
        seq, table = seq.contiguous(), table.contiguous()
        # The fused backward (rb_item_ce_bwd) recomputes the logits on the fp32
        # pipe only, so its forward runs there too: P = exp(x - lse) - onehot
        # needs x and lse from the same logits.  With the f16 pipe's lse a
        # confident row (1 - p ~ 1e-2) lost 9x the accuracy of every other path
        # (tests/test_gpu_item_ce_ref.py, peaked 600 x 4100 x 128).
        ctx.fused = CE_BACKWARD == "fused"
        if CE_PIPE == "f16" and not ctx.fused:
            # the split also gives the 32-row group maxima the f16 backward's
            # weight-gradient GEMMs scale these operands by
            s_seq = kernels.item_split_h(seq, group_max=True)
            s_tab = kernels.item_split_h(table, group_max=True)
            loss, lse = kernels.item_ce_fwd_h(s_seq, s_tab, target)
            ctx.split = (s_seq, s_tab)
        else:
            loss, lse = kernels.item_ce_fwd(seq, table, target)
            ctx.split = None
        ctx.save_for_backward(seq, table, target, lse)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        seq, table, target, lse = ctx.saved_tensors
        want_seq, want_items = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if ctx.fused:   # as the forward chose: the same logits on both sides
            dseq, dtable = kernels.item_ce_bwd(seq, table, target, lse, dloss.float(),
                                               want_seq=want_seq, want_items=want_items)
        elif ctx.split is not None and _f16_grads_ok(seq, table):
            dseq, dtable = _bwd_f16(seq, table, target, lse, dloss.float(), want_seq,
                                    want_items, ctx.split)
        else:
            dseq, dtable = _bwd_slices(seq, table, target, lse, dloss.float(), want_seq,
                                       want_items, split=ctx.split)
        ctx.split = None
        return dseq, dtable, None


def item_cross_entropy(seq: torch.Tensor, table: torch.Tensor,
                       target: torch.Tensor) -> torch.Tensor:
    """nn.CrossEntropyLoss()(seq @ table.T, target) without the [B, V] logits."""
    if not supported(seq, table):
        return F.cross_entropy(seq @ table.t(), target)
    return _ItemCE.apply(seq, table, target)


# ---- the same loss over many rows, some of them ignored ----------------------------
CE_ROWS_ALIGN = 256   # rb_gemm_tn_h's N: a chunk's rows are a multiple of it


class _ItemCERows(torch.autograd.Function):
    """seq [Mp, d] (Mp a multiple of 256, padding rows zero with target -1),
    table [V, d], target [Mp] in [0, V) or -1; inv_n = 1 / live rows."""

    @staticmethod
    def forward(ctx, seq, table, target, chunk_rows, inv_n):
        seq, table = seq.contiguous(), table.contiguous()
        Mp = seq.shape[0]
        s_seq = kernels.item_split_h(seq, group_max=True)
        s_tab = kernels.item_split_h(table, group_max=True)   # once for every chunk
        lse = torch.empty((Mp,), device=seq.device, dtype=torch.float32)
        loss = torch.empty((), device=seq.device, dtype=torch.float32)
        # the chunks' partial sums are added to loss in chunk order (stream order)
        for r0 in range(0, Mp, chunk_rows):
            r1 = min(r0 + chunk_rows, Mp)
            kernels.item_ce_fwd_h_rows(s_seq.rows(r0, r1), s_tab, target[r0:r1], inv_n,
                                       lse[r0:r1], loss, accumulate=r0 > 0)
        ctx.split = (s_seq, s_tab)
        ctx.chunk_rows, ctx.inv_n = chunk_rows, inv_n
        ctx.save_for_backward(seq, table, target, lse)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        seq, table, target, lse = ctx.saved_tensors
        want_seq, want_items = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        s_seq, s_tab = ctx.split
        ctx.split = None
        chunk, inv_n = ctx.chunk_rows, ctx.inv_n
        Mp, d = seq.shape
        V = table.shape[0]
        dloss = dloss.float()
        # both of a chunk's products on rb_gemm_tn_h, as in _ItemCE; other
        # supported d: one library GEMM pair per chunk.  (chunk is a multiple
        # of 256 and table contiguous: item_cross_entropy_rows, forward)
        f16 = _f16_grads_ok(seq, table, rows=chunk)
        dseq = torch.empty_like(seq) if want_seq else None
        dtable = None
        # chunk by chunk in row order: P of one chunk at a time, dtable summed
        # in that fixed order
        for r0 in range(0, Mp, chunk):
            r1 = min(r0 + chunk, Mp)
            n = r1 - r0
            rows, tgt, l = seq[r0:r1], target[r0:r1], lse[r0:r1]
            sr = kernels.SplitRows(s_seq.img[r0:r1], s_seq.exps[r0:r1])
            fl = 2 * n * V * d
            if f16:
                probs = kernels.item_ce_probs_h_both_rows(sr, s_tab, tgt, l, dloss, inv_n,
                                                          pad_to=256)
                dr, dt = _f16_products(probs, rows, s_seq.gmax[r0 // 32:r1 // 32], table,
                                       s_tab.gmax, want_seq, want_items, _round_splits)
                if want_items:
                    dtable = dt.contiguous() if dtable is None else dtable.add_(dt)
                if want_seq:
                    dseq[r0:r1] = dr
            else:
                p = kernels.item_ce_probs_h_rows(sr, s_tab, tgt, l, dloss, inv_n)
                if want_seq:
                    _timed("gemm", fl, torch.mm, p, table, out=dseq[r0:r1])
                if want_items:
                    dtable = (_timed("gemm", fl, torch.mm, p.t(), rows) if dtable is None
                              else _timed("gemm", fl, dtable.addmm_, p.t(), rows))
        return dseq, dtable, None, None, None


def item_cross_entropy_rows(seq: torch.Tensor, table: torch.Tensor, target: torch.Tensor,
                            chunk_rows: int = 2048, n_live: int | None = None) -> torch.Tensor:
    """F.cross_entropy(seq @ table.T, target, ignore_index=-1) for many rows
    without the [M, V] logits: the mean of lse - target score over the live
    rows (target in [0, V)); a row with target -1 is ignored (no loss, zero
    gradient; its seq values must be finite); any other target gives NaN.

    The rows are walked in chunks of chunk_rows (a multiple of 256; 2048 is
    the shape the CE kernels are measured at) on the f16-pipe CE kernels'
    rows variants; the backward stores one chunk's P at a time and sums the
    table's gradient over the chunks in row order (deterministic).  With d a
    multiple of 128 and the f16x3 GEMM format both products of a chunk run on
    rb_gemm_tn_h (no library GEMM); other d in kernels.ITEM_DIMS use one
    library GEMM pair per chunk.  M is padded to a multiple of 256 with zero
    rows and -1 targets; a caller that already holds such a buffer
    (RecBLR.forward_all) passes it as it is and nothing is copied.
    n_live: the number of live rows when the caller knows it on the host (no
    sync); otherwise it is counted on the device (one sync).  No live row:
    loss 0 and zero gradients.  CPU tensors, other dtypes and other d take
    the plain torch expression above."""
    chunk_rows = int(chunk_rows)
    if chunk_rows < CE_ROWS_ALIGN or chunk_rows % CE_ROWS_ALIGN:
        raise ValueError(f"chunk_rows = {chunk_rows} must be a positive multiple of {CE_ROWS_ALIGN}")
    if seq.dim() != 2 or target.shape != (seq.shape[0],):
        raise ValueError(f"seq [M, d] and target [M] required, got {tuple(seq.shape)} and "
                         f"{tuple(target.shape)}")
    if n_live is None:
        n_live = int((target != -1).sum())
    if n_live <= 0:   # nothing to average: 0 with zero gradients
        return (seq.sum() + table.sum()) * 0.0
    if not supported(seq, table):
        return F.cross_entropy(seq @ table.t(), target, ignore_index=-1)
    M = seq.shape[0]
    pad = -M % CE_ROWS_ALIGN
    if pad:
        seq = F.pad(seq, (0, 0, 0, pad))
        target = F.pad(target, (0, pad), value=-1)
    return _ItemCERows.apply(seq, table, target.contiguous(), chunk_rows, 1.0 / n_live)


def pair_loss_reference(h: torch.Tensor, table: torch.Tensor, pos: torch.Tensor,
                        neg: torch.Tensor, gamma: float = 1e-10) -> torch.Tensor:
    """pair_loss in torch ops, any device and dtype: the CPU path and the
    fallback for a d the kernels refuse.  An id outside [-1, V) gives NaN."""
    V = table.shape[0]
    live = (pos >= 0)[:, None] & (neg >= 0)
    bad = ((pos < -1) | (pos >= V))[:, None] | (neg < -1) | (neg >= V)
    ps = (h * table[pos.clamp(0, V - 1)]).sum(-1)
    ns = (h[:, None, :] * table[neg.clamp(0, V - 1)]).sum(-1)
    l = -torch.log(gamma + torch.sigmoid(ps[:, None] - ns))
    l = torch.where(live & ~bad, l, torch.zeros_like(l))
    loss = l.sum() / live.sum().clamp(min=1)
    return torch.where(bad.any(), torch.full_like(loss, float("nan")), loss)


class _PairLoss(torch.autograd.Function):
    """h [M, d], table [V, d], pos [M], neg [M, n]: the forward saves diff and
    plans the table's scatter (index work only); the backward is the
    coefficient kernel and the scaled apply."""

    @staticmethod
    def forward(ctx, h, table, pos, neg, gamma):
        table = table.contiguous()
        if h.stride(1) != 1 or h.stride(0) % 4 or h.data_ptr() % 16:
            h = h.contiguous()
        pos, neg = pos.contiguous(), neg.contiguous()
        loss, n_live, diff = kernels.pair_loss_fwd(h, table, pos, neg, gamma)
        ctx.plan = None
        if ctx.needs_input_grad[1]:   # ids [pos | neg_0 | neg_1 ...], one block of M each
            ids = torch.cat([pos, neg.t().reshape(-1)])
            ctx.plan = kernels.embedding_plan(ids, table.shape[0], table.shape[1])
        ctx.gamma = gamma
        ctx.save_for_backward(h, table, pos, neg, diff, n_live)
        ctx.mark_non_differentiable(n_live)
        return loss, n_live

    @staticmethod
    def backward(ctx, dloss, _):
        h, table, pos, neg, diff, n_live = ctx.saved_tensors
        plan, ctx.plan = ctx.plan, None
        dh, coef = kernels.pair_loss_bwd(table, pos, neg, diff, dloss.float().contiguous(),
                                         n_live, ctx.gamma)
        dtable = None
        if plan is not None:
            dtable = kernels.embedding_bwd_scaled(coef, h, table.shape[0], plan)
        return (dh if ctx.needs_input_grad[0] else None), dtable, None, None, None


def pair_loss(h: torch.Tensor, table: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor,
              gamma: float = 1e-10, return_live: bool = False) -> torch.Tensor:
    """The sampled pairwise (BPR) loss of rows h [M, d] against table [V, d]:
    the mean over the live pairs (r, j) of

        -log(gamma + sigmoid(h_r . table[pos_r] - h_r . table[neg_rj]))

    with pos [M] and neg [M, n] int64; pos_r = -1 ignores row r and neg_rj =
    -1 pair (r, j) (no loss, exactly zero gradient); any other id outside [0,
    V) gives NaN.  No live pair: loss 0 and zero gradients.  With n = 1 and
    every pair live this is RecBole's BPRLoss (gamma 1e-10) on the pairs.
    Only (2 + n) rows of d floats are read per row of h; the table's gradient
    goes through the embedding backward's deterministic plan with its
    gradient rows formed on the fly (rb_embedding_bwd_apply_scaled), so the
    result is bitwise reproducible.  return_live: also the live-pair count (a
    device scalar, no sync).  CPU tensors, other dtypes and a d that is no
    multiple of 4 up to 512 take pair_loss_reference."""
    if h.dim() != 2 or pos.shape != (h.shape[0],) or neg.dim() != 2 or neg.shape[0] != h.shape[0]:
        raise ValueError(f"h [M, d], pos [M] and neg [M, n] required, got {tuple(h.shape)}, "
                         f"{tuple(pos.shape)} and {tuple(neg.shape)}")
    n = neg.shape[1]
    if not 1 <= n <= kernels.MAX_NEGATIVES:
        raise ValueError(f"n = {n} negatives per row: expected 1 .. {kernels.MAX_NEGATIVES}")
    pos, neg = pos.to(torch.int64), neg.to(torch.int64)
    if not kernels.pair_loss_supported(h, table):
        loss = pair_loss_reference(h, table, pos, neg, gamma)
        return (loss, ((pos >= 0)[:, None] & (neg >= 0)).sum()) if return_live else loss
    loss, n_live = _PairLoss.apply(h, table, pos, neg, float(gamma))
    return (loss, n_live) if return_live else loss


def shared_softmax_reference(h: torch.Tensor, table: torch.Tensor, target: torch.Tensor,
                             neg: torch.Tensor, offsets: torch.Tensor, order: torch.Tensor,
                             shift: float = 0.0, item_shift: torch.Tensor | None = None
                             ) -> torch.Tensor:
    """shared_softmax_loss in torch ops, any device and dtype: the CPU path,
    the fallback for shapes the kernels refuse, and the tests' reference.  The
    sequences are padded to the longest one and scored against their own
    lists with one batched product.  item_shift [V] is added after shift, as
    the kernels add it, in the scores' dtype; it takes no gradient."""
    V, (B, n) = table.shape[0], neg.shape
    lens = offsets[1:] - offsets[:-1]
    rows = torch.arange(int(offsets[0]), int(offsets[-1]), device=h.device)
    if rows.numel() == 0:
        return (h.sum() + table.sum()) * 0.0
    seq_of = torch.repeat_interleave(torch.arange(B, device=h.device), lens)
    t_in = rows - offsets[seq_of]
    hr, tr = h[rows], target[rows]
    padded = hr.new_zeros((B, int(lens.max()), h.shape[1])).index_put((seq_of, t_in), hr)
    lists = neg[order]                                       # [B, n], packed-sequence order
    col_ok = (lists >= 0) & (lists < V)
    z = torch.bmm(padded, table[lists.clamp(0, V - 1)].transpose(1, 2))[seq_of, t_in] + shift
    if item_shift is not None:
        z = z + item_shift.detach().to(z.dtype)[lists.clamp(0, V - 1)][seq_of]
    z = torch.where(col_ok[seq_of], z, torch.full_like(z, float("-inf")))
    row_ok = (tr >= 0) & (tr < V)
    z0 = (hr * table[tr.clamp(0, V - 1)]).sum(-1)
    l = torch.logsumexp(torch.cat([z0[:, None], z], 1), 1) - z0
    loss = torch.where(row_ok, l, torch.zeros_like(l)).sum() / row_ok.sum().clamp(min=1)
    bad = ((tr < -1) | (tr >= V)).any() | ((neg < -1) | (neg >= V)).any()
    return torch.where(bad, torch.full_like(loss, float("nan")), loss)


class _SharedSoftmax(torch.autograd.Function):
    """h [M, d], table [V, d], target [M], neg [B, n] and the pack plan: the
    forward saves lse and plans the table's two scatters (index work only);
    the backward is the two gradient kernels, the scaled apply over the
    targets and the plain apply of dneg over the lists."""

    @staticmethod
    def forward(ctx, h, table, target, neg, offsets, order, shift, max_len, item_shift=None):
        table = table.contiguous()
        if h.stride(1) != 1 or h.stride(0) % 4 or h.data_ptr() % 16:
            h = h.contiguous()
        target, neg = target.contiguous(), neg.contiguous()
        offsets, order = offsets.contiguous(), order.contiguous()
        loss, n_live, lse, _ = kernels.shared_softmax_fwd(h, table, target, neg, offsets, order,
                                                          shift, max_len, item_shift)
        ctx.plans = None
        if ctx.needs_input_grad[1]:
            V, d = table.shape
            ctx.plans = (kernels.embedding_plan(target, V, d),
                         kernels.embedding_plan(neg.reshape(-1), V, d))
        ctx.shift, ctx.max_len, ctx.item_shift = shift, max_len, item_shift
        ctx.save_for_backward(h, table, target, neg, offsets, order, lse, n_live)
        ctx.mark_non_differentiable(n_live)
        return loss, n_live

    @staticmethod
    def backward(ctx, dloss, _):
        h, table, target, neg, offsets, order, lse, n_live = ctx.saved_tensors
        plans, ctx.plans = ctx.plans, None
        dh, coef, dneg = kernels.shared_softmax_bwd(h, table, target, neg, offsets, order, lse,
                                                    dloss.float().contiguous(), n_live,
                                                    ctx.shift, ctx.max_len, ctx.item_shift)
        dtable = None
        if plans is not None:
            V, d = table.shape
            dtable = kernels.embedding_bwd_scaled(coef, h, V, plans[0])
            dtable += kernels.embedding_bwd(neg.reshape(-1), dneg.reshape(-1, d), V,
                                            padding_idx=None, plan=plans[1])
        return ((dh if ctx.needs_input_grad[0] else None), dtable, None, None, None, None, None,
                None, None)


def shared_softmax_loss(h: torch.Tensor, table: torch.Tensor, target: torch.Tensor,
                        neg: torch.Tensor, offsets: torch.Tensor, order: torch.Tensor,
                        shift: float = 0.0, return_live: bool = False, *,
                        max_len: int | None = None, item_shift: torch.Tensor | None = None):
    """Sampled softmax of the packed rows h [M, d] against table [V, d] with
    the negatives shared by the rows of a sequence: neg [B, n] holds one list
    per batch row, and packed sequence s (rows offsets[s] .. offsets[s + 1])
    is batch row order[s].  For row r of batch row b

        z0 = h_r . table[target_r],  z_j = h_r . table[neg[b, j]] + shift
        loss_r = logsumexp(z0, z_j ...) - z0

    and the loss is the mean of loss_r over the live rows.  target_r = -1
    ignores row r (no loss, exactly zero gradient) and neg[b, j] = -1 is a
    dead column; any other id outside [0, V) gives NaN.  No live row: loss 0
    and zero gradients; a live row without a live column has loss 0 and counts.
    A repeated id counts once per occurrence, and a column may equal a row's
    target.  shift is the log-Q correction of the proposal (log((V' - 1) / n)
    for n uniform draws over V' items makes sum_j exp(z_j) an estimate of the
    full softmax's sum over the non-targets).  The scores of a sequence are
    one product on the exact-fp32 MFMA and no [M, n] matrix is stored; the
    table's gradient goes through the embedding backward's deterministic plan,
    so the result is bitwise reproducible.  return_live: also the live-row
    count (a device scalar, no sync).  max_len: an upper estimate of the
    longest sequence (it sizes the launch; without it the lengths are read
    back once).  item_shift [V]: a per-item correction for a proposal that is
    not uniform — a column of id j scores z_j = (h_r . table[j] + shift) +
    item_shift[j]; with ids drawn with probability q_j (kernels.
    negative_sampler), shift = -log(n) and item_shift = -log(q) generalise the
    uniform formula.  It takes no gradient and is read only at the live
    columns' ids.  CPU tensors, other dtypes, d no multiple of 16 up to 224 and
    n > 256 take shared_softmax_reference."""
    if (h.dim() != 2 or target.shape != (h.shape[0],) or neg.dim() != 2 or neg.shape[1] < 1
            or offsets.shape != (neg.shape[0] + 1,) or order.shape != (neg.shape[0],)):
        raise ValueError(f"h [M, d], target [M], neg [B, n >= 1], offsets [B + 1] and order [B] "
                         f"required, got {tuple(h.shape)}, {tuple(target.shape)}, "
                         f"{tuple(neg.shape)}, {tuple(offsets.shape)} and {tuple(order.shape)}")
    target, neg = target.to(torch.int64), neg.to(torch.int64)
    offsets, order = offsets.to(torch.int64), order.to(torch.int64)
    if item_shift is not None and item_shift.shape != (table.shape[0],):
        raise ValueError(f"item_shift must be [V] = [{table.shape[0]}], got "
                         f"{tuple(item_shift.shape)}")
    if not kernels.shared_softmax_supported(h, table, neg.shape[1]):
        loss = shared_softmax_reference(h, table, target, neg, offsets, order, shift, item_shift)
        if not return_live:
            return loss
        covered = target[int(offsets[0]):int(offsets[-1])]
        return loss, ((covered >= 0) & (covered < table.shape[0])).sum()
    if max_len is None:
        max_len = int((offsets[1:] - offsets[:-1]).max())
    if item_shift is not None:
        item_shift = item_shift.detach().to(device=h.device, dtype=torch.float32).contiguous()
    loss, n_live = _SharedSoftmax.apply(h, table, target, neg, offsets, order, float(shift),
                                        int(max_len), item_shift)
    return (loss, n_live) if return_live else loss


def full_sort_scores(seq: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """seq @ table.T ([B, V]); the MFMA kernel when no gradient is needed."""
    if supported(seq, table) and not (torch.is_grad_enabled()
                                      and (seq.requires_grad or table.requires_grad)):
        return kernels.item_scores(seq, table)
    return seq @ table.t()


# ---- catalogue filters: allow-lists as bitmaps (include/recblr_filters.h) -----------
class ItemFilters:
    """F named allow-lists over a catalogue of n_items items, as bitmaps: words
    int32 [F, ceil(n_items / 32)] contiguous, bit i of word w of row f set iff
    filter f allows item 32 w + i (bit 31 is the sign bit), bits at or beyond
    n_items zero.  One word is one 32-item tile of the full-sort kernels, which
    AND it into the tile's pass mask (top_items, target_ranks; a request row
    picks its filter with allow_rows).  Built by item_filters."""

    __slots__ = ("words", "n_items")

    def __init__(self, words: torch.Tensor, n_items: int):
        n_items = int(n_items)
        if (words.dtype != torch.int32 or words.dim() != 2 or words.shape[0] < 1
                or n_items < 1 or words.shape[1] != (n_items + 31) // 32):
            raise ValueError(f"words must be int32 [F >= 1, ceil({n_items} / 32)], got "
                             f"{words.dtype} {tuple(words.shape)}")
        self.words = words.contiguous()
        self.n_items = n_items

    @property
    def n_filters(self) -> int:
        return self.words.shape[0]

    def to(self, device) -> "ItemFilters":
        """The same filters on `device` (itself when already there)."""
        words = self.words.to(device)
        return self if words is self.words else ItemFilters(words, self.n_items)

    def mask(self) -> torch.Tensor:
        """bool [F, n_items]: True where the filter allows the item."""
        bits = torch.arange(32, device=self.words.device, dtype=torch.int64)
        m = (self.words.to(torch.int64)[:, :, None] >> bits) & 1
        return m.view(self.n_filters, -1)[:, :self.n_items].bool()

    def count(self) -> torch.Tensor:
        """int64 [F]: allowed items per filter."""
        return self.mask().sum(1)


def item_filters(allowed, n_items: int | None = None, device=None) -> ItemFilters:
    """Filters as data: ItemFilters from a bool tensor [F, V], a bool tensor
    [V] (F = 1), or a sequence of F id sequences over n_items items (ids
    outside [0, n_items) raise ValueError; duplicates are fine).  Plain torch
    ops on the input's device; the words then move to `device`.  Rebuilding
    one filter after a stock change is this call on one [V] mask and a copy
    into words[f]."""
    if isinstance(allowed, torch.Tensor):
        if allowed.dtype != torch.bool or allowed.dim() not in (1, 2):
            raise ValueError(f"allowed must be a bool tensor [F, V] or [V], got {allowed.dtype} "
                             f"{tuple(allowed.shape)}")
        mask = allowed if allowed.dim() == 2 else allowed[None]
        if n_items is not None and int(n_items) != mask.shape[1]:
            raise ValueError(f"n_items = {n_items} but the mask covers {mask.shape[1]} items")
    else:
        if n_items is None:
            raise ValueError("id lists need n_items")
        lists = [torch.as_tensor(ids, dtype=torch.int64).reshape(-1) for ids in allowed]
        mask = torch.zeros((len(lists), int(n_items)), dtype=torch.bool)
        for f, ids in enumerate(lists):
            if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= int(n_items)):
                raise ValueError(f"filter {f}: ids must lie in [0, {int(n_items)})")
            mask[f, ids] = True
    F_, V = mask.shape
    if F_ < 1 or V < 1:
        raise ValueError(f"need at least one filter and one item, got {tuple(mask.shape)}")
    # bit i of a word through int64 (bit 31 set is 2^31), then wrapped into int32
    bits = F.pad(mask, (0, -V % 32)).view(F_, -1, 32).to(torch.int64)
    words = (bits << torch.arange(32, device=mask.device, dtype=torch.int64)).sum(-1)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
    return ItemFilters(words if device is None else words.to(device), V)


def _check_allow(allow, allow_rows, B: int, V: int, device):
    """top_items' and target_ranks' filter arguments -> (allow on `device`,
    allow_rows int64 [B] on `device` or None).  allow_rows is moved, not read:
    no sync and no range check (-1: no filter; a value outside [-1, F): the row
    selects nothing)."""
    if allow is None:
        if allow_rows is not None:
            raise ValueError("allow_rows without allow")
        return None, None
    if not isinstance(allow, ItemFilters):
        raise TypeError("allow must be an ItemFilters (scoring.item_filters)")
    if allow.n_items != V:
        raise ValueError(f"allow covers {allow.n_items} items, the table has {V}")
    if allow_rows is not None:
        if not isinstance(allow_rows, torch.Tensor) or allow_rows.shape != (B,):
            raise ValueError(f"allow_rows must be [B] = [{B}], got "
                             f"{tuple(getattr(allow_rows, 'shape', ()))}")
        allow_rows = allow_rows.to(device=device, dtype=torch.int64)
    return allow.to(device), allow_rows


def _allowed_mask(allow: ItemFilters, allow_rows, B: int) -> torch.Tensor:
    """bool [B, V]: what each row's filter allows, by the kernels' rule."""
    mask = allow.mask()
    if allow_rows is None:
        return mask[:1].expand(B, -1)
    n = allow.n_filters
    ok = mask[allow_rows.clamp(0, n - 1)] & ((allow_rows >= 0) & (allow_rows < n))[:, None]
    return ok | (allow_rows == -1)[:, None]


# ---- diversity caps: one group id per item (include/recblr_groups.h) ----------------
class ItemGroups:
    """One group id per catalogue item (brand, seller, category, series) for
    top_items' cap "at most max_per_group items of a group in a list": ids int32
    [n_items] contiguous, -1 for an item that is never capped.  n_groups is the
    largest id + 1.  Built by item_groups."""

    __slots__ = ("ids", "n_items", "n_groups")

    def __init__(self, ids: torch.Tensor, n_groups: int):
        if ids.dtype != torch.int32 or ids.dim() != 1 or ids.shape[0] < 1:
            raise ValueError(f"ids must be int32 [V >= 1], got {ids.dtype} {tuple(ids.shape)}")
        self.ids = ids.contiguous()
        self.n_items = ids.shape[0]
        self.n_groups = int(n_groups)

    def to(self, device) -> "ItemGroups":
        """The same groups on `device` (itself when already there)."""
        ids = self.ids.to(device)
        return self if ids is self.ids else ItemGroups(ids, self.n_groups)


def item_groups(group_of_item, device=None) -> ItemGroups:
    """ItemGroups from an integer tensor or sequence [V]: item v's group id, -1
    for an item that no cap applies to.  A value below -1 (or one that does not
    fit int32) raises ValueError.  The ids then move to `device`."""
    ids = torch.as_tensor(group_of_item)
    if ids.dim() != 1 or ids.numel() < 1 or ids.dtype.is_floating_point or ids.dtype in (
            torch.bool, torch.complex64, torch.complex128):
        raise ValueError(f"group_of_item must be an integer [V >= 1], got {ids.dtype} "
                         f"{tuple(ids.shape)}")
    lo, hi = int(ids.min()), int(ids.max())
    if lo < -1 or hi >= 2 ** 31 - 1:
        raise ValueError(f"group ids must lie in [-1, 2^31 - 1), got [{lo}, {hi}]")
    ids = ids.to(torch.int32)
    return ItemGroups(ids if device is None else ids.to(device), hi + 1)


def _check_groups(groups, max_per_group, V: int, device):
    """top_items' cap arguments -> (groups on `device` or None, m)."""
    if (groups is None) != (max_per_group is None):
        raise ValueError("groups and max_per_group are given together or not at all")
    if groups is None:
        return None, None
    if not isinstance(groups, ItemGroups):
        raise TypeError("groups must be an ItemGroups (scoring.item_groups)")
    if groups.n_items != V:
        raise ValueError(f"groups covers {groups.n_items} items, the table has {V}")
    m = int(max_per_group)
    if m < 1:
        raise ValueError(f"max_per_group = {max_per_group} must be >= 1")
    return groups.to(device), m


# ---- score priors: a per-item term, weighted per row (include/recblr_priors.h) ------
class ItemPriors:
    """P per-item score priors over a catalogue of n_items items: values fp32
    [P, n_items] contiguous.  top_items and target_ranks rank by score +
    (prior_weight * values[prior_rows[b], item]): a promotion, a recency or
    margin boost, a popularity damping (log_popularity), a per-market prior.
    Built by item_priors."""

    __slots__ = ("values", "n_items")

    def __init__(self, values: torch.Tensor):
        if (values.dtype != torch.float32 or values.dim() != 2 or values.shape[0] < 1
                or values.shape[1] < 1):
            raise ValueError(f"values must be fp32 [P >= 1, V >= 1], got {values.dtype} "
                             f"{tuple(values.shape)}")
        self.values = values.contiguous()
        self.n_items = values.shape[1]

    @property
    def n_priors(self) -> int:
        return self.values.shape[0]

    def to(self, device) -> "ItemPriors":
        """The same priors on `device` (itself when already there)."""
        values = self.values.to(device)
        return self if values is self.values else ItemPriors(values)


def item_priors(values, n_items: int | None = None, device=None) -> ItemPriors:
    """ItemPriors from a float tensor [V] (P = 1) or [P, V], or a sequence of P
    sequences of V numbers; stored as fp32, contiguous.  n_items, when given,
    must be V.  inf and NaN are values like any other: +inf lifts an item to
    the top, -inf sinks it without hiding it, NaN drops it for the rows that
    take that prior.  The values then move to `device`."""
    v = values if isinstance(values, torch.Tensor) else torch.as_tensor(values)
    if not v.dtype.is_floating_point:
        if isinstance(values, torch.Tensor):
            raise ValueError(f"values must be a float tensor, got {v.dtype}")
        v = v.to(torch.float32)
    if v.dim() == 1:
        v = v[None]
    if v.dim() != 2 or v.shape[0] < 1 or v.shape[1] < 1:
        raise ValueError(f"values must be [V] or [P, V], got {tuple(v.shape)}")
    if n_items is not None and int(n_items) != v.shape[1]:
        raise ValueError(f"n_items = {n_items} but the values cover {v.shape[1]} items")
    v = v.detach().to(torch.float32).contiguous()
    return ItemPriors(v if device is None else v.to(device))


def log_popularity(counts, smoothing: float = 1.0, alpha: float = 1.0) -> torch.Tensor:
    """fp32 [V]: alpha * log(counts + smoothing), normalised by its logsumexp —
    the log of the smoothed, alpha-tempered popularity distribution.  With
    data.train_item_counts it is a prior (item_priors), and prior_weight =
    -beta damps popular items at serving time."""
    c = torch.as_tensor(counts).to(torch.float64)
    if c.dim() != 1 or c.numel() < 1:
        raise ValueError(f"counts must be [V >= 1], got {tuple(c.shape)}")
    logq = float(alpha) * torch.log(c + float(smoothing))
    return (logq - torch.logsumexp(logq, 0)).to(torch.float32)


def _check_prior(prior, prior_rows, prior_weight, B: int, V: int, device):
    """top_items' and target_ranks' prior arguments -> (prior on `device`,
    prior_rows int64 [B] on `device` or None, prior_weight fp32 [B] on `device`
    or None), all None without a prior.  prior_rows is moved, not read (-1: no
    prior; a value outside [-1, P): the row selects nothing)."""
    if prior is None:
        if prior_rows is not None or prior_weight is not None:
            raise ValueError("prior_rows / prior_weight without prior")
        return None, None, None
    if not isinstance(prior, ItemPriors):
        raise TypeError("prior must be an ItemPriors (scoring.item_priors)")
    if prior.n_items != V:
        raise ValueError(f"prior covers {prior.n_items} items, the table has {V}")
    if prior_rows is not None:
        if not isinstance(prior_rows, torch.Tensor) or prior_rows.shape != (B,):
            raise ValueError(f"prior_rows must be [B] = [{B}], got "
                             f"{tuple(getattr(prior_rows, 'shape', ()))}")
        prior_rows = prior_rows.to(device=device, dtype=torch.int64)
    if isinstance(prior_weight, torch.Tensor):
        if prior_weight.shape != (B,) or not prior_weight.dtype.is_floating_point:
            raise ValueError(f"a tensor prior_weight must be float [B] = [{B}], got "
                             f"{prior_weight.dtype} {tuple(prior_weight.shape)}")
        prior_weight = prior_weight.detach().to(device=device, dtype=torch.float32)
    elif prior_weight is not None:
        prior_weight = torch.full((B,), float(prior_weight), dtype=torch.float32, device=device)
    return prior.to(device), prior_rows, prior_weight


def _adjusted(scores, prior: ItemPriors, prior_rows, prior_weight):
    """(adj fp32 [B, V], none bool [B]) by the kernels' rule: adj = scores +
    (w[:, None] * values[p]), product and sum each rounded to fp32, for rows
    with p in [0, P); the scores themselves (a select) for p = -1; none marks
    the rows whose p is outside [-1, P), which select nothing."""
    B = scores.shape[0]
    dev = scores.device
    n = prior.n_priors
    p = torch.zeros(B, dtype=torch.int64, device=dev) if prior_rows is None else prior_rows
    w = torch.ones(B, dtype=torch.float32, device=dev) if prior_weight is None else prior_weight
    term = w[:, None] * prior.values[p.clamp(0, n - 1)]
    adj = torch.where(((p >= 0) & (p < n))[:, None], scores + term, scores)
    return adj, (p < -1) | (p >= n)


def _target_ranks_torch(seq, table, target, first_item=1, allow=None, allow_rows=None,
                        prior=None, prior_rows=None, prior_weight=None, scores=None):
    """target_ranks' contract in plain torch on the [B, V] matrix (scores:
    the model scores to use instead of seq @ table.T)."""
    scores = seq.float() @ table.float().t() if scores is None else scores
    B, V = scores.shape
    dev = scores.device
    target = target.to(device=dev, dtype=torch.int64)
    bad = (target < 0) | (target >= V)
    tc = target.clamp(0, V - 1)
    cols = torch.arange(V, device=dev)[None, :]
    sel = (cols >= int(first_item)) & (cols != tc[:, None])
    allow, allow_rows = _check_allow(allow, allow_rows, B, V, dev)
    if allow is not None:
        ok = _allowed_mask(allow, allow_rows, B)
        sel &= ok
        bad |= ~ok.gather(1, tc[:, None])[:, 0]
    prior, prior_rows, prior_weight = _check_prior(prior, prior_rows, prior_weight, B, V, dev)
    if prior is not None:
        scores, none = _adjusted(scores, prior, prior_rows, prior_weight)
        bad |= none
    ts = scores.gather(1, tc[:, None])
    bad |= torch.isnan(ts[:, 0])
    minus = torch.full((B,), -1, dtype=torch.int64, device=dev)
    n_gt = torch.where(bad, minus, (sel & (scores > ts)).sum(1))
    n_eq = torch.where(bad, minus, (sel & (scores == ts)).sum(1))
    return n_gt, n_eq


def target_ranks(seq: torch.Tensor, table: torch.Tensor, target: torch.Tensor,
                 first_item: int = 1, allow: ItemFilters | None = None,
                 allow_rows: torch.Tensor | None = None, prior: ItemPriors | None = None,
                 prior_rows: torch.Tensor | None = None, prior_weight=None):
    """(n_greater, n_equal) over items [first_item, V) other than the target.

    first_item = 1 excludes the padding item 0, as RecBole's full-sort
    evaluation does (scores[:, 0] = -inf) and as run_with_unseen.py:237 does
    (scores[1:]).  allow / allow_rows (top_items' arguments): only the items
    that the row's filter allows are counted, and a target that it does not
    allow gives -1, -1, which rank_metrics drops.  prior / prior_rows /
    prior_weight (top_items' arguments): the counts compare adjusted scores,
    the target's included (rb_item_rank_prior); a target whose adjusted score
    is NaN, or whose row's prior index is outside [-1, P), gives -1, -1."""
    if not supported(seq, table):
        raise kernels.RecBLRNativeError("target_ranks needs fp32 CUDA tensors with d in "
                                        f"{kernels.ITEM_DIMS}")
    allow, allow_rows = _check_allow(allow, allow_rows, seq.shape[0], table.shape[0], seq.device)
    prior, prior_rows, prior_weight = _check_prior(prior, prior_rows, prior_weight, seq.shape[0],
                                                   table.shape[0], seq.device)
    opts = dict(allow=allow.words if allow is not None else None, allow_rows=allow_rows,
                prior=prior.values if prior is not None else None, prior_rows=prior_rows,
                prior_weight=prior_weight)
    # an absent option stays out of the call (item_rank picks the entry point from the rest)
    return kernels.item_rank(seq.detach(), table.detach(), target, first_item=first_item,
                             **{name: v for name, v in opts.items() if v is not None})


def _top_items_torch(seq, table, k, first_item, exclude, allow=None, allow_rows=None,
                     groups=None, max_per_group=None, prior=None, prior_rows=None,
                     prior_weight=None, scores=None):
    """top_items' contract in plain torch (any device, any d, any k, any group
    id).  scores: the [B, V] model scores to select on instead of seq @ table.T
    (full_sort_scores' matrix makes this the kernels' reference, bit for bit)."""
    scores = seq.float() @ table.float().t() if scores is None else scores
    B, V = scores.shape
    dev = scores.device
    prior, prior_rows, prior_weight = _check_prior(prior, prior_rows, prior_weight, B, V, dev)
    none = None
    if prior is not None:
        scores, none = _adjusted(scores, prior, prior_rows, prior_weight)
    drop = torch.isnan(scores)
    if none is not None:
        drop |= none[:, None]
    drop[:, :min(max(int(first_item), 0), V)] = True
    allow, allow_rows = _check_allow(allow, allow_rows, B, V, dev)
    if allow is not None:
        drop |= ~_allowed_mask(allow, allow_rows, B)
    if exclude is not None and exclude.numel() > 0:
        ex = exclude.to(device=dev, dtype=torch.int64)
        ok = (ex >= 0) & (ex < V)
        rows = torch.arange(B, device=dev)[:, None].expand_as(ex)
        drop[rows[ok], ex[ok]] = True
    masked = torch.where(drop, torch.full_like(scores, float("-inf")), scores)
    # ids ascending, stable descending sort: equal scores keep the smaller id
    # first; a second stable sort moves the dropped columns behind the rest
    # (a selectable item may itself score -inf)
    order = torch.sort(masked, dim=1, descending=True, stable=True).indices
    back = torch.sort(drop.gather(1, order).to(torch.int8), dim=1, stable=True).indices
    order = order.gather(1, back)
    n_ok = (~drop).sum(1, keepdim=True)
    groups, m = _check_groups(groups, max_per_group, V, dev)
    if groups is not None:
        # the cap as a segmented count: a stable sort of the ordered items by
        # group keeps each group's run in walk order, so an item's place in its
        # run is the number of its group walked before it (the dropped columns
        # stand behind every selectable one and disturb no count)
        g = groups.ids.to(torch.int64)[order]
        by = torch.sort(g, dim=1, stable=True)
        pos = torch.arange(V, device=dev)[None, :].expand(B, -1)
        head = torch.ones_like(drop)
        head[:, 1:] = by.values[:, 1:] != by.values[:, :-1]
        seen = pos - torch.where(head, pos, torch.zeros_like(pos)).cummax(1).values
        seen = torch.empty_like(seen).scatter_(1, by.indices, seen)
        keep = (pos < n_ok) & ((g < 0) | (seen < m))
        order = order.gather(1, torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices)
        n_ok = keep.sum(1, keepdim=True)
    kk = min(k, V)
    ids = torch.full((B, k), -1, dtype=torch.int64, device=dev)
    out = torch.full((B, k), float("-inf"), dtype=torch.float32, device=dev)
    live = torch.arange(kk, device=dev)[None, :] < n_ok
    ids[:, :kk] = torch.where(live, order[:, :kk], ids[:, :kk])
    out[:, :kk] = torch.where(live, scores.gather(1, order[:, :kk]), out[:, :kk])
    return ids, out


@torch.no_grad()
def top_items(seq: torch.Tensor, table: torch.Tensor, k: int, first_item: int = 1,
              exclude: torch.Tensor | None = None, allow: ItemFilters | None = None,
              allow_rows: torch.Tensor | None = None, groups: ItemGroups | None = None,
              max_per_group: int | None = None, prior: ItemPriors | None = None,
              prior_rows: torch.Tensor | None = None, prior_weight=None):
    """Each row's k best items: (ids int64 [B, k], scores fp32 [B, k]).

    Selects over items in [first_item, V) not listed in exclude [B, E] (int64;
    entries outside [0, V) are ignored and duplicates allowed, so item_seq
    with its 0 padding serves as the seen-item list), ordered by (score
    descending, item id ascending) — rank_metrics' "optimistic" convention for
    a target with the smallest id of its tied group.  NaN scores are never
    selected; when fewer than k items are selectable the tail holds id -1,
    score -inf.  On fp32 GPU tensors with d in kernels.ITEM_DIMS and k <= 64
    the selection runs inside the scoring kernel (rb_item_topk: no [B, V]
    buffer, scores bit-identical to full_sort_scores'); anything else takes a
    plain torch path with the same contract.

    allow (an ItemFilters over the table's V items, from item_filters)
    restricts the selection to a catalogue filter: "in stock", "sold in this
    region", "on this category page".  allow_rows [B] (int64, any device; moved
    to the GPU but never read on the host) names each row's filter: None means
    filter 0 for every row, -1 no filter for that row (the unfiltered result,
    bit for bit), and a value outside [-1, F) selects nothing (k times -1 /
    -inf).  exclude, first_item and the NaN rule apply on top.  In the kernel
    a filter costs one word load per (row, 32-item tile) and a sparse one
    saves selection work (rb_item_topk_allowed).

    groups (an ItemGroups over the table's V items, from item_groups) with
    max_per_group = m >= 1, given together, cap a list's diversity: at most m
    items of one brand, seller, category or series.  The result is that of a
    walk over the row's selectable items (all the rules above) in the order
    above that takes an item unless m of its group were taken, and stops after
    k; an item of group -1 is never capped; where fewer than k are taken the
    tail is id -1 / score -inf.  The selection kernel applies the cap in its
    own sweep (rb_item_topk_grouped, exact: no depth to guess); m >= k, or
    groups that are all distinct or all -1, give the uncapped result bit for
    bit.  A group id above kernels.ITEM_GROUP_ID_MAX takes the torch path.

    prior (an ItemPriors over the table's V items, from item_priors) ranks by
    the adjusted score adj = score + (w_b * prior.values[p_b, item]) instead of
    the model score: the product is rounded to fp32, then the sum (no fused
    multiply-add), so full_sort_scores(seq, table) + w[:, None] * values[p]
    gives the same bits on any device.  prior_rows [B] (int64, any device;
    moved to the GPU but never read on the host) is p: None means prior 0 for
    every row, -1 no prior for that row (a select, not an addition of zero: the
    un-priored result bit for bit, a -0.0 score included), and a value outside
    [-1, P) selects nothing.  prior_weight is w: None (1.0), a Python float,
    or a float [B] tensor.  Every rule above then applies to adj: the order is
    (adj descending, id ascending), a NaN adj is never selected (a NaN prior,
    inf - inf), a -inf prior sinks an item without hiding it, exclude,
    first_item, the filter and the cap apply unchanged, and the scores returned
    are adjusted scores.  The kernel adds the term to a tile's scores before
    its threshold compare (rb_item_topk_prior); without prior the calls are the
    ones above.  Candidate reranking (top_candidates, candidate_ranks) takes no
    prior: candidate_scores, plus a gather of the prior at the candidates, plus
    order_candidates already does that without a [B, V] matrix."""
    k = int(k)
    if k < 1:
        raise ValueError(f"k = {k} must be positive")
    if int(first_item) < 0:
        raise ValueError(f"first_item = {first_item} must be >= 0")
    if exclude is not None and (exclude.dim() != 2 or exclude.shape[0] != seq.shape[0]):
        raise ValueError(f"exclude must be [B, E], got {tuple(exclude.shape)}")
    allow, allow_rows = _check_allow(allow, allow_rows, seq.shape[0], table.shape[0], seq.device)
    groups, m = _check_groups(groups, max_per_group, table.shape[0], seq.device)
    prior, prior_rows, prior_weight = _check_prior(prior, prior_rows, prior_weight, seq.shape[0],
                                                   table.shape[0], seq.device)
    if supported(seq, table) and k <= kernels.ITEM_TOPK_MAX and (
            groups is None or groups.n_groups <= kernels.ITEM_GROUP_ID_MAX + 1):
        if exclude is not None:
            exclude = exclude.to(device=seq.device, dtype=torch.int64)
        opts = dict(allow=allow.words if allow is not None else None, allow_rows=allow_rows,
                    groups=groups.ids if groups is not None else None, max_per_group=m,
                    prior=prior.values if prior is not None else None, prior_rows=prior_rows,
                    prior_weight=prior_weight)
        # an absent option stays out of the call (item_topk picks the entry point from the rest)
        return kernels.item_topk(seq.detach(), table.detach(), k, first_item=first_item,
                                 exclude=exclude,
                                 **{name: v for name, v in opts.items() if v is not None})
    return _top_items_torch(seq.detach(), table.detach(), k, first_item, exclude, allow,
                            allow_rows, groups, m, prior, prior_rows, prior_weight)


# ---- candidate lists: scoring chosen items (csrc/candidates.hip) --------------------
def _check_candidates(seq, table, candidates):
    if seq.dim() != 2 or table.dim() != 2 or seq.shape[1] != table.shape[1]:
        raise ValueError(f"seq [B, d] and table [V, d] required, got {tuple(seq.shape)} and "
                         f"{tuple(table.shape)}")
    if (not isinstance(candidates, torch.Tensor) or candidates.dim() != 2
            or candidates.shape[0] != seq.shape[0]):
        raise ValueError("candidates must be [B, C], got "
                         f"{tuple(getattr(candidates, 'shape', ()))}")
    return candidates.to(device=seq.device, dtype=torch.int64)


def _candidate_scores_torch(seq, table, candidates):
    """candidate_scores in torch ops (differentiable; materialises [B, C, d])."""
    V = table.shape[0]
    ok = (candidates >= 0) & (candidates < V)
    s = (seq[:, None, :] * table[candidates.clamp(0, V - 1)]).sum(-1)
    return torch.where(ok, s, torch.full_like(s, float("-inf")))


def candidate_scores(seq: torch.Tensor, table: torch.Tensor,
                     candidates: torch.Tensor) -> torch.Tensor:
    """scores [B, C]: seq_b . table[candidates[b, c]]; -inf for an id outside
    [0, V), so -1 pads a ragged list.  On fp32 GPU tensors with d a multiple
    of 4 up to 512 and no gradient needed this is one launch
    (rb_candidate_scores: no [B, C, d] gather, no [B, V] matrix), and a (row,
    id) pair's score has the same bits wherever the id stands and whatever B
    and C are.  Anything else takes the torch expression with the same
    masking, which is differentiable: RecBLR.predict for several items."""
    candidates = _check_candidates(seq, table, candidates)
    needs_grad = torch.is_grad_enabled() and (seq.requires_grad or table.requires_grad)
    if kernels.candidates_supported(seq, table) and not needs_grad:
        return kernels.candidate_scores(seq.detach(), table.detach(), candidates)
    return _candidate_scores_torch(seq, table, candidates)


@torch.no_grad()
def order_candidates(scores: torch.Tensor, candidates: torch.Tensor, k: int, first_item: int = 0,
                     exclude: torch.Tensor | None = None, num_items: int | None = None):
    """The selection rule of top_candidates alone, in torch ops on any device:
    ``(ids int64 [B, k], scores fp32 [B, k])`` from scores [B, C] and their ids
    candidates [B, C].

    Per row it selects over the distinct ids that lie in [first_item,
    num_items) (num_items None: no upper limit), are not listed in exclude
    [B, E] (entries outside [0, num_items) are ignored, duplicates allowed —
    top_items' rule) and whose score is not NaN, ordered by (score descending,
    id ascending).  An id listed several times appears once, where its first
    entry in that order stands.  When fewer than k survive the tail holds id
    -1, score -inf; a selectable candidate that itself scores -inf comes before
    that padding."""
    k, first = int(k), int(first_item)
    if k < 1:
        raise ValueError(f"k = {k} must be positive")
    if first < 0:
        raise ValueError(f"first_item = {first_item} must be >= 0")
    if scores.dim() != 2 or candidates.shape != scores.shape:
        raise ValueError(f"scores and candidates must both be [B, C], got {tuple(scores.shape)} "
                         f"and {tuple(candidates.shape)}")
    B, C = scores.shape
    dev = scores.device
    scores = scores.float()
    ids = candidates.to(device=dev, dtype=torch.int64)
    drop = torch.isnan(scores) | (ids < first)
    if num_items is not None:
        drop |= ids >= int(num_items)
    if exclude is not None and exclude.numel() > 0:
        if exclude.dim() != 2 or exclude.shape[0] != B:
            raise ValueError(f"exclude must be [B, E], got {tuple(exclude.shape)}")
        ex = exclude.to(device=dev, dtype=torch.int64)
        bad = ex < 0
        if num_items is not None:
            bad |= ex >= int(num_items)
        # membership by a sorted search: an ignored entry becomes -1, which only
        # a dropped candidate (id < 0 <= first_item) can equal
        ex = torch.sort(torch.where(bad, torch.full_like(ex, -1), ex), dim=1).values
        at = torch.searchsorted(ex, ids.contiguous()).clamp(max=ex.shape[1] - 1)
        drop |= ex.gather(1, at) == ids
    masked = torch.where(drop, torch.full_like(scores, float("-inf")), scores)
    # three stable sorts: by id, then by score descending (equal scores keep
    # the smaller id first), then the dropped entries behind the rest
    order = torch.sort(ids, dim=1, stable=True).indices
    order = order.gather(1, torch.sort(masked.gather(1, order), dim=1, descending=True,
                                       stable=True).indices)
    order = order.gather(1, torch.sort(drop.gather(1, order).to(torch.int8), dim=1,
                                       stable=True).indices)
    # duplicates by id: in a stable sort of the ordered ids each id's run
    # starts with its earliest entry; every later one is dropped as well
    sid, sdrop = ids.gather(1, order), drop.gather(1, order)
    by_id = torch.sort(sid, dim=1, stable=True)
    run_start = torch.ones_like(sid, dtype=torch.bool)
    run_start[:, 1:] = by_id.values[:, 1:] != by_id.values[:, :-1]
    dup = torch.ones_like(sdrop).scatter_(1, by_id.indices, ~run_start)
    gone = sdrop | dup
    order = order.gather(1, torch.sort(gone.to(torch.int8), dim=1, stable=True).indices)
    n_ok = (~gone).sum(1, keepdim=True)
    kk = min(k, C)
    out_ids = torch.full((B, k), -1, dtype=torch.int64, device=dev)
    out = torch.full((B, k), float("-inf"), dtype=torch.float32, device=dev)
    live = torch.arange(kk, device=dev)[None, :] < n_ok
    out_ids[:, :kk] = torch.where(live, ids.gather(1, order[:, :kk]), out_ids[:, :kk])
    out[:, :kk] = torch.where(live, scores.gather(1, order[:, :kk]), out[:, :kk])
    return out_ids, out


@torch.no_grad()
def top_candidates(seq: torch.Tensor, table: torch.Tensor, candidates: torch.Tensor, k: int,
                   first_item: int = 0, exclude: torch.Tensor | None = None):
    """Each row's candidate list ordered by the model: ``(ids int64 [B, k],
    scores fp32 [B, k])``, the k best distinct ids of candidates [B, C] (-1
    pads a ragged list) by (score descending, id ascending) — top_items'
    order and top_items' rules for first_item, exclude [B, E] and NaN scores;
    a repeated id appears once; where fewer than k survive the tail holds id
    -1, score -inf.  k = C orders the whole list.

    On fp32 GPU tensors with d a multiple of 4 up to 512, C <=
    kernels.CANDIDATE_MAX and E <= kernels.CANDIDATE_EXCLUDE_MAX it is one
    launch that scores, filters, sorts and writes (rb_candidate_topk), its
    scores bit-identical to candidate_scores'; anything else is
    order_candidates(candidate_scores(...), ...)."""
    k = int(k)
    if k < 1:
        raise ValueError(f"k = {k} must be positive")
    if int(first_item) < 0:
        raise ValueError(f"first_item = {first_item} must be >= 0")
    candidates = _check_candidates(seq, table, candidates)
    if exclude is not None:
        if exclude.dim() != 2 or exclude.shape[0] != seq.shape[0]:
            raise ValueError(f"exclude must be [B, E], got {tuple(exclude.shape)}")
        exclude = exclude.to(device=seq.device, dtype=torch.int64)
    V, C = table.shape[0], candidates.shape[1]
    E = 0 if exclude is None else exclude.shape[1]
    seq, table = seq.detach(), table.detach()
    if (kernels.candidates_supported(seq, table) and 1 <= C <= kernels.CANDIDATE_MAX
            and E <= kernels.CANDIDATE_EXCLUDE_MAX and int(first_item) <= V):
        return kernels.candidate_topk(seq, table, candidates, k, first_item=first_item,
                                      exclude=exclude if E else None)
    return order_candidates(candidate_scores(seq, table, candidates), candidates, k, first_item,
                            exclude, num_items=V)


def _candidate_ranks_torch(seq, table, target, candidates, first_item):
    V = table.shape[0]
    s = _candidate_scores_torch(seq, table, torch.cat([target[:, None], candidates], 1))
    st, s = s[:, :1], s[:, 1:]
    ok = ((candidates >= first_item) & (candidates < V) & (candidates != target[:, None])
          & ~torch.isnan(s))
    gt, eq = (ok & (s > st)).sum(1), (ok & (s == st)).sum(1)
    bad = (target < first_item) | (target >= V)
    return gt.masked_fill(bad, -1), eq.masked_fill(bad, -1)


@torch.no_grad()
def candidate_ranks(seq: torch.Tensor, table: torch.Tensor, target: torch.Tensor,
                    candidates: torch.Tensor, first_item: int = 1):
    """(n_greater, n_equal) int64 [B] of each row's target among its own
    candidates [B, C] (sampled negatives): over the entries that lie in
    [first_item, V), differ from the target and have a non-NaN score, how many
    score strictly above the target and how many exactly equal to it.  Entries
    count as listed (a repeated negative counts twice, as a batch expanded
    through predict counts it); a target outside [first_item, V) gives -1, -1,
    which rank_metrics drops.  One launch on the GPU (rb_candidate_ranks, any
    C); the CPU and an unsupported d take torch ops."""
    if int(first_item) < 0:
        raise ValueError(f"first_item = {first_item} must be >= 0")
    candidates = _check_candidates(seq, table, candidates)
    if target.shape != (seq.shape[0],):
        raise ValueError(f"target must be [B], got {tuple(target.shape)}")
    target = target.to(device=seq.device, dtype=torch.int64)
    seq, table = seq.detach(), table.detach()
    if (kernels.candidates_supported(seq, table) and candidates.shape[1] >= 1
            and int(first_item) <= table.shape[0]):
        return kernels.candidate_ranks(seq, table, target, candidates, first_item=first_item)
    return _candidate_ranks_torch(seq, table, target, candidates, int(first_item))


def rank_metrics(n_greater: torch.Tensor, n_equal: torch.Tensor | None = None,
                 topk=(10, 20), ties: str = "optimistic") -> dict:
    """Mean Hit@k, MRR@k and NDCG@k of single-target rows from their ranks.

    ties="optimistic": rank = n_greater (the target placed first among equal
    scores).  ties="average": the gain averaged over the positions the tied
    group spans, as sklearn.metrics.ndcg_score(ignore_ties=False) does
    (run_with_unseen.py:247); Hit/MRR then use the same averaging.
    Rows with a negative rank (invalid target) are dropped."""
    g = n_greater.double()
    e = (n_equal.double() if n_equal is not None and ties == "average"
         else torch.zeros_like(g))
    keep = g >= 0
    g, e = g[keep], e[keep]
    out = {}
    if g.numel() == 0:
        for k in topk:
            out[f"hit@{k}"] = out[f"mrr@{k}"] = out[f"ndcg@{k}"] = 0.0
        return out
    cnt = e + 1.0
    for k in topk:
        pos = torch.arange(k, dtype=torch.float64, device=g.device)[None, :]
        hit = ((pos >= g[:, None]) & (pos <= (g + e)[:, None])).double()  # positions < k only
        out[f"hit@{k}"] = float((hit.sum(1) / cnt).mean())
        out[f"mrr@{k}"] = float(((hit / (pos + 1.0)).sum(1) / cnt).mean())
        out[f"ndcg@{k}"] = float(((hit / torch.log2(pos + 2.0)).sum(1) / cnt).mean())
    return out

"""RecBLR sequential recommender on the MI355X encoder.

Drop-in for the reference's ``RecBLR.py``: same class names, constructor
arguments, config keys (RecBLR.py:22-30), submodule and parameter names
(``item_embedding``, ``recurrent_layers.{i}.behavior_modeling.{input, conv1d,
gates, Lambda, output}``, ``...ffn.{w_1, w_2, layer_norm}``, ...), so RecBole
checkpoints and ``state_dict``s move between the two unchanged.  Modules are
created in the reference's order, so under the same seed the initial weights
are identical too.

What differs is the execution:
* ``GatedRecurrentLayer.forward``: the reference's ~25-kernel chain (pad copy,
  transposes, conv, a dozen elementwise gate ops, Triton scan, truncate,
  merge) is two fused HIP kernels around the gates GEMM (``recurrence.py``);
* embedding -> dropout -> LayerNorm, dropout + residual + LayerNorm and the
  FFN's SiLU + dropout are fused HIP kernels (``blocks.py``), with a
  deterministic sort-based embedding backward;
* projections are MFMA GEMMs with split-K weight gradients (``linear.py``).
Everything needs a ROCm GPU; there is no CPU fallback.
"""
from __future__ import annotations

import functools
import math
import os

import torch
import torch.nn.functional as F
from torch import nn

from ._lib import RecBLRNativeError
from .blocks import (ResidualGrad, add_dropout_layer_norm, draw_seed, embed_dropout_layer_norm,
                     feed_forward, linear_add_dropout_layer_norm)
from .kernels import (MAX_NEGATIVES, MAX_SHARED_NEGATIVES, Packed, grl_max_tiles, grl_pieces,
                      next_item_targets, next_item_targets_reference, sample_negatives_reference,
                      negative_sampler, pack_plan, sample_negatives)
from .linear import (MIN_ROWS_FOR_SPLIT, HipLinearForward, fire_hooks, has_hooks, linear,
                     split_in_projection)
from .recbole_compat import BPRLoss, SequentialRecommender, install_interaction_hook
from .recurrence import bd_lru, fused_ok, pow2_pad_len, row_pad_lens


from .scoring import (candidate_ranks, candidate_scores, full_sort_scores, item_cross_entropy,
                      item_cross_entropy_rows, pair_loss, shared_softmax_loss, target_ranks, top_candidates, top_items)

# RECBLR_CONV_ROWS=0: packed conv forward per sequence instead of per row tile
_CONV_ROWS = os.environ.get("RECBLR_CONV_ROWS", "1") != "0"
class _PinnedRing:
    """A few reusable page-locked staging buffers for the per-batch host ->
    device copy of the packed layout (offsets, order): no pinned allocation
    per step; slot i is reused only after the copy from it has completed
    (its event; only waits if the device runs >= k batches behind).

    Under HIP-graph capture the ring is bypassed: a captured non_blocking
    copy reads its pinned source when the graph is REPLAYED, so a ring slot
    overwritten by a later stage() would change what the graph uploads.  A
    captured stage() therefore copies into a pinned buffer of its own that is
    kept alive (and never rewritten) for the life of the process — the graph
    replays exactly the batch layout it captured."""

    def __init__(self, k: int = 4):
        self.k, self.i = k, 0
        self.bufs = [None] * k
        self.events = [None] * k
        self.captured = []   # pinned sources of captured copies (kept alive)

    def stage(self, host: torch.Tensor, device) -> torch.Tensor:
        if torch.cuda.is_current_stream_capturing():
            buf = torch.empty(host.numel(), dtype=host.dtype, pin_memory=True)
            buf.copy_(host.reshape(-1))
            self.captured.append(buf)
            with torch.cuda.device(device):
                return buf.to(device, non_blocking=True)
        i = self.i
        self.i = (i + 1) % self.k
        n = host.numel()
        buf = self.bufs[i]
        if buf is None or buf.numel() < n or buf.dtype != host.dtype:
            buf = self.bufs[i] = torch.empty(max(n, 4096), dtype=host.dtype, pin_memory=True)
            self.events[i] = None
        if self.events[i] is not None:
            self.events[i].synchronize()
        buf[:n].copy_(host)
        # the copy and its event on the TARGET device's current stream (the
        # current device may be another one)
        with torch.cuda.device(device):
            out = buf[:n].to(device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(device))
        self.events[i] = ev
        return out


_host_ring = _PinnedRing()
_host_ring32 = _PinnedRing()   # int32 staging (the fused kernel's work lists)
_ncus: dict = {}


def _num_cus(dev) -> int:
    n = _ncus.get(dev)
    if n is None:
        n = _ncus[dev] = torch.cuda.get_device_properties(dev).multi_processor_count
    return n

# RECBLR_LAST_ONLY=0: the last layer's scan writes y at every position
_LAST_ONLY = os.environ.get("RECBLR_LAST_ONLY", "1") != "0"
# RECBLR_SPARSE_Z=0: that layer still computes z, and dz's zeros, at every row.
# Default: y_last reads z only at each sequence's last row, so the
# in-projection makes x [ntok, H] and z_last [B, H] (linear.SplitInProjFn) and
# the scan kernels take z_last / write dz_last — from SPARSE_Z_MIN_ROWS packed
# rows (the row count from which linear switches kernels: below it the saved
# bytes are microseconds and the extra few-rows launches cost more)
_SPARSE_Z = os.environ.get("RECBLR_SPARSE_Z", "1") != "0"
SPARSE_Z_MIN_ROWS = MIN_ROWS_FOR_SPLIT


def set_sparse_z(on: bool, min_rows: int | None = None):
    """Switch the last layer's sparse z and, optionally, its minimum packed
    row count (A/B runs, tests); returns the previous (on, min_rows)."""
    global _SPARSE_Z, SPARSE_Z_MIN_ROWS
    prev = (_SPARSE_Z, SPARSE_Z_MIN_ROWS)
    _SPARSE_Z = bool(on)
    if min_rows is not None:
        SPARSE_Z_MIN_ROWS = int(min_rows)
    return prev


__all__ = ["RecBLR", "RecurrentLayer", "GatedRecurrentLayer", "FeedForward",
           "softplus_inverse", "lambda_init_range"]


def softplus_inverse(x):
    """log(exp(x) - 1): the Lambda init helper (RecBLR.py:14-15)."""
    return torch.log(torch.exp(x) - 1)


def lambda_init_range(r_min: float = 0.9, r_max: float = 0.999):
    """Lambda endpoints such that exp(-softplus(Lambda)) spans [r_min, r_max]
    (RecBLR.py:153-158), computed in fp32 like the reference."""
    lo = softplus_inverse(torch.tensor(-math.log(r_min))).item()
    hi = softplus_inverse(torch.tensor(-math.log(r_max))).item()
    return lo, hi


class GatedRecurrentLayer(nn.Module):
    """in-proj -> causal conv + SiLU -> BD-LRU gates -> scan -> silu(z)*h -> out-proj.

    Parameters as RecBLR.py:149-167.  ``bd_lru_only`` is stored but, as in the
    reference (:151), does not change this block."""

    def __init__(self, d_model=64, expansion_factor=2, kernel_size=4, bd_lru_only=False,
                 disable_conv1d=False):
        super().__init__()
        self.bd_lru_only = bd_lru_only
        self.disable_conv1d = disable_conv1d
        lo, hi = lambda_init_range()
        hidden = int(d_model * expansion_factor)
        self.hidden = hidden
        self.input = nn.Linear(d_model, 2 * hidden, bias=False)
        self.conv1d = nn.Conv1d(hidden, hidden, kernel_size, groups=hidden,
                                padding=kernel_size - 1, bias=True)
        self.gates = nn.Linear(hidden, 2 * hidden, bias=True)
        self.Lambda = nn.Parameter(torch.linspace(lo, hi, hidden))
        self.output = nn.Linear(hidden, d_model, bias=False)
        # the projections run on the HIP path through their own nn.Linear
        # __call__ (forward hooks fire, the module type stays nn.Linear)
        for m in (self.input, self.output):
            m.forward = HipLinearForward(m)

    def forward(self, x, pad=None, slot=None, rows=None, seq=None, project=True, capture=None):
        """capture: optional callable (x, xc, rg, carries) handed to
        recurrence.bd_lru (the scan's inputs and tile carries of this layer).
        pad: None (the reference's pow2 pad prefix for x's length) or an
        int64 tensor [B] of per-row pad lengths (see recurrence.bd_lru).
        slot: blocks.ResidualGrad of the enclosing RecurrentLayer.
        rows: flat positions at which the output is needed (the
        out-projection is position-wise, so only those rows are projected;
        returns [len(rows), d]).
        seq: kernels.Packed — x is [ntok, d], the sequences' valid positions
        packed back to back (RecBLR.forward)."""
        if x.device.type != "cuda":
            raise RecBLRNativeError(
                "GatedRecurrentLayer runs only on the MI355X HIP path (ROCm GPU tensors); "
                "move the model to a GPU. The CPU restatement under oracle/ is test-only.")
        observe = None
        if has_hooks(self.gates) or has_hooks(self.conv1d):
            def observe(x_, xc, rg):   # hooks of the Linear / Conv1d fused into bd_lru
                if not self.disable_conv1d:
                    fire_hooks(self.conv1d, (x_.transpose(-1, -2),), xc.transpose(-1, -2))
                fire_hooks(self.gates, (xc,), rg + self.gates.bias)
        z_last = None
        if self._sparse_z(x, rows, seq, observe, capture):
            # ... and z only there: no [ntok, 2H] xz exists (the hooks of
            # self.input, which would see it, select the dense path)
            xz, z_last = split_in_projection(x, self.input.weight, seq.last, slot)
        else:
            self.input._recblr_slot = slot
            xz = self.input(x)
        # the last layer under gather_indexes on packed sequences needs y only
        # at each sequence's last row: the scan kernels keep just those
        last_only = (_LAST_ONLY and rows is not None and seq is not None
                     and rows is seq.last and xz.dtype == torch.float32)
        y = bd_lru(xz, self.conv1d.weight, self.conv1d.bias, self.gates.weight,
                   self.gates.bias, self.Lambda, use_conv=not self.disable_conv1d, pad=pad,
                   seq=seq, last_only=last_only, observe=observe, capture=capture,
                   z_last=z_last)
        if last_only:
            if seq.order is None:   # packed-sequence order -> batch order
                y = y.index_select(0, seq.inv)
        elif rows is not None:
            y = y.reshape(-1, y.shape[-1]).index_select(0, rows)
        # project=False: y before the out-projection (the caller fuses the
        # projection with its residual LayerNorm, blocks.linear_add_dropout_layer_norm)
        return self.output(y) if project else y

    def _sparse_z(self, x, rows, seq, observe, capture) -> bool:
        """Whether this call takes the sparse-z path: the last_only conditions
        of forward() on fp32, from SPARSE_Z_MIN_ROWS packed rows, with nothing
        that reads xz or the scan's inputs (hooks, observe, capture) and the
        three-launch recurrence."""
        w = self.input.weight
        return (_SPARSE_Z and _LAST_ONLY and rows is not None and seq is not None
                and rows is seq.last and seq.order is not None
                and seq.ntok >= SPARSE_Z_MIN_ROWS and x.dim() == 2
                and x.dtype == torch.float32 and w.dtype == torch.float32
                and self.input.bias is None and observe is None and capture is None
                and not has_hooks(self.input)
                and not fused_ok(seq.pieces is not None, self.hidden,
                                 not self.disable_conv1d, self.conv1d.weight.shape[-1], x.dtype))

    @staticmethod
    def pad_len(seq_len: int) -> int:
        return pow2_pad_len(seq_len)


class FeedForward(nn.Module):
    """Position-wise FFN with SiLU, residual and LayerNorm (RecBLR.py:210-227)."""

    def __init__(self, d_model, inner_size, dropout=0.2):
        super().__init__()
        self.w_1 = nn.Linear(d_model, inner_size)
        self.w_2 = nn.Linear(inner_size, d_model)
        self.dropout = nn.Dropout(dropout)
        self.layer_norm = nn.LayerNorm(d_model, eps=1e-12)

    def forward(self, input_tensor, in_addend=None, out_addend=None):
        return feed_forward(input_tensor, self, self.training, in_addend, out_addend)


class RecurrentLayer(nn.Module):
    """GRL + dropout + residual LayerNorm, then the FFN (RecBLR.py:124-145)."""

    def __init__(self, d_model, d_conv, expand, dropout, num_layers, bd_lru_only,
                 disable_conv1d, disable_ffn):
        super().__init__()
        self.num_layers = num_layers
        self.disable_ffn = disable_ffn
        self.behavior_modeling = GatedRecurrentLayer(
            d_model=d_model, expansion_factor=expand, kernel_size=d_conv,
            bd_lru_only=bd_lru_only, disable_conv1d=disable_conv1d)
        self.dropout = nn.Dropout(dropout)
        self.layer_norm = nn.LayerNorm(d_model, eps=1e-12)
        self.ffn = FeedForward(d_model=d_model, inner_size=d_model * 4, dropout=dropout)

    def forward(self, input_tensor, pad=None, rows=None, seq=None, slot=None, out_addend=None,
                capture=None):
        """capture: see GatedRecurrentLayer.forward.
        rows: evaluate the position-wise tail (out-projection, residual
        LayerNorm, FFN) only at these flat positions -> [len(rows), d].
        seq: kernels.Packed (input_tensor is [ntok, d]).
        slot: blocks.ResidualGrad for the residual branch's gradient (RecBLR
        creates it so that input_tensor's producer can take it);
        out_addend: the next layer's slot (a second gradient of the output)."""
        grad = torch.is_grad_enabled() and input_tensor.requires_grad
        if slot is None and grad:
            slot = ResidualGrad(rows)
        if not grad:
            slot = out_addend = None
        residual = input_tensor
        if rows is not None:
            residual = input_tensor.reshape(-1, input_tensor.shape[-1]).index_select(0, rows)
        out = self.behavior_modeling.output
        # full rows: the out-projection and the residual LayerNorm in one
        # launch where it applies (blocks.linear_add_dropout_layer_norm)
        fuse = rows is None and not has_hooks(out)
        y = self.behavior_modeling(input_tensor, pad, slot, rows, seq, project=not fuse,
                                   capture=capture)

        def add_ln(addend):
            if fuse:
                return linear_add_dropout_layer_norm(y, out, residual, self.dropout,
                                                     self.layer_norm, self.training, slot, addend)
            return add_dropout_layer_norm(y, residual, self.dropout, self.layer_norm,
                                          self.training, slot, addend)

        if self.disable_ffn:
            return add_ln(out_addend)
        # the FFN's own residual gradient goes back through h_slot to the
        # LayerNorm that produced h
        h_slot = ResidualGrad() if grad else None
        h = add_ln(h_slot)
        return self.ffn(h, h_slot, out_addend)


# Attribute a data path may set on the item_seq_len device tensor: the same
# lengths as a CPU tensor, so the packed forward needs no device sync to size
# its buffers (distributed.synthetic_interaction, data.SequentialLoader).
HOST_LENGTHS = "_recblr_host_lengths"


def attach_host_lengths(lengths_dev: torch.Tensor, lengths_cpu: torch.Tensor) -> torch.Tensor:
    setattr(lengths_dev, HOST_LENGTHS, lengths_cpu.detach().to("cpu"))
    return lengths_dev


class RecBLR(SequentialRecommender):
    """RecBole sequential recommender with the BD-LRU encoder (RecBLR.py:18-122)."""

    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        self.hidden_size = config["hidden_size"]
        self.loss_type = config["loss_type"]
        self.num_layers = config["num_layers"]
        self.dropout_prob = config["dropout_prob"]
        self.expand = config["expand"]
        self.d_conv = config["d_conv"]
        self.bd_lru_only = config["bd_lru_only"]
        self.disable_conv1d = config["disable_conv1d"]
        self.disable_ffn = config["disable_ffn"]
        # train on every position of a row instead of its last one
        # (calculate_loss_dense; the rows then come from a dense loader,
        # data.SequentialLoader(dense=True)); not a reference key, default off
        try:
            self.train_all_positions = bool(config["train_all_positions"])
        except (KeyError, TypeError):
            self.train_all_positions = False
        if self.train_all_positions and self.loss_type == "BPR":
            raise ValueError("train_all_positions needs loss_type 'CE': the BPR loss has one "
                             "sampled negative per row, not per position")
        # all-position training with n sampled negatives per position in place
        # of the full-vocabulary CE (calculate_loss_pairs); not a reference
        # key, default 0 = off.  loss_type keeps the reference's meaning
        try:
            self.dense_negatives = int(config["dense_negatives"] or 0)
        except (KeyError, TypeError):
            self.dense_negatives = 0
        # what the sampled negatives feed: 'pairs' (calculate_loss_pairs, n per
        # position) or 'sampled_softmax' (calculate_loss_sampled, n per row,
        # shared by its positions); not a reference key
        try:
            self.dense_loss = config["dense_loss"] or "pairs"
        except (KeyError, TypeError):
            self.dense_loss = "pairs"
        if self.dense_loss not in ("pairs", "sampled_softmax"):
            raise ValueError(f"dense_loss must be 'pairs' or 'sampled_softmax', got "
                             f"{self.dense_loss!r}")
        sampled = self.dense_loss == "sampled_softmax"
        most = MAX_SHARED_NEGATIVES if sampled else MAX_NEGATIVES
        if not 0 <= self.dense_negatives <= most:
            raise ValueError(f"dense_negatives must be in [0, {most}] for dense_loss "
                             f"{self.dense_loss!r}")
        if sampled and not self.dense_negatives:
            raise ValueError("dense_loss 'sampled_softmax' needs dense_negatives >= 1")
        if sampled and self.loss_type != "CE":
            raise ValueError("dense_loss 'sampled_softmax' needs loss_type 'CE'")
        # the log-Q correction of the uniform proposal (calculate_loss_sampled)
        try:
            correct = config["sampled_softmax_correct"]
        except (KeyError, TypeError):
            correct = None
        self.sampled_softmax_correct = True if correct is None else bool(correct)
        if self.dense_negatives and not self.train_all_positions:
            raise ValueError("dense_negatives needs train_all_positions: True (the negatives "
                             "are sampled at every position of a row)")
        # the proposal the sampled negatives are drawn from: 'uniform', or
        # 'popularity' — in proportion to (train count + dense_sampling_smoothing)
        # ** dense_sampling_alpha, from the counts given to set_item_counts; not
        # reference keys
        def key(name, default):
            try:
                value = config[name]
            except (KeyError, TypeError):
                value = None
            return default if value is None else value

        self.dense_sampling = key("dense_sampling", "uniform")
        if self.dense_sampling not in ("uniform", "popularity"):
            raise ValueError(f"dense_sampling must be 'uniform' or 'popularity', got "
                             f"{self.dense_sampling!r}")
        self.dense_sampling_alpha = float(key("dense_sampling_alpha", 0.75))
        self.dense_sampling_smoothing = float(key("dense_sampling_smoothing", 1.0))
        if not (math.isfinite(self.dense_sampling_alpha)
                and math.isfinite(self.dense_sampling_smoothing)
                and self.dense_sampling_smoothing >= 0):
            raise ValueError("dense_sampling_alpha must be finite and dense_sampling_smoothing "
                             "finite and >= 0")
        if self.dense_sampling == "popularity" and not self.dense_negatives:
            raise ValueError("dense_sampling 'popularity' needs dense_negatives >= 1 (it is the "
                             "proposal of the sampled losses)")
        if self.bd_lru_only:  # RecBLR.py:33-35
            self.disable_conv1d = True
            self.disable_ffn = True
        # evaluate the last layer's position-wise tail only where gather_indexes
        # reads it (RECBLR_FULL_LAST_LAYER=1: every position, as the reference)
        self.gather_last_layer = os.environ.get("RECBLR_FULL_LAST_LAYER", "0") != "1"
        # run the encoder on each sequence's first item_seq_len positions only,
        # packed back to back (RECBLR_PACKED=0: the dense [B, L] batch, as the
        # reference); identical outputs and gradients, see DESIGN.md
        self.pack_sequences = os.environ.get("RECBLR_PACKED", "1") != "0"

        # run.py's Trainer moves each batch with Interaction.to(device): keep the
        # host lengths on the device tensor (no per-step sync in the packed forward)
        install_interaction_hook(self.ITEM_SEQ_LEN)
        self.item_embedding = nn.Embedding(self.n_items, self.hidden_size, padding_idx=0)
        self.layer_norm = nn.LayerNorm(self.hidden_size, eps=1e-12)
        self.dropout = nn.Dropout(self.dropout_prob)
        self.recurrent_layers = nn.ModuleList(
            RecurrentLayer(d_model=self.hidden_size, d_conv=self.d_conv, expand=self.expand,
                           dropout=self.dropout_prob, num_layers=self.num_layers,
                           bd_lru_only=self.bd_lru_only, disable_conv1d=self.disable_conv1d,
                           disable_ffn=self.disable_ffn)
            for _ in range(self.num_layers))
        if self.loss_type == "BPR":
            self.loss_fct = BPRLoss()
        elif self.loss_type == "CE":
            self.loss_fct = nn.CrossEntropyLoss()
        else:
            raise NotImplementedError("Make sure 'loss_type' in ['BPR', 'CE']!")
        # the popularity proposal (set_item_counts): derived from the data, so
        # not part of the state_dict
        self.register_buffer("neg_alias", None, persistent=False)
        self.register_buffer("neg_item_shift", None, persistent=False)
        self.apply(self._init_weights)

    def set_item_counts(self, counts):
        """Build the popularity proposal of dense_sampling 'popularity' from
        counts [n_items] (how often each item occurs in the train split,
        data.train_item_counts): kernels.negative_sampler with the model's
        dense_sampling_alpha and dense_sampling_smoothing over the ids [1,
        n_items), kept on the model's device as the non-persistent buffers
        neg_alias and neg_item_shift.  Returns the NegativeSampler (host
        tensors; .q is the proposal's exact distribution)."""
        if torch.is_tensor(counts):
            counts = counts.detach().cpu().numpy()
        sampler = negative_sampler(counts, self.dense_sampling_alpha,
                                   self.dense_sampling_smoothing, 1, self.n_items)
        dev = self.item_embedding.weight.device
        self.neg_alias = sampler.alias.to(dev)
        self.neg_item_shift = sampler.item_shift.to(dev)
        return sampler

    def _proposal(self):
        """(alias, item_shift) of the sampled losses' proposal: (None, None)
        for the uniform one."""
        if self.dense_sampling != "popularity":
            return None, None
        if self.neg_alias is None:
            raise RuntimeError("dense_sampling 'popularity' needs the items' train counts: call "
                               "model.set_item_counts(data.train_item_counts(dataset)) first "
                               "(trainer.fit does)")
        return self.neg_alias, self.neg_item_shift

    @staticmethod
    def _init_weights(module):
        # RecBLR.py:66-73: N(0, 0.02) for Linear/Embedding (every embedding row,
        # padding_idx included), zero Linear biases, LayerNorm (1, 0); the conv
        # keeps PyTorch's default init.
        if isinstance(module, (nn.Linear, nn.Embedding)):
            module.weight.data.normal_(std=0.02)
        elif isinstance(module, nn.LayerNorm):
            module.bias.data.zero_()
            module.weight.data.fill_(1.0)
        if isinstance(module, nn.Linear) and module.bias is not None:
            module.bias.data.zero_()

    def forward(self, item_seq, item_seq_len, exact_lengths: bool = False):
        """RecBLR.py:75-84.  exact_lengths=True makes each row behave as the
        batch-1 forward of its unpadded sequence item_seq[b, :len_b] (its own
        pow2 pad prefix), so users of different lengths batch together
        without changing results (run_with_unseen.py:222-225 runs them one
        by one)."""
        pad = row_pad_lens(item_seq_len) if exact_lengths else None
        if self.pack_sequences:
            return self._forward_packed(item_seq, item_seq_len, pad)
        n = len(self.recurrent_layers)
        rows = None
        if self.gather_last_layer:
            # Everything after the last layer's scan is position-wise and only
            # the positions gather_indexes picks reach the output: evaluate
            # that tail at those B positions (identical results).
            B, L = item_seq.shape
            rows = torch.arange(B, device=item_seq.device) * L + (item_seq_len - 1)
        slots = self._residual_slots(rows)
        h = embed_dropout_layer_norm(item_seq, self.item_embedding, self.dropout, self.layer_norm,
                                     self.training, slots[0])
        for i, layer in enumerate(self.recurrent_layers):
            if i == n - 1 and rows is not None:
                return layer(h, pad, rows, slot=slots[i])
            h = layer(h, pad, slot=slots[i], out_addend=slots[i + 1])
        return self.gather_indexes(h, item_seq_len - 1)

    def _residual_slots(self, last_rows):
        """One blocks.ResidualGrad per layer (+ None): layer i's residual
        gradient, taken by its input's producer (slot i is handed to that
        producer as its out_addend)."""
        n = len(self.recurrent_layers)
        if not torch.is_grad_enabled():
            return [None] * (n + 1)
        return [ResidualGrad(last_rows if i == n - 1 else None) for i in range(n)] + [None]

    def _forward_packed(self, item_seq, item_seq_len, pad, capture=None, all_rows=False):
        """all_rows: the last layer on full rows too, returns (h [ntok, d], seq)
        (forward_all) instead of the rows gather_indexes picks.
        capture: optional callable (layer index, seq, x, xc, rg, carries)
        run once per layer with the packed layout (kernels.Packed: offsets,
        order) and that layer's scan inputs and tile carries
        (recurrence.bd_lru); session.prefill(method="forward") reads the
        sessions' state from them.

        forward() on the valid positions only.  RecBole right-pads every
        sequence to L; the encoder is causal (causal conv, forward scan,
        position-wise projections / LayerNorms / FFN), so position t of row b
        influences only positions >= t of that row, and forward() returns
        position len_b - 1 (gather_indexes, RecBLR.py:84).  Positions >= len_b
        therefore never reach the output or any gradient; they are dropped
        before the embedding and the sequences run packed back to back
        ([ntok, d], ntok = sum of lengths; the recurrence kernels take the
        per-sequence offsets).  The pow2 pad prefix still uses the batch's L."""
        B, L = item_seq.shape
        dev = item_seq.device
        # sequences are packed longest first: the recurrence kernels give one
        # wave per sequence, so the short ones fill in behind the long ones
        host = getattr(item_seq_len, HOST_LENGTHS, None)
        if host is None or host.shape != item_seq_len.shape:
            # lengths only on the device: one sync (RecBole's Trainer path
            # attaches them instead, recbole_compat.install_interaction_hook)
            host = item_seq_len.to("cpu")
        lens_h = host.to(torch.int64).clamp(1, L)
        order_h = torch.argsort(lens_h, descending=True, stable=True)
        offs_h = torch.zeros(B + 1, dtype=torch.int64)
        lens_p = lens_h[order_h]
        torch.cumsum(lens_p, 0, out=offs_h[1:])
        ntok = int(offs_h[-1])
        both = _host_ring.stage(torch.cat([offs_h, order_h]), dev)
        offsets, order = both[:B + 1], both[B + 1:]
        pieces = None
        H = self.hidden_size * self.expand
        if fused_ok(True, H, not self.disable_conv1d, self.d_conv, torch.float32):
            G = _num_cus(dev)
            pieces = _host_ring32.stage(grl_pieces(lens_p, offs_h, G), dev)
            max_tiles = grl_max_tiles(lens_p, G)
        # one launch (rb_pack_plan): the packed item ids, each token's position
        # in its sequence (lets the conv forward tile the packed rows), each
        # batch row's packed index and last token
        ids, pos, inv, last = pack_plan(item_seq.to(torch.int64), offsets, order, ntok)
        seq = Packed(offsets, L, ntok, pos if _CONV_ROWS else None)
        seq.last, seq.inv, seq.order = last, inv, order
        if pieces is not None and pad is None:   # per-row pad prefixes: three-launch path
            seq.pieces, seq.G, seq.max_tiles = pieces, G, max_tiles
        if pad is not None:
            pad = pad.index_select(0, order)
        n = len(self.recurrent_layers)
        gather = self.gather_last_layer and not all_rows
        slots = self._residual_slots(last if gather else None)
        seq.ids = ids
        h = embed_dropout_layer_norm(ids, self.item_embedding, self.dropout, self.layer_norm,
                                     self.training, slots[0])
        for i, layer in enumerate(self.recurrent_layers):
            cap = None if capture is None else functools.partial(capture, i, seq)
            if i == n - 1 and gather:
                return layer(h, pad, last, seq, slot=slots[i], capture=cap)
            h = layer(h, pad, seq=seq, slot=slots[i], out_addend=slots[i + 1], capture=cap)
        if all_rows:
            return h, seq
        return h.index_select(0, last)

    def forward_all(self, item_seq, item_seq_len):
        """(h [ntok, d], seq): forward() at every valid position.  The encoder
        is causal and its pow2 pad prefix depends only on L, so row
        seq.offsets[s] + t holds what forward() returns for the prefix
        item_seq[seq.order[s], :t + 1] right-padded to L — the representation
        the reference computes for RecBole's augmented sample items[:t+1] ->
        items[t+1].  seq is the call's kernels.Packed (offsets, order, inv,
        last, ntok, and ids: the packed item ids); rows are in packed order,
        longest sequence first, and h[seq.last] equals forward().  The last
        layer runs on full rows like every other layer; gradients, dropout
        and hooks as in forward()."""
        if self.pack_sequences:
            return self._forward_packed(item_seq, item_seq_len, None, all_rows=True)
        # the dense [B, L] batch without the gather, its valid positions
        # selected into the packed order: one contract for both modes
        B, L = item_seq.shape
        dev = item_seq.device
        host = getattr(item_seq_len, HOST_LENGTHS, None)
        if host is None or host.shape != item_seq_len.shape:
            host = item_seq_len.to("cpu")
        lens_h = host.to(torch.int64).clamp(1, L)
        order_h = torch.argsort(lens_h, descending=True, stable=True)
        offs_h = torch.zeros(B + 1, dtype=torch.int64)
        torch.cumsum(lens_h[order_h], 0, out=offs_h[1:])
        ntok = int(offs_h[-1])
        both = _host_ring.stage(torch.cat([offs_h, order_h]), dev)
        offsets, order = both[:B + 1], both[B + 1:]
        ids, pos, inv, last = pack_plan(item_seq.to(torch.int64), offsets, order, ntok)
        seq = Packed(offsets, L, ntok, pos)
        seq.last, seq.inv, seq.order, seq.ids = last, inv, order, ids
        slots = self._residual_slots(None)
        h = embed_dropout_layer_norm(item_seq, self.item_embedding, self.dropout, self.layer_norm,
                                     self.training, slots[0])
        for i, layer in enumerate(self.recurrent_layers):
            h = layer(h, None, slot=slots[i], out_addend=slots[i + 1])
        row_of = torch.repeat_interleave(order, offsets[1:] - offsets[:-1], output_size=ntok)
        return h.reshape(B * L, -1).index_select(0, row_of * L + pos), seq

    def _scores_all(self, seq_output):
        return full_sort_scores(seq_output, self.item_embedding.weight)

    def calculate_loss_dense(self, interaction):
        """The CE loss at every valid position of every row: the mean over all
        ntok positions of -log softmax(h_t . items)[next item], the next item
        of a row's last position being POS_ITEM_ID.  Equals calculate_loss on
        the batch expanded to one right-padded row per prefix (RecBole's
        augmentation) with one encoder pass over the rows as they are."""
        if self.loss_type != "CE":
            raise ValueError("calculate_loss_dense needs loss_type 'CE'")
        h, seq = self.forward_all(interaction[self.ITEM_SEQ], interaction[self.ITEM_SEQ_LEN])
        pos_items = interaction[self.POS_ITEM_ID].to(torch.int64)
        m_pad = -(-seq.ntok // 256) * 256
        target = next_item_targets(seq.ids, seq.offsets, seq.order, pos_items, m_pad)
        if m_pad != seq.ntok:   # the loss's padding rows: zeros, target -1
            h = F.pad(h, (0, 0, 0, m_pad - seq.ntok))
        # every packed row is live (ntok from the host lengths: no sync)
        return item_cross_entropy_rows(h, self.item_embedding.weight, target, n_live=seq.ntok)

    def calculate_loss_pairs(self, interaction, negatives=None):
        """The sampled pairwise (BPR) loss at every valid position of every
        row: the mean over all positions t and negatives j of -log(1e-10 +
        sigmoid(h_t . E[next item] - h_t . E[neg_tj])).  negatives: int64
        [ntok or more rows, n] in packed order (forward_all's rows; -1 = no
        pair), or None: dense_negatives (at least 1) ids per position drawn on
        the device (kernels.sample_negatives, seeded from torch's generator
        like the dropout), uniform over the items outside the row's own
        window and target.  RecBole rejects against the user's whole history;
        a row here knows only its window.  With one negative per position
        this equals the reference's BPR calculate_loss on the batch expanded
        to one row per prefix with those negatives as NEG_ITEM_ID.
        dense_sampling 'popularity': the candidates come from the popularity
        proposal (set_item_counts) instead; the pairwise loss has no proposal
        correction, it simply meets harder negatives."""
        item_seq, lengths = interaction[self.ITEM_SEQ], interaction[self.ITEM_SEQ_LEN]
        alias, _ = self._proposal()
        h, seq = self.forward_all(item_seq, lengths)
        pos_items = interaction[self.POS_ITEM_ID].to(torch.int64)
        target = next_item_targets(seq.ids, seq.offsets, seq.order, pos_items)
        if negatives is None:
            negatives = sample_negatives(item_seq.to(torch.int64), lengths.to(torch.int64),
                                         pos_items, max(self.dense_negatives, 1), 1, self.n_items,
                                         draw_seed(), seq.offsets, seq.inv, seq.ntok, alias=alias)
        elif negatives.dim() != 2 or negatives.shape[0] < seq.ntok:
            raise ValueError(f"negatives must be [{seq.ntok} or more rows, n] in packed order, "
                             f"got {tuple(negatives.shape)}")
        return pair_loss(h, self.item_embedding.weight, target, negatives[:seq.ntok])

    def calculate_loss_sampled(self, interaction, negatives=None):
        """The sampled softmax at every valid position of every row, the
        negatives shared by the positions of a row: the mean over all
        positions t of logsumexp(z0, z_1 .. z_n) - z0 with z0 = h_t . E[next
        item] and z_j = h_t . E[neg_j] + shift (scoring.shared_softmax_loss).
        negatives: int64 [B, n] in batch-row order (-1 = no column), or None:
        dense_negatives ids per row drawn on the device (kernels.
        sample_negatives' last-position mode, seeded from torch's generator
        like the dropout), uniform over the items outside the row's window
        and target — every position's target is one of those, so a row's
        list is a valid list for each of its positions.  shift =
        log((n_items - 1) / n), the log-Q correction that makes sum_j
        exp(z_j) an estimate of the full softmax's sum over the other items
        (sampled_softmax_correct: False gives shift = 0).
        dense_sampling 'popularity': the candidates come from the popularity
        proposal q (set_item_counts) and the correction is per item, z_j = h_t
        . E[neg_j] - log(n q_j): shift = -log(n) plus item_shift = -log(q), the
        uniform formula's generalisation (both dropped with
        sampled_softmax_correct: False).  Rejecting against the row's window
        renormalises the proposal per row by 1 / (1 - q(seen)); as on the
        uniform path (which uses n_items - 1, not the unseen count) that factor
        is ignored."""
        item_seq, lengths = interaction[self.ITEM_SEQ], interaction[self.ITEM_SEQ_LEN]
        alias, item_shift = self._proposal()
        h, seq = self.forward_all(item_seq, lengths)
        pos_items = interaction[self.POS_ITEM_ID].to(torch.int64)
        # rows on the host (an encoder run elsewhere): the host restatements
        targets, draw = ((next_item_targets, sample_negatives) if h.is_cuda else
                         (next_item_targets_reference, sample_negatives_reference))
        target = targets(seq.ids, seq.offsets, seq.order, pos_items)
        if negatives is None:
            negatives = draw(item_seq.to(torch.int64), lengths.to(torch.int64), pos_items,
                             max(self.dense_negatives, 1), 1, self.n_items, draw_seed(),
                             alias=alias)
        elif negatives.dim() != 2 or negatives.shape[0] != item_seq.shape[0]:
            raise ValueError(f"negatives must be [{item_seq.shape[0]}, n] in batch-row order, "
                             f"got {tuple(negatives.shape)}")
        n = negatives.shape[1]
        if not self.sampled_softmax_correct:
            shift, item_shift = 0.0, None
        elif item_shift is not None:
            shift = -math.log(n)
        else:
            shift = math.log((self.n_items - 1) / n)
        return shared_softmax_loss(h, self.item_embedding.weight, target, negatives, seq.offsets,
                                   seq.order, shift, max_len=seq.L, item_shift=item_shift)

    def calculate_loss(self, interaction):
        if self.train_all_positions:
            if self.dense_negatives and self.dense_loss == "sampled_softmax":
                return self.calculate_loss_sampled(interaction)
            if self.dense_negatives:
                return self.calculate_loss_pairs(interaction)
            return self.calculate_loss_dense(interaction)
        seq_output = self.forward(interaction[self.ITEM_SEQ], interaction[self.ITEM_SEQ_LEN])
        pos_items = interaction[self.POS_ITEM_ID]
        if self.loss_type == "BPR":
            neg_items = interaction[self.NEG_ITEM_ID]
            pos_score = (seq_output * self.item_embedding(pos_items)).sum(-1)
            neg_score = (seq_output * self.item_embedding(neg_items)).sum(-1)
            return self.loss_fct(pos_score, neg_score)
        # logits + nn.CrossEntropyLoss fused on MFMA, [B, n_items] never stored
        return item_cross_entropy(seq_output, self.item_embedding.weight, pos_items)

    def predict(self, interaction):
        seq_output = self.forward(interaction[self.ITEM_SEQ], interaction[self.ITEM_SEQ_LEN])
        return (seq_output * self.item_embedding(interaction[self.ITEM_ID])).sum(dim=1)

    def full_sort_predict(self, interaction):
        seq_output = self.forward(interaction[self.ITEM_SEQ], interaction[self.ITEM_SEQ_LEN])
        return self._scores_all(seq_output)

    def full_sort_rank(self, interaction, first_item: int = 1, allow=None, allow_rows=None,
                       prior=None, prior_rows=None, prior_weight=None):
        """Rank of each row's target (POS_ITEM_ID) under full_sort_predict's
        scores without materialising them: (n_greater, n_equal) over items
        [first_item, n_items) (item 0 is RecBole's padding id, masked to -inf
        by its full-sort evaluator).  allow / allow_rows: a catalogue filter
        per row (scoring.item_filters, scoring.target_ranks).  prior /
        prior_rows / prior_weight: the ranks under score + weight * prior[item]
        (scoring.item_priors, scoring.target_ranks)."""
        seq_output = self.forward(interaction[self.ITEM_SEQ], interaction[self.ITEM_SEQ_LEN])
        return target_ranks(seq_output, self.item_embedding.weight,
                            interaction[self.POS_ITEM_ID], first_item, allow=allow,
                            allow_rows=allow_rows, prior=prior, prior_rows=prior_rows,
                            prior_weight=prior_weight)

    @torch.no_grad()
    def full_sort_topk(self, interaction, k: int = 10, exclude_seen: bool = True,
                       first_item: int = 1, allow=None, allow_rows=None, groups=None,
                       max_per_group=None, prior=None, prior_rows=None, prior_weight=None):
        """(ids, scores) [B, k]: each row's k best items under
        full_sort_predict's scores (RecBLR.py:114-122) without materialising
        them, by (score descending, id ascending) over items [first_item,
        n_items); exclude_seen drops the row's own ITEM_SEQ entries.  allow /
        allow_rows: a catalogue filter per row (scoring.item_filters,
        scoring.top_items).  groups / max_per_group: at most that many items
        of one group in a list (scoring.item_groups, scoring.top_items).  prior
        / prior_rows / prior_weight: rank by score + weight * prior[item]
        (scoring.item_priors, scoring.top_items)."""
        item_seq = interaction[self.ITEM_SEQ]
        seq_output = self.forward(item_seq, interaction[self.ITEM_SEQ_LEN])
        return top_items(seq_output, self.item_embedding.weight, k, first_item=first_item,
                         exclude=item_seq if exclude_seen else None, allow=allow,
                         allow_rows=allow_rows, groups=groups, max_per_group=max_per_group,
                         prior=prior, prior_rows=prior_rows, prior_weight=prior_weight)

    # ---- candidate lists (scoring.candidate_scores / top_candidates) ----------
    def predict_candidates(self, interaction, candidates):
        """scores [B, C] of each row's own candidates [B, C] (int64; an id
        outside [0, n_items) scores -inf): predict for several items per row.
        Under no_grad one launch after the forward, no [B, C, d] gather; with
        gradients enabled the torch expression, which backpropagates to the
        item table and the encoder."""
        seq_output = self.forward(interaction[self.ITEM_SEQ], interaction[self.ITEM_SEQ_LEN])
        return candidate_scores(seq_output, self.item_embedding.weight, candidates)

    @torch.no_grad()
    def rerank(self, interaction, candidates, k: int = 10, exclude_seen: bool = False,
               first_item: int = 1):
        """(ids, scores) [B, k]: each row's k best of its own candidates
        [B, C] (-1 pads a ragged list) by (score descending, id ascending) over
        the distinct ids in [first_item, n_items); exclude_seen drops the row's
        own ITEM_SEQ entries, as full_sort_topk does.  k = C orders the list."""
        item_seq = interaction[self.ITEM_SEQ]
        seq_output = self.forward(item_seq, interaction[self.ITEM_SEQ_LEN])
        return top_candidates(seq_output, self.item_embedding.weight, candidates, k,
                              first_item=first_item, exclude=item_seq if exclude_seen else None)

    @torch.no_grad()
    def sampled_rank(self, interaction, negatives, first_item: int = 1):
        """Rank of each row's target (POS_ITEM_ID) among its sampled negatives
        [B, n] (RecBole's uni100-style protocol): (n_greater, n_equal) for
        rank_metrics, negatives counted as listed, the target's own id skipped."""
        seq_output = self.forward(interaction[self.ITEM_SEQ], interaction[self.ITEM_SEQ_LEN])
        return candidate_ranks(seq_output, self.item_embedding.weight,
                               interaction[self.POS_ITEM_ID], negatives, first_item)

    # ---- stateful session inference (session.py) ----------------------------
    def session_open(self, capacity: int, seq_len: int | None = None, history: int = 0):
        """A session.SessionState of `capacity` slots for the window seq_len
        (default max_seq_length): after t <= seq_len appended items a slot's
        output equals forward() on the right-padded row of those items.
        history = S > 0: the slots also remember their last S item ids on the
        device (state.items, state.history(); session_recommend's seen-item
        lists)."""
        from .session import SessionState

        return SessionState(self, capacity, seq_len, history)

    def session_step(self, state, items, slots=None):
        """Append one item per row (0 = no event) and return the rows'
        seq_output [B, d]: the whole encoder in one launch (session.step)."""
        from .session import step

        return step(self, state, items, slots)

    def session_append(self, state, item_seq, item_seq_len=None, slots=None, reset: bool = False,
                       return_all: bool = False):
        """Append several events per row (item_seq [B, W], right-padded with
        0), 16 columns per launch, and return the slots' seq_output [B, d]
        (session.append); bitwise a session_step per column."""
        from .session import append

        return append(self, state, item_seq, item_seq_len, slots, reset, return_all)

    def session_prefill(self, state, item_seq, item_seq_len, slots=None, reset: bool = True,
                        method: str = "steps"):
        """Open sessions from stored histories (session.prefill): one step
        per column (method="steps"), or one packed forward whose
        intermediates give the state (method="forward")."""
        from .session import prefill

        return prefill(self, state, item_seq, item_seq_len, slots, reset, method)

    def session_recommend(self, state, items=None, slots=None, k: int = 10,
                          exclude_seen: bool = True, first_item: int = 1, allow=None,
                          allow_rows=None, groups=None, max_per_group=None, prior=None,
                          prior_rows=None, prior_weight=None):
        """(ids, scores) [B, k]: the rows' k best items after one step (items
        [B]) or append (items [B, W]), or from the slots' stored outputs (items
        None), the slots' own last S item ids excluded (session.recommend).
        allow / allow_rows: a catalogue filter per row (scoring.item_filters);
        groups / max_per_group: a cap per group (scoring.item_groups); prior /
        prior_rows / prior_weight: a score prior per row (scoring.item_priors)."""
        from .session import recommend

        return recommend(self, state, items, slots, k, exclude_seen, first_item, allow=allow,
                         allow_rows=allow_rows, groups=groups, max_per_group=max_per_group,
                         prior=prior, prior_rows=prior_rows, prior_weight=prior_weight)

    def session_rerank(self, state, candidates, items=None, slots=None, k: int = 10,
                       exclude_seen: bool = False, first_item: int = 1):
        """(ids, scores) [B, k]: the rows' own candidates [B, C] ordered for
        their sessions after one step (items [B]) or append (items [B, W]), or
        from the slots' stored outputs (items None) (session.rerank)."""
        from .session import rerank

        return rerank(self, state, candidates, items, slots, k, exclude_seen, first_item)

    def session_park(self, state, slots=None, release: bool = False, out=None):
        """The slots' sessions as rows of an int32 [B, state.blob_words] blob,
        one launch (session.park); release=True also frees the slots."""
        from .session import park

        return park(state, slots, release, out)

    def session_resume(self, state, blob, slots=None):
        """Put parked sessions (session_park's rows, or their host copy) into
        the slots; returns the rows' statuses (session.resume)."""
        from .session import resume

        return resume(state, blob, slots)

    def session_exchange(self, state, blob, slots=None, out=None):
        """Park the slots' sessions and resume the rows of blob into the same
        slots in one launch; returns the outgoing blob (session.exchange)."""
        from .session import exchange

        return exchange(state, blob, slots, out)

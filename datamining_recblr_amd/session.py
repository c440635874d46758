"""Stateful session inference: the encoder advanced by one event per call.

RecBLR is a linear recurrent model, so a user's history is summarised by a
fixed-size state and a new interaction costs O(1): ``step`` runs the whole
encoder for one new item per session slot in ONE launch (rb_session_step,
session/session_step.hip) instead of ``RecBLR.forward`` over the ``[B, L]``
history.

A session is opened for a window ``seq_len = L`` (default: the model's
``max_seq_length``).  After ``t <= L`` items have been appended to a slot its
output equals ``RecBLR.forward(item_seq, item_seq_len=t)`` in eval mode for the
``[1, L]`` right-padded row of those items (the default mode: the pad prefix
pow2(L) - L of the batch's L).  That holds because the pad prefix depends only
on L (``recurrence.pad_prefix_state``) and everything after it is causal
(``model.RecBLR._forward_packed``).  Past ``count == L`` the recurrence simply
continues over the whole history; the reference would slide its L-window
instead, which is not emulated.

State per slot (``SessionState``): per layer the recurrent state ``h [H]``
(initially that layer's pad-prefix state ``h0``) and the last ``K - 1``
pre-conv rows ``[K - 1, H]`` (initially zero: the reference's causal conv
zero-pads); ``count`` and the slot's last ``seq_output`` row ``out [d]``.

Item id 0 means "no event for this slot in this call": the state is untouched
and the returned row is the stored ``out``.  An item id outside ``[0, V)`` (or
a slot outside the state) is never dereferenced: the row is masked, its state
left alone, and ``state.status`` (int32 ``[B]``, a device tensor of the last
call: ``STEPPED``, ``NO_EVENT``, ``BAD_ITEM``, ``BAD_SLOT``) reports it without
a host sync.

``step_reference`` is the same step in plain torch ops on whatever device the
state lives on (CPU included): the checked restatement of the kernel, and the
path ``step`` takes for shapes the kernel refuses (``kernel_supports``).

``prefill`` opens sessions from stored histories: one step per column
(``method="steps"``, bitwise a step loop), or one packed forward plus one
rb_session_capture launch per layer (``method="forward"``,
session/session_capture.hip), which reads the state off the forward's
intermediates; ``capture_reference`` is that kernel's restatement in torch ops.

``append`` adds several events per slot at once: 16 columns of a right-padded
``[B, W]`` batch per launch (rb_session_append, session/session_append.hip: a
workgroup's 16 MFMA rows are T consecutive events of 16 / T slots), bitwise
what a ``step`` per column leaves, appendable to a live slot, and with
``reset=True`` a third way to open sessions from histories.
``append_reference`` is its restatement as a column loop of ``step_reference``.

A state opened with ``history=S`` also remembers, on the device, the last S
item ids each slot consumed (``SessionState.items [N, S]``, a ring positioned
by ``count``; rb_session_record, session/session_record.hip: one small launch
per call, before the encoder launches).  ``state.history()`` reads it oldest
first, and ``recommend`` is the serving call it is for: a step or an append,
then ``scoring.top_items`` with the slots' rings as the seen-item lists.
``record_reference`` is that kernel's restatement in torch ops.

A live session can leave its slot and come back later: ``park`` writes the
slots' whole state (h, conv history, count, out, item ring) as rows of an
int32 ``[B, W]`` blob in one launch (rb_session_transfer,
session/session_transfer.hip; the format is documented in
session/recblr_session.h), ``resume`` puts such rows into any slots of a state
of the same shape, ``exchange`` does both at once.  A row carries
``SessionState.blob_tag``; a row with another tag, a negative count or a ring
entry outside ``[-1, V)`` is refused as a whole (``BAD_BLOB``) and its slot left
alone.  ``transfer_reference`` is the kernel's restatement in torch ops.
"""
from __future__ import annotations

import ctypes
import os
import zlib

import torch
import torch.nn.functional as F

from . import _lib, kernels
from ._lib import RecBLRNativeError
from .recurrence import pad_prefix_state, pow2_pad_len

__all__ = ["SessionState", "EncoderParams", "step", "step_reference", "prefill",
           "capture_reference", "append", "append_reference", "record_reference", "recommend",
           "rerank",
           "kernel_supports", "STEPPED", "NO_EVENT", "BAD_ITEM", "BAD_SLOT", "park", "resume",
           "exchange", "transfer_reference", "MOVED", "BAD_BLOB"]

_header = _lib._read(os.path.join(_lib._HERE, "session", "recblr_session.h"))
STEPPED = _lib._define(_header, "RB_SESSION_STEPPED")
NO_EVENT = _lib._define(_header, "RB_SESSION_NO_EVENT")
BAD_ITEM = _lib._define(_header, "RB_SESSION_BAD_ITEM")
BAD_SLOT = _lib._define(_header, "RB_SESSION_BAD_SLOT")
MOVED = _lib._define(_header, "RB_SESSION_MOVED")
BAD_BLOB = _lib._define(_header, "RB_SESSION_BAD_BLOB")
BLOB_FORMAT = _lib._define(_header, "RB_SESSION_BLOB_FORMAT")
MAX_LAYERS = _lib._define(_header, "RB_SESSION_MAX_LAYERS")
MAX_LDS = _lib._define(_header, "RB_SESSION_MAX_LDS")
TILE = _lib._define(_header, "RB_SESSION_TILE")   # events per rb_session_append launch
LN_EPS = 1e-12   # every LayerNorm of the model (RecBLR.py:45, :131, :216)

_LAYER_FIELDS = ("w_in", "conv_w", "conv_b", "w_gate", "b_gate", "lam", "w_out", "ln_w", "ln_b",
                 "w1", "b1", "w2", "b2", "ffn_ln_w", "ffn_ln_b", "h0", "h", "conv_state")
# rb_session_layer's fields -> parameter names under recurrent_layers.{i}.
_PARAM_OF = {"w_in": "behavior_modeling.input.weight", "conv_w": "behavior_modeling.conv1d.weight",
             "conv_b": "behavior_modeling.conv1d.bias", "w_gate": "behavior_modeling.gates.weight",
             "b_gate": "behavior_modeling.gates.bias", "lam": "behavior_modeling.Lambda",
             "w_out": "behavior_modeling.output.weight", "ln_w": "layer_norm.weight",
             "ln_b": "layer_norm.bias", "w1": "ffn.w_1.weight", "b1": "ffn.w_1.bias",
             "w2": "ffn.w_2.weight", "b2": "ffn.w_2.bias", "ffn_ln_w": "ffn.layer_norm.weight",
             "ffn_ln_b": "ffn.layer_norm.bias"}


class _Layer(ctypes.Structure):
    """rb_session_layer (session/recblr_session.h)."""
    _fields_ = [(name, ctypes.c_void_p) for name in _LAYER_FIELDS]


class EncoderParams:
    """The tensors and flags one step reads: a ``state_dict``-style mapping
    with RecBLR's parameter names plus the configuration that is not in the
    tensors' shapes."""

    def __init__(self, tensors, num_layers: int, disable_conv1d: bool = False,
                 disable_ffn: bool = False):
        self.t = tensors
        self.num_layers = int(num_layers)
        self.use_conv = not disable_conv1d
        self.use_ffn = not disable_ffn
        emb = tensors["item_embedding.weight"]
        self.V, self.d = emb.shape
        self.H = tensors["recurrent_layers.0.behavior_modeling.Lambda"].shape[0]
        self.K = tensors["recurrent_layers.0.behavior_modeling.conv1d.weight"].shape[-1]
        self.device, self.dtype = emb.device, emb.dtype

    @classmethod
    def from_model(cls, model) -> "EncoderParams":
        return cls(dict(model.named_parameters()), len(model.recurrent_layers),
                   model.disable_conv1d, model.disable_ffn)

    @classmethod
    def from_state_dict(cls, state_dict, config) -> "EncoderParams":
        only = bool(config.get("bd_lru_only", False))   # RecBLR.py:33-35
        return cls(state_dict, config["num_layers"],
                   only or bool(config.get("disable_conv1d", False)),
                   only or bool(config.get("disable_ffn", False)))

    def layer(self, i: int, field: str) -> torch.Tensor:
        return self.t[f"recurrent_layers.{i}.{_PARAM_OF[field]}"]

    def conv_w(self, i: int) -> torch.Tensor:
        return self.layer(i, "conv_w").reshape(self.H, self.K)   # [H, 1, K] -> [H, K]

    @property
    def shape(self):
        return (self.V, self.d, self.H, self.K, self.num_layers, self.use_conv, self.use_ffn)


def _params(model_or_params) -> EncoderParams:
    if isinstance(model_or_params, EncoderParams):
        return model_or_params
    return EncoderParams.from_model(model_or_params)


def kernel_supports(d: int, H: int, K: int, num_layers: int) -> bool:
    """Whether rb_session_step takes this shape: d and H multiples of 16 (the
    MFMA tile), K in [1, 8], at most MAX_LAYERS layers, and the three LDS
    activation buffers within a compute unit's LDS."""
    if d % 16 or H % 16 or not 1 <= K <= 8 or not 1 <= num_layers <= MAX_LAYERS:
        return False
    return 0 < _lib.load_session().rb_session_lds_bytes(d, H) <= MAX_LDS


class SessionState:
    """The carried state of ``capacity`` session slots of one model, for the
    window ``seq_len`` (see the module doc).  ``h[i] [N, H]``, ``conv[i]
    [N, K-1, H]`` (None without a conv history), ``count [N]`` int64,
    ``out [N, d]``, ``h0[i] [H]``; ``status``: the last call's row statuses.
    ``history = S > 0`` adds ``items [N, S]`` int64, the ring of the last S item
    ids each slot consumed: event e of a slot since its reset (e from 0) at
    ``items[slot, e % S]``, -1 where nothing was written; ``count`` is its only
    position.  ``history = 0`` (the default): no ring, ``items is None``."""

    def __init__(self, model_or_params, capacity: int, seq_len: int | None = None,
                 history: int = 0):
        p = _params(model_or_params)
        if capacity <= 0:
            raise ValueError("SessionState: capacity must be positive")
        if history < 0:
            raise ValueError("SessionState: history must be >= 0 (0: no item ring)")
        if seq_len is None:
            seq_len = getattr(model_or_params, "max_seq_length", None)
        if seq_len is None or seq_len <= 0:
            raise ValueError("SessionState: seq_len must be a positive window length")
        self.source = model_or_params
        self.capacity, self.seq_len = int(capacity), int(seq_len)
        self.shape = p.shape
        self.device = p.device
        N, kw = self.capacity, dict(device=p.device, dtype=torch.float32)
        hist = p.use_conv and p.K > 1
        self.h = [torch.empty((N, p.H), **kw) for _ in range(p.num_layers)]
        self.conv = [torch.empty((N, p.K - 1, p.H), **kw) if hist else None
                     for _ in range(p.num_layers)]
        self.h0 = [torch.zeros((p.H,), **kw) for _ in range(p.num_layers)]
        self.count = torch.empty((N,), device=p.device, dtype=torch.int64)
        self.out = torch.empty((N, p.d), **kw)
        self.status = torch.zeros((0,), device=p.device, dtype=torch.int32)
        self.items = (torch.empty((N, int(history)), device=p.device, dtype=torch.int64)
                      if history else None)
        self._plan = None
        self._transfer_plan = None
        self.reset()

    @property
    def blob_words(self) -> int:
        """W, the 4-byte words of one parked session of this state
        (rb_session_blob_words: the one statement of the sum)."""
        _, d, H, K, layers, use_conv, _ = self.shape
        S = 0 if self.items is None else self.items.shape[1]
        W = _lib.load_session().rb_session_blob_words(d, H, K, layers, S, int(use_conv))
        if W < 0:
            raise ValueError(f"SessionState.blob_words: no blob format for the shape {self.shape}")
        return W

    @property
    def blob_tag(self) -> int:
        """Word 0 of this state's parked rows, as the int32 it is stored as:
        the CRC-32 of the format number, ``shape``, the ring length S and
        ``seq_len``, bit 0 forced on so it is never 0 (0 marks an invalid row).
        It guards the shape only: a blob of another model with the same shape
        (other weights) carries the same tag."""
        S = 0 if self.items is None else self.items.shape[1]
        text = repr((BLOB_FORMAT, tuple(int(v) for v in self.shape), int(S), self.seq_len))
        tag = zlib.crc32(text.encode()) | 1
        return tag - (1 << 32) if tag >= 1 << 31 else tag

    def blob_layout(self) -> dict:
        """name -> (first word, word count) of a parked row's parts, in row
        order: ``tag``, ``reserved``, ``count`` (int64, low word first), ``out``,
        per layer ``h{i}`` and ``conv{i}`` (absent without a conv history),
        ``items`` (the ring, int64 each; absent with history=0) and ``pad``
        (zeros up to a multiple of 4 words; absent when there is none)."""
        _, d, H, K, layers, use_conv, _ = self.shape
        S = 0 if self.items is None else self.items.shape[1]
        parts = [("tag", 1), ("reserved", 1), ("count", 2), ("out", d)]
        for i in range(layers):
            parts.append((f"h{i}", H))
            if use_conv and K > 1:
                parts.append((f"conv{i}", (K - 1) * H))
        if S:
            parts.append(("items", 2 * S))
        layout, w = {}, 0
        for name, n in parts:
            layout[name] = (w, n)
            w += n
        if w % 4:
            layout["pad"] = (w, 4 - w % 4)
        return layout

    @torch.no_grad()
    def reset(self, slots=None) -> None:
        """Re-initialise the slots (all of them by default) to the empty
        history; h0 is recomputed from the current parameters."""
        p = _params(self.source)
        if p.shape != self.shape:
            raise ValueError(f"SessionState.reset: the model's shape {p.shape} is not the one "
                             f"the state was opened for {self.shape}")
        P = pow2_pad_len(self.seq_len)
        for i, h0 in enumerate(self.h0):
            if not (P and p.use_conv):     # as recurrence.bd_lru: no prefix state
                h0.zero_()
                continue
            args = [p.layer(i, f).detach().float() for f in ("conv_b", "w_gate", "b_gate", "lam")]
            h0.copy_(kernels.pad_prefix_fwd(*args, P) if h0.device.type == "cuda"
                     else pad_prefix_state(*args, P))
        idx = slice(None) if slots is None else _slot_tensor(slots, self)
        for h, h0, conv in zip(self.h, self.h0, self.conv):
            h[idx] = h0
            if conv is not None:
                conv[idx] = 0.0
        self.count[idx] = 0
        self.out[idx] = 0.0
        if self.items is not None:
            self.items[idx] = -1

    @torch.no_grad()
    def history(self, slots=None):
        """The slots' recorded item ids (all slots by default), oldest first:
        ``(ids [n, S] int64, n_valid [n] int64)``, row i holding the slot's last
        ``n_valid[i] = min(count, S)`` events and -1 to the right of them.
        Torch ops on the state's device, no host sync."""
        if self.items is None:
            raise ValueError("SessionState.history: the state was opened without an item ring "
                             "(history=0)")
        S = self.items.shape[1]
        ring, count = self.items, self.count
        if slots is not None:
            idx = _slot_tensor(slots, self)
            ring, count = ring[idx], count[idx]
        n_valid = count.clamp(0, S)
        # a full ring starts at its oldest entry, count % S; a partial one at 0
        start = torch.where(count >= S, count % S, torch.zeros_like(count))
        col = torch.arange(S, device=self.device)[None]
        ids = ring.gather(1, (start[:, None] + col) % S)
        return torch.where(col < n_valid[:, None], ids, torch.full_like(ids, -1)), n_valid


def _slot_tensor(slots, state: SessionState) -> torch.Tensor:
    """slots as an int64 tensor on the state's device.  A list or CPU tensor
    is checked here (range, uniqueness); a device tensor is taken as is:
    uniqueness is then the caller's precondition (no sync on the hot path),
    and rb_session_step masks an out-of-range slot."""
    if isinstance(slots, torch.Tensor) and slots.device.type != "cpu":
        return slots.to(device=state.device, dtype=torch.int64).reshape(-1).contiguous()
    host = torch.as_tensor(slots, dtype=torch.int64).reshape(-1)
    if host.numel() and (int(host.min()) < 0 or int(host.max()) >= state.capacity):
        raise ValueError(f"slots must lie in [0, {state.capacity})")
    if torch.unique(host).numel() != host.numel():
        raise ValueError("slots must be unique: a slot takes one event per call")
    return host.to(state.device)


def _host_lengths(lengths, sync: bool = False):
    """The lengths as a host tensor, or None where they are known on the device
    only.  attach_host_lengths' copy wins; a list or CPU tensor counts as host
    lengths; a device tensor does not, unless sync (one device-to-host copy,
    as forward() pays)."""
    from .model import HOST_LENGTHS

    host = getattr(lengths, HOST_LENGTHS, None)
    if host is None and (sync or not (isinstance(lengths, torch.Tensor)
                                      and lengths.device.type != "cpu")):
        host = torch.as_tensor(lengths).to("cpu")
    return host


def _rows(state: SessionState, items, lengths=None, slots=None, name: str = "items",
          check_slots: bool = True, empty_ok: bool = False):
    """A call's rows on the state's device: ``(items [B, W'] int64, slots [B]
    or None, B, W')``.  items: [B, W] or [B] (W = 1).  With lengths the columns
    at or past a row's length are zeroed, and W' is cut to the longest row
    where the lengths are known on the host (_host_lengths).  slots go through
    _slot_tensor; check_slots=False only moves them (record_reference masks a
    bad slot, it refuses none).  name: what the messages call items."""
    items = torch.as_tensor(items, dtype=torch.int64)
    if items.dim() == 1:
        items = items[:, None]
    if items.dim() != 2:
        raise ValueError(f"{name} must be [B, W] (or [B]: one event per row)")
    B, W = items.shape
    if B == 0 and not empty_ok:
        raise ValueError(f"{name} must hold at least one row")
    items = items.to(state.device)
    if lengths is not None:
        host_len = _host_lengths(lengths)
        lens = torch.as_tensor(lengths).to(state.device).reshape(-1, 1)
        if lens.shape[0] != B:
            raise ValueError(f"{name} and item_seq_len must have the same number of rows")
        if host_len is not None:        # known on the host: stop at the longest row
            W = min(W, max(int(host_len.max()), 0)) if B else 0
        items = items[:, :W]
        items = torch.where(torch.arange(W, device=state.device)[None] < lens, items,
                            torch.zeros_like(items))
    if slots is None:
        if B > state.capacity:
            raise ValueError(f"{B} rows for a state of {state.capacity} slots")
    else:
        slots = (_slot_tensor(slots, state) if check_slots else
                 torch.as_tensor(slots, dtype=torch.int64).reshape(-1).to(state.device))
        if slots.numel() != B:
            raise ValueError(f"{name} and slots must have the same length")
    return items.contiguous(), slots, B, W


def _bad_slot(state: SessionState, slots) -> torch.Tensor:
    return (slots < 0) | (slots >= state.capacity)


def _stored_rows(state: SessionState, slots, B: int) -> torch.Tensor:
    """The slots' stored out rows [B, d]; zeros for a slot outside the state."""
    if slots is None:
        return state.out[:B].clone()
    y = state.out[slots.clamp(0, state.capacity - 1)]
    y[_bad_slot(state, slots)] = 0.0
    return y


def _idle_status(state: SessionState, slots, B: int) -> torch.Tensor:
    """The statuses of a call without a column: NO_EVENT, BAD_SLOT for a slot
    outside the state."""
    status = torch.full((B,), NO_EVENT, device=state.device, dtype=torch.int32)
    if slots is not None:
        status[_bad_slot(state, slots)] = BAD_SLOT
    return status


def _chunk_events(chunks, V: int):
    """The encoder kernel's masking rule for chunks [..., <= 16] of item ids:
    ``(live, bad)``.  live: the entries before a chunk's first 0, its events;
    bad [..., 1]: one of them lies outside [0, V), which masks the chunk."""
    live = (chunks != 0).cumprod(-1).bool()
    return live, (live & ((chunks < 0) | (chunks >= V))).any(-1, keepdim=True)


def _match(p: EncoderParams, state: SessionState) -> None:
    if p.shape != state.shape:
        raise ValueError(f"the state was opened for a different model shape: {state.shape} "
                         f"(V, d, H, K, layers, conv, ffn) vs the model's {p.shape}")
    if p.device != state.device:
        raise ValueError(f"the state lives on {state.device}, the model on {p.device}")


def _ln(p: EncoderParams, prefix: str, x):
    return F.layer_norm(x, (x.shape[-1],), p.t[prefix + "weight"], p.t[prefix + "bias"], eps=LN_EPS)


@torch.no_grad()
def record_reference(state: SessionState, items, slots=None, want_seen: bool = False):
    """rb_session_record in plain torch ops, on the state's device: write the
    events the encoder is about to consume into the state's item ring, and
    with want_seen return ``seen [B, S]``, the rows' rings as they stand
    afterwards (all -1 for a slot outside the state).  Call it before the
    encoder advances ``state.count``.

    items: int64 [B, W] right-padded with 0 (or [B]: W = 1), W >= 0; slots: int64
    [B], unique (None: slot b); a slot outside [0, N) is masked, not refused.
    The rule is the encoder kernels' masking, per row: cut the row into chunks
    of 16 columns (``TILE``); a chunk's events are its entries before its first
    0; a chunk with an event outside [0, V) contributes nothing; a bad slot
    records nothing.  Event j of the row's n recorded events goes to
    ``items[slot, (count[slot] + j) % S]``; when n > S only the last S are
    written."""
    ring = state.items
    if ring is None:
        raise ValueError("record_reference: the state was opened without an item ring "
                         "(history=0)")
    (N, S), V = ring.shape, state.shape[0]
    items, slots, B, W = _rows(state, items, None, slots, check_slots=False)
    if slots is None:
        slots = torch.arange(B, device=state.device)
    slot_ok = ~_bad_slot(state, slots)
    safe = slots.clamp(0, N - 1)
    nc = -(-W // TILE)
    chunks = F.pad(items, (0, nc * TILE - W)).reshape(B, nc, TILE)
    live, bad = _chunk_events(chunks, V)
    event = (live & ~bad & slot_ok[:, None, None]).reshape(B, nc * TILE)
    j = event.cumsum(1) - 1                                   # the event's number in its row
    keep = event & (j >= event.sum(1, keepdim=True) - S)      # the last S events
    pos = (state.count[safe][:, None] + j) % S
    # kept positions are distinct within a row; everything else lands in a
    # spare column S that is cut off again
    rows = torch.cat([ring[safe], ring.new_zeros((B, 1))], 1)
    rows.scatter_(1, torch.where(keep, pos, torch.full_like(pos, S)),
                  chunks.reshape(B, nc * TILE))
    rows = rows[:, :S]
    ring[slots[slot_ok]] = rows[slot_ok]
    if not want_seen:
        return None
    return torch.where(slot_ok[:, None], rows, torch.full_like(rows, -1))


def _record_kernel(state: SessionState, items, slots, seen) -> None:
    """One launch (rb_session_record): items [B, W] int64, contiguous."""
    B, W = items.shape
    N, S = state.items.shape
    _lib.call_session(
        "rb_session_record", items.data_ptr() if W else None, B, W,
        slots.data_ptr() if slots is not None else None, state.count.data_ptr(),
        state.items.data_ptr(), seen.data_ptr() if seen is not None else None, N, S,
        state.shape[0], kernels._stream(state.items))


def _record(state: SessionState, items, slots, want_seen: bool = False):
    """Record a call's [B, W] items on a GPU state before its encoder launches
    (they advance count): one rb_session_record launch; returns seen [B, S] or
    None.  Nothing at all for a state without a ring."""
    if state.items is None:
        return None
    B, W = items.shape
    if W == 0 and not want_seen:
        return None
    seen = (torch.empty((B, state.items.shape[1]), device=state.device, dtype=torch.int64)
            if want_seen else None)
    with torch.cuda.device(state.device):
        _record_kernel(state, items.contiguous(), slots, seen)
    return seen


def _step_reference(p: EncoderParams, state: SessionState, items, slots, record: bool = True,
                    want_seen: bool = False):
    """step_reference's body: (y, seen).  record=False: the caller has
    recorded the call's items already (append_reference's column loop)."""
    _match(p, state)
    items, stored, B, _ = _rows(state, torch.as_tensor(items).reshape(-1), None, slots)
    seen = None
    if record and state.items is not None:
        seen = record_reference(state, items, stored, want_seen)
    items = items[:, 0]
    slots = stored if stored is not None else torch.arange(B, device=state.device)
    slot_ok = ~_bad_slot(state, slots)
    item_ok = (items >= 0) & (items < p.V)
    valid = slot_ok & item_ok & (items != 0)
    status = torch.full((B,), NO_EVENT, device=state.device, dtype=torch.int32)
    status[valid] = STEPPED
    status[slot_ok & ~item_ok] = BAD_ITEM
    status[~slot_ok] = BAD_SLOT
    state.status = status
    idx, x = slots[valid], None
    if idx.numel():
        x = _ln(p, "layer_norm.", p.t["item_embedding.weight"][items[valid]].float())
    for i in range(p.num_layers if x is not None else 0):
        W = {f: p.layer(i, f).float() for f in _PARAM_OF if f != "conv_w"}
        H = p.H
        xz = x @ W["w_in"].t()
        u, z = xz[:, :H], xz[:, H:]
        if p.use_conv:
            win = u[:, None] if state.conv[i] is None else torch.cat(
                [state.conv[i][idx], u[:, None]], dim=1)              # [n, K, H], oldest first
            xc = F.silu(W["conv_b"] + (win * p.conv_w(i).float().t()[None]).sum(1))
            if state.conv[i] is not None:
                state.conv[i][idx] = win[:, 1:]
        else:
            xc = u
        r, g = (xc @ W["w_gate"].t() + W["b_gate"]).split(H, dim=-1)
        alpha = torch.exp(-F.softplus(W["lam"]) * torch.sigmoid(r))
        beta = torch.sqrt(1 - alpha * alpha + 1e-8) * torch.sigmoid(g)
        h = state.h[i][idx] * alpha + beta * xc
        state.h[i][idx] = h
        pre = f"recurrent_layers.{i}."
        x = _ln(p, pre + "layer_norm.", (F.silu(z) * h) @ W["w_out"].t() + x)
        if p.use_ffn:
            f = F.silu(x @ W["w1"].t() + W["b1"]) @ W["w2"].t() + W["b2"]
            x = _ln(p, pre + "ffn.layer_norm.", f + x)
    if x is not None:
        state.out[idx] = x
        state.count[idx] += 1
    return _stored_rows(state, stored, B), seen


@torch.no_grad()
def step_reference(model_or_params, state: SessionState, items, slots=None) -> torch.Tensor:
    """``step`` in plain torch ops (RecBLR.py:75-84 / :140-145 / :170-207 /
    :218-227 at one position), on the state's device; a state with an item
    ring records through record_reference."""
    return _step_reference(_params(model_or_params), state, items, slots)[0]


def _refuse_training(model) -> None:
    if model.training:
        raise ValueError("session step: the model is in training mode (dropout would be "
                         "active); call model.eval()")


def _refuse(model, p: EncoderParams, state: SessionState, hooks: bool = True) -> None:
    """What the fused step cannot honour is an error that names the cause.
    hooks=False: forward hooks are no obstacle (the caller runs the model's
    forward, which fires them)."""
    _refuse_training(model)
    if state.device.type != "cuda":
        raise RecBLRNativeError(f"session step: the state is on {state.device}; the HIP path "
                                "needs a ROCm GPU (step_reference runs anywhere)")
    for name, t in p.t.items():
        if t.dtype != torch.float32:
            raise RecBLRNativeError(f"session step: parameter {name} is {t.dtype}; the fused "
                                    "step takes fp32 parameters only")
    if not hooks:
        return
    # the fused step cannot fire module hooks: refuse rather than skip them
    g = torch.nn.modules.module
    if g._global_forward_hooks or g._global_forward_pre_hooks:
        raise RecBLRNativeError("session step: global forward hooks are registered; the fused "
                                "step cannot fire hooks")
    for name, m in model.named_modules():
        if name and (m._forward_hooks or m._forward_pre_hooks):
            raise RecBLRNativeError(f"session step: submodule {name} carries a forward hook; "
                                    "the fused step cannot fire hooks")


def _plan(p: EncoderParams, state: SessionState):
    """The rb_session_layer array for (parameters, state), rebuilt only when a
    tensor has moved."""
    tensors = []
    for i in range(p.num_layers):
        row = {f: p.layer(i, f) for f in _PARAM_OF}
        row["conv_w"] = p.conv_w(i)
        if not p.use_ffn:
            for f in ("w1", "b1", "w2", "b2", "ffn_ln_w", "ffn_ln_b"):
                row[f] = None
        if not p.use_conv:
            row["conv_w"] = row["conv_b"] = None
        row.update(h0=state.h0[i], h=state.h[i], conv_state=state.conv[i])
        tensors.append(row)
    key = tuple(t.data_ptr() if t is not None else 0 for row in tensors for t in row.values())
    if state._plan is not None and state._plan[0] == key:
        return state._plan[1]
    arr = (_Layer * p.num_layers)()
    for dst, row in zip(arr, tensors):
        for f, t in row.items():
            if t is not None and not t.is_contiguous():
                raise ValueError(f"session step: {f} must be contiguous")
            setattr(dst, f, t.data_ptr() if t is not None else None)
    state._plan = (key, arr)
    return arr


def _encoder_args(p: EncoderParams, state: SessionState, layers, items, slots, y):
    """The arguments rb_session_step and rb_session_append share: ``(head,
    tail)``, layers .. y and N .. stream; between them stand the entry's own
    ([y_all,] status, B [, T])."""
    t = p.t
    head = (ctypes.addressof(layers), p.num_layers, t["item_embedding.weight"].data_ptr(),
            t["layer_norm.weight"].data_ptr(), t["layer_norm.bias"].data_ptr(), LN_EPS,
            items.data_ptr(), slots.data_ptr() if slots is not None else None,
            state.count.data_ptr(), state.out.data_ptr(), y.data_ptr())
    tail = (state.capacity, p.V, p.d, p.H, p.K, int(not p.use_conv), int(not p.use_ffn),
            kernels._stream(y))
    return head, tail


def _step_kernel(p: EncoderParams, state: SessionState, layers, items, slots, y, status) -> None:
    """The one launch (rb_session_step): items [B] (or [B, 1]), one event per row."""
    head, tail = _encoder_args(p, state, layers, items, slots, y)
    _lib.call_session("rb_session_step", *head, status.data_ptr(), items.numel(), *tail)


@torch.no_grad()
def step(model, state: SessionState, items, slots=None) -> torch.Tensor:
    """Append items[b] to slot slots[b] (slots None: slot b) and return the
    rows' seq_output [B, d]: one launch for the whole encoder.  items: int64
    [B], list or tensor; 0 = no event for that row.  slots must be unique: a
    list or CPU tensor is checked, for a device tensor it is a precondition
    (no sync on the hot path).  A shape the kernel refuses (kernel_supports)
    runs step_reference instead.  A state with an item ring records the items
    first (one rb_session_record launch)."""
    return _step(model, state, items, slots)[0]


def _step(model, state: SessionState, items, slots, want_seen: bool = False):
    """step's body: (y, seen [B, S] or None)."""
    p = _params(model)
    _refuse(model, p, state)
    _match(p, state)
    if not kernel_supports(p.d, p.H, p.K, p.num_layers):
        return _step_reference(p, state, items, slots, want_seen=want_seen)
    items, slots, B, _ = _rows(state, torch.as_tensor(items).reshape(-1), None, slots)
    seen = _record(state, items, slots, want_seen)
    y = torch.empty((B, p.d), device=state.device, dtype=torch.float32)
    status = torch.empty((B,), device=state.device, dtype=torch.int32)
    with torch.cuda.device(state.device):
        _step_kernel(p, state, _plan(p, state), items, slots, y, status)
    state.status = status
    return y, seen


def _first_status(seen, new):
    """Per row the first status over the chunks that is not NO_EVENT."""
    return new if seen is None else torch.where(seen == NO_EVENT, new, seen)


@torch.no_grad()
def append_reference(model_or_params, state: SessionState, item_seq, item_seq_len=None,
                     slots=None, reset: bool = False, return_all: bool = False):
    """``append`` as a column loop of ``step_reference``, on the state's
    device: the checked restatement of rb_session_append, one 16-column chunk
    after the other.  Within a chunk a row's events are the entries before its
    first 0; a row with an event outside [0, V) among them is masked for the
    whole chunk (BAD_ITEM: nothing of its slot is touched).  A state with an
    item ring records the whole [B, W'] once, through record_reference."""
    return _append_reference(_params(model_or_params), state, item_seq, item_seq_len, slots,
                             reset, return_all)[0]


def _append_reference(p: EncoderParams, state: SessionState, item_seq, item_seq_len, slots,
                      reset: bool, return_all: bool, want_seen: bool = False):
    """append_reference's body: (its result, seen [B, S] or None)."""
    _match(p, state)
    items, slots, B, W = _rows(state, item_seq, item_seq_len, slots, "item_seq")
    if reset:
        state.reset(slots if slots is not None else torch.arange(B))
    seen = None
    if state.items is not None and (W or want_seen):
        seen = record_reference(state, items, slots, want_seen)
    y, status, cols = _stored_rows(state, slots, B), None, []
    for c0 in range(0, W, TILE):
        chunk = items[:, c0:c0 + TILE]
        live, bad = _chunk_events(chunk, p.V)
        fed = torch.where(live & ~bad, chunk, torch.zeros_like(chunk))
        st = torch.full((B,), NO_EVENT, device=state.device, dtype=torch.int32)
        for t in range(chunk.shape[1]):
            y = _step_reference(p, state, fed[:, t], slots, record=False)[0]
            if t == 0:
                st = state.status.clone()          # STEPPED, NO_EVENT or BAD_SLOT
            cols.append(torch.where((fed[:, t] != 0)[:, None] & (state.status == STEPPED)[:, None],
                                    y, torch.zeros_like(y)))
        st[bad[:, 0] & (st != BAD_SLOT)] = BAD_ITEM
        status = _first_status(status, st)
    state.status = status if status is not None else _idle_status(state, slots, B)
    if not return_all:
        return y, seen
    y_all = torch.stack(cols, 1) if cols else y.new_zeros((B, 0, p.d))
    return (y, y_all), seen


def _append_kernel(p: EncoderParams, state: SessionState, layers, items, slots, y, y_all,
                   status) -> None:
    """One launch (rb_session_append): items [B, T], T events per row."""
    head, tail = _encoder_args(p, state, layers, items, slots, y)
    _lib.call_session("rb_session_append", *head,
                      y_all.data_ptr() if y_all is not None else None, status.data_ptr(),
                      *items.shape, *tail)


@torch.no_grad()
def append(model, state: SessionState, item_seq, item_seq_len=None, slots=None,
           reset: bool = False, return_all: bool = False):
    """Append row b's events item_seq[b, :] to slot slots[b] (slots None: slot
    b), 16 columns per launch, and return the slots' seq_output [B, d]
    afterwards; with return_all=True ``(y, y_all [B, W', d])``, the output
    after every event (zeros where a row has none), W' the columns processed.

    item_seq: int64 [B, W] right-padded with 0 (or [B]: W = 1).  With
    item_seq_len the columns at or past a row's length are zeroed; lengths
    known on the host (a list, a CPU tensor, attach_host_lengths) also stop
    the loop at the longest row, lengths on the device cost no sync and all W
    columns are processed.  Each chunk of 16 columns is one rb_session_append
    launch; a last chunk of r < 16 columns is zero-padded to the smallest T of
    1, 2, 4, 8, 16 that holds it (a workgroup carries 16 / T rows).  A slot is
    left bitwise as a ``step`` per column would leave it, past the window too.

    reset=True resets the rows' slots first: ceil(L / 16) launches open
    sessions from L-item histories.  ``state.status`` holds per row the first
    status over the chunks that is not NO_EVENT.  A row with an id outside
    [0, V) among a chunk's events is masked for that chunk (BAD_ITEM) and keeps
    the events of the chunks before it: a launch is atomic per row, the call
    is not.  slots, the refusals and the fallback are ``step``'s: a shape the
    kernel refuses (kernel_supports) or a state on the CPU runs
    append_reference.  A state with an item ring records the whole [B, W']
    first: one rb_session_record launch per call, after the reset and before
    the first encoder launch."""
    return _append(model, state, item_seq, item_seq_len, slots, reset, return_all)[0]


def _append(model, state: SessionState, item_seq, item_seq_len, slots, reset: bool,
            return_all: bool, want_seen: bool = False):
    """append's body: (its result, seen [B, S] or None)."""
    p = _params(model)
    _refuse_training(model)
    if state.device.type != "cuda":
        return _append_reference(p, state, item_seq, item_seq_len, slots, reset, return_all,
                                 want_seen)
    _refuse(model, p, state)
    _match(p, state)
    if not kernel_supports(p.d, p.H, p.K, p.num_layers):
        return _append_reference(p, state, item_seq, item_seq_len, slots, reset, return_all,
                                 want_seen)
    items, slots, B, W = _rows(state, item_seq, item_seq_len, slots, "item_seq")
    if reset:
        state.reset(slots if slots is not None else torch.arange(B))
    seen = _record(state, items, slots, want_seen)
    kw = dict(device=state.device, dtype=torch.float32)
    y, status, cols = (torch.empty((B, p.d), **kw) if W else None), None, []
    with torch.cuda.device(state.device):
        layers = _plan(p, state)
        for c0 in range(0, W, TILE):
            r = min(TILE, W - c0)
            T = 1 << (r - 1).bit_length()
            chunk = F.pad(items[:, c0:c0 + r], (0, T - r)).contiguous()
            y_all = torch.empty((B, T, p.d), **kw) if return_all else None
            st = torch.empty((B,), device=state.device, dtype=torch.int32)
            _append_kernel(p, state, layers, chunk, slots, y, y_all, st)
            status = _first_status(status, st)
            if return_all:
                cols.append(y_all[:, :r])
    if y is None:                       # no column at all
        y, status = _stored_rows(state, slots, B), _idle_status(state, slots, B)
    state.status = status
    if not return_all:
        return y, seen
    return (y, (torch.cat(cols, 1) if cols else y.new_zeros((B, 0, p.d)))), seen


@torch.no_grad()
def capture_reference(u, xc, rg, lam, gate_b, carries, seq_offsets, slots, h,
                      conv_state=None) -> None:
    """rb_session_capture in plain torch ops, on the tensors' device: the
    state of one layer after each packed sequence's last position, read off
    that layer's forward.  u, xc [ntok, H] (pre-conv rows, conv + SiLU
    output), rg [ntok, 2H] (gates GEMM without bias), carries
    [B, tiles, H] (the state entering every RB_TILE-step tile, as the gate
    scan wrote them), seq_offsets [B + 1], slots [B].  Writes h[slots[b]] =
    the carry of sequence b's last tile advanced by that tile's steps, and
    conv_state[slots[b]] ([N, K - 1, H], or None) = the last K - 1 rows of u,
    oldest first, zeros before the sequence's start.  A sequence that is
    empty, has more tiles than carries holds, or names a slot outside
    [0, N) is skipped; no other slot is written."""
    T, (N, H) = _lib.RB_TILE, h.shape
    B, ntok, dev = seq_offsets.numel() - 1, u.shape[0], h.device
    start, n = seq_offsets[:-1], seq_offsets[1:] - seq_offsets[:-1]
    valid = (n >= 1) & (n <= carries.shape[1] * T) & (slots >= 0) & (slots < N)
    nc = n.clamp(1, carries.shape[1] * T)        # skipped sequences: any row in range
    tile = (nc - 1) // T
    hv = carries[torch.arange(B, device=dev), tile]
    nsp = -F.softplus(lam)
    for s in range(T):
        t = tile * T + s
        row = (start + torch.minimum(t, nc - 1)).clamp(0, ntok - 1)
        alpha = torch.exp(nsp * torch.sigmoid(rg[row, :H] + gate_b[:H]))
        beta = torch.sqrt(1 - alpha * alpha + 1e-8) * torch.sigmoid(rg[row, H:] + gate_b[H:])
        hv = torch.where((t < nc)[:, None], hv * alpha + beta * xc[row], hv)
    idx = slots[valid]
    h[idx] = hv[valid]
    if conv_state is not None and conv_state.shape[1]:
        hist = conv_state.shape[1]
        pos = n[:, None] - hist + torch.arange(hist, device=dev)[None]        # [B, K - 1]
        rows = (start[:, None] + pos.clamp_min(0)).clamp(0, ntok - 1)
        conv_state[idx] = torch.where((pos >= 0)[..., None], u[rows], 0.0)[valid]


def _row_stride(t: torch.Tensor, C: int) -> int:
    return t.stride(0) if t.shape[0] > 1 else C


def _capture_kernel(state: SessionState, i: int, u, xc, rg, lam, gate_b, carries, seq, slots,
                    K: int) -> None:
    """One launch (rb_session_capture): layer i's state from its forward."""
    H, conv = u.shape[1], state.conv[i]
    _lib.call_session(
        "rb_session_capture", u.data_ptr(), _row_stride(u, H), xc.data_ptr(), _row_stride(xc, H),
        rg.data_ptr(), _row_stride(rg, 2 * H), lam.data_ptr(), gate_b.data_ptr(),
        carries.data_ptr(), seq.offsets.data_ptr(), slots.data_ptr(), state.h[i].data_ptr(),
        conv.data_ptr() if conv is not None else None, seq.B, seq.L, state.capacity, H, K,
        kernels._stream(u))


def _capture_ok(H: int, K: int, u, xc, rg, *aligned) -> bool:
    """Whether rb_session_capture's argument check passes: 16-byte row
    pieces (H and the row strides multiples of 4, aligned pointers)."""
    if H % 4 or not 1 <= K <= 8:
        return False
    if any(t.stride(1) != 1 or _row_stride(t, C) % 4 for t, C in ((u, H), (xc, H), (rg, 2 * H))):
        return False
    return all(t is None or (t.is_contiguous() and t.data_ptr() % 16 == 0) for t in aligned) \
        and all(t.data_ptr() % 16 == 0 for t in (u, xc, rg))


def _prefill_forward(model, state: SessionState, item_seq, item_seq_len, slots):
    """prefill(method="forward"), see prefill."""
    from .model import attach_host_lengths

    # lengths only on the device: one sync, as forward()
    host_len = _host_lengths(item_seq_len, sync=True).to(torch.int64).reshape(-1)
    # no lengths for _rows: the forward reads none of the columns past a
    # length, and zeroing them measurably slowed a host-bound call
    seq, slots, B, T = _rows(state, item_seq, None, slots, "item_seq", empty_ok=True)
    if host_len.numel() != B:
        raise ValueError("item_seq and item_seq_len must have the same number of rows")
    dev, lens_h = state.device, host_len
    longest = int(host_len.max()) if B else 0
    if longest > state.seq_len:
        raise ValueError(f'prefill(method="forward"): a history of {longest} items is longer '
                         f"than the state's window seq_len = {state.seq_len} "
                         '(method="steps" continues past the window)')
    if longest > T:
        raise ValueError(f'prefill(method="forward"): a length of {longest} exceeds item_seq\'s '
                         f"width {T}")
    p = _params(model)
    _refuse(model, p, state, hooks=False)
    _match(p, state)
    if slots is None:
        slots = torch.arange(B, device=dev)
    state.reset(slots)
    status = torch.full((B,), NO_EVENT, device=dev, dtype=torch.int32)
    y = torch.zeros((B, p.d), device=dev, dtype=torch.float32)
    state.status = status
    rows_h = torch.nonzero(host_len > 0).reshape(-1)    # a row of length 0 stays reset
    if rows_h.numel() == 0:
        return y
    if rows_h.numel() < B:
        rows = rows_h.to(dev)
        seq, slots, lens_h = seq.index_select(0, rows), slots.index_select(0, rows), host_len[rows_h]
    # the state's window: its pad prefix pow2(L) - L is the forward's.  Ids are
    # clamped into the table (forward()'s contract is ids in [1, V))
    L = state.seq_len
    seq = (seq[:, :L] if T >= L else F.pad(seq, (0, L - T))).clamp(0, p.V - 1).contiguous()
    lens = attach_host_lengths(lens_h.to(dev), lens_h)
    K = p.K if p.use_conv else 1
    if state.items is not None:     # the rows the forward consumes, before count moves
        _record(state, torch.where(torch.arange(L, device=dev)[None] < lens[:, None], seq,
                                   torch.zeros_like(seq)), slots)
    packed_slots = []

    def sink(i, packed, u, xc, rg, carries):
        if not packed_slots:        # sequence b of the packed order is row packed.order[b]
            packed_slots.append(slots.index_select(0, packed.order).contiguous())
        lam, gate_b = p.layer(i, "lam"), p.layer(i, "b_gate")
        if _capture_ok(p.H, K, u, xc, rg, lam, gate_b, carries, state.h[i], state.conv[i]):
            _capture_kernel(state, i, u, xc, rg, lam, gate_b, carries, packed, packed_slots[0], K)
        else:
            capture_reference(u, xc, rg, lam, gate_b, carries, packed.offsets, packed_slots[0],
                              state.h[i], state.conv[i])

    with torch.cuda.device(dev):
        out = model._forward_packed(seq, lens, None, capture=sink)
    state.out[slots] = out
    state.count[slots] = lens
    if rows_h.numel() < B:
        status[rows] = STEPPED
        y[rows] = out
        return y
    status.fill_(STEPPED)
    return out


@torch.no_grad()
def prefill(model, state: SessionState, item_seq, item_seq_len, slots=None,
            reset: bool = True, method: str = "steps") -> torch.Tensor:
    """Open sessions from stored histories: item_seq [B, T] right-padded,
    item_seq_len [B].  Returns the rows' seq_output [B, d].

    method="steps" (the default): one step per column (item 0 for rows
    already exhausted), so exact by construction.  The slots are reset first
    unless reset=False (which appends to what they hold).  A state on the CPU
    steps with step_reference.

    method="forward": one packed forward over the histories
    (RecBLR._forward_packed at the state's window, whatever RECBLR_PACKED
    says) and one rb_session_capture launch per layer, which reads the slots'
    state off the forward's intermediates: h from the gate scan's tile
    carries, the conv history from the in-projection's rows; out is the
    forward's row, count the length.  No step launch.  It needs reset=True,
    every length <= state.seq_len, item ids of [1, V) in the valid prefixes
    (forward()'s contract; step's "item 0 = no event" has no meaning inside a
    history), an eval-mode fp32 model and a GPU state; forward hooks fire.  A
    row of length 0 is reset and returns its zero row.  The state agrees with
    the step-built one to rounding (the forward's f16x3 projections against
    the step's fp32 MFMA), not bitwise."""
    if method not in ("steps", "forward"):
        raise ValueError(f'prefill: method must be "steps" or "forward", got {method!r}')
    if method == "forward" and not reset:
        raise ValueError('prefill(method="forward") needs reset=True: the forward starts from '
                         'the empty history (method="steps" appends to a slot)')
    item_seq = torch.as_tensor(item_seq, dtype=torch.int64)
    if item_seq.dim() != 2:
        raise ValueError("item_seq must be [B, T]")
    if method == "forward":
        return _prefill_forward(model, state, item_seq, item_seq_len, slots)
    items, slots, B, T = _rows(state, item_seq, item_seq_len, slots, "item_seq", empty_ok=True)
    cols = items.t().contiguous()
    if reset:
        state.reset(slots if slots is not None else torch.arange(B))
    fn = step if state.device.type == "cuda" else step_reference
    y = None
    for t in range(T):
        y = fn(model, state, cols[t], slots)
    return y if y is not None else _stored_rows(state, slots, B)


@torch.no_grad()
def recommend(model, state: SessionState, items=None, slots=None, k: int = 10,
              exclude_seen: bool = True, first_item: int = 1, allow=None, allow_rows=None,
              groups=None, max_per_group=None, prior=None, prior_rows=None, prior_weight=None):
    """Click in, recommendation list out: ``(ids int64 [B, k], scores fp32
    [B, k])``, each row's k best items by ``scoring.top_items`` for its slot's
    seq_output after the call's events.

    items None: no event, the slots' stored ``out`` rows (slots None: every
    slot of the state).  items [B]: one ``step`` first; items [B, W]: one
    ``append`` first (right-padded with 0).  With exclude_seen the slot's item
    ring as it stands after those events (its last S item ids, ``history=S``) is
    the seen-item list: the record launch of the step or append writes the
    [B, S] rows ``top_items`` excludes, so nothing is gathered or copied from
    the host.  A state opened without a ring cannot exclude: ValueError.

    A row whose slot lies outside the state, or whose slot has consumed no
    event yet (count == 0: its ``out`` is the zero row), returns id -1 and score
    -inf in every position (masked on the device, no sync).  slots, the
    refusals and the fallbacks are ``step``'s; a state on the CPU runs the
    whole call in torch ops.  ``state.status`` is left as the step or append
    left it.

    allow (``scoring.item_filters``) and allow_rows [B] restrict each row to a
    catalogue filter, as ``scoring.top_items`` takes them: the row's filter
    index, None for filter 0 everywhere, -1 for no filter.  groups
    (``scoring.item_groups``) and max_per_group cap every list at that many
    items of one group, again as ``scoring.top_items`` takes them.  prior
    (``scoring.item_priors``), prior_rows [B] and prior_weight (a float or a
    float [B] tensor) rank each row by score + weight * prior[item], likewise."""
    from .scoring import top_items

    p, y, seen, dead = _serve_rows(model, state, items, slots, exclude_seen, "recommend")
    ids, scores = top_items(y, p.t["item_embedding.weight"], k, first_item,
                            exclude=seen if exclude_seen else None, allow=allow,
                            allow_rows=allow_rows, groups=groups, max_per_group=max_per_group,
                            prior=prior, prior_rows=prior_rows, prior_weight=prior_weight)
    ids.masked_fill_(dead[:, None], -1)
    scores.masked_fill_(dead[:, None], float("-inf"))
    return ids, scores


def _serve_rows(model, state: SessionState, items, slots, exclude_seen: bool, who: str):
    """The front half recommend and rerank share: the call's events, then
    ``(params, y [B, d], seen [B, S] or None, dead [B])`` — the rows'
    seq_output afterwards, their item rings as the seen lists (with
    exclude_seen) and the rows that must come back as -1 / -inf (a slot outside
    the state, or one that has consumed no event yet)."""
    if exclude_seen and state.items is None:
        raise ValueError(f"{who}(exclude_seen=True) needs the slots' item ring: open the "
                         "state with history=S (session_open(capacity, history=S)), or pass "
                         "exclude_seen=False")
    p = _params(model)
    on_gpu = state.device.type == "cuda"
    if items is None:
        _refuse_training(model)
        if on_gpu:
            _refuse(model, p, state)
        _match(p, state)
        B = state.capacity if slots is None else torch.as_tensor(slots).numel()
        none, slots, B, _ = _rows(state, torch.empty((B, 0)), None, slots, "slots")
        y, seen = _stored_rows(state, slots, B), None
        if exclude_seen:
            seen = (_record(state, none, slots, True) if on_gpu
                    else record_reference(state, none, slots, True))
    else:
        items = torch.as_tensor(items, dtype=torch.int64)
        if items.dim() == 1 and on_gpu:
            y, seen = _step(model, state, items, slots, exclude_seen)
        elif items.dim() == 1:
            _refuse_training(model)
            y, seen = _step_reference(p, state, items, slots, want_seen=exclude_seen)
        else:
            y, seen = _append(model, state, items, None, slots, False, False, exclude_seen)
        B = y.shape[0]
        if slots is not None:
            slots = _slot_tensor(slots, state)
    if slots is None:
        dead = state.count[:B] == 0
    else:
        dead = _bad_slot(state, slots) | (state.count[slots.clamp(0, state.capacity - 1)] == 0)
    return p, y, seen, dead


@torch.no_grad()
def rerank(model, state: SessionState, candidates, items=None, slots=None, k: int = 10,
           exclude_seen: bool = False, first_item: int = 1):
    """Order these items for this session: ``(ids int64 [B, k], scores fp32
    [B, k])``, each row's k best of its own candidates [B, C] (int64, -1 pads a
    ragged list) by ``scoring.top_candidates`` for its slot's seq_output after
    the call's events; k = C orders the whole list.

    items, slots, the masked rows (-1 / -inf for a slot outside the state or
    one without an event yet), the refusals and the fallbacks are exactly
    ``recommend``'s; exclude_seen drops the ids in the slot's item ring and
    needs a state opened with ``history=S``.  A state on the CPU runs the whole
    call in torch ops."""
    from .scoring import top_candidates

    candidates = torch.as_tensor(candidates, dtype=torch.int64)
    if candidates.dim() != 2:
        raise ValueError(f"candidates must be [B, C], got {tuple(candidates.shape)}")
    # the call's rows, known before any event is consumed
    B = (torch.as_tensor(items).shape[0] if items is not None
         else state.capacity if slots is None else torch.as_tensor(slots).numel())
    if candidates.shape[0] != B:
        raise ValueError(f"candidates has {candidates.shape[0]} rows, the call {B}")
    p, y, seen, dead = _serve_rows(model, state, items, slots, exclude_seen, "rerank")
    ids, scores = top_candidates(y, p.t["item_embedding.weight"], candidates.to(state.device), k,
                                 first_item, exclude=seen if exclude_seen else None)
    ids.masked_fill_(dead[:, None], -1)
    scores.masked_fill_(dead[:, None], float("-inf"))
    return ids, scores


# ---- parked sessions ------------------------------------------------------------
def _blob_check(state: SessionState, blob, B, name: str, who: str, device_ok) -> None:
    """A blob argument is int32 [B, W], contiguous, on one of device_ok."""
    if not isinstance(blob, torch.Tensor) or blob.dtype != torch.int32:
        raise ValueError(f"{who}: {name} must be an int32 tensor")
    if blob.dim() != 2 or blob.shape[1] != state.blob_words:
        raise ValueError(f"{who}: {name} must be [B, {state.blob_words}] (state.blob_words), "
                         f"got {tuple(blob.shape)}")
    if B is not None and blob.shape[0] != B:
        raise ValueError(f"{who}: slots and {name} must have the same length "
                         f"({B} slots, {blob.shape[0]} rows)")
    if not blob.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous")
    if blob.device not in device_ok:
        raise ValueError(f"{who}: {name} is on {blob.device}, the state on {state.device}")


def _overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.device != b.device or not a.numel() or not b.numel():
        return False
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * 4 and b0 < a0 + a.numel() * 4


def _transfer_rows(state: SessionState, slots, blob_in, out, who: str, check_slots: bool = True):
    """A transfer call's rows: ``(slots [B] or None, blob_in on the state's
    device or None, B)``, with the blobs validated (ValueError)."""
    if slots is not None:
        slots = (_slot_tensor(slots, state) if check_slots else
                 torch.as_tensor(slots, dtype=torch.int64).reshape(-1).to(state.device))
    B = None if slots is None else slots.numel()
    if blob_in is not None:
        _blob_check(state, blob_in, B, "blob", who, (state.device, torch.device("cpu")))
        B = blob_in.shape[0]
        blob_in = blob_in.to(state.device)      # a host blob: one copy to the device
    elif B is None:
        B = state.capacity
    if B == 0:
        raise ValueError(f"{who}: no row to move")
    if slots is None and B > state.capacity:
        raise ValueError(f"{who}: {B} rows for a state of {state.capacity} slots")
    if out is not None:
        _blob_check(state, out, B, "out", who, (state.device,))
        if blob_in is not None and _overlap(blob_in, out):
            raise ValueError(f"{who}: the incoming blob and out overlap")
    return slots, blob_in, B


def _blob_words(t: torch.Tensor, B: int) -> torch.Tensor:
    """Rows of a state tensor as their int32 words [B, n], bit for bit."""
    return t.reshape(B, -1).contiguous().view(torch.int32)


@torch.no_grad()
def transfer_reference(state: SessionState, slots=None, blob_in=None, want_out: bool = True,
                       release: bool = False):
    """rb_session_transfer in plain torch ops, on the state's device (CPU
    included): ``(blob_out int32 [B, W] or None, status int32 [B])``; the
    status is also left in ``state.status``.  Blob contents and status are
    bit-identical to the kernel's.

    slots: int64 [B], unique (None: slot b); a slot outside [0, N) is masked,
    not refused: its outgoing row is all zeros, its status BAD_SLOT, and
    nothing of the state is touched.  want_out: build the outgoing blob from
    the slots' state as it stands before the call (the row format:
    session/recblr_session.h, ``SessionState.blob_layout``).  blob_in: rows to
    put into the slots; a row is applied as a whole (MOVED) when its word 0 is
    ``state.blob_tag``, its count >= 0 and every ring entry in [-1, V), and
    otherwise leaves the slot untouched (BAD_BLOB).  release (without blob_in):
    the slots are left as ``state.reset(slots)`` leaves them, with the h0 the
    state holds."""
    who = "transfer_reference"
    if blob_in is None and not want_out and not release:
        raise ValueError(f"{who}: nothing to do: give blob_in, want_out or release")
    if blob_in is not None and release:
        raise ValueError(f"{who}: release cannot be combined with an incoming blob")
    slots, blob_in, B = _transfer_rows(state, slots, blob_in, None, who, check_slots=False)
    dev, N, V, W = state.device, state.capacity, state.shape[0], state.blob_words
    if slots is None:
        slots = torch.arange(B, device=dev)
    slot_ok = ~_bad_slot(state, slots)
    safe = slots.clamp(0, N - 1)
    lay, tag = state.blob_layout(), state.blob_tag
    convs = [(i, c) for i, c in enumerate(state.conv) if c is not None]
    status = torch.full((B,), MOVED, device=dev, dtype=torch.int32)
    blob_out = None
    if want_out:
        head = torch.tensor([tag, 0], device=dev, dtype=torch.int32).expand(B, 2)
        parts = [head, _blob_words(state.count[safe], B), _blob_words(state.out[safe], B)]
        for i, h in enumerate(state.h):
            parts.append(_blob_words(h[safe], B))
            if state.conv[i] is not None:
                parts.append(_blob_words(state.conv[i][safe], B))
        if state.items is not None:
            parts.append(_blob_words(state.items[safe], B))
        used = sum(p.shape[1] for p in parts)
        parts.append(torch.zeros((B, W - used), device=dev, dtype=torch.int32))
        blob_out = torch.cat(parts, 1)
        blob_out[~slot_ok] = 0
    if blob_in is not None:
        def part(name, dtype):
            w0, n = lay[name]
            return blob_in[:, w0:w0 + n].contiguous().view(dtype)

        count_in = part("count", torch.int64)[:, 0]
        valid = slot_ok & (blob_in[:, 0] == tag) & (count_in >= 0)
        if state.items is not None:
            ring_in = part("items", torch.int64)
            valid &= ((ring_in >= -1) & (ring_in < V)).all(1)
        idx = slots[valid]
        state.count[idx] = count_in[valid]
        state.out[idx] = part("out", torch.float32)[valid]
        for i, h in enumerate(state.h):
            h[idx] = part(f"h{i}", torch.float32)[valid]
        for i, c in convs:
            c[idx] = part(f"conv{i}", torch.float32)[valid].reshape(-1, *c.shape[1:])
        if state.items is not None:
            state.items[idx] = ring_in[valid]
        status[slot_ok & ~valid] = BAD_BLOB
    elif release:
        idx = slots[slot_ok]
        for h, h0 in zip(state.h, state.h0):
            h[idx] = h0
        for _, c in convs:
            c[idx] = 0.0
        state.count[idx] = 0
        state.out[idx] = 0.0
        if state.items is not None:
            state.items[idx] = -1
    status[~slot_ok] = BAD_SLOT
    state.status = status
    return blob_out, status


def _transfer_layers(state: SessionState):
    """The rb_session_layer array rb_session_transfer reads: h, conv_state and
    h0 only (no weights), rebuilt only when a tensor has moved."""
    tensors = [dict(h0=h0, h=h, conv_state=c) for h0, h, c in zip(state.h0, state.h, state.conv)]
    key = tuple(t.data_ptr() if t is not None else 0 for row in tensors for t in row.values())
    if state._transfer_plan is not None and state._transfer_plan[0] == key:
        return state._transfer_plan[1]
    arr = (_Layer * len(tensors))()
    for dst, row in zip(arr, tensors):
        for f, t in row.items():
            setattr(dst, f, t.data_ptr() if t is not None else None)
    state._transfer_plan = (key, arr)
    return arr


def _transfer_kernel(state: SessionState, slots, blob_in, blob_out, status, release: bool) -> None:
    """The one launch (rb_session_transfer)."""
    V, d, H, K, n_layers, use_conv, _ = state.shape
    ptr = lambda t: t.data_ptr() if t is not None else None     # noqa: E731
    S = 0 if state.items is None else state.items.shape[1]
    _lib.call_session(
        "rb_session_transfer", ctypes.addressof(_transfer_layers(state)), n_layers,
        state.count.data_ptr(), state.out.data_ptr(), ptr(state.items), ptr(slots), ptr(blob_in),
        ptr(blob_out), status.data_ptr(), state.blob_tag, int(release), status.numel(),
        state.capacity, V, d, H, K, S, int(use_conv), state.blob_words,
        kernels._stream(state.out))


def _transfer(state: SessionState, slots, blob_in, want_out: bool, release: bool, out, who: str):
    """park / resume / exchange: (blob_out or None, status)."""
    slots, blob_in, B = _transfer_rows(state, slots, blob_in, out, who)
    _, d, H = state.shape[:3]
    if state.device.type != "cuda" or d % 4 or H % 4:
        blob_out, status = transfer_reference(state, slots, blob_in, want_out, release)
        if out is not None and blob_out is not None:
            blob_out = out.copy_(blob_out)
        return blob_out, status
    blob_out = None
    if want_out:
        blob_out = out if out is not None else torch.empty(
            (B, state.blob_words), device=state.device, dtype=torch.int32)
    status = torch.empty((B,), device=state.device, dtype=torch.int32)
    with torch.cuda.device(state.device):
        _transfer_kernel(state, slots, blob_in, blob_out, status, release)
    state.status = status
    return blob_out, status


@torch.no_grad()
def park(state: SessionState, slots=None, release: bool = False, out=None) -> torch.Tensor:
    """Take the slots' sessions out of the state: one launch writes each
    slot's whole state (count, out, per layer h and the conv history, the item
    ring) as a row of the returned int32 ``[B, W]`` blob (``W =
    state.blob_words``) on the state's device; ``blob.cpu()`` is the host copy
    a service stores.  slots None: every slot.  release=True also leaves the
    slots as ``state.reset(slots)`` does (free for the next session); otherwise
    the state is only read.  out: a buffer to write into (int32 [B, W],
    contiguous, on the state's device).

    The rows carry ``state.blob_tag``, which guards the model *shape* (and the
    window and ring length), not its weights: resuming a blob under a model
    of the same shape and other weights is the caller's error and goes
    undetected.  slots are ``step``'s: a list is checked; a device tensor costs
    no sync, must be unique, and a slot outside the state yields an all-zero
    row and BAD_SLOT in ``state.status`` (MOVED for the others).  A state on the
    CPU, or with d or H no multiple of 4, runs transfer_reference."""
    return _transfer(state, slots, None, True, release, out, "park")[0]


@torch.no_grad()
def resume(state: SessionState, blob, slots=None) -> torch.Tensor:
    """Put parked sessions back: row b of blob (int32 [B, W], on the state's
    device or the CPU, then copied over) replaces the whole state of slot
    slots[b] (None: slot b), which need not be the slot it was parked from.
    Returns the rows' statuses (also ``state.status``): MOVED, BAD_SLOT, or
    BAD_BLOB for a row that is not a parked session of this state's shape
    (another tag, e.g. the all-zero row of a bad park), has a negative count
    or a ring entry outside [-1, V); such a row leaves its slot untouched, the
    other rows of the call are applied.  One launch, no host sync."""
    if blob is None:
        raise ValueError("resume: blob must be an int32 tensor")
    return _transfer(state, slots, blob, False, False, None, "resume")[1]


@torch.no_grad()
def exchange(state: SessionState, blob, slots=None, out=None) -> torch.Tensor:
    """park and resume in one launch: the slots' present sessions go out (the
    returned blob, the state as it stood before the call), the rows of blob
    come in.  A refused incoming row (``state.status``: BAD_BLOB) still parks
    the slot's session and leaves it in place.  blob and out must not
    overlap."""
    if blob is None:
        raise ValueError("exchange: blob must be an int32 tensor")
    return _transfer(state, slots, blob, True, False, out, "exchange")[0]

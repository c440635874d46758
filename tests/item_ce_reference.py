"""A plain torch restatement of the item cross-entropy head (csrc/item_scores.hip:
rb_item_ce_fwd / _bwd / _probs, their f16-pipe forms _fwd_h / _probs_h / _h_t /
_h_both and the row-chunked _rows forms), and the comparison the tests judge
the kernels by.  No GPU, no product code.

    x      = seq @ table^T                                 [B, V]
    lse_b  = m_b + log(sum_v exp(x_bv - m_b)),  m_b = max_v x_bv
    loss_b = lse_b - x_b,target_b              (0 for an ignored row, target -1)
    loss   = inv_n * sum_b loss_b              (inv_n = 1 / live rows by default)
    P      = (exp(x - lse) - onehot(target)) * dloss * inv_n   (ignored rows exactly 0)
    dseq   = P @ table,   ditems = P^T @ seq

Run in float64 this is the reference; run in float32 (lse rounded to fp32
before P = exp(x - lse) - onehot is formed from it, which is how the kernels
form P) it is the yardstick e32: the error plain fp32 arithmetic makes on the
same inputs.  Nothing here shares the kernels' tiling, their split merge, their
exp2-based exponential or the f16 pipe's two-part operands.

The error measure and the bar are gate_scan_reference's (channel_error, judge,
bar, FLOOR); judge_all below says at which scale each tensor is judged.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

from gate_scan_reference import FLOOR, bar, channel_error, judge  # noqa: F401

TILE = 32           # kTile: rows (items or sequences) of one wave tile
WG_ROWS = 128       # kWaves * kTile: fixed rows of one workgroup
TARGET_WGS = 512    # kTargetWgs
TENSORS = ("lse", "loss_rows", "loss", "P", "dseq", "ditems")
REGIMES = ("random", "peaked", "large", "scaled", "ties")

# Regime "peaked": the margin (target logit minus the log-sum-exp of the other
# logits, in nats) is spread over the rows from PEAKED_MARGIN_MIN to
# PEAKED_MARGIN_MAX.  With a dominant target every entry of the row's P, and so
# the row of dseq, is of size 1 - p = e^-margin, while P = exp(x - lse) - onehot
# carries the rounding of lse (half an ulp at magnitude 8..32: up to 1e-6) in
# any fp32 arithmetic.  The worst e32 of the fp32 run of this reference over the
# listed peaked cases (ditems and dseq at 600 x 4100 x 128, where lse is
# largest: logits up to 23):
#     margins 2 .. 6   2.9e-4   (smallest row loss 2.5e-3)
#     margins 2 .. 5   1.3e-4   (6.7e-3)
#     margins 2 .. 4   5.1e-5   (1.8e-2)
# a property of fp32, so the regime stops where that yardstick is under 1e-4
# (test_item_ce_reference_host.py holds every case to it).
PEAKED_MARGIN_MIN = 2.0
PEAKED_MARGIN_MAX = 4.0

# Regime "scaled": every seq row times 2^k and every item row times 2^-k (the
# logits are unchanged, every exponent path of the split image moves); k by the
# case's seed.  One k per case: exponents that differ from row to row multiply
# into the logits themselves.
SCALED_K = (60, -60, 37, -23)


# ---- the launch plan (item_scores.hip: plan(), place()) ---------------------------
def plan(n_fixed: int, n_streamed: int):
    """(blocks, splits, per, tiles) of a row-stationary launch: `blocks`
    workgroups of 128 fixed rows, the streamed extent's `tiles` 32-row tiles
    dealt into `splits` runs of `per` tiles (the last may be shorter)."""
    blocks = -(-n_fixed // WG_ROWS)
    tiles = -(-n_streamed // TILE)
    s = max(1, min(-(-TARGET_WGS // blocks), tiles))
    per = -(-tiles // s)
    return blocks, -(-tiles // per), per, tiles


def plan_rows_fixed(B: int, V: int):
    """k_ce_fwd, k_ce_bwd_seq, k_item_scores<probs>, k_ce_fwd_h, k_ce_probs_h:
    the sequence rows fixed, the item table streamed."""
    return plan(B, V)


def plan_items_fixed(B: int, V: int):
    """k_ce_bwd_item: the item rows fixed, the sequence rows streamed."""
    return plan(V, B)


def last_split_tiles(p) -> int:
    blocks, splits, per, tiles = p
    return tiles - (splits - 1) * per


def idle_last_wave(n_fixed: int) -> bool:
    """The last workgroup's last wave starts at or past the end of the fixed rows."""
    return ((n_fixed - 1) // TILE) % 4 != 3


# ---- inputs ------------------------------------------------------------------------
def place_targets(B, V, g, ignored=()):
    """int64 [B] targets: random, then on purpose in part of the rows item 0,
    item V - 1, the last item of the first 32-item tile and the first of the
    second, the first and the last item of the (ragged) last tile, one target
    shared by a run of rows in the middle; the item `untargeted` (V // 2, V >=
    3) is the target of no row.  Rows in `ignored` get -1.  Returns (target,
    untargeted | None)."""
    tgt = torch.randint(0, V, (B,), generator=g)
    un = V // 2 if V >= 3 else None
    special = [v for v in (0, V - 1, 31, 32, (V - 1) // TILE * TILE, V - 1, 63, 64)
               if 0 <= v < V and v != un]
    for i, v in enumerate(special):          # the first rows, and the last (a ragged batch tile)
        if i < B:
            tgt[i] = v
        if B - 1 - i >= len(special):
            tgt[B - 1 - i] = v
    if B >= 8:                               # one target in many rows
        run = min(max(B // 4, 2), 40)
        tgt[B // 2:B // 2 + run] = special[min(4, len(special) - 1)]
    if un is not None:
        tgt[tgt == un] = (un + 1) % V
    tgt[list(ignored)] = -1
    return tgt, un


def make_inputs(regime, B, V, d, seed, ignored=()):
    """fp32 seq [B, d], table [V, d] and int64 target [B] of one case, on the CPU.

    "random": 0.5 * randn, the scale the existing parity tests use.
    "peaked": random, then each row moved along its target's item row until
    the target leads the other items' log-sum-exp by the row's margin
    (PEAKED_MARGIN_MIN .. _MAX over the rows; 8 fixed-point steps, as the move
    shifts the other logits too): the state of a trained model.
    "large": a shared direction u carries a_b u in the seq rows (|a_b| in 3 ..
    10, sign alternating) and +-10 u in the item rows, on top of 0.5 * randn:
    logits up to +-100 and beyond, both signs in every row, every item led by
    half the rows.
    "scaled": random, seq rows times 2^k and item rows times 2^-k (k =
    SCALED_K[seed % 4]), one all-zero seq row (B // 3) and one all-zero item
    row (V // 3) where there are three.
    "ties": random with several item rows bit-equal (items 2, 31, 32, V - 1
    where they exist), some of them targets (place_targets)."""
    g = torch.Generator().manual_seed(seed * 7919 + B * 7 + V * 3 + d)
    seq = 0.5 * torch.randn(B, d, generator=g)
    table = 0.5 * torch.randn(V, d, generator=g)
    tgt, un = place_targets(B, V, g, ignored)
    info = {}
    if regime == "random":
        pass
    elif regime == "peaked":
        if V >= 2:
            s, w = seq.double(), table.double()
            live = tgt >= 0
            t = tgt.clamp_min(0)
            wt = w[t]
            margin = torch.linspace(PEAKED_MARGIN_MIN, PEAKED_MARGIN_MAX, B)[torch.randperm(B, generator=g)]
            for _ in range(8):      # the move shifts the other logits too: repeat until the margin holds
                x = s @ w.t()
                xt = x.gather(1, t[:, None])[:, 0]
                others = x.scatter(1, t[:, None], -math.inf).logsumexp(1)
                step = (margin.double() + others - xt) / (wt * wt).sum(1)
                s = torch.where(live[:, None], s + step[:, None] * wt, s)
            seq = s.float()
    elif regime == "large":
        u = torch.randn(d, generator=g)
        u = u / u.norm()
        a = (3.0 + 7.0 * torch.rand(B, generator=g)) * torch.where(torch.arange(B) % 2 == 0, 1.0, -1.0)
        if B:
            a[0] = 10.0
        b = 10.0 * torch.where((torch.arange(V) // 3) % 2 == 0, 1.0, -1.0)
        seq = seq + a[:, None] * u
        table = table + b[:, None] * u
    elif regime == "scaled":
        k = SCALED_K[seed % len(SCALED_K)]
        if B >= 3:
            seq[B // 3] = 0.0
        if V >= 3:
            table[V // 3] = 0.0
        seq = torch.ldexp(seq, torch.tensor(k))
        table = torch.ldexp(table, torch.tensor(-k))
        info["k"] = k
    elif regime == "ties":
        same = sorted({v for v in (2, 31, 32, V - 1) if 0 <= v < V})
        table[same] = table[same[0]].clone()
        info["tied"] = same
    else:
        raise ValueError(regime)
    return SimpleNamespace(seq=seq.contiguous(), table=table.contiguous(), target=tgt,
                           untargeted=un, ignored=tuple(ignored), **info)


# ---- the operation -----------------------------------------------------------------
def logits(seq, table, dtype):
    return seq.detach().to(dtype) @ table.detach().to(dtype).t()


def log_sum_exp(x):
    """Per row, in x's dtype (and so rounded to it)."""
    m = x.max(1, keepdim=True).values
    return (m + torch.log(torch.exp(x - m).sum(1, keepdim=True)))[:, 0]


def one_hot(target, V, dtype):
    oh = torch.zeros(target.numel(), V, dtype=dtype)
    live = target >= 0
    oh[live.nonzero()[:, 0], target[live]] = 1.0
    return oh


def finish(seq, table, target, x, lse, dloss=1.0, inv_n=None, onehot=None):
    """Everything after the log-sum-exp, in x's dtype, from the logits x, the
    per-row lse (already rounded to the dtype) and the one-hot matrix."""
    dtype = x.dtype
    B, V = x.shape
    s, w = seq.detach().to(dtype), table.detach().to(dtype)
    live = target >= 0
    if inv_n is None:
        inv_n = 1.0 / max(int(live.sum()), 1)
    if onehot is None:
        onehot = one_hot(target, V, dtype)
    zero = torch.zeros((), dtype=dtype)
    xt = x.gather(1, target.clamp_min(0)[:, None])[:, 0]
    loss_rows = torch.where(live, lse - xt, zero)
    g = torch.tensor(float(dloss) * float(inv_n), dtype=dtype)
    P = torch.where(live[:, None], (torch.exp(x - lse[:, None]) - onehot) * g, zero)
    aP, asq, aw = P.abs(), s.abs(), w.abs()
    return SimpleNamespace(
        x=x, lse=lse, loss_rows=loss_rows, loss=loss_rows.sum() * inv_n, P=P,
        dseq=P @ w, ditems=P.t() @ s, inv_n=float(inv_n), g=abs(float(dloss) * float(inv_n)),
        # what the sums add up, in magnitude: the scales they are judged at
        dseq_scale=aP @ aw, ditems_scale=aP.t() @ asq, logit_scale=(asq @ aw.t()).amax(1))


def reference(seq, table, target, dloss=1.0, inv_n=None, dtype=torch.float64):
    """seq [B, d], table [V, d], target [B] int64 in [0, V) or -1 (an ignored
    row), the scalar upstream gradient dloss, inv_n (default 1 / live rows).
    Returns lse, loss_rows [B], loss, P [B, V], dseq [B, d], ditems [V, d] and
    the summand scales dseq_scale [B, d] = |P| |table|, ditems_scale [V, d] =
    |P|^T |seq|, logit_scale [B] = max_v sum_k |seq_bk table_vk|."""
    x = logits(seq, table, dtype)
    return finish(seq, table, target, x, log_sum_exp(x), dloss, inv_n)


def both(inp, dloss=1.0, inv_n=None):
    """(fp64 reference, fp32 yardstick run) of one make_inputs case."""
    return (reference(inp.seq, inp.table, inp.target, dloss, inv_n, torch.float64),
            reference(inp.seq, inp.table, inp.target, dloss, inv_n, torch.float32))


# ---- the comparison ----------------------------------------------------------------
def row_scale(r64):
    """The scale lse and loss_rows are judged at, per row: the logit summand
    scale max_v sum_k |seq_bk table_vk| or, where that is smaller (an all-zero
    seq row: lse = log V whatever the table holds), |lse| itself, whose own
    rounding no arithmetic avoids."""
    return torch.maximum(r64.logit_scale, r64.lse.abs())


def judge_all(got, r64, r32, M, names=None):
    """judge() for each tensor of `got` (a dict) against the two reference
    runs: {name: (passes, error, bar, ratio)}.  M: one number or {name: number}.

    The last axis is channel_error's "channel", so tensors go in transposed
    where rows are the unit:
      lse, loss_rows [B]  per row, at row_scale();
      P [B, V]            per row, at |dloss * inv_n|: in probability units;
      dseq [B, d]         per sequence row, at max_k sum_v |P_bv table_vk|;
      ditems [V, d]       per item row, at max_k sum_b |P_bv seq_bk|; an item
                          that no live row gives weight to (scale 0) must equal
                          the reference exactly;
      loss                as the sum of inv_n * loss_rows, on sum |summands|."""
    out = {}
    for n in (names or got.keys()):
        t = got[n]
        m = M[n] if isinstance(M, dict) else M
        ref, r3 = getattr(r64, n), getattr(r32, n)
        if n in ("lse", "loss_rows"):
            out[n] = judge(t.reshape(1, -1), ref[None, :], r3[None, :], m, scale=row_scale(r64)[None, :])
        elif n == "P":
            B = ref.shape[0]
            out[n] = judge(t.t(), ref.t(), r3.t(), m, scale=torch.full((1, B), r64.g, dtype=torch.float64))
        elif n == "dseq":
            out[n] = judge(t.t(), ref.t(), r3.t(), m, scale=r64.dseq_scale.amax(1)[None, :])
        elif n == "ditems":
            out[n] = judge(t.t(), ref.t(), r3.t(), m, scale=r64.ditems_scale.amax(1)[None, :])
        elif n == "loss":
            out[n] = judge(t.reshape(1), ref.reshape(1), r3.reshape(1), m,
                           scale=(r64.loss_rows * r64.inv_n)[:, None],
                           scale32=(r32.loss_rows * r32.inv_n)[:, None])
        else:
            raise KeyError(n)
    return out


def e32_all(r64, r32):
    """{name: e32}: the yardstick run judged as a kernel would be."""
    got = {n: getattr(r32, n) for n in TENSORS}
    out = {n: res[1] for n, res in judge_all(got, r64, r32, 0.0).items()}
    # the loss' yardstick is the larger of the sum's and its summands' (judge)
    out["loss"] = max(out["loss"], channel_error((r32.loss_rows * r32.inv_n)[:, None],
                                                 (r64.loss_rows * r64.inv_n)[:, None]))
    return out


# ---- the cases the GPU tests run ---------------------------------------------------
# (B, V): the tiny ones, then one per loop geometry (plan(); forward / bwd_item
# as blocks x splits x per [tiles], last split):
#   (600, 4100)   5 x 65 x 2 [129], last 1      33 x 10 x 2 [19], last 1
#   (1100, 5000)  9 x 53 x 3 [157], last 1      40 x 12 x 3 [35], last 2
#   (2049, 3900)  17 x 31 x 4 [122], last 2     31 x 17 x 4 [65], last 1
#   (2049, 4003)  17 x 26 x 5 [126], last 1     32 x 13 x 5 [65], last 5
TINY_SHAPES = ((1, 1), (5, 7), (33, 64), (130, 97))
GEOMETRY_SHAPES = ((600, 4100), (1100, 5000), (2049, 3900), (2049, 4003))


def _cases():
    out = []
    for B, V in TINY_SHAPES + GEOMETRY_SHAPES:      # d = 128 and 64 on every shape
        for d in (128, 64):
            out.append(("random", B, V, d))
    for d in (16, 32, 256):                         # every d on a ragged case
        out.append(("random", 130, 97, d))
    out += [("random", 5, 7, 16), ("random", 33, 64, 32), ("random", 5, 7, 256)]
    out += [("peaked", 130, 97, 128), ("peaked", 130, 97, 64), ("peaked", 33, 64, 64),
            ("peaked", 600, 4100, 128)]
    out += [("large", 130, 97, 128), ("large", 33, 64, 64), ("large", 1100, 5000, 64)]
    out += [("scaled", 130, 97, 128), ("scaled", 130, 97, 64), ("scaled", 33, 64, 32),
            ("scaled", 600, 4100, 128)]
    out += [("ties", 130, 97, 128), ("ties", 33, 64, 64), ("ties", 5, 7, 16)]
    return tuple(out)


CASES = _cases()                                    # (regime, B, V, d)
# the autograd paths: one shape meeting scoring._f16_grads_ok (B % 256 == 0, d
# = 128) and shapes that do not
AUTOGRAD_CASES = (("random", 256, 515, 128), ("random", 130, 97, 128), ("random", 130, 97, 64),
                  ("peaked", 600, 4100, 128))
# the rows forms: M rows in chunks, V = 97 (ragged) and 4100 (per = 2, a short
# last split)
ROWS_CASES = (("random", 600, 97, 128), ("random", 600, 97, 64), ("peaked", 600, 97, 128),
              ("random", 600, 4100, 128), ("random", 600, 4100, 64))
ROWS_IGNORED = (0, 31, 32) + tuple(range(64, 96)) + tuple(range(256, 456)) + (599,)


def case_id(c):
    return "%s-%dx%dx%d" % c


ALL_CASES = CASES + AUTOGRAD_CASES + ROWS_CASES


def case_seed(c):
    """One seed per case (its first place in ALL_CASES); for "scaled" it also
    picks k (SCALED_K), so the four scaled cases take the four exponents."""
    return ALL_CASES.index(c)


def case_inputs(c, ignored=()):
    regime, B, V, d = c
    return make_inputs(regime, B, V, d, case_seed(c), ignored)

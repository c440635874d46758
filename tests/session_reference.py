"""A plain torch restatement of the stateful session encoder (session/*.hip:
rb_session_step / _append / _capture; session.py), event by event, and the
parameter regimes the tests run it in.  No GPU, no product code.

Per slot the encoder is a serial loop over that slot's events.  Per layer it
carries the last K - 1 pre-conv rows (oldest first) and the recurrent state h:

    x       = LN(emb[item])
    u | z   = W_in x
    xc      = silu(conv_b + sum_j conv_w[:, j] * window[j]),  window = [rows, u]
    r | i   = W_g xc + b_g
    alpha   = exp(-softplus(Lambda) * sigmoid(r))
    beta    = sqrt(1 - alpha^2 + 1e-8) * sigmoid(i)
    h       = alpha * h + beta * xc
    x       = LN(W_out (silu(z) * h) + x)
    x       = LN(W_2 silu(W_1 x + b_1) + b_2 + x)             (unless disable_ffn)

The state of an empty history is what the reference model's zero-padded causal
conv and scan leave after the P = pow2(L) - L pad positions of a window L: P
explicit steps with u = 0 (rows of zeros enter the conv window, xc =
silu(conv_b), h advances), not a closed form.  Without the conv xc = u = 0
there and h stays 0.  The K - 1 rows are zeros afterwards either way.  Events
may run past L: the loop just continues.

Everything is computed in `dtype`: float64 for the reference, float32 for the
yardstick e32 (what plain fp32 arithmetic makes of the same inputs).  The
LayerNorm is written out (two-pass variance) so that nothing here depends on a
library kernel's choice of algorithm.

`wrong` plants one subtle error (WRONG) into the run: the host test uses them
to show that the bar the GPU tests apply rejects each.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from gate_scan_reference import FLOOR, WIDE_LAMBDA_MIN, bar, channel_error, judge  # noqa: F401

LN_EPS = 1e-12
WRONG = ("gate_fp16", "ln_eps", "no_beta_eps", "conv_shift", "one_pass_var", "zero_h0")
# "wide": the channel whose r gate is shut for good (gates.bias = STUCK_BIAS):
# alpha = 1 in any arithmetic and beta = sqrt(1e-8) sigmoid(i), the one place
# where the 1e-8 under the root is more than an fp32 rounding of 1 - alpha^2
STUCK_CHANNEL, STUCK_BIAS = 3, -40.0
SHIFTED_EVERY = 7      # "wide": embedding rows 0, 7, 14, ... are shifted by +300


def pow2_pad_len(L: int) -> int:
    return (1 << (L - 1).bit_length()) - L


def _flags(cfg):
    only = bool(cfg.get("bd_lru_only", False))
    return (not (only or cfg.get("disable_conv1d", False)),
            not (only or cfg.get("disable_ffn", False)))


def make_params(regime, d, expand, K, layers, V, seed):
    """fp32 parameters under RecBLR's names, on the CPU.

    "init": the model's initialisation moved off its zeros and ones the way
    tests/test_gpu_session.py::_model does: Linear and embedding weights
    3 * N(0, 0.02), biases and LayerNorm parameters + 0.1 N(0, 1), the conv
    PyTorch's default U(-1/sqrt(K), 1/sqrt(K)), Lambda over the initial range
    (exp(-softplus(Lambda)) from 0.9 to 0.999).
    "wide": gate weights and bias scaled until r and i saturate
    (|pre-activation| up to about 8), Lambda from WIDE_LAMBDA_MIN to 25 with
    one channel at exactly 20.0 and one at the next float above it (the two
    sides of softplus' x > 20 branch), every 7th embedding row shifted by +300
    (mean far above spread: the LayerNorm's variance), LayerNorm gammas in
    [0.5, 1.5], and one channel per layer with its r gate shut (STUCK_CHANNEL)."""
    if regime not in ("init", "wide"):
        raise ValueError(regime)
    wide = regime == "wide"
    g = torch.Generator().manual_seed(seed)
    H = d * expand

    def n(*shape, std=1.0):
        return std * torch.randn(*shape, generator=g)

    def u(*shape, lo, hi):
        return lo + (hi - lo) * torch.rand(*shape, generator=g)

    p = {}

    def ln(prefix):
        p[prefix + "weight"] = u(d, lo=0.5, hi=1.5) if wide else 1.0 + n(d, std=0.1)
        p[prefix + "bias"] = n(d, std=0.1)

    p["item_embedding.weight"] = n(V, d, std=0.06)
    if wide:
        p["item_embedding.weight"][::SHIFTED_EVERY] += 300.0
    ln("layer_norm.")
    bound = 1.0 / math.sqrt(K)
    for i in range(layers):
        pre = f"recurrent_layers.{i}."
        bm = pre + "behavior_modeling."
        p[bm + "input.weight"] = n(2 * H, d, std=0.06)
        p[bm + "conv1d.weight"] = u(H, 1, K, lo=-bound, hi=bound)
        p[bm + "conv1d.bias"] = u(H, lo=-bound, hi=bound) + n(H, std=0.1)
        if wide:
            p[bm + "gates.weight"] = n(2 * H, H, std=8.0 / math.sqrt(H))
            p[bm + "gates.bias"] = n(2 * H, std=2.0)
            p[bm + "gates.bias"][STUCK_CHANNEL] = STUCK_BIAS
            lam = torch.linspace(WIDE_LAMBDA_MIN, 25, H)
            lam[1] = 20.0
            lam[H - 2] = torch.nextafter(torch.tensor(20.0), torch.tensor(math.inf))
        else:
            p[bm + "gates.weight"] = n(2 * H, H, std=0.06)
            p[bm + "gates.bias"] = n(2 * H, std=0.1)
            lam = torch.linspace(math.log(math.expm1(-math.log(0.9))),
                                 math.log(math.expm1(-math.log(0.999))), H)
        p[bm + "Lambda"] = lam
        p[bm + "output.weight"] = n(d, H, std=0.06)
        ln(pre + "layer_norm.")
        p[pre + "ffn.w_1.weight"] = n(4 * d, d, std=0.06)
        p[pre + "ffn.w_1.bias"] = n(4 * d, std=0.1)
        p[pre + "ffn.w_2.weight"] = n(d, 4 * d, std=0.06)
        p[pre + "ffn.w_2.bias"] = n(d, std=0.1)
        ln(pre + "ffn.layer_norm.")
    return p


def config(d, expand, K, layers, L, **flags):
    """The model configuration that goes with make_params' shapes."""
    cfg = dict(hidden_size=d, loss_type="CE", num_layers=layers, dropout_prob=0.0, expand=expand,
               d_conv=K, bd_lru_only=False, disable_conv1d=False, disable_ffn=False,
               MAX_ITEM_LIST_LENGTH=L)
    cfg.update(flags)
    return cfg


def takes_shifted(b: int) -> bool:
    """Whether slot b's events may name a shifted embedding row (every third
    slot does).  The other slots never see one, so that the fp32 yardstick of
    their tensors is not the shifted rows' (a LayerNorm of 300 +- 0.06 in fp32
    is 1e-4 off, 300 times what it is on the other rows): judge_run judges the
    two kinds of slot separately in "wide"."""
    return b % 3 == 2


def make_events(counts, V, seed):
    """Per slot a list of counts[b] item ids of [1, V).  A slot that takes
    shifted rows (takes_shifted) has one at every other event, its first
    included; the other slots have none."""
    g = torch.Generator().manual_seed(seed)
    plain = [i for i in range(1, V) if i % SHIFTED_EVERY]
    shifted = list(range(SHIFTED_EVERY, V, SHIFTED_EVERY))
    out = []
    for b, c in enumerate(counts):
        ids = [plain[j] for j in torch.randint(0, len(plain), (int(c),), generator=g).tolist()]
        other = torch.randint(0, len(shifted), (int(c),), generator=g).tolist()
        if takes_shifted(b):
            ids[::2] = [shifted[j] for j in other[::2]]
        out.append(ids)
    return out


def reference(params, cfg, L, events, dtype=torch.float64, wrong=None):
    """params: RecBLR's parameter names -> tensors; cfg: num_layers and the
    flags disable_conv1d / disable_ffn / bd_lru_only (expand is in the shapes);
    L: the session window; events: per slot a list of item ids in [1, V).

    Returns, per slot b with n_b events: out[b] [n_b, d], h[i][b] [n_b, H],
    conv[i][b] [n_b, K - 1, H] (conv[i] None without a conv history: K = 1 or
    no conv) — the state after each event; h0[i] [H], the state of the empty
    history; gate_max, the largest |r| or |i| pre-activation at a real event
    outside the stuck channel."""
    assert wrong is None or wrong in WRONG, wrong
    use_conv, use_ffn = _flags(cfg)
    layers = cfg["num_layers"]
    p = {k: v.detach().to(dtype) for k, v in params.items()}
    if wrong == "gate_fp16":
        for k in p:
            if k.endswith("gates.weight"):
                p[k] = p[k].half().to(dtype)
    eps = 1e-5 if wrong == "ln_eps" else LN_EPS
    beta_eps = 0.0 if wrong == "no_beta_eps" else 1e-8
    shift = 1 if wrong == "conv_shift" else 0

    def ln(prefix, x):
        mean = x.mean()
        if wrong == "one_pass_var":
            var = (x * x).mean() - mean * mean
        else:
            var = ((x - mean) ** 2).mean()
        return (x - mean) / torch.sqrt(var + eps) * p[prefix + "weight"] + p[prefix + "bias"]

    def name(i, s):
        return f"recurrent_layers.{i}.behavior_modeling.{s}"

    H = p[name(0, "Lambda")].shape[0]
    K = p[name(0, "conv1d.weight")].shape[-1]
    keep = K - 1 if use_conv else 0            # rows of conv history
    gate_max = 0.0

    def recur(i, rows, h, u_row, real):
        """One position of layer i's recurrent block: (rows, h) -> (rows, h)."""
        nonlocal gate_max
        if use_conv:
            rows = torch.cat([rows, u_row[None]])          # K + shift rows, oldest first
            w = p[name(i, "conv1d.weight")].reshape(H, K)
            xc = F.silu(p[name(i, "conv1d.bias")] + (rows[:K] * w.t()).sum(0))
            rows = rows[1:]
        else:
            xc = u_row
        rg = p[name(i, "gates.weight")] @ xc + p[name(i, "gates.bias")]
        if real:
            gate_max = max(gate_max, float(rg[p[name(i, "gates.bias")] != STUCK_BIAS].abs().max()))
        alpha = torch.exp(-F.softplus(p[name(i, "Lambda")]) * torch.sigmoid(rg[:H]))
        beta = torch.sqrt(1 - alpha * alpha + beta_eps) * torch.sigmoid(rg[H:])
        return rows, alpha * h + beta * xc

    # the empty history: P pad positions with u = 0, per layer
    P = 0 if wrong == "zero_h0" else pow2_pad_len(L)
    zero = torch.zeros(H, dtype=dtype)
    start = []
    for i in range(layers):
        rows, h = torch.zeros(keep + shift, H, dtype=dtype), zero
        for _ in range(P):
            rows, h = recur(i, rows, h, zero, False)
        start.append((rows, h))

    out, hs, convs = [], [[] for _ in range(layers)], [[] for _ in range(layers)]
    d = p["item_embedding.weight"].shape[1]
    for ev in events:
        state = list(start)
        o, hh, cc = [], [[] for _ in range(layers)], [[] for _ in range(layers)]
        for item in ev:
            x = ln("layer_norm.", p["item_embedding.weight"][item])
            for i in range(layers):
                xz = p[name(i, "input.weight")] @ x
                rows, h = recur(i, *state[i], xz[:H], True)
                state[i] = (rows, h)
                hh[i].append(h)
                cc[i].append(rows[shift:])
                pre = f"recurrent_layers.{i}."
                x = ln(pre + "layer_norm.", p[name(i, "output.weight")] @ (F.silu(xz[H:]) * h) + x)
                if use_ffn:
                    f = F.silu(p[pre + "ffn.w_1.weight"] @ x + p[pre + "ffn.w_1.bias"])
                    x = ln(pre + "ffn.layer_norm.",
                           p[pre + "ffn.w_2.weight"] @ f + p[pre + "ffn.w_2.bias"] + x)
            o.append(x)
        out.append(torch.stack(o) if o else torch.zeros(0, d, dtype=dtype))
        for i in range(layers):
            hs[i].append(torch.stack(hh[i]) if ev else torch.zeros(0, H, dtype=dtype))
            convs[i].append(torch.stack(cc[i]) if ev else torch.zeros(0, keep, H, dtype=dtype))
    return SimpleNamespace(out=out, h=hs, conv=convs if keep else [None] * layers,
                           h0=[s[1] for s in start], gate_max=gate_max)


# ---- the comparison ----------------------------------------------------------

def row_error_args(t):
    """[rows, C] (or [rows, K - 1, C]) turned so that gate_scan_reference's
    channel_error, which scales by the last axis, scales each row by its own
    max |ref|."""
    return t.reshape(-1, t.shape[-1]).t()


def tensor_names(ref):
    names = ["out"]
    for i in range(len(ref.h)):
        names.append(f"h[{i}]")
        if ref.conv[i] is not None:
            names.append(f"conv[{i}]")
    return names


def flat(run, name, slots=None, upto=None):
    """Tensor `name` ("out", "h[i]", "conv[i]") of a run (reference()'s result,
    or anything with the same per-slot lists) over the slots' events (all
    slots by default), one after the other: [sum n_b, ...].  upto: per slot the
    number of events to take."""
    if name == "out":
        per_slot = run.out
    else:
        per_slot = getattr(run, name[:name.index("[")])[int(name[name.index("[") + 1:-1])]
    if upto is not None:
        per_slot = [t[:n] for t, n in zip(per_slot, upto)]
    if slots is not None:
        per_slot = [per_slot[b] for b in slots]
    return torch.cat([t.double() for t in per_slot])


def multiplier(name, regime, M_init, M_wide):
    """M of a tensor: M_init in "init" and for layer 0's conv rows (a GEMM and
    LayerNorms only, in either regime), M_wide for h and what follows it."""
    return M_init if regime == "init" or name == "conv[0]" else M_wide


def judge_run(got, r64, r32, regime, M_init, M_wide, upto=None, names=None):
    """judge() for every state tensor of `got` against the two reference runs:
    {name: (passes, error, bar, ratio)}.  h per channel, out and conv per row.
    In "wide" the slots that take shifted embedding rows and the others are
    judged apart, each kind against its own yardstick ("out", "out+300")."""
    B = len(r64.out)
    kinds = {"": list(range(B))}
    if regime == "wide":
        kinds = {"": [b for b in range(B) if not takes_shifted(b)],
                 "+300": [b for b in range(B) if takes_shifted(b)]}
    res = {}
    for n in names or tensor_names(r64):
        for kind, slots in kinds.items():
            g, a, b = (flat(run, n, slots, upto) for run in (got, r64, r32))
            if a.shape[0] == 0:
                continue
            if not n.startswith("h"):
                g, a, b = row_error_args(g), row_error_args(a), row_error_args(b)
            res[n + kind] = judge(g, a, b, multiplier(n, regime, M_init, M_wide))
    return res

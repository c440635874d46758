"""A plain torch restatement of the conv + SiLU kernels (csrc/conv_silu.hip:
rb_conv_silu_fwd, _fwd_rows, _bwd and their _bf16 forms), with autograd, and
the comparison the tests judge them by.  No GPU, no product code.

    acc[t, c] = bias[c] + sum_k w[c, k] * x[t - (K-1) + k, c]     (x = 0 before t = 0)
    xc        = silu(acc)

The K taps are K shifted multiply-adds in an explicit loop; the gradients come
from autograd on sum(xc * (g1 + g2)).  Nothing here shares the kernels' tiles,
halo rows, look-ahead shuffles or hardware exp2 / rcp.  Run it in float64 for
the reference and in float32 for the yardstick e32.

Every sequence stands alone (`lengths`): rows past its end do not exist, they
get xc = 0 and no gradient whatever x and g hold there.

The error measure, the bar and the bf16 allowance are gate_scan_reference's.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch
import torch.nn.functional as F

from gate_scan_reference import FLOOR, bar, bf16_ulp, channel_error, judge  # noqa: F401

TENSORS = ("xc", "dx", "dw", "db")
BF16_ROUNDED = ("xc", "dx")          # stored in bf16 by the _bf16 kernels; dw and db stay fp32
SILU_ZERO_SLOPE = -1.2784645         # silu'(x) = 0 here

WIDE_X = 12.0                        # x scale of regime "wide"


def make_inputs(regime, B, L, H, K, seed, g2=True):
    """fp32 operands of one case, on the CPU: x, g1, g2 [B, L, H], w [H, K], bias [H].

    "init": randn x, 0.5 * randn weights and bias.
    "wide": x scaled by 12, so the pre-activations (std 6 sqrt(K)) run past
    +-30 and SiLU saturates on both sides; channel 0 has bias +20, channel 1
    bias -20, and channel 2 bias -1.278 with weights scaled by 0.01, which
    keeps its pre-activation within about +-0.3 of the zero of silu'."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, H, generator=g)
    w = 0.5 * torch.randn(H, K, generator=g)
    bias = 0.5 * torch.randn(H, generator=g)
    g1 = torch.randn(B, L, H, generator=g)
    g2_ = torch.randn(B, L, H, generator=g)
    if regime == "wide":
        x = WIDE_X * x
        bias[0] = 20.0
        if H > 1:
            bias[1] = -20.0
        if H > 2:
            bias[2] = SILU_ZERO_SLOPE
            w[2] = 0.01 * w[2]
    elif regime != "init":
        raise ValueError(regime)
    return SimpleNamespace(x=x, w=w, bias=bias, g1=g1, g2=g2_ if g2 else None)


def reference(x, w, bias, g1, g2=None, lengths=None, dtype=torch.float64):
    """x, g1, g2 [B, L, H], w [H, K], bias [H], lengths None | B ints in 1..L.

    Returns xc, dx [B, L, H] (zero past a sequence's end), dw [H, K], db [H]
    and terms: the summands of dw [B, L, H, K] and of db [B, L, H]."""
    B, L, H = x.shape
    K = w.shape[1]
    assert w.shape == (H, K) and bias.shape == (H,) and g1.shape == x.shape
    lens = torch.full((B,), L) if lengths is None else torch.as_tensor(lengths)
    assert lens.shape == (B,) and int(lens.min()) >= 1 and int(lens.max()) <= L

    def leaf(t):
        return t.detach().to(dtype).clone().requires_grad_()

    x_ = leaf(x)
    w_ = leaf(w.expand(B, L, H, K))          # one leaf per row: dw's summands
    b_ = leaf(bias.expand(B, L, H))
    g = g1.detach().to(dtype)
    if g2 is not None:
        g = g + g2.detach().to(dtype)
    valid = (torch.arange(L)[None, :] < lens[:, None]).unsqueeze(2)

    xp = torch.cat([torch.zeros(B, K - 1, H, dtype=dtype), x_], 1)    # K-1 rows of zero history
    acc = b_
    for k in range(K):
        acc = acc + w_[..., k] * xp[:, k:k + L]
    xc = torch.where(valid, F.silu(acc), torch.zeros((), dtype=dtype))
    (xc * g).sum().backward()
    return SimpleNamespace(
        xc=xc.detach(), dx=x_.grad, dw=w_.grad.sum((0, 1)), db=b_.grad.sum((0, 1)), lengths=lens,
        terms=dict(dw=w_.grad, db=b_.grad))


def judge_all(got, r64, r32, M, bf16=False, names=TENSORS):
    """judge() for each named tensor of `got` (attributes or keys): {name:
    (passes, error, bar, ratio)}.  dw and db are sums over rows: they are
    judged on the sum of their summands' magnitudes, one channel per (c, k)."""
    out = {}
    for n in names:
        t = got[n] if isinstance(got, dict) else getattr(got, n)
        ref, r3 = getattr(r64, n), getattr(r32, n)
        m = M[n] if isinstance(M, dict) else M
        if n in ("dw", "db"):
            C = ref.numel()
            out[n] = judge(t.reshape(C), ref.reshape(C), r3.reshape(C), m, False,
                           r64.terms[n].reshape(-1, C), r32.terms[n].reshape(-1, C))
        else:
            out[n] = judge(t, ref, r3, m, bf16 and n in BF16_ROUNDED)
    return out

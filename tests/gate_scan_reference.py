"""A plain torch restatement of the gate-scan kernels (csrc/gate_scan.hip:
rb_gate_scan_fwd / _bwd, their _bf16 and _last forms), with autograd, and the
comparison the tests judge the kernels by.  No GPU, no product code.

    alpha_t = exp(-softplus(Lambda) * sigmoid(r_t + b_r))
    beta_t  = sqrt(1 - alpha_t^2 + 1e-8) * sigmoid(i_t + b_i)
    h_t     = alpha_t * h_{t-1} + beta_t * xc_t          (h_{-1} = h0)
    y_t     = silu(z_t) * h_t

The recurrence is a serial loop over t and the gradients come from autograd on
sum(y * dy): nothing here shares the kernels' chunked scan, their adjoint
derivation or their hardware approximations.  Run it in float64 for the
reference and in float32 for the yardstick e32, the error that plain fp32
arithmetic makes on the same inputs.

Sequences shorter than L (`lengths`) stop at their own end: positions past it
get y = 0 and no gradient, whatever the operands hold there.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

TILE = 16                      # RB_TILE: the kernels checkpoint h every 16 steps
FLOOR = 4 * 2.0 ** -24         # four fp32 half-ulps: the bar where e32 is almost nothing
TENSORS = ("y", "drg", "dxc", "dz", "dlam", "dgate_b", "dh0")
BF16_ROUNDED = ("y", "y_last", "drg", "dxc", "dz")   # stored in bf16 by the _bf16 kernels


# Most negative Lambda of regime "wide".  With saturated r gates alpha comes
# within a few ulp of 1 and 1 - alpha^2 cancels, in any arithmetic: from -7 the
# fp32 run of this reference is itself 1.1e-3 off in drg (B=5, L=37, H=24, seed
# 3; 1.1e-4 from -4, 4.9e-5 from -3.5), a property of the formula, so the
# regime starts where that yardstick is under 1e-4.  "init" covers [-6.9, -2.2]
# with unsaturated gates.
WIDE_LAMBDA_MIN = -3.5


def make_inputs(regime, B, L, H, seed, h0=None, gate_b=True):
    """fp32 operands of one case, on the CPU.

    "init": everything randn, Lambda over the initial range [-6.9, -2.2]: the
    gates near sigmoid(0), alpha close to 1 (the long-memory end).
    "wide": rg and z scaled by 4 (saturated sigmoids), Lambda from
    WIDE_LAMBDA_MIN to 25 with one channel at exactly 20.0 and one at the next
    float above it, the two sides of softplus' x > 20 branch.
    h0: None, "shared" ([H]) or "rows" ([B, H])."""
    g = torch.Generator().manual_seed(seed)
    rg = torch.randn(B, L, 2 * H, generator=g)
    xc = torch.randn(B, L, H, generator=g)
    z = torch.randn(B, L, H, generator=g)
    dy = torch.randn(B, L, H, generator=g)
    gb = 0.3 * torch.randn(2 * H, generator=g)
    h0_rows = torch.randn(B, H, generator=g)
    if regime == "init":
        lam = torch.linspace(-2.2, -6.9, H)
    elif regime == "wide":
        rg, z = 4 * rg, 4 * z
        lam = torch.linspace(WIDE_LAMBDA_MIN, 25, H)
        lam[1] = 20.0
        lam[H - 2] = torch.nextafter(torch.tensor(20.0), torch.tensor(math.inf))
    else:
        raise ValueError(regime)
    h = {None: None, "shared": h0_rows[0].clone(), "rows": h0_rows}[h0]
    return SimpleNamespace(rg=rg, xc=xc, z=z, dy=dy, lam=lam, gate_b=gb if gate_b else None, h0=h)


def reference(rg, xc, z, lam, gate_b, h0, dy, lengths=None, dtype=torch.float64):
    """rg [B, L, 2H], xc / z / dy [B, L, H], lam [H], gate_b [2H] | None,
    h0 None | [H] | [B, H], lengths None | B ints in 1..L.  Computed in `dtype`.

    Returns y [B, L, H], y_last [B, H] (y at each sequence's last position),
    tile_h [B, ceil(L / 16), H] (h entering tile k: h0 for k = 0, h at
    t = 16k - 1 after), drg, dxc, dz, dlam [H], dgate_b [2H] and dh0: [B, H]
    for a per-row h0, [H] (summed over rows) for a shared or absent one."""
    B, L, H = xc.shape
    assert rg.shape == (B, L, 2 * H) and z.shape == xc.shape == dy.shape and lam.shape == (H,)
    lens = torch.full((B,), L) if lengths is None else torch.as_tensor(lengths)
    assert lens.shape == (B,) and int(lens.min()) >= 1 and int(lens.max()) <= L

    def leaf(t):
        return t.detach().to(dtype).clone().requires_grad_()

    rg_, xc_, z_ = leaf(rg), leaf(xc), leaf(z)
    lam_ = leaf(lam.expand(B, L, H))      # one leaf per position: dlam's summands
    gb_ = leaf(torch.zeros(2 * H) if gate_b is None else gate_b)
    per_row = h0 is not None and h0.dim() == 2
    h0_ = leaf(torch.zeros(B, H) if h0 is None else h0.expand(B, H))
    dy_ = dy.detach().to(dtype)

    g = rg_ + gb_
    alpha = torch.exp(-F.softplus(lam_) * torch.sigmoid(g[..., :H]))
    beta = torch.sqrt(1 - alpha.pow(2) + 1e-8) * torch.sigmoid(g[..., H:])
    bx = beta * xc_
    h, hs, tile_h = h0_, [], []
    for t in range(L):
        if t % TILE == 0:
            tile_h.append(h)
        live = (t < lens).unsqueeze(1)
        h = torch.where(live, alpha[:, t] * h + bx[:, t], h)
        hs.append(h)
    valid = (torch.arange(L)[None, :] < lens[:, None]).unsqueeze(2)
    y = torch.where(valid, F.silu(z_) * torch.stack(hs, 1), torch.zeros((), dtype=dtype))
    (y * dy_).sum().backward()

    y = y.detach()
    dh0 = h0_.grad
    return SimpleNamespace(
        y=y, y_last=y[torch.arange(B), lens - 1], tile_h=torch.stack(tile_h, 1).detach(),
        drg=rg_.grad, dxc=xc_.grad, dz=z_.grad, dlam=lam_.grad.sum((0, 1)), dgate_b=gb_.grad,
        dh0=dh0 if per_row else dh0.sum(0), lengths=lens,
        # what the three sums add up, for their scale (channel_error)
        terms=dict(dlam=lam_.grad, dgate_b=rg_.grad, dh0=dh0))


def bf16_ulp(ref: torch.Tensor) -> torch.Tensor:
    """One bf16 unit in the last place (8 significant bits) of each element."""
    a = ref.detach().double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def channel_error(got, ref64, slack=None, scale=None) -> float:
    """max |got - ref64| / cmax, cmax the per-channel (last axis) max of
    |ref64| over rows and time.  Channels differ in conditioning as Lambda
    does, so each is judged at its own scale.

    scale: for a tensor that is itself a sum over rows and time (dlam,
    dgate_b, a shared dh0), the summands [..., C]; the channel's scale is
    then the sum of their magnitudes, the quantity a summation error is
    proportional to (|error| <= n eps sum|t_i|).  A sum has no rows or time of
    its own, and |sum| is no scale: where the summands cancel (init regime,
    B=5, L=37, H=24, seed 3: dlam[19] = 4.9e-3 among neighbours of 0.1 .. 1)
    plain fp32 is already 1.6e-3 off relative to it, 4e-5 or less elsewhere.
    slack: an absolute allowance per element (one bf16 ulp for bf16 storage)
    taken off the difference."""
    got, ref64 = got.detach().double().cpu(), ref64.detach().double()
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    diff = (got - ref64).abs()
    if slack is not None:
        diff = (diff - slack).clamp_min(0.0)
    C = ref64.shape[-1]
    if scale is None:
        cmax = ref64.abs().reshape(-1, C).max(0).values
    else:
        assert scale.shape[-1] == C
        cmax = scale.detach().double().abs().reshape(-1, C).sum(0)
    rel = torch.where(cmax > 0, diff / cmax.clamp_min(1e-300),
                      torch.where(diff > 0, math.inf, 0.0).to(diff.dtype))
    rel = torch.nan_to_num(rel, nan=math.inf)     # a NaN from the kernel never passes
    return float(rel.max()) if rel.numel() else 0.0


def bar(e32: float, M: float) -> float:
    return M * e32 + FLOOR


def judge(got, ref64, ref32, M, bf16=False, scale=None, scale32=None):
    """(passes, error, bar, ratio) of one tensor.  ratio = error / max(e32,
    FLOOR) is the figure M is sized from (twice its worst measured value).

    For a sum (scale given, scale32 its summands in the fp32 run) the yardstick
    is the larger of the sum's own e32 and its summands': the fp32 run's
    rounding errors can cancel in a sum by luck (wide regime, 3 x 17 x 5:
    dgate_b 7.6e-8 of sum|t_i|, under one rounding, from summands 1.9e-6 off),
    and no fp32 sum can be asked to be more exact than what it adds up."""
    e32 = channel_error(ref32, ref64, scale=scale)
    if scale is not None and scale32 is not None:
        e32 = max(e32, channel_error(scale32, scale))
    err = channel_error(got, ref64, bf16_ulp(ref64) if bf16 else None, scale)
    limit = bar(e32, M)
    return err <= limit, err, limit, err / max(e32, FLOOR)


def judge_all(got, r64, r32, M, bf16=False, names=TENSORS):
    """judge() for each named tensor of `got` (anything with those attributes
    or keys) against the two reference runs: {name: (passes, error, bar,
    ratio)}.  M: one number or {name: number}."""
    out = {}
    for n in names:
        g = got[n] if isinstance(got, dict) else getattr(got, n)
        ref = getattr(r64, n)
        is_sum = ref.dim() == 1
        m = M[n] if isinstance(M, dict) else M
        out[n] = judge(g, ref, getattr(r32, n), m, bf16 and n in BF16_ROUNDED,
                       r64.terms[n] if is_sum else None, r32.terms[n] if is_sum else None)
    return out

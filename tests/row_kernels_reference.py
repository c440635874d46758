"""A plain torch restatement of the row kernels (csrc/rownorm.hip: rb_add_ln_fwd
/ _bwd2, rb_silu_dropout_fwd / _bwd, rb_dropout_mask), with autograd, and the
comparison the tests judge them by.  No GPU; of the product only the host
Philox generator (kernels.philox4x32_10, held to known answers by
test_pairs_host.py).

    s = a * keep / (1 - p) + r                    (a = table[idx] when idx is given)
    y = (s - mean) * rstd * gamma + beta,          rstd = (var + eps)^-1/2
    u = silu(a + bias) * keep / (1 - p)

The row statistics are spelt out (mean, then the biased variance of the
centred row); the gradients come from autograd on sum(y * (dy + dy2)) and
sum(u * du).  Run in float64 for the reference and in float32 for the
yardstick e32.  The error measure and the bar are gate_scan_reference's.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from gate_scan_reference import FLOOR, bar, channel_error, judge  # noqa: F401

EPS = 1e-12                    # the model's layer_norm_eps
SILU_ZERO_SLOPE = -1.2784645   # silu'(x) = 0 here
LN_TENSORS = ("y", "s", "mean", "rstd", "ds", "da", "dgamma", "dbeta", "dbias")
SILU_TENSORS = ("u", "da", "dbias")
SUMS = ("dgamma", "dbeta", "dbias")

# Largest |row mean| of regime "offset".  A row of mean m and unit spread loses
# log2(m) bits of its centred values to the rounding of s and of the mean in
# any fp32 arithmetic: the fp32 run of this reference is then about m * 2^-24
# off in y, judged per row.  With means over +-1e3 that run is 1.2e-4 off in y
# in the worst of the 262161 rows of 16 that the GPU test lists (8.7e-5 at 67
# x 16), over the 1e-4 the regimes are held to; that number decided it, and the
# regime is narrowed to +-500 (test_conv_row_reference_host.py prints what it
# reaches there).
OFFSET_MEAN_MAX = 500.0


def philox_keep(seed, p, n):
    """uint8 [n] keep flags of the row kernels' dropout stream (capi.hip:
    make_drop, common.h: DropSpec::get4): elements 4i .. 4i+3 are the four
    words of Philox4x32-10 at counter (i low, i high, 0, 0) under key (seed
    low, seed high); an element is kept iff its word < floor((1 - p) * 2^32).
    p is the kernels' float32 p."""
    from datamining_recblr_amd.kernels import philox4x32_10

    assert n % 4 == 0
    i = np.arange(n // 4, dtype=np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    zero = np.zeros_like(i)
    words = philox4x32_10((i & m32, i >> np.uint64(32), zero, zero),
                          (np.uint64(seed) & m32, np.uint64(seed) >> np.uint64(32)))
    thresh = np.uint64(int((1.0 - float(np.float32(p))) * 4294967296.0))
    keep = np.stack([w < thresh for w in words], 1).reshape(n)
    return torch.from_numpy(keep.astype(np.uint8))


def make_ln_inputs(regime, rows, d, seed, r=True, table=0):
    """fp32 operands of one LayerNorm case: a [rows, d] (table > 0: a [table,
    d] table and idx [rows], in range, with id 0 and a repeated id), r, gamma,
    beta, dy, dy2.

    "init": everything randn.
    "offset": row means spread over +-OFFSET_MEAN_MAX; even rows have unit
    spread, odd rows a spread of 1e-2 of their |mean| (at least 1e-2); gamma in
    [0.5, 2) with random sign, and dy = randn + a column profile of size 3
    with non-zero mean, so mean(g) and mean(g * xh) are as large as g.  The
    offset sits in r when there is one, else in a.  No row is constant."""
    g = torch.Generator().manual_seed(seed)
    n_a = table if table else rows
    a = torch.randn(n_a, d, generator=g)
    rr = torch.randn(rows, d, generator=g)
    gamma = torch.randn(d, generator=g)
    beta = torch.randn(d, generator=g)
    dy = torch.randn(rows, d, generator=g)
    dy2 = torch.randn(rows, d, generator=g)
    idx = None
    if table:
        idx = torch.randint(0, table, (rows,), generator=g)
        idx[0] = 0
        if rows > 2:
            idx[rows - 1] = idx[1]
    if regime == "offset":
        def offset(n):
            mean = torch.linspace(-OFFSET_MEAN_MAX, OFFSET_MEAN_MAX, n) if n > 1 else \
                torch.tensor([OFFSET_MEAN_MAX])
            spread = torch.ones(n)
            spread[1::2] = (1e-2 * mean[1::2].abs()).clamp_min(1e-2)
            return mean[:, None], spread[:, None]
        if r:
            mean, spread = offset(rows)
            rr = mean + spread * rr
            a = a * (spread if not table else 1.0)
        else:
            mean, spread = offset(n_a)
            a = mean + spread * a
        gamma = (0.5 + 1.5 * torch.rand(d, generator=g)) * torch.where(gamma < 0, -1.0, 1.0)
        col = 3.0 * (1.0 + 0.5 * torch.randn(d, generator=g))
        dy = dy + col
    elif regime != "init":
        raise ValueError(regime)
    return SimpleNamespace(a=a, r=rr if r else None, gamma=gamma, beta=beta, dy=dy, dy2=dy2,
                           idx=idx)


def ln_reference(a, r, gamma, beta, dy, dy2=None, keep=None, p=0.0, idx=None, eps=EPS,
                 dtype=torch.float64):
    """a [rows, d] (or the table [V, d] with idx [rows]), r [rows, d] | None,
    keep [rows, d] of 0 / 1 | None.  Returns y, s [rows, d], mean, rstd [rows],
    ds, da [rows, d], dgamma, dbeta, dbias [d], dtable [V, d] (idx given) and
    terms: the per-row summands of the three column sums."""
    def leaf(t):
        return t.detach().to(dtype).clone().requires_grad_()

    rows = idx.numel() if idx is not None else a.shape[0]
    d = a.shape[1]
    a_ = leaf(a if idx is None else a[idx])           # one leaf per row: da
    r_ = leaf(torch.zeros(rows, d) if r is None else r)   # ds = the gradient of s = ... + r
    gm_ = leaf(gamma.expand(rows, d))
    bt_ = leaf(beta.expand(rows, d))
    g = dy.detach().to(dtype)
    if dy2 is not None:
        g = g + dy2.detach().to(dtype)
    s = a_
    if keep is not None:
        s = s * keep.to(dtype) / (1.0 - p)
    s = s + r_
    mean = s.sum(1, keepdim=True) / d
    c = s - mean
    var = (c * c).sum(1, keepdim=True) / d
    rstd = (var + eps) ** -0.5
    y = c * rstd * gm_ + bt_
    (y * g).sum().backward()
    da = a_.grad
    out = SimpleNamespace(
        y=y.detach(), s=s.detach(), mean=mean.detach()[:, 0], rstd=rstd.detach()[:, 0],
        ds=r_.grad, da=da, dgamma=gm_.grad.sum(0), dbeta=bt_.grad.sum(0), dbias=da.sum(0),
        dtable=None, terms=dict(dgamma=gm_.grad, dbeta=bt_.grad, dbias=da))
    if idx is not None:
        out.dtable = torch.zeros(a.shape, dtype=dtype).index_add_(0, idx, da)
    return out


def make_silu_inputs(regime, rows, d, seed, bias=True):
    """fp32 a, du [rows, d] and bias [d] | None.  "init": randn (bias 0.5 *
    randn).  "wide": a scaled by 12, so SiLU saturates on both sides, column 0
    biased by +20, column 1 by -20, and column 2 by -1.278 with a scaled by
    0.01 there: within about +-0.4 of the zero of silu'.  (Without a bias the
    columns keep their scales.)"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(rows, d, generator=g)
    du = torch.randn(rows, d, generator=g)
    b = 0.5 * torch.randn(d, generator=g)
    if regime == "wide":
        a = 12.0 * a
        a[:, 2] = 0.01 * a[:, 2]
        b[0], b[1], b[2] = 20.0, -20.0, SILU_ZERO_SLOPE
    elif regime != "init":
        raise ValueError(regime)
    return SimpleNamespace(a=a, du=du, bias=b if bias else None)


def silu_reference(a, du, bias=None, keep=None, p=0.0, dtype=torch.float64):
    """u = silu(a + bias) * keep / (1 - p); da, dbias [d] (the column sum of
    da) from autograd on sum(u * du); terms: dbias' summands."""
    a_ = a.detach().to(dtype).clone().requires_grad_()
    x = a_ if bias is None else a_ + bias.detach().to(dtype)
    u = F.silu(x)
    if keep is not None:
        u = u * keep.to(dtype) / (1.0 - p)
    (u * du.detach().to(dtype)).sum().backward()
    da = a_.grad
    return SimpleNamespace(u=u.detach(), da=da, dbias=da.sum(0), terms=dict(dbias=da))


def judge_all(got, r64, r32, M, names, by_row=False):
    """judge() for each named tensor of `got` (a dict): {name: (passes, error,
    bar, ratio)}.

    SiLU (by_row False): a [rows, d] tensor is judged per column, as the bias
    makes the columns differ, and dbias on the sum of its summands' magnitudes.

    LayerNorm (by_row True): a [rows, d] tensor is judged per row, each row at
    its own max, because the rows are what differ in conditioning (their mean
    and spread) and each holds at least 16 elements; a column of a 1-row case
    is a single element, and an element of y or ds next to a zero crossing has
    no relative accuracy in any arithmetic (fp32 run, offset regime, 1 x 16
    with a mask: 5.7e-3 of the element in dgamma, 2.1e-4 in y).  For the same
    reason a summand of dgamma, dbeta or dbias counts with its row's max
    magnitude, the scale its own error is proportional to, in the sum of
    magnitudes that a column sum is judged on.  mean [rows] is itself a sum
    over its row and is judged on sum_j |s_ij| / d (a row mean may be anything
    near 0: 1 x 256 randn, mean 0.06); rstd [rows] is positive and each row's
    is judged on its own value."""
    out = {}
    for n in names:
        ref, r3, t = getattr(r64, n), getattr(r32, n), got[n]
        m = M[n] if isinstance(M, dict) else M
        if n in SUMS and by_row:
            terms = r64.terms[n].abs()
            out[n] = judge(t, ref, r3, m, False, terms.max(1, keepdim=True).values.expand_as(terms))
        elif n in SUMS:
            out[n] = judge(t, ref, r3, m, False, r64.terms[n], r32.terms[n])
        elif n == "mean":       # a sum over its row: judged on sum_j |s_ij| / d
            out[n] = judge(t, ref, r3, m, False, r64.s.t() / r64.s.shape[1])
        elif n == "rstd":       # positive: each row at its own value
            out[n] = judge(t, ref, r3, m)
        elif by_row and n != "dtable":
            out[n] = judge(t.t(), ref.t(), r3.t(), m)
        else:
            out[n] = judge(t, ref, r3, m)
    return out

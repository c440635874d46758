"""The conv + SiLU and row-kernel references (tests/conv_silu_reference.py,
tests/row_kernels_reference.py) and their bars, checked on the CPU before the
GPU tests (test_gpu_conv_silu_ref.py, test_gpu_row_kernels_ref.py) rely on them.

1. Each reference agrees in fp64, to 1e-12 of the tensor's scale, with an
   independent formulation and its autograd: F.conv1d on the left-padded input,
   F.layer_norm / F.silu / F.embedding.
2. The yardstick e32 (the reference's fp32 run against its fp64 run) stays
   under 1e-4 on every tensor of every case the GPU tests list, so no bar
   M * e32 + floor exceeds about 2e-3; and that fp32 run passes at M = 1.
3. The bar can fail: planted errors, emulated in fp32 on the listed cases'
   own inputs, are each rejected at M = 16.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_silu_reference as C
import row_kernels_reference as R
import test_gpu_conv_silu_ref as TC
import test_gpu_row_kernels_ref as TR

CONV = {p.id: p.values[0] for p in TC.CASES}
ROW = {p.id: p.values[0] for p in TR.LN_CASES + TR.SILU_CASES + TR.OPTION_CASES}
GRID = [i for i in ROW if "-grid-" in i]


def _close(a, b, what):
    scale = float(b.abs().max())
    assert float((a - b).abs().max()) <= 1e-12 * max(scale, 1e-300), what


# ---------------------------------------------------------------- 1. cross-checks

@pytest.mark.parametrize("regime", ["init", "wide"])
@pytest.mark.parametrize("K", [1, 2, 4, 7, 8])
@pytest.mark.parametrize("lengths", [None, [19, 5, 1, 16]])
def test_conv_reference_equals_conv1d(regime, K, lengths):
    B, L, H = 4, 19, 7
    i = C.make_inputs(regime, B, L, H, K, seed=K)
    r = C.reference(i.x, i.w, i.bias, i.g1, i.g2, lengths)
    x, w, b = (t.double().requires_grad_() for t in (i.x, i.w, i.bias))
    acc = F.conv1d(F.pad(x.transpose(1, 2), (K - 1, 0)), w.unsqueeze(1), b, groups=H)
    lens = torch.tensor(lengths if lengths else [L] * B)
    valid = (torch.arange(L)[None, :] < lens[:, None]).unsqueeze(2)
    xc = F.silu(acc).transpose(1, 2) * valid
    (xc * (i.g1.double() + i.g2.double())).sum().backward()
    _close(r.xc, xc.detach(), "xc")
    _close(r.dx, x.grad, "dx")
    _close(r.dw, w.grad, "dw")
    _close(r.db, b.grad, "db")
    _close(r.terms["dw"].sum((0, 1)), r.dw, "dw terms")
    _close(r.terms["db"].sum((0, 1)), r.db, "db terms")
    assert float(r.xc[~valid.expand_as(r.xc)].abs().max() if lengths else 0) == 0


@pytest.mark.parametrize("regime", ["init", "offset"])
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("table", [0, 9])
@pytest.mark.parametrize("r", [True, False])
def test_ln_reference_equals_layer_norm(regime, drop, table, r):
    rows, d = 13, 32
    i = R.make_ln_inputs(regime, rows, d, seed=3, r=r, table=table)
    p = 0.2 if drop else 0.0
    keep = R.philox_keep(11, p, rows * d).view(rows, d) if drop else None
    ref = R.ln_reference(i.a, i.r, i.gamma, i.beta, i.dy, i.dy2, keep, p, i.idx)
    a, gamma, beta = (t.double().requires_grad_() for t in (i.a, i.gamma, i.beta))
    s = F.embedding(i.idx, a) if table else a
    if drop:
        s = s * keep.double() / (1.0 - p)
    if r:
        s = s + i.r.double()
    s.retain_grad()
    y = F.layer_norm(s, (d,), gamma, beta, R.EPS)
    (y * (i.dy.double() + i.dy2.double())).sum().backward()
    _close(ref.y, y.detach(), "y")
    _close(ref.s, s.detach(), "s")
    _close(ref.mean, s.detach().mean(1), "mean")
    _close(ref.rstd, (s.detach().var(1, unbiased=False) + R.EPS).rsqrt(), "rstd")
    _close(ref.ds, s.grad, "ds")
    _close(ref.dgamma, gamma.grad, "dgamma")
    _close(ref.dbeta, beta.grad, "dbeta")
    if table:
        _close(ref.dtable, a.grad, "dtable")
    else:
        _close(ref.da, a.grad, "da")
    _close(ref.dbias, ref.da.sum(0), "dbias")
    for n in R.SUMS:
        _close(ref.terms[n].sum(0), getattr(ref, n), n + " terms")


@pytest.mark.parametrize("regime", ["init", "wide"])
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("bias", [True, False])
def test_silu_reference_equals_functional(regime, drop, bias):
    rows, d = 13, 32
    i = R.make_silu_inputs(regime, rows, d, seed=5, bias=bias)
    p = 0.2 if drop else 0.0
    keep = R.philox_keep(12, p, rows * d).view(rows, d) if drop else None
    ref = R.silu_reference(i.a, i.du, i.bias, keep, p)
    a = i.a.double().requires_grad_()
    b = torch.zeros(d).double().requires_grad_() if not bias else i.bias.double().requires_grad_()
    x = a + b
    u = x * torch.sigmoid(x)
    if drop:
        u = u * keep.double() / (1.0 - p)
    (u * i.du.double()).sum().backward()
    _close(ref.u, u.detach(), "u")
    _close(ref.da, a.grad, "da")
    _close(ref.dbias, b.grad, "dbias")


def test_philox_keep_counter_and_threshold():
    """The stream restated: element e takes word e % 4 of the block at counter
    e / 4 under key (seed low, seed high)."""
    from datamining_recblr_amd.kernels import philox4x32_10

    seed, p = (3 << 32) + 9, 0.5
    keep = R.philox_keep(seed, p, 64)
    for e in (0, 5, 63):
        w = philox4x32_10((e // 4, 0, 0, 0), (9, 3))[e % 4]
        assert int(keep[e]) == int(int(w) < 2 ** 31)
    # p is the kernels' float32: 1 - float32(0.2) is not 0.8
    frac = float(R.philox_keep(1, 0.2, 1 << 16).float().mean())
    assert abs(frac - 0.8) < 0.01


# ---------------------------------------------------------------- 2. the regimes' yardsticks

def _yard(mod, cases):
    worst, bad = {}, {}
    for id, c in cases.items():
        for n, e in mod.yardsticks(c).items():
            if e > worst.get(n, (0.0, ""))[0]:
                worst[n] = (e, id)
            if not e <= 1e-4:
                bad[(id, n)] = e
    print({n: f"{e:.2e} {id}" for n, (e, id) in worst.items()})
    assert not bad, bad


def test_conv_yardsticks_under_1e_4():
    """Every listed conv case: e32 <= 1e-4 on every tensor (and, e32 being the
    fp32 run's own error, that run passes at M = 1)."""
    _yard(TC, CONV)


def test_row_yardsticks_under_1e_4():
    _yard(TR, {i: c for i, c in ROW.items() if i not in GRID})


@pytest.mark.parametrize("id", GRID)
def test_row_grid_yardsticks_under_1e_4(id):
    _yard(TR, {id: ROW[id]})


def test_fp32_run_passes_at_m_1():
    for id in ("dense-wide-K4-3x17x5", "packed-wide-K7-11seq-H36-g2"):
        _, r64, r32 = TC._prepare(CONV[id])
        assert all(v[0] for v in C.judge_all(r32, r64, r32, 1).values()), id
    for id in ("ln-offset-7x64-philox", "silu-wide-7x16-mask", "ln-gather-offset-19x64-philox"):
        c = ROW[id]
        _, _, _, r64, r32 = TR._prepare(c)
        got = {n: getattr(r32, n) for n in TR._names(c)}
        assert all(v[0] for v in R.judge_all(got, r64, r32, 1, TR._names(c), c["kind"] == "ln").values()), id


# ---------------------------------------------------------------- 3. planted errors

def _dsilu(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def conv_fp32(c, fault=None):
    """The conv forward and backward of a listed case by the kernels' formulas
    in fp32 torch, with one planted error.  "history": a packed sequence's first
    rows see the rows packed before them; "lookahead": du of a later backward
    tile taken as zero; "tail": the rows of the last partial backward tile past
    L (clamped loads) summed into dw and db; "g2": g2 left out."""
    i, r64, _ = TC._prepare(c)
    K, H = c["K"], c["H"]
    tile = 32 if K >= 6 else 16          # conv_silu.hip: launch_conv_bwd
    B, L, _ = i.x.shape
    xc, dx = torch.zeros(B, L, H), torch.zeros(B, L, H)
    dw, db = torch.zeros(H, K), torch.zeros(H)
    prev = torch.zeros(K - 1, H)
    for b in range(B):
        n = int(r64.lengths[b])
        x = i.x[b, :n]
        hist = prev if fault == "history" else torch.zeros(K - 1, H)
        xp = torch.cat([hist, x])
        prev = torch.cat([prev, x])[-(K - 1):] if K > 1 else prev
        acc = i.bias + sum(i.w[:, k] * xp[k:k + n] for k in range(K))
        xc[b, :n] = F.silu(acc)
        g = i.g1[b, :n] + (i.g2[b, :n] if i.g2 is not None and fault != "g2" else 0)
        du = g * _dsilu(acc)
        for t in range(n):
            for k in range(K):
                m = t + K - 1 - k
                if m < n and not (fault == "lookahead" and m // tile > t // tile):
                    dx[b, t] += i.w[:, k] * du[m]
        db += du.sum(0)
        for k in range(K):
            dw[:, k] += (du * xp[k:k + n]).sum(0)
        if fault == "tail":
            for t in range(n, -(-n // tile) * tile):
                rows = [x[min(max(t - (K - 1) + k, 0), n - 1)] * (t - (K - 1) + k >= 0)
                        for k in range(K)]
                e = g[n - 1] * _dsilu(i.bias + sum(i.w[:, k] * rows[k] for k in range(K)))
                db += e
                for k in range(K):
                    dw[:, k] += e * rows[k]
    return dict(xc=xc, dx=dx, dw=dw, db=db)


def ln_fp32(c, fault=None):
    """add_ln_fwd / _bwd by the kernels' formulas in fp32 torch, with one
    planted error.  "var": E[s^2] - mean^2; "mgx": the mean(g * xh) term
    dropped from ds; "dy2": dy2 left out; "dgamma": dgamma summed from g = dy *
    gamma; "dbeta": the rows of the last partial wave step counted twice."""
    i, keep, p, _, _ = TR._prepare(c)
    a = i.a if i.idx is None else i.a[i.idx]
    m = torch.ones_like(a) if keep is None else keep.float() * (1.0 / (1.0 - p))
    s = a * m + (i.r if i.r is not None else 0)
    d = s.shape[1]
    mean = s.mean(1, keepdim=True)
    var = (s * s).mean(1, keepdim=True) - mean * mean if fault == "var" else \
        ((s - mean) ** 2).mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(var + R.EPS)
    xh = (s - mean) * rstd
    y = xh * i.gamma + i.beta
    dy = i.dy + (i.dy2 if c["dy2"] and fault != "dy2" else 0)
    g = dy * i.gamma
    mgx = 0 if fault == "mgx" else (g * xh).mean(1, keepdim=True)
    ds = rstd * (g - g.mean(1, keepdim=True) - xh * mgx)
    da = ds * m
    dbeta = dy.sum(0)
    if fault == "dbeta":
        w = TR.rpw(d)
        dbeta = dbeta + dy[len(dy) // w * w:].sum(0)
    return dict(y=y, s=s, mean=mean[:, 0], rstd=rstd[:, 0], ds=ds, da=da,
                dgamma=((g if fault == "dgamma" else dy) * xh).sum(0), dbeta=dbeta,
                dbias=da.sum(0))


def silu_fp32(c, fault=None):
    """silu_dropout_fwd / _bwd in fp32 torch.  "bias": the derivative taken at
    a instead of a + bias; "dbias": dbias summed from du instead of da."""
    i, keep, p, _, _ = TR._prepare(c)
    m = torch.ones_like(i.a) if keep is None else keep.float() * (1.0 / (1.0 - p))
    x = i.a + (i.bias if i.bias is not None else 0)
    da = i.du * m * _dsilu(i.a if fault == "bias" else x)
    return dict(u=F.silu(x) * m, da=da, dbias=(i.du if fault == "dbias" else da).sum(0))


def _conv_rejected(id, fault):
    c = CONV[id]
    _, r64, r32 = TC._prepare(c)
    res = C.judge_all(conv_fp32(c, fault), r64, r32, 16)
    return [n for n, v in res.items() if not v[0]]


def _row_rejected(id, fault):
    c = ROW[id]
    _, _, _, r64, r32 = TR._prepare(c)
    names = [n for n in TR._names(c) if n != "dtable"]
    got = (ln_fp32 if c["kind"] == "ln" else silu_fp32)(c, fault)
    return [n for n, v in R.judge_all(got, r64, r32, 16, names, c["kind"] == "ln").items() if not v[0]]


CONV_FAULTS = {
    "history": ("packed-init-K4-4seq-H6-g2", "packed-wide-K7-11seq-H36-g2"),
    "lookahead": ("dense-init-K4-3x17x5", "dense-wide-K7-2x65x20"),
    "tail": ("dense-init-K4-3x17x5", "dense-wide-K8-3x33x6"),
    "g2": ("dense-init-K4-3x17x5", "packed-wide-K4-4seq-H5-g2"),
}
ROW_FAULTS = {
    "var": ("ln-offset-7x64-none", "ln-offset-17x16-philox"),
    "mgx": ("ln-init-7x64-none", "ln-offset-7x1024-mask"),
    "dy2": ("ln-options-init-19x64-philox", "ln-options-offset-6x512-none"),
    "dgamma": ("ln-init-7x64-none", "ln-offset-17x16-philox"),
    "dbeta": ("ln-init-17x16-none", "ln-offset-67x16-mask"),
    "bias": ("silu-init-7x16-none", "silu-wide-7x512-philox"),
    "dbias": ("silu-init-7x16-mask", "silu-wide-7x512-philox"),
}


@pytest.mark.parametrize("id", sorted({i for v in CONV_FAULTS.values() for i in v}))
def test_conv_emulation_without_fault_passes(id):
    assert _conv_rejected(id, None) == []


@pytest.mark.parametrize("fault", sorted(CONV_FAULTS))
def test_conv_judge_rejects(fault):
    for id in CONV_FAULTS[fault]:
        assert _conv_rejected(id, fault), (fault, id)


@pytest.mark.parametrize("id", sorted({i for v in ROW_FAULTS.values() for i in v}))
def test_row_emulation_without_fault_passes(id):
    assert _row_rejected(id, None) == []


@pytest.mark.parametrize("fault", sorted(ROW_FAULTS))
def test_row_judge_rejects(fault):
    for id in ROW_FAULTS[fault]:
        assert _row_rejected(id, fault), (fault, id)


def test_var_fault_needs_offset():
    """E[s^2] - mean^2 is harmless on randn rows: only "offset" shows it."""
    assert _row_rejected("ln-init-7x64-none", "var") == []

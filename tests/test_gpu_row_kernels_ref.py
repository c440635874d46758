"""The row kernels (rb_add_ln_fwd / _bwd2, rb_silu_dropout_fwd / _bwd,
rb_dropout_mask) against an independent fp64 reference
(tests/row_kernels_reference.py: spelt-out statistics with autograd, the host
Philox generator), not against torch fp32 or one another.

Per output tensor the error is max |got - ref64| / scale and the bar
M * e32 + 4 * 2^-24, e32 the same error of the reference's own fp32 run on the
same inputs (gate_scan_reference.channel_error / judge).  LayerNorm tensors are
judged per row and SiLU tensors per column, the column sums (dgamma, dbeta,
dbias) on the sum of their summands' magnitudes: row_kernels_reference.judge_all
says how and why.

Value regimes: "init" (randn), "offset" for LayerNorm (row means over +-500,
rows whose spread is 1e-2 of their mean, gamma away from 1, dy with a common
column profile) and "wide" for SiLU (saturated on both sides, one column at
the zero of silu'): row_kernels_reference.make_ln_inputs / make_silu_inputs.

Which path a case runs (rownorm.hip; RPW = 64 / LPR rows per wave step, RPB =
4 * RPW rows per block step):
    every width, rows 1, 7, RPW - 1, RPW + 1, 4 RPW + 3     "ln-*" / "silu-*"
    grid-stride loop of the backward kernels (rows > 1024 RPB)       "*-grid-bwd-*"
    grid-stride loop of add_ln_fwd (rows > 4096 RPB)                 "ln-grid-fwd-*"
    grid-stride loop of silu_dropout_fwd (rows > 8192 RPB)           "silu-grid-fwd-*"
    dy2, want_dbias, want_ds / want_da = False                       test_add_ln_bwd_options
    r = None, save = False, the gathered form                        "ln-nor-*", test_add_ln_save_false,
                                                                     "ln-gather-*"
    dropout: none, an explicit mask, Philox regenerated from (seed, p): the reference
    takes the Philox flags from the host generator (philox_keep), never from the device

M is twice the worst ratio error / max(e32, 4 * 2^-24) measured on an MI355X
over all cases below, rounded up:

    tensor    worst ratio   case                                  M
    add_ln_fwd / add_ln_bwd
    y         2.58          ln-offset-7x64-mask                   6
    s         0.45          ln-init-67x16-mask                    1
    mean      0.71          ln-grid-fwd-offset-262161x16-mask     2
    rstd      1.23          ln-offset-7x128-philox                3
    ds        2.40          ln-offset-7x64-mask                   5
    da        2.61          ln-offset-7x64-mask                   6
    dgamma    2.27          ln-offset-17x16-mask                  5
    dbeta     0.43          ln-grid-bwd-offset-4098x256-philox    1
    dbias     1.80          ln-offset-2x512-mask                  4
    dtable    1.86          ln-gather-offset-6x512-philox         4
    silu_dropout_fwd / silu_dropout_bwd
    u         3.54          silu-wide-7x1024-philox               8
    da        2.96          silu-wide-1x256-none                  6
    dbias     2.96          silu-wide-1x256-none                  6
"""
import functools

import pytest
import torch

import row_kernels_reference as R

pytestmark = pytest.mark.gpu

M_LN = {"y": 6, "s": 1, "mean": 2, "rstd": 3, "ds": 5, "da": 6, "dgamma": 5, "dbeta": 1, "dbias": 4,
        "dtable": 4}
M_SILU = {"u": 8, "da": 6, "dbias": 6}

ROW_SIZES = (16, 32, 64, 128, 256, 512, 1024)
P = 0.2
DROPS = ("none", "mask", "philox")


def rpw(d):
    """Rows per wave step: 64 / LPR, LPR = d / 4 lanes per row (at most 64)."""
    return 64 // min(64, d // 4)


def _rows_of(d):
    w = rpw(d)
    return sorted({1, 7, w - 1, w + 1, 4 * w + 3} - {0})


def _case(id, kind, regime, rows, d, drop, **kw):
    c = dict(kind=kind, regime=regime, rows=rows, d=d, drop=drop, r=True, dy2=False, table=0,
             bias=True)
    c.update(kw)
    return pytest.param(c, id=id)


def _cases():
    ln, silu = [], []
    # 1. every width, the row counts around a wave step, the three dropout modes
    for d in ROW_SIZES:
        for rows in _rows_of(d):
            for drop in DROPS:
                for r in ("init", "offset"):
                    ln.append(_case(f"ln-{r}-{rows}x{d}-{drop}", "ln", r, rows, d, drop))
                for r in ("init", "wide"):
                    silu.append(_case(f"silu-{r}-{rows}x{d}-{drop}", "silu", r, rows, d, drop))
    # 2. the smallest row count past each kernel's grid, plus an odd tail
    for d in (16, 128, 256, 1024):
        w = rpw(d)
        tail = w + 1
        n_bwd, n_lnf, n_sif = 1024 * 4 * w + tail, 4096 * 4 * w + tail, 8192 * 4 * w + tail
        ln.append(_case(f"ln-grid-bwd-offset-{n_bwd}x{d}-philox", "ln", "offset", n_bwd, d, "philox"))
        ln.append(_case(f"ln-grid-fwd-offset-{n_lnf}x{d}-mask", "ln", "offset", n_lnf, d, "mask"))
        silu.append(_case(f"silu-grid-bwd-wide-{n_bwd}x{d}-philox", "silu", "wide", n_bwd, d,
                          "philox"))
        silu.append(_case(f"silu-grid-fwd-wide-{n_sif}x{d}-mask", "silu", "wide", n_sif, d, "mask"))
    # 3. no residual; the gathered form (a repeated id and id 0)
    for r in ("init", "offset"):
        for d, rows in ((64, 19), (512, 6)):
            ln.append(_case(f"ln-nor-{r}-{rows}x{d}-philox", "ln", r, rows, d, "philox", r=False))
            ln.append(_case(f"ln-gather-{r}-{rows}x{d}-philox", "ln", r, rows, d, "philox",
                            table=11))
            ln.append(_case(f"ln-gather-nor-{r}-{rows}x{d}-none", "ln", r, rows, d, "none",
                            table=11, r=False))
    # 4. SiLU without the folded bias
    for r in ("init", "wide"):
        for d in (16, 512, 1024):
            rows = 4 * rpw(d) + 3
            silu.append(_case(f"silu-nobias-{r}-{rows}x{d}-philox", "silu", r, rows, d, "philox",
                              bias=False))
    return ln, silu


LN_CASES, SILU_CASES = _cases()
OPTION_CASES = [_case(f"ln-options-{r}-{rows}x{d}-{drop}", "ln", r, rows, d, drop, dy2=True)
                for r in ("init", "offset") for d, rows in ((64, 19), (512, 6))
                for drop in ("philox", "none")]


def _seed(c):
    return 7 * c["rows"] + c["d"] + 1000003 * DROPS.index(c["drop"])


def _keep(c):
    """(keep [rows, d] uint8 | None, p): the flags the reference uses.  Philox:
    from the host generator at the case's seed."""
    rows, d = c["rows"], c["d"]
    if c["drop"] == "none":
        return None, 0.0
    if c["drop"] == "philox":
        return R.philox_keep(_seed(c), P, rows * d).view(rows, d), P
    g = torch.Generator().manual_seed(_seed(c) + 1)
    return (torch.rand(rows, d, generator=g) >= P).to(torch.uint8), P


@functools.lru_cache(maxsize=8)
def _prepare_key(key):
    c = dict(key)
    keep, p = _keep(c)
    if c["kind"] == "ln":
        i = R.make_ln_inputs(c["regime"], c["rows"], c["d"], _seed(c), r=c["r"], table=c["table"])
        args = (i.a, i.r, i.gamma, i.beta, i.dy, i.dy2 if c["dy2"] else None, keep, p, i.idx)
        return i, keep, p, R.ln_reference(*args), R.ln_reference(*args, dtype=torch.float32)
    i = R.make_silu_inputs(c["regime"], c["rows"], c["d"], _seed(c), bias=c["bias"])
    args = (i.a, i.du, i.bias, keep, p)
    return i, keep, p, R.silu_reference(*args), R.silu_reference(*args, dtype=torch.float32)


def _prepare(c):
    """Inputs, keep flags and the two reference runs of a case (CPU)."""
    return _prepare_key(tuple(sorted(c.items())))


def _names(c):
    if c["kind"] == "silu":
        return R.SILU_TENSORS
    return R.LN_TENSORS + (("dtable",) if c["table"] else ())


def yardsticks(c):
    """{tensor: e32} of a case: what plain fp32 makes of its inputs (no GPU)."""
    _, _, _, r64, r32 = _prepare(c)
    got = {n: getattr(r32, n) for n in _names(c)}
    return {n: (v[2] - R.FLOOR) / 16 for n, v in R.judge_all(got, r64, r32, 16, _names(c), c["kind"] == "ln").items()}


def _drop_args(c, keep, dev, force_mask=False):
    if c["drop"] == "none":
        return {}
    if c["drop"] == "philox" and not force_mask:
        return dict(seed=_seed(c), p=P)
    return dict(mask=keep.to(dev), p=P)


def _ln_gpu(c, i, keep, dev, force_mask=False, **bwd_kw):
    """add_ln_fwd and add_ln_bwd of a case: the outputs by name (on the GPU)."""
    from datamining_recblr_amd import kernels

    kw = _drop_args(c, keep, dev, force_mask)
    idx = None if i.idx is None else i.idx.to(dev)
    r = None if i.r is None else i.r.to(dev)
    gamma = i.gamma.to(dev)
    y, s, mean, rstd = kernels.add_ln_fwd(i.a.to(dev), r, gamma, i.beta.to(dev), R.EPS, idx=idx,
                                          **kw)
    opts = dict(want_dbias=True, dy2=i.dy2.to(dev) if c["dy2"] else None)
    opts.update(bwd_kw)
    ds, da, dgamma, dbeta, dbias = kernels.add_ln_bwd(i.dy.to(dev), s, gamma, mean, rstd, **kw,
                                                      **opts)
    got = dict(y=y, s=s, mean=mean, rstd=rstd, ds=ds, da=da, dgamma=dgamma, dbeta=dbeta,
               dbias=dbias)
    if idx is not None and da is not None:
        got["dtable"] = kernels.embedding_bwd(idx, da, i.a.shape[0], padding_idx=None)
    torch.cuda.synchronize()
    return got


def _silu_gpu(c, i, keep, dev, force_mask=False, want_dbias=True):
    from datamining_recblr_amd import kernels

    kw = _drop_args(c, keep, dev, force_mask)
    a = i.a.to(dev)
    bias = None if i.bias is None else i.bias.to(dev)
    u = kernels.silu_dropout_fwd(a, bias=bias, **kw)
    da, dbias = kernels.silu_dropout_bwd(a, i.du.to(dev), want_dbias=want_dbias, bias=bias, **kw)
    torch.cuda.synchronize()
    return dict(u=u, da=da, dbias=dbias)


def run_case(c, dev):
    """Runs one case on the GPU: {tensor: (passes, error, bar, ratio)} plus
    "dropped": da is exactly 0 wherever keep is 0."""
    i, keep, p, r64, r32 = _prepare(c)
    ln = c["kind"] == "ln"
    got = (_ln_gpu if ln else _silu_gpu)(c, i, keep, dev)
    got = {n: v.cpu() for n, v in got.items()}
    out = R.judge_all(got, r64, r32, M_LN if ln else M_SILU, _names(c), ln)
    if keep is not None:
        out["dropped"] = (bool((got["da"][keep == 0] == 0).all()), 0.0, 0.0, 0.0)
    return out


def _report(res):
    for n, (ok, err, limit, ratio) in res.items():
        print(f"{n:8s} err {err:.3e}  bar {limit:.3e}  ratio {ratio:.2f}")
    bad = {n: v for n, v in res.items() if not v[0]}
    assert not bad, bad


@pytest.mark.parametrize("case", LN_CASES + OPTION_CASES)
def test_add_ln_vs_fp64_reference(cuda, case):
    _report(run_case(case, cuda))


@pytest.mark.parametrize("case", SILU_CASES)
def test_silu_dropout_vs_fp64_reference(cuda, case):
    _report(run_case(case, cuda))


@pytest.mark.parametrize("case", OPTION_CASES)
def test_add_ln_bwd_options(cuda, case):
    """Leaving an output out changes no bit of the others (dy2 present)."""
    i, keep, _, _, _ = _prepare(case)
    full = _ln_gpu(case, i, keep, cuda)
    no_ds = _ln_gpu(case, i, keep, cuda, want_ds=False)
    no_da = _ln_gpu(case, i, keep, cuda, want_da=False)
    bare = _ln_gpu(case, i, keep, cuda, want_da=False, want_dbias=False)
    assert no_ds["ds"] is None and no_da["da"] is None and bare["da"] is None
    assert bare["dbias"] is None
    for other, names in ((no_ds, ("da", "dgamma", "dbeta", "dbias")),
                         (no_da, ("ds", "dgamma", "dbeta", "dbias")),
                         (bare, ("ds", "dgamma", "dbeta"))):
        for n in names:
            assert torch.equal(other[n], full[n]), n


@pytest.mark.parametrize("case", [c for c in LN_CASES if "-7x" in c.id or "-nor-" in c.id
                                  or "-gather-" in c.id])
def test_add_ln_save_false(cuda, case):
    """save=False returns y alone, bitwise the saved call's."""
    from datamining_recblr_amd import kernels

    c = case
    i, keep, _, _, _ = _prepare(c)
    dev = cuda
    args = (i.a.to(dev), None if i.r is None else i.r.to(dev), i.gamma.to(dev), i.beta.to(dev),
            R.EPS)
    kw = dict(idx=None if i.idx is None else i.idx.to(dev), **_drop_args(c, keep, dev))
    y, s, mean, rstd = kernels.add_ln_fwd(*args, **kw)
    y2, s2, mean2, rstd2 = kernels.add_ln_fwd(*args, save=False, **kw)
    assert s2 is None and mean2 is None and rstd2 is None and s is not None
    assert torch.equal(y, y2)


@pytest.mark.parametrize("case", [c for c in SILU_CASES if "-grid-" not in c.id
                                  and ("x16-" in c.id or "x512-" in c.id or "x1024-" in c.id)
                                  and "-philox" in c.id])
def test_silu_da_same_without_dbias(cuda, case):
    i, keep, _, _, _ = _prepare(case)
    a, b = _silu_gpu(case, i, keep, cuda), _silu_gpu(case, i, keep, cuda, want_dbias=False)
    assert b["dbias"] is None and a["dbias"] is not None
    assert torch.equal(a["da"], b["da"]) and torch.equal(a["u"], b["u"])


# ---- exact checks, no tolerance

def test_row_sizes():
    from datamining_recblr_amd import kernels

    assert kernels.ROW_SIZES == ROW_SIZES


@pytest.mark.parametrize("shape", [(7, 16), (1029, 64)])
@pytest.mark.parametrize("seed", [0, 1234, (5 << 32) + 77])
@pytest.mark.parametrize("p", [0.1, 0.2, 0.5])
def test_dropout_mask_equals_host_philox(cuda, p, seed, shape):
    from datamining_recblr_amd import kernels

    got = kernels.dropout_mask(seed, p, shape, cuda).cpu()
    want = R.philox_keep(seed, p, shape[0] * shape[1]).view(shape)
    assert torch.equal(got, want)
    assert 0 < int(want.sum()) < want.numel()


@pytest.mark.parametrize("case", [c for c in LN_CASES + SILU_CASES
                                  if "-philox" in c.id and "-grid-" not in c.id
                                  and ("x16-" in c.id or "x256-" in c.id or "x1024-" in c.id
                                       or "-gather-" in c.id)])
def test_mask_run_equals_philox_run(cuda, case):
    """The explicit-mask run with the host generator's flags and the Philox run
    give the same bits."""
    i, keep, _, _, _ = _prepare(case)
    run = _ln_gpu if case["kind"] == "ln" else _silu_gpu
    a, b = run(case, i, keep, cuda), run(case, i, keep, cuda, force_mask=True)
    for n in ("y", "s", "da", "u"):
        if n in a:
            assert torch.equal(a[n], b[n]), n

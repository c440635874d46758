"""The gate-scan kernels (rb_gate_scan_fwd / _bwd, their _bf16 and _last forms)
against an independent fp64 reference (tests/gate_scan_reference.py: a serial
recurrence with autograd), not against one another.

Per output tensor the error is max |got - ref64| / (channel scale) and the bar
M * e32 + 4 * 2^-24, e32 the same error of the reference's own fp32 run on the
same inputs (gate_scan_reference.channel_error / judge).  bf16 storage: inputs
rounded to bf16 first, one bf16 ulp of the reference element allowed on the
bf16 outputs.  The carries are held to y's bar against the reference state
entering each tile; every output is a view into a buffer pre-filled with a
sentinel, which must survive everywhere outside the view.

Value regimes "init" and "wide" (saturated sigmoids, Lambda across softplus'
x > 20 branch): gate_scan_reference.make_inputs.

For the three sums (dlam, dgate_b, a shared dh0) the scale is the sum of the
summands' magnitudes and the yardstick the larger of the sum's and the
summands' e32 (gate_scan_reference.channel_error / judge say why).

M is twice the worst ratio error / max(e32, 4 * 2^-24) measured on an MI355X
over all cases below, rounded up:

    tensor    worst ratio   case                       M
    y         10.68         dense-wide-3x33x6          22
    drg        9.65         dense-wide-3x33x6          20
    dxc        2.68         dense-wide-3x33x6           6
    dz        12.75         dense-wide-3x33x6          26
    dlam       1.43         dense-wide-5x16x36          3
    dgate_b    1.00         dense-init-1x1x4            2
    dh0        3.80         bf16-wide-packed-4seq-H6    8
    y_last     1.08         last-wide-4seq-H6           3
    carries    9.83 of their own e32 (last-wide-11seq-H36); held to y's bar

Everywhere but dense-wide-3x33x6 the ratio of y, drg and dz is 2 or less
(mostly 1.00: the dominant error, alpha's rounding amplified by 1 - alpha^2,
is the same in the kernel and in plain fp32).  y, drg and dz need M > 16 for
that one case, and the cause is the formula's conditioning, not the kernel: a
saturated r gate puts alpha within one ulp of 1 there (min 1 - alpha =
3.7e-8), so 1 - alpha^2 is all rounding error of alpha.  torch's expf rounds
alpha correctly; the hardware exp2 (common.h: fexp) is good to 1 ulp.  Moving
the fp32 reference's alpha by one ulp up or down at random on the CPU gives
ratios of 15, 22, 1.7 and 21 for y in four draws of the same case: the
measured 10.7 is what a 1-ulp exp costs here.  Narrowing Lambda does not
remove it (it is the r gate that saturates, at any Lambda), so the case stays
and the three M follow the measurement.
"""
import pytest
import torch

import gate_scan_reference as G

pytestmark = pytest.mark.gpu

M = {"y": 22, "y_last": 3, "drg": 20, "dxc": 6, "dz": 26, "dlam": 3, "dgate_b": 2, "dh0": 8}

SENTINEL = -4096.0
PAD = 4            # spare channels after each view (keeps every vector width's alignment)
BF = torch.bfloat16

LENS_A = [100, 49, 33, 32, 17, 16, 16, 15, 3, 2, 1]   # odd count: the pairing wave's middle
LENS_B = [17, 16, 2, 1]


def _case(id, regime, B=None, L=None, H=None, lengths=None, h0="rows", gate_b=True,
          layout="halves", dtype=torch.float32, last_only=False):
    if lengths is not None:
        B, L = len(lengths), max(lengths)
    return pytest.param(dict(regime=regime, B=B, L=L, H=H, lengths=lengths, h0=h0, gate_b=gate_b,
                             layout=layout, dtype=dtype, last_only=last_only), id=id)


def _cases():
    out = []
    # 1. dense fp32: every B in {1, 3, 5}, L in {1, 2, 15, 16, 17, 33, 100}, H in {4, 5, 6, 20,
    #    32, 36, 96}; H = 5 -> 1 channel per lane, 6 -> 2, else 4 (backward) / 2 (forward)
    for r in ("init", "wide"):
        for B, L, H in ((5, 100, 96), (1, 1, 4), (3, 17, 5), (3, 33, 6), (5, 16, 36), (1, 2, 20),
                        (3, 15, 32)):
            out.append(_case(f"dense-{r}-{B}x{L}x{H}", r, B, L, H))
    # 2. xc and z contiguous tensors instead of the halves of one [B, L, 2H] buffer,
    #    outputs allocated by the wrapper
    for r in ("init", "wide"):
        out.append(_case(f"contiguous-{r}-5x16x36", r, 5, 16, 36, layout="contiguous"))
    # 3. h0 absent / shared / per row, with and without the gates bias, on the 2- and 1-channel paths
    for r, (B, L, H) in (("init", (3, 33, 6)), ("wide", (3, 17, 5))):
        for h0 in (None, "shared", "rows"):
            for gb in (True, False):
                if (h0, gb) != ("rows", True):      # that one is case 1
                    out.append(_case(f"h0-{r}-{B}x{L}x{H}-{h0}-{'bias' if gb else 'nobias'}", r,
                                     B, L, H, h0=h0, gate_b=gb))
    # 4. packed fp32, sorted longest first   5. last_only with a batch_row permutation
    for r in ("init", "wide"):
        for lens, H in ((LENS_A, 36), (LENS_B, 6), (LENS_B, 5)):
            out.append(_case(f"packed-{r}-{len(lens)}seq-H{H}", r, lengths=lens, H=H))
            if H != 5:
                out.append(_case(f"last-{r}-{len(lens)}seq-H{H}", r, lengths=lens, H=H,
                                 last_only=True))
    # 6. bf16 storage: the 4-wide two-pass backward (H % 4 == 0) and its 2-wide fallback (H = 6)
    for r in ("init", "wide"):
        out.append(_case(f"bf16-{r}-3x33x36", r, 3, 33, 36, dtype=BF))
        out.append(_case(f"bf16-{r}-2x100x64", r, 2, 100, 64, dtype=BF))
        out.append(_case(f"bf16-{r}-packed-11seq-H64", r, lengths=LENS_A, H=64, dtype=BF))
        out.append(_case(f"bf16-{r}-packed-4seq-H6", r, lengths=LENS_B, H=6, dtype=BF))
    return out


CASES = _cases()


def _guarded(rows, width, dtype, dev):
    """[rows, width] view in the middle of a sentinel-filled [rows + 2, width + PAD] buffer."""
    buf = torch.full((rows + 2, width + PAD), SENTINEL, device=dev, dtype=dtype)
    return buf, buf[1:rows + 1, :width]


def _untouched(buf, rows, width):
    return bool((buf[0] == SENTINEL).all() and (buf[rows + 1] == SENTINEL).all()
                and (buf[:, width:] == SENTINEL).all())


def _prepare(c):
    """Inputs and the two reference runs of a case (CPU)."""
    B, L, H = c["B"], c["L"], c["H"]
    seed = 1000 * B + 10 * L + H
    i = G.make_inputs(c["regime"], B, L, H, seed, h0=c["h0"], gate_b=c["gate_b"])
    if c["dtype"] == BF:
        for n in ("rg", "xc", "z", "dy"):
            setattr(i, n, getattr(i, n).to(BF).float())
    lens = c["lengths"]
    lens_t = torch.tensor(lens if lens is not None else [L] * B)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(seed)) if c["last_only"] else None
    dy_ref = i.dy
    if c["last_only"]:      # dy only at each sequence's last position
        dy_ref = torch.zeros_like(i.dy)
        dy_ref[torch.arange(B), lens_t - 1] = i.dy[torch.arange(B), lens_t - 1]
    args = (i.rg, i.xc, i.z, i.lam, i.gate_b, i.h0, dy_ref, lens)
    return i, lens_t, perm, G.reference(*args), G.reference(*args, dtype=torch.float32)


def yardsticks(c):
    """{tensor: e32} of a case: what plain fp32 makes of its inputs (no GPU)."""
    _, _, _, r64, r32 = _prepare(c)
    names = G.TENSORS + ("y_last",)
    return {n: (v[2] - G.FLOOR) / 16 for n, v in G.judge_all(r32, r64, r32, 16, names=names).items()}


def run_case(c, dev):
    """Runs one case on the GPU: {tensor: (passes, error, bar, ratio)} plus
    "carries" judged on y's bar and "guard" (the sentinels survived)."""
    from datamining_recblr_amd import kernels

    B, L, H, dt = c["B"], c["L"], c["H"], c["dtype"]
    bf = dt == BF
    lens = c["lengths"]
    packed = lens is not None
    i, lens_t, perm, r64, r32 = _prepare(c)

    # ---- operands in the kernels' layout
    valid = torch.arange(L)[None, :] < lens_t[:, None]
    rows = int(lens_t.sum())

    def flat(t):            # [B, L, C] -> the live rows [rows, C] (dense: all of them)
        return t[valid]

    def shaped(t):          # [rows, C] -> what the kernels take
        return t if packed else t.view(B, L, -1)

    to = dict(device=dev, dtype=dt)
    rg = shaped(flat(i.rg).to(**to))
    if c["layout"] == "halves":     # as the model passes them: row stride 2H
        xz = torch.cat([flat(i.xc), flat(i.z)], 1).to(**to)
        xc, z = shaped(xz)[..., :H], shaped(xz)[..., H:]
    else:
        xc, z = shaped(flat(i.xc).to(**to).contiguous()), shaped(flat(i.z).to(**to).contiguous())
    lam = i.lam.to(dev)
    gb = None if i.gate_b is None else i.gate_b.to(dev)
    h0 = None if i.h0 is None else i.h0.to(dev)
    seq = None
    if packed:
        offs = torch.zeros(B + 1, dtype=torch.int64)
        offs[1:] = lens_t.cumsum(0)
        seq = kernels.Packed(offs.to(dev), L, rows)
    kw = dict(gate_b=gb, seq=seq)
    guards = []

    def out_view(width):
        if c["layout"] != "halves":
            return None
        buf, v = _guarded(rows, width, dt, dev)
        guards.append((buf, width))
        return v

    # ---- forward
    got = {}
    if c["last_only"]:
        pd = perm.to(dev)
        yl, car = kernels.gate_scan_fwd(rg, xc, z, lam, h0, last_only=True, batch_row=pd, **kw)
        got["y_last"] = yl.index_select(0, pd)
        dy = torch.empty(B, H, device=dev)
        dy[pd] = i.dy[torch.arange(B), lens_t - 1].to(dev)
    else:
        yv = out_view(H)
        y, car = kernels.gate_scan_fwd(rg, xc, z, lam, h0, y=None if yv is None else shaped(yv),
                                       **kw)
        got["y"] = y
        dy = shaped(flat(i.dy).to(**to).contiguous())
        pd = None

    # ---- backward: dxc and dz as the halves of one buffer, drg in its own
    if c["layout"] == "halves":
        both = out_view(2 * H)
        dxc, dz, drg = shaped(both)[..., :H], shaped(both)[..., H:], shaped(out_view(2 * H))
    else:
        dxc, drg, dz = None, None, torch.empty_like(z)
    res = kernels.gate_scan_bwd(rg, xc, z, lam, car, dy, dz, drg, dxc, dh0_rows=c["h0"] == "rows",
                                last_only=c["last_only"], batch_row=pd, **kw)
    torch.cuda.synchronize()
    got.update(drg=res[0], dxc=res[1], dz=dz, dlam=res[2], dgate_b=res[3], dh0=res[4])

    out = {}
    names = [n for n in got]
    for n in names:
        ref = getattr(r64, n)
        g = got[n].float().cpu()
        if ref.dim() == 3:  # back to [B, L, C]; positions past a sequence's end do not exist
            full = ref.clone().float()
            full[valid] = g.reshape(rows, -1)
            g = full
        got[n] = g
    out.update(G.judge_all(got, r64, r32, M, bf16=bf, names=names))

    # ---- carries: the reference state entering each tile the sequence reaches, on y's bar
    nT = car.shape[1]
    reached = torch.arange(nT)[None, :] < ((lens_t + G.TILE - 1) // G.TILE)[:, None]
    cg = torch.where(reached[..., None], car.cpu().double(), r64.tile_h)
    ybar = G.bar(G.channel_error(r32.y, r64.y), M["y"])
    cerr = G.channel_error(cg, r64.tile_h)
    e32c = G.channel_error(r32.tile_h, r64.tile_h)
    out["carries"] = (cerr <= ybar, cerr, ybar, cerr / max(e32c, G.FLOOR))
    out["guard"] = (all(_untouched(b, rows, w) for b, w in guards), 0.0, 0.0, 0.0)
    return out


@pytest.mark.parametrize("case", CASES)
def test_gate_scan_vs_fp64_reference(cuda, case):
    res = run_case(case, cuda)
    for n, (ok, err, limit, ratio) in res.items():
        print(f"{n:8s} err {err:.3e}  bar {limit:.3e}  ratio {ratio:.2f}")
    bad = {n: v for n, v in res.items() if not v[0]}
    assert not bad, bad

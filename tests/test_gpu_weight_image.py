"""The f16 weight image (rb_gemm_h_split_weights) against its documented
layout (csrc/common.h, "the f16 weight image"), decoded on the host from the
formulas alone:

  exponents  int32 e_c at byte C * R * 4: frexp exponent of max_r |Bm[c, r]|
             (0 for an all-zero column)
  32-column planes at byte 0: 16-B slot ((cb * (R / 16) + kb) * 2 + p) * 64 + lane
             = plane p of Bm[32 cb + lane % 32][16 kb + 8 (lane / 32) + 0..7]
  16-column planes at byte C * R * 4 + round_up(4 C, 16):
             slot ((cb * (R / 32) + ks) * 2 + p) * 64 + lane
             = plane p of Bm[16 cb + lane % 16][32 ks + 8 (lane / 16) + 0..7]
  plane 0 = fp16(Bm 2^(14 - e_c)), plane 1 = fp16(Bm 2^(14 - e_c) - plane 0)

The reference is float arithmetic on the CPU: the scale is a power of two
(exact in fp32), plane 0 is one RNE rounding to fp16, and the residual of an
fp32 value and its fp16 rounding is exact in fp32, so every stored half is
determined bit for bit."""
import pytest
import torch

from datamining_recblr_amd import kernels

pytestmark = pytest.mark.gpu

SCALE = 14   # kWeightScale


def _decode(planes, C, R, cols, kstep):
    """planes: int16 [C / cols, R / kstep, 2, 64, 8] in slot order -> the two
    [C, R] planes (lane l of a slot: column l % cols, k 8 (l / cols) + 0..7)"""
    nk = kstep // 8
    p = planes.view(C // cols, R // kstep, 2, nk, cols, 8)   # lane = kq * cols + c
    p = p.permute(2, 0, 4, 1, 3, 5).reshape(2, C, R)         # [p][cb, c][kb, kq, j]
    return p[0], p[1]


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("C,R", [(32, 32), (96, 64)])
def test_f16_weight_image_matches_documented_layout(cuda, C, R, transpose):
    g = torch.Generator().manual_seed(1000 * C + R)
    # column magnitudes over 2^-20 .. 2^20 (both ends present), one zero column
    ce = torch.randint(-20, 21, (C,), generator=g)
    ce[0], ce[1] = -20, 20
    bm = torch.randn(C, R, generator=g) * torch.exp2(ce.float())[:, None]
    bm[C // 2] = 0.0
    w = bm.t().contiguous() if transpose else bm
    img = kernels.gemm_h_weight(w.to(cuda), transpose=transpose).cpu()
    raw = img.view(torch.int16)

    # expected: exponents, then the two planes
    e_ref = torch.frexp(bm.abs().amax(1))[1].to(torch.int32)
    assert e_ref[C // 2] == 0
    assert e_ref.unique().numel() > 4
    scaled = torch.ldexp(bm, (SCALE - e_ref)[:, None])
    p0_ref = scaled.to(torch.float16)
    p1_ref = (scaled - p0_ref.float()).to(torch.float16)
    assert p0_ref.isfinite().all() and p0_ref.abs().max() < 2.0 ** SCALE

    e = img.view(torch.int32)[C * R:C * R + C]
    assert torch.equal(e, e_ref)

    n = C * R * 2                                            # halfs per layout
    a0, a1 = _decode(raw[:n], C, R, 32, 16)
    off = (C * R * 4 + (C * 4 + 15) // 16 * 16) // 2         # ws_image_offset, in halfs
    b0, b1 = _decode(raw[off:off + n], C, R, 16, 32)
    assert raw.numel() == off + n
    for q0, q1 in ((a0, a1), (b0, b1)):
        assert torch.equal(q0, p0_ref.view(torch.int16))
        assert torch.equal(q1, p1_ref.view(torch.int16))
    assert torch.equal(a0, b0) and torch.equal(a1, b1)

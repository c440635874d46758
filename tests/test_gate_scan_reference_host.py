"""The gate-scan reference (tests/gate_scan_reference.py) and its bar, checked
on the CPU before the GPU tests rely on them.

1. The reference agrees with the oracle's GatedRecurrentLayer (grl_forward,
   pinned to the reference implementation by test_oracle_golden.py) through a
   layer whose in- and out-projections are identities.
2. The bar can fail: five planted errors are each rejected at M = 16.
3. The yardstick e32 (fp32 run of the reference against its fp64 run, per
   channel) stays under 1e-4 in both value regimes, so the bar M * e32 + floor
   never exceeds about 2e-3.  At B=5, L=37, H=24, lengths 37/20/16/5/1, per-row
   h0, seed 3:

       tensor    init      wide
       y         2.5e-06   1.1e-05
       drg       3.7e-05   4.9e-05
       dxc       3.3e-05   9.9e-06
       dz        3.2e-06   8.6e-06
       dlam      8.7e-06   2.1e-06
       dgate_b   1.2e-05   8.2e-06
       dh0       5.1e-07   8.5e-07

   "wide" starts at Lambda = -3.5, not -7: see WIDE_LAMBDA_MIN.  (Other seeds
   of "init" reach 1.3e-4 in dxc: the figure is a property of the draw's most
   saturated step, which is why the GPU tests compute e32 on their own inputs.)
"""
import pytest
import torch

import gate_scan_reference as G
from oracle import recblr_oracle as orc

B, L, H = 5, 37, 24
LENGTHS = [37, 20, 16, 5, 1]


def _refs(regime, seed=3):
    i = G.make_inputs(regime, B, L, H, seed, h0="rows")
    args = (i.rg, i.xc, i.z, i.lam, i.gate_b, i.h0, i.dy, LENGTHS)
    return i, G.reference(*args), G.reference(*args, dtype=torch.float32)


@pytest.fixture(scope="module", params=["init", "wide"])
def refs(request):
    return request.param, *_refs(request.param)


def test_reference_equals_oracle_layer():
    """x = [u | z] through W_in = I, no conv, W_out = [I; 0]: the oracle layer
    then computes exactly the gate scan of (rg = u W_g^T, xc = u, z) with
    gate_b = b_g and no h0.  L is a power of two, so the oracle pads nothing.
    Forward and every gradient, fp32 against fp32."""
    Bo, Lo, Ho = 3, 32, 12
    g = torch.Generator().manual_seed(0)
    x = torch.randn(Bo, Lo, 2 * Ho, generator=g)
    gy = torch.randn(Bo, Lo, Ho, generator=g)
    W_g = torch.randn(2 * Ho, Ho, generator=g) * 0.5
    p = {"input.weight": torch.eye(2 * Ho), "conv1d.weight": torch.zeros(Ho, 1, 4),
         "conv1d.bias": torch.zeros(Ho), "gates.weight": W_g,
         "gates.bias": 0.3 * torch.randn(2 * Ho, generator=g),
         "Lambda": torch.linspace(-6.9, 3.0, Ho),
         "output.weight": torch.cat([torch.eye(Ho), torch.zeros(Ho, Ho)])}
    p = {k: v.clone().requires_grad_() for k, v in p.items()}
    xo = x.clone().requires_grad_()
    yo = orc.grl_forward(p, "", xo, disable_conv1d=True)[..., :Ho]
    (yo * gy).sum().backward()

    u, z = x[..., :Ho], x[..., Ho:]
    r = G.reference(u @ W_g.t(), u, z, p["Lambda"].detach(), p["gates.bias"].detach(), None, gy,
                    dtype=torch.float32)
    tol = dict(rtol=1e-5, atol=2e-6)
    torch.testing.assert_close(r.y, yo.detach(), **tol)
    torch.testing.assert_close(r.dz, xo.grad[..., Ho:], **tol)
    torch.testing.assert_close(r.dxc + r.drg @ W_g, xo.grad[..., :Ho], rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(r.dlam, p["Lambda"].grad, rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(r.dgate_b, p["gates.bias"].grad, rtol=1e-4, atol=2e-5)
    # the tile states are h itself: y / silu(z) at t = 15
    torch.testing.assert_close(r.tile_h[:, 1] * torch.nn.functional.silu(z[:, 15]), r.y[:, 15])
    assert r.tile_h[:, 0].abs().max() == 0 and r.y_last.equal(r.y[:, -1])


def test_yardstick_is_small(refs):
    regime, _, r64, r32 = refs
    res = G.judge_all(r32, r64, r32, 16)
    e32 = {n: v[1] for n, v in res.items()}
    print(regime, {n: f"{e:.1e}" for n, e in e32.items()})
    for n, e in e32.items():
        assert 0 < e < 1e-4, (regime, n, e)
        assert res[n][2] < 2e-3, (regime, n, res[n][2])
    assert G.channel_error(r32.tile_h, r64.tile_h) < 1e-4


def _copy(r32):
    return {n: getattr(r32, n).clone() for n in G.TENSORS}


def _plant_drg(got, r64, r32, inp):
    """(a) one drg element (the largest) changed by a relative 1e-3"""
    k = r64.drg.abs().argmax()
    got["drg"].view(-1)[k] *= 1 + 1e-3
    return "drg"


def _plant_dlam(got, r64, r32, inp):
    """(b) dlam without the softplus derivative"""
    got["dlam"] = r32.dlam / torch.sigmoid(inp.lam)
    return "dlam"


def _plant_dh0(got, r64, r32, inp):
    """(c) dh0 of one row zeroed"""
    got["dh0"][2] = 0
    return "dh0"


def _plant_dz(got, r64, r32, inp):
    """(d) the last time step of dz of the shortest sequence zeroed"""
    s = min(range(B), key=lambda b: LENGTHS[b])
    got["dz"][s, LENGTHS[s] - 1] = 0
    return "dz"


def _plant_y(got, r64, r32, inp):
    """(e) y shifted by one position in one sequence"""
    got["y"][1] = torch.roll(got["y"][1], 1, 0)
    return "y"


@pytest.mark.parametrize("plant", [_plant_drg, _plant_dlam, _plant_dh0, _plant_dz, _plant_y],
                         ids=["drg_1e-3", "dlam_no_dsoftplus", "dh0_row_zero", "dz_tail_zero",
                              "y_shifted"])
def test_bar_rejects_planted_error(refs, plant):
    regime, inp, r64, r32 = refs
    got = _copy(r32)
    clean = G.judge_all(got, r64, r32, 16)
    assert all(v[0] for v in clean.values()), clean      # the unperturbed fp32 run passes
    name = plant(got, r64, r32, inp)
    res = G.judge_all(got, r64, r32, 16)
    ok, err, limit, _ = res[name]
    assert not ok, (regime, name, err, limit)
    assert all(v[0] for n, v in res.items() if n != name)

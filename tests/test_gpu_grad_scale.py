"""Whole-model gradients judged at each parameter's own scale.

test_gpu_parity's golden comparison carries an absolute 1e-4, and at the
initial parameter values most recurrence gradients (Lambda, conv1d, gates) lie
below it: zeros would pass.  Here the parameters are moved off their initial
values (test_gpu_session._model) so that no gradient is vanishingly small
(asserted: every max|ref| >= 1e-4), and each one is compared with the CPU
oracle in float64 relative to its own maximum:

    max|got - ref64| / max|ref64|  <=  M_MODEL * max(e32, 2^-22)

e32 being the same figure for the oracle's own fp32 run.  RecBLR at
hidden_size 64, 2 layers, d_conv 4, L = 20, B = 6 with lengths 20, 13, 7, 2, 1,
20, 200 items, no dropout; CE, BPR and the three flag variants.

M_MODEL is twice the worst ratio error / max(e32, 2^-22) measured on an
MI355X, rounded up (up to 32 is expected with the f16x3 GEMMs in between):

    worst ratio per kind of parameter over the five variants: input.weight
    1.90 (BPR), gates.bias 1.69, layer_norm.weight 1.66, Lambda 1.60,
    output.weight 1.59 (all bd_lru_only), conv1d.bias 1.49 (BPR),
    item_embedding.weight 1.36 (BPR), gates.weight 1.32 (disable_conv1d),
    conv1d.weight 1.28 (CE), w_2.weight 1.19, w_1.weight 1.08; every e32 is
    5e-6 or less, every max|ref64| 3e-4 or more.
"""
import pytest

import model_grad_reference as R
from test_gpu_session import V

pytestmark = pytest.mark.gpu

M_MODEL = 4
FLOOR = 2.0 ** -22
L, LENGTHS = 20, [20, 13, 7, 2, 1, 20]

VARIANTS = [dict(), dict(loss_type="BPR"), dict(disable_conv1d=True), dict(disable_ffn=True),
            dict(bd_lru_only=True)]


def run_variant(dev, flags):
    """{parameter: (error, e32, ratio, max|ref64|)}; parameters the variant
    does not use (no oracle gradient) must have none on the GPU either
    (model_grad_reference.judge)."""
    flags = dict(flags)
    loss_type = flags.pop("loss_type", "CE")
    case = R.make_case(flags, 64, V, L, LENGTHS, loss_type)
    return R.run_case(case, dev, floor=FLOOR)[0]


@pytest.mark.parametrize("flags", VARIANTS, ids=["CE", "BPR", "disable_conv1d", "disable_ffn", "bd_lru_only"])
def test_every_gradient_at_its_own_scale(cuda, flags):
    res = run_variant(cuda, flags)
    assert any("Lambda" in n for n in res) and any("gates.weight" in n for n in res)
    bad = {}
    for name, (err, e32, ratio, scale) in res.items():
        print(f"{name:60s} max|ref| {scale:.2e}  err {err:.2e}  e32 {e32:.2e}  ratio {ratio:.2f}")
        assert scale >= 1e-4, f"{name}: max|ref64| {scale:.2e} is back under the absolute bar"
        if not err <= M_MODEL * max(e32, FLOOR):
            bad[name] = (err, e32, ratio)
    assert not bad, bad

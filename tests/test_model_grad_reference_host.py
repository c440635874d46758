"""The whole-model gradient reference (tests/model_grad_reference.py) and its
judgement, checked on the CPU before the GPU tests rely on them.

The model itself runs only on the GPU, so here a second float32 run of the
oracle stands in for the device: the same step on the batch in reverse row
order, whose sums over the batch associate differently — an honest fp32 run
that is not the yardstick's own (ratios 0.4 to 1.3 at this shape).  Reduced
shape: B = 8, L = 12, d = 32, 200 items, weights at the init's scale.

1. The unmodified stand-in passes err <= M_MODEL * max(e32, FLOOR).
2. Three planted faults in gradients below 1e-4 — a tensor zeroed, a tensor
   scaled by 1 + 2^-10, one element's sign flipped — are each flagged by that
   judgement and each pass test_gpu_e2e.close: the gap the own-scale tests close.
3. The two oracle runs are made once per Case and shared.
4. A BPR item row that no sequence or target touches must be exactly zero.
5. At the GPU tests' full shape (test_gpu_grad_scale_routes) the reference
   alone satisfies their validity conditions: every e32 <= 1e-4, every
   max|ref64| > 1e-12, at least one max|ref64| < 1e-4 per loss.
6. build_model restates test_gpu_session._model's parameters bit for bit.
"""
import pytest
import torch

import model_grad_reference as R
import test_gpu_grad_scale_routes as routes
from test_gpu_e2e import close
from test_gpu_grad_scale import FLOOR, M_MODEL

LENGTHS = [12, 9, 5, 2, 1, 12, 7, 3]


def _case(loss_type="CE"):
    return R.make_case({}, 32, 200, 12, LENGTHS, loss_type, 0.1, 1.0)


def _stand_in(case):
    """(loss, gradients) of the fp32 oracle on the reversed batch."""
    ref = R.reference(case)
    loss, grads = R.oracle_grads(ref.state, ref.cfg, *(t.flip(0) for t in ref.inputs),
                                 torch.float32)
    return loss, {k: None if g is None else g.clone() for k, g in grads.items()}


def _flagged(res):
    return {n for n, (err, e32, _, _) in res.items() if not err <= M_MODEL * max(e32, FLOOR)}


def _passes_close(case, grads):
    g64 = R.reference(case).g64
    for n, g in grads.items():
        close(g, g64[n], what=n)   # raises where the 1e-4 bar sees a difference


@pytest.mark.parametrize("loss_type", ["CE", "BPR"])
def test_unmodified_run_passes(loss_type):
    case = _case(loss_type)
    loss, grads = _stand_in(case)
    res, (lerr, le32) = R.judge(case, loss, grads, floor=FLOOR)
    print(R.table(res, (lerr, le32)))
    assert len(res) == 33 and not _flagged(res), _flagged(res)
    assert lerr <= M_MODEL * max(le32, FLOOR)
    assert all(ratio == err / max(e32, FLOOR) for err, e32, ratio, _ in res.values())
    _passes_close(case, grads)


def _zero(g):
    g.zero_()


def _scale(g):
    g.mul_(1 + 2.0 ** -10)


def _flip_sign(g):
    k = g.abs().argmax()
    g.view(-1)[k] = -g.view(-1)[k]


@pytest.mark.parametrize("plant,name", [
    (_zero, "recurrent_layers.0.behavior_modeling.gates.bias"),
    (_zero, "recurrent_layers.1.behavior_modeling.conv1d.bias"),
    (_scale, "recurrent_layers.0.behavior_modeling.gates.weight"),
    (_scale, "recurrent_layers.1.behavior_modeling.conv1d.weight"),
    (_flip_sign, "recurrent_layers.1.behavior_modeling.Lambda"),
    (_flip_sign, "recurrent_layers.0.behavior_modeling.gates.weight"),
], ids=lambda v: v.__name__.strip("_") if callable(v) else v.split(".", 1)[1])
def test_planted_fault_is_flagged_here_and_passes_close(plant, name):
    case = _case()
    loss, grads = _stand_in(case)
    scale = R.reference(case).g64[name].abs().max().item()
    # where an absolute 1e-4 is blind (a flipped sign is off by twice the value)
    assert 1e-12 < scale < (5e-5 if plant is _flip_sign else 1e-4), (name, scale)
    plant(grads[name])
    res, _ = R.judge(case, loss, grads, floor=FLOOR)
    assert _flagged(res) == {name}, (res[name], _flagged(res))
    _passes_close(case, grads)


def test_oracle_runs_once_per_case():
    case = _case()
    ref = R.reference(case)
    n = R.oracle_runs[0]
    again = R.reference(_case())            # an equal Case, built anew
    assert again is ref and R.oracle_runs[0] == n
    assert all(again.g64[k] is ref.g64[k] and again.g32[k] is ref.g32[k] for k in ref.g64)
    loss, grads = _stand_in(case)
    R.judge(case, loss, grads)              # judging pays for no oracle run
    R.yardstick(case)
    assert R.oracle_runs[0] == n
    before = {k: v.clone() for k, v in ref.g64.items()}
    R.judge(case, loss, grads)
    assert all(torch.equal(before[k], ref.g64[k]) for k in before)   # and leaves it unchanged
    new = _case("BPR") not in R._cache
    other = R.reference(_case("BPR"))       # another input case: its own two runs
    assert other is not ref and R.oracle_runs[0] == n + 2 * new
    assert R.make_case({"disable_ffn": True}) != R.make_case({})


def test_bpr_rows_no_sequence_touches_must_be_exactly_zero():
    case = _case("BPR")
    ref = R.reference(case)
    seq, _, pos, neg = ref.inputs
    g64 = ref.g64["item_embedding.weight"]
    untouched = g64.abs().amax(1) == 0
    used = torch.zeros(case.n_items, dtype=torch.bool)
    used[torch.cat([seq[seq > 0], pos, neg])] = True
    assert torch.equal(untouched, ~used) and untouched[0] and 100 < untouched.sum() < 200
    loss, grads = _stand_in(case)
    R.judge(case, loss, grads)                       # the clean run holds the rule
    row = int(untouched.nonzero()[7])
    grads["item_embedding.weight"][row, 3] = 1e-30   # far under any tolerance
    with pytest.raises(AssertionError, match="item_embedding.weight"):
        R.judge(case, loss, grads)


def test_parameters_without_an_oracle_gradient_must_have_none():
    case = R.make_case({"disable_ffn": True}, 32, 200, 12, LENGTHS, "CE", 0.1, 1.0)
    ref = R.reference(case)
    unused = [k for k, g in ref.g64.items() if g is None]
    assert unused and all(".ffn." in k for k in unused)
    loss, grads = _stand_in(case)
    res, _ = R.judge(case, loss, grads)
    assert not set(unused) & set(res) and not _flagged(res)
    grads[unused[0]] = torch.zeros_like(ref.state[unused[0]])    # all-zero: allowed
    R.judge(case, loss, grads)
    grads[unused[0]][0] = 1e-20
    with pytest.raises(AssertionError):
        R.judge(case, loss, grads)
    grads[unused[0]] = None
    used = next(k for k, g in ref.g64.items() if g is not None)
    grads[used] = None                                           # a missing gradient
    with pytest.raises(AssertionError, match="no gradient"):
        R.judge(case, loss, grads)


@pytest.mark.parametrize("loss_type", ["CE", "BPR"])
def test_full_gpu_shape_reference_is_valid(loss_type):
    """The validity conditions of test_gpu_grad_scale_routes, on its own Case:
    facts of the oracle alone."""
    from datamining_recblr_amd import linear

    assert routes.NTOK == 19350 >= linear.MIN_ROWS_FOR_SPLIT
    case = routes.route_case(loss_type)
    per, loss_e32 = R.yardstick(case)
    for name, (e32, scale) in per.items():
        print(f"{name:60s} max|ref| {scale:.2e}  e32 {e32:.2e}")
    print(f"loss e32 {loss_e32:.2e}")
    assert len(per) == 33 and loss_e32 <= 1e-4
    assert max(e for e, _ in per.values()) <= 1e-4
    assert min(s for _, s in per.values()) > 1e-12
    small = routes._assert_reference_is_valid(case)
    assert len(small) >= 1
    print(f"{len(small)} of {len(per)} under 1e-4: {small}")


def test_build_model_restates_the_session_tests_model():
    from datamining_recblr_amd.model import RecBLR
    from datamining_recblr_amd.recbole_compat import SyntheticDataset
    from test_gpu_session import V, _model

    cfg = R.make_cfg(64, 4, 20, 2, disable_conv1d=True)
    torch.manual_seed(0)
    model = RecBLR(cfg, SyntheticDataset(V)).eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("bias") or "layer_norm" in name:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
            elif "Lambda" not in name and "conv1d" not in name:
                p.mul_(3.0)
    got, got_cfg = _model(torch.device("cpu"), 64, 4, 20, 2, disable_conv1d=True)
    assert got_cfg == cfg and not got.training
    want = model.state_dict()
    assert all(torch.equal(v, want[k]) for k, v in got.state_dict().items())
    wide, _ = R.build_model(1003, 128, 4, 50, 2)
    assert wide.item_embedding.weight.shape == (1003, 128)


def test_kind_names():
    assert R.kind("recurrent_layers.1.behavior_modeling.gates.weight") == "gates.weight"
    assert R.kind("recurrent_layers.0.ffn.layer_norm.bias") == "ffn.layer_norm.bias"
    assert R.kind("recurrent_layers.0.layer_norm.bias") == "layer.layer_norm.bias"
    assert R.kind("layer_norm.bias") == "layer_norm.bias"

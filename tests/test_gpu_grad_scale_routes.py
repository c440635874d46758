"""Whole-model gradients at their own scale on the large-batch routes.

test_gpu_grad_scale.py judges every gradient of a training step at its own
scale, but on about 60 packed rows: every GEMM there is the few-rows kernel.
From 16,384 rows (linear.MIN_ROWS_FOR_SPLIT / ACT_MIN_ROWS) a step runs other
kernels — the weight-stationary NT GEMM (csrc/gemm_ws.hip), the fused
activation epilogue and its backward (gemm_nt_h_act / gemm_nt_h_dact), the
LayerNorm epilogue (gemm_nt_h_ln), rb_gemm_tn_h weight gradients scaled by the
rmax side outputs of the GEMMs before them, and the CE backward's P in both
layouts with both products on the f16x3 weight-gradient kernel — and the tests
that see those (test_gpu_e2e, test_gpu_scale, test_gpu_parity) carry an
absolute 1e-4.  Here the same judgement as test_gpu_grad_scale.py,

    max|got - ref64| / max|ref64|  <=  M_MODEL * max(e32, 2^-22)

for every parameter and the loss, at the smallest shape that takes every
large route: d = 128 (the LayerNorm epilogue's N; _f16_grads_ok's d % 128), 2
layers, d_conv 4, no dropout, eval mode, B = 512 (_f16_grads_ok's B % 256),
L = 50, lengths 1, 2, 50 and then 26 + i % 25 (19,350 packed rows), 1003 items
(no multiple of 32 or 256: the partial last tile, item_ce_probs_h_both's
pad_to=256, gmax's last group).  Each case first asserts, with recorders of
its own, that its route ran.

The parameters are moved off their initial values like test_gpu_session._model
does, but with the weights left at the init's scale (gain 1, not 3): at gain 3
every gradient of this shape is 1.8e-4 or more, and the point is to look where
an absolute 1e-4 cannot.  Facts of the reference alone (asserted here and, on
the CPU, in test_model_grad_reference_host.py): every e32 <= 1e-4, every
max|ref64| > 1e-12, at least one max|ref64| < 1e-4 per case.  Measured on the
CPU oracle: CE 9 of 33 parameters under 1e-4 (Lambda, conv1d.weight,
gates.weight, gates.bias of both layers, conv1d.bias of layer 0; the smallest
6.0e-6), e32 from 2.0e-7 to 3.3e-6, the loss 3.8e-8; BPR 10 of 33 under 1e-4
(the smallest 3.6e-6), e32 up to 3.8e-6, the loss 6.6e-8.

e32 per kind of parameter (the larger of the two layers), CE / BPR:
item_embedding.weight 4.3e-7 / 2.4e-7, layer_norm.weight 7.1e-7 / 7.3e-7,
layer_norm.bias 7.0e-7 / 6.9e-7, Lambda 3.1e-6 / 3.3e-6, input.weight 2.8e-6 /
2.5e-6, conv1d.weight 1.6e-6 / 2.8e-6, conv1d.bias 1.7e-6 / 1.5e-6,
gates.weight 1.3e-6 / 1.4e-6, gates.bias 1.2e-6 / 1.3e-6, output.weight 2.0e-6
/ 2.6e-6, the layer's layer_norm.weight 5.5e-7 / 5.7e-7 and .bias 7.4e-7 /
9.3e-7, ffn.w_1.weight 5.1e-7 / 4.9e-7, ffn.w_1.bias 4.6e-7 / 3.8e-7,
ffn.w_2.weight 7.4e-7 / 5.4e-7, ffn.w_2.bias 3.2e-7 / 2.2e-7,
ffn.layer_norm.weight 7.3e-7 / 6.1e-7, ffn.layer_norm.bias 6.1e-7 / 8.7e-7.

Measured on an MI355X, worst ratio err / max(e32, 2^-22) per kind of parameter
(over both layers) and case; M_MODEL = 4 holds everywhere with a factor of two
to spare, so no bar was widened:

    kind                    CE     BPR    CE     CE packed  CE packed
                            packed packed dense  full tail  persistent tiles
    Lambda                  1.81   1.82   1.77   1.79       1.77
    gates.weight            1.66   1.49   1.68   1.66       1.68
    gates.bias              1.58   1.48   1.64   1.60       1.66
    output.weight           1.61   1.34   1.62   1.62       1.62
    input.weight            1.44   1.40   1.43   1.43       1.43
    conv1d.bias             1.40   1.62   1.40   1.40       1.42
    conv1d.weight           1.08   1.40   1.08   1.08       1.08
    ffn.w_1.weight          1.70   1.58   1.41   0.63       1.61
    ffn.w_2.weight          1.19   1.51   1.14   0.53       1.30
    ffn.w_1.bias            0.91   1.21   0.91   0.93       1.04
    ffn.w_2.bias            0.87   1.06   0.91   0.94       0.85
    ffn.layer_norm.weight   0.91   0.87   0.91   0.91       0.95
    ffn.layer_norm.bias     0.76   0.68   0.79   0.66       0.82
    layer.layer_norm.weight 0.66   0.57   0.57   0.66       0.60
    layer.layer_norm.bias   1.04   0.75   0.73   0.85       0.83
    item_embedding.weight   0.60   0.96   0.65   0.60       0.59
    layer_norm.weight       0.31   0.26   0.31   0.26       0.28
    layer_norm.bias         0.38   0.35   0.44   0.35       0.33
    loss: err / e32         3.0e-8 / 3.8e-8 (CE), 1.9e-8 / 1.9e-8 (BPR)
    under 1e-4              9      10     9      9          9    of 33

(ffn.w_1 / w_2.weight drop below 1 with the full tail: layer 1's FFN weight
gradients then run on rb_gemm_tn_h, not on the library GEMM the B gathered
rows take.)  The two planted faults of the last test: the gates' weight
gradient without one row chunk's partial errs by 0.13 and 0.07 of its maximum
(9.6e-6, 1.3e-5), ratio about 1e5; a dbias off by 2^-10 has ratio 2128; both
pass test_gpu_e2e.close.
"""
import pytest

import model_grad_reference as R
from test_gpu_grad_scale import FLOOR, M_MODEL

pytestmark = pytest.mark.gpu

D, B, L, N_ITEMS = 128, 512, 50, 1003
LENGTHS = [1, 2, 50] + [26 + i % 25 for i in range(3, B)]
NTOK = sum(LENGTHS)
BIAS_STD, GAIN = 0.1, 1.0

NT_NAMES = ("gemm_nt_h", "gemm_nt_h_act", "gemm_nt_h_dact", "gemm_nt_h_ln")


def route_case(loss_type="CE"):
    return R.make_case({}, D, N_ITEMS, L, LENGTHS, loss_type, BIAS_STD, GAIN)


@pytest.fixture
def launches(monkeypatch):
    """{kernel wrapper: [its calls]}: (M, R, C) for the four NT GEMM wrappers,
    (M, N, K) for gemm_tn_h, (B, V) for item_ce_probs_h_both."""
    from datamining_recblr_amd import kernels

    calls = {n: [] for n in (*NT_NAMES, "gemm_tn_h", "item_ce_probs_h_both")}
    for name in NT_NAMES:
        def nt(a, wf, C, *args, _orig=getattr(kernels, name), _calls=calls[name], **kw):
            _calls.append((a.shape[0], a.shape[1], C))
            return _orig(a, wf, C, *args, **kw)

        monkeypatch.setattr(kernels, name, nt)
    orig_tn, orig_both = kernels.gemm_tn_h, kernels.item_ce_probs_h_both

    def tn(dy, x, *args, **kw):
        calls["gemm_tn_h"].append((dy.shape[0], dy.shape[1], x.shape[1]))
        return orig_tn(dy, x, *args, **kw)

    def both(seq, items, target, *args, **kw):
        calls["item_ce_probs_h_both"].append((target.shape[0], kw.get("pad_to")))
        return orig_both(seq, items, target, *args, **kw)

    monkeypatch.setattr(kernels, "gemm_tn_h", tn)
    monkeypatch.setattr(kernels, "item_ce_probs_h_both", both)
    return calls


def _assert_route(calls, rows, ce, ws=True, full_tail=False):
    """The large-batch kernels ran on the [rows]-row operands; a fallback to
    torch leaves its recorder short and fails here."""
    from datamining_recblr_amd import recurrence

    print(calls)
    at = {n: [c[1:] for c in v if c[0] == rows] for n, v in calls.items()}
    ffns = 2 if full_tail else 1   # the gathered tail's FFN runs on B rows
    assert at["gemm_nt_h_act"] == [(D, 4 * D)] * ffns, calls["gemm_nt_h_act"]
    assert at["gemm_nt_h_dact"] == [(D, 4 * D)] * ffns, calls["gemm_nt_h_dact"]
    if ws:
        # each full-rows layer: the out-projection and w_2 with the LayerNorm
        assert sorted(at["gemm_nt_h_ln"]) == sorted([(2 * D, D), (4 * D, D)] * ffns), \
            calls["gemm_nt_h_ln"]
    else:
        # ... as plain GEMMs, beside layer 1's in-projection dX (256 -> 128)
        # and the dX GEMMs of w_1 and layer 0's in-projection (512 -> 128)
        assert calls["gemm_nt_h_ln"] == [], calls["gemm_nt_h_ln"]
        assert at["gemm_nt_h"].count((2 * D, D)) == 2, at["gemm_nt_h"]
        assert at["gemm_nt_h"].count((4 * D, D)) == 3, at["gemm_nt_h"]
    # the shapes test_gpu_e2e lists, over the four wrappers as its recorder sees them
    every = [s for n in NT_NAMES for s in at[n]]
    for s in ((128, 512), (256, 128), (512, 128), (128, 256)):
        assert s in every, (s, every)
    assert len(every) >= 12, every
    # ... and the plain ones no epilogue takes: the in-projection, the dX
    # GEMMs of w_1 / the in-projection and of the out-projection, the gates
    plain = [(D, 4 * D), (4 * D, D), (D, 2 * D)]
    if not recurrence._FUSED:
        plain += [(2 * D, 4 * D), (4 * D, 2 * D)]
    for s in plain:
        assert s in at["gemm_nt_h"], (s, at["gemm_nt_h"])
    # weight gradients: layer 0's input, gates, output, w_1, w_2; layer 1's
    # input and gates (+ output, w_1, w_2 with the tail on all rows)
    tn = at["gemm_tn_h"]
    assert len(tn) == (10 if full_tail else 7), calls["gemm_tn_h"]
    for s in ((4 * D, D), (4 * D, 2 * D), (D, 2 * D), (D, 4 * D)):
        assert s in tn, (s, tn)
    if ce:
        assert calls["item_ce_probs_h_both"] == [(B, 256)], calls["item_ce_probs_h_both"]
        # P [B, 1024] x seq and P^T [1003, B] x table
        assert (B, 1024, D) in calls["gemm_tn_h"] and (N_ITEMS, B, D) in calls["gemm_tn_h"], \
            calls["gemm_tn_h"]
    else:
        assert calls["item_ce_probs_h_both"] == []


def _assert_reference_is_valid(case):
    per, loss_e32 = R.yardstick(case)
    assert loss_e32 <= 1e-4, loss_e32
    for name, (e32, scale) in per.items():
        assert e32 <= 1e-4, f"{name}: the yardstick itself is loose, e32 {e32:.2e}"
        assert scale > 1e-12, f"{name}: max|ref64| {scale:.2e}"
    small = [n for n, (_, s) in per.items() if s < 1e-4]
    assert small, "no gradient under 1e-4: close() would see all of this case"
    return small


def _step_and_judge(case, dev, calls, rows, packed=True, gather=True, ws=True):
    small = _assert_reference_is_valid(case)
    loss, grads = R.device_step(case, dev, pack_sequences=packed, gather_last_layer=gather)
    _assert_route(calls, rows, case.loss_type == "CE", ws=ws, full_tail=not gather)
    res, (lerr, le32) = R.judge(case, loss, grads, floor=FLOOR)
    print(R.table(res, (lerr, le32)))
    print(f"{len(small)} of {len(res)} parameters have max|ref64| < 1e-4")
    worst = {}
    for name, (_, _, ratio, _) in res.items():
        worst[R.kind(name)] = max(worst.get(R.kind(name), 0.0), ratio)
    print("worst ratio per kind: " + ", ".join(f"{k} {v:.2f}" for k, v in
                                               sorted(worst.items(), key=lambda kv: -kv[1])))
    bad = {n: v[:3] for n, v in res.items() if not v[0] <= M_MODEL * max(v[1], FLOOR)}
    if not lerr <= M_MODEL * max(le32, FLOOR):
        bad["loss"] = (lerr, le32, lerr / max(le32, FLOOR))
    assert len(res) == 33 and any("Lambda" in n for n in res)
    assert not bad, bad


CASES = {
    "CE_packed": dict(loss_type="CE", packed=True, gather=True),
    "BPR_packed": dict(loss_type="BPR", packed=True, gather=True),
    "CE_dense": dict(loss_type="CE", packed=False, gather=True),
    "CE_packed_full_tail": dict(loss_type="CE", packed=True, gather=False),
}


def test_shape_reaches_the_large_routes():
    from datamining_recblr_amd import linear

    assert NTOK >= linear.MIN_ROWS_FOR_SPLIT and NTOK >= linear.ACT_MIN_ROWS, NTOK
    assert N_ITEMS % 32 and N_ITEMS % 256 and B % 256 == 0 and D % 128 == 0


@pytest.mark.parametrize("name", list(CASES))
def test_every_gradient_at_its_own_scale_on_the_large_routes(cuda, launches, name):
    from datamining_recblr_amd import kernels, linear, scoring

    c = CASES[name]
    assert scoring.CE_PIPE == "f16" and scoring.CE_GRADS == "f16" and linear.rmax_wanted()
    _step_and_judge(route_case(c["loss_type"]), cuda, launches,
                    NTOK if c["packed"] else B * L, c["packed"], c["gather"])
    assert kernels.gemm_nt_h_mode() == 1


def test_every_gradient_at_its_own_scale_on_the_persistent_tiles(cuda, launches):
    """CE packed with linear.set_nt_ws(False): rb_gemm_nt_h's large calls on
    the persistent 256-row tiles, the LayerNorm as a launch of its own."""
    from datamining_recblr_amd import kernels, linear

    prev = linear.set_nt_ws(False)
    try:
        assert kernels.gemm_nt_h_mode() == 0
        _step_and_judge(route_case("CE"), cuda, launches, NTOK, ws=False)
    finally:
        linear.set_nt_ws(prev)
    assert kernels.gemm_nt_h_mode() == int(prev)


def _drop_a_split(kernels, monkeypatch):
    """the gates' weight gradient without its first row chunk's partial (the last
    chunks can be empty: 32-row groups are dealt out whole)"""
    orig = kernels.gemm_tn_h

    def tn(dy, x, *args, **kw):
        parts = orig(dy, x, *args, **kw)
        if (dy.shape[0], dy.shape[1], x.shape[1]) == (NTOK, 4 * D, 2 * D):
            parts[0].zero_()
        return parts

    monkeypatch.setattr(kernels, "gemm_tn_h", tn)
    return {f"recurrent_layers.{i}.behavior_modeling.gates.weight" for i in (0, 1)}


def _scale_dbias(kernels, monkeypatch):
    """gemm_nt_h_dact's dbias off by a relative 2^-10"""
    orig = kernels.gemm_nt_h_dact

    def dact(*args, **kw):
        da, dbias = orig(*args, **kw)
        return da, dbias * (1 + 2.0 ** -10)

    monkeypatch.setattr(kernels, "gemm_nt_h_dact", dact)
    return {"recurrent_layers.0.ffn.w_1.bias"}


@pytest.mark.parametrize("plant", [_drop_a_split, _scale_dbias], ids=["tn_split", "dact_dbias"])
def test_a_small_fault_between_the_kernels_is_flagged_and_passes_close(cuda, launches,
                                                                       monkeypatch, plant):
    """What this file is for, shown on the route itself: a fault planted at a
    kernel wrapper's output (never in a kernel) is flagged by the own-scale
    judgement in exactly the parameters it reaches, while test_gpu_e2e.close
    passes loss and every gradient against the fp32 oracle."""
    from datamining_recblr_amd import kernels
    from test_gpu_e2e import close

    case = route_case("CE")
    expected = plant(kernels, monkeypatch)
    loss, grads = R.device_step(case, cuda, pack_sequences=True, gather_last_layer=True)
    _assert_route(launches, NTOK, True)
    res, (lerr, le32) = R.judge(case, loss, grads, floor=FLOOR)
    print(R.table(res, (lerr, le32)))
    flagged = {n for n, v in res.items() if not v[0] <= M_MODEL * max(v[1], FLOOR)}
    assert flagged == expected, {n: res[n][:3] for n in flagged | expected}
    ref = R.reference(case)
    close(loss, ref.loss32, what="loss")
    for n, g in grads.items():
        close(g, ref.g32[n], what=n)

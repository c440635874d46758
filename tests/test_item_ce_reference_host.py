"""The item cross-entropy reference (tests/item_ce_reference.py) checked on the
host: against torch's own cross_entropy with autograd, that its fp32 run (the
yardstick e32) stays under 1e-4 on every case the GPU tests list, that those
cases reach every loop geometry of the kernels' launch plan, and that the bar
of tests/test_gpu_item_ce_ref.py rejects twelve planted errors.

Planted errors (each applied to the fp32 run of the reference, on the smallest
listed case that can show it) and the tensor that catches each:

     1  the ragged tile's clamped duplicate rows counted into the lse   lse
     2  the last valid item of a ragged tile dropped                    lse
     3  one split's partial omitted from the merge                      lse
     4  partials merged without the exp(m - M) rescale                  lse
     5  one-hot at target + 1 for a target on a tile's last item        P
     6  one-hot missing for a target in the ragged tile                 P
     7  an ignored row given a P of 1 / V instead of 0                  P
     8  inv_n taken over padded rows instead of live rows               loss, P
     9  a second chunk's loss overwriting instead of accumulating       loss
    10  one row's scale exponent off by one                             lse, P
    11  the x0.y1 cross term of the f16 split dropped (~2^-11)          lse
    12  one item row of ditems missing the rows of the last batch tile  ditems
"""
import math

import pytest
import torch
import torch.nn.functional as F

import item_ce_reference as R
import test_gpu_item_ce_ref as TG

E32_MAX = 1e-4
LISTED = tuple(dict.fromkeys(R.ALL_CASES))


def _ignored(c):
    return R.ROWS_IGNORED if c in R.ROWS_CASES else ()


# ---- the reference against torch's cross_entropy -----------------------------------
@pytest.mark.parametrize("c,ignored", [(("random", 5, 7, 16), ()), (("random", 33, 64, 32), (0, 32)),
                                       (("peaked", 130, 97, 64), (5, 129)),
                                       (("large", 130, 97, 128), ()),
                                       (("ties", 130, 97, 128), (31, 32, 33))],
                         ids=lambda v: R.case_id(v) if v and isinstance(v[0], str) else len(v))
def test_reference_matches_torch_cross_entropy(c, ignored):
    inp = R.case_inputs(c, ignored)
    dloss = 0.7
    r = R.reference(inp.seq, inp.table, inp.target, dloss)
    s = inp.seq.double().requires_grad_()
    w = inp.table.double().requires_grad_()
    x = s @ w.t()
    loss = F.cross_entropy(x, inp.target, ignore_index=-1)
    (dloss * loss).backward()

    def rel(a, b):
        return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)

    assert rel(r.lse, torch.logsumexp(x.detach(), 1)) <= 1e-12
    assert abs(float(r.loss) - float(loss.detach())) <= 1e-12 * max(1.0, abs(float(loss.detach())))
    assert rel(r.dseq, s.grad) <= 1e-12 and rel(r.ditems, w.grad) <= 1e-12
    rows = F.cross_entropy(x.detach(), inp.target, ignore_index=-1, reduction="none")
    assert rel(r.loss_rows, rows) <= 1e-12
    if ignored:
        ig = list(ignored)
        assert not r.P[ig].any() and not r.dseq[ig].any() and not r.loss_rows[ig].any()
    assert r.inv_n == 1.0 / (c[1] - len(ignored))


def test_inputs_are_what_they_claim():
    for c in LISTED:
        inp = R.case_inputs(c, _ignored(c))
        regime, B, V, d = c
        live = inp.target[inp.target >= 0]
        assert inp.seq.dtype == torch.float32 and inp.seq.shape == (B, d) and inp.table.shape == (V, d)
        assert int(live.min()) >= 0 and int(live.max()) < V
        if inp.untargeted is not None:
            assert not (inp.target == inp.untargeted).any()
        x = inp.seq.double() @ inp.table.double().t()
        if regime == "large":
            assert 100 <= float(x.max()) <= 150 and -150 <= float(x.min()) <= -100
        if regime == "scaled":
            assert abs(inp.k) >= 23 and float(x.abs().max()) < 40
            if B >= 3 and V >= 3:
                assert not inp.seq[B // 3].any() and not inp.table[V // 3].any()
        if regime == "ties":
            assert len(inp.tied) >= 2 and (inp.table[inp.tied] == inp.table[inp.tied[0]]).all()
            assert any(int(t) in inp.tied for t in live)
        if regime == "peaked":
            p = torch.softmax(x, 1).gather(1, inp.target.clamp_min(0)[:, None])[:, 0]
            assert float(p[inp.target >= 0].min()) > 0.6      # the target dominates every live row
    # the target placements, on a shape that has room for all of them
    tgt = R.case_inputs(("random", 130, 97, 128)).target
    for v in (0, 96, 31, 32):
        assert (tgt == v).any(), v
    assert int(tgt.bincount().max()) >= 30          # one target in many rows
    assert {int(t) for t in R.case_inputs(("random", 600, 4100, 128)).target} >= {0, 4099, 31, 32, 4096}


# ---- the yardstick -----------------------------------------------------------------
@pytest.mark.parametrize("c", LISTED, ids=R.case_id)
def test_fp32_run_within_1e_4(c):
    """e32 of every judged tensor of every listed case (the peaked regime's
    margin range is narrowed until this holds: item_ce_reference.PEAKED_MARGIN_MAX)."""
    r64, r32 = R.both(R.case_inputs(c, _ignored(c)), dloss=0.7)
    e = R.e32_all(r64, r32)
    print(R.case_id(c), " ".join(f"{n}={v:.2e}" for n, v in e.items()))
    for n, v in e.items():
        assert v <= E32_MAX, (n, v)


# ---- the launch plan ---------------------------------------------------------------
def test_plan_restated():
    """The figures worked out by hand from item_scores.hip's plan()."""
    assert R.plan(300, 10544) == (3, 165, 2, 330)
    assert R.plan(2048, 10544) == (16, 30, 11, 330)
    assert R.plan(128, 16384) == (1, 512, 1, 512)
    assert R.plan(1100, 5000) == (9, 53, 3, 157) and R.last_split_tiles(R.plan(1100, 5000)) == 1
    assert R.plan(5000, 1100) == (40, 12, 3, 35) and R.last_split_tiles(R.plan(5000, 1100)) == 2
    assert R.plan(600, 4100) == (5, 65, 2, 129) and R.last_split_tiles(R.plan(600, 4100)) == 1
    assert R.plan(2049, 3900) == (17, 31, 4, 122) and R.last_split_tiles(R.plan(2049, 3900)) == 2
    assert R.plan(2049, 4003) == (17, 26, 5, 126) and R.last_split_tiles(R.plan(2049, 4003)) == 1
    assert R.plan(1, 1) == (1, 1, 1, 1)


@pytest.mark.parametrize("which", ["rows_fixed", "items_fixed"])
def test_listed_cases_reach_every_geometry(which):
    """Together the cases of the GPU tests run, in the kernels that keep the
    sequence rows fixed and in k_ce_bwd_item (item rows fixed): every kind of
    `per`, a short last split, idle placements, a partial and an idle wave."""
    shapes = sorted({(B, V) for _, B, V, _ in R.CASES})
    if which == "rows_fixed":
        plans = {s: R.plan_rows_fixed(*s) for s in shapes}
        fixed = {s: s[0] for s in shapes}
    else:
        plans = {s: R.plan_items_fixed(*s) for s in shapes}
        fixed = {s: s[1] for s in shapes}
    pers = {p[2] for p in plans.values()}
    assert {1, 2, 3} <= pers
    assert any(p >= 4 and p % 2 == 0 for p in pers) and any(p >= 5 and p % 2 == 1 for p in pers)
    assert any(p[2] >= 2 and R.last_split_tiles(p) < p[2] for p in plans.values())
    assert any(p[1] % 8 != 0 and p[0] > 1 for p in plans.values())
    assert any(fixed[s] % 32 != 0 for s in shapes)
    assert any(R.idle_last_wave(fixed[s]) for s in shapes)
    assert any(B % 32 != 0 for B, _ in shapes) and any(V % 32 != 0 for _, V in shapes)
    assert any(V < 32 for _, V in shapes)
    # d: every width on a ragged case, 128 and 64 on every shape
    for d in (16, 32, 64, 128, 256):
        assert any(dd == d and V % 32 != 0 for _, _, V, dd in R.CASES), d
    for s in shapes:
        assert {d for _, B, V, d in R.CASES if (B, V) == s} >= {64, 128}, s
    assert max(B * V for B, V in shapes) <= 8.3e6


# ---- planted errors ----------------------------------------------------------------
def _split_h(x):
    """(x0, x1, e): the f16 pipe's two-part rows, x = 2^(e - 14) (x0 + x1)."""
    m = x.abs().amax(1)
    e = torch.where(m > 0, torch.frexp(m).exponent, torch.zeros((), dtype=torch.int32)).to(torch.int32)
    sv = torch.ldexp(x, (14 - e)[:, None])
    x0 = sv.half().float()
    return x0, (sv - x0).half().float(), e


def _planted(n):
    """(got: the fp32 run with error n planted, r64, r32, the tensors that must fail)."""
    small, mid = ("random", 5, 7, 64), ("random", 33, 64, 64)
    c, ignored = {3: (mid, ()), 4: (mid, ()), 5: (mid, ()), 12: (mid, ()),
                  7: (small, (1,)), 8: (small, (1,))}.get(n, (small, ()))
    inp = R.case_inputs(c, ignored)
    B, V = c[1], c[2]
    dloss = 0.7
    r64, r32 = R.both(inp, dloss)
    f32 = torch.float32
    x = R.logits(inp.seq, inp.table, f32)

    def fin(x=x, lse=None, **kw):
        return R.finish(inp.seq, inp.table, inp.target, x, R.log_sum_exp(x) if lse is None else lse,
                        dloss, **kw)

    if n == 1:
        dup = x[:, V - 1:].expand(-1, R.TILE - V % R.TILE)
        bad, fails = fin(lse=R.log_sum_exp(torch.cat([x, dup], 1))), ("lse",)
    elif n == 2:
        bad, fails = fin(lse=R.log_sum_exp(x[:, :V - 1])), ("lse",)
    elif n == 3:
        assert R.plan_rows_fixed(B, V)[1] == 2
        bad, fails = fin(lse=R.log_sum_exp(x[:, :R.TILE])), ("lse",)
    elif n == 4:
        m1, m2 = x[:, :R.TILE].amax(1), x[:, R.TILE:].amax(1)
        s1 = torch.exp(x[:, :R.TILE] - m1[:, None]).sum(1)
        s2 = torch.exp(x[:, R.TILE:] - m2[:, None]).sum(1)
        bad, fails = fin(lse=torch.maximum(m1, m2) + torch.log(s1 + s2)), ("lse",)
    elif n == 5:
        t = inp.target.clone()
        hit = (t % R.TILE == R.TILE - 1) & (t + 1 < V)
        assert hit.any()
        t[hit] += 1
        bad, fails = fin(onehot=R.one_hot(t, V, f32)), ("P",)
    elif n == 6:
        t = inp.target.clone()
        hit = t >= V // R.TILE * R.TILE
        assert V % R.TILE and hit.any()
        t[hit] = -1
        bad, fails = fin(onehot=R.one_hot(t, V, f32)), ("P",)
    elif n == 7:
        bad, fails = fin(), ("P",)
        bad.P[list(ignored)] = bad.g / V
    elif n == 8:
        bad, fails = fin(inv_n=1.0 / B), ("loss", "P")
    elif n == 9:
        bad, fails = fin(), ("loss",)
        bad.loss = bad.loss_rows[3:].sum() * bad.inv_n       # chunks [0, 3) and [3, 5)
    elif n == 10:
        x2 = x.clone()
        x2[0] *= 2.0
        bad, fails = fin(x=x2), ("lse", "P")
    elif n == 11:
        s0, s1, es = _split_h(inp.seq)
        w0, w1, ew = _split_h(inp.table)
        sc = (es[:, None] + ew[None, :] - 28)
        full = torch.ldexp(w1 @ s0.t() + w0 @ s1.t() + w0 @ s0.t(), sc.t()).t()
        assert float((full - r64.x).abs().max()) <= 2.0 ** -20 * float(r64.logit_scale.max())
        bad, fails = fin(x=torch.ldexp(w1 @ s0.t() + w0 @ s0.t(), sc.t()).t().contiguous()), ("lse",)
    elif n == 12:
        bad, fails = fin(), ("ditems",)
        v = int(inp.target[B - 1])
        last = (B - 1) // R.TILE * R.TILE
        bad.ditems[v] = bad.P[:last, v] @ inp.seq[:last]
    else:
        raise ValueError(n)
    return {k: getattr(bad, k) for k in R.TENSORS}, r64, r32, fails


@pytest.mark.parametrize("n", range(1, 13))
def test_planted_error_is_rejected(n):
    got, r64, r32, fails = _planted(n)
    res = R.judge_all(got, r64, r32, TG.M)
    print(n, {k: "ok" if v[0] else f"err {v[1]:.2e} > bar {v[2]:.2e}" for k, v in res.items()})
    for k in fails:
        assert not res[k][0], (n, k, res[k])


def test_unplanted_fp32_run_passes():
    """The same bar accepts the fp32 run itself, on the planted errors' cases."""
    for c, ignored in ((("random", 5, 7, 64), (1,)), (("random", 33, 64, 64), ())):
        r64, r32 = R.both(R.case_inputs(c, ignored), 0.7)
        res = R.judge_all({k: getattr(r32, k) for k in R.TENSORS}, r64, r32, TG.M)
        assert all(v[0] for v in res.values()), res
    assert all(math.isfinite(m) and m >= 1 for m in TG.M.values())

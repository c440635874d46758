"""Candidate-list scoring, host side: the header and its binding, the C-ABI's
argument checks (before any HIP call: host integers stand in for pointers),
the selection rule and the ranks in torch ops against plain Python loops, the
bad-argument errors, and session.rerank on a CPU state.  No GPU."""
import ctypes
import math

import pytest
import torch

from datamining_recblr_amd import _lib, kernels, scoring, session

from test_gpu_session import _model, _sequences

NAMES = ("rb_candidate_scores", "rb_candidate_topk", "rb_candidate_ranks")
NINF = float("-inf")


# ---- header and binding --------------------------------------------------------------
def test_header_declares_exactly_the_three_entry_points():
    p, i64, f32, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_int
    want = {
        "rb_candidate_scores": (i32, [p, i64, p, p, i64, i64, i64, i64, p, p]),
        "rb_candidate_topk": (i32, [p, i64, p, p, i64, i64, i64, i64, i64, i64, p, i64, p, p, p]),
        "rb_candidate_ranks": (i32, [p, i64, p, p, p, i64, i64, i64, i64, i64, p, p, p]),
    }
    assert f32 not in sum((a for _, a in want.values()), [])
    assert set(_lib.CANDIDATE_SIGNATURES) == set(NAMES)
    assert dict(_lib.CANDIDATE_SIGNATURES) == want
    assert not set(NAMES) & set(_lib.SIGNATURES)          # recblr_hip.h keeps its entries


def test_library_exports_them_at_the_headers_version():
    lib = _lib.load()
    assert lib.rb_version() == _lib.ABI_VERSION
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.CANDIDATE_SIGNATURES[name][1]
    assert {"candidate_scores", "candidate_topk", "candidate_ranks",
            "candidates_supported"} <= set(kernels.__all__)
    assert kernels.CANDIDATE_MAX == 4096 and kernels.CANDIDATE_EXCLUDE_MAX == 4096
    assert not set(NAMES) & set(kernels.FLOP_KERNELS)     # counted in bytes


# ---- argument checks -----------------------------------------------------------------
# a valid call's arguments; 16, 32 ... are "pointers" (16-B aligned, never read)
GOOD = dict(h=16, ldh=8, table=32, cand=48, B=2, C=5, d=8, V=10, first_item=1, k=3, exclude=64,
            E=2, ids=80, scores=96, target=112, gt=128, eq=144)


def _call(name, **over):
    a = dict(GOOD, **over)
    lib = _lib.load()
    if name == "rb_candidate_scores":
        return lib.rb_candidate_scores(a["h"], a["ldh"], a["table"], a["cand"], a["B"], a["C"],
                                       a["d"], a["V"], a["scores"], None)
    if name == "rb_candidate_topk":
        return lib.rb_candidate_topk(a["h"], a["ldh"], a["table"], a["cand"], a["B"], a["C"],
                                     a["d"], a["V"], a["first_item"], a["k"], a["exclude"],
                                     a["E"], a["ids"], a["scores"], None)
    return lib.rb_candidate_ranks(a["h"], a["ldh"], a["table"], a["target"], a["cand"], a["B"],
                                  a["C"], a["d"], a["V"], a["first_item"], a["gt"], a["eq"], None)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("over", [dict(d=6, ldh=8), dict(d=516, ldh=516), dict(h=24),
                                  dict(ldh=9), dict(C=0), dict(V=0), dict(V=1 << 31),
                                  dict(table=None), dict(cand=None), dict(B=-1)],
                         ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_shared_argument_checks(name, over):
    assert _call(name, **over) == _lib.RB_EINVAL
    assert name.encode() in _lib.load().rb_last_error_string()


@pytest.mark.parametrize("over", [dict(C=4097), dict(E=4097), dict(k=0), dict(first_item=11),
                                  dict(first_item=-1), dict(E=-1), dict(exclude=None),
                                  dict(ids=None)],
                         ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_topk_argument_checks(over):
    assert _call("rb_candidate_topk", **over) == _lib.RB_EINVAL


def test_ranks_argument_checks_and_empty_batches():
    assert _call("rb_candidate_ranks", first_item=11) == _lib.RB_EINVAL
    assert _call("rb_candidate_ranks", target=None) == _lib.RB_EINVAL
    assert _call("rb_candidate_scores", scores=None) == _lib.RB_EINVAL
    for name in NAMES:                                    # B = 0: nothing to do, before any check
        assert _call(name, B=0, h=None, cand=None) == 0


# ---- the selection rule against a loop ------------------------------------------------
V_SMALL = 9


def _crafted():
    """scores, ids [3, 12] and an exclude list [3, 3] that between them hold:
    exact ties, duplicate ids (with equal scores, as a pure score function
    gives), ids -1 and V, id 0 (dropped by first_item = 1), exclude entries
    outside [0, V), a NaN score, and a selectable candidate scoring -inf."""
    nan = float("nan")
    ids = torch.tensor([[5, 3, 3, -1, 9, 0, 7, 2, 8, 5, 1, 4],
                        [1, 2, 3, 4, 5, 6, 7, 8, 8, 8, -1, 9],
                        [-1, -1, 9, 0, 0, 9, -1, 4, 4, 6, 2, 2]])
    scores = torch.tensor([[1.5, 2.0, 2.0, NINF, 9.0, 7.0, 2.0, nan, NINF, 1.5, -0.0, 0.0],
                           [0.5, 0.5, 0.5, 0.25, nan, NINF, 3.0, -1.0, -1.0, -1.0, NINF, 4.0],
                           [NINF, NINF, 1.0, 5.0, 5.0, 1.0, NINF, NINF, NINF, 2.5, 2.5, 2.5]])
    exclude = torch.tensor([[7, -1, 9], [100, 3, 3], [-5, 9, 10]])
    return scores, ids, exclude


def order_by_loop(scores, ids, k, first_item, exclude, V):
    out_ids, out_scores = [], []
    for b in range(scores.shape[0]):
        banned = set() if exclude is None else {int(e) for e in exclude[b] if 0 <= int(e) < V}
        best = {}
        for s, i in zip(scores[b].tolist(), ids[b].tolist()):
            if not first_item <= i < V or i in banned or math.isnan(s):
                continue
            best[i] = max(best.get(i, NINF), s)
        ranked = sorted(best.items(), key=lambda t: (-t[1], t[0]))[:k]
        out_ids.append([i for i, _ in ranked] + [-1] * (k - len(ranked)))
        out_scores.append([s for _, s in ranked] + [NINF] * (k - len(ranked)))
    return torch.tensor(out_ids), torch.tensor(out_scores)


@pytest.mark.parametrize("k", [1, 12, 15])
@pytest.mark.parametrize("first_item", [0, 1])
@pytest.mark.parametrize("with_exclude", [False, True])
def test_order_candidates_equals_the_loop(k, first_item, with_exclude):
    scores, ids, exclude = _crafted()
    exclude = exclude if with_exclude else None
    got = scoring.order_candidates(scores, ids, k, first_item, exclude, num_items=V_SMALL)
    want = order_by_loop(scores, ids, k, first_item, exclude, V_SMALL)
    assert torch.equal(got[0], want[0])
    assert torch.equal(got[1], want[1])
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32


def test_order_candidates_named_cases():
    scores, ids, exclude = _crafted()
    got_ids, got = scoring.order_candidates(scores, ids, 15, 1, exclude, num_items=V_SMALL)
    # row 0: 3 before 5 (2.0 > 1.5), once each; 7 excluded; 9 = V, 0 and -1 dropped; the NaN (2)
    # dropped; 1 and 4 tie at zero (-0 == 0), smaller id first; 8 scores -inf but is selectable
    assert got_ids[0].tolist() == [3, 5, 1, 4, 8] + [-1] * 10
    assert got[0, 4] == NINF and got_ids[0, 4] == 8
    # row 1: ties among 1, 2 (3 excluded); 8 three times, once; 6 at -inf before the padding
    assert got_ids[1].tolist() == [7, 1, 2, 4, 8, 6] + [-1] * 9
    # row 2: 4 scores -inf and survives; 2 twice -> once
    assert got_ids[2].tolist() == [2, 6, 4] + [-1] * 12
    # without an upper limit the id 9 is a candidate like any other
    free, _ = scoring.order_candidates(scores, ids, 1, 1)
    assert free[:, 0].tolist() == [9, 9, 2]


# ---- the CPU paths against fp64 loops ---------------------------------------------------
def _small(seed=3):
    g = torch.Generator().manual_seed(seed)
    B, C, d, V = 3, 7, 8, 20
    h = torch.randn(B, d, generator=g)
    table = torch.randn(V, d, generator=g)
    cand = torch.randint(0, V, (B, C), generator=g)
    cand[0, 2], cand[1, 0], cand[2, 6] = -1, V, cand[2, 0]
    return h, table, cand, V


def test_cpu_candidate_scores_and_top_candidates():
    h, table, cand, V = _small()
    got = scoring.candidate_scores(h, table, cand)
    assert got.shape == cand.shape and got.dtype == torch.float32
    for b in range(cand.shape[0]):
        for c, i in enumerate(cand[b].tolist()):
            if not 0 <= i < V:
                assert got[b, c] == NINF
                continue
            ref = float(h[b].double() @ table[i].double())
            bound = h.shape[1] * 2.0 ** -23 * float((h[b].double() * table[i].double()).abs().sum())
            assert abs(float(got[b, c]) - ref) <= bound
    exclude = torch.stack([cand[:, 1], torch.full((3,), -1), torch.full((3,), V + 3)], 1)
    for k in (1, 7, 9):
        ids, scores = scoring.top_candidates(h, table, cand, k, first_item=1, exclude=exclude)
        want = order_by_loop(got, cand, k, 1, exclude, V)
        assert torch.equal(ids, want[0]) and torch.equal(scores, want[1])
    # differentiable: the several-item predict
    hh, tt = h.clone().requires_grad_(), table.clone().requires_grad_()
    s = scoring.candidate_scores(hh, tt, cand)
    s[torch.isfinite(s)].sum().backward()
    assert torch.isfinite(hh.grad).all() and torch.isfinite(tt.grad).all()
    assert float(tt.grad[cand[0, 0]].abs().sum()) > 0


def test_cpu_candidate_ranks():
    h, table, cand, V = _small()
    target = torch.tensor([int(cand[0, 0]), 0, V])        # listed itself; below first_item; = V
    table[int(cand[0, 1])] = table[int(cand[0, 0])]       # an exact tie with the target
    gt, eq = scoring.candidate_ranks(h, table, target, cand, first_item=1)
    t0 = int(target[0])
    st = float(h[0].double() @ table[t0].double())
    want_gt = want_eq = 0
    for i in cand[0].tolist():
        if not 1 <= i < V or i == t0:
            continue
        s = float(h[0].double() @ table[i].double())
        same = torch.equal(table[i], table[t0])
        want_gt += (not same) and s > st
        want_eq += same
    assert (int(gt[0]), int(eq[0])) == (want_gt, want_eq) and want_eq >= 1
    assert gt[1:].tolist() == [-1, -1] and eq[1:].tolist() == [-1, -1]
    assert gt.dtype == torch.int64
    m = scoring.rank_metrics(gt, eq, topk=(5,))
    assert 0.0 <= m["ndcg@5"] <= 1.0


def test_bad_arguments_raise():
    h, table, cand, _ = _small()
    with pytest.raises(ValueError, match="k ="):
        scoring.top_candidates(h, table, cand, 0)
    with pytest.raises(ValueError, match="first_item"):
        scoring.top_candidates(h, table, cand, 3, first_item=-1)
    with pytest.raises(ValueError, match=r"\[B, C\]"):
        scoring.top_candidates(h, table, cand[0], 3)
    with pytest.raises(ValueError, match=r"\[B, C\]"):
        scoring.top_candidates(h, table, cand[:2], 3)
    with pytest.raises(ValueError, match=r"\[B, E\]"):
        scoring.top_candidates(h, table, cand, 3, exclude=cand[0])
    with pytest.raises(ValueError, match=r"\[B, E\]"):
        scoring.top_candidates(h, table, cand, 3, exclude=cand[:2])
    with pytest.raises(ValueError, match="k ="):
        scoring.order_candidates(torch.zeros(3, 7), cand, 0)
    with pytest.raises(ValueError, match=r"\[B, C\]"):
        scoring.candidate_scores(h, table, cand.reshape(-1))
    with pytest.raises(ValueError, match=r"target must be \[B\]"):
        scoring.candidate_ranks(h, table, cand[:, :2], cand)
    assert not kernels.candidates_supported(h, table)      # CPU tensors


# ---- session.rerank on a CPU state --------------------------------------------------------
def test_rerank_on_a_cpu_state():
    L, S, N, k, C = 12, 6, 4, 5, 9
    model, _ = _model(torch.device("cpu"), L=L)
    emb = model.item_embedding.weight.detach()
    V = emb.shape[0]
    state, twin = model.session_open(N, L, history=S), model.session_open(N, L, history=S)
    seq, _ = _sequences(L, [L, 7, 0, 3])
    slots = torch.tensor([3, 0, 2, 1])                     # row 2 holds no event: slot 2 stays dead
    g = torch.Generator().manual_seed(4)
    for t in range(8):
        cand = torch.randint(-1, V + 1, (4, C), generator=g)
        cand[0, :3] = seq[0, :3]                           # seen items among the candidates
        ids, scores = model.session_rerank(state, cand, seq[:, t], slots, k=k, exclude_seen=True)
        y = session.step_reference(model, twin, seq[:, t], slots)
        seen = twin.items[slots.clamp(0, N - 1)]
        want = scoring.order_candidates(scoring.candidate_scores(y, emb, cand), cand, k, 1,
                                        seen, num_items=V)
        assert torch.equal(ids[:2], want[0][:2]) and torch.equal(scores[:2], want[1][:2])
        assert torch.equal(ids[3], want[0][3]) and torch.equal(scores[3], want[1][3])
        assert ids[2].tolist() == [-1] * k and torch.isneginf(scores[2]).all()      # dead
        assert state.status.tolist() == twin.status.tolist()
        if 3 <= t < S:                                     # while the ring still holds them
            assert not set(ids[0].tolist()) & set(seq[0, :3].tolist())
    assert torch.equal(state.items, twin.items) and torch.equal(state.out, twin.out)
    # no event: the stored rows of the whole state; then without the exclusion
    cand = torch.randint(1, V, (N, C), generator=g)
    ids, scores = session.rerank(model, state, cand, k=C)
    want = scoring.order_candidates(scoring.candidate_scores(state.out, emb, cand), cand, C, 1,
                                    num_items=V)
    live = (state.count > 0).nonzero().reshape(-1)
    assert live.numel() == 3
    assert torch.equal(ids[live], want[0][live]) and torch.equal(scores[live], want[1][live])
    assert (ids[state.count == 0] == -1).all()
    # several events per row
    wide, _ = _sequences(20, [20, 2, 0, 5], seed=6)
    ids, scores = session.rerank(model, state, cand, wide, slots, k=k, exclude_seen=True)
    y = session.append_reference(model, twin, wide, slots=slots)
    want = scoring.order_candidates(scoring.candidate_scores(y, emb, cand), cand, k, 1,
                                    twin.items[slots.clamp(0, N - 1)], num_items=V)
    assert torch.equal(ids[:2], want[0][:2]) and torch.equal(scores[:2], want[1][:2])
    # a slot outside the state: a host slot list is checked, as step and recommend check it;
    # on the device such a row is masked to -1 / -inf (tests/test_gpu_candidates.py)
    with pytest.raises(ValueError, match="slots must lie in"):
        session.rerank(model, state, cand, None, [0, 1, 2, N], k=k)
    # refusals: no ring, a candidates tensor of another batch (before any event is consumed)
    plain = model.session_open(N, L)
    with pytest.raises(ValueError, match="history="):
        model.session_rerank(plain, cand, seq[:, 0], slots, exclude_seen=True)
    before = state.count.clone()
    with pytest.raises(ValueError, match="candidates"):
        session.rerank(model, state, cand[:2], seq[:, 0], slots)
    assert torch.equal(state.count, before)

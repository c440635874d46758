"""Score priors, the parts that need no GPU: scoring.item_priors and
log_popularity, the contract of top_items' prior / prior_rows / prior_weight on
the torch path (small cases checked by hand), the argument errors,
evaluation.recommend's per-user alignment, the header include/recblr_priors.h
and the argument checks of rb_item_topk_prior / rb_item_rank_prior (made before
any HIP call)."""
import ctypes
import math

import pytest
import torch

from datamining_recblr_amd import _lib, evaluation, kernels, scoring

NINF = float("-inf")


def bits(x):
    return x.contiguous().view(torch.int32)


# ---- item_priors ----------------------------------------------------------------------
def test_item_priors_forms():
    p = scoring.item_priors(torch.tensor([0.5, -1.0, 2.0]))
    assert isinstance(p, scoring.ItemPriors)
    assert p.values.dtype == torch.float32 and p.values.shape == (1, 3) and p.values.is_contiguous()
    assert (p.n_priors, p.n_items) == (1, 3)
    assert p.to("cpu") is p
    q = scoring.item_priors(torch.arange(12, dtype=torch.float64).view(3, 4).t())   # strided, fp64
    assert q.values.dtype == torch.float32 and q.values.is_contiguous()
    assert (q.n_priors, q.n_items) == (4, 3) and q.values[1].tolist() == [1.0, 5.0, 9.0]
    r = scoring.item_priors([[1, 2, 3], [0.5, NINF, float("nan")]], n_items=3, device="cpu")
    assert r.values.dtype == torch.float32 and r.values.shape == (2, 3)
    assert r.values[1, 1] == NINF and math.isnan(float(r.values[1, 2]))
    h = scoring.item_priors(torch.tensor([1.0, 2.0], dtype=torch.float16))
    assert h.values.dtype == torch.float32
    assert {"item_priors", "ItemPriors", "log_popularity"} <= set(scoring.__all__)


def test_item_priors_rejects_bad_input():
    with pytest.raises(ValueError):
        scoring.item_priors(torch.zeros(4), n_items=5)
    with pytest.raises(ValueError):
        scoring.item_priors(torch.zeros((2, 4)), n_items=2)
    with pytest.raises(ValueError):
        scoring.item_priors(torch.zeros((2, 3, 4)))
    with pytest.raises(ValueError):
        scoring.item_priors(torch.zeros((0, 4)))
    with pytest.raises(ValueError):
        scoring.item_priors(torch.tensor([1, 2, 3]))                 # an integer tensor
    with pytest.raises(ValueError):
        scoring.ItemPriors(torch.zeros((1, 4), dtype=torch.float64))
    with pytest.raises(ValueError):
        scoring.ItemPriors(torch.zeros(4))


# ---- log_popularity -------------------------------------------------------------------
def test_log_popularity():
    counts = torch.tensor([0, 3, 3, 10, 1, 250])
    lp = scoring.log_popularity(counts)
    assert lp.dtype == torch.float32 and lp.shape == (6,)
    assert abs(float(lp.double().exp().sum()) - 1.0) < 1e-6
    order = torch.argsort(counts, stable=True)
    assert (lp[order][1:] >= lp[order][:-1]).all() and lp[1] == lp[2] and lp[5] > lp[3] > lp[4]
    # smoothing 1: q proportional to counts + 1
    want = torch.log((counts + 1).double() / (counts + 1).sum())
    assert torch.allclose(lp.double(), want, atol=1e-6)
    # alpha tempers (0: uniform), smoothing flattens
    flat = scoring.log_popularity(counts, alpha=0.0)
    assert torch.allclose(flat, torch.full((6,), -math.log(6.0)), atol=1e-6)
    half = scoring.log_popularity(counts, alpha=0.5)
    assert abs(float(half.double().exp().sum()) - 1.0) < 1e-6
    assert (half[5] - half[0]) < (lp[5] - lp[0])
    assert torch.allclose((half[5] - half[0]).double(), 0.5 * (lp[5] - lp[0]).double(), atol=1e-6)
    smooth = scoring.log_popularity(counts, smoothing=100.0)
    assert (smooth[5] - smooth[0]) < (lp[5] - lp[0])
    assert scoring.log_popularity([1, 2, 3]).shape == (3,)
    with pytest.raises(ValueError):
        scoring.log_popularity(torch.zeros((2, 2)))


# ---- the torch path's contract, by hand ----------------------------------------------
# d = 1 and seq = 1: an item's score is its table entry.  Item 0 is below first_item.
SCORES = [9.0, 5.0, 4.0, 3.0, -0.0, 1.0, 2.0, 2.0]
V = len(SCORES)


def _top(prior=None, k=3, B=1, **kw):
    seq = torch.ones((B, 1))
    W = torch.tensor(SCORES)[:, None]
    if prior is not None:
        kw["prior"] = scoring.item_priors(prior)
    return scoring.top_items(seq, W, k, **kw)


def test_a_prior_reorders_and_returns_adjusted_scores():
    ids, sc = _top()
    assert ids.tolist() == [[1, 2, 3]] and sc.tolist() == [[5.0, 4.0, 3.0]]
    ids, sc = _top([0, 0, 1.5, 0, 0, 0, 0, 0])
    assert ids.tolist() == [[2, 1, 3]] and sc.tolist() == [[5.5, 5.0, 3.0]]
    # a prior on item 0 does not bring it past first_item
    ids, _ = _top([100.0, 0, 0, 0, 0, 0, 0, 0])
    assert ids.tolist() == [[1, 2, 3]]
    ids, _ = _top([100.0, 0, 0, 0, 0, 0, 0, 0], first_item=0)
    assert ids[0, 0] == 0


def test_inf_and_nan_priors():
    # -inf sinks item 1 but does not hide it: it is the last of the 7 selectable
    ids, sc = _top([0, NINF, 0, 0, 0, 0, 0, 0], k=8)
    assert ids.tolist() == [[2, 3, 6, 7, 5, 4, 1, -1]]
    assert sc[0, 6] == NINF and sc[0, 7] == NINF and sc[0, 5] == 0.0
    ids, _ = _top([0, NINF, 0, 0, 0, 0, 0, 0], k=3)
    assert ids.tolist() == [[2, 3, 6]]
    # NaN drops it: six selectable items
    ids, sc = _top([0, float("nan"), 0, 0, 0, 0, 0, 0], k=8)
    assert ids.tolist() == [[2, 3, 6, 7, 5, 4, -1, -1]] and (sc[0, 6:] == NINF).all()
    # +inf lifts; inf * 0 and inf - inf are NaN: dropped
    ids, sc = _top([0, 0, 0, 0, 0, float("inf"), 0, 0])
    assert ids.tolist() == [[5, 1, 2]] and sc[0, 0] == float("inf")
    ids, _ = _top([0, 0, 0, 0, 0, float("inf"), 0, 0], prior_weight=0.0, k=8)
    assert 5 not in ids[0].tolist() and (ids[0] >= 0).sum() == 6
    W = torch.tensor(SCORES)[:, None].clone()
    W[5] = float("inf")
    ids, _ = scoring.top_items(torch.ones((1, 1)), W, 8,
                               prior=scoring.item_priors([0, 0, 0, 0, 0, NINF, 0, 0]))
    assert 5 not in ids[0].tolist()


def test_prior_rows_and_weights():
    prior = [[0, 0, 1.5, 0, 0, 0, 0, 0], [0, -10.0, 0, 0, 0, 0, 0, 0]]
    rows = torch.tensor([0, 1, -1, 2, -2])
    ids, sc = _top(prior, B=5, prior_rows=rows)
    plain_ids, plain_sc = _top(B=5)
    assert ids[0].tolist() == [2, 1, 3] and ids[1].tolist() == [2, 3, 6]
    assert torch.equal(ids[2], plain_ids[2]) and torch.equal(bits(sc[2]), bits(plain_sc[2]))
    assert (ids[3:] == -1).all() and (sc[3:] == NINF).all()          # outside [-1, P)
    # None: prior 0 for every row
    ids, _ = _top(prior, B=2)
    assert ids.tolist() == [[2, 1, 3]] * 2
    # a scalar weight, and one per row (negative, zero)
    ids, sc = _top(prior, prior_weight=-2.0)
    assert ids.tolist() == [[1, 3, 6]] and sc.tolist() == [[5.0, 3.0, 2.0]]
    w = torch.tensor([1.0, -2.0, 0.0, 4.0])
    ids, sc = _top(prior, B=4, prior_weight=w, k=2)
    assert ids.tolist() == [[2, 1], [1, 3], [1, 2], [2, 1]]
    assert sc.tolist() == [[5.5, 5.0], [5.0, 3.0], [5.0, 4.0], [10.0, 5.0]]
    ids64, sc64 = _top(prior, B=4, prior_weight=w.double(), k=2)     # any float dtype
    assert torch.equal(ids64, ids) and torch.equal(sc64, sc)


def test_no_prior_row_keeps_a_negative_zero():
    """prior_rows = -1 is a select: item 4 scores -0.0 and keeps its sign bit,
    where adding a zero prior gives +0.0."""
    zero = scoring.item_priors([0.0] * V)
    S = torch.tensor([SCORES])               # a matmul never yields -0.0: the matrix is given
    assert math.copysign(1.0, float(S[0, 4])) == -1.0

    def top(**kw):
        return scoring._top_items_torch(torch.ones((1, 1)), torch.zeros((V, 1)), 8, 1, None,
                                        scores=S, **kw)

    ids, sc = top(prior=zero, prior_rows=torch.tensor([-1]))
    _, plain = top()
    assert torch.equal(bits(sc), bits(plain))
    assert ids[0, 6] == 4 and sc[0, 6] == 0.0 and math.copysign(1.0, float(sc[0, 6])) == -1.0
    ids, sc = top(prior=zero)
    assert ids[0, 6] == 4 and math.copysign(1.0, float(sc[0, 6])) == 1.0


def test_ties_made_by_the_prior_resolve_by_id():
    # 5 + 0 = 4 + 1 = 3 + 2 = 1 + 4: items 1, 2, 3, 5 tie at 5.0
    ids, sc = _top([0, 0, 1.0, 2.0, 0, 4.0, 0, 0], k=5)
    assert ids.tolist() == [[1, 2, 3, 5, 6]] and sc.tolist() == [[5.0, 5.0, 5.0, 5.0, 2.0]]
    # and a tie of the model's (6 and 7) is split by the prior
    ids, _ = _top([0, 0, 0, 0, 0, 0, 0, 0.25], k=5)
    assert ids.tolist() == [[1, 2, 3, 7, 6]]


def test_prior_with_exclude_filter_and_cap():
    prior = [0, 0, 1.5, 0, 0, 3.0, 0, 0.5]     # adj: 1: 5, 2: 5.5, 3: 3, 4: -0, 5: 4, 6: 2, 7: 2.5
    ids, _ = _top(prior, k=4)
    assert ids.tolist() == [[2, 1, 5, 3]]
    ids, _ = _top(prior, k=4, exclude=torch.tensor([[2, 0, -1, 99]]))
    assert ids.tolist() == [[1, 5, 3, 7]]
    allow = scoring.item_filters([[1, 3, 5, 6, 7]], n_items=V)
    ids, _ = _top(prior, k=4, allow=allow)
    assert ids.tolist() == [[1, 5, 3, 7]]
    groups = scoring.item_groups([-1, 0, 0, 1, 1, 0, 1, -1])
    ids, sc = _top(prior, k=4, groups=groups, max_per_group=1)
    assert ids.tolist() == [[2, 3, 7, -1]] and sc.tolist()[0][:3] == [5.5, 3.0, 2.5]
    ids, _ = _top(prior, k=4, groups=groups, max_per_group=1, allow=allow,
                  exclude=torch.tensor([[3]]))
    assert ids.tolist() == [[1, 7, 6, -1]]      # group 0: 1 (5 capped); group 1: 6; 7 is free
    # k beyond the kernel's 64 is the torch path's too
    ids, _ = _top(prior, k=100)
    assert ids[0, :7].tolist() == [2, 1, 5, 3, 7, 6, 4] and (ids[0, 7:] == -1).all()


def test_two_roundings():
    """The product is rounded to fp32 before the sum: with w = 1 + 2^-12 and
    prior = 1 + 2^-12 the exact product 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11,
    and score -1 leaves 2^-11 where one rounding (an fma) leaves 2^-11 + 2^-24."""
    e = 2.0 ** -12
    seq = torch.ones((1, 1))
    W = torch.tensor([[0.0], [-1.0]])
    _, sc = scoring.top_items(seq, W, 1, prior=scoring.item_priors([0.0, 1.0 + e]),
                              prior_weight=1.0 + e)
    assert float(sc[0, 0]) == 2.0 ** -11


def test_torch_ranks_reference():
    seq = torch.ones((4, 1))
    W = torch.tensor(SCORES)[:, None]
    prior = scoring.item_priors([0, 0, 1.0, 2.0, 0, 4.0, 0, float("nan")])   # 1, 2, 3, 5 tie at 5
    target = torch.tensor([3, 6, 7, 2])
    gt, eq = scoring._target_ranks_torch(seq, W, target, prior=prior,
                                         prior_rows=torch.tensor([0, 0, 0, 4]))
    assert gt.tolist() == [0, 4, -1, -1] and eq.tolist() == [3, 0, -1, -1]
    gt, eq = scoring._target_ranks_torch(seq, W, target)
    assert gt.tolist() == [2, 3, 3, 1] and eq.tolist() == [0, 1, 1, 0]


# ---- argument errors ------------------------------------------------------------------
def test_argument_errors():
    seq, W = torch.ones((2, 1)), torch.tensor(SCORES)[:, None]
    prior = scoring.item_priors([0.0] * V)
    with pytest.raises(ValueError):
        scoring.top_items(seq, W, 3, prior_rows=torch.tensor([0, 0]))
    with pytest.raises(ValueError):
        scoring.top_items(seq, W, 3, prior_weight=2.0)
    with pytest.raises(ValueError):
        scoring.top_items(seq, W, 3, prior=scoring.item_priors([0.0] * (V + 1)))
    with pytest.raises(TypeError):
        scoring.top_items(seq, W, 3, prior=torch.zeros((1, V)))
    with pytest.raises(ValueError):
        scoring.top_items(seq, W, 3, prior=prior, prior_rows=torch.tensor([0, 0, 0]))
    with pytest.raises(ValueError):
        scoring.top_items(seq, W, 3, prior=prior, prior_weight=torch.ones(3))
    with pytest.raises(ValueError):
        scoring.top_items(seq, W, 3, prior=prior, prior_weight=torch.ones(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        scoring._target_ranks_torch(seq, W, torch.tensor([1, 2]), prior_rows=torch.tensor([0, 0]))
    with pytest.raises(ValueError):
        scoring._target_ranks_torch(seq, W, torch.tensor([1, 2]),
                                    prior=scoring.item_priors([0.0] * (V - 1)))
    with pytest.raises(ValueError):
        evaluation.recommend(None, [[1]], prior_rows=[0], device="cpu")
    with pytest.raises(ValueError):
        evaluation.full_sort_metrics(None, [], prior_weight=1.0)


# ---- evaluation.recommend: per-user arguments follow the length sort --------------------
def test_recommend_keeps_per_user_priors_through_the_length_sort(monkeypatch):
    n_items = 40

    class Mean(torch.nn.Module):
        """A CPU stand-in with the model's interface: a row's output is its
        last item's embedding (d = 5: the torch paths)."""

        def __init__(self):
            super().__init__()
            self.item_embedding = torch.nn.Embedding(n_items, 5)

        def forward(self, item_seq, item_seq_len, exact_lengths=False):
            last = item_seq[torch.arange(item_seq.shape[0]), item_seq_len - 1]
            return self.item_embedding(last)

    torch.manual_seed(0)
    model = Mean().eval()
    g = torch.Generator().manual_seed(2)
    lengths = [5, 1, 8, 2, 2, 7, 3]
    n = len(lengths)
    users = [torch.randint(1, n_items, (L,), generator=g).tolist() for L in lengths]
    prior = scoring.item_priors(torch.randn((3, n_items), generator=g))
    rows = torch.tensor([0, 1, 2, -1, 1, 0, 2])
    weight = torch.tensor([1.0, -0.5, 2.0, 3.0, 0.25, -1.0, 0.0])
    calls = []
    real = scoring.top_items

    def spy(out, *a, **kw):
        calls.append((out.shape[0], kw["prior_rows"].clone(), kw["prior_weight"].clone()))
        return real(out, *a, **kw)

    monkeypatch.setattr(evaluation, "top_items", spy)
    ids, sc = evaluation.recommend(model, users, k=5, batch_size=3, prior=prior, prior_rows=rows,
                                   prior_weight=weight, device="cpu")
    order = torch.argsort(torch.tensor(lengths), stable=True)
    assert order.tolist() != list(range(n)) and len(calls) == 3
    for i, (nb, r, w) in enumerate(calls):
        idx = order[3 * i:3 * i + 3]
        assert nb == len(idx) and torch.equal(r, rows[idx]) and torch.equal(w, weight[idx])
    # every user alone, with their own row and weight, gives their list (the
    # scores to a few ulp: a matmul's bits may depend on the batch's shape,
    # while a row or weight gone astray moves them by whole units)
    monkeypatch.setattr(evaluation, "top_items", real)
    for u in range(n):
        one = evaluation.recommend(model, [users[u]], k=5, prior=prior, prior_rows=rows[u:u + 1],
                                   prior_weight=float(weight[u]), device="cpu")
        assert torch.equal(one[0][0], ids[u])
        assert torch.allclose(one[1][0], sc[u], rtol=1e-5, atol=1e-6)
    # the priors matter: without them some list differs
    plain = evaluation.recommend(model, users, k=5, device="cpu")
    assert not torch.equal(plain[0], ids)
    assert torch.equal(plain[0][3], ids[3]) and torch.equal(bits(plain[1][3]), bits(sc[3]))


# ---- header and binding --------------------------------------------------------------
TOPK, RANK = "rb_item_topk_prior", "rb_item_rank_prior"


def test_header_declares_the_entry_points():
    p, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert dict(_lib.PRIOR_SIGNATURES) == {
        TOPK + "_workspace": (i64, [i64, i64, i64, i64]),
        TOPK: (i32, _lib.GROUP_SIGNATURES["rb_item_topk_grouped"][1] + [p, i64, p, p]),
        RANK: (i32, _lib.FILTER_SIGNATURES["rb_item_rank_allowed"][1] + [p, i64, p, p]),
    }
    others = set(_lib.SIGNATURES) | set(_lib.FILTER_SIGNATURES) | set(_lib.GROUP_SIGNATURES)
    assert not set(_lib.PRIOR_SIGNATURES) & others
    hip = open(_lib.HEADER_PATH).read()
    assert "recblr_priors.h" in hip


def test_library_exports_them_at_the_headers_version():
    lib = _lib.load()
    assert lib.rb_version() == _lib.ABI_VERSION
    for name, (_, args) in _lib.PRIOR_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args
    assert {TOPK, RANK} <= kernels.FLOP_KERNELS
    for shape in ((4, 70, 128, 10), (130, 20000, 16, 64), (2048, 10544, 128, 1)):
        assert lib.rb_item_topk_prior_workspace(*shape) == \
            lib.rb_item_topk_grouped_workspace(*shape) > 0
    for shape in ((0, 70, 128, 10), (4, 70, 128, 0), (4, 70, 128, 65)):
        assert lib.rb_item_topk_prior_workspace(*shape) == 0


# a valid call's arguments; 16 is a "pointer" (16-B aligned, never read)
def _topk(lib, seq=16, items=16, n_rows=4, n_items=70, d=128, k=10, first=1, ex=None, E=0,
          ids=16, scores=16, ws=16, ws_bytes=1 << 20, allow=16, F=2, words=3, rows=16,
          groups=16, m=2, prior=16, P=2, prows=16, pw=16):
    return lib.rb_item_topk_prior(seq, items, n_rows, n_items, d, k, first, ex, E, ids, scores,
                                  ws, ws_bytes, None, allow, F, words, rows, groups, m, prior, P,
                                  prows, pw)


def _rank(lib, seq=16, items=16, target=16, n_rows=4, n_items=70, d=128, first=1, gt=16, eq=16,
          ws=16, ws_bytes=1 << 20, allow=16, F=2, words=3, rows=16, prior=16, P=2, prows=16,
          pw=16):
    return lib.rb_item_rank_prior(seq, items, target, n_rows, n_items, d, first, gt, eq, ws,
                                  ws_bytes, None, allow, F, words, rows, prior, P, prows, pw)


def test_argument_errors_come_back_before_any_hip_call():
    lib = _lib.load()

    def rejected(call, name, msg, **kw):
        assert call(lib, **kw) == _lib.RB_EINVAL, kw
        err = lib.rb_last_error_string()
        assert msg in err, (kw, err)
        if b"prior" in msg or b"P must" in msg or b"workspace" in msg:
            assert err.startswith(name.encode() + b":"), (kw, err)

    for call, name in ((_topk, TOPK), (_rank, RANK)):
        rejected(call, name, b"null pointer (prior)", prior=None)
        rejected(call, name, b"P must be", P=0)
        rejected(call, name, b"P must be", P=-3)
        # the filter is optional, and checked when given
        rejected(call, name, b"F must be", F=0)
        rejected(call, name, b"words must be", words=2)
        rejected(call, name, b"P must be", allow=None, F=0, words=0, P=0)
        rejected(call, name, b"null pointer", seq=None)
        rejected(call, name, b"null pointer", ws=None)
        rejected(call, name, b"d must be", d=48)
        rejected(call, name, b"first_item must be", first=-1)
    rejected(_topk, TOPK, b"max_per_group must be", m=0)
    rejected(_topk, TOPK, b"P must be", groups=None, m=0, P=0)       # no groups: m is ignored
    rejected(_topk, TOPK, b"k must be", k=0)
    rejected(_topk, TOPK, b"k must be", k=65)
    rejected(_topk, TOPK, b"null pointer", E=3, ex=None)
    rejected(_topk, TOPK, b"null pointer", ids=None)
    rejected(_rank, RANK, b"null pointer", target=None)
    rejected(_rank, RANK, b"null pointer", gt=None)
    plain, grouped = lib.rb_item_topk_workspace, lib.rb_item_topk_grouped_workspace
    rejected(_topk, TOPK, b"workspace too small", ws_bytes=grouped(4, 70, 128, 10) - 1)
    rejected(_topk, TOPK, b"workspace too small", groups=None,
             ws_bytes=plain(4, 70, 128, 10) - 1)
    rejected(_rank, RANK, b"workspace too small",
             ws_bytes=lib.rb_item_rank_workspace(4, 70, 128) - 1)

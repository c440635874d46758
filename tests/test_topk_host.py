"""Top-k item retrieval, the parts that need no GPU: scoring.top_items' torch
path against a brute-force sort, rb_item_topk's argument checks (made before
any HIP call) and the size of its workspace."""
import math

import torch

from datamining_recblr_amd import _lib, scoring


def _brute(S, k, first_item, exclude):
    B, V = S.shape
    ids, sc = [], []
    for b in range(B):
        banned = set() if exclude is None else {int(e) for e in exclude[b]}
        cand = [(-float(S[b, v]), v) for v in range(first_item, V)
                if v not in banned and not math.isnan(float(S[b, v]))]
        cand.sort()          # score descending, then id ascending
        cand = cand[:k]
        ids.append([v for _, v in cand] + [-1] * (k - len(cand)))
        sc.append([-s for s, _ in cand] + [float("-inf")] * (k - len(cand)))
    return torch.tensor(ids, dtype=torch.int64), torch.tensor(sc, dtype=torch.float32)


def _ints(B, V, d, seed):
    """Small integer features: exact scores, many ties."""
    g = torch.Generator().manual_seed(seed)
    seq = torch.randint(-2, 3, (B, d), generator=g).float()
    W = torch.randint(-2, 3, (V, d), generator=g).float()
    return seq, W


def test_top_items_torch_path_contract():
    B, V, d = 6, 40, 5          # d = 5: no kernel for it on any device
    seq, W = _ints(B, V, d, 0)
    W[20:24] = W[3]             # a tied group by construction
    S = seq @ W.t()
    assert not scoring.supported(seq, W)
    g = torch.Generator().manual_seed(1)
    ex = torch.randint(1, V, (B, 9), generator=g)
    ex[:, 2] = ex[:, 1]                          # duplicate
    ex[:, 3], ex[:, 4], ex[:, 5] = -1, V, V + 7  # out of range
    ex[:, 6:] = 0                                # padding
    for first_item in (0, 1, 7):
        for exclude in (None, ex, torch.empty((B, 0), dtype=torch.int64)):
            for k in (1, 5, 38, 64):
                ids, sc = scoring.top_items(seq, W, k, first_item=first_item, exclude=exclude)
                ref_ids, ref_sc = _brute(S, k, first_item, exclude)
                assert ids.dtype == torch.int64 and sc.dtype == torch.float32
                assert torch.equal(ids, ref_ids), (first_item, k)
                assert torch.equal(sc, ref_sc), (first_item, k)
    # the tie rule, spelled out: among equal scores the smaller id first
    ids, sc = scoring.top_items(seq, W, V, first_item=0)
    for b in range(B):
        for i in range(V - 1):
            assert sc[b, i] > sc[b, i + 1] or (sc[b, i] == sc[b, i + 1]
                                              and ids[b, i] < ids[b, i + 1])


def test_top_items_torch_path_short_tail_and_non_finite():
    seq, W = _ints(3, 6, 4, 2)
    ids, sc = scoring.top_items(seq, W, 10, first_item=1)
    assert (ids[:, 5:] == -1).all() and (sc[:, 5:] == float("-inf")).all()
    assert sorted(ids[0, :5].tolist()) == [1, 2, 3, 4, 5]
    # first_item beyond the table: nothing selectable
    ids, sc = scoring.top_items(seq, W, 3, first_item=6)
    assert (ids == -1).all() and (sc == float("-inf")).all()
    # NaN is never selected, -inf is an ordinary (last) score, +inf comes first
    seq = torch.ones(2, 4)
    W = torch.arange(24.0).view(6, 4)
    W[2] = float("nan")
    W[3] = float("-inf")
    W[4] = float("inf")
    S = seq @ W.t()
    ids, sc = scoring.top_items(seq, W, 6, first_item=0)
    ref_ids, ref_sc = _brute(S, 6, 0, None)
    assert torch.equal(ids, ref_ids) and torch.equal(sc, ref_sc)
    assert ids[0].tolist() == [4, 5, 1, 0, 3, -1]


def test_top_items_rejects_bad_arguments():
    seq, W = _ints(3, 6, 4, 3)
    for bad in (dict(k=0), dict(k=2, first_item=-1),
                dict(k=2, exclude=torch.zeros((2, 3), dtype=torch.int64))):
        try:
            scoring.top_items(seq, W, **bad)
        except ValueError:
            continue
        raise AssertionError(f"accepted {bad}")


def _topk(lib, seq=16, items=16, B=4, V=8, d=128, k=10, first=1, ex=None, E=0, ids=16,
          scores=16, ws=16, ws_bytes=1 << 20):
    return lib.rb_item_topk(seq, items, B, V, d, k, first, ex, E, ids, scores, ws, ws_bytes, None)


def test_item_topk_argument_errors():
    """Every argument is validated before any HIP call (no GPU here)."""
    lib = _lib.load()

    def rejected(msg, **kw):
        assert _topk(lib, **kw) == _lib.RB_EINVAL, kw
        assert msg in lib.rb_last_error_string(), (kw, lib.rb_last_error_string())

    rejected(b"null pointer", seq=None)
    rejected(b"null pointer", items=None)
    rejected(b"null pointer", ids=None)
    rejected(b"null pointer", scores=None)
    rejected(b"null pointer", ws=None)
    rejected(b"k must be", k=0)
    rejected(b"k must be", k=65)
    rejected(b"d must be", d=48)
    rejected(b"null pointer", E=3, ex=None)
    rejected(b"E must be", E=-1)
    rejected(b"first_item must be", first=-1)
    rejected(b"positive", B=0)
    need = lib.rb_item_topk_workspace(4, 8, 128, 10)
    assert need > 0
    rejected(b"workspace too small", ws_bytes=need - 1)
    assert lib.rb_item_topk_workspace(4, 8, 128, 0) == 0
    assert lib.rb_item_topk_workspace(4, 8, 128, 65) == 0


def test_item_topk_workspace_holds_no_score_matrix():
    lib = _lib.load()
    B, V, d, k = 2048, 1 << 20, 128, 20
    need = lib.rb_item_topk_workspace(B, V, d, k)
    assert 0 < need < 0.01 * B * V * 4
    # candidates only: 8 bytes per (row, split, slot), whatever V is
    small = lib.rb_item_topk_workspace(B, 1 << 14, d, k)
    assert need <= small * 1.01


def test_python_surface():
    from datamining_recblr_amd import evaluation, kernels
    from datamining_recblr_amd.model import RecBLR

    assert "top_items" in scoring.__all__ and "recommend" in evaluation.__all__
    assert "item_topk" in kernels.__all__ and "rb_item_topk" in kernels.FLOP_KERNELS
    assert callable(RecBLR.full_sort_topk)

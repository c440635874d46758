"""GPU tests of the fused top-k item retrieval (rb_item_topk, k_item_topk in
csrc/item_scores.hip) and of what is built on it: scoring.top_items,
RecBLR.full_sort_topk and evaluation.recommend.

The reference never comes from the code under test: it is the existing score
kernel's matrix (kernels.item_scores), each row reduced to the ascending list
of its selectable ids (columns < first_item, excluded ids and NaN scores
removed) and ordered by a stable descending sort, so equal scores keep the
smaller id first.  The top-k kernel runs the score kernel's fma chain, so ids
are compared with torch.equal and scores bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 16), (5, 7, 32), (33, 64, 64), (130, 97, 64), (37, 515, 256), (64, 1000, 128),
          (300, 10544, 128), (5, 300, 16)]
KS = (1, 10, 20, 64)


def _data(B, V, d, cuda, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed * 1000 + B * 7 + V * 3 + d)
    seq = (scale * torch.randn(B, d, generator=g)).to(cuda)
    W = (scale * torch.randn(V, d, generator=g)).to(cuda)
    return seq, W


def _reference(S, k, first_item=1, exclude=None):
    """(ids [B, k], scores [B, k]) on the CPU from a score matrix S [B, V]."""
    S = S.detach().cpu()
    B, V = S.shape
    ids = torch.full((B, k), -1, dtype=torch.int64)
    sc = torch.full((B, k), float("-inf"), dtype=torch.float32)
    ex = None if exclude is None else exclude.detach().cpu()
    for b in range(B):
        keep = ~torch.isnan(S[b])
        keep[:first_item] = False
        if ex is not None and ex.shape[1] > 0:
            e = ex[b]
            keep[e[(e >= 0) & (e < V)]] = False
        idx = torch.nonzero(keep)[:, 0]          # ascending ids
        order = torch.sort(S[b, idx], descending=True, stable=True).indices[:k]
        n = order.numel()
        ids[b, :n] = idx[order]
        sc[b, :n] = S[b, idx[order]]
    return ids, sc


def _same(got, ref, what=""):
    ids, sc = got[0].cpu(), got[1].cpu()
    assert ids.dtype == torch.int64 and sc.dtype == torch.float32
    assert ids.shape == ref[0].shape and sc.shape == ref[1].shape
    assert torch.equal(ids, ref[0]), f"{what}: ids differ in rows " \
        f"{torch.nonzero((ids != ref[0]).any(1))[:8, 0].tolist()}"
    assert torch.equal(sc.view(torch.int32), ref[1].view(torch.int32)), f"{what}: scores differ"


_cache = {}


def _case(B, V, d, cuda, seed=0):
    """(seq, W, score matrix) of a shape, built once per session."""
    from datamining_recblr_amd import kernels

    key = (B, V, d, seed)
    if key not in _cache:
        seq, W = _data(B, V, d, cuda, seed)
        _cache[key] = (seq, W, kernels.item_scores(seq, W).cpu())
    return _cache[key]


@pytest.mark.parametrize("first_item", [0, 1])
@pytest.mark.parametrize("B,V,d", SHAPES)
def test_topk_exact_against_scores(cuda, monkeypatch, B, V, d, first_item):
    from datamining_recblr_amd import kernels

    seq, W, S = _case(B, V, d, cuda)
    ref_ids, ref_sc = _reference(S, max(KS), first_item)
    launches, real_launch = [], kernels._launch

    def spy_launch(name, *a, **kw):
        launches.append(name)
        return real_launch(name, *a, **kw)

    monkeypatch.setattr(kernels, "_launch", spy_launch)
    for k in KS:
        got = kernels.item_topk(seq, W, k, first_item=first_item)
        _same(got, (ref_ids[:, :k], ref_sc[:, :k]), f"k={k}")
        n_ok = max(V - first_item, 0)
        if k > n_ok:   # the short tail
            assert (got[0][:, n_ok:] == -1).all()
            assert (got[1][:, n_ok:] == float("-inf")).all()
            assert (got[0][:, :n_ok] >= first_item).all()
    assert launches == ["rb_item_topk"] * len(KS)      # the plain entry, at both list capacities


def _group_rank(S, item, first_item=1):
    """Per row: how many selectable items score above `item`."""
    ts = S[:, item:item + 1]
    return (S[:, first_item:] > ts).sum(1)


def test_topk_ties_keep_ascending_ids(cuda):
    """Eleven identical item rows (5 and 100..109): the copies come out in
    ascending id order, and a k that cuts the group keeps its smallest ids."""
    from datamining_recblr_amd import kernels

    seq, W = _data(64, 1000, 128, cuda, seed=3)
    W[100:110] = W[5]
    S = kernels.item_scores(seq, W).cpu()
    group = [5] + list(range(100, 110))
    assert all(torch.equal(S[:, 5].view(torch.int32), S[:, g].view(torch.int32)) for g in group)
    r = _group_rank(S, 5)
    row = int(torch.argmin((r - 12).abs()))   # a row with the group well inside the list
    r0 = int(r[row])
    k = r0 + 5          # the group spans positions r0 .. r0 + 10: k cuts it
    assert 1 <= k <= 64, f"test data: best group rank {r0}"
    got = kernels.item_topk(seq, W, k)
    _same(got, _reference(S, k), "ties")
    assert got[0][row, r0:].tolist() == group[:5]
    got = kernels.item_topk(seq, W, 64)
    _same(got, _reference(S, 64), "ties k=64")
    for b in range(64):
        inside = [i for i in got[0][b].tolist() if i in group]
        assert inside == group[:len(inside)]


def test_topk_ties_across_splits(cuda):
    """Copies of one item row at ids 5, 5000 and V - 3 live in different item
    splits: the tie is settled by the merge.  Row 0 leans towards the copied
    row so that the group lands inside the first 64 positions."""
    from datamining_recblr_amd import kernels

    B, V, d = 300, 10544, 128
    seq, W = _data(B, V, d, cuda, seed=4)
    W[5000] = W[5]
    W[V - 3] = W[5]
    seq[0] = seq[0] + 0.35 * W[5]
    S = kernels.item_scores(seq, W).cpu()
    r = _group_rank(S, 5)
    row = int(torch.argmin(r))
    r0 = int(r[row])
    k = r0 + 2          # positions r0, r0 + 1 inside, r0 + 2 outside
    assert 2 <= k <= 64, f"test data: best group rank {r0}"
    got = kernels.item_topk(seq, W, k)
    _same(got, _reference(S, k), "split ties")
    assert got[0][row, r0:].tolist() == [5, 5000]
    got = kernels.item_topk(seq, W, k + 1)
    assert got[0][row, r0:].tolist() == [5, 5000, V - 3]


@pytest.mark.parametrize("B,V,d,k", [(64, 1000, 128, 10), (300, 10544, 128, 20)])
def test_topk_exclusion(cuda, B, V, d, k):
    from datamining_recblr_amd import kernels

    seq, W, S = _case(B, V, d, cuda)
    free_ids, free_sc = _reference(S, k + 5)
    # (a) each row's own top-5 excluded: ranks 6 .. k + 5 remain
    top5 = free_ids[:, :5].to(cuda)
    _same(kernels.item_topk(seq, W, k, exclude=top5), (free_ids[:, 5:], free_sc[:, 5:]), "(a)")
    # (b) a padded list with duplicates and out-of-range ids
    g = torch.Generator(device="cpu").manual_seed(11)
    ex = torch.randint(1, V, (B, 12), generator=g)
    ex[:, 0:2] = free_ids[:, 0:2]
    ex[:, 3] = ex[:, 2]
    ex[:, 4] = free_ids[:, 1]
    ex[:, 5], ex[:, 6], ex[:, 7] = -1, V, V + 7
    ex[:, 8:] = 0
    _same(kernels.item_topk(seq, W, k, exclude=ex.to(cuda)), _reference(S, k, 1, ex), "(b)")
    _same(kernels.item_topk(seq, W, k, first_item=0, exclude=ex.to(cuda)),
          _reference(S, k, 0, ex), "(b) first_item=0")
    # (c) no list, and an empty one
    _same(kernels.item_topk(seq, W, k, exclude=None), (free_ids[:, :k], free_sc[:, :k]), "(c)")
    empty = torch.empty((B, 0), dtype=torch.int64, device=cuda)
    _same(kernels.item_topk(seq, W, k, exclude=empty), (free_ids[:, :k], free_sc[:, :k]), "(c')")
    # (d) one id excluded for everybody: top-1 of some rows only
    q = int(free_ids[0, 0])
    hit = free_ids[:, 0] == q
    assert hit.any() and not hit.all()
    exq = torch.full((B, 1), q, dtype=torch.int64)
    got = kernels.item_topk(seq, W, k, exclude=exq.to(cuda))
    _same(got, _reference(S, k, 1, exq), "(d)")
    assert not (got[0] == q).any()
    assert torch.equal(got[0][~hit.to(cuda)][:, 0].cpu(), free_ids[~hit][:, 0])


def test_topk_exclusion_long_splits(cuda):
    """B = 520 rows over V = 56,000 items: every item split (544 items) spans
    more items than the kernel's per-row exclusion map has bits (its hashed
    path, where a set bit is confirmed against the row's list).  Ids 512
    apart share a bit: excluding the neighbours of a row's best item must not
    remove it."""
    from datamining_recblr_amd import kernels

    B, V, d, k = 520, 56000, 16, 20
    seq, W = _data(B, V, d, cuda, seed=5)
    S = kernels.item_scores(seq, W)
    top = S[:, 1:].topk(4, dim=1).indices.cpu() + 1     # only to build the list
    S = S.cpu()
    g = torch.Generator(device="cpu").manual_seed(12)
    ex = torch.randint(0, V, (B, 40), generator=g)
    best = top[:, 0]
    ex[:, 0], ex[:, 1], ex[:, 2], ex[:, 3] = best - 512, best + 512, best - 1024, best + 1024
    ex[:, 4] = top[:, 1]
    ex[:, 5] = top[:, 3]
    ex[ex == best[:, None]] = 0
    got = kernels.item_topk(seq, W, k, exclude=ex.to(cuda))
    _same(got, _reference(S, k, 1, ex), "hashed")
    assert torch.equal(got[0][:, 0].cpu(), best)


def test_topk_non_finite_scores(cuda):
    from datamining_recblr_amd import kernels

    B, V, d, k = 33, 515, 64, 10
    seq, W = _data(B, V, d, cuda, seed=6)
    clean = kernels.item_scores(seq, W).cpu()
    q = 77
    seq[0] = float("nan")
    seq[1], seq[2] = seq[1].abs(), seq[2].abs()        # dot with +inf components: +inf
    W[q] = float("inf")
    W[300] = float("-inf")                              # -inf for rows 1, 2: a selectable score
    S = kernels.item_scores(seq, W).cpu()
    assert torch.isnan(S[0]).all() and (S[1:3, q] == float("inf")).all()
    assert torch.isnan(S[3:, q]).all() and (S[1:3, 300] == float("-inf")).all()
    got = kernels.item_topk(seq, W, k)
    _same(got, _reference(S, k), "non-finite")
    ids, sc = got[0].cpu(), got[1].cpu()
    assert (ids[0] == -1).all() and (sc[0] == float("-inf")).all()
    assert (ids[1:3, 0] == q).all() and (sc[1:3, 0] == float("inf")).all()
    assert not (ids[3:] == q).any()
    # rows whose inputs did not change: what the clean data gives, minus the two items
    ref = _reference(clean, k, 1, torch.tensor([[q, 300]]).expand(B, 2))
    assert torch.equal(ids[3:], ref[0][3:])
    # -inf is an ordinary score: with every item listed it comes last, before nothing
    full = kernels.item_topk(seq[1:3].contiguous(), W[250:310].contiguous(), 64)
    assert (full[0][:, 58].cpu() == 50).all() and (full[1][:, 58] == float("-inf")).all()
    assert (full[0][:, 59:] == -1).all()


def test_topk_deterministic(cuda):
    from datamining_recblr_amd import kernels

    seq, W, _ = _case(300, 10544, 128, cuda)
    ex = torch.randint(0, 10544, (300, 30), generator=torch.Generator().manual_seed(1)).to(cuda)
    a = kernels.item_topk(seq, W, 20, exclude=ex)
    b = kernels.item_topk(seq, W, 20, exclude=ex)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_top_items_dispatch(cuda):
    """scoring.top_items: the kernel for supported operands and k <= 64, the
    torch path (same contract) for larger k."""
    from datamining_recblr_amd import scoring

    seq, W, S = _case(64, 1000, 128, cuda)
    ex = _reference(S, 3)[0]
    _same(scoring.top_items(seq, W, 20, exclude=ex.to(cuda)), _reference(S, 20, 1, ex), "kernel")
    # k = 100: torch's own GEMM rounds differently, so the contract is checked
    # rather than the list (the CPU test pins the torch path exactly)
    ids, sc = scoring.top_items(seq, W, 100, exclude=ex.to(cuda))
    ids, sc = ids.cpu(), sc.cpu()
    assert ids.shape == (64, 100) and (ids >= 1).all()
    assert not (ids[:, :, None] == ex[:, None, :]).any()
    assert (sc[:, 1:] <= sc[:, :-1]).all()
    bound = ((seq.double().abs() @ W.double().abs().t()) * (128 * 2.0 ** -22)).cpu()
    assert ((sc.double() - S.double().gather(1, ids)).abs() <= bound.gather(1, ids)).all()


def _model(cuda, n_items=3000):
    from datamining_recblr_amd.model import RecBLR
    from datamining_recblr_amd.recbole_compat import SyntheticDataset

    cfg = {"hidden_size": 64, "loss_type": "CE", "num_layers": 2, "dropout_prob": 0.2,
           "expand": 2, "d_conv": 4, "bd_lru_only": False, "disable_conv1d": False,
           "disable_ffn": False, "MAX_ITEM_LIST_LENGTH": 50}
    torch.manual_seed(0)
    return RecBLR(cfg, SyntheticDataset(n_items)).to(cuda).eval()


def test_model_full_sort_topk(cuda):
    from datamining_recblr_amd.distributed import synthetic_interaction

    model = _model(cuda)
    B, k = 257, 20
    inter = synthetic_interaction(B, 50, 3000, cuda, seed=7)
    with torch.no_grad():
        S = model.full_sort_predict(inter).cpu()
        gt, _ = model.full_sort_rank(inter)
    got = model.full_sort_topk(inter, k=k)
    assert not got[1].requires_grad
    seen = inter["item_id_list"]
    _same(got, _reference(S, k, 1, seen), "exclude_seen")
    assert not (got[0][:, :, None] == seen[:, None, :]).any()
    # without exclusion: the target is listed iff its position is below k
    got = model.full_sort_topk(inter, k=k, exclude_seen=False)
    _same(got, _reference(S, k, 1), "all items")
    t = inter["item_id"].cpu()
    ts = S.gather(1, t[:, None])
    cols = torch.arange(S.shape[1])[None, :]
    pos = gt.cpu() + ((S == ts) & (cols >= 1) & (cols < t[:, None])).sum(1)
    listed = (got[0].cpu() == t[:, None]).any(1)
    assert torch.equal(listed, pos < k)
    at = (got[0].cpu() == t[:, None]).float().argmax(1)
    assert torch.equal(at[listed], pos[listed])


def test_recommend_matches_per_user_loop(cuda, monkeypatch):
    """evaluation.recommend over users of mixed lengths against a batch-1
    loop.  Where a user's batched and batch-1 forwards give bit-equal scores
    the lists are equal; elsewhere (a GEMM path that depends on the batch
    composition) scores agree within the fp32 dot-product bound
    d * 2^-23 * sum|a||b| and only items closer than that bound swap."""
    from datamining_recblr_amd import evaluation, kernels, scoring

    model = _model(cuda)
    table = model.item_embedding.weight.detach()
    g = torch.Generator(device="cpu").manual_seed(21)
    n, k = 40, 10
    lengths = [1, 50, 2, 49] + torch.randint(1, 51, (n - 4,), generator=g).tolist()
    users = [torch.randint(1, 3000, (L,), generator=g).tolist() for L in lengths]
    outs = []

    def spy(out, *a, **kw):
        outs.append(out.detach().clone())
        return scoring.top_items(out, *a, **kw)

    monkeypatch.setattr(evaluation, "top_items", spy)
    model.train()
    ids, sc = evaluation.recommend(model, users, k=k, batch_size=16)
    assert model.training
    model.eval()
    assert ids.shape == (n, k) and sc.shape == (n, k) and len(outs) == 3
    order = torch.argsort(torch.tensor(lengths), stable=True)
    batched = torch.empty((n, table.shape[1]), device=cuda)
    batched[order.to(cuda)] = torch.cat(outs)
    d = table.shape[1]
    n_exact = 0
    for u, row in enumerate(users):
        seq = torch.tensor([row], device=cuda)
        with torch.no_grad():
            out = model.forward(seq, torch.tensor([len(row)], device=cuda), exact_lengths=True)
        one = scoring.top_items(out, table, k, first_item=1, exclude=seq)
        Su = kernels.item_scores(out, table)[0]
        Sb = kernels.item_scores(batched[u:u + 1].contiguous(), table)[0]
        ri, rs = ids[u], sc[u]
        assert not set(ri.tolist()) & (set(row) | {0})
        if torch.equal(Su.view(torch.int32), Sb.view(torch.int32)):
            n_exact += 1
            assert torch.equal(ri, one[0][0].cpu())
            assert torch.equal(rs.view(torch.int32), one[1][0].cpu().view(torch.int32))
            continue
        bound = ((out[0].double().abs() @ table.double().abs().t()) * (d * 2.0 ** -23)).cpu()
        Su = Su.double().cpu()
        assert ((rs.double() - Su[ri]).abs() <= bound[ri]).all(), u
        oi = one[0][0].cpu()
        moved = ri != oi
        gap = (Su[ri[moved]] - Su[oi[moved]]).abs()
        assert (gap < torch.maximum(bound[ri[moved]], bound[oi[moved]])).all(), u
    print(f"recommend: {n_exact} of {n} users with bit-equal batched and batch-1 scores")

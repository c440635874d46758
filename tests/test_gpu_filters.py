"""GPU tests of catalogue filters: the allow-bitmaps of rb_item_topk_allowed and
rb_item_rank_allowed (k_item_topk_allowed / k_item_rank_allowed in
csrc/item_scores.hip) and what passes them through: scoring.top_items,
scoring.target_ranks, RecBLR.full_sort_topk, evaluation.recommend and
RecBLR.session_recommend.

Everything is exact.  The reference is the score kernel's matrix
(kernels.item_scores), each row reduced to the ascending list of its selectable
ids (columns below first_item, excluded ids, NaN scores and what the row's
filter drops removed) and ordered by a stable descending sort; the filter is
applied to it as a bool matrix built row by row in Python, never through the
bitmaps.  Ids are compared with torch.equal and scores bit for bit.

Shapes are the smallest at which the kernels can go wrong: V = 300 has a partial
last tile and item splits of one tile, V = 20,000 more than 512 tiles (splits of
several tiles, so the filter words of a split's range matter), B = 5 a partial
wave tile and B = 130 a second, nearly empty workgroup; k = 1, 10, 64 covers
both list capacities."""
import pytest
import torch

from datamining_recblr_amd import evaluation, kernels, scoring

pytestmark = pytest.mark.gpu

NINF = float("-inf")
SHAPES = [(5, 300, 16), (130, 300, 16), (5, 300, 128), (130, 300, 128), (130, 20000, 16)]
KS = (1, 10, 64)
TWINS = (3, 40, 41)      # equal table rows: an exact tie
NAN_ITEM = 50
FILTERS = ("ones", "empty", "one", "few", "half", "last_tile")


def bits(x):
    return x.contiguous().view(torch.int32)


_cache = {}


def _case(B, V, d, cuda):
    """(seq, W, score matrix on the CPU, exclude list, filter masks [6, V]) of a
    shape, built once per session and never changed."""
    key = (B, V, d)
    if key in _cache:
        return _cache[key]
    g = torch.Generator().manual_seed(B * 7 + V * 3 + d)
    seq = torch.randn(B, d, generator=g)
    W = torch.randn(V, d, generator=g)
    W[TWINS[1]] = W[TWINS[0]]
    W[TWINS[2]] = W[TWINS[0]]
    seq[0] += 2.0 * W[TWINS[0]]           # row 0 ranks the twins near the top
    W[NAN_ITEM] = float("nan")
    seq, W = seq.to(cuda), W.to(cuda)
    S = kernels.item_scores(seq, W).cpu()
    masks = torch.zeros((len(FILTERS), V), dtype=torch.bool)
    masks[0] = True
    masks[2, 171] = True
    masks[3, [2, 64, 171, V - 1]] = True                      # fewer than k = 10 items
    masks[4] = torch.rand(V, generator=g) < 0.5
    masks[4, list(TWINS)] = torch.tensor([True, False, True])  # the tie crosses the boundary
    masks[5, (V - 1) // 32 * 32 + 1:] = True                   # only the last (partial) tile
    masks[:, NAN_ITEM] = True                                  # allowed, never selected
    masks[1] = False
    ex = torch.randint(1, V, (B, 12), generator=g)
    ex[:, 0] = TWINS[2]                   # excluded, and allowed by "half"
    ex[:, 1] = 171
    ex[:, 3], ex[:, 4], ex[:, 5] = -1, V, V + 7
    ex[:, 8:] = 0
    _cache[key] = (seq, W, S, ex, masks)
    return _cache[key]


def _allowed(masks, rows, B):
    """bool [B, V], one row at a time: rows None is filter 0 everywhere, -1 no
    filter, a value outside [-1, F) nothing."""
    F, V = masks.shape
    out = torch.zeros((B, V), dtype=torch.bool)
    for b in range(B):
        f = 0 if rows is None else int(rows[b])
        if f == -1:
            out[b] = True
        elif 0 <= f < F:
            out[b] = masks[f]
    return out


def _reference(S, k, first_item, exclude, allowed):
    B, V = S.shape
    ids = torch.full((B, k), -1, dtype=torch.int64)
    sc = torch.full((B, k), NINF, dtype=torch.float32)
    for b in range(B):
        keep = ~torch.isnan(S[b]) & allowed[b]
        keep[:first_item] = False
        if exclude is not None:
            e = exclude[b]
            keep[e[(e >= 0) & (e < V)]] = False
        idx = torch.nonzero(keep)[:, 0]          # ascending ids
        order = torch.sort(S[b, idx], descending=True, stable=True).indices[:k]
        n = order.numel()
        ids[b, :n] = idx[order]
        sc[b, :n] = S[b, idx[order]]
    return ids, sc


def _same(got, ref, what):
    ids, sc = got[0].cpu(), got[1].cpu()
    assert ids.dtype == torch.int64 and sc.dtype == torch.float32
    assert ids.shape == ref[0].shape and sc.shape == ref[1].shape
    assert torch.equal(ids, ref[0]), f"{what}: ids differ in rows " \
        f"{torch.nonzero((ids != ref[0]).any(1))[:8, 0].tolist()}"
    assert torch.equal(bits(sc), bits(ref[1])), f"{what}: scores differ"


def _mixed_rows(B):
    """Filters 0, 1, 2, no filter and out-of-range values inside one wave."""
    rows = torch.arange(B) % 3
    rows[1::5] = -1
    rows[min(3, B - 1)] = 3
    if B > 40:
        rows[17], rows[40], rows[B - 1] = -2, 1 << 40, -(1 << 40)
    return rows


# ---- top-k -----------------------------------------------------------------------------
@pytest.mark.parametrize("B,V,d", SHAPES)
def test_topk_mixed_filters_in_one_wave(cuda, B, V, d):
    seq, W, S, ex, masks = _case(B, V, d, cuda)
    bank = masks[[4, 3, 5]]                          # half, few, last tile: F = 3
    allow = scoring.item_filters(bank, device=cuda)
    rows = _mixed_rows(B)
    assert {-1, 0, 1, 2, 3} <= set(rows[:64].tolist())
    allowed = _allowed(bank, rows, B)
    plain = {}
    for first_item in (0, 1):
        for exclude in (None, ex):
            ref = _reference(S, max(KS), first_item, exclude, allowed)
            for k in KS:
                what = f"first_item={first_item} ex={exclude is not None} k={k}"
                exc = None if exclude is None else exclude.to(cuda)
                got = kernels.item_topk(seq, W, k, first_item=first_item, exclude=exc,
                                        allow=allow.words, allow_rows=rows.to(cuda))
                _same(got, (ref[0][:, :k], ref[1][:, :k]), what)
                # the -1 rows: the unfiltered kernel's rows, bit for bit
                free = kernels.item_topk(seq, W, k, first_item=first_item, exclude=exc)
                none = rows == -1
                assert torch.equal(got[0][none], free[0][none]), what
                assert torch.equal(bits(got[1][none]), bits(free[1][none])), what
                plain[(first_item, exclude is None, k)] = free
    ids = kernels.item_topk(seq, W, 64, first_item=0, allow=allow.words,
                            allow_rows=rows.to(cuda))[0].cpu()
    # out-of-range rows select nothing; "few" rows end in a -1 tail
    assert (ids[(rows < -1) | (rows > 2)] == -1).all()
    few = allowed.sum(1) - allowed[:, NAN_ITEM].long()
    assert (few[rows == 1] == 4).all() and ((ids[rows == 1] >= 0).sum(1) == 4).all()
    # the tie: row 0 (filter "half") lists twins 3 and 41 in id order, never 40
    assert rows[0] == 0
    row0 = ids[0].tolist()
    assert TWINS[1] not in row0 and row0.index(TWINS[0]) + 1 == row0.index(TWINS[2])
    assert not (ids == NAN_ITEM).any()
    # the all-ones filter, and every row at -1: the unfiltered result bitwise
    ones = scoring.item_filters(masks[0], device=cuda)
    for (first_item, no_ex, k), free in plain.items():
        exc = None if no_ex else ex.to(cuda)
        for kw in (dict(allow=ones.words),
                   dict(allow=allow.words, allow_rows=torch.full((B,), -1, device=cuda))):
            got = kernels.item_topk(seq, W, k, first_item=first_item, exclude=exc, **kw)
            assert torch.equal(got[0], free[0]) and torch.equal(bits(got[1]), bits(free[1]))


@pytest.mark.parametrize("B,V,d", SHAPES)
def test_topk_each_filter_alone_without_rows(cuda, B, V, d):
    """F = 1 and allow_rows None, through scoring.top_items."""
    seq, W, S, ex, masks = _case(B, V, d, cuda)
    for f, name in enumerate(FILTERS):
        allow = scoring.item_filters(masks[f])            # on the CPU: top_items moves it
        allowed = _allowed(masks[f:f + 1], None, B)
        for first_item, exclude in ((1, None), (0, ex)):
            ref = _reference(S, max(KS), first_item, exclude, allowed)
            for k in KS:
                got = scoring.top_items(seq, W, k, first_item=first_item, exclude=exclude,
                                        allow=allow)
                _same(got, (ref[0][:, :k], ref[1][:, :k]), f"{name} k={k}")
        n = int(allowed[0, 1:].sum()) - (1 if name != "empty" else 0)   # less the NaN item
        ids = scoring.top_items(seq, W, 64, allow=allow)[0]
        assert ((ids >= 0).sum(1) == min(n, 64)).all(), name
        if name == "last_tile":
            assert (ids[ids >= 0] > (V - 1) // 32 * 32).all() and (ids >= 0).any()
        if name == "one":
            assert (ids[:, 0] == 171).all() and (ids[:, 1:] == -1).all()


def test_topk_equals_the_torch_path_on_the_kernels_scores(cuda):
    """scoring._top_items_torch run on the score matrix itself (scores times
    the identity are the scores, NaN-free data), filters through the bitmaps
    on both sides."""
    B, V, d = 130, 300, 128
    seq, W, _, ex, masks = _case(B, V, d, cuda)
    W = W.clone()
    W[NAN_ITEM] = 0.5
    S = kernels.item_scores(seq, W).cpu()
    allow = scoring.item_filters(masks[[4, 3, 5]], device=cuda)
    rows = _mixed_rows(B).to(cuda)
    for k in KS:
        got = scoring.top_items(seq, W, k, exclude=ex, allow=allow, allow_rows=rows)
        ref = scoring._top_items_torch(S, torch.eye(V), k, 1, ex, allow, rows)
        assert torch.equal(got[0].cpu(), ref[0]) and torch.equal(bits(got[1].cpu()), bits(ref[1])), k


def test_topk_deterministic(cuda):
    seq, W, _, ex, masks = _case(130, 20000, 16, cuda)
    allow = scoring.item_filters(masks[[4, 3, 5]], device=cuda)
    rows = _mixed_rows(130).to(cuda)
    a = scoring.top_items(seq, W, 64, exclude=ex, allow=allow, allow_rows=rows)
    b = scoring.top_items(seq, W, 64, exclude=ex, allow=allow, allow_rows=rows)
    assert torch.equal(a[0], b[0]) and torch.equal(bits(a[1]), bits(b[1]))


# ---- ranks -----------------------------------------------------------------------------
@pytest.mark.parametrize("B,V,d", SHAPES)
def test_ranks_count_allowed_items_only(cuda, B, V, d):
    seq, W, S, _, masks = _case(B, V, d, cuda)
    bank = masks[[4, 3, 5]]
    allow = scoring.item_filters(bank, device=cuda)
    rows = _mixed_rows(B)
    allowed = _allowed(bank, rows, B)
    g = torch.Generator().manual_seed(V + B)
    target = torch.randint(1, V, (B,), generator=g)
    for b in range(0, B, 2):                        # every other row: a target its filter allows
        ok = torch.nonzero(allowed[b, 1:])[:, 0] + 1
        ok = ok[ok != NAN_ITEM]
        if ok.numel():
            target[b] = ok[int(torch.randint(0, ok.numel(), (1,), generator=g))]
    target[0] = TWINS[0]                            # ties with 41 (allowed) and 40 (not)
    target[4 if B == 5 else 6] = V + 3              # out of range, under a filter / under -1
    cols = torch.arange(V)[None, :]
    tc = target.clamp(0, V - 1)
    ts = S.gather(1, tc[:, None])
    for first_item in (0, 1):
        ok = allowed & (cols >= first_item) & (cols != target[:, None])
        want_gt, want_eq = (ok & (S > ts)).sum(1), (ok & (S == ts)).sum(1)
        bad = (target >= V) | ~allowed.gather(1, tc[:, None])[:, 0] | torch.isnan(ts[:, 0])
        want_gt[bad], want_eq[bad] = -1, -1
        a = scoring.target_ranks(seq, W, target.to(cuda), first_item, allow=allow,
                                 allow_rows=rows)          # rows on the CPU: moved
        assert torch.equal(a[0].cpu(), want_gt) and torch.equal(a[1].cpu(), want_eq), first_item
        b2 = scoring.target_ranks(seq, W, target.to(cuda), first_item, allow=allow,
                                  allow_rows=rows.to(cuda))
        assert torch.equal(a[0], b2[0]) and torch.equal(a[1], b2[1])      # two runs, same bits
        # -1 rows: the unfiltered ranks
        free = scoring.target_ranks(seq, W, target.to(cuda), first_item)
        none = rows == -1
        assert torch.equal(a[0][none], free[0][none]) and torch.equal(a[1][none], free[1][none])
        ones = scoring.item_filters(masks[0], device=cuda)
        full = scoring.target_ranks(seq, W, target.to(cuda), first_item, allow=ones)
        assert torch.equal(full[0], free[0]) and torch.equal(full[1], free[1])
    assert bad.any() and (~bad).any() and want_eq[0] == 1
    disallowed = ~allowed.gather(1, tc[:, None])[:, 0] & (target < V)
    assert disallowed.any() and (a[0].cpu()[disallowed] == -1).all()
    assert (a[1].cpu()[disallowed] == -1).all()


# ---- the model, the evaluator, the session call -------------------------------------------
N_ITEMS, MAX_LEN, N_SLOTS, S_RING = 60, 12, 8, 6


@pytest.fixture(scope="module")
def tiny(cuda):
    """d = 16, 2 layers, 60 items; its filters: the even ids, ids below 20, none."""
    from datamining_recblr_amd.model import RecBLR
    from datamining_recblr_amd.recbole_compat import SyntheticDataset

    cfg = dict(hidden_size=16, loss_type="CE", num_layers=2, dropout_prob=0.0, expand=2,
               d_conv=4, bd_lru_only=False, disable_conv1d=False, disable_ffn=False,
               MAX_ITEM_LIST_LENGTH=MAX_LEN)
    torch.manual_seed(0)
    model = RecBLR(cfg, SyntheticDataset(N_ITEMS)).eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():   # off the init's N(0, 0.02): scores well apart
        for name, p in model.named_parameters():
            if "Lambda" not in name and "conv1d" not in name and p.dim() == 2:
                p.mul_(3.0)
            elif name.endswith("bias"):
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    masks = torch.zeros((3, N_ITEMS), dtype=torch.bool)
    masks[0, ::2] = True
    masks[1, :20] = True
    return model.to(cuda), masks, scoring.item_filters(masks, device=cuda)


def _on_scores(out, table, k, exclude, allow, rows):
    """The torch path on the kernel's scores of these seq_output rows (on the
    CPU: scores times the identity are the scores, bit for bit)."""
    S = kernels.item_scores(out.contiguous(), table).cpu()
    ids, sc = scoring._top_items_torch(S, torch.eye(table.shape[0]), k, 1, exclude, allow, rows)
    return ids.to(out.device), sc.to(out.device)


def test_model_full_sort_topk_and_rank_with_filters(cuda, tiny):
    model, masks, allow = tiny
    table = model.item_embedding.weight.detach()
    B, k = 9, 10
    g = torch.Generator().manual_seed(3)
    lens = torch.randint(1, MAX_LEN + 1, (B,), generator=g)
    seq = torch.randint(1, N_ITEMS, (B, MAX_LEN), generator=g) * (torch.arange(MAX_LEN)[None]
                                                                  < lens[:, None])
    rows = torch.tensor([0, 1, 2, -1, 3, 0, 1, -1, 0])
    inter = {"item_id_list": seq.to(cuda), "item_length": lens.to(cuda),
             "item_id": torch.randint(1, N_ITEMS, (B,), generator=g).to(cuda)}
    with torch.no_grad():
        out = model.forward(inter["item_id_list"], inter["item_length"])
    for exclude_seen in (True, False):
        got = model.full_sort_topk(inter, k=k, exclude_seen=exclude_seen, allow=allow,
                                   allow_rows=rows)
        ref = _on_scores(out, table, k, inter["item_id_list"] if exclude_seen else None, allow,
                         rows.to(cuda))
        assert torch.equal(got[0], ref[0]) and torch.equal(bits(got[1]), bits(ref[1]))
    ids = got[0].cpu()
    assert (ids[[2, 4]] == -1).all() and (ids[0][ids[0] >= 0] % 2 == 0).all()
    assert (ids[1] < 20).all() and (ids[1] >= 1).all() and (ids[3] >= 1).all()
    gt, eq = model.full_sort_rank(inter, allow=allow, allow_rows=rows)
    S = kernels.item_scores(out.contiguous(), table).cpu()
    allowed = _allowed(masks, rows, B)
    t = inter["item_id"].cpu()
    ts = S.gather(1, t[:, None])
    cols = torch.arange(N_ITEMS)[None, :]
    ok = allowed & (cols >= 1) & (cols != t[:, None])
    bad = ~allowed.gather(1, t[:, None])[:, 0]
    assert torch.equal(gt.cpu(), (ok & (S > ts)).sum(1).masked_fill(bad, -1))
    assert torch.equal(eq.cpu(), (ok & (S == ts)).sum(1).masked_fill(bad, -1))
    m = evaluation.full_sort_metrics(model, [dict(inter, rows=rows)], topk=(5,), allow=allow,
                                     allow_rows_key="rows")
    assert m == scoring.rank_metrics(gt.cpu(), eq.cpu(), topk=(5,))


def test_recommend_filters_follow_users_through_the_length_sort(cuda, tiny, monkeypatch):
    model, masks, allow = tiny
    table = model.item_embedding.weight.detach()
    g = torch.Generator().manual_seed(5)
    n, k = 11, 8
    lengths = [7, 1, 12, 3, 3, 9, 2, 12, 5, 1, 6]
    users = [torch.randint(1, N_ITEMS, (L,), generator=g).tolist() for L in lengths]
    rows = torch.tensor([0, 1, -1, 2, 0, 1, 0, 5, 1, 0, -1])
    calls = []

    def spy(out, *a, **kw):
        calls.append((out.detach().clone(), kw["exclude"].clone(), kw["allow_rows"].clone()))
        return scoring.top_items(out, *a, **kw)

    monkeypatch.setattr(evaluation, "top_items", spy)
    ids, sc = evaluation.recommend(model, users, k=k, batch_size=4, allow=allow, allow_rows=rows)
    order = torch.argsort(torch.tensor(lengths), stable=True)
    assert len(calls) == 3 and order.tolist() != list(range(n))
    for i, (out, ex, r) in enumerate(calls):
        idx = order[4 * i:4 * i + 4]
        assert torch.equal(r.cpu(), rows[idx])            # each user kept their own filter
        ref = _on_scores(out, table, k, ex, allow, rows[idx].to(cuda))
        assert torch.equal(ids[idx], ref[0].cpu())
        assert torch.equal(bits(sc[idx]), bits(ref[1].cpu()))
    for u in range(n):
        row = ids[u][ids[u] >= 0]
        assert not set(row.tolist()) & (set(users[u]) | {0})
        if rows[u] == 0:
            assert (row % 2 == 0).all() and row.numel() > 0
        elif rows[u] == 1:
            assert (row < 20).all() and row.numel() > 0
        elif rows[u] == -1:
            assert row.numel() == k
        else:
            assert row.numel() == 0


def test_session_recommend_with_filters(cuda, tiny):
    model, masks, allow = tiny
    table = model.item_embedding.weight.detach()
    k = 10
    state = model.session_open(N_SLOTS, MAX_LEN, history=S_RING)
    twin = model.session_open(N_SLOTS, MAX_LEN, history=S_RING)
    slots = torch.tensor([5, 0, 3, N_SLOTS, 6, 2], device=cuda)   # N_SLOTS: outside the state
    rows = torch.tensor([0, 1, -1, 0, 1, 2], device=cuda)
    g = torch.Generator().manual_seed(9)
    seq = torch.randint(1, N_ITEMS, (6, 4), generator=g).to(cuda)
    seq[4] = 0                                                    # slot 6: never an event
    live, dead = [0, 1, 2, 5], [3, 4]
    for t in range(3):
        got = model.session_recommend(state, seq[:, t], slots, k=k, allow=allow, allow_rows=rows)
        y = model.session_step(twin, seq[:, t], slots)
        seen = twin.items[slots.clamp(0, N_SLOTS - 1)]
        ref = _on_scores(y, table, k, seen, allow, rows)
        assert torch.equal(got[0][live], ref[0][live])
        assert torch.equal(bits(got[1][live]), bits(ref[1][live]))
        assert (got[0][dead] == -1).all() and (got[1][dead] == NINF).all()
    ids = got[0].cpu()
    assert (ids[0][ids[0] >= 0] % 2 == 0).all() and (ids[0] >= 0).any()
    assert (ids[1][ids[1] >= 0] < 20).all() and (ids[2] >= 1).all() and (ids[5] == -1).all()
    assert not (got[0][live][:, :, None] == seq[live][:, None, :3]).any()
    # no event: the stored rows, the same filters
    again = model.session_recommend(state, None, slots, k=k, allow=allow, allow_rows=rows)
    assert torch.equal(again[0], got[0]) and torch.equal(bits(again[1]), bits(got[1]))
    assert torch.equal(state.items, twin.items) and torch.equal(state.count, twin.count)

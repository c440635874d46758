"""GPU tests of diversity caps: rb_item_topk_grouped (k_item_topk_grouped and
k_topk_rows_grouped in csrc/item_scores.hip) and what passes the cap through:
scoring.top_items, RecBLR.full_sort_topk, evaluation.recommend and
RecBLR.session_recommend.

Everything is exact.  The reference is the defining walk over the score kernel's
matrix (kernels.item_scores): each row's selectable ids (columns below
first_item, excluded ids, NaN scores and what the row's filter drops removed) in
(score descending, id ascending) order, walked in Python with a count per group;
the groups come from a Python list, never through ItemGroups.ids, and the filter
is a bool matrix built row by row.  Ids are compared with torch.equal and scores
bit for bit.

Shapes: V = 300 has a partial last tile and item splits of one tile, V = 20,000
splits of several tiles, B = 5 a partial wave tile and B = 130 a second, nearly
empty workgroup, d = 256 the instantiation with the least LDS to spare; k = 1,
10, 64 covers both list capacities.

Rows with a purpose (all shapes): row 0 leans on the mean of the "hot" items
(ids with id % 7 == 5, which share a table offset), so they fill its uncapped
list and a cap on them binds with the list full; row 1's scores rise with the id
(feature 0 is a ramp that only rows 1 and 2 read), so every tile brings
admissions and a group fills while the list still has empty slots; row 2's fall;
row 3 leans on the twins (equal table rows: exact ties)."""
import pytest
import torch

from datamining_recblr_amd import evaluation, kernels, scoring

pytestmark = pytest.mark.gpu

NINF = float("-inf")
SHAPES = [(5, 300, 16), (130, 300, 16), (5, 300, 128), (130, 300, 128), (130, 20000, 16),
          (5, 300, 256)]
KS = (1, 10, 64)
MS = (1, 2, 5, 64)
TWINS = (3, 40, 41)
NAN_ITEM = 50
HOT = 5                      # the hot items: id % 7 == HOT


def _layouts(V):
    """name -> Python list [V] of group ids."""
    return {
        "one": [0] * V,
        "mod7": [v % 7 for v in range(V)],
        "own": list(range(V)),
        "none": [-1] * V,
        "blocks32": [v // 32 for v in range(V)],        # a group inside one tile
        "blocks352": [v // 352 for v in range(V)],      # ... inside one split of 11 tiles
        "mod3_free": [-1 if v % 5 == 0 else v % 3 for v in range(V)],
    }


LAYOUTS = tuple(_layouts(1))
TAILS = ("one", "mod7", "blocks352")     # layouts that cannot fill 64 entries at m = 1


def bits(x):
    return x.contiguous().view(torch.int32)


_cache = {}


def _case(B, V, d, cuda):
    """(seq, W, score matrix on the CPU, exclude list, filter masks [3, V]) of a
    shape, built once per session and never changed."""
    key = (B, V, d)
    if key in _cache:
        return _cache[key]
    g = torch.Generator().manual_seed(B * 7 + V * 3 + d)
    seq = torch.randn(B, d, generator=g)
    W = torch.randn(V, d, generator=g)
    ids = torch.arange(V)
    hot = ids % 7 == HOT
    u = torch.randint(0, 2, (d,), generator=g).float() * 2 - 1
    u[0] = 0.0
    W[hot] += 2.5 * u
    seq[0] += 4.0 * W[hot].mean(0)
    W[TWINS[0]] *= 3.0                     # long rows: nothing random comes near them
    seq[3] += 2.0 * W[TWINS[0]]
    seq[3] -= (seq[3] @ u) / (u @ u) * u   # ... nor the hot items' offset
    seq[:, 0] = 0.0
    seq[1, 0], seq[2, 0] = 1.0, -1.0
    W[:, 0] = ids.float() * d ** 0.5 / 12.0   # 2.7 score deviations per 32-item tile
    W[TWINS[1]] = W[TWINS[0]]
    W[TWINS[2]] = W[TWINS[0]]
    W[NAN_ITEM] = float("nan")
    seq, W = seq.to(cuda), W.to(cuda)
    S = kernels.item_scores(seq, W).cpu()
    masks = torch.zeros((3, V), dtype=torch.bool)
    masks[0] = torch.rand(V, generator=g) < 0.5
    masks[0, list(TWINS)] = torch.tensor([True, False, True])   # a twin dropped by the filter
    masks[1, [2, 64, 171, V - 1]] = True                        # fewer than k = 10 items
    masks[2, (V - 1) // 32 * 32 + 1:] = True                    # only the last (partial) tile
    masks[:, NAN_ITEM] = True                                   # allowed, never selected
    ex = torch.randint(1, V, (B, 12), generator=g)
    ex[:, 0] = TWINS[2]                   # a twin excluded (and allowed by filter 0)
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


def _mixed_rows(B):
    """Filters 0, 1, 2, no filter and out-of-range values inside one wave; rows
    0 to 3 (the rows with a purpose) keep filter 0 or none."""
    rows = torch.arange(B) % 3
    rows[:4] = torch.tensor([0, -1, 0, -1])
    if B > 40:
        rows[6::5] = -1
        rows[7], rows[17], rows[40], rows[B - 1] = 3, -2, 1 << 40, -(1 << 40)
    return rows


_orders = {}


def _order(S, first_item, exclude, allowed):
    """Per row the selectable ids by (score descending, id ascending), as lists;
    kept per (score matrix, arguments): every layout walks the same orders (the
    matrix is kept with them, so its id stays its own)."""
    key = (id(S), first_item, exclude is not None, allowed is not None)
    if key in _orders:
        return _orders[key][1]
    B, V = S.shape
    out = []
    for b in range(B):
        keep = ~torch.isnan(S[b])
        if allowed is not None:
            keep &= allowed[b]
        keep[:first_item] = False
        if exclude is not None:
            e = exclude[b]
            keep[e[(e >= 0) & (e < V)]] = False
        idx = torch.nonzero(keep)[:, 0]          # ascending ids
        out.append(idx[torch.sort(S[b, idx], descending=True, stable=True).indices].tolist())
    _orders[key] = (S, out)
    return out


def _walk(S, first_item, exclude, allowed, group_of, kmax=max(KS), mmax=max(MS)):
    """Per row the walk's record [(id, n)]: the selectable items in order, n the
    number of its group walked before it (0 for group -1).  Under a cap m <=
    mmax the row's list is the first k <= kmax ids with n < m.  The walk stops
    when nothing later can enter such a list: kmax items with n = 0 are on
    record (they pass every cap), or every group that exists has mmax on
    record and no item is free of a cap."""
    sizes = {}
    for g in group_of:
        sizes[g] = sizes.get(g, 0) + 1
    n_groups = len([g for g in sizes if g != -1])
    out = []
    for order in _order(S, first_item, exclude, allowed):
        seen, rec, first, done = {}, [], 0, 0
        for v in order:
            g = group_of[v]
            n = 0
            if g != -1:
                n = seen.get(g, 0)
                seen[g] = n + 1
                done += n + 1 == mmax
            first += n == 0
            if n < mmax:
                rec.append((v, n))
            if first >= kmax or (done == n_groups and -1 not in sizes):
                break
        out.append(rec)
    return out


def _lists(S, rec, k, m):
    B = S.shape[0]
    ids = torch.full((B, k), -1, dtype=torch.int64)
    sc = torch.full((B, k), NINF, dtype=torch.float32)
    for b in range(B):
        got = [v for v, n in rec[b] if n < m][:k]
        ids[b, :len(got)] = torch.tensor(got, dtype=torch.int64)
        sc[b, :len(got)] = S[b, got]
    return ids, sc


def _same(got, ref, what):
    ids, sc = got[0].cpu(), got[1].cpu()
    assert ids.dtype == torch.int64 and sc.dtype == torch.float32
    assert ids.shape == ref[0].shape and sc.shape == ref[1].shape
    assert torch.equal(ids, ref[0]), f"{what}: ids differ in rows " \
        f"{torch.nonzero((ids != ref[0]).any(1))[:8, 0].tolist()}"
    assert torch.equal(bits(sc), bits(ref[1])), f"{what}: scores differ"


def _groups(group_of, cuda):
    return scoring.item_groups(group_of, device=cuda)


# ---- the kernel against the walk ------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("B,V,d", SHAPES)
def test_capped_topk_is_the_walk(cuda, B, V, d, layout):
    """Every k and m, alone and with exclude, first_item 0 and mixed filters in
    one wave (-1 and out-of-range rows included)."""
    seq, W, S, ex, masks = _case(B, V, d, cuda)
    group_of = _layouts(V)[layout]
    groups = _groups(group_of, cuda)
    rows = _mixed_rows(B)
    allow = scoring.item_filters(masks, device=cuda)
    full = tail = 0
    for first_item, exclude, filtered in ((1, None, False), (0, ex, True), (1, ex, False)):
        allowed = _allowed(masks, rows, B) if filtered else None
        rec = _walk(S, first_item, exclude, allowed, group_of)
        exc = None if exclude is None else exclude.to(cuda)
        kw = dict(allow=allow.words, allow_rows=rows.to(cuda)) if filtered else {}
        for k in KS:
            plain = kernels.item_topk(seq, W, k, first_item=first_item, exclude=exc, **kw)
            for m in MS:
                what = f"{layout} first_item={first_item} ex={exclude is not None} " \
                       f"filtered={filtered} k={k} m={m}"
                ref = _lists(S, rec, k, m)
                got = kernels.item_topk(seq, W, k, first_item=first_item, exclude=exc,
                                        groups=groups.ids, max_per_group=m, **kw)
                _same(got, ref, what)
                if m >= k or layout in ("own", "none"):
                    # a cap that cannot bind: the uncapped kernel's result, bit for bit
                    assert torch.equal(got[0], plain[0]), what
                    assert torch.equal(bits(got[1]), bits(plain[1])), what
                if not filtered:
                    full += int((ref[0][:, -1] >= 0).sum()) if k == 64 else 0
                    tail += int((ref[0][:, -1] < 0).sum()) if m == 1 else 0
                    if layout == "one":
                        assert ((ref[0] >= 0).sum(1) == min(m, k)).all(), what
                    if layout == "mod7" and m == 1:
                        assert ((ref[0] >= 0).sum(1) == min(7, k)).all(), what
            assert not (got[0] == NAN_ITEM).any()
        if filtered:
            # out-of-range rows select nothing; filter 1 keeps four items
            ids = got[0].cpu()
            assert (ids[(rows < -1) | (rows > 2)] == -1).all()
            assert ((ids[rows == 1] >= 0).sum(1) <= 4).all()
    # the case is not hollow: lists of 64 do fill, and -1 tails appear where meant
    assert full > 0, layout
    few = layout in ("blocks32", "mod3_free") and V == 300     # 10 groups; 3 and 58 free items
    assert (tail > 0) == (layout in TAILS or few), layout


@pytest.mark.parametrize("B,V,d", [(5, 300, 16), (130, 20000, 16), (5, 300, 256)])
def test_rows_with_a_purpose(cuda, B, V, d):
    """The adversarial rows are what the module's text says, and the cap moves
    them as it must."""
    seq, W, S, ex, masks = _case(B, V, d, cuda)
    lay = _layouts(V)
    k = 10
    free = kernels.item_topk(seq, W, 64)[0].cpu()
    # row 0: the hot group fills the uncapped list (rule 1 on a full list)
    n_hot = len([v for v in range(1, V) if v % 7 == HOT and v not in TWINS])   # 40 is a twin
    assert (free[0, :min(64, n_hot)] % 7 == HOT).all()
    got = kernels.item_topk(seq, W, k, groups=_groups(lay["mod7"], cuda).ids,
                            max_per_group=2)[0].cpu()
    assert (got[0, :2] % 7 == HOT).all() and (got[0, 2:] % 7 != HOT).all()
    assert torch.equal(got[0, :2], free[0, :2])
    # rows 1 and 2: scores rising / falling with the id, tile after tile
    tiles = [t * 32 + 16 for t in range(V // 32) if not t * 32 <= NAN_ITEM < t * 32 + 32]
    means = torch.stack([S[:, c - 16:c + 16].mean(1) for c in tiles], 1)
    assert (means[1, 1:] > means[1, :-1]).all() and (means[2, 1:] < means[2, :-1]).all()
    assert (free[1, :k] >= V - 128).all() and (free[2, :k] < 128).all()
    # one group, rising scores: the list is the best m items, found last
    got = kernels.item_topk(seq, W, k, groups=_groups(lay["one"], cuda).ids, max_per_group=3)
    assert torch.equal(got[0][:, :3].cpu(), free[:, :3]) and (got[0][:, 3:] == -1).all()
    # row 3, the twins 3 = 40 = 41 lead it
    assert free[3, :3].tolist() == list(TWINS)
    same = _groups([9 if v in TWINS else -1 for v in range(V)], cuda).ids
    apart = _groups([TWINS.index(v) if v in TWINS else -1 for v in range(V)], cuda).ids
    a, b, c = TWINS
    ids = kernels.item_topk(seq, W, k, groups=same, max_per_group=1)[0].cpu()
    assert ids[3, 0] == a and not set(ids[3].tolist()) & {b, c}     # the smaller id wins
    assert torch.equal(ids[3, 1:], free[3, 3:k + 2])
    ids = kernels.item_topk(seq, W, k, groups=apart, max_per_group=1)[0].cpu()
    assert torch.equal(ids, free[:, :k])                            # different groups: all three
    ids = kernels.item_topk(seq, W, k, exclude=ex.to(cuda), groups=same,
                            max_per_group=1)[0].cpu()
    assert ids[3, 0] == a and b not in ids[3].tolist()              # c excluded: still a
    ids = kernels.item_topk(seq, W, k, first_item=4, groups=same, max_per_group=1)[0].cpu()
    assert ids[3, 0] == b and c not in ids[3].tolist()              # a out of range: b
    allow = scoring.item_filters(masks[0], device=cuda)             # drops b
    ids = scoring.top_items(seq, W, k, allow=allow, groups=scoring.item_groups(same.cpu()),
                            max_per_group=2)[0].cpu()
    assert ids[3, :2].tolist() == [a, c]
    ids = scoring.top_items(seq, W, k, first_item=4, allow=allow,
                            groups=scoring.item_groups(same.cpu()), max_per_group=1)[0].cpu()
    assert ids[3, 0] == c                                           # a out, b dropped: c


def test_capped_topk_deterministic(cuda):
    B, V, d = 130, 20000, 16
    seq, W, _, ex, masks = _case(B, V, d, cuda)
    allow = scoring.item_filters(masks, device=cuda)
    rows = _mixed_rows(B).to(cuda)
    for layout, m in (("mod7", 2), ("blocks352", 1), ("mod3_free", 5)):
        groups = _groups(_layouts(V)[layout], cuda)
        kw = dict(exclude=ex, allow=allow, allow_rows=rows, groups=groups, max_per_group=m)
        a = scoring.top_items(seq, W, 64, **kw)
        b = scoring.top_items(seq, W, 64, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(bits(a[1]), bits(b[1]))


def test_top_items_routes(cuda, monkeypatch):
    """Without groups: kernels.item_topk's arguments and bits as before.  With
    groups: the grouped entry point, the ItemGroups moved to the table's
    device; a group id beyond the kernel's 16 bits takes the torch path."""
    B, V, d = 5, 300, 16
    seq, W, S, ex, masks = _case(B, V, d, cuda)
    allow = scoring.item_filters(masks[0], device=cuda)
    calls = []
    real = kernels.item_topk

    def spy(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)

    monkeypatch.setattr(kernels, "item_topk", spy)
    for kw in (dict(), dict(exclude=ex), dict(exclude=ex, allow=allow)):
        got = scoring.top_items(seq, W, 10, **kw)
        assert not {"groups", "max_per_group"} & set(calls[-1])
        exc = kw["exclude"].to(cuda) if "exclude" in kw else None
        ref = real(seq, W, 10, exclude=exc, allow=allow.words if "allow" in kw else None)
        assert torch.equal(got[0], ref[0]) and torch.equal(bits(got[1]), bits(ref[1]))
    group_of = _layouts(V)["mod7"]
    n = len(calls)
    got = scoring.top_items(seq, W, 10, exclude=ex, groups=scoring.item_groups(group_of),
                            max_per_group=1)                       # groups on the CPU: moved
    assert len(calls) == n + 1 and calls[-1]["groups"].is_cuda and calls[-1]["max_per_group"] == 1
    _same(got, _lists(S, _walk(S, 1, ex, None, group_of), 10, 1), "top_items")
    far = [g * 70001 for g in group_of]                             # the same partition
    assert max(far) > kernels.ITEM_GROUP_ID_MAX
    n = len(calls)
    W2 = W.clone()
    W2[NAN_ITEM] = 0.5                                              # torch's matmul: no NaN row
    near = scoring.top_items(seq, W2, 10, exclude=ex, groups=scoring.item_groups(group_of),
                             max_per_group=1)
    calls.clear()
    torch_path = scoring.top_items(seq, W2, 10, exclude=ex, groups=scoring.item_groups(far),
                                   max_per_group=1)
    assert not calls                                                # no kernel launch
    assert torch_path[0].is_cuda and (torch_path[0] >= 0).sum() == (near[0] >= 0).sum()
    with pytest.raises(ValueError):
        real(seq, W, 10, groups=scoring.item_groups(group_of, device=cuda).ids)
    with pytest.raises(TypeError):
        real(seq, W, 10, groups=torch.tensor(group_of, device=cuda), max_per_group=1)   # int64


# ---- the model, the evaluator, the session call -------------------------------------------
N_ITEMS, MAX_LEN, N_SLOTS, S_RING = 60, 12, 8, 6
TINY_GROUPS = [-1 if v % 10 == 0 else v % 4 for v in range(N_ITEMS)]


@pytest.fixture(scope="module")
def tiny(cuda):
    """d = 16, 2 layers, 60 items (the filters tests' model); four groups and a
    few items free of any cap."""
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
    return model.to(cuda), scoring.item_groups(TINY_GROUPS, device=cuda)


def _on_scores(out, table, k, exclude, m, live=None):
    """The walk on the kernel's scores of these seq_output rows."""
    S = kernels.item_scores(out.contiguous(), table).cpu()
    ref = _lists(S, _walk(S, 1, None if exclude is None else exclude.cpu(), None, TINY_GROUPS),
                 k, m)
    return ref


def test_model_full_sort_topk_with_a_cap(cuda, tiny):
    model, groups = tiny
    table = model.item_embedding.weight.detach()
    B, k = 9, 10
    g = torch.Generator().manual_seed(3)
    lens = torch.randint(1, MAX_LEN + 1, (B,), generator=g)
    seq = torch.randint(1, N_ITEMS, (B, MAX_LEN), generator=g) * (torch.arange(MAX_LEN)[None]
                                                                  < lens[:, None])
    inter = {"item_id_list": seq.to(cuda), "item_length": lens.to(cuda)}
    with torch.no_grad():
        out = model.forward(inter["item_id_list"], inter["item_length"])
    for exclude_seen in (True, False):
        for m in (1, 2):
            got = model.full_sort_topk(inter, k=k, exclude_seen=exclude_seen, groups=groups,
                                       max_per_group=m)
            ref = _on_scores(out, table, k, seq if exclude_seen else None, m)
            _same(got, ref, f"exclude_seen={exclude_seen} m={m}")
    ids = got[0].cpu()                                  # m = 2, nothing excluded
    free = N_ITEMS // 10 - 1                            # ids 10 .. 50
    assert ((ids >= 0).sum(1) == k).all()
    for row in ids.tolist():
        capped = [TINY_GROUPS[v] for v in row if TINY_GROUPS[v] != -1]
        assert all(capped.count(q) <= 2 for q in range(4)) and len(capped) >= k - free
    one = model.full_sort_topk(inter, k=k, exclude_seen=False, groups=groups,
                               max_per_group=1)[0].cpu()
    assert ((one >= 0).sum(1) == 4 + free).all()        # a -1 tail under m = 1


def test_recommend_keeps_the_groups_through_the_length_sort(cuda, tiny, monkeypatch):
    model, groups = tiny
    table = model.item_embedding.weight.detach()
    g = torch.Generator().manual_seed(5)
    n, k, m = 11, 8, 1
    lengths = [7, 1, 12, 3, 3, 9, 2, 12, 5, 1, 6]
    users = [torch.randint(1, N_ITEMS, (L,), generator=g).tolist() for L in lengths]
    calls = []

    def spy(out, *a, **kw):
        calls.append((out.detach().clone(), kw["exclude"].clone(), kw["groups"],
                      kw["max_per_group"]))
        return scoring.top_items(out, *a, **kw)

    monkeypatch.setattr(evaluation, "top_items", spy)
    ids, sc = evaluation.recommend(model, users, k=k, batch_size=4,
                                   groups=scoring.item_groups(TINY_GROUPS), max_per_group=m)
    order = torch.argsort(torch.tensor(lengths), stable=True)
    assert len(calls) == 3 and order.tolist() != list(range(n))
    for i, (out, ex, gr, mm) in enumerate(calls):
        idx = order[4 * i:4 * i + 4]
        assert gr.ids.is_cuda and gr.ids.cpu().tolist() == TINY_GROUPS and mm == m
        ref = _on_scores(out, table, k, ex, m)
        assert torch.equal(ids[idx], ref[0]) and torch.equal(bits(sc[idx]), bits(ref[1]))
    for u in range(n):
        row = ids[u][ids[u] >= 0].tolist()
        assert not set(row) & (set(users[u]) | {0})
        capped = [TINY_GROUPS[v] for v in row if TINY_GROUPS[v] != -1]
        assert len(capped) == len(set(capped)) and len(row) >= 4


def test_session_recommend_with_a_cap(cuda, tiny):
    model, groups = tiny
    table = model.item_embedding.weight.detach()
    k, m = 10, 2
    state = model.session_open(N_SLOTS, MAX_LEN, history=S_RING)
    twin = model.session_open(N_SLOTS, MAX_LEN, history=S_RING)
    slots = torch.tensor([5, 0, 3, N_SLOTS, 6, 2], device=cuda)   # N_SLOTS: outside the state
    g = torch.Generator().manual_seed(9)
    seq = torch.randint(1, N_ITEMS, (6, 4), generator=g).to(cuda)
    seq[4] = 0                                                    # slot 6: never an event
    live, dead = [0, 1, 2, 5], [3, 4]
    for t in range(3):
        got = model.session_recommend(state, seq[:, t], slots, k=k, groups=groups,
                                      max_per_group=m)
        y = model.session_step(twin, seq[:, t], slots)
        seen = twin.items[slots.clamp(0, N_SLOTS - 1)]
        ref = _on_scores(y, table, k, seen, m)
        assert torch.equal(got[0][live].cpu(), ref[0][live])
        assert torch.equal(bits(got[1][live].cpu()), bits(ref[1][live]))
        assert (got[0][dead] == -1).all() and (got[1][dead] == NINF).all()
        # and top_items on forward()'s rows
        again = scoring.top_items(y, table, k, exclude=seen, groups=groups, max_per_group=m)
        assert torch.equal(got[0][live], again[0][live])
        assert torch.equal(bits(got[1][live]), bits(again[1][live]))
    for row in got[0][live].cpu().tolist():
        capped = [TINY_GROUPS[v] for v in row if v >= 0 and TINY_GROUPS[v] != -1]
        assert all(capped.count(q) <= m for q in range(4))
    assert torch.equal(state.items, twin.items) and torch.equal(state.count, twin.count)

"""Candidate-list scoring on the GPU (csrc/candidates.hip): rb_candidate_scores
against fp64, the bitwise rule the three kernels share, rb_candidate_topk
against scoring.order_candidates exactly, the fallback routing,
rb_candidate_ranks, and the model- and session-level calls built on them.

Shapes are the smallest at which each mechanism can still break: every
float4-count variant of the scoring core (d = 4 .. 512, with a partly filled
last vector at 68 and 260), C on both sides of the 16-candidate pass, of a
power of two and at the 4096 limit, lists that are nearly all duplicates and
lists with few."""
import pytest
import torch

from datamining_recblr_amd import kernels, scoring, session

from test_gpu_dense import close
from test_gpu_session import _model, _sequences

pytestmark = pytest.mark.gpu

NINF = float("-inf")


def bits(x):
    return x.contiguous().view(torch.int32)


def _case(cuda, B, C, d, V, seed=0, wide=8):
    """h [B, d] as a column slice of a [B, d + wide] buffer (ldh > d, still
    16-B aligned), table [V, d], cand [B, C] in [0, V)."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(B, d + wide, generator=g).to(cuda)
    h = buf[:, wide // 2:wide // 2 + d]
    table = torch.randn(V, d, generator=g).to(cuda)
    cand = torch.randint(0, V, (B, C), generator=g).to(cuda)
    return h, table, cand


# ---- 1. scores against fp64 ------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 64, 68, 128, 260, 512])
def test_scores_against_fp64(cuda, d):
    """|got - ref| <= d * 2^-23 * sum_i |h_i e_i| per pair: the any-order
    summation bound gamma_d = d u / (1 - d u), u = 2^-24, with a factor of two
    to spare."""
    V = 300
    for B in (1, 3, 65):
        for C in (1, 15, 16, 17, 257):
            h, table, cand = _case(cuda, B, C, d, V, seed=B * 1000 + C)
            assert h.stride(0) > d and not h.is_contiguous() or B == 1
            cand[0, 0] = -1
            cand[-1, -1] = V
            got = scoring.candidate_scores(h, table, cand)
            ok = (cand >= 0) & (cand < V)
            prod = h.double()[:, None, :] * table.double()[cand.clamp(0, V - 1)]
            ref, mag = prod.sum(-1), prod.abs().sum(-1)
            err = (got.double() - ref).abs()
            assert got.shape == (B, C) and got.dtype == torch.float32
            assert (got[~ok] == NINF).all() and int((~ok).sum()) == (1 if B * C == 1 else 2)
            assert (err[ok] <= d * 2.0 ** -23 * mag[ok]).all(), (B, C, float(err[ok].max()))


# ---- 2. the bitwise rule -----------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 260])
def test_a_pairs_score_has_the_same_bits_everywhere(cuda, d):
    V = 300
    h, table, cand = _case(cuda, 65, 257, d, V, seed=5)
    full = scoring.candidate_scores(h, table, cand)
    # a permuted list: permuted scores
    perm = torch.randperm(257, generator=torch.Generator().manual_seed(1)).to(cuda)
    assert torch.equal(bits(scoring.candidate_scores(h, table, cand[:, perm])), bits(full[:, perm]))
    # the same (row, id) alone, and inside one row's list of 4096
    b, c = 37, 101
    alone = scoring.candidate_scores(h[b:b + 1], table, cand[b:b + 1, c:c + 1])
    assert torch.equal(bits(alone)[0, 0], bits(full)[b, c])
    long = torch.randint(0, V, (1, 4096), generator=torch.Generator().manual_seed(2)).to(cuda)
    long[0, 4095] = cand[b, c]
    assert torch.equal(bits(scoring.candidate_scores(h[b:b + 1], table, long))[0, 4095],
                       bits(full)[b, c])
    # equal table rows tie exactly, for every h
    table[7] = table[250]
    pair = torch.tensor([[7, 250]], device=cuda).expand(65, 2)
    s = scoring.candidate_scores(h, table, pair)
    assert torch.equal(bits(s[:, 0]), bits(s[:, 1]))


@pytest.mark.parametrize("d", [64, 512])
def test_topk_and_ranks_compute_the_scores_kernels_bits(cuda, d):
    V, B, C = 300, 9, 100
    h, table, cand = _case(cuda, B, C, d, V, seed=6)
    scores = scoring.candidate_scores(h, table, cand)
    ids, top = scoring.top_candidates(h, table, cand, C)
    for b in range(B):
        n = int((ids[b] >= 0).sum())
        assert n == len(set(cand[b].tolist()))
        first = {int(i): c for c, i in reversed(list(enumerate(cand[b].tolist())))}
        assert torch.equal(bits(top[b, :n]), bits(scores[b, [first[int(i)] for i in ids[b, :n]]]))
    target = cand[:, 3].clone()
    gt, eq = scoring.candidate_ranks(h, table, target, cand, first_item=0)
    both = scoring.candidate_scores(h, table, torch.cat([target[:, None], cand], 1))
    st, s = both[:, :1], both[:, 1:]
    assert torch.equal(bits(s), bits(scores))
    other = cand != target[:, None]
    assert torch.equal(gt, (other & (s > st)).sum(1)) and torch.equal(eq, (other & (s == st)).sum(1))


# ---- 3. top-k, exact -----------------------------------------------------------------------
def _topk_case(cuda, C, V, d=64, seed=0):
    """B = 5 rows: row 1's h is NaN, row 3's list is all -1; the table holds 8
    pairs of identical rows; the lists hold ids -1 and V as well."""
    B = 5
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(B, d, generator=g)
    h[1] = float("nan")
    table = torch.randn(V, d, generator=g)
    twins = torch.randperm(V, generator=g)[:16]
    table[twins[8:]] = table[twins[:8]]
    cand = torch.randint(-1, V + 1, (B, C), generator=g)
    cand[3] = -1
    if C >= 17:                      # every twin in row 0's list: ties resolved by id
        cand[0, :16] = twins
    return h.to(cuda), table.to(cuda), cand.to(cuda), g


def _check_topk(h, table, cand, k, first_item, exclude):
    V = table.shape[0]
    ids, scores = scoring.top_candidates(h, table, cand, k, first_item, exclude)
    want = scoring.order_candidates(scoring.candidate_scores(h, table, cand), cand, k, first_item,
                                    exclude, num_items=V)
    assert ids.shape == (h.shape[0], k) and ids.dtype == torch.int64
    assert torch.equal(ids, want[0]), (cand.shape, k, first_item)
    assert torch.equal(scores, want[1]), (cand.shape, k, first_item)
    return ids, scores


@pytest.mark.parametrize("C,V", [(1, 300), (2, 300), (17, 300), (256, 300), (257, 300),
                                 (4096, 50), (4096, 6000)])
def test_topk_equals_order_candidates(cuda, C, V):
    h, table, cand, g = _topk_case(cuda, C, V, seed=C + V)
    for E in (0, 1, 200, 4096):
        exclude = torch.randint(-2, V + 2, (5, E), generator=g).to(cuda) if E else None
        for k in sorted({1, 10, C, C + 5}):
            for first_item in (0, 1):
                ids, scores = _check_topk(h, table, cand, k, first_item, exclude)
                # the NaN row and the empty row; their neighbours are live
                assert (ids[[1, 3]] == -1).all() and (scores[[1, 3]] == NINF).all()
    if V == 50:
        ids, _ = scoring.top_candidates(h, table, cand, 60, first_item=1)
        assert int((ids[0] >= 0).sum()) <= 49 and (ids[0, 49:] == -1).all()


def test_topk_is_deterministic_and_orders_ties_by_id(cuda):
    h, table, cand, g = _topk_case(cuda, 4096, 6000, seed=9)
    exclude = torch.randint(0, 6000, (5, 200), generator=g).to(cuda)
    a = scoring.top_candidates(h, table, cand, 4096, 1, exclude)
    b = scoring.top_candidates(h, table, cand, 4096, 1, exclude)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ids, scores = a[0][0], a[1][0]
    n = int((ids >= 0).sum())
    tied = scores[1:n] == scores[:n - 1]
    assert int(tied.sum()) >= 1                     # the twins met
    assert (ids[1:n][tied] > ids[:n - 1][tied]).all()
    assert (scores[1:n] <= scores[:n - 1]).all()


def test_topk_other_widths(cuda):
    for d in (4, 68, 128, 260, 512):
        h, table, cand, g = _topk_case(cuda, 257, 300, d=d, seed=d)
        _check_topk(h, table, cand, 10, 1, torch.randint(0, 300, (5, 7), generator=g).to(cuda))


# ---- 4. fallback routing -------------------------------------------------------------------
def test_routing_at_the_kernels_limits(cuda, monkeypatch):
    ran = []
    orig = kernels.candidate_topk

    def recorded(h, table, cand, k, **kw):
        ran.append((cand.shape[1], 0 if kw.get("exclude") is None else kw["exclude"].shape[1]))
        return orig(h, table, cand, k, **kw)

    monkeypatch.setattr(kernels, "candidate_topk", recorded)
    V = 6000
    h, table, cand, g = _topk_case(cuda, 4097, V, seed=3)
    ex = torch.randint(-2, V + 2, (5, 4097), generator=g).to(cuda)
    _check_topk(h, table, cand[:, :4096], 10, 1, ex[:, :4096])
    assert ran == [(4096, 4096)]
    _check_topk(h, table, cand, 10, 1, ex[:, :5])          # C = 4097: torch ops
    _check_topk(h, table, cand[:, :100], 10, 1, ex)        # E = 4097: torch ops
    assert ran == [(4096, 4096)]
    ids, scores = scoring.top_candidates(h, table, cand, 4100, 1, ex)
    assert ran == [(4096, 4096)] and ids.shape == (5, 4100)
    assert (ids[[1, 3]] == -1).all() and (scores[:, -3:] == NINF).all()
    # an unsupported width: torch ops as well
    h6, t6 = h[:, :6].contiguous(), table[:, :6].contiguous()
    assert not kernels.candidates_supported(h6, t6)
    _check_topk(h6, t6, cand[:, :100], 10, 1, None)
    assert ran == [(4096, 4096)]
    with pytest.raises(ValueError):
        orig(h, table, cand, 10)                           # the kernel itself refuses C = 4097


# ---- 5. ranks --------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 100, 5000])
def test_ranks(cuda, C):
    V, B, d = 300, 7, 64
    h, table, cand = _case(cuda, B, C, d, V, seed=C)
    target = torch.tensor([5, 17, 0, V, -1, 299, 40], device=cuda)
    cand[:, 0] = target.clamp(0, V - 1)                    # the target itself is listed: skipped
    if C >= 100:
        cand[:, 1:4] = cand[:, 4:5]                        # a repeated negative counts each time
        cand[:, 10] = -1
        table[int(cand[0, 4])] = table[5]                  # exact ties with row 0's target
    gt, eq = scoring.candidate_ranks(h, table, target, cand, first_item=1)
    both = scoring.candidate_scores(h, table, torch.cat([target.clamp(0, V - 1)[:, None], cand], 1))
    st, s = both[:, :1], both[:, 1:]
    ok = (cand >= 1) & (cand < V) & (cand != target[:, None])
    want_gt, want_eq = (ok & (s > st)).sum(1), (ok & (s == st)).sum(1)
    bad = [2, 3, 4]                                        # below first_item, = V, -1
    live = [0, 1, 5, 6]
    assert gt[bad].tolist() == [-1] * 3 and eq[bad].tolist() == [-1] * 3
    assert torch.equal(gt[live], want_gt[live]) and torch.equal(eq[live], want_eq[live])
    if C >= 100:
        assert int(eq[0]) >= 4 and int(cand[0, 4]) != 5
    m = scoring.rank_metrics(gt, eq, topk=(10,), ties="average")
    assert 0.0 <= m["hit@10"] <= 1.0
    again = scoring.candidate_ranks(h, table, target, cand, first_item=1)
    assert torch.equal(again[0], gt) and torch.equal(again[1], eq)


# ---- 6. the model's calls ----------------------------------------------------------------------
L, B_MODEL = 12, 5


@pytest.fixture(scope="module")
def model(cuda):
    return _model(cuda, d=64, L=L, layers=2)[0]


def _interaction(model, cuda, seed=2):
    seq, lens = _sequences(L, [L, 7, 3, 1, 9], seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    V = model.item_embedding.weight.shape[0]
    pos = torch.randint(1, V, (B_MODEL,), generator=g)
    return {model.ITEM_SEQ: seq.to(cuda), model.ITEM_SEQ_LEN: lens.to(cuda),
            model.POS_ITEM_ID: pos.to(cuda)}, g, V


def _expanded(model, inter, cand):
    C = cand.shape[1]
    return {model.ITEM_SEQ: inter[model.ITEM_SEQ].repeat_interleave(C, 0),
            model.ITEM_SEQ_LEN: inter[model.ITEM_SEQ_LEN].repeat_interleave(C, 0),
            model.ITEM_ID: cand.reshape(-1)}


def test_predict_candidates_equals_predict_on_the_expanded_batch(cuda, model, monkeypatch):
    inter, g, V = _interaction(model, cuda)
    cand = torch.randint(1, V, (B_MODEL, 7), generator=g).to(cuda)
    ran = []
    orig = kernels.candidate_scores
    monkeypatch.setattr(kernels, "candidate_scores", lambda *a: ran.append(1) or orig(*a))
    with torch.no_grad():
        got = model.predict_candidates(inter, cand)
        ref = model.predict(_expanded(model, inter, cand)).view(B_MODEL, 7)
    assert ran == [1]
    close(got, ref, "predict_candidates")


def test_predict_candidates_backpropagates_through_the_torch_path(cuda, model, monkeypatch):
    inter, g, V = _interaction(model, cuda)
    cand = torch.randint(1, V, (B_MODEL, 7), generator=g).to(cuda)
    w = torch.randn(B_MODEL, 7, generator=g).to(cuda)
    monkeypatch.setattr(kernels, "candidate_scores",
                        lambda *a: pytest.fail("the kernel has no gradient"))
    model.zero_grad()
    (model.predict_candidates(inter, cand) * w).sum().backward()
    got = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad()
    (model.predict(_expanded(model, inter, cand)).view(B_MODEL, 7) * w).sum().backward()
    ref = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad()
    assert set(got) == set(ref) and "item_embedding.weight" in got
    assert any(n.startswith("recurrent_layers.0") for n in got)
    for n in ref:
        close(got[n], ref[n], n)


def test_rerank_of_every_item_equals_full_sort_topk(cuda, model):
    """The two kernels round differently, so ids are compared only where the
    full sort's neighbouring scores differ by more than the bar (1e-4 of the
    largest score).  With this seed the CPU torch paths (session.append_reference
    for the encoder, then the two torch selections) skip none of the 50
    positions: the smallest gap among them is 3.4e-3 against a bar of 1.5e-4.
    At most 10 % may be skipped here."""
    inter, _, V = _interaction(model, cuda)
    k = 10
    cand = torch.arange(1, V, device=cuda)[None].expand(B_MODEL, V - 1).contiguous()
    ids, scores = model.rerank(inter, cand, k=k, exclude_seen=True)
    ref_ids, ref = model.full_sort_topk(inter, k=k + 1, exclude_seen=True)
    close(scores, ref[:, :k], "rerank scores")
    bar = 1e-4 * float(ref.abs().max())
    gap = (ref[:, :-1] - ref[:, 1:]).abs()                 # [B, k]: gap below position i
    clear = gap > bar
    clear[:, 1:] &= gap[:, :-1] > bar
    skipped = 1.0 - float(clear.float().mean())
    print(f"rerank vs full sort: {skipped:.1%} of {clear.numel()} positions skipped")
    assert skipped <= 0.10
    assert torch.equal(ids[clear], ref_ids[:, :k][clear])
    seen = inter[model.ITEM_SEQ]
    assert not (ids[:, :, None] == seen[:, None, :]).any()


def test_sampled_rank_against_the_full_sort_scores(cuda, model):
    inter, g, V = _interaction(model, cuda, seed=4)
    n = 100
    neg = torch.randint(1, V, (B_MODEL, n), generator=g).to(cuda)
    pos = inter[model.POS_ITEM_ID]
    neg[:, 0] = pos                                        # skipped
    gt, eq = model.sampled_rank(inter, neg)
    with torch.no_grad():
        full = model.full_sort_predict(inter)
    st, s = full.gather(1, pos[:, None]), full.gather(1, neg)
    bar = 1e-4 * float(full.abs().max())
    other = neg != pos[:, None]
    above, near = other & (s - st > bar), other & ((s - st).abs() <= bar)
    share = float(near.float().mean())
    print(f"sampled rank: {share:.1%} of {near.numel()} negatives within the bar of the target")
    assert share <= 0.10
    lo, hi = above.sum(1), (above | near).sum(1)
    assert (gt >= lo).all() and (gt <= hi).all() and (gt + eq <= hi).all()
    m = scoring.rank_metrics(gt, eq)
    assert set(m) == {"hit@10", "mrr@10", "ndcg@10", "hit@20", "mrr@20", "ndcg@20"}


# ---- 7. sessions -----------------------------------------------------------------------------------
N_SLOTS, S_RING = 8, 6


def test_session_rerank(cuda, model):
    emb = model.item_embedding.weight.detach()
    V, k, C = emb.shape[0], 10, 40
    state = model.session_open(N_SLOTS, L, history=S_RING)
    twin = model.session_open(N_SLOTS, L, history=S_RING)
    g = torch.Generator().manual_seed(8)
    slots = torch.tensor([5, 0, 3, N_SLOTS, 6], device=cuda)   # N_SLOTS: outside the state
    seq, _ = _sequences(20, [20, 20, 20, 20, 0], seed=3)       # row 4 (slot 6): never an event
    seq = seq.to(cuda)

    def want(y, cand):
        seen = twin.items[slots.clamp(0, N_SLOTS - 1)]
        return scoring.top_candidates(y, emb, cand, k, first_item=1, exclude=seen)

    def check(got, ref):
        live = [0, 1, 2]
        assert torch.equal(got[0][live], ref[0][live]) and torch.equal(got[1][live], ref[1][live])
        assert (got[0][[3, 4]] == -1).all() and (got[1][[3, 4]] == NINF).all()
        assert (got[0][live, 0] >= 1).all()

    for t in range(3):                                         # items [B]: one step
        cand = torch.randint(-1, V + 1, (5, C), generator=g).to(cuda)
        cand[:, :2] = seq[:, :2]                               # seen items among the candidates
        got = model.session_rerank(state, cand, seq[:, t], slots, k=k, exclude_seen=True)
        y = model.session_step(twin, seq[:, t], slots)
        check(got, want(y, cand))
        if t >= 1:
            assert not (got[0][:3, :, None] == seq[:3, None, :2]).any()
    got = model.session_rerank(state, cand, seq[:, 3:12], slots, k=k, exclude_seen=True)  # [B, W]
    y = model.session_append(twin, seq[:, 3:12], slots=slots)
    check(got, want(y, cand))
    before = model.session_recommend(state, None, slots, k=k)
    counts = state.count.clone()
    got = model.session_rerank(state, cand, None, slots, k=k, exclude_seen=True)   # no event
    check(got, want(twin.out[slots.clamp(0, N_SLOTS - 1)], cand))
    after = model.session_recommend(state, None, slots, k=k)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert torch.equal(state.count, counts) and torch.equal(state.items, twin.items)
    # the whole state, without exclusion
    cand = torch.randint(1, V, (N_SLOTS, C), generator=g).to(cuda)
    got = session.rerank(model, state, cand, k=C)
    ref = scoring.top_candidates(state.out, emb, cand, C, first_item=1)
    live = (state.count > 0).nonzero().reshape(-1)
    assert live.tolist() == [0, 3, 5]
    assert torch.equal(got[0][live], ref[0][live]) and torch.equal(got[1][live], ref[1][live])
    assert (got[0][state.count == 0] == -1).all()
    plain = model.session_open(N_SLOTS, L)
    with pytest.raises(ValueError, match="history="):
        model.session_rerank(plain, cand, exclude_seen=True)

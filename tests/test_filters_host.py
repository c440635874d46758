"""Catalogue filters, the parts that need no GPU: scoring.item_filters' bitmaps
(three input forms, the sign bit, the tail bits), scoring.top_items' torch path
under a filter against a brute-force sort, the binding of
include/recblr_filters.h and the argument checks of its two entry points (made
before any HIP call)."""
import ctypes
import math

import pytest
import torch

from datamining_recblr_amd import _lib, kernels, scoring

NAMES = ("rb_item_topk_allowed", "rb_item_rank_allowed")
SIZES = (1, 31, 32, 33, 300)


# ---- filters as data -------------------------------------------------------------------
def _random_mask(F, V, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((F, V), generator=g) < 0.5


def _words_by_hand(mask):
    """The layout, spelled out in Python integers: bit i of word w of row f."""
    F, V = mask.shape
    out = []
    for f in range(F):
        row = []
        for w in range((V + 31) // 32):
            x = sum(1 << i for i in range(32) if 32 * w + i < V and bool(mask[f, 32 * w + i]))
            row.append(x - (1 << 32) if x >= 1 << 31 else x)   # wrapped into int32
        out.append(row)
    return torch.tensor(out, dtype=torch.int32)


@pytest.mark.parametrize("V", SIZES)
def test_item_filters_round_trips_for_all_three_forms(V):
    mask = _random_mask(3, V, V)
    mask[1] = False                       # an empty filter
    mask[2] = True                        # a full one: every word's bit 31 up to V
    f = scoring.item_filters(mask)
    assert isinstance(f, scoring.ItemFilters)
    assert f.n_items == V and f.n_filters == 3
    assert f.words.dtype == torch.int32 and f.words.is_contiguous()
    assert tuple(f.words.shape) == (3, (V + 31) // 32)
    assert torch.equal(f.words, _words_by_hand(mask))
    assert torch.equal(f.mask(), mask)
    assert f.mask().dtype == torch.bool
    assert torch.equal(f.count(), mask.sum(1)) and torch.equal(f.count(), f.mask().sum(1))
    # [V] gives F = 1
    one = scoring.item_filters(mask[0])
    assert one.n_filters == 1 and one.n_items == V
    assert torch.equal(one.words, f.words[:1]) and torch.equal(one.mask(), mask[:1])
    # id lists, shuffled and with duplicates
    lists = []
    for r in range(3):
        ids = torch.nonzero(mask[r]).flatten().tolist()
        lists.append(list(reversed(ids)) + ids[:2])
    by_ids = scoring.item_filters(lists, n_items=V)
    assert torch.equal(by_ids.words, f.words) and by_ids.n_items == V
    assert torch.equal(scoring.item_filters([torch.tensor(x, dtype=torch.int64) for x in lists],
                                            n_items=V).words, f.words)


def test_item_filters_sign_bit_and_tail_bits():
    # bit 31 of a word alone: the int32 is its minimum, not an overflow
    f = scoring.item_filters([[31], [63, 0], []], n_items=70)
    assert f.words.tolist() == [[-(1 << 31), 0, 0], [1, -(1 << 31), 0], [0, 0, 0]]
    assert f.count().tolist() == [1, 2, 0]
    assert f.mask()[0].nonzero().flatten().tolist() == [31]
    full = scoring.item_filters(torch.ones(33, dtype=torch.bool))
    assert full.words.tolist() == [[-1, 1]]            # bits at or beyond V are zero
    for V in SIZES:
        w = scoring.item_filters(torch.ones((2, V), dtype=torch.bool)).words
        tail = V % 32
        if tail:
            assert (w[:, -1].to(torch.int64) & 0xFFFFFFFF == (1 << tail) - 1).all()
        assert int(scoring.item_filters(torch.ones(V, dtype=torch.bool)).count()) == V


def test_item_filters_rejects_bad_input():
    for bad in ([[0, 5]], [[-1]], [[2], [7, 5]]):
        with pytest.raises(ValueError):
            scoring.item_filters(bad, n_items=5)
    with pytest.raises(ValueError):
        scoring.item_filters([[0, 1]])                                   # id lists need n_items
    with pytest.raises(ValueError):
        scoring.item_filters(torch.ones(4, dtype=torch.bool), n_items=5)
    with pytest.raises(ValueError):
        scoring.item_filters(torch.ones(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        scoring.item_filters(torch.ones((2, 2, 2), dtype=torch.bool))
    with pytest.raises(ValueError):
        scoring.ItemFilters(torch.zeros((1, 2), dtype=torch.int32), 100)


# ---- the torch path under a filter ---------------------------------------------------
def _brute(S, k, first_item, exclude, mask, rows):
    """rows None: filter 0 everywhere; -1: no filter; outside [-1, F): nothing."""
    B, V = S.shape
    F = mask.shape[0]
    ids, sc = [], []
    for b in range(B):
        f = 0 if rows is None else int(rows[b])
        banned = set() if exclude is None else {int(e) for e in exclude[b]}
        cand = [(-float(S[b, v]), v) for v in range(first_item, V)
                if v not in banned and not math.isnan(float(S[b, v]))
                and (f == -1 or (0 <= f < F and bool(mask[f, v])))]
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


def test_top_items_on_cpu_with_filters_matches_brute_force():
    B, V, d = 8, 70, 5          # d = 5: no kernel for it on any device
    seq, W = _ints(B, V, d, 0)
    W[40:44] = W[3]             # exact ties across the allowed / disallowed boundary
    W[50] = float("nan")        # a NaN column, allowed by every filter below
    S = seq @ W.t()
    mask = _random_mask(4, V, 7)
    mask[0, 3], mask[0, 40], mask[0, 41], mask[0, 42] = False, True, False, True
    mask[:, 50] = True
    mask[1] = False                                     # empty
    mask[2] = False
    mask[2, [1, 5, 64, 69]] = True                      # fewer than k items
    mask[3, :12] = True                                 # first_item cuts into it
    allow = scoring.item_filters(mask)
    rows = torch.tensor([0, 1, 2, 3, -1, 4, -2, 0])     # mixed, -1, two out of range
    g = torch.Generator().manual_seed(1)
    ex = torch.randint(1, V, (B, 9), generator=g)
    ex[:, 0] = 40                                       # excluded and allowed (filter 0)
    ex[:, 3], ex[:, 4] = -1, V + 7
    for first_item in (0, 1, 9):
        for exclude in (None, ex):
            for k in (1, 6, 64, 80):
                for r in (rows, None):
                    ids, sc = scoring.top_items(seq, W, k, first_item=first_item,
                                                exclude=exclude, allow=allow, allow_rows=r)
                    want_ids, want_sc = _brute(S, k, first_item, exclude, mask, r)
                    assert ids.dtype == torch.int64 and sc.dtype == torch.float32
                    assert torch.equal(ids, want_ids), (first_item, k)
                    assert torch.equal(sc, want_sc), (first_item, k)
                    assert not (ids == 50).any()        # NaN is never selected
    ids, sc = scoring.top_items(seq, W, 6, first_item=1, exclude=ex, allow=allow, allow_rows=rows)
    plain_ids, plain_sc = scoring.top_items(seq, W, 6, first_item=1, exclude=ex)
    # a -1 row is the unfiltered call's row
    assert torch.equal(ids[4], plain_ids[4]) and torch.equal(sc[4], plain_sc[4])
    # an out-of-range row and an empty filter select nothing
    for b in (1, 5, 6):
        assert (ids[b] == -1).all() and (sc[b] == float("-inf")).all()
    # fewer than k allowed: a -1 / -inf tail
    assert (ids[2, :3] >= 0).all() and (ids[2, 4:] == -1).all()
    assert (sc[2, 4:] == float("-inf")).all()
    # the twins: 3 and 41 tie with 40 and 42 exactly; only the allowed ones show,
    # and 40 is excluded, so of the four only 42 can
    assert not ((ids[0] == 3) | (ids[0] == 41) | (ids[0] == 40)).any()
    all_ids, _ = scoring.top_items(seq, W, V, first_item=0, allow=allow,
                                   allow_rows=torch.zeros(B, dtype=torch.int64))
    assert (all_ids[0] == 42).any() and (all_ids[0] == 40).any()
    # the all-ones filter is the unfiltered call
    ones = scoring.item_filters(torch.ones(V, dtype=torch.bool))
    ids, sc = scoring.top_items(seq, W, 6, exclude=ex, allow=ones)
    assert torch.equal(ids, plain_ids) and torch.equal(sc, plain_sc)


def test_top_items_rejects_bad_filter_arguments():
    seq, W = _ints(3, 40, 4, 3)
    allow = scoring.item_filters(torch.ones(40, dtype=torch.bool))
    rows = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError):
        scoring.top_items(seq, W, 2, allow_rows=rows)                    # rows without allow
    with pytest.raises(ValueError):
        scoring.top_items(seq, W, 2, allow=scoring.item_filters(torch.ones(41, dtype=torch.bool)))
    with pytest.raises(ValueError):
        scoring.top_items(seq, W, 2, allow=allow, allow_rows=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(TypeError):
        scoring.top_items(seq, W, 2, allow=allow.words)
    with pytest.raises(ValueError):
        scoring._top_items_torch(seq, W, 2, 1, None, None, rows)
    with pytest.raises(kernels.RecBLRNativeError):                       # no torch path for ranks
        scoring.target_ranks(seq, W, rows, allow=allow)


# ---- header and binding --------------------------------------------------------------
def test_header_declares_exactly_the_two_entry_points():
    p, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    tail = [p, i64, i64, p]                              # allow, F, words, allow_rows
    assert set(_lib.FILTER_SIGNATURES) == set(NAMES)
    assert dict(_lib.FILTER_SIGNATURES) == {
        "rb_item_topk_allowed": (i32, _lib.SIGNATURES["rb_item_topk"][1] + tail),
        "rb_item_rank_allowed": (i32, _lib.SIGNATURES["rb_item_rank"][1] + tail),
    }
    assert not set(NAMES) & set(_lib.SIGNATURES)          # recblr_hip.h keeps its entries


def test_library_exports_them_at_the_headers_version():
    lib = _lib.load()
    assert lib.rb_version() == _lib.ABI_VERSION
    for name in NAMES:
        assert getattr(lib, name).argtypes == _lib.FILTER_SIGNATURES[name][1]
    assert set(NAMES) <= set(kernels.FLOP_KERNELS)        # MFMA sweeps, counted in FLOPs
    assert {"item_filters", "ItemFilters"} <= set(scoring.__all__)


# ---- argument checks -----------------------------------------------------------------
# a valid call's arguments; 16 is a "pointer" (16-B aligned, never read)
def _topk(lib, seq=16, items=16, B=4, V=70, d=128, k=10, first=1, ex=None, E=0, ids=16,
          scores=16, ws=16, ws_bytes=1 << 20, allow=16, F=2, words=3, rows=16):
    return lib.rb_item_topk_allowed(seq, items, B, V, d, k, first, ex, E, ids, scores, ws,
                                    ws_bytes, None, allow, F, words, rows)


def _rank(lib, seq=16, items=16, target=16, B=4, V=70, d=128, first=1, gt=16, eq=16, ws=16,
          ws_bytes=1 << 20, allow=16, F=2, words=3, rows=16):
    return lib.rb_item_rank_allowed(seq, items, target, B, V, d, first, gt, eq, ws, ws_bytes, None,
                                    allow, F, words, rows)


def test_argument_errors_come_back_before_any_hip_call():
    lib = _lib.load()

    def rejected(call, msg, **kw):
        assert call(lib, **kw) == _lib.RB_EINVAL, kw
        assert msg in lib.rb_last_error_string(), (kw, lib.rb_last_error_string())

    for call in (_topk, _rank):
        rejected(call, b"null pointer (allow)", allow=None)
        rejected(call, b"F must be", F=0)
        rejected(call, b"F must be", F=-3)
        rejected(call, b"words must be", words=2)
        rejected(call, b"words must be", words=4)
        rejected(call, b"words must be", V=64, words=3)       # exactly two words at V = 64
        rejected(call, b"words must be", V=65, words=2)
        # what the unfiltered entry points check
        rejected(call, b"null pointer", seq=None)
        rejected(call, b"null pointer", items=None)
        rejected(call, b"null pointer", ws=None)
        rejected(call, b"d must be", d=48)
        rejected(call, b"first_item must be", first=-1)
        rejected(call, b"positive", B=0)
    rejected(_topk, b"null pointer", ids=None)
    rejected(_topk, b"null pointer", scores=None)
    rejected(_topk, b"k must be", k=0)
    rejected(_topk, b"k must be", k=65)
    rejected(_topk, b"null pointer", E=3, ex=None)
    rejected(_topk, b"E must be", E=-1)
    rejected(_rank, b"null pointer", target=None)
    rejected(_rank, b"null pointer", gt=None)
    # the messages name the entry point, and the workspaces are the unfiltered calls'
    _topk(lib, F=0)
    assert lib.rb_last_error_string().startswith(b"rb_item_topk_allowed:")
    _rank(lib, F=0)
    assert lib.rb_last_error_string().startswith(b"rb_item_rank_allowed:")
    rejected(_topk, b"rb_item_topk_allowed: workspace too small",
             ws_bytes=lib.rb_item_topk_workspace(4, 70, 128, 10) - 1)
    rejected(_rank, b"rb_item_rank_allowed: workspace too small",
             ws_bytes=lib.rb_item_rank_workspace(4, 70, 128) - 1)

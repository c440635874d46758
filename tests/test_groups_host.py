"""Diversity caps, the parts that need no GPU: scoring.item_groups, the argument
errors of scoring.top_items' groups / max_per_group, the torch path under a cap
against a plain Python walk, the header include/recblr_groups.h and the argument
checks of rb_item_topk_grouped (made before any HIP call)."""
import ctypes
import math

import pytest
import torch

from datamining_recblr_amd import _lib, evaluation, kernels, scoring

B, V, D = 5, 300, 5          # d = 5: no kernel for it on any device
KS = (1, 10, 64, 100)
TWINS = (3, 40, 41, 42)      # equal table rows: exact ties
NAN_ITEM = 50
LAYOUTS = {
    "one_group": [0] * V,
    "mod7": [v % 7 for v in range(V)],
    "own": list(range(V)),
    "mixed": [-1 if v % 4 == 0 else v % 3 for v in range(V)],
}


# ---- item_groups ----------------------------------------------------------------------
def test_item_groups_fields_and_forms():
    g = scoring.item_groups([2, -1, 0, 2, 5])
    assert isinstance(g, scoring.ItemGroups)
    assert g.ids.dtype == torch.int32 and g.ids.is_contiguous() and g.ids.shape == (5,)
    assert g.ids.tolist() == [2, -1, 0, 2, 5]
    assert (g.n_items, g.n_groups) == (5, 6)
    assert g.to("cpu") is g and g.ids.device.type == "cpu"
    for dtype in (torch.int64, torch.int32, torch.int16, torch.int8):
        h = scoring.item_groups(torch.tensor([2, -1, 0, 2, 5], dtype=dtype), device="cpu")
        assert torch.equal(h.ids, g.ids) and h.n_groups == 6
    # a strided view becomes contiguous; all -1 has no group at all
    assert scoring.item_groups(torch.arange(10)[::2]).ids.tolist() == [0, 2, 4, 6, 8]
    assert scoring.item_groups([-1, -1]).n_groups == 0
    # ids beyond the kernel's 16 bits are accepted (top_items takes the torch path)
    big = scoring.item_groups([0, kernels.ITEM_GROUP_ID_MAX + 1, 1 << 20])
    assert big.n_groups == (1 << 20) + 1 and big.ids.tolist()[2] == 1 << 20
    assert {"item_groups", "ItemGroups"} <= set(scoring.__all__)


def test_item_groups_rejects_bad_input():
    for bad in ([0, -2, 1], [-5], torch.tensor([3, -1, -2])):
        with pytest.raises(ValueError):
            scoring.item_groups(bad)
    with pytest.raises(ValueError):
        scoring.item_groups(torch.tensor([0.0, 1.0]))              # not integers
    with pytest.raises(ValueError):
        scoring.item_groups(torch.tensor([True, False]))
    with pytest.raises(ValueError):
        scoring.item_groups(torch.zeros((2, 3), dtype=torch.int64))  # not [V]
    with pytest.raises(ValueError):
        scoring.item_groups([])
    with pytest.raises(ValueError):
        scoring.item_groups([0, 1 << 31])                           # does not fit int32
    with pytest.raises(ValueError):
        scoring.ItemGroups(torch.zeros(4, dtype=torch.int64), 1)


# ---- top_items' argument errors -------------------------------------------------------
def _ints(n_rows, n_items, d, seed):
    """Small integer features: exact scores, many ties."""
    g = torch.Generator().manual_seed(seed)
    seq = torch.randint(-2, 3, (n_rows, d), generator=g).float()
    W = torch.randint(-2, 3, (n_items, d), generator=g).float()
    return seq, W


def test_top_items_rejects_bad_group_arguments():
    seq, W = _ints(3, 40, 4, 3)
    groups = scoring.item_groups([v % 5 for v in range(40)])
    with pytest.raises(ValueError):
        scoring.top_items(seq, W, 2, groups=groups)                  # one without the other
    with pytest.raises(ValueError):
        scoring.top_items(seq, W, 2, max_per_group=1)
    for m in (0, -1):
        with pytest.raises(ValueError):
            scoring.top_items(seq, W, 2, groups=groups, max_per_group=m)
    with pytest.raises(ValueError):                                  # wrong V
        scoring.top_items(seq, W, 2, groups=scoring.item_groups([0] * 41), max_per_group=1)
    with pytest.raises(TypeError):
        scoring.top_items(seq, W, 2, groups=groups.ids, max_per_group=1)
    with pytest.raises(ValueError):
        scoring._top_items_torch(seq, W, 2, 1, None, None, None, groups, None)
    with pytest.raises(ValueError):
        evaluation.recommend(None, [[1]], groups=groups, device="cpu")


def test_no_cap_arguments_where_a_cap_has_no_meaning():
    import inspect

    from datamining_recblr_amd import session
    from datamining_recblr_amd.model import RecBLR

    takes = (scoring.top_items, RecBLR.full_sort_topk, RecBLR.session_recommend,
             session.recommend, evaluation.recommend, kernels.item_topk)
    leaves = (scoring.target_ranks, scoring.top_candidates, evaluation.full_sort_metrics,
              RecBLR.full_sort_rank, RecBLR.rerank, RecBLR.session_rerank)
    for fn in takes:
        assert {"groups", "max_per_group"} <= set(inspect.signature(fn).parameters), fn
    for fn in leaves:
        assert not {"groups", "max_per_group"} & set(inspect.signature(fn).parameters), fn


# ---- the torch path against the defining walk ----------------------------------------
def _walk(S, k, first_item, exclude, allowed, group_of, m):
    """The contract, literally: the row's selectable items by (score
    descending, id ascending), an item taken unless m of its group were."""
    n_rows, n_items = S.shape
    ids, sc = [], []
    for b in range(n_rows):
        banned = set() if exclude is None else {int(e) for e in exclude[b]}
        cand = [(-float(S[b, v]), v) for v in range(first_item, n_items)
                if v not in banned and not math.isnan(float(S[b, v]))
                and (allowed is None or bool(allowed[v]))]
        cand.sort()
        taken, got = {}, []
        for s, v in cand:
            if len(got) == k:
                break
            g = group_of[v] if group_of is not None else -1
            if g != -1:
                if taken.get(g, 0) >= m:
                    continue
                taken[g] = taken.get(g, 0) + 1
            got.append((s, v))
        ids.append([v for _, v in got] + [-1] * (k - len(got)))
        sc.append([-s for s, _ in got] + [float("-inf")] * (k - len(got)))
    return torch.tensor(ids, dtype=torch.int64), torch.tensor(sc, dtype=torch.float32)


@pytest.fixture(scope="module")
def case():
    seq, W = _ints(B, V, D, 0)
    W[list(TWINS)] = torch.tensor([2.0, -2.0, 2.0, -2.0, 2.0])   # the longest row there is
    assert ((W == W[TWINS[0]]).all(1).sum()) == len(TWINS)
    seq[0] = 2.0 * W[TWINS[0]]                # row 0 ranks the twins at the top, alone
    W[NAN_ITEM] = float("nan")
    S = seq @ W.t()
    g = torch.Generator().manual_seed(1)
    ex = torch.randint(1, V, (B, 9), generator=g)
    ex[:, 0] = TWINS[1]                       # a twin excluded
    ex[:, 3], ex[:, 4] = -1, V + 7
    mask = torch.rand(V, generator=g) < 0.6
    mask[TWINS[2]] = False                    # a twin dropped by the filter
    mask[[TWINS[0], TWINS[3], NAN_ITEM]] = True
    return seq, W, S, ex, mask


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_top_items_on_cpu_with_a_cap_matches_the_walk(case, layout):
    seq, W, S, ex, mask = case
    group_of = LAYOUTS[layout]
    groups = scoring.item_groups(group_of)
    allow = scoring.item_filters(mask)
    full = tail = 0
    for k in KS:
        for m in (1, 2, k):
            for first_item in (0, 1):
                for exclude, allowed in ((None, None), (ex, None), (ex, mask)):
                    ids, sc = scoring.top_items(seq, W, k, first_item=first_item,
                                                exclude=exclude,
                                                allow=allow if allowed is not None else None,
                                                groups=groups, max_per_group=m)
                    want = _walk(S, k, first_item, exclude, allowed, group_of, m)
                    what = (layout, k, m, first_item, exclude is not None, allowed is not None)
                    assert ids.dtype == torch.int64 and sc.dtype == torch.float32
                    assert torch.equal(ids, want[0]), what
                    assert torch.equal(sc, want[1]), what
                    assert not (ids == NAN_ITEM).any()
                    full += int((want[0][:, -1] >= 0).sum())
                    tail += int((want[0][:, -1] < 0).sum())
    assert full > 0                            # the cases do fill lists ...
    if layout in ("one_group", "mod7"):
        assert tail > 0                        # ... and leave -1 tails where meant to
    # one group: min(m, k) entries; id % 7 with m = 1: seven
    if layout == "one_group":
        ids, _ = scoring.top_items(seq, W, 10, groups=groups, max_per_group=2)
        assert ((ids >= 0).sum(1) == 2).all() and (ids[:, 2:] == -1).all()
    if layout == "mod7":
        ids, sc = scoring.top_items(seq, W, 10, groups=groups, max_per_group=1)
        assert ((ids >= 0).sum(1) == 7).all() and (sc[:, 7:] == float("-inf")).all()
        for row in ids[:, :7].tolist():
            assert sorted(v % 7 for v in row) == list(range(7))


def test_twins_under_a_cap(case):
    seq, W, S, ex, mask = case
    a, b, c, d = TWINS
    # all four twins in one group, m = 1: the smallest id wins, the others never show
    one = [7 if v in TWINS else -1 for v in range(V)]
    ids, _ = scoring.top_items(seq, W, 10, first_item=0, groups=scoring.item_groups(one),
                               max_per_group=1)
    assert ids[0, 0] == a and not set(ids[0].tolist()) & {b, c, d}
    # ... with that one excluded (ex lists b) and m = 2: a and c
    ids, _ = scoring.top_items(seq, W, 10, exclude=ex, groups=scoring.item_groups(one),
                               max_per_group=2)
    assert ids[0, :2].tolist() == [a, c] and d not in ids[0].tolist()
    # ... and c dropped by the filter as well: a and d
    ids, _ = scoring.top_items(seq, W, 10, exclude=ex, allow=scoring.item_filters(mask),
                               groups=scoring.item_groups(one), max_per_group=2)
    assert ids[0, :2].tolist() == [a, d]
    # twins in different groups: all four, in id order
    apart = [TWINS.index(v) if v in TWINS else -1 for v in range(V)]
    ids, _ = scoring.top_items(seq, W, 10, groups=scoring.item_groups(apart), max_per_group=1)
    assert ids[0, :4].tolist() == [a, b, c, d]


def test_a_cap_that_cannot_bind_is_the_uncapped_call(case):
    seq, W, S, ex, mask = case
    allow = scoring.item_filters(mask)
    for k in KS:
        for kw in (dict(), dict(exclude=ex), dict(exclude=ex, allow=allow, first_item=0)):
            plain = scoring.top_items(seq, W, k, **kw)
            for layout, m in (("one_group", k), ("mod7", k), ("mixed", k + 3), ("own", 1),
                              ("own", 2)):
                got = scoring.top_items(seq, W, k, groups=scoring.item_groups(LAYOUTS[layout]),
                                        max_per_group=m, **kw)
                assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]), (k, layout)
            none = scoring.item_groups([-1] * V)
            got = scoring.top_items(seq, W, k, groups=none, max_per_group=1, **kw)
            assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]), k


def test_group_ids_beyond_the_kernels_range(case):
    """Any non-negative id names a group on the torch path."""
    seq, W, S, ex, mask = case
    small = LAYOUTS["mod7"]
    big = [g * 100003 + kernels.ITEM_GROUP_ID_MAX + 1 for g in small]
    a = scoring.top_items(seq, W, 10, exclude=ex, groups=scoring.item_groups(small),
                          max_per_group=1)
    b = scoring.top_items(seq, W, 10, exclude=ex, groups=scoring.item_groups(big),
                          max_per_group=1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- header and binding --------------------------------------------------------------
NAME = "rb_item_topk_grouped"


def test_header_declares_the_entry_point_and_its_workspace_query():
    p, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert dict(_lib.GROUP_SIGNATURES) == {
        NAME + "_workspace": (i64, [i64, i64, i64, i64]),
        NAME: (i32, _lib.FILTER_SIGNATURES["rb_item_topk_allowed"][1] + [p, i64]),
    }
    assert not set(_lib.GROUP_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.FILTER_SIGNATURES))
    header = open(_lib.HEADER_PATH.replace("recblr_hip.h", "recblr_groups.h")).read()
    assert _lib._define(header, "RB_GROUP_ID_MAX") == kernels.ITEM_GROUP_ID_MAX == 65534


def test_library_exports_it_at_the_headers_version():
    lib = _lib.load()
    assert lib.rb_version() == _lib.ABI_VERSION
    for name, (_, args) in _lib.GROUP_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args
    assert NAME in kernels.FLOP_KERNELS
    # the lists' workspace and one more array of the same size
    plain, grouped = lib.rb_item_topk_workspace, lib.rb_item_topk_grouped_workspace
    for shape in ((4, 70, 128, 10), (130, 20000, 16, 64), (2048, 10544, 128, 1)):
        assert grouped(*shape) * 2 == plain(*shape) * 3 > 0
    for shape in ((0, 70, 128, 10), (4, 70, 128, 0), (4, 70, 128, 65)):
        assert grouped(*shape) == 0


# a valid call's arguments; 16 is a "pointer" (16-B aligned, never read)
def _grouped(lib, seq=16, items=16, n_rows=4, n_items=70, d=128, k=10, first=1, ex=None, E=0,
             ids=16, scores=16, ws=16, ws_bytes=1 << 20, allow=16, F=2, words=3, rows=16,
             groups=16, m=2):
    return lib.rb_item_topk_grouped(seq, items, n_rows, n_items, d, k, first, ex, E, ids, scores,
                                    ws, ws_bytes, None, allow, F, words, rows, groups, m)


def test_argument_errors_come_back_before_any_hip_call():
    lib = _lib.load()

    def rejected(msg, **kw):
        assert _grouped(lib, **kw) == _lib.RB_EINVAL, kw
        assert msg in lib.rb_last_error_string(), (kw, lib.rb_last_error_string())

    rejected(b"null pointer (groups)", groups=None)
    rejected(b"max_per_group must be", m=0)
    rejected(b"max_per_group must be", m=-4)
    # the filter is optional, and checked when given
    rejected(b"F must be", F=0)
    rejected(b"words must be", words=2)
    rejected(b"max_per_group must be", allow=None, F=0, words=0, m=0)
    # what rb_item_topk checks
    rejected(b"null pointer", seq=None)
    rejected(b"null pointer", ids=None)
    rejected(b"null pointer", ws=None)
    rejected(b"d must be", d=48)
    rejected(b"k must be", k=0)
    rejected(b"k must be", k=65)
    rejected(b"first_item must be", first=-1)
    rejected(b"null pointer", E=3, ex=None)
    assert lib.rb_last_error_string().startswith(b"rb_item_topk_grouped:")
    for allow in (16, None):
        rejected(b"rb_item_topk_grouped: workspace too small", allow=allow,
                 ws_bytes=lib.rb_item_topk_grouped_workspace(4, 70, 128, 10) - 1)

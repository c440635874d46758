"""The sessions' item ring on a GPU-less host: rb_session_record's boundary
(header, exports, argument errors before any GPU call), session.record_reference
against a plain-Python simulation (one collections.deque(maxlen=S) per slot and
the masking rule written with lists), the ring through step / append / prefill
on a CPU state, and session.recommend on a CPU state.

Every comparison is exact: the ring holds integers and the recommendation is
the same top-k on the same inputs."""
import collections
import ctypes
import os
import re

import pytest
import torch

from datamining_recblr_amd import _lib, scoring, session
from datamining_recblr_amd.model import RecBLR
from test_gpu_session import V, _model, _sequences, _state_tensors

HEADER = os.path.join(os.path.dirname(_lib.__file__), "session", "recblr_session.h")
TILE = 16


# ---- the boundary --------------------------------------------------------------
def test_record_is_declared_exported_and_typed_from_the_header():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert "rb_session_record" in re.findall(r"\b(rb_[a-z0-9_]+)\s*\(", text)
    assert session.TILE == TILE
    res, args = _lib.SESSION_SIGNATURES["rb_session_record"]
    proto = re.search(r"int rb_session_record\(([^)]*)\)", text).group(1)
    want = [ctypes.c_void_p if "*" in a else ctypes.c_int64 for a in proto.split(",")]
    assert res is ctypes.c_int and args == want and len(args) == 11
    lib = _lib.load_session()
    assert hasattr(lib, "rb_session_record")
    assert lib.rb_session_record.argtypes == want
    assert not hasattr(ctypes.CDLL(_lib.LIB_PATH), "rb_session_record")
    assert {"record_reference", "recommend"} <= set(session.__all__)
    assert callable(RecBLR.session_recommend)


# a call that passes every check (fake non-null pointers that are never
# dereferenced: each case below fails a check before any HIP call)
_P = 256


def _args(**bad):
    a = dict(items=_P, B=3, W=5, slots=None, count=_P, ring=_P, seen=_P, N=8, S=4, V=50,
             stream=None)
    assert set(bad) <= set(a)
    a.update(bad)
    assert len(a) == len(_lib.SESSION_SIGNATURES["rb_session_record"][1])
    return list(a.values())


_NULL = "rb_session_record: null pointer"
_POS = "rb_session_record: B, N, S and V must be positive"
RECORD_ERRORS = [
    (dict(items=None), _NULL),                      # null items with W > 0
    (dict(count=None), _NULL),
    (dict(ring=None), _NULL),
    (dict(items=None, W=0, ring=None), _NULL),      # W = 0 excuses items only
    (dict(S=0), _POS),
    (dict(N=0), _POS),
    (dict(B=0), _POS),
    (dict(V=0), _POS),
    (dict(W=-1), "rb_session_record: W must be >= 0"),
    (dict(S=1 << 31), "rb_session_record: B, W, N, S and V must be < 2^31"),
]


@pytest.mark.parametrize("bad,message", RECORD_ERRORS,
                         ids=["-".join(f"{k}={v}" for k, v in b.items()) for b, _ in RECORD_ERRORS])
def test_record_argument_errors_are_reported_before_any_gpu_call(bad, message):
    lib = _lib.load_session()
    assert lib.rb_session_record(*_args(**bad)) == _lib.RB_EINVAL
    assert lib.rb_session_last_error_string().decode() == message
    with pytest.raises(_lib.RecBLRNativeError, match="invalid argument"):
        _lib.call_session("rb_session_record", *_args(**bad))


# ---- the plain-Python simulation ---------------------------------------------------
def recorded_events(row, n_items=V):
    """The masking rule with lists: the events of one call row."""
    events = []
    for c0 in range(0, len(row), TILE):
        chunk = []
        for v in row[c0:c0 + TILE]:
            if v == 0:
                break
            chunk.append(v)
        if all(0 <= v < n_items for v in chunk):
            events += chunk
    return events


class Simulation:
    """One deque(maxlen=S) and one event count per slot."""

    def __init__(self, N, S):
        self.N, self.S = N, S
        self.last = [collections.deque(maxlen=S) for _ in range(N)]
        self.count = [0] * N

    def feed(self, items, slots=None):
        """Feed a call's rows (lists); returns the rows' seen lists [B][S] in
        ring order, as they stand after the call."""
        seen = []
        for b, row in enumerate(items):
            slot = b if slots is None else slots[b]
            if not 0 <= slot < self.N:
                seen.append([-1] * self.S)
                continue
            for v in recorded_events(row):
                self.last[slot].append(v)
                self.count[slot] += 1
            seen.append(self.ring_row(slot))
        return seen

    def reset(self, slots):
        for s in slots:
            self.last[s].clear()
            self.count[s] = 0

    def ring_row(self, slot):
        """The slot's ring: event e at position e % S, -1 where nothing was written."""
        row, kept = [-1] * self.S, self.last[slot]
        for i, v in enumerate(kept):
            row[(self.count[slot] - len(kept) + i) % self.S] = v
        return row

    def ring(self):
        return torch.tensor([self.ring_row(s) for s in range(self.N)], dtype=torch.int64)

    def history(self, slots=None):
        slots = range(self.N) if slots is None else slots
        ids = [list(self.last[s]) + [-1] * (self.S - len(self.last[s])) for s in slots]
        return torch.tensor(ids, dtype=torch.int64), torch.tensor([len(self.last[s]) for s in slots])


def row_mix(B, W, N, S, seed=0):
    """A call's rows and slots (lists), and the events the slots hold already.
    Rows by b % 8: full; an interior 0; a bad id (V) in chunk 0; a bad id (-3)
    in chunk 1 (chunk 0's events are kept); slot -1; slot N; one event; no
    event.  Slots: a permutation of N, non-contiguous; they hold 0, 1, S - 1, S
    and S + 2 events by b % 5."""
    g = torch.Generator().manual_seed(1000 * seed + 97 * B + 13 * W + S)
    items = torch.randint(1, V, (B, W), generator=g).tolist()
    slots = torch.randperm(N, generator=g)[:B].tolist()
    for b, row in enumerate(items):
        kind = b % 8
        if kind == 1 and W >= 2:
            row[W // 3] = 0
        elif kind == 2 and W >= 1:
            row[min(2, W - 1)] = V
        elif kind == 3 and W > TILE:
            row[min(TILE + 1, W - 1)] = -3
        elif kind == 4:
            slots[b] = -1
        elif kind == 5:
            slots[b] = N
        elif kind == 6:
            row[1:] = [0] * (W - 1)
        elif kind == 7:
            row[:] = [0] * W
    held = [(0, 1, S - 1, S, S + 2)[b % 5] for b in range(B)]
    return items, slots, held


def preload(sim, slots, held, seed=3):
    """The slots' earlier events, into the simulation."""
    g = torch.Generator().manual_seed(seed)
    for slot, n in zip(slots, held):
        if 0 <= slot < sim.N and n:
            sim.feed([torch.randint(1, V, (1,), generator=g).tolist() for _ in range(n)],
                     [slot] * n)


def load_state(state, sim):
    """The simulation's rings and counts as the state's (the encoder tensors
    are not touched: record reads count and the ring only)."""
    state.items.copy_(sim.ring())
    state.count.copy_(torch.tensor(sim.count))


@pytest.fixture(scope="module")
def model():
    return _model(torch.device("cpu"), L=12)[0]


@pytest.mark.parametrize("S", [1, 3, 16, 20])
@pytest.mark.parametrize("W", [0, 1, 15, 16, 17, 35])
def test_record_reference_equals_the_simulation(model, S, W):
    B, N = 21, 30
    items, slots, held = row_mix(B, W, N, S)
    assert {0, 1, S - 1, S, S + 2} == set(held)
    sim = Simulation(N, S)
    preload(sim, slots, held)
    state = session.SessionState(model, N, 12, history=S)
    assert state.items.shape == (N, S) and state.items.dtype == torch.int64
    assert torch.equal(state.items, torch.full((N, S), -1))
    load_state(state, sim)
    before, count = state.items.clone(), state.count.clone()
    want_seen = sim.feed(items, slots)
    if W == 35 and S < 16:
        assert max(len(recorded_events(r)) for r in items) > S      # more than S in one call
    seen = session.record_reference(state, torch.tensor(items).reshape(B, W),
                                    torch.tensor(slots), want_seen=True)
    assert torch.equal(state.items, sim.ring())
    assert torch.equal(seen, torch.tensor(want_seen))
    assert torch.equal(state.count, count)                          # read, never written
    others = sorted(set(range(N)) - set(slots))
    assert others and torch.equal(state.items[others], before[others])
    if W == 0:
        assert torch.equal(state.items, before)
    # the same call without seen returns nothing and leaves the same ring
    again = session.SessionState(model, N, 12, history=S)
    again.items.copy_(before)
    again.count.copy_(count)
    assert session.record_reference(again, torch.tensor(items).reshape(B, W),
                                    torch.tensor(slots)) is None
    assert torch.equal(again.items, state.items)


def test_record_reference_keeps_the_first_chunk_of_a_row_with_a_bad_second_chunk(model):
    S, N = 20, 4
    state = session.SessionState(model, N, 12, history=S)
    row = list(range(1, 17)) + [5, V + 3, 6] + [0] * 13 + [7, 8]      # chunks: ok, bad, ok
    session.record_reference(state, [row, [V] + row[1:]], [2, 0])
    ring = state.items                                    # count stays 0: the encoder's to move
    assert ring[2].tolist() == list(range(1, 17)) + [7, 8, -1, -1]
    assert ring[0].tolist() == [7, 8] + [-1] * 18         # row 1's chunk 0 is masked too
    assert torch.equal(ring[[1, 3]], torch.full((2, S), -1))


# ---- the ring through the public calls, CPU state ----------------------------------
def test_cpu_state_remembers_the_last_five_events():
    L, S, N = 12, 5, 6
    model, _ = _model(torch.device("cpu"), L=L)
    plain = model.session_open(N, L)
    assert plain.items is None
    with pytest.raises(ValueError, match="history"):
        plain.history()
    state = model.session_open(N, L, history=S)
    sim = Simulation(N, S)

    def check():
        ids, n = state.history()
        want_ids, want_n = sim.history()
        assert torch.equal(ids, want_ids) and torch.equal(n, want_n)
        assert torch.equal(state.items, sim.ring())
        assert state.count.tolist() == sim.count
        part, n_part = state.history([4, 1])
        assert torch.equal(part, want_ids[[4, 1]]) and torch.equal(n_part, want_n[[4, 1]])

    check()
    seq, lens = _sequences(L, [L, 7, 3, 0])
    slots = [4, 0, 2, 5]
    for t in range(L):                                    # step: item 0 = no event
        session.step_reference(model, state, seq[:, t], slots)
        session.step_reference(model, plain, seq[:, t], slots)
        sim.feed(seq[:, t:t + 1].tolist(), slots)
    check()
    bad = seq.clone()
    bad[1, 2] = V                                         # masks row 1's (only) chunk
    session.append(model, state, bad, slots=slots)        # a CPU state: append_reference
    session.append(model, plain, bad, slots=slots)
    sim.feed(bad.tolist(), slots)
    check()
    assert state.status.tolist() == [session.STEPPED, session.BAD_ITEM, session.STEPPED,
                                     session.NO_EVENT]
    wide, wlens = _sequences(35, [35, 17, 1], seed=4)
    session.append(model, state, wide, wlens, slots=[1, 4, 3])
    session.append(model, plain, wide, wlens, slots=[1, 4, 3])
    sim.feed(wide.tolist(), [1, 4, 3])
    check()
    # the feature changes nothing in the encoder
    for a, b in zip(_state_tensors(state), _state_tensors(plain)):
        assert torch.equal(a, b)
    session.prefill(model, state, seq[:2], lens[:2], slots=[3, 5])     # method="steps", reset
    sim.reset([3, 5])
    sim.feed(seq[:2].tolist(), [3, 5])
    check()
    session.append(model, state, seq[2:3], slots=[0], reset=True)
    sim.reset([0])
    sim.feed(seq[2:3].tolist(), [0])
    check()
    state.reset([4, 2])
    sim.reset([4, 2])
    check()
    ids, n = state.history([4, 2])
    assert n.tolist() == [0, 0] and torch.equal(ids, torch.full((2, S), -1))
    assert torch.equal(state.items[[4, 2]], torch.full((2, S), -1))


# ---- recommend on a CPU state ------------------------------------------------------
def _exclusion(sim, slots):
    return torch.tensor([sim.ring_row(s) if 0 <= s < sim.N else [-1] * sim.S for s in slots])


@pytest.mark.parametrize("k", [1, 10])
def test_recommend_on_a_cpu_state(k):
    L, S, N = 12, 5, 6
    model, _ = _model(torch.device("cpu"), L=L)
    emb = model.item_embedding.weight.detach()
    state, twin = model.session_open(N, L, history=S), model.session_open(N, L)
    sim = Simulation(N, S)
    seq, _ = _sequences(L, [L, 7, 3, 0])
    slots = [4, 0, 2, 5]
    for t in range(8):
        items = seq[:, t]
        ids, scores = model.session_recommend(state, items, slots, k=k)
        y = session.step_reference(model, twin, items, slots)
        sim.feed(items[:, None].tolist(), slots)
        want = scoring._top_items_torch(y, emb, k, 1, _exclusion(sim, slots))
        assert torch.equal(ids[:3], want[0][:3]) and torch.equal(scores[:3], want[1][:3])
        assert state.status.tolist() == twin.status.tolist()
        for b, slot in enumerate(slots[:3]):
            assert not set(ids[b].tolist()) & (set(sim.last[slot]) | {0})
        # slot 5 has consumed nothing: its out is the zero row
        assert ids[3].tolist() == [-1] * k and torch.isneginf(scores[3]).all()
    assert state.count.tolist() == sim.count == twin.count.tolist()
    # no event: from the stored rows; the whole state, then named slots
    ids, scores = session.recommend(model, state, k=k)
    want = scoring._top_items_torch(state.out, emb, k, 1, _exclusion(sim, range(N)))
    live = [s for s in range(N) if sim.count[s]]
    dead = [s for s in range(N) if not sim.count[s]]
    assert dead and torch.equal(ids[live], want[0][live])
    assert torch.equal(scores[live], want[1][live])
    assert (ids[dead] == -1).all() and torch.isneginf(scores[dead]).all()
    ids2, scores2 = session.recommend(model, state, None, [2, 4], k=k)
    # (torch's CPU matmul is only reproducible for equal shapes: the same two rows)
    want = scoring._top_items_torch(state.out[[2, 4]], emb, k, 1, _exclusion(sim, [2, 4]))
    assert torch.equal(ids2, want[0]) and torch.equal(scores2, want[1])
    # several events per row, then the list; and without exclusion
    wide, _ = _sequences(20, [20, 2, 0, 5], seed=6)
    ids, scores = model.session_recommend(state, wide, slots, k=k)
    y = session.append_reference(model, twin, wide, slots=slots)
    sim.feed(wide.tolist(), slots)
    want = scoring._top_items_torch(y, emb, k, 1, _exclusion(sim, slots))
    assert torch.equal(ids[:3], want[0][:3]) and torch.equal(scores[:3], want[1][:3])
    assert torch.equal(state.items, sim.ring())
    ids, scores = model.session_recommend(state, None, slots[:3], k=k, exclude_seen=False)
    want = scoring._top_items_torch(state.out[slots[:3]], emb, k, 1, None)
    assert torch.equal(ids, want[0]) and torch.equal(scores, want[1])


def test_recommend_refusals():
    model, _ = _model(torch.device("cpu"), L=12)
    plain = model.session_open(3, 12)
    with pytest.raises(ValueError, match="history="):
        model.session_recommend(plain, [1, 2, 3])
    with pytest.raises(ValueError, match="history="):
        session.recommend(model, plain)
    ids, scores = model.session_recommend(plain, [1, 2, 0], exclude_seen=False, k=2)
    assert ids.shape == (3, 2) and ids[2].tolist() == [-1, -1] and (ids[:2] >= 1).all()
    assert plain.items is None
    with pytest.raises(ValueError, match="history must be >= 0"):
        model.session_open(3, 12, history=-1)
    model.train()
    with pytest.raises(ValueError, match="training mode"):
        model.session_recommend(plain, [1, 2, 3], exclude_seen=False)

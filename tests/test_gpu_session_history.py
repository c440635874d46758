"""The sessions' item ring on the GPU: rb_session_record against
session.record_reference, the ring through step / append / prefill beside a
state without one (whose encoder tensors must stay bitwise equal), the
launches the calls make, and session_recommend against scoring.top_items with
an exclusion matrix built on the host.

Every comparison is torch.equal: the ring holds integers, and the
recommendation is the same top-k kernel on the same inputs."""
import pytest
import torch

from datamining_recblr_amd import scoring, session
from test_gpu_session import V, _model, _sequences, _state_tensors
from test_session_history_host import Simulation, load_state, preload, row_mix

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(cuda):
    return _model(cuda)[0]            # d = 64, K = 4, L = 20, 2 layers


@pytest.fixture
def launches(monkeypatch):
    """(kernel, shape) of every record, step and append launch: a silent
    fallback to the torch path cannot pass."""
    calls = []

    def count(name, shape_of):
        orig = getattr(session, name)

        def counted(*args):
            calls.append((name, shape_of(args)))
            return orig(*args)

        monkeypatch.setattr(session, name, counted)

    count("_record_kernel", lambda a: tuple(a[1].shape))        # (state, items, slots, seen)
    count("_step_kernel", lambda a: (a[3].numel(),))            # (p, state, layers, items, ...)
    count("_append_kernel", lambda a: tuple(a[3].shape))
    return calls


def _names(calls):
    return [name for name, _ in calls]


# ---- the kernel against record_reference ---------------------------------------------
@pytest.mark.parametrize("S", [1, 3, 16, 20, 200])
@pytest.mark.parametrize("B", [5, 37])
def test_record_kernel_equals_the_reference(cuda, model, launches, B, S):
    N = 64
    widths = [0, 1, 2, 15, 16, 17, 35] + ([3 * S + 1] if S <= 20 else [])
    by_kernel, by_ref = (session.SessionState(model, N, 20, history=S) for _ in range(2))
    for W in widths:
        items, slots, held = row_mix(B, W, N, S)
        sim = Simulation(N, S)
        preload(sim, slots, held)
        load_state(by_kernel, sim)
        load_state(by_ref, sim)
        before = by_kernel.items.clone()
        items_d = torch.tensor(items, dtype=torch.int64).reshape(B, W).to(cuda)
        slots_d = torch.tensor(slots, device=cuda)
        seen = torch.full((B, S), -7, device=cuda, dtype=torch.int64)
        session._record_kernel(by_kernel, items_d, slots_d, seen)
        want_seen = session.record_reference(by_ref, items_d, slots_d, want_seen=True)
        assert torch.equal(by_kernel.items, by_ref.items), (W, S)
        assert torch.equal(seen, want_seen), (W, S)
        assert torch.equal(by_kernel.count, by_ref.count)
        # and both equal the plain-Python simulation
        want = torch.tensor(sim.feed(items, slots)).to(cuda)
        assert torch.equal(seen, want) and torch.equal(by_kernel.items, sim.ring().to(cuda))
        if W:
            assert not torch.equal(by_kernel.items, before)
        # without seen the ring is the same (count is as it was: record never writes it)
        by_ref.items.copy_(before)
        session._record_kernel(by_ref, items_d, slots_d, None)
        assert torch.equal(by_ref.items, by_kernel.items)
    assert _names(launches) == ["_record_kernel"] * (2 * len(widths))


def test_record_kernel_with_the_identity_slots(cuda, model):
    """slots NULL: row b is slot b."""
    B, N, S, W = 37, 40, 3, 35
    items, _, held = row_mix(B, W, N, S)
    sim = Simulation(N, S)
    preload(sim, range(B), held)
    state = session.SessionState(model, N, 20, history=S)
    load_state(state, sim)
    seen = torch.empty((B, S), device=cuda, dtype=torch.int64)
    session._record_kernel(state, torch.tensor(items, device=cuda), None, seen)
    assert torch.equal(seen, torch.tensor(sim.feed(items)).to(cuda))
    assert torch.equal(state.items, sim.ring().to(cuda))


# ---- through the public calls -----------------------------------------------------
def _same_encoder(a, b):
    for x, y in zip(_state_tensors(a), _state_tensors(b)):
        assert torch.equal(x, y)


def _check_ring(state, sim):
    assert torch.equal(state.items.cpu(), sim.ring())
    assert state.count.tolist() == sim.count
    ids, n = state.history()
    want_ids, want_n = sim.history()
    assert torch.equal(ids.cpu(), want_ids) and torch.equal(n.cpu(), want_n)


def test_the_ring_follows_the_public_calls_and_the_encoder_does_not_notice(cuda, model, launches):
    L, S, N, B = 20, 20, 48, 37
    ring, plain = model.session_open(N, L, history=S), model.session_open(N, L)
    assert plain.items is None and ring.items.shape == (N, S)
    sim = Simulation(N, S)
    slots = torch.randperm(N, generator=torch.Generator().manual_seed(9))[:B]
    slots_d = slots.to(cuda)
    seq, lens = _sequences(L, [(L, 0, 1, 7, L - 1)[b % 5] for b in range(B)])
    seq_d = seq.to(cuda)
    for t in range(9):                                            # a step loop, ragged
        ya = session.step(model, ring, seq_d[:, t], slots_d)
        yb = session.step(model, plain, seq_d[:, t], slots_d)
        assert torch.equal(ya, yb) and torch.equal(ring.status, plain.status)
        sim.feed(seq[:, t:t + 1].tolist(), slots.tolist())
    _same_encoder(ring, plain)
    _check_ring(ring, sim)
    assert _names(launches) == ["_record_kernel", "_step_kernel", "_step_kernel"] * 9
    for W in range(1, 36):                                        # append, widths 1 .. 35
        wide, wlens = _sequences(W, [(W, 0, 1, W // 2, W - 1)[(b + W) % 5] for b in range(B)],
                                 seed=W)
        if W in (17, 35):                                         # BAD_ITEM in chunk 0 / chunk 1
            wide[3, 1], wide[8, 16] = V, -1
            wide *= torch.arange(W)[None] < wlens[:, None]
        del launches[:]
        ya = session.append(model, ring, wide.to(cuda), wlens, slots_d)
        yb = session.append(model, plain, wide.to(cuda), wlens, slots_d)
        assert torch.equal(ya, yb) and torch.equal(ring.status, plain.status)
        longest = int(wlens.max())                                # host lengths cut the width
        n_app = -(-longest // 16)
        assert _names(launches) == ["_record_kernel"] + ["_append_kernel"] * (2 * n_app)
        assert launches[0][1] == (B, longest)
        sim.feed(wide.tolist(), slots.tolist())
    _same_encoder(ring, plain)
    _check_ring(ring, sim)
    some = slots[:11]                                             # append(reset=True)
    session.append(model, ring, seq_d[:11], lens[:11], some.to(cuda), reset=True)
    session.append(model, plain, seq_d[:11], lens[:11], some.to(cuda), reset=True)
    sim.reset(some.tolist())
    sim.feed(seq[:11].tolist(), some.tolist())
    _same_encoder(ring, plain)
    _check_ring(ring, sim)
    some = slots[20:33]                                           # prefill, both methods
    session.prefill(model, ring, seq[20:33], lens[20:33], some.tolist())
    session.prefill(model, plain, seq[20:33], lens[20:33], some.tolist())
    sim.reset(some.tolist())
    sim.feed(seq[20:33].tolist(), some.tolist())
    _same_encoder(ring, plain)
    _check_ring(ring, sim)
    del launches[:]
    session.prefill(model, ring, seq, lens, slots.tolist(), method="forward")
    session.prefill(model, plain, seq, lens, slots.tolist(), method="forward")
    assert launches == [("_record_kernel", (int((lens > 0).sum()), L))]
    sim.reset(slots.tolist())
    sim.feed(seq.tolist(), slots.tolist())
    _same_encoder(ring, plain)
    _check_ring(ring, sim)
    assert ring.count[slots_d].tolist() == lens.tolist()
    ids, n = ring.history(slots_d)                                # the last 20 of each history
    assert n.tolist() == lens.tolist() and torch.equal(ids.cpu(), seq + (seq == 0) * -1)


def test_a_long_history_keeps_its_last_twenty(cuda, model, launches):
    """prefill(method="forward") at a window longer than the ring."""
    L, S, B = 52, 20, 6
    long_model = _model(cuda, L=L)[0]
    seq, lens = _sequences(L, [L, 21, 20, 19, 1, 33])
    state = long_model.session_open(B, L, history=S)
    session.prefill(long_model, state, seq, lens, method="forward")
    assert launches == [("_record_kernel", (B, L))]
    ids, n = state.history()
    assert state.count.tolist() == lens.tolist() and n.tolist() == [min(x, S) for x in lens.tolist()]
    for b, x in enumerate(lens.tolist()):
        assert ids[b, :min(x, S)].tolist() == seq[b, max(x - S, 0):x].tolist()
        assert ids[b, min(x, S):].tolist() == [-1] * (S - min(x, S))


def test_a_state_without_a_ring_makes_no_record_launch(cuda, model, launches):
    L, B = 20, 5
    state = model.session_open(B, L)
    seq, lens = _sequences(L, [L, 3, 0, 17, 9])
    session.step(model, state, seq[:, 0].to(cuda))
    session.append(model, state, seq.to(cuda), lens)
    session.prefill(model, state, seq, lens)
    session.prefill(model, state, seq, lens, method="forward")
    model.session_recommend(state, seq[:, 1].to(cuda), exclude_seen=False)
    assert state.items is None
    assert "_record_kernel" not in _names(launches) and len(launches) == 1 + 2 + L + 1


# ---- session_recommend ------------------------------------------------------------
def _exclusion(sim, slots, dev):
    return torch.tensor([sim.ring_row(s) if 0 <= s < sim.N else [-1] * sim.S
                         for s in slots]).to(dev)


@pytest.mark.parametrize("k", [1, 10])
def test_session_recommend_equals_top_items_on_the_twin(cuda, model, launches, k):
    L, S, N, B = 20, 20, 40, 21
    emb = model.item_embedding.weight
    state, twin = model.session_open(N, L, history=S), model.session_open(N, L)
    sim = Simulation(N, S)
    slots = torch.randperm(N, generator=torch.Generator().manual_seed(k))[:B].tolist()
    slots[4], slots[9] = -1, N                                    # bad slots ride as a device tensor
    slots_d = torch.tensor(slots, device=cuda)
    seq, _ = _sequences(30, [(30, 30, 2, 30, 30)[b % 5] for b in range(B)])
    seq[6] = 0                                                    # a slot that never gets an event
    seq_d = seq.to(cuda)

    def check(ids, scores, y, exclude=True):
        M = _exclusion(sim, slots, cuda) if exclude else None
        want_ids, want_scores = scoring.top_items(y, emb, k, exclude=M)
        live = torch.tensor([0 <= s < N and sim.count[s] > 0 for s in slots], device=cuda)
        assert torch.equal(ids[live], want_ids[live])
        assert torch.equal(scores[live], want_scores[live])
        assert (ids[~live] == -1).all() and torch.isneginf(scores[~live]).all()
        assert ids.shape == (B, k) and ids.dtype == torch.int64 and scores.dtype == torch.float32
        if exclude:
            for b in torch.nonzero(live).reshape(-1).tolist():
                assert not set(ids[b].tolist()) & (set(sim.last[slots[b]]) | {0, -1})
        return live

    for t in range(25):                                           # past the ring's 20 entries
        del launches[:]
        ids, scores = model.session_recommend(state, seq_d[:, t], slots_d, k=k)
        assert launches == [("_record_kernel", (B, 1)), ("_step_kernel", (B,))]
        y = session.step(model, twin, seq_d[:, t], slots_d)
        sim.feed(seq[:, t:t + 1].tolist(), slots)
        live = check(ids, scores, y)
        assert torch.equal(state.status, twin.status)
    assert live.tolist() == [b not in (4, 6, 9) for b in range(B)]
    assert max(sim.count) == 25 > S
    # several events per row: one record launch, ceil(W / 16) append launches
    wide, _ = _sequences(35, [(35, 0, 17, 1, 16)[b % 5] for b in range(B)], seed=11)
    wide[6] = 0
    del launches[:]
    ids, scores = model.session_recommend(state, wide.to(cuda), slots_d, k=k)
    assert launches == [("_record_kernel", (B, 35)), ("_append_kernel", (B, 16)),
                        ("_append_kernel", (B, 16)), ("_append_kernel", (B, 4))]
    y = session.append(model, twin, wide.to(cuda), slots=slots_d)
    sim.feed(wide.tolist(), slots)
    check(ids, scores, y)
    assert torch.equal(state.status, twin.status)
    _same_encoder(state, twin)
    # no event: the stored rows; the record launch only hands the rings over
    status = state.status.clone()
    before = [t.clone() for t in (*_state_tensors(state), state.items)]
    del launches[:]
    ids, scores = model.session_recommend(state, None, slots_d, k=k)
    assert launches == [("_record_kernel", (B, 0))]
    y = session.step(model, twin, torch.zeros(B, dtype=torch.int64, device=cuda), slots_d)
    check(ids, scores, y)
    for now, was in zip((*_state_tensors(state), state.items), before):
        assert torch.equal(now, was)
    assert torch.equal(state.status, status)
    # without exclusion: top_items without a list, and no seen rows
    del launches[:]
    ids, scores = model.session_recommend(state, None, slots_d, k=k, exclude_seen=False)
    assert launches == []
    check(ids, scores, y, exclude=False)
    ids, scores = model.session_recommend(state, seq_d[:, 25], slots_d, k=k, exclude_seen=False)
    y = session.step(model, twin, seq_d[:, 25], slots_d)
    sim.feed(seq[:, 25:26].tolist(), slots)
    check(ids, scores, y, exclude=False)
    assert torch.equal(state.items.cpu(), sim.ring())             # still recorded
    # the whole state, slots None
    ids, scores = model.session_recommend(state, k=k)
    want_ids, want_scores = scoring.top_items(state.out, emb, k,
                                              exclude=_exclusion(sim, range(N), cuda))
    live = state.count > 0
    assert 0 < int(live.sum()) < N
    assert torch.equal(ids[live], want_ids[live]) and torch.equal(scores[live], want_scores[live])
    assert (ids[~live] == -1).all() and torch.isneginf(scores[~live]).all()


def test_recommend_refuses_what_it_cannot_honour(cuda, model):
    plain = model.session_open(3)
    with pytest.raises(ValueError, match="history="):
        model.session_recommend(plain, [1, 2, 3])
    state = model.session_open(3, history=4)
    model.train()
    try:
        with pytest.raises(ValueError, match="training mode"):
            model.session_recommend(state, [1, 2, 3])
        with pytest.raises(ValueError, match="training mode"):
            model.session_recommend(state)
    finally:
        model.eval()
    ids, _ = model.session_recommend(state, [1, 2, 0], k=3)
    assert ids[2].tolist() == [-1] * 3 and 1 not in ids[0].tolist() and 2 not in ids[1].tolist()

"""session.prefill(method="forward") on the GPU: sessions opened from stored
histories by one packed forward and one rb_session_capture launch per layer,
against the state that method="steps" (a step loop) builds.

Bar for values: test_gpu_e2e.close (1e-4 abs + 1e-4 rel + 2e-6 max|ref|), the
project's forward-vs-oracle bar; the two methods differ by the forward's f16x3
projections against the step's fp32 MFMA, so they agree to rounding, not
bitwise.  What concerns a slot's independence of its neighbours, of the row
order and of earlier calls is torch.equal."""
import pytest
import torch

from datamining_recblr_amd import session
from oracle import recblr_oracle as orc
from test_gpu_e2e import close
from test_gpu_session import V, _model, _sequences, _state_tensors

pytestmark = pytest.mark.gpu


@pytest.fixture
def launches(monkeypatch):
    """Counts rb_session_step and rb_session_capture launches."""
    calls = {"step": 0, "capture": 0}

    def counted(name, orig):
        def fn(*args, **kw):
            calls[name] += 1
            return orig(*args, **kw)
        return fn

    monkeypatch.setattr(session, "_step_kernel", counted("step", session._step_kernel))
    monkeypatch.setattr(session, "_capture_kernel", counted("capture", session._capture_kernel))
    return calls


def _cycle_lengths(B, L):
    cyc = [1, 2, 3, 4, 15, 16, 17, 31, 32, 33, L]
    return [min(cyc[b % len(cyc)], L) for b in range(B)]


def _named(state):
    out = {f"h[{i}]": h for i, h in enumerate(state.h)}
    out.update({f"conv[{i}]": c for i, c in enumerate(state.conv) if c is not None})
    out["out"] = state.out
    return out


def _both(model, L, lens, slots=None, capacity=None):
    """The same histories prefilled by steps and by one forward."""
    dev = next(model.parameters()).device
    seq, lens = _sequences(L, lens)
    B = len(lens)
    by_steps = model.session_open(capacity or B, L)
    by_fwd = model.session_open(capacity or B, L)
    ys = model.session_prefill(by_steps, seq.to(dev), lens, slots)
    yf = model.session_prefill(by_fwd, seq.to(dev), lens, slots, method="forward")
    return by_steps, by_fwd, ys, yf


def _assert_same_state(by_steps, by_fwd, ys, yf, what=""):
    close(yf, ys, what=f"{what} returned rows")
    for (name, a), b in zip(_named(by_fwd).items(), _named(by_steps).values()):
        close(a, b, what=f"{what} {name}")
    assert torch.equal(by_fwd.count, by_steps.count)


def test_forward_prefill_launches_no_step_and_one_capture_per_layer(cuda, launches):
    L = 20
    model, _ = _model(cuda, 64, 4, L, 2)
    seq, lens = _sequences(L, [L, 7, 1, 16, 17])
    state = model.session_open(5, L)
    y = model.session_prefill(state, seq.to(cuda), lens, method="forward")
    assert launches == {"step": 0, "capture": 2}
    assert y.shape == (5, 64) and state.count.tolist() == lens.tolist()
    assert state.status.tolist() == [session.STEPPED] * 5
    with torch.no_grad():
        assert torch.equal(y, model(seq.to(cuda), lens.to(cuda)))
    assert torch.equal(y, state.out)


@pytest.mark.parametrize("L", [40, 32])   # pad prefix 24 and 0
def test_state_equals_the_step_built_state(cuda, launches, L):
    assert orc.pow2_pad_len(L) == (24 if L == 40 else 0)
    model, _ = _model(cuda, 64, 4, L, 2)
    got = _both(model, L, _cycle_lengths(37, L))
    _assert_same_state(*got, what=f"L={L}")
    assert launches["capture"] == 2 and launches["step"] == L


@pytest.mark.parametrize("d,K,L,layers,B,flags", [
    (48, 4, 20, 2, 9, {}),                      # H = 96: the channel tail
    (64, 1, 20, 2, 9, {}),
    (64, 2, 20, 2, 9, {}),
    (64, 8, 20, 2, 9, {}),
    (64, 4, 20, 2, 9, {"disable_conv1d": True}),
    (64, 4, 20, 2, 9, {"disable_ffn": True}),
    (64, 4, 20, 2, 9, {"bd_lru_only": True}),
    (64, 4, 20, 1, 9, {}),
    (64, 4, 20, 2, 1, {}),
    (256, 4, 9, 1, 5, {}),                      # (d, H) = (256, 512)
], ids=lambda v: "-".join(v) if isinstance(v, dict) else str(v))
def test_further_shapes(cuda, launches, d, K, L, layers, B, flags):
    model, _ = _model(cuda, d, K, L, layers, **flags)
    lens = [L] if B == 1 else [min(n, L) for n in (L, 1, 2, 3, 7, 8, 16, 17, 19)][:B]
    got = _both(model, L, lens)
    _assert_same_state(*got, what=f"d={d} K={K} {flags}")
    assert launches["capture"] == layers


def test_the_state_is_usable(cuda, launches):
    """Three more events per slot after the forward prefill, each against the
    CPU oracle on the extended history."""
    L = 20
    model, cfg = _model(cuda, 64, 4, L, 2)
    lens0 = torch.tensor([1, 2, 3, 4, 13, 14, 15, 16, 17])
    seq, _ = _sequences(L, [L] * len(lens0))
    state = model.session_open(len(lens0), L)
    model.session_prefill(state, seq.to(cuda), lens0, method="forward")
    params = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    for extra in range(1, 4):
        lens = lens0 + extra
        assert int(lens.max()) <= L
        items = seq[torch.arange(len(lens0)), lens - 1]
        y = model.session_step(state, items.to(cuda))
        close(y, orc.model_forward(params, cfg, seq, lens), what=f"event {extra}")
        assert state.count.tolist() == lens.tolist()
    assert launches == {"step": 3, "capture": 2}


def test_scattered_slots_row_order_and_repetition(cuda, launches):
    L, N, B = 20, 60, 17
    model, _ = _model(cuda, 64, 4, L, 2)
    g = torch.Generator().manual_seed(5)
    slots = torch.randperm(N, generator=g)[:B]
    order = torch.randperm(B, generator=g)
    seq, lens = _sequences(L, _cycle_lengths(B, L))
    seq = seq.to(cuda)
    base, perm = model.session_open(N, L), model.session_open(N, L)
    # make the untouched slots recognisable
    for st in (base, perm):
        for t in _state_tensors(st):
            t.copy_(torch.arange(t.numel(), device=cuda).reshape(t.shape) % 7)
    before = [t.clone() for t in _state_tensors(base)]
    ya = model.session_prefill(base, seq, lens, slots.tolist(), method="forward")
    yb = model.session_prefill(perm, seq[order.to(cuda)], lens[order], slots[order].to(cuda),
                               method="forward")
    assert torch.equal(ya[order.to(cuda)], yb)
    others = torch.tensor(sorted(set(range(N)) - set(slots.tolist())), device=cuda)
    assert others.numel() == N - B
    for now, was, other in zip(_state_tensors(base), before, _state_tensors(perm)):
        assert torch.equal(now[others], was[others])
        assert torch.equal(now, other)
        assert not torch.equal(now[slots.to(cuda)], was[slots.to(cuda)])
    assert base.count[slots.to(cuda)].tolist() == lens.tolist()
    # the same call again: the same state, bit for bit
    kept = [t.clone() for t in _state_tensors(base)]
    yc = model.session_prefill(base, seq, lens, slots.tolist(), method="forward")
    assert torch.equal(yc, ya)
    for now, was in zip(_state_tensors(base), kept):
        assert torch.equal(now, was)
    assert launches == {"step": 0, "capture": 6}


def test_rows_of_length_zero_are_reset_and_left_alone(cuda, launches):
    L = 20
    model, _ = _model(cuda, 64, 4, L, 2)
    seq, lens = _sequences(L, [5, 0, 17, 0, 1, L])
    seq = seq.to(cuda)
    full = model.session_open(6, L)
    for t in range(3):   # the slots hold something that the reset has to clear
        session.step(model, full, seq[:, 0].clamp(min=1))
    y = model.session_prefill(full, seq, lens, method="forward")
    fresh = model.session_open(6, L)
    live = torch.tensor([0, 2, 4, 5], device=cuda)
    empty = torch.tensor([1, 3], device=cuda)
    for now, init in zip(_state_tensors(full), _state_tensors(fresh)):
        assert torch.equal(now[empty], init[empty])
    assert not y[empty].any()
    assert full.status.tolist() == [session.STEPPED, session.NO_EVENT, session.STEPPED,
                                    session.NO_EVENT, session.STEPPED, session.STEPPED]
    # the other rows: as a call without the empty ones
    part = model.session_open(6, L)
    yp = model.session_prefill(part, seq[live], lens[live.cpu()], live, method="forward")
    assert torch.equal(y[live], yp)
    for now, other in zip(_state_tensors(full), _state_tensors(part)):
        assert torch.equal(now[live], other[live])
    # and a call with no history at all
    y0 = model.session_prefill(full, seq, torch.zeros(6, dtype=torch.int64), method="forward")
    assert not y0.any() and full.count.tolist() == [0] * 6
    assert full.status.tolist() == [session.NO_EVENT] * 6
    assert launches["capture"] == 4


@pytest.mark.parametrize("d,K", [(64, 4), (48, 8)])
def test_kernel_equals_its_restatement(cuda, monkeypatch, d, K):
    """rb_session_capture against session.capture_reference on the same
    captured tensors of a forward."""
    L = 40
    model, _ = _model(cuda, d, K, L, 2)
    seq, lens = _sequences(L, _cycle_lengths(23, L))
    state = model.session_open(30, L)
    orig, seen = session._capture_kernel, []

    def both(state_, i, u, xc, rg, lam, gate_b, carries, packed, slots, K_):
        h_ref, conv_ref = state_.h[i].clone(), state_.conv[i].clone()
        session.capture_reference(u, xc, rg, lam, gate_b, carries, packed.offsets, slots,
                                  h_ref, conv_ref)
        orig(state_, i, u, xc, rg, lam, gate_b, carries, packed, slots, K_)
        seen.append((i, h_ref, conv_ref))

    monkeypatch.setattr(session, "_capture_kernel", both)
    slots = torch.arange(23) + 4
    model.session_prefill(state, seq.to(cuda), lens, slots.tolist(), method="forward")
    assert [i for i, _, _ in seen] == [0, 1]
    for i, h_ref, conv_ref in seen:
        close(state.h[i], h_ref, what=f"h[{i}]")
        assert torch.equal(state.conv[i], conv_ref)       # copies
        assert not torch.equal(state.h[i][4:27], model.session_open(30, L).h[i][4:27])


def test_a_forward_without_capture_is_what_it_was(cuda, launches):
    """capture=None is inert: forward() before and after a forward prefill,
    and on an identically built model that never ran one, gives the same bits
    (no_grad and with autograd's carries)."""
    L = 20
    used, _ = _model(cuda, 64, 4, L, 2)
    never, _ = _model(cuda, 64, 4, L, 2)
    seq, lens = _sequences(L, _cycle_lengths(13, L))
    seq, lens = seq.to(cuda), lens.to(cuda)
    with torch.no_grad():
        before = used(seq, lens)
    before_grad = used(seq, lens)
    used.session_prefill(used.session_open(13, L), seq, lens, method="forward")
    assert launches["capture"] == 2
    with torch.no_grad():
        after, other = used(seq, lens), never(seq, lens)
    assert torch.equal(before, after) and torch.equal(before, other)
    after_grad = never(seq, lens)
    assert torch.equal(before_grad, after_grad) and torch.equal(before_grad, before)
    after_grad.sum().backward()      # the backward takes the extra None
    assert never.item_embedding.weight.grad is not None

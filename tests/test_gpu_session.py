"""Stateful session inference on the GPU: session.step (one rb_session_step
launch for the whole encoder step) against the CPU oracle and RecBLR.forward
at every prefix, its bitwise independence of tiling / batch / slot order, the
no-event and out-of-range rows, prefill, reset, the refusals and the fallback.

Bar for values: test_gpu_e2e.close (1e-4 abs + 1e-4 rel + 2e-6 max|ref|), the
project's forward-vs-oracle bar.  Everything about a slot's independence of
its neighbours is torch.equal."""
import pytest
import torch

from datamining_recblr_amd import _lib, session
from model_grad_reference import build_model
from oracle import recblr_oracle as orc
from test_gpu_e2e import close

pytestmark = pytest.mark.gpu

V = 200


def _model(dev, d=64, K=4, L=20, layers=2, **flags):
    # off the init's zeros / ones / N(0, 0.02): every term matters
    model, cfg = build_model(V, d, K, L, layers, **flags)
    return model.to(dev), cfg


def _sequences(L, lens, seed=2):
    g = torch.Generator().manual_seed(seed)
    lens = torch.as_tensor(lens)
    seq = torch.randint(1, V, (len(lens), L), generator=g)
    return seq * (torch.arange(L)[None] < lens[:, None]), lens


@pytest.fixture
def step_launches(monkeypatch):
    """Counts rb_session_step launches: a silent fallback cannot pass."""
    calls = []
    orig = session._step_kernel

    def counted(p, state, layers, items, *args):
        calls.append(items.numel())
        return orig(p, state, layers, items, *args)

    monkeypatch.setattr(session, "_step_kernel", counted)
    return calls


def _state_tensors(state):
    return [*state.h, *[c for c in state.conv if c is not None], state.count, state.out]


def _check_against_oracle(model, cfg, L, step_launches=None, step=session.step):
    dev = next(model.parameters()).device
    seq, lens = _sequences(L, [L, L - 3, 7, 2, 1])
    state = model.session_open(5, L)
    ys = [step(model, state, seq[:, t].to(dev)) for t in range(L)]
    statuses = state.status.tolist()
    params = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    for t, y in enumerate(ys):
        ref = orc.model_forward(params, cfg, seq, torch.clamp(lens, max=t + 1))
        close(y, ref, what=f"step {t}")
    assert state.count.tolist() == lens.tolist()
    assert statuses == [session.STEPPED] + [session.NO_EVENT] * 4
    if step_launches is not None:
        assert step_launches == [5] * L


@pytest.mark.parametrize("d,K,L,layers", [(64, 4, 20, 2), (128, 4, 12, 2), (64, 2, 16, 1),
                                          (64, 1, 9, 1), (64, 8, 20, 1)])
def test_kernel_equals_the_oracle_at_every_prefix(cuda, step_launches, d, K, L, layers):
    model, cfg = _model(cuda, d, K, L, layers)
    _check_against_oracle(model, cfg, L, step_launches)


def test_the_largest_required_shape_runs_on_the_kernel(cuda, step_launches):
    """(d, H) = (256, 512): 145 KiB of the compute unit's 160 KiB of LDS."""
    model, cfg = _model(cuda, 256, 4, 9, 1)
    _check_against_oracle(model, cfg, 9, step_launches)


@pytest.mark.parametrize("flags", [{"disable_conv1d": True}, {"disable_ffn": True},
                                   {"bd_lru_only": True}], ids=lambda f: "-".join(f))
def test_kernel_equals_the_oracle_for_the_flag_variants(cuda, step_launches, flags):
    model, cfg = _model(cuda, 64, 4, 12, 2, **flags)
    _check_against_oracle(model, cfg, 12, step_launches)


def test_kernel_equals_model_forward_at_every_step(cuda, step_launches):
    L, B = 20, 33
    model, _ = _model(cuda, 128, 4, L, 2)
    seq, lens = _sequences(L, [1 + b % L for b in range(B)])
    seq, lens = seq.to(cuda), lens.to(cuda)
    state = model.session_open(B)
    assert state.seq_len == L
    with torch.no_grad():
        for t in range(L):
            y = model.session_step(state, seq[:, t])
            close(y, model(seq, torch.clamp(lens, max=t + 1)), what=f"step {t}")
    assert step_launches == [B] * L


def test_a_slot_does_not_depend_on_its_tile_or_batch(cuda, step_launches):
    L, T = 12, 10
    model, _ = _model(cuda, 64, 4, L, 2)
    seq, _ = _sequences(L, [L] * 33)
    seq = seq.to(cuda)
    runs = []
    for B in (1, 17, 33):          # the sequence rides in the last row: tile 0, 1, 2
        rows = torch.cat([seq[1:B], seq[:1]])
        state = model.session_open(B, L)
        runs.append(torch.stack([session.step(model, state, rows[:, t])[B - 1]
                                 for t in range(T)]))
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert step_launches == [1] * T + [17] * T + [33] * T


def test_scattered_slots_in_any_order(cuda, step_launches):
    L, T, N = 12, 6, 40
    model, _ = _model(cuda, 64, 4, L, 2)
    g = torch.Generator().manual_seed(5)
    slots = torch.randperm(N, generator=g)[:17]
    order = torch.randperm(17, generator=g)
    seq, _ = _sequences(L, [L] * 17)
    seq = seq.to(cuda)
    base, perm = model.session_open(N, L), model.session_open(N, L)
    before = [t.clone() for t in _state_tensors(base)]
    for t in range(T):
        ya = session.step(model, base, seq[:, t], slots.tolist())
        yb = session.step(model, perm, seq[order.to(cuda), t], slots[order].to(cuda))
        assert torch.equal(ya[order.to(cuda)], yb)
    others = torch.tensor(sorted(set(range(N)) - set(slots.tolist())), device=cuda)
    assert others.numel() == 23
    for now, was, other in zip(_state_tensors(base), before, _state_tensors(perm)):
        assert torch.equal(now[others], was[others])
        assert torch.equal(now, other)
    # and the identity order over the first 17 slots gives the same rows
    ident = model.session_open(17, L)
    for t in range(T):
        yi = session.step(model, ident, seq[:, t])
    assert torch.equal(yi, ya)
    assert len(step_launches) == 3 * T


def test_no_event_rows(cuda, step_launches):
    L, B = 12, 20
    model, _ = _model(cuda, 64, 4, L, 2)
    seq, _ = _sequences(L, [L] * B)
    seq = seq.to(cuda)
    dense, sparse = model.session_open(B, L), model.session_open(B, L)
    for t in range(4):
        yd = session.step(model, dense, seq[:, t])
    # a call with no event at all changes nothing and returns the stored rows
    before = [t.clone() for t in _state_tensors(dense)]
    y0 = session.step(model, dense, torch.zeros(B, dtype=torch.int64, device=cuda))
    assert torch.equal(y0, yd) and torch.equal(y0, dense.out)
    assert dense.status.tolist() == [session.NO_EVENT] * B
    for now, was in zip(_state_tensors(dense), before):
        assert torch.equal(now, was)
    # odd rows skip every other call and catch up afterwards: same per-row results
    odd = (torch.arange(B, device=cuda) % 2 == 1)
    fed = torch.zeros(B, dtype=torch.int64, device=cuda)
    call = 0
    while int(fed.min()) < 4:
        go = (fed < 4) & (~odd | (call % 2 == 0))
        items = torch.where(go, seq[torch.arange(B, device=cuda), fed.clamp(max=L - 1)], 0)
        ys = session.step(model, sparse, items)
        fed += go
        call += 1
    assert call > 4
    assert torch.equal(ys, yd)
    for a, b in zip(_state_tensors(sparse), _state_tensors(dense)):
        assert torch.equal(a, b)
    assert all(n == B for n in step_launches)


def test_prefill_then_step_and_reset_replay(cuda, step_launches):
    L, B = 12, 6
    model, _ = _model(cuda, 64, 4, L, 2)
    seq, lens = _sequences(L, [9, 4, 11, 1, 6, 8])
    nxt = torch.tensor([3, 9, 0, 7, 5, 2], device=cuda)
    scratch = model.session_open(B, L)
    for t in range(int(lens.max())):
        ys = session.step(model, scratch, seq[:, t].to(cuda))
    y_next = session.step(model, scratch, nxt)

    state = model.session_open(B, L)
    yp = model.session_prefill(state, seq, lens)
    assert torch.equal(yp, ys)
    assert torch.equal(model.session_step(state, nxt), y_next)
    for a, b in zip(_state_tensors(state), _state_tensors(scratch)):
        assert torch.equal(a, b)
    # reset two slots, replay their histories: the other slots keep theirs
    state.reset([1, 4])
    assert state.count.tolist() == [10, 0, 11, 2, 0, 9]
    model.session_prefill(state, seq[[1, 4]], lens[[1, 4]], slots=[1, 4])
    session.step(model, state, nxt[[1, 4]], [1, 4])
    for a, b in zip(_state_tensors(state), _state_tensors(scratch)):
        assert torch.equal(a, b)
    assert len(step_launches) > 0


def test_refusals_name_their_cause(cuda, step_launches):
    L = 12
    model, _ = _model(cuda, 64, 4, L, 1)
    state = model.session_open(2, L)
    model.train()
    with pytest.raises(ValueError, match="training mode"):
        session.step(model, state, [1, 2])
    model.eval()
    handle = model.recurrent_layers[0].behavior_modeling.register_forward_hook(lambda *a: None)
    with pytest.raises(_lib.RecBLRNativeError, match="recurrent_layers.0.behavior_modeling"):
        session.step(model, state, [1, 2])
    handle.remove()
    other, _ = _model(cuda, 64, 4, L, 2)
    with pytest.raises(ValueError, match="different model shape"):
        session.step(other, state, [1, 2])
    with pytest.raises(ValueError, match="unique"):
        session.step(model, state, [1, 2], [0, 0])
    session.step(model, state, [1, 2])           # and it runs once nothing stands in the way
    model.to(torch.bfloat16)
    with pytest.raises(_lib.RecBLRNativeError, match="bfloat16"):
        session.step(model, state, [1, 2])
    assert step_launches == [2]


def test_a_refused_shape_takes_the_reference_path(cuda, step_launches):
    """d = 24 is no multiple of the MFMA tile ((256, 512) fits the LDS and
    runs on the kernel): session.step falls back to step_reference."""
    assert session.kernel_supports(256, 512, 4, 2)
    assert not session.kernel_supports(24, 48, 4, 2)
    model, cfg = _model(cuda, 24, 4, 12, 2)
    _check_against_oracle(model, cfg, 12)
    assert step_launches == []


def test_out_of_range_item_is_masked_and_reported(cuda, step_launches):
    L, B = 12, 18
    model, _ = _model(cuda, 64, 4, L, 2)
    seq, _ = _sequences(L, [L] * B)
    seq = seq.to(cuda)
    good, bad = model.session_open(B, L), model.session_open(B, L)
    for t in range(3):
        session.step(model, good, seq[:, t])
        session.step(model, bad, seq[:, t])
    row = 16                                   # in the second tile, beside a live row
    kept = [t[row].clone() for t in _state_tensors(bad)]
    items = seq[:, 3].clone()
    yg = session.step(model, good, items)
    items[row] = V                             # first id past the table
    yb = session.step(model, bad, items)
    status = bad.status.tolist()
    assert status[row] == session.BAD_ITEM
    assert status[:row] + status[row + 1:] == [session.STEPPED] * (B - 1)
    for now, was in zip(_state_tensors(bad), kept):
        assert torch.equal(now[row], was)      # state, count and out untouched
    assert torch.equal(yb[row], bad.out[row])  # the stored row comes back
    keep = torch.arange(B, device=cuda) != row
    assert torch.equal(yb[keep], yg[keep])
    for a, b in zip(_state_tensors(bad), _state_tensors(good)):
        assert torch.equal(a[keep], b[keep])
    assert step_launches == [B] * 8

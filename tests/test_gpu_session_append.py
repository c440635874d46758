"""session.append on the GPU (rb_session_append: up to 16 events per slot in
one launch) against the step kernel it must equal bit for bit, the CPU oracle
and RecBLR.forward; its independence of batch, tile position and chunking; the
masked rows; and the launches it makes.

Everything against the step kernel is torch.equal: the append kernel's rows
run the step's GEMMs and LayerNorms, and its conv and scan use the step's
expressions in the step's order.  Bar for values against the oracle and
forward: test_gpu_e2e.close, the project's forward-vs-oracle bar."""
import pytest
import torch

from datamining_recblr_amd import session
from oracle import recblr_oracle as orc
from test_gpu_e2e import close
from test_gpu_session import V, _model, _sequences, _state_tensors

pytestmark = pytest.mark.gpu


@pytest.fixture
def append_launches(monkeypatch):
    """(B, T) of every rb_session_append launch: a silent fallback cannot pass."""
    calls = []
    orig = session._append_kernel

    def counted(p, state, layers, items, *args):
        calls.append(tuple(items.shape))
        return orig(p, state, layers, items, *args)

    monkeypatch.setattr(session, "_append_kernel", counted)
    return calls


def _launches(B, W):
    """ceil(W / 16) launches: 16 columns each, the last the smallest T that holds the rest."""
    full, r = divmod(W, 16)
    return [(B, 16)] * full + ([(B, next(t for t in (1, 2, 4, 8, 16) if t >= r))] if r else [])


def _same(a, b):
    for x, y in zip(_state_tensors(a), _state_tensors(b)):
        assert torch.equal(x, y)


def _live_pair(model, N, slots, K, L=20):
    """Two states advanced alike by step: the rows' slots hold 0, 1, K - 2,
    K - 1 and 9 events."""
    held = [(0, 1, max(K - 2, 0), K - 1, 9)[b % 5] for b in range(len(slots))]
    seq, _ = _sequences(9, held, seed=7)
    seq = seq.to(slots.device)
    a, b = model.session_open(N, L), model.session_open(N, L)
    for t in range(9):
        session.step(model, a, seq[:, t], slots)
        session.step(model, b, seq[:, t], slots)
    _same(a, b)
    return a, b, held


def _step_loop(model, state, seq, slots):
    y, per_event = None, []
    for t in range(seq.shape[1]):
        y = session.step(model, state, seq[:, t], slots)
        per_event.append(torch.where((state.status == session.STEPPED)[:, None], y,
                                     torch.zeros_like(y)))
    return y, torch.stack(per_event, 1)


def _check_bitwise(model, K, W, B, launches):
    dev = next(model.parameters()).device
    N = B + 3
    slots = torch.randperm(N, generator=torch.Generator().manual_seed(B))[:B].to(dev)
    by_step, by_append, held = _live_pair(model, N, slots, K)
    lens = [(W, 0, 1, W - 1, W // 2, min(W, 3), min(W, 17))[b % 7] for b in range(B)]
    seq, lens = _sequences(W, lens, seed=W)
    seq = seq.to(dev)
    y_ref, all_ref = _step_loop(model, by_step, seq, slots)
    y, y_all = session.append(model, by_append, seq, lens, slots, return_all=True)
    assert launches == _launches(B, W)
    assert torch.equal(y, y_ref)
    assert y_all.shape == all_ref.shape and torch.equal(y_all, all_ref)
    _same(by_append, by_step)
    assert by_append.count[slots].tolist() == [h + n for h, n in zip(held, lens.tolist())]
    assert by_append.status.tolist() == [session.STEPPED if n else session.NO_EVENT
                                         for n in lens.tolist()]


@pytest.mark.parametrize("B", [5, 37])
@pytest.mark.parametrize("W", [1, 2, 3, 4, 8, 16, 17, 35])
def test_append_is_bitwise_a_step_per_column(cuda, append_launches, W, B):
    model, _ = _model(cuda, 64, 4, 20, 2)
    _check_bitwise(model, 4, W, B, append_launches)


@pytest.mark.parametrize("B", [5, 37])
@pytest.mark.parametrize("d,K,layers", [(128, 4, 2), (64, 1, 1), (64, 8, 1)])
def test_append_is_bitwise_a_step_per_column_for_other_shapes(cuda, append_launches, d, K,
                                                              layers, B):
    model, _ = _model(cuda, d, K, 20, layers)
    _check_bitwise(model, K, 35, B, append_launches)


@pytest.mark.parametrize("B", [5, 37])
@pytest.mark.parametrize("flags", [{"disable_conv1d": True}, {"disable_ffn": True},
                                   {"bd_lru_only": True}], ids=lambda f: "-".join(f))
def test_append_is_bitwise_a_step_per_column_for_the_flag_variants(cuda, append_launches, flags,
                                                                   B):
    model, _ = _model(cuda, 64, 4, 20, 2, **flags)
    _check_bitwise(model, 4, 35, B, append_launches)


def test_the_largest_required_shape_runs_on_the_kernel(cuda, append_launches):
    """(d, H) = (256, 512) in one launch of W = 9 (T = 16), against the oracle."""
    L = 9
    model, cfg = _model(cuda, 256, 4, L, 1)
    seq, lens = _sequences(L, [L, L - 3, 7, 2, 1])
    state = model.session_open(5, L)
    y, y_all = session.append(model, state, seq, lens, return_all=True)
    assert append_launches == [(5, 16)]
    y_all = y_all.cpu()
    params = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    for t in range(L):
        ref = orc.model_forward(params, cfg, seq, torch.clamp(lens, max=t + 1))
        live = t < lens
        close(y_all[live, t], ref[live], what=f"event {t}")
        assert not y_all[~live, t].any()
    close(y, orc.model_forward(params, cfg, seq, lens), what="y")
    assert state.count.tolist() == lens.tolist()


def test_opening_sessions_equals_model_forward(cuda, append_launches):
    L, B = 20, 33
    model, _ = _model(cuda, 128, 4, L, 2)
    seq, lens = _sequences(L, [1 + b % L for b in range(B)])
    state = model.session_open(B)
    session.step(model, state, seq[:, 0].to(cuda))        # something for reset to clear
    y = model.session_append(state, seq, lens, reset=True)
    assert append_launches == [(B, 16), (B, 4)]
    with torch.no_grad():
        close(y, model(seq.to(cuda), lens.to(cuda)), what="append(reset=True) vs forward")
    assert state.count.tolist() == lens.tolist()
    assert state.status.tolist() == [session.STEPPED] * B


def test_a_slot_does_not_depend_on_its_batch_tile_or_chunking(cuda, append_launches):
    L = 20
    model, _ = _model(cuda, 64, 4, L, 2)
    seq, _ = _sequences(16, [16] * 37)
    seq = seq.to(cuda)
    runs = []
    for B, at in ((1, 0), (37, 35)):   # the sequence rides in row `at`
        rows = torch.cat([seq[1:at + 1], seq[:1], seq[at + 1:B]])
        for cut in ((16,), (5, 11)):   # T = 16: alone in its tile; T = 8: its first or second half
            state, c0, ys = model.session_open(B, L), 0, []
            for w in cut:
                y, y_all = session.append(model, state, rows[:, c0:c0 + w], return_all=True)
                ys.append(y_all[at])
                c0 += w
            runs.append((torch.cat(ys), y[at], [t[at].clone() for t in _state_tensors(state)]))
    for y_all, y, tensors in runs[1:]:
        assert torch.equal(y_all, runs[0][0]) and torch.equal(y, runs[0][1])
        for now, first in zip(tensors, runs[0][2]):
            assert torch.equal(now, first)
    assert append_launches == [(1, 16), (1, 8), (1, 16), (37, 16), (37, 8), (37, 16)]


def test_permuted_rows_and_slots(cuda, append_launches):
    L, N, B, W = 20, 40, 17, 20
    model, _ = _model(cuda, 64, 4, L, 2)
    g = torch.Generator().manual_seed(5)
    slots = torch.randperm(N, generator=g)[:B]
    order = torch.randperm(B, generator=g)
    seq, lens = _sequences(W, [(b * 3) % (W + 1) for b in range(B)])
    base, perm = model.session_open(N, L), model.session_open(N, L)
    before = [t.clone() for t in _state_tensors(base)]
    ya, alla = session.append(model, base, seq, lens, slots.tolist(), return_all=True)
    yb, allb = session.append(model, perm, seq[order], lens[order], slots[order].to(cuda),
                              return_all=True)
    assert torch.equal(ya[order.to(cuda)], yb) and torch.equal(alla[order.to(cuda)], allb)
    _same(base, perm)
    others = torch.tensor(sorted(set(range(N)) - set(slots.tolist())), device=cuda)
    for now, was in zip(_state_tensors(base), before):
        assert torch.equal(now[others], was[others])
    assert int(lens.max()) == 18 and alla.shape[1] == 18      # host lengths: the longest row
    assert append_launches == _launches(B, 18) * 2


def test_masked_rows(cuda, append_launches):
    L, B, W = 20, 9, 12
    model, _ = _model(cuda, 64, 4, L, 2)
    seq, _ = _sequences(W, [W] * B)
    seq = seq.to(cuda)
    good, bad = model.session_open(B, L), model.session_open(B, L)
    for st in (good, bad):
        session.append(model, st, seq[:, :3])
    kept = [t.clone() for t in _state_tensors(bad)]
    tail = seq[:, 3:].clone()
    tail[6, 1] = 0                  # one event; the id past the table after the 0 is ignored
    tail[6, 4] = V + 3
    clean = tail.clone()
    clean[[2, 4, 7]] = 0
    yg, allg = session.append(model, good, clean, return_all=True)
    tail[2, 5] = V                  # a bad id in the middle of the row
    tail[4] = 0                     # no event
    slots = torch.arange(B, device=cuda)
    slots[7] = B                    # a slot outside the state
    yb, allb = session.append(model, bad, tail, slots=slots, return_all=True)
    assert append_launches[-2:] == [(B, 16), (B, 16)]
    status = bad.status.tolist()
    assert [status[r] for r in (2, 4, 6, 7)] == [session.BAD_ITEM, session.NO_EVENT,
                                                 session.STEPPED, session.BAD_SLOT]
    assert all(status[r] == session.STEPPED for r in (0, 1, 3, 5, 8))
    for now, was in zip(_state_tensors(bad), kept):
        assert torch.equal(now[[2, 4, 7]], was[[2, 4, 7]])      # untouched
    assert bad.count.tolist() == [12, 12, 3, 12, 3, 12, 4, 3, 12]
    assert torch.equal(yb[2], bad.out[2]) and torch.equal(yb[4], bad.out[4])
    assert not yb[7].any() and not allb[[2, 4, 7]].any()
    keep = [0, 1, 3, 5, 6, 8]       # the neighbours, as without the masked rows
    assert torch.equal(yb[keep], yg[keep]) and torch.equal(allb[keep], allg[keep])
    _same(bad, good)


def test_past_the_window_continues_as_the_step_does(cuda, append_launches):
    L, B = 12, 5
    model, _ = _model(cuda, 64, 4, L, 2)
    seq, _ = _sequences(L + 20, [L + 20] * B)
    seq = seq.to(cuda)
    by_step, by_append = model.session_open(B), model.session_open(B)
    _step_loop(model, by_step, seq[:, :L], None)
    session.append(model, by_append, seq[:, :L])
    _same(by_append, by_step)
    assert by_append.count.tolist() == [L] * B
    y_ref, all_ref = _step_loop(model, by_step, seq[:, L:], None)
    y, y_all = session.append(model, by_append, seq[:, L:], return_all=True)
    assert torch.equal(y, y_ref) and torch.equal(y_all, all_ref)
    _same(by_append, by_step)
    assert by_append.count.tolist() == [L + 20] * B
    assert append_launches == _launches(B, L) + _launches(B, 20)

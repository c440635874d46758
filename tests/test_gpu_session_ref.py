"""The session encoder kernels (rb_session_step, rb_session_append,
rb_session_capture behind prefill(method="forward")) against an independent
fp64 reference (tests/session_reference.py: a serial loop over each slot's
events from explicit pad steps), state by state: after every event state.out,
every state.h[i] and every state.conv[i] are judged, not only the returned row.

Per tensor the error is max |got - ref64| / scale, the scale being the
channel's max |ref| for h and the row's max |ref| for out and conv, and the bar
M * e32 + 4 * 2^-24, e32 the same error of the reference's own fp32 run on the
same inputs (gate_scan_reference.channel_error / judge).  M is fixed from what
the project already holds, not from these kernels:

    M = 4 in "init", and for layer 0's conv rows in either regime: a GEMM and
    LayerNorms only, the margin test_gpu_gemm_half.py gives an fp32-class GEMM
    with another summation order;
    M = test_gpu_gate_scan_ref.M["y"] = 22 in "wide" for h and what follows it
    (out, the deeper layers' conv rows): the same alpha / beta formula with the
    same 1-ulp hardware exp (that file's docstring says where 22 comes from).

Value regimes (session_reference.make_params): "init", and "wide" with
saturated gates, Lambda across softplus' x > 20 branch, LayerNorm gammas in
[0.5, 1.5], one channel whose r gate is shut (alpha = 1, beta = sqrt(1e-8)
sigmoid(i)) and every 7th embedding row shifted by +300.  In "wide" the slots
that take shifted rows (every third slot, "+300" below) are judged apart from
the others: fp32 is 1e-4 off on such a row, 300 times its error elsewhere, and
one yardstick for both would hide everything under it.

Every case asserts kernel_supports and counts the launches, so no case can
pass on step_reference; a slot without an event in a call must stay bitwise
as it was.

B = 19 slots (one full tile of 16 rows and one of 3), V = 60.  The shapes and
the paths of session_tile.h::gemm16 they reach (K extents 128 / 64 / 16 wide:
mfma_blocks<8> / <4> / <1>; 8 waves, two column tiles each per trip):

    d16e4    d=16  H=64   K=2 layers=1 L=12  K extent 16 = one <1>; the
                                             out-projection's single column tile
    d48e2    d=48  H=96   K=4 layers=2 L=20  K extent 48 = 3 x <1>, 96 = <4> +
                                             2 x <1>; 3 column tiles (waves 0-2,
                                             no second tile: w1 = w0)
    d80e1    d=80  H=80   K=8 layers=1 L=16  80 = <4> + <1>; 5 column tiles;
                                             g_width = 4d > 2H; no pad prefix
    d48e4    d=48  H=192  K=3 layers=1 L=9   24 column tiles: a second trip of
                                             the tile loop; g_width = 2H > 4d
    d128e4   d=128 H=512  K=4 layers=1 L=9   140 KB of the 160 KB of LDS; <8>
    d64e2K1  d=64  H=128  K=1 layers=8 L=12  RB_SESSION_MAX_LAYERS; no conv history
    d64e2    d=64  H=128  K=4 layers=2 L=20  the three flag variants

d48e2 and d80e1 run as long sessions: slot b takes 15 b + 1 events, up to 271,
far past the window.  d48e2 also goes through append (W = 35, ragged) and
through prefill(method="forward") at L = 40 plus three steps.

Worst measured ratio error / max(e32, 4 * 2^-24) on an MI355X, per tensor
kind and regime, with the case that produced it ("+300": the slots that take
shifted embedding rows; h[>0], conv[>0]: the layers after the first):

    tensor        regime   worst ratio   case                 M
    out           init      1.45         long-d80e1            4
    h[0]          init      1.77         long-d48e2            4
    h[>0]         init      1.86         long-d48e2            4
    conv[0]       init      2.27         step-d128e4           4
    conv[>0]      init      1.82         step-d64e2-noffn      4
    out           wide      1.12         long-d48e2           22
    h[0]          wide      1.17         long-d80e1           22
    h[>0]         wide      2.31         step-d64e2-noffn     22
    conv[0]       wide      2.37         long-d80e1            4
    conv[>0]      wide      1.76         step-d64e2-noffn     22
    out+300       wide      1.00         step-d16e4           22
    h[0]+300      wide      1.00         step-d16e4           22
    h[>0]+300     wide      0.96         step-d64e2-noffn     22
    conv[0]+300   wide      1.00         step-d16e4            4
    conv[>0]+300  wide      1.07         step-d64e2-noffn     22

No ratio is above its M.  One was, and the cause was fixed in the code:
prefill(method="forward") in "wide" gave 4.27 on conv[0]+300 (error 2.730e-03,
bar 2.558e-03; 4.20 on conv[1]+300, 5.12 on h[1]+300).  rb_session_capture
only copies the forward's pre-conv rows; the error came from the packed
forward's embedding LayerNorm, which at d = 48 (no row-kernel size) was
torch's own: on the shifted rows it is 3.47e-03 off where two-pass fp32 is
5.3e-04 (the yardstick: 6.4e-04).  blocks._two_pass_layer_norm now does that
LayerNorm with the row kernels' arithmetic, and the case measures 1.00 or
less on every "+300" tensor.
"""
import functools
from types import SimpleNamespace

import pytest
import torch

import session_reference as S
from datamining_recblr_amd import session
from datamining_recblr_amd.model import RecBLR
from datamining_recblr_amd.recbole_compat import SyntheticDataset
from test_gpu_gate_scan_ref import M as GATE_SCAN_M
from test_session_reference_host import steps_on

pytestmark = pytest.mark.gpu

M_INIT, M_WIDE = 4, GATE_SCAN_M["y"]
B, V = 19, 60

SHAPES = {
    "d16e4": dict(d=16, expand=4, K=2, layers=1, L=12),
    "d48e2": dict(d=48, expand=2, K=4, layers=2, L=20),
    "d80e1": dict(d=80, expand=1, K=8, layers=1, L=16),
    "d48e4": dict(d=48, expand=4, K=3, layers=1, L=9),
    "d128e4": dict(d=128, expand=4, K=4, layers=1, L=9),
    "d64e2K1": dict(d=64, expand=2, K=1, layers=8, L=12),
    "d64e2": dict(d=64, expand=2, K=4, layers=2, L=20),
}
FLAGS = {"full": {}, "noconv": {"disable_conv1d": True}, "noffn": {"disable_ffn": True},
         "bdlru": {"bd_lru_only": True}}


def _short_counts(L):
    """0 .. L + 3 events over the 19 slots: no event at all, one, the window, past it."""
    return tuple((5 * b) % (L + 4) for b in range(B))


LONG_COUNTS = tuple(15 * b + 1 for b in range(B))
APPEND_COUNTS = (35, 17, 16, 15, 3, 1, 0)
PREFILL_COUNTS = (40, 33, 32, 17, 16, 15, 3, 2, 1)


@functools.lru_cache(maxsize=None)
def _case(shape, regime, flags, counts, L=None):
    """Parameters, events and the two reference runs of a case, computed once
    per module and shared (nothing changes them afterwards)."""
    sh = dict(SHAPES[shape])
    L = L or sh["L"]
    dims = (sh["d"], sh["expand"], sh["K"], sh["layers"])
    seed = 100 * sh["d"] + 10 * sh["expand"] + sh["K"]
    params = S.make_params(regime, *dims, V, seed)
    cfg = S.config(*dims, L, **FLAGS[flags])
    events = S.make_events(counts, V, seed + 1)
    return SimpleNamespace(
        shape=sh, L=L, regime=regime, params=params, cfg=cfg, events=events, counts=list(counts),
        r64=S.reference(params, cfg, L, events),
        r32=S.reference(params, cfg, L, events, dtype=torch.float32))


def _model(c, dev):
    sh = c.shape
    assert session.kernel_supports(sh["d"], sh["d"] * sh["expand"], sh["K"], sh["layers"])
    model = RecBLR(c.cfg, SyntheticDataset(V)).eval()
    model.load_state_dict(c.params)
    return model.to(dev)


@pytest.fixture
def launches(monkeypatch):
    """Counts the launches of the three kernels: a silent fallback cannot pass."""
    calls = {"step": [], "append": [], "capture": 0}
    step, app, cap = session._step_kernel, session._append_kernel, session._capture_kernel

    def counted_step(p, state, layers, items, *args):
        calls["step"].append(items.numel())
        return step(p, state, layers, items, *args)

    def counted_append(p, state, layers, items, *args):
        calls["append"].append(tuple(items.shape))
        return app(p, state, layers, items, *args)

    def counted_capture(*args):
        calls["capture"] += 1
        return cap(*args)

    monkeypatch.setattr(session, "_step_kernel", counted_step)
    monkeypatch.setattr(session, "_append_kernel", counted_append)
    monkeypatch.setattr(session, "_capture_kernel", counted_capture)
    return calls


def _judge(got, c, what, lo=None, hi=None):
    """Judge `got` against the case's reference runs, print every figure,
    assert the bars.  With lo / hi `got` holds events lo[b] .. hi[b] - 1 of
    every slot only (a state read once, after a call): they are judged on the
    scales and against the yardstick of the whole case, which the other
    events enter with no error."""
    if lo is not None:
        got = _among_all(got, c.r64, lo, hi)
    res = S.judge_run(got, c.r64, c.r32, c.regime, M_INIT, M_WIDE)
    for n, (ok, err, limit, ratio) in res.items():
        print(f"RATIO {what} {c.regime} {n:12s} err {err:.3e}  bar {limit:.3e}  ratio {ratio:.2f}")
    bad = {n: v for n, v in res.items() if not v[0]}
    assert not bad, (what, bad)


def _among_all(got, r64, lo, hi):
    """The reference run with events lo[b] .. hi[b] - 1 of every slot replaced by got's."""
    def put(per_slot, part):
        out = []
        for t, g, a, b in zip(per_slot, part, lo, hi):
            t = t.clone()
            assert g.shape == t[a:b].shape, (g.shape, t[a:b].shape)
            t[a:b] = g.double()
            out.append(t)
        return out

    return SimpleNamespace(out=put(r64.out, got.out),
                           h=[put(h, g) for h, g in zip(r64.h, got.h)],
                           conv=[put(cv, g) if cv is not None else None
                                 for cv, g in zip(r64.conv, got.conv)])


def _final_state(state, n):
    """The state's tensors as one-event runs (no event for a slot with n = 0)."""
    def rows(t):
        return [t[b:b + 1].cpu() if n[b] else t[:0].cpu() for b in range(len(n))]

    return SimpleNamespace(out=rows(state.out), h=[rows(h) for h in state.h],
                           conv=[rows(cv) if cv is not None else None for cv in state.conv])


def _stepped(c, dev, launches):
    model = _model(c, dev)
    state = model.session_open(B, c.L)
    got = steps_on(model, state, c.events, session.step, dev)
    assert got.idle_ok, "a slot without an event changed"
    assert state.count.tolist() == c.counts
    assert launches["step"] == [B] * max(c.counts)
    assert launches["append"] == [] and launches["capture"] == 0
    return got


STEP_CASES = ([(s, "init", "full") for s in ("d16e4", "d48e4", "d128e4", "d64e2K1")]
              + [("d64e2", "init", f) for f in ("noconv", "noffn", "bdlru")]
              + [("d16e4", "wide", "full"), ("d64e2", "wide", "noffn")])


@pytest.mark.parametrize("shape,regime,flags", STEP_CASES, ids=lambda v: v)
def test_step_vs_fp64_reference(cuda, launches, shape, regime, flags):
    c = _case(shape, regime, flags, _short_counts(SHAPES[shape]["L"]))
    got = _stepped(c, cuda, launches)
    _judge(got, c, f"step-{shape}-{flags}")


@pytest.mark.parametrize("regime", ["init", "wide"])
@pytest.mark.parametrize("shape", ["d48e2", "d80e1"])
def test_long_sessions_vs_fp64_reference(cuda, launches, shape, regime):
    """Slot b takes 15 b + 1 events, every one of them judged: up to 271
    events in a window of 20 (16): the recurrence simply continues."""
    c = _case(shape, regime, "full", LONG_COUNTS)
    got = _stepped(c, cuda, launches)
    assert len(launches["step"]) == 271
    _judge(got, c, f"long-{shape}")


@pytest.mark.parametrize("regime", ["init", "wide"])
def test_append_vs_fp64_reference(cuda, launches, regime):
    """rb_session_append over W = 35 ragged columns (launches of T = 16, 16 and
    4): y_all at every event and the state left behind."""
    c = _case("d48e2", regime, "full", APPEND_COUNTS)
    model = _model(c, cuda)
    n, W = c.counts, max(c.counts)
    seq = torch.zeros(len(n), W, dtype=torch.int64)
    for b, ev in enumerate(c.events):
        seq[b, :len(ev)] = torch.tensor(ev, dtype=torch.int64)
    state = model.session_open(len(n), c.L)
    idle = [t[-1].clone() for t in (state.out, *state.h, *state.conv)]
    y, y_all = session.append(model, state, seq.to(cuda), torch.tensor(n), return_all=True)
    assert launches["append"] == [(7, 16), (7, 16), (7, 4)] and launches["step"] == []
    assert state.count.tolist() == n and y_all.shape == (len(n), W, 48)
    assert torch.equal(y, state.out)
    for now, was in zip((state.out, *state.h, *state.conv), idle):   # the slot of length 0
        assert torch.equal(now[-1], was)
    y_all = y_all.cpu()
    for b in range(len(n)):
        assert not y_all[b, n[b]:].any()
    every = SimpleNamespace(out=[y_all[b, :n[b]] for b in range(len(n))])
    res = S.judge_run(every, c.r64, c.r32, regime, M_INIT, M_WIDE, names=["out"])
    for name, (ok, err, limit, ratio) in res.items():
        print(f"RATIO append-y_all {regime} {name:12s} err {err:.3e}  bar {limit:.3e}  "
              f"ratio {ratio:.2f}")
    assert all(v[0] for v in res.values()), res
    _judge(_final_state(state, n), c, "append-final", [max(k - 1, 0) for k in n], n)


@pytest.mark.parametrize("regime", ["init", "wide"])
def test_forward_prefill_vs_fp64_reference(cuda, launches, regime):
    """prefill(method="forward") at L = 40 (pad prefix 24): lengths on both
    sides of the capture kernel's 16-step tile boundary and histories shorter
    than K - 1 rows; then three step events on the captured state."""
    L, n0 = 40, list(PREFILL_COUNTS)
    c = _case("d48e2", regime, "full", tuple(k + 3 for k in n0), L=L)
    model = _model(c, cuda)
    seq = torch.zeros(len(n0), L, dtype=torch.int64)
    for b, ev in enumerate(c.events):
        seq[b, :n0[b]] = torch.tensor(ev[:n0[b]], dtype=torch.int64)
    state = model.session_open(len(n0), L)
    y = session.prefill(model, state, seq.to(cuda), torch.tensor(n0), method="forward")
    assert launches["capture"] == 2 and launches["step"] == [] and launches["append"] == []
    assert state.count.tolist() == n0 and torch.equal(y, state.out)
    _judge(_final_state(state, n0), c, "prefill-forward", [k - 1 for k in n0], n0)
    for extra in range(3):
        items = torch.tensor([ev[k + extra] for ev, k in zip(c.events, n0)])
        session.step(model, state, items.to(cuda))
        now = [k + extra + 1 for k in n0]
        assert state.count.tolist() == now
        _judge(_final_state(state, now), c, f"prefill-step{extra + 1}", [k - 1 for k in now], now)
    assert launches["capture"] == 2 and launches["step"] == [len(n0)] * 3

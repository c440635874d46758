"""The session reference (tests/session_reference.py) and its bars, checked on
the CPU before the GPU tests (test_gpu_session_ref.py) rely on them.

1. In float64 the reference's out equals the oracle's model_forward (pinned to
   the reference implementation by test_oracle_golden.py) at every prefix
   t <= L, to 1e-11 of max |ref|: with and without a pad prefix, for every flag
   variant and for expand 1, 2 and 4.
2. session.step_reference on a CPU SessionState passes the bars the GPU tests
   apply (M = 4 in "init" and for layer 0's conv rows, test_gpu_gate_scan_ref's
   M["y"] in "wide" for h and what follows it): out, h and conv, both regimes,
   past the window.  So plain fp32 arithmetic in another order, with the
   closed-form pad prefix, stays inside them.
3. The bars can fail: six subtly wrong fp32 runs (session_reference.WRONG) are
   each rejected on at least one tensor in at least one regime.
"""
from types import SimpleNamespace

import pytest
import torch

import session_reference as S
from datamining_recblr_amd import session
from oracle import recblr_oracle as orc
from test_gpu_gate_scan_ref import M as GATE_SCAN_M

M_INIT, M_WIDE = 4, GATE_SCAN_M["y"]
V = 60


# ---- 1. the reference against the oracle -------------------------------------

def _oracle_check(regime, L, expand, flags, K=4):
    d, layers = 16, 2
    params = S.make_params(regime, d, expand, K, layers, V, seed=11)
    cfg = S.config(d, expand, K, layers, L, **flags)
    lens = [L, 5, 1]
    events = S.make_events(lens, V, seed=12)
    ref = S.reference(params, cfg, L, events)
    seq = torch.zeros(len(lens), L, dtype=torch.int64)
    for b, ev in enumerate(events):
        seq[b, :len(ev)] = torch.tensor(ev)
    p64 = {k: v.double() for k, v in params.items()}
    worst = 0.0
    for t in range(L):
        done = torch.clamp(torch.tensor(lens), max=t + 1)
        want = orc.model_forward(p64, cfg, seq, done)
        got = torch.stack([ref.out[b][int(done[b]) - 1] for b in range(len(lens))])
        worst = max(worst, float((got - want).abs().max() / want.abs().max()))
    assert worst <= 1e-11, worst


@pytest.mark.parametrize("flags", [{}, {"disable_conv1d": True}, {"disable_ffn": True},
                                   {"bd_lru_only": True}], ids=lambda f: "-".join(f) or "full")
@pytest.mark.parametrize("L", [12, 16])   # pad prefix P = 4 and P = 0
def test_reference_equals_the_oracle_at_every_prefix(L, flags):
    assert S.pow2_pad_len(L) == orc.pow2_pad_len(L) == (4 if L == 12 else 0)
    _oracle_check("init", L, 2, flags)


@pytest.mark.parametrize("regime", ["init", "wide"])
@pytest.mark.parametrize("expand", [1, 2, 4])
@pytest.mark.parametrize("L", [12, 16])
def test_reference_equals_the_oracle_for_every_expand(L, expand, regime):
    _oracle_check(regime, L, expand, {})


def test_reference_equals_the_oracle_for_other_kernel_sizes():
    for K in (1, 2, 8):
        _oracle_check("init", 12, 2, {}, K=K)


# ---- 2. and 3.: the bars --------------------------------------------------------

D, EXPAND, K, LAYERS, L = 16, 4, 4, 2, 12
COUNTS = [40, 17, 13, 12, 5, 1, 0]          # past the window, at it, and no event at all


def _runs(regime):
    params = S.make_params(regime, D, EXPAND, K, LAYERS, V, seed=21)
    cfg = S.config(D, EXPAND, K, LAYERS, L)
    events = S.make_events(COUNTS, V, seed=22)
    r64 = S.reference(params, cfg, L, events)
    r32 = S.reference(params, cfg, L, events, dtype=torch.float32)
    return SimpleNamespace(regime=regime, params=params, cfg=cfg, events=events, r64=r64, r32=r32)


@pytest.fixture(scope="module")
def both():
    return {r: _runs(r) for r in ("init", "wide")}


@pytest.fixture(params=["init", "wide"])
def runs(request, both):
    return both[request.param]


def test_regimes_are_what_they_claim(runs):
    lo, hi = (6.0, 16.0) if runs.regime == "wide" else (0.0, 2.0)
    assert lo < runs.r64.gate_max < hi, runs.r64.gate_max
    if runs.regime == "wide":
        # the shut r gate: alpha is exactly 1, the channel only ever adds sqrt(1e-8) sigmoid(i) xc
        h = runs.r64.h[0][0][:, S.STUCK_CHANNEL]
        assert 0 < float(h.abs().max()) < 1e-2


def steps_on(source, state, events, step, dev="cpu"):
    """Feed the events one call per column (item 0 for a finished slot) and
    collect the state after every call: per slot lists like reference()'s,
    and whether a slot without an event stayed bitwise unchanged."""
    B, T = len(events), max(len(e) for e in events)
    seq = torch.zeros(B, max(T, 1), dtype=torch.int64)
    for b, ev in enumerate(events):
        seq[b, :len(ev)] = torch.tensor(ev, dtype=torch.int64)
    layers = len(state.h)

    def snap():
        return ([state.out.clone()], [h.clone() for h in state.h],
                [c.clone() if c is not None else None for c in state.conv])

    snaps = [snap()]
    for t in range(T):
        step(source, state, seq[:, t].to(dev))
        snaps.append(snap())

    def series(pick):            # [T + 1, B, ...] on the CPU
        return torch.stack([pick(s) for s in snaps]).cpu()

    out = series(lambda s: s[0][0])
    hs = [series(lambda s, i=i: s[1][i]) for i in range(layers)]
    cs = [series(lambda s, i=i: s[2][i]) if state.conv[i] is not None else None
          for i in range(layers)]
    idle_ok = True
    for b, ev in enumerate(events):
        for t in (out, *hs, *[c for c in cs if c is not None]):
            idle_ok &= bool((t[len(ev):, b] == t[len(ev), b]).all())
    n = [len(e) for e in events]
    return SimpleNamespace(
        out=[out[1:n[b] + 1, b] for b in range(B)],
        h=[[h[1:n[b] + 1, b] for b in range(B)] for h in hs],
        conv=[[c[1:n[b] + 1, b] for b in range(B)] if c is not None else None for c in cs],
        idle_ok=idle_ok)


def test_step_reference_passes_the_bars(runs):
    source = session.EncoderParams.from_state_dict(runs.params, runs.cfg)
    state = session.SessionState(source, len(COUNTS), L)
    got = steps_on(source, state, runs.events, session.step_reference)
    assert got.idle_ok and state.count.tolist() == COUNTS
    res = S.judge_run(got, runs.r64, runs.r32, runs.regime, M_INIT, M_WIDE)
    for n, (ok, err, limit, ratio) in res.items():
        print(f"{runs.regime} {n:8s} err {err:.3e}  bar {limit:.3e}  ratio {ratio:.2f}")
    assert all(v[0] for v in res.values()), res


def test_the_bars_reject_each_wrong_variant(both):
    """Each wrong fp32 run fails judge on at least one tensor in at least one regime."""
    rejected = {w: [] for w in S.WRONG}
    for regime, runs in both.items():
        for w in S.WRONG:
            got = S.reference(runs.params, runs.cfg, L, runs.events, dtype=torch.float32, wrong=w)
            res = S.judge_run(got, runs.r64, runs.r32, regime, M_INIT, M_WIDE)
            rejected[w] += [(regime, n) for n, v in res.items() if not v[0]]
            print(regime, w, {n: f"{v[3]:.1f}" for n, v in res.items()})
    missed = [w for w, hits in rejected.items() if not hits]
    assert not missed, missed

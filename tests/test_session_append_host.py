"""Several events per slot in one launch, on a GPU-less host: rb_session_append's
boundary (declared, exported, argument errors before any GPU call) and
session.append_reference, the restatement of its contract, against a
step_reference loop (torch.equal) and the CPU oracle (test_gpu_e2e.close)."""
import ctypes
import inspect
import re

import pytest
import torch

from datamining_recblr_amd import _lib, session
from datamining_recblr_amd.model import RecBLR
from oracle import recblr_oracle as orc
from test_gpu_e2e import close
from test_session_host import HEADER, V, _header_names, _layers, _model, _sequences, _state_tensors

NAMES = ["layers", "n_layers", "emb", "ln_w", "ln_b", "eps", "items", "slots", "count", "out", "y",
         "y_all", "status", "B", "T", "N", "V", "d", "H", "K", "disable_conv1d", "disable_ffn",
         "stream"]


def test_the_header_declares_and_the_library_exports_append():
    names = _header_names()
    assert "rb_session_append" in names
    assert all(n.startswith("rb_session_") for n in names)
    lib = _lib.load_session()
    assert hasattr(lib, "rb_session_append")
    res, args = _lib.SESSION_SIGNATURES["rb_session_append"]
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    proto = re.search(r"int rb_session_append\(([^)]*)\)", text).group(1)
    params = [" ".join(p.split()) for p in proto.split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == NAMES
    by_value = {"float": ctypes.c_float, "int": ctypes.c_int, "int64_t": ctypes.c_int64}
    want = [ctypes.c_void_p if "*" in p else by_value[p.split()[0]] for p in params]
    assert res is ctypes.c_int and args == want
    assert lib.rb_session_append.argtypes == want
    assert {"append", "append_reference"} <= set(session.__all__)
    assert lib.rb_session_version() == _lib.ABI_VERSION


# a call that passes every check (fake non-null, 16-byte aligned pointers that
# are never dereferenced: each case below fails a check before any HIP call)
_P = 256


def _args(arr, **bad):
    a = dict(layers=ctypes.addressof(arr), n_layers=len(arr), emb=_P, ln_w=_P, ln_b=_P,
             eps=1e-12, items=_P, slots=None, count=_P, out=_P, y=_P, y_all=_P, status=_P, B=3,
             T=4, N=8, V=50, d=64, H=128, K=4, disable_conv1d=0, disable_ffn=0, stream=None)
    assert list(a) == NAMES and set(bad) <= set(a)
    a.update(bad)
    return list(a.values())


_NULL = "rb_session_append: null pointer"
_T = "rb_session_append: T must be 1, 2, 4, 8 or 16"
APPEND_ERRORS = [
    *[({name: None}, _NULL) for name in ("layers", "emb", "ln_w", "ln_b", "items", "count", "out")],
    *[(dict(T=t), _T) for t in (0, 3, 32)],
    (dict(K=0), "rb_session_append: conv kernel size K must be in [1, 8]"),
    (dict(K=9), "rb_session_append: conv kernel size K must be in [1, 8]"),
    (dict(d=24), "rb_session_append: d and H must be positive multiples of 16"),
    (dict(H=100), "rb_session_append: d and H must be positive multiples of 16"),
    (dict(n_layers=0), "rb_session_append: n_layers must be in [1, 8]"),
    (dict(n_layers=9), "rb_session_append: n_layers must be in [1, 8]"),
    (dict(B=0), "rb_session_append: B, N and V must be positive"),
    (dict(d=1024, H=2048),
     "rb_session_append: shape needs more LDS than a compute unit has (160 KiB)"),
    (dict(emb=8), "rb_session_append: emb, out and y must be 16-byte aligned"),
    (dict(y_all=_P + 8), "rb_session_append: y_all must be 16-byte aligned"),
]


@pytest.mark.parametrize("bad,message", APPEND_ERRORS,
                         ids=["-".join(f"{k}={v}" for k, v in b.items())
                              for b, _ in APPEND_ERRORS])
def test_append_argument_errors_are_reported_before_any_gpu_call(bad, message):
    lib = _lib.load_session()
    layers = _layers()
    assert lib.rb_session_append(*_args(layers, **bad)) == _lib.RB_EINVAL
    assert lib.rb_session_last_error_string().decode() == message
    with pytest.raises(_lib.RecBLRNativeError, match="invalid argument"):
        _lib.call_session("rb_session_append", *_args(layers, **bad))


@pytest.mark.parametrize("field,value,message", [
    ("w_gate", None, "rb_session_append: null pointer in a layer"),
    ("h", None, "rb_session_append: null pointer in a layer"),
    ("conv_state", None, "rb_session_append: null conv pointer in a layer"),
    ("w2", None, "rb_session_append: null ffn pointer in a layer"),
    ("w_in", 8, "rb_session_append: weight matrices must be 16-byte aligned"),
])
def test_append_checks_every_layer(field, value, message):
    lib = _lib.load_session()
    layers = _layers(2)
    setattr(layers[1], field, value)
    assert lib.rb_session_append(*_args(layers)) == _lib.RB_EINVAL
    assert lib.rb_session_last_error_string().decode() == message


# ---- append_reference against a step_reference loop and the oracle -------------
L, K, W = 80, 4, 35
LENS = [0, 1, 2, K - 1, 16, 17, 35]


@pytest.fixture(scope="module")
def model_cfg():
    return _model(L)


def _step_loop(model, state, cols, slots):
    """One step_reference per column: (out rows after the last column, the
    rows' output after each event with zeros where a row had none)."""
    y, per_event = None, []
    for t in range(cols.shape[1]):
        y = session.step_reference(model, state, cols[:, t], slots)
        per_event.append(torch.where((state.status == session.STEPPED)[:, None], y,
                                     torch.zeros_like(y)))
    return y, torch.stack(per_event, 1)


def _same_state(a, b):
    for x, y in zip(_state_tensors(a), _state_tensors(b)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("slots", [None, [6, 1, 8, 3, 0, 9, 4]], ids=["identity", "permuted"])
def test_append_reference_equals_a_step_loop_on_fresh_slots(model_cfg, slots):
    model, cfg = model_cfg
    seq, lens = _sequences(W, LENS)
    by_step, by_append = (session.SessionState(model, 10, L) for _ in range(2))
    y_ref, all_ref = _step_loop(model, by_step, seq, slots)
    y, y_all = session.append_reference(model, by_append, seq, lens, slots, return_all=True)
    assert y_all.shape == (len(LENS), W, 16)
    assert torch.equal(y, y_ref) and torch.equal(y_all, all_ref)
    _same_state(by_append, by_step)
    idx = slots if slots is not None else list(range(len(LENS)))
    assert by_append.count[idx].tolist() == LENS
    assert by_append.status.tolist() == [session.NO_EVENT] + [session.STEPPED] * 6
    for b, n in enumerate(LENS):       # y_all: the row's output after event t, zeros past n
        assert not y_all[b, n:].any() and (n == 0 or torch.equal(y_all[b, n - 1], y[b]))
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    wide = torch.nn.functional.pad(seq, (0, L - W))
    ref = orc.model_forward(params, cfg, wide[1:], lens[1:])
    close(y[1:], ref, what="append_reference vs the oracle")
    # without lengths the zeros of the padding say the same
    again = session.SessionState(model, 10, L)
    assert torch.equal(session.append_reference(model, again, seq, slots=slots), y)
    _same_state(again, by_step)


def test_append_reference_equals_a_step_loop_on_live_slots(model_cfg):
    """Slots that hold 0, 1, K - 2, K - 1 and many events take 0 .. 35 more:
    among them a slot with fewer than K - 1 events that receives fewer than
    K - 1 (1 + 1, 2 + 2 with K = 4)."""
    model, cfg = model_cfg
    first = [3, 1, K - 2, K - 1, 20, 0, 7]
    more = [0, 1, 2, 1, 17, 35, 16]
    seq1, lens1 = _sequences(20, first, seed=3)
    seq2, lens2 = _sequences(W, more, seed=4)
    slots = [2, 5, 0, 7, 1, 9, 4]
    by_step, by_append = (session.SessionState(model, 10, L) for _ in range(2))
    _step_loop(model, by_step, seq1, slots)
    y_ref, all_ref = _step_loop(model, by_step, seq2, slots)
    session.append_reference(model, by_append, seq1, lens1, slots)
    y, y_all = session.append_reference(model, by_append, seq2, lens2, slots, return_all=True)
    assert torch.equal(y, y_ref) and torch.equal(y_all, all_ref)
    _same_state(by_append, by_step)
    total = [a + b for a, b in zip(first, more)]
    assert by_append.count[slots].tolist() == total
    assert by_append.status.tolist() == [session.NO_EVENT] + [session.STEPPED] * 6
    both = torch.zeros(len(first), L, dtype=torch.int64)
    for b, (n1, n2) in enumerate(zip(first, more)):
        both[b, :n1] = seq1[b, :n1]
        both[b, n1:n1 + n2] = seq2[b, :n2]
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    close(y, orc.model_forward(params, cfg, both, torch.tensor(total)), what="live slots")
    # reset=True starts the same rows from the empty history instead
    opened = session.SessionState(model, 10, L)
    fresh = session.append_reference(model, opened, seq2, lens2, slots)
    assert torch.equal(session.append_reference(model, by_append, seq2, lens2, slots, reset=True),
                       fresh)
    _same_state(by_append, opened)


def test_a_bad_item_masks_its_row_for_the_chunk(model_cfg):
    model, _ = model_cfg
    seq, lens = _sequences(12, [12, 9, 5, 0])
    ok, bad = (session.SessionState(model, 4, L) for _ in range(2))
    for st in (ok, bad):
        session.append_reference(model, st, seq[:, :3])
    before = [t.clone() for t in _state_tensors(bad)]
    tail = seq[:, 3:].clone()
    tail[2, 1] = 0                  # row 2: one event, then an id past the table that is ignored
    tail[2, 3] = V + 7
    skipped = tail.clone()
    skipped[1] = 0
    y_ok, all_ok = session.append_reference(model, ok, skipped, return_all=True)
    tail[1, 4] = V                  # row 1: a bad id in the middle of its 6 events
    y, y_all = session.append_reference(model, bad, tail, return_all=True)
    assert bad.status.tolist() == [session.STEPPED, session.BAD_ITEM, session.STEPPED,
                                   session.NO_EVENT]
    for now, was in zip(_state_tensors(bad), before):
        assert torch.equal(now[1], was[1])
    assert bad.count.tolist() == [12, 3, 4, 0]
    _same_state(bad, ok)            # the other rows as if row 1 had sent nothing
    assert torch.equal(y, y_ok) and torch.equal(y_all, all_ok)
    assert torch.equal(y[1], bad.out[1]) and not y_all[1].any()


def test_atomicity_is_per_chunk_of_16_columns(model_cfg):
    model, _ = model_cfg
    seq, _ = _sequences(40, [40, 40])
    seq[1, 21] = -3                 # in the second chunk
    state, want = (session.SessionState(model, 2, L) for _ in range(2))
    session.append_reference(model, state, seq)
    kept = seq.clone()
    kept[1, 16:32] = 0
    _step_loop(model, want, kept, None)
    _same_state(state, want)
    assert state.count.tolist() == [40, 24]
    assert state.status.tolist() == [session.STEPPED, session.STEPPED]   # the first chunk's
    # a row whose first chunk is the bad one reports it
    session.append_reference(model, state, seq[:, 16:])
    assert state.status.tolist() == [session.STEPPED, session.BAD_ITEM]


def test_the_public_surface_of_append(model_cfg):
    model, _ = model_cfg
    assert callable(RecBLR.session_append)
    want = inspect.signature(session.append).parameters
    got = inspect.signature(RecBLR.session_append).parameters
    assert list(got)[1:] == list(want)[1:] == ["state", "item_seq", "item_seq_len", "slots",
                                               "reset", "return_all"]
    for name in list(want)[3:]:
        assert got[name].default == want[name].default
    assert want["reset"].default is False and want["return_all"].default is False
    # a CPU state takes the reference path
    seq, lens = _sequences(20, [20, 3, 0])
    a, b = (session.SessionState(model, 3, L) for _ in range(2))
    ya, alla = model.session_append(a, seq, lens, return_all=True)
    yb, allb = session.append_reference(model, b, seq, lens, return_all=True)
    assert torch.equal(ya, yb) and torch.equal(alla, allb)
    _same_state(a, b)
    # one event per row as a 1-D input
    assert torch.equal(session.append(model, a, [4, 0, 9]),
                       session.step_reference(model, b, [4, 0, 9]))
    _same_state(a, b)
    model.train()
    try:
        with pytest.raises(ValueError, match="training mode"):
            session.append(model, a, seq, lens)
    finally:
        model.eval()

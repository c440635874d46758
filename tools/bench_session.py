#!/usr/bin/env python
"""Per-event serving cost: RecBLR.session_step (one launch, O(1) in the
history) against the only way to get the same rows without a carried state,
RecBLR.forward over the full [B, L] history.

Model: d = 128, 2 layers, expand 2 (H = 256), K = 4, L = 200, 10,544 items
(BASELINE's C2 shape); B = 1, 64 and 2048 sessions with full-length
histories.  Both paths run in eval mode under no_grad.  Each is warmed up,
then timed in windows of back-to-back calls between two device events
(ending in a synchronise); the two paths alternate window by window and the
figure is the median window's time per call.  Before timing, the sessions
are prefilled with the L items and their rows compared with forward's.

A second leg times opening the B sessions from their histories:
session_prefill(method="steps"), L step launches, against
session_prefill(method="forward"), one packed forward plus one capture launch
per layer, and session_append(reset=True), ceil(L / 16) append launches; same
windows, alternating, with the largest deviation of the forward-built state's
h, conv history and out from the step-built one and whether the append-built
one equals it bitwise (prefill_rows).

A third leg times 16 new events per live session: one session_append call
(one launch) against 16 session_step calls, the only way without it
(append_rows).

--recommend adds a fourth leg, click in, recommendation list out (k = 10,
S = L = 200 remembered items, recommend_rows): (a) session_recommend on a
state opened with history=S, the seen-item lists coming from its record
launch; (b) the same result without the ring: session_step, a caller-kept
[N, 200] device matrix of the slots' items updated with torch indexing,
index_select of the rows' lists and top_items(exclude=...); (c) session_step
and top_items without exclusion, so (a) - (c) is what the bookkeeping costs.

--park runs only a fifth leg (park_rows): taking B of 4,096 live sessions
(S = 200 remembered items, 2,580 words each) out of the state and putting B
others in: session.park, session.resume and session.exchange, one
rb_session_transfer launch each, against the torch composition of the same
result (out: one index_select per state tensor and the cat into the blob; in:
the split and one index_copy_ per tensor); for B = 2,048 also the bytes moved
per second, every word counted once read and once written.

Prints one JSON line; --out also writes it to a file."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from datamining_recblr_amd.model import RecBLR, attach_host_lengths  # noqa: E402
from datamining_recblr_amd.recbole_compat import SyntheticDataset  # noqa: E402

N_ITEMS, L = 10544, 200


def window_ms(fn, calls: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def prefill_leg(model, B: int, seq, lens, windows: int) -> dict:
    """Opening B sessions from their L-item histories: session_prefill by a
    step per column (method="steps", the default) against one packed forward
    plus a capture launch per layer (method="forward"), alternating window by
    window; and how far the two states are apart."""
    by_steps, by_fwd, by_app = (model.session_open(B) for _ in range(3))
    steps = lambda: model.session_prefill(by_steps, seq, lens)                    # noqa: E731
    fwd = lambda: model.session_prefill(by_fwd, seq, lens, method="forward")      # noqa: E731
    app = lambda: model.session_append(by_app, seq, lens, reset=True)             # noqa: E731
    steps_calls = 2                       # 2 x 200 step launches, as the step leg's window
    fwd_calls = 20 if B <= 64 else 5      # as the forward leg's window
    app_calls = 20 if B <= 64 else 5      # 13 append launches a call
    for _ in range(2):
        window_ms(steps, steps_calls)
        window_ms(fwd, fwd_calls)
        window_ms(app, app_calls)
    ts, tf, ta = [], [], []
    for _ in range(windows):
        ts.append(window_ms(steps, steps_calls))
        tf.append(window_ms(fwd, fwd_calls))
        ta.append(window_ms(app, app_calls))
    s, f, a = statistics.median(ts), statistics.median(tf), statistics.median(ta)
    dev = lambda a, b: max((x - y).abs().max().item() for x, y in zip(a, b))     # noqa: E731
    return dict(B=B, steps_ms=round(s, 4), steps_ms_min=round(min(ts), 4),
                steps_ms_max=round(max(ts), 4), forward_ms=round(f, 4),
                forward_ms_min=round(min(tf), 4), forward_ms_max=round(max(tf), 4),
                append_ms=round(a, 4), append_ms_min=round(min(ta), 4),
                append_ms_max=round(max(ta), 4),
                steps_over_forward=round(s / f, 1), steps_over_append=round(s / a, 2),
                append_over_forward=round(a / f, 2),
                append_equals_steps=bool(same_state(by_app, by_steps)),
                h_max_abs_dev=dev(by_fwd.h, by_steps.h),
                conv_max_abs_dev=dev(by_fwd.conv, by_steps.conv),
                out_max_abs_dev=dev([by_fwd.out], [by_steps.out]),
                h_max_abs=max(h.abs().max().item() for h in by_steps.h),
                count_equal=bool(torch.equal(by_fwd.count, by_steps.count)))


def same_state(a, b) -> bool:
    return all(torch.equal(x, y) for x, y in zip([*a.h, *a.conv, a.count, a.out],
                                                 [*b.h, *b.conv, b.count, b.out]))


def append_leg(model, B: int, seq, lens, g, windows: int) -> dict:
    """16 new events for each of B live sessions (opened from their L-item
    histories): one session_append call against 16 session_step calls,
    alternating window by window."""
    by_step, by_app = model.session_open(B), model.session_open(B)
    for st in (by_step, by_app):
        model.session_append(st, seq, lens, reset=True)
    events = torch.randint(1, N_ITEMS, (B, 16), generator=g).to(seq.device)
    cols = events.t().contiguous()

    def step16():
        for t in range(16):
            model.session_step(by_step, cols[t])

    app16 = lambda: model.session_append(by_app, events)                          # noqa: E731
    step16()
    app16()
    equal = same_state(by_app, by_step)
    step_calls = 12 if B <= 64 else 4     # 16 step launches a call
    app_calls = 100 if B <= 64 else 10
    for _ in range(2):
        window_ms(step16, step_calls)
        window_ms(app16, app_calls)
    ts, ta = [], []
    for _ in range(windows):
        ts.append(window_ms(step16, step_calls))
        ta.append(window_ms(app16, app_calls))
    s, a = statistics.median(ts), statistics.median(ta)
    return dict(B=B, events=16, steps16_ms=round(s, 4), steps16_ms_min=round(min(ts), 4),
                steps16_ms_max=round(max(ts), 4), append_ms=round(a, 4),
                append_ms_min=round(min(ta), 4), append_ms_max=round(max(ta), 4),
                steps16_over_append=round(s / a, 2), append_equals_steps=bool(equal))


def recommend_leg(model, B: int, seq, lens, g, windows: int, k: int = 10) -> dict:
    """One click per live session and its recommendation list, three ways,
    alternating window by window (see the module doc)."""
    from datamining_recblr_amd.scoring import top_items

    dev, S = seq.device, L
    emb = model.item_embedding.weight
    with_ring, kept, bare = model.session_open(B, history=S), model.session_open(B), \
        model.session_open(B)
    for st in (with_ring, kept, bare):
        model.session_append(st, seq, lens, reset=True)
    nxt = torch.randint(1, N_ITEMS, (B,), generator=g).to(dev)
    # (b)'s bookkeeping, as a caller without the ring must keep it: the slots'
    # last S items and a write position per slot
    mine, pos = seq.clone(), torch.zeros(B, dtype=torch.int64, device=dev)
    rows = torch.arange(B, device=dev)

    def a():
        return model.session_recommend(with_ring, nxt, k=k)

    def b():
        y = model.session_step(kept, nxt)
        mine[rows, pos] = nxt
        pos.add_(1).remainder_(S)
        return top_items(y, emb, k, exclude=mine.index_select(0, rows))

    def c():
        return top_items(model.session_step(bare, nxt), emb, k)

    ra, rb = a(), b()
    equal = bool(torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1]))
    calls = 100 if B <= 64 else 20
    for _ in range(2):
        for fn in (a, b, c):
            window_ms(fn, calls)
    ta, tb, tc = [], [], []
    for _ in range(windows):
        ta.append(window_ms(a, calls))
        tb.append(window_ms(b, calls))
        tc.append(window_ms(c, calls))
    med = statistics.median
    return dict(B=B, k=k, S=S, recommend_ms=round(med(ta), 4), recommend_ms_min=round(min(ta), 4),
                recommend_ms_max=round(max(ta), 4), caller_kept_ms=round(med(tb), 4),
                caller_kept_ms_min=round(min(tb), 4), caller_kept_ms_max=round(max(tb), 4),
                no_exclusion_ms=round(med(tc), 4), no_exclusion_ms_min=round(min(tc), 4),
                no_exclusion_ms_max=round(max(tc), 4),
                caller_kept_over_recommend=round(med(tb) / med(ta), 2),
                first_call_equal=equal)


def torch_park(state, slots, head, out):
    """park as torch ops: one index_select per state tensor and the cat into
    the blob (the row format of session/recblr_session.h)."""
    B, i32 = slots.numel(), torch.int32
    parts = [head, state.count.index_select(0, slots)[:, None].view(i32),
             state.out.index_select(0, slots).view(i32)]
    for h, conv in zip(state.h, state.conv):
        parts.append(h.index_select(0, slots).view(i32))
        parts.append(conv.index_select(0, slots).reshape(B, -1).view(i32))
    parts.append(state.items.index_select(0, slots).view(i32))
    return torch.cat(parts, 1, out=out)


def torch_resume(state, blob, slots):
    """resume as torch ops: the split and one index_copy_ per state tensor (no
    check of the rows: the composition of the same result for valid rows)."""
    lay, f32, i64 = state.blob_layout(), torch.float32, torch.int64

    def part(name, dtype):
        w0, n = lay[name]
        return blob[:, w0:w0 + n].view(dtype)

    state.count.index_copy_(0, slots, part("count", i64)[:, 0])
    state.out.index_copy_(0, slots, part("out", f32))
    for i, (h, conv) in enumerate(zip(state.h, state.conv)):
        h.index_copy_(0, slots, part(f"h{i}", f32))
        conv.index_copy_(0, slots, part(f"conv{i}", f32).reshape(-1, *conv.shape[1:]))
    state.items.index_copy_(0, slots, part("items", i64))


def park_leg(model, B: int, seq, windows: int, N: int = 4096) -> dict:
    """Parking, resuming and exchanging B of N live sessions (S = L remembered
    items): session.park / resume / exchange, one rb_session_transfer launch
    each, against the torch composition of the same result, alternating window
    by window in this process."""
    from datamining_recblr_amd import session

    dev = seq.device
    g = torch.Generator().manual_seed(B)
    states = [model.session_open(N, history=L) for _ in range(2)]     # kernel's, torch's
    fill = torch.randint(1, N_ITEMS, (N, 32), generator=g).to(dev)
    for st in states:
        model.session_append(st, fill)                                # live slots, full of values
    ker, tor = states
    slots = torch.randperm(N, generator=g)[:B].to(dev)
    W = ker.blob_words
    lay = ker.blob_layout()
    assert "pad" not in lay, "the composition below cats no pad"
    head = torch.tensor([ker.blob_tag, 0], device=dev, dtype=torch.int32).expand(B, 2)
    # the sessions that come in: B other live sessions
    donor = model.session_open(B, history=L)
    model.session_append(donor, seq[:, :48])
    incoming = session.park(donor)
    buf_k, buf_t = (torch.empty((B, W), device=dev, dtype=torch.int32) for _ in range(2))
    # the same results first
    equal = torch.equal(session.park(ker, slots, out=buf_k), torch_park(tor, slots, head, buf_t))
    session.resume(ker, incoming, slots)
    torch_resume(tor, incoming, slots)
    same = lambda: all(torch.equal(a, b) for a, b in zip(                      # noqa: E731
        [*ker.h, *ker.conv, ker.count, ker.out, ker.items],
        [*tor.h, *tor.conv, tor.count, tor.out, tor.items]))
    equal = equal and same() and bool((ker.status == session.MOVED).all())
    swap_k, swap_t = [incoming.clone(), buf_k], [incoming.clone(), buf_t]

    def exchange_kernel():
        session.exchange(ker, swap_k[0], slots, out=swap_k[1])
        swap_k.reverse()

    def exchange_torch():
        torch_park(tor, slots, head, swap_t[1])
        torch_resume(tor, swap_t[0], slots)
        swap_t.reverse()

    legs = dict(
        park=(lambda: session.park(ker, slots, out=buf_k),
              lambda: torch_park(tor, slots, head, buf_t)),
        resume=(lambda: session.resume(ker, incoming, slots),
                lambda: torch_resume(tor, incoming, slots)),
        exchange=(exchange_kernel, exchange_torch))
    calls = 2000          # a call is 20-130 us: windows of 40-250 ms
    row = dict(B=B, N=N, S=L, blob_words=W, blob_bytes=4 * W, calls_per_window=calls)
    for name, (kernel, composed) in legs.items():
        for _ in range(2):
            window_ms(kernel, calls)
            window_ms(composed, calls)
        tk, tt = [], []
        for _ in range(windows):
            tk.append(window_ms(kernel, calls))
            tt.append(window_ms(composed, calls))
        k, t = statistics.median(tk), statistics.median(tt)
        row.update({f"{name}_ms": round(k, 4), f"{name}_ms_min": round(min(tk), 4),
                    f"{name}_ms_max": round(max(tk), 4), f"{name}_torch_ms": round(t, 4),
                    f"{name}_torch_ms_min": round(min(tt), 4),
                    f"{name}_torch_ms_max": round(max(tt), 4),
                    f"torch_over_{name}": round(t / k, 2)})
        if B >= 2048:       # bytes moved: each word read once and written once
            moved = (4 if name == "exchange" else 2) * B * W * 4
            row[f"{name}_bytes"] = moved
            row[f"{name}_gb_per_s"] = round(moved / (k * 1e-3) / 1e9, 1)
    equal = equal and same()              # after an even number of exchanges on both sides
    row.update(round_trip_ms=round(row["park_ms"] + row["resume_ms"], 4),
               kernel_equals_torch=bool(equal))
    return row


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 2048])
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--recommend", action="store_true",
                    help="also time session_recommend against a caller-kept seen-item matrix")
    ap.add_argument("--park", action="store_true",
                    help="time only session park / resume / exchange against their torch "
                         "composition (B of 4,096 slots)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_session needs the GPU: a CPU timing says nothing about it")
    dev = torch.device("cuda:0")
    cfg = dict(hidden_size=128, loss_type="CE", num_layers=2, dropout_prob=0.2, expand=2,
               d_conv=4, bd_lru_only=False, disable_conv1d=False, disable_ffn=False,
               MAX_ITEM_LIST_LENGTH=L)
    torch.manual_seed(2020)
    model = RecBLR(cfg, SyntheticDataset(N_ITEMS)).to(dev).eval()
    if args.park:
        park_rows = []
        with torch.no_grad():
            for B in args.batches:
                g = torch.Generator().manual_seed(B)
                seq = torch.randint(1, N_ITEMS, (B, L), generator=g).to(dev)
                park_rows.append(park_leg(model, B, seq, args.windows))
        line = json.dumps(dict(bench="session_park", d=128, layers=2, K=4, L=L, S=L,
                               n_items=N_ITEMS, windows=args.windows, park_rows=park_rows))
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(line + "\n")
        return
    rows, prefill_rows, append_rows, recommend_rows = [], [], [], []
    with torch.no_grad():
        for B in args.batches:
            g = torch.Generator().manual_seed(B)
            seq_h = torch.randint(1, N_ITEMS, (B, L), generator=g)
            lens_h = torch.full((B,), L, dtype=torch.int64)
            seq = seq_h.to(dev)
            lens = attach_host_lengths(lens_h.to(dev), lens_h)   # forward without a host sync
            state = model.session_open(B)
            got = model.session_prefill(state, seq, lens)
            ref = model(seq, lens)
            err = (got - ref).abs().max().item()
            nxt = torch.randint(1, N_ITEMS, (B,), generator=g).to(dev)
            step = lambda: model.session_step(state, nxt)       # noqa: E731
            full = lambda: model(seq, lens)                      # noqa: E731
            step_calls = 200
            full_calls = 20 if B <= 64 else 5
            for _ in range(2):   # warm-up of both shapes
                window_ms(step, step_calls)
                window_ms(full, full_calls)
            ts, tf = [], []
            for _ in range(args.windows):   # alternate the two paths
                ts.append(window_ms(step, step_calls))
                tf.append(window_ms(full, full_calls))
            s, f = statistics.median(ts), statistics.median(tf)
            rows.append(dict(B=B, step_ms=round(s, 4), step_ms_min=round(min(ts), 4),
                             step_ms_max=round(max(ts), 4), forward_ms=round(f, 4),
                             forward_ms_min=round(min(tf), 4), forward_ms_max=round(max(tf), 4),
                             forward_over_step=round(f / s, 1),
                             prefill_vs_forward_max_abs_err=err))
            prefill_rows.append(prefill_leg(model, B, seq, lens, args.windows))
            append_rows.append(append_leg(model, B, seq, lens, g, args.windows))
            if args.recommend:
                recommend_rows.append(recommend_leg(model, B, seq, lens, g, args.windows))
    line = json.dumps(dict(bench="session_step", d=128, layers=2, K=4, L=L, n_items=N_ITEMS,
                           windows=args.windows, rows=rows, prefill_rows=prefill_rows,
                           append_rows=append_rows,
                           **(dict(recommend_rows=recommend_rows) if args.recommend else {})))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

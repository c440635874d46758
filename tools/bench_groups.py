#!/usr/bin/env python
"""Diversity caps in top-k retrieval: scoring.top_items under groups /
max_per_group beside the uncapped call and the torch composition.

One run per (k, B) in k = 10 / 64, B = 1 / 64 / 2,048 (d = 128, V = 10,544), the
legs alternated window by window (tools/bench_dense.window_ms):

  * plain            top_items without a cap (rb_item_topk);
  * <layout>_m<m>    with a cap of m = 1 / 3 per group (rb_item_topk_grouped);
  * torch_<layout>_m<m>
                     the composition: full_sort_scores, a stable descending
                     sort, the cap as a segmented count over a stable sort by
                     group, the first k — the [B, V] matrix and two sorts of it.

Layouts: mod50 (group = id % 50), blocks500 (500 contiguous blocks of 21 or 22
items) and hot (mod50, but the table rows of group 7 share an offset that every
request leans on, so one group holds each row's best items and the cap binds
on every list).

Reported per leg: the median window, its min and max and the spread (max -
min) / median; per capped leg its ratio to plain and to its torch composition,
and whether the two legs' windows overlap.

--plain-only times the plain leg alone and needs nothing this feature adds, so
the same file runs on the commit before it; --baseline takes the JSON lines of
such runs (of either tree, alternated by the caller in one job) and reports the
uncapped call against them: "the un-grouped call is unchanged".

    python tools/bench_groups.py [--windows 7] [--steps 100] [--out result.json]
                                 [--plain-only --tag NAME] [--baseline a.json b.json ...]

Prints one JSON line.  Needs the GPU; there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_dense import window_ms  # noqa: E402
from datamining_recblr_amd import scoring  # noqa: E402

BATCHES = (1, 64, 2048)
KS = (10, 64)
CAPS = (1, 3)
LAYOUTS = ("mod50", "blocks500", "hot")
HOT_GROUP = 7


def _legs(B, k, a, dev, plain_only):
    g = torch.Generator().manual_seed(1000 + B)
    seq = torch.randn(B, a.hidden, generator=g)
    table = torch.randn(a.items, a.hidden, generator=g)
    V = a.items
    legs = {"plain": lambda: scoring.top_items(seq_d, table_d, k)}
    seq_d, table_d = seq.to(dev), table.to(dev)
    if plain_only:
        return legs, {}
    ids = torch.arange(V)
    group_of = {"mod50": ids % 50, "blocks500": ids * 500 // V, "hot": ids % 50}
    # hot: group 7's rows share an offset u and every request leans on u
    u = torch.randn(a.hidden, generator=g)
    hot_table = table.clone()
    hot_table[ids % 50 == HOT_GROUP] += u
    hot_seq = (seq + 2.0 * u).to(dev)
    hot_table = hot_table.to(dev)
    same, binds = {}, {}
    for layout in LAYOUTS:
        groups = scoring.item_groups(group_of[layout], device=dev)
        s, t = (hot_seq, hot_table) if layout == "hot" else (seq_d, table_d)
        gid = groups.ids.to(torch.int64)
        for m in CAPS:
            name = f"{layout}_m{m}"

            def capped(s=s, t=t, groups=groups, m=m):
                return scoring.top_items(s, t, k, groups=groups, max_per_group=m)

            def composed(s=s, t=t, gid=gid, m=m):
                sc = scoring.full_sort_scores(s, t)
                sc[:, 0] = float("-inf")
                order = torch.sort(sc, dim=1, descending=True, stable=True).indices
                by = torch.sort(gid[order], dim=1, stable=True)
                pos = torch.arange(V, device=dev)[None, :].expand(B, -1)
                head = torch.ones_like(pos, dtype=torch.bool)
                head[:, 1:] = by.values[:, 1:] != by.values[:, :-1]
                seen = pos - torch.where(head, pos, torch.zeros_like(pos)).cummax(1).values
                seen = torch.empty_like(seen).scatter_(1, by.indices, seen)
                first = torch.sort((seen >= m).to(torch.int8), dim=1, stable=True).indices[:, :k]
                top, dead = order.gather(1, first), seen.gather(1, first) >= m
                return (top.masked_fill(dead, -1),
                        sc.gather(1, top).masked_fill(dead, float("-inf")))

            legs[name] = capped
            legs[f"torch_{name}"] = composed
            got, ref = capped()[0], composed()[0]
            same[name] = float((got == ref).float().mean())
            binds[name] = float((got != scoring.top_items(s, t, k)[0]).any(1).float().mean())
    return legs, {"ids_equal_torch_composition": same, "rows_the_cap_changes": binds}


def _measure(legs, a):
    times = {name: [] for name in legs}
    for w in range(a.warmup_windows + a.windows):
        for name, fn in legs.items():           # alternated: one window of each per round
            ms = window_ms(fn, a.steps)
            if w >= a.warmup_windows:
                times[name].append(ms)
    return times


def _versus(times, x, y):
    """Leg x against leg y: the medians' ratio x / y and whether the windows of
    the two overlap (a difference inside the legs' own spread)."""
    mx, my = statistics.median(times[x]), statistics.median(times[y])
    overlap = min(times[x]) <= max(times[y]) and min(times[y]) <= max(times[x])
    return {"ratio": round(mx / my, 3), "windows_overlap": overlap}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--items", type=int, default=10544)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup-windows", type=int, default=1)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--tag", default="this")
    ap.add_argument("--baseline", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_groups needs a ROCm GPU")
    dev = torch.device("cuda:0")
    res = {"tag": a.tag, "shape": {"hidden": a.hidden, "items": a.items},
           "windows": a.windows, "steps_per_window": a.steps, "cases": {}}
    capped = [f"{layout}_m{m}" for layout in LAYOUTS for m in CAPS]
    for k in KS:
        for B in BATCHES:
            legs, info = _legs(B, k, a, dev, a.plain_only)
            times = _measure(legs, a)
            med = {name: statistics.median(v) for name, v in times.items()}
            out = {"ms": {n: round(v, 4) for n, v in med.items()},
                   "ms_min_max": {n: [round(min(v), 4), round(max(v), 4)]
                                  for n, v in times.items()},
                   "spread": {n: round((max(v) - min(v)) / med[n], 3) for n, v in times.items()},
                   **info}
            if not a.plain_only:
                out["vs_plain"] = {n: _versus(times, n, "plain") for n in capped}
                out["torch_vs_capped"] = {n: _versus(times, f"torch_{n}", n) for n in capped}
            res["cases"][f"k{k}_B{B}"] = out
    # this run's plain leg against --plain-only runs (JSON lines of this tool,
    # each tagged with the tree it ran on)
    if a.baseline:
        runs = []
        for path in a.baseline:
            with open(path) as f:
                runs.append(json.loads(f.readline()))
        res["plain_runs"] = {}
        for case in res["cases"]:
            rows = [{"tag": r["tag"], "ms": r["cases"][case]["ms"]["plain"],
                     "ms_min_max": r["cases"][case]["ms_min_max"]["plain"]} for r in runs]
            rows.append({"tag": a.tag + " (all legs)", "ms": res["cases"][case]["ms"]["plain"],
                         "ms_min_max": res["cases"][case]["ms_min_max"]["plain"]})
            res["plain_runs"][case] = rows
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

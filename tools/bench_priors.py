#!/usr/bin/env python
"""Score priors in top-k retrieval: scoring.top_items under prior / prior_rows /
prior_weight beside the un-priored call and the torch composition.

One run per batch size B in 1 / 64 / 2,048 (d = 128, V = 10,544, k = 10), the
legs alternated window by window (tools/bench_dense.window_ms):

  * plain            top_items without a prior (rb_item_topk);
  * shared           one prior row for every sequence (prior_rows None, a
                     scalar weight): the one-value-per-lane shuffle path;
  * mixed8           prior rows drawn per sequence from P = 8 and a [B] weight:
                     the per-lane gathers;
  * combined         the shared prior with a filter keeping about 5 % of the
                     items and a cap of m = 1 over id % 50;
  * filtered_capped  that filter and cap without a prior (what `combined` adds
                     the prior to);
  * torch_shared, torch_mixed8
                     the composition: full_sort_scores, add w[:, None] *
                     values[p], mask item 0, torch.topk — the [B, V] matrix;
  * torch_filtered   the composition with the filter's masked_fill on top; it
                     leaves the cap out (a cap needs the full sort of
                     tools/bench_groups.py), so it is a lower bound for what
                     composes `combined`.

Reported per leg: the median window, its min and max and the spread (max -
min) / median; per priored leg its ratio to plain and to its torch composition,
and whether the two legs' windows overlap.

--plain-only times the plain leg alone and needs nothing this feature adds, so
the same file runs on the commit before it; --baseline takes the JSON lines of
such runs (of either tree, alternated by the caller in one job) and reports the
un-priored call against them: "the call without a prior is unchanged".

    python tools/bench_priors.py [--windows 9] [--steps 200] [--out result.json]
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
PRIORED = ("shared", "mixed8", "combined")
COMPOSED = {"shared": "torch_shared", "mixed8": "torch_mixed8", "combined": "torch_filtered"}


def _legs(B, a, dev, plain_only):
    g = torch.Generator().manual_seed(1000 + B)
    seq = torch.randn(B, a.hidden, generator=g).to(dev)
    table = torch.randn(a.items, a.hidden, generator=g).to(dev)
    k, V = a.k, a.items
    legs = {"plain": lambda: scoring.top_items(seq, table, k)}
    if plain_only:
        return legs, {}
    counts = torch.randint(0, 1000, (V,), generator=g)
    bank = torch.stack([scoring.log_popularity(counts)] +
                       [torch.randn(V, generator=g) for _ in range(7)])
    one = scoring.item_priors(bank[0], device=dev)
    eight = scoring.item_priors(bank, device=dev)
    rows8 = torch.randint(0, 8, (B,), generator=g).to(dev)
    w8 = (0.5 + torch.rand(B, generator=g)).to(dev)
    mask = torch.rand(V, generator=g) < 0.05
    allow = scoring.item_filters(mask, device=dev)
    allowed = allow.mask()[0]
    groups = scoring.item_groups(torch.arange(V) % 50, device=dev)
    w1 = -0.5

    def composed(prior, rows, w, drop=None):
        def run():
            s = scoring.full_sort_scores(seq, table)
            s = s + w * (prior.values[rows] if rows is not None else prior.values[:1])
            if drop is not None:
                s = s.masked_fill(drop, float("-inf"))
            s[:, 0] = float("-inf")
            return torch.topk(s, k, dim=1)
        return run

    legs["shared"] = lambda: scoring.top_items(seq, table, k, prior=one, prior_weight=w1)
    legs["mixed8"] = lambda: scoring.top_items(seq, table, k, prior=eight, prior_rows=rows8,
                                               prior_weight=w8)
    legs["combined"] = lambda: scoring.top_items(seq, table, k, prior=one, prior_weight=w1,
                                                 allow=allow, groups=groups, max_per_group=1)
    legs["filtered_capped"] = lambda: scoring.top_items(seq, table, k, allow=allow, groups=groups,
                                                        max_per_group=1)
    legs["torch_shared"] = composed(one, None, w1)
    legs["torch_mixed8"] = composed(eight, rows8, w8[:, None])
    legs["torch_filtered"] = composed(one, None, w1, ~allowed[None, :])
    # the fused call and the composition select the same items (ties aside)
    same = {}
    for name in ("shared", "mixed8"):
        ids = legs[name]()[0]
        same[name] = float((ids == legs[COMPOSED[name]]().indices).float().mean())
    return legs, {"kept_items": int(mask.sum()), "ids_equal_torch_composition": same}


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
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup-windows", type=int, default=2)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--tag", default="this")
    ap.add_argument("--baseline", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_priors needs a ROCm GPU")
    dev = torch.device("cuda:0")
    res = {"tag": a.tag, "shape": {"hidden": a.hidden, "items": a.items, "k": a.k},
           "windows": a.windows, "steps_per_window": a.steps, "batches": {}}
    for B in BATCHES:
        legs, info = _legs(B, a, dev, a.plain_only)
        times = _measure(legs, a)
        med = {name: statistics.median(v) for name, v in times.items()}
        out = {"ms": {n: round(v, 4) for n, v in med.items()},
               "ms_min_max": {n: [round(min(v), 4), round(max(v), 4)] for n, v in times.items()},
               "spread": {n: round((max(v) - min(v)) / med[n], 3) for n, v in times.items()},
               **info}
        if not a.plain_only:
            out["vs_plain"] = {n: _versus(times, n, "plain") for n in PRIORED}
            out["combined_vs_filtered_capped"] = _versus(times, "combined", "filtered_capped")
            out["torch_vs_priored"] = {n: _versus(times, COMPOSED[n], n) for n in PRIORED}
        res["batches"][str(B)] = out
    # this run's plain leg against --plain-only runs (JSON lines of this tool,
    # each tagged with the tree it ran on)
    if a.baseline:
        runs = []
        for path in a.baseline:
            with open(path) as f:
                runs.append(json.loads(f.readline()))
        res["plain_runs"] = {}
        for B in BATCHES:
            rows = [{"tag": r["tag"], "ms": r["batches"][str(B)]["ms"]["plain"],
                     "ms_min_max": r["batches"][str(B)]["ms_min_max"]["plain"]} for r in runs]
            rows.append({"tag": a.tag + " (all legs)", "ms": res["batches"][str(B)]["ms"]["plain"],
                         "ms_min_max": res["batches"][str(B)]["ms_min_max"]["plain"]})
            res["plain_runs"][str(B)] = rows
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

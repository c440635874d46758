"""Reranking candidate lists: scoring.top_candidates (rb_candidate_topk, one
launch) against the torch composition and against sweeping the whole table,
and scoring.candidate_ranks against predict on the expanded batch.

Shapes: d = 128, V = 10,544, B in {1, 64, 2048}, C in {100, 1000, 4096}, k = 10.
Legs per shape, on the same h [B, d], table and candidates [B, C]:

  top_candidates   the kernel path;
  torch            what a user writes today: table[cand] ([B, C, d]), a batched
                   product, scoring.order_candidates on the scores;
  top_items        scoring.top_items over the whole table, the "just sweep
                   everything" baseline (it ranks V items, not the C asked for).

For C = 100, sampled evaluation: scoring.candidate_ranks on h against the torch
path on h, and at the model level RecBLR.sampled_rank (one forward of B rows,
then the kernel) against RecBLR.predict on the batch expanded to B * 101 rows
(sequences of --seq-len items, lengths ~ U{1..L}).

All legs of a shape alternate window by window in one process; a window is
--steps calls (fewer for the slow legs) and ends in a device synchronise; the
first windows are warm-up; the reported time is the median window per call
with the smallest and largest beside it.  The kernels are then timed by HIP
events in a pass of their own and set against the bytes they must read, (C +
1) * d * 4 * B, at 8 TB/s.

    python tools/bench_candidates.py [--windows 9] [--steps 200] [--seq-len 50]
                                     [--out profiles/candidates_bench.json]

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
from datamining_recblr_amd import kernels, scoring  # noqa: E402
from datamining_recblr_amd.distributed import synthetic_interaction  # noqa: E402
from datamining_recblr_amd.model import RecBLR  # noqa: E402
from datamining_recblr_amd.recbole_compat import SyntheticDataset  # noqa: E402

HBM_BYTES_PER_S = 8e12
BATCHES = (1, 64, 2048)
LISTS = (100, 1000, 4096)
K = 10


def torch_composition(h, table, cand, k):
    scores = torch.bmm(table[cand], h[:, :, None])[:, :, 0]
    return scoring.order_candidates(scores, cand, k, 1, num_items=table.shape[0])


def run_legs(legs, steps, windows, warmup):
    """legs: name -> (fn, steps divisor).  Alternated: one window of each per
    round.  name -> [ms per call of every kept window]."""
    times = {k: [] for k in legs}
    for w in range(warmup + windows):
        for name, (fn, div) in legs.items():
            ms = window_ms(fn, max(1, steps // div))
            if w >= warmup:
                times[name].append(ms)
    return times


def report(times):
    return {k: {"ms": round(statistics.median(v), 4), "min": round(min(v), 4),
                "max": round(max(v), 4)} for k, v in times.items()}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--items", type=int, default=10544)
    ap.add_argument("--seq-len", type=int, default=50)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup-windows", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_candidates needs a ROCm GPU")
    dev = torch.device("cuda:0")
    d, V = a.hidden, a.items
    cfg = dict(hidden_size=d, loss_type="CE", num_layers=a.layers, dropout_prob=0.2, expand=2,
               d_conv=4, bd_lru_only=False, disable_conv1d=False, disable_ffn=False,
               MAX_ITEM_LIST_LENGTH=a.seq_len)
    torch.manual_seed(0)
    model = RecBLR(cfg, SyntheticDataset(V)).to(dev).eval()
    table = model.item_embedding.weight.detach()
    g = torch.Generator().manual_seed(1)
    shapes = {}
    for B in BATCHES:
        inter = synthetic_interaction(B, a.seq_len, V, dev, seed=B)
        with torch.no_grad():
            h = model(inter["item_id_list"], inter["item_length"]).contiguous()
        for C in LISTS:
            cand = torch.randint(1, V, (B, C), generator=g).to(dev)
            slow = 1 if B * C <= 64 * 4096 else 4       # fewer calls per window for the slow legs
            legs = {
                "top_candidates": (lambda: scoring.top_candidates(h, table, cand, K, 1), 1),
                "torch": (lambda: torch_composition(h, table, cand, K), slow),
                "top_items": (lambda: scoring.top_items(h, table, K, 1), 1),
            }
            # the legs agree before they are timed (ids; the torch product rounds its own way)
            ids, _ = scoring.top_candidates(h, table, cand, K, 1)
            ids_t, _ = torch_composition(h, table, cand, K)
            agree = float((ids == ids_t).float().mean())
            if C == 100:
                target = inter["item_id"].to(torch.int64)
                expanded = {"item_id_list": inter["item_id_list"].repeat_interleave(C + 1, 0),
                            "item_length": inter["item_length"].repeat_interleave(C + 1, 0),
                            "item_id": torch.cat([target[:, None], cand], 1).reshape(-1)}
                rows = 4 if B >= 2048 else 1

                def predict_expanded():
                    with torch.no_grad():
                        return model.predict(expanded)

                legs.update({
                    "ranks_kernel": (lambda: scoring.candidate_ranks(h, table, target, cand), 1),
                    "ranks_torch": (lambda: scoring._candidate_ranks_torch(h, table, target, cand,
                                                                          1), slow),
                    "sampled_rank": (lambda: model.sampled_rank(inter, cand), rows),
                    "predict_expanded": (predict_expanded, 4 * rows),
                })
            times = run_legs(legs, a.steps, a.windows, a.warmup_windows)
            rep = report(times)
            names = {"rb_candidate_topk", "rb_candidate_ranks"}
            with kernels.kernel_timing(only=names) as t:
                for _ in range(20):
                    scoring.top_candidates(h, table, cand, K, 1)
                    if C == 100:
                        scoring.candidate_ranks(h, table, target, cand)
            model_bytes = (C + 1) * d * 4 * B
            kern = {}
            for name, s in t.summary().items():
                kern[name] = {"us": round(s["avg_ms"] * 1e3, 2),
                              "model_gb_per_s": round(model_bytes / s["avg_ms"] / 1e6, 1),
                              "share_of_8tb_per_s": round(model_bytes / HBM_BYTES_PER_S * 1e3
                                                          / s["avg_ms"], 4)}
            med = {k: v["ms"] for k, v in rep.items()}
            entry = {"legs": rep, "kernels": kern, "model_bytes": model_bytes,
                     "ids_agree_with_torch": round(agree, 4),
                     "torch_over_top_candidates": round(med["torch"] / med["top_candidates"], 2),
                     "top_items_over_top_candidates": round(med["top_items"]
                                                            / med["top_candidates"], 2)}
            if C == 100:
                entry["ranks_torch_over_kernel"] = round(med["ranks_torch"] / med["ranks_kernel"], 2)
                entry["predict_expanded_over_sampled_rank"] = round(
                    med["predict_expanded"] / med["sampled_rank"], 2)
            shapes[f"B{B}_C{C}"] = entry
            del legs
            torch.cuda.empty_cache()
    res = {"shape": {"hidden": d, "items": V, "k": K, "seq_len": a.seq_len, "layers": a.layers},
           "windows": a.windows, "calls_per_window": a.steps, "shapes": shapes,
           "peak_mem_gib": round(torch.cuda.max_memory_allocated(dev) / 2**30, 2)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

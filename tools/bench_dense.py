"""All-position ("dense") training step against the ordinary step.

Both steps are forward, loss, backward and Adam of the same model on the same
synthetic batch (B rows, lengths ~ U{1..L}): the ordinary step trains on each
row's last position (B targets; the step bench.py times), the dense step on
every valid position (ntok = sum of lengths targets; RecBLR.calculate_loss_dense).
The two legs alternate window by window in one process, each window ends in a
device synchronise, and the reported time is the median window; the first
windows of both legs are warm-up and are dropped.  A third leg times the
row-chunked CE alone (item_cross_entropy_rows forward + backward on the dense
step's own rows) to give its share of the dense step.

    python tools/bench_dense.py [--batch 2048] [--seq-len 200] [--hidden 128]
                                [--items 10544] [--windows 9] [--steps 5]
                                [--out result.json]

Prints one JSON line.  Needs the GPU; there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from datamining_recblr_amd import scoring  # noqa: E402
from datamining_recblr_amd.distributed import synthetic_interaction  # noqa: E402
from datamining_recblr_amd.model import RecBLR  # noqa: E402
from datamining_recblr_amd.optim import make_adam  # noqa: E402
from datamining_recblr_amd.recbole_compat import SyntheticDataset  # noqa: E402


def window_ms(fn, steps: int) -> float:
    """Host clock around `steps` calls that end in a device synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--seq-len", type=int, default=200)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--items", type=int, default=10544)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup-windows", type=int, default=2)
    ap.add_argument("--chunk-rows", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dense needs a ROCm GPU")
    dev = torch.device("cuda:0")
    cfg = dict(hidden_size=a.hidden, loss_type="CE", num_layers=a.layers, dropout_prob=0.2,
               expand=2, d_conv=4, bd_lru_only=False, disable_conv1d=False, disable_ffn=False,
               MAX_ITEM_LIST_LENGTH=a.seq_len)
    torch.manual_seed(0)
    model = RecBLR(cfg, SyntheticDataset(a.items)).to(dev).train()
    opt = make_adam(model.parameters(), lr=1e-3, weight_decay=0.0)
    inter = synthetic_interaction(a.batch, a.seq_len, a.items, dev, seed=1)
    ntok = int(getattr(inter["item_length"], "_recblr_host_lengths").clamp(1, a.seq_len).sum())

    def step(loss_fn):
        def run():
            loss = loss_fn(inter)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        return run

    model.train_all_positions = False
    ordinary = step(model.calculate_loss)
    dense = step(model.calculate_loss_dense)

    # the CE alone on the dense step's rows (detached: forward + both gradients)
    with torch.no_grad():
        h, _ = model.forward_all(inter["item_id_list"], inter["item_length"])
    m_pad = -(-ntok // 256) * 256
    rows = torch.zeros((m_pad, a.hidden), device=dev)
    rows[:ntok] = h
    rows.requires_grad_()
    g = torch.Generator(device="cpu").manual_seed(2)
    tgt = torch.full((m_pad,), -1, dtype=torch.int64)
    tgt[:ntok] = torch.randint(1, a.items, (ntok,), generator=g)
    tgt = tgt.to(dev)
    table = model.item_embedding.weight

    def ce_only():
        rows.grad = None
        table.grad = None
        scoring.item_cross_entropy_rows(rows, table, tgt, chunk_rows=a.chunk_rows,
                                        n_live=ntok).backward()

    legs = {"ordinary": ordinary, "dense": dense, "dense_ce_only": ce_only}
    times = {k: [] for k in legs}
    for w in range(a.warmup_windows + a.windows):
        for name, fn in legs.items():           # alternated: one window of each per round
            ms = window_ms(fn, a.steps)
            if w >= a.warmup_windows:
                times[name].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {
        "shape": {"batch": a.batch, "seq_len": a.seq_len, "hidden": a.hidden, "items": a.items,
                  "layers": a.layers, "ntok": ntok, "chunk_rows": a.chunk_rows},
        "windows": a.windows, "steps_per_window": a.steps,
        "ordinary_ms": round(med["ordinary"], 3),
        "ordinary_ms_min_max": [round(min(times["ordinary"]), 3), round(max(times["ordinary"]), 3)],
        "ordinary_targets_per_s": round(a.batch / med["ordinary"] * 1e3),
        "dense_ms": round(med["dense"], 3),
        "dense_ms_min_max": [round(min(times["dense"]), 3), round(max(times["dense"]), 3)],
        "dense_targets_per_s": round(ntok / med["dense"] * 1e3),
        "targets_per_s_ratio": round((ntok / med["dense"]) / (a.batch / med["ordinary"]), 2),
        "step_time_ratio": round(med["dense"] / med["ordinary"], 2),
        "dense_ce_only_ms": round(med["dense_ce_only"], 3),
        "dense_ce_share": round(med["dense_ce_only"] / med["dense"], 3),
        "peak_mem_gib": round(torch.cuda.max_memory_allocated(dev) / 2**30, 2),
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

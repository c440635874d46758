"""Top-k item retrieval: the fused kernel (kernels.item_topk, no [B, V]
buffer) against the composed path it replaces, kernels.item_scores +
torch.topk(k) — with a seen-item list of E ids per row the composed path
also scatters -inf over them, the fused one takes the list as an argument.

Both legs run in one process, alternating call by call after warm-up; each
call is timed with HIP events, medians are reported and the outputs of the
two legs are compared on the timed inputs.  Peak memory is torch's allocator
peak above the resident operands.  One JSON line per configuration.

    python tools/topk_bench.py [--shape B V d k]... [--exclude E] [--reps N] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from datamining_recblr_amd import kernels  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, out


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def bench(B, V, d, k, E, reps, warmup, dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    seq = (0.3 * torch.randn(B, d, generator=g)).to(dev)
    W = (0.3 * torch.randn(V, d, generator=g)).to(dev)
    ex = torch.randint(0, V, (B, E), generator=g).to(dev) if E else None

    def fused():
        return kernels.item_topk(seq, W, k, first_item=0, exclude=ex)

    def composed():
        s = kernels.item_scores(seq, W)
        if ex is not None:
            s.scatter_(1, ex, float("-inf"))
        top = torch.topk(s, k, dim=1)
        return top.indices, top.values

    for _ in range(warmup):
        fused()
        composed()
    torch.cuda.synchronize()
    tf, tc = [], []
    for _ in range(reps):
        t, a = timed(fused)
        tf.append(t)
        t, b = timed(composed)
        tc.append(t)
    # same scores; ids may differ only inside groups of equal scores
    same_scores = bool(torch.equal(a[1], b[1]))
    same_ids = float((a[0] == b[0]).float().mean())
    res = {"B": B, "V": V, "d": d, "k": k, "E": E, "reps": reps,
           "fused_us": round(median(tf), 1), "composed_us": round(median(tc), 1),
           "fused_us_min_max": [round(min(tf), 1), round(max(tf), 1)],
           "composed_us_min_max": [round(min(tc), 1), round(max(tc), 1)],
           "fused_peak_mib": round(peak_mib(fused), 1),
           "composed_peak_mib": round(peak_mib(composed), 1),
           "scores_equal": same_scores, "ids_equal_frac": round(same_ids, 6)}
    res["fused_over_composed"] = round(res["fused_us"] / res["composed_us"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, action="append", metavar=("B", "V", "d", "k"))
    ap.add_argument("--exclude", type=int, default=200)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("topk_bench: no GPU (timings are taken on the device only)")
    dev = torch.device("cuda:0")
    shapes = a.shape or [[2048, 10544, 128, 20], [2048, 1 << 18, 128, 20]]
    lines = []
    for B, V, d, k in shapes:
        for E in (0, a.exclude):
            reps = a.reps if B * V <= 1 << 26 else max(20, a.reps // 5)
            line = json.dumps(bench(B, V, d, k, E, reps, a.warmup, dev))
            print(line, flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

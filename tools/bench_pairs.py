"""All-position training with sampled negatives against the dense CE step and
the ordinary step, and the pair-loss kernels against the torch composition.

Steps (forward, loss, backward and Adam of the same model on the same
synthetic batch, B rows, lengths ~ U{1..L}): the ordinary step
(calculate_loss, last position), the dense CE step (calculate_loss_dense) and
the dense pairs step (calculate_loss_pairs: negatives sampled on the device at
every position) at n = 1 and n = 4 negatives.

The loss alone, forward + backward including the table's gradient, on the
dense step's own rows h [ntok, d] with sampled negatives: scoring.pair_loss
(rb_pair_loss_fwd / rb_pair_loss_bwd / rb_embedding_bwd_apply_scaled) against
what a user would write in torch today — two embedding gathers, multiply-sum,
RecBole's BPRLoss and autograd's embedding backward — and the row-chunked CE
on the same rows.

All legs alternate window by window in one process, each window ends in a
device synchronise, the reported time is the median window and the first
windows are warm-up.  The two loss kernels are then timed by HIP events in a
pass of their own and set against their byte floor at 8 TB/s: (2 + n) M d 4
bytes for the forward, the same plus the dh write for the backward.

--popularity adds the dense pairs steps with the negatives drawn from the
popularity proposal (dense_pairs_pop_n{n}; counts: bench_sampled.zipf_counts)
and the sampler alone at every position with and without the alias table
(sample_uniform_n{n}, sample_pop_n{n}); "popularity" in the result holds each
one's ratio to its uniform leg and the two samplers by HIP events.

    python tools/bench_pairs.py [--batch 2048] [--seq-len 200] [--hidden 128]
                                [--items 10544] [--windows 9] [--steps 5]
                                [--popularity] [--out result.json]

Prints one JSON line.  Needs the GPU; there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_dense import window_ms  # noqa: E402
from bench_sampled import zipf_counts  # noqa: E402
from datamining_recblr_amd import kernels, scoring  # noqa: E402
from datamining_recblr_amd.distributed import synthetic_interaction  # noqa: E402
from datamining_recblr_amd.model import RecBLR  # noqa: E402
from datamining_recblr_amd.optim import make_adam  # noqa: E402
from datamining_recblr_amd.recbole_compat import BPRLoss, SyntheticDataset  # noqa: E402

HBM_BYTES_PER_S = 8e12
NEGATIVES = (1, 4)


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
    ap.add_argument("--popularity", action="store_true",
                    help="add the popularity proposal's legs beside the uniform ones")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pairs needs a ROCm GPU")
    dev = torch.device("cuda:0")
    cfg = dict(hidden_size=a.hidden, loss_type="CE", num_layers=a.layers, dropout_prob=0.2,
               expand=2, d_conv=4, bd_lru_only=False, disable_conv1d=False, disable_ffn=False,
               MAX_ITEM_LIST_LENGTH=a.seq_len)
    torch.manual_seed(0)
    model = RecBLR(cfg, SyntheticDataset(a.items)).to(dev).train()
    opt = make_adam(model.parameters(), lr=1e-3, weight_decay=0.0)
    inter = synthetic_interaction(a.batch, a.seq_len, a.items, dev, seed=1)

    def step(loss_fn):
        def run():
            loss = loss_fn(inter)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        return run

    def pairs_loss(n, sampling="uniform"):
        def loss(interaction):
            model.dense_negatives, model.dense_sampling = n, sampling
            return model.calculate_loss_pairs(interaction)
        return loss

    legs = {"ordinary": step(model.calculate_loss), "dense_ce": step(model.calculate_loss_dense)}
    for n in NEGATIVES:
        legs[f"dense_pairs_n{n}"] = step(pairs_loss(n))
    if a.popularity:   # the same step with the negatives drawn from the popularity proposal
        model.set_item_counts(zipf_counts(a.items))
        for n in NEGATIVES:
            legs[f"dense_pairs_pop_n{n}"] = step(pairs_loss(n, "popularity"))

    # ---- the loss alone on the dense step's rows (detached) -------------------------
    with torch.no_grad():
        h, seq = model.forward_all(inter["item_id_list"], inter["item_length"])
    ntok = seq.ntok
    rows = h.clone().requires_grad_()
    table = model.item_embedding.weight
    pos_items = inter["item_id"].to(torch.int64)
    target = kernels.next_item_targets(seq.ids, seq.offsets, seq.order, pos_items)
    negs = {n: kernels.sample_negatives(inter["item_id_list"], inter["item_length"], pos_items, n,
                                        1, a.items, 1234 + n, seq.offsets, seq.inv, ntok)
            for n in NEGATIVES}
    bpr = BPRLoss()

    def loss_kernels(n):
        def run():
            rows.grad = table.grad = None
            scoring.pair_loss(rows, table, target, negs[n]).backward()
        return run

    def loss_torch(n):
        def run():
            rows.grad = table.grad = None
            pos_score = (rows * F.embedding(target, table)).sum(-1)
            neg_score = (rows[:, None, :] * F.embedding(negs[n], table)).sum(-1)
            bpr(pos_score[:, None].expand_as(neg_score), neg_score).backward()
        return run

    m_pad = -(-ntok // 256) * 256
    ce_rows = torch.zeros((m_pad, a.hidden), device=dev)
    ce_rows[:ntok] = h
    ce_rows.requires_grad_()
    ce_tgt = F.pad(target, (0, m_pad - ntok), value=-1)

    def ce_only():
        ce_rows.grad = table.grad = None
        scoring.item_cross_entropy_rows(ce_rows, table, ce_tgt, n_live=ntok).backward()

    legs["loss_ce_rows"] = ce_only
    for n in NEGATIVES:
        legs[f"loss_kernels_n{n}"] = loss_kernels(n)
        legs[f"loss_torch_n{n}"] = loss_torch(n)

    def sample(n, alias):   # the sampler alone, every position of every row
        def run():
            kernels.sample_negatives(inter["item_id_list"], inter["item_length"], pos_items, n, 1,
                                     a.items, 99, seq.offsets, seq.inv, ntok, alias=alias)
        return run

    if a.popularity:
        for n in NEGATIVES:
            legs[f"sample_uniform_n{n}"] = sample(n, None)
            legs[f"sample_pop_n{n}"] = sample(n, model.neg_alias)

    # the two compositions compute the same thing (sampled negatives are never -1 here)
    check = {}
    for n in NEGATIVES:
        loss_kernels(n)()
        gk = (rows.grad.clone(), table.grad.clone())
        loss_torch(n)()
        check[f"n{n}"] = [float((gk[0] - rows.grad).abs().max() / rows.grad.abs().max()),
                          float((gk[1] - table.grad).abs().max() / table.grad.abs().max())]

    times = {k: [] for k in legs}
    for w in range(a.warmup_windows + a.windows):
        for name, fn in legs.items():           # alternated: one window of each per round
            ms = window_ms(fn, a.steps)
            if w >= a.warmup_windows:
                times[name].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}

    # ---- the loss kernels by HIP events, against their byte floor ---------------------
    floors = {}
    names = {"rb_pair_loss_fwd", "rb_pair_loss_bwd", "rb_embedding_bwd_scaled",
             "rb_sample_negatives"}
    for n in NEGATIVES:
        with kernels.kernel_timing(only=names) as t:
            for _ in range(20):
                loss_kernels(n)()
                kernels.sample_negatives(inter["item_id_list"], inter["item_length"], pos_items, n,
                                         1, a.items, 99, seq.offsets, seq.inv, ntok)
        s = t.summary()
        fwd_bytes = (2 + n) * ntok * a.hidden * 4
        bwd_bytes = fwd_bytes + ntok * a.hidden * 4
        out = {k: round(v["avg_ms"] * 1e3, 1) for k, v in s.items()}
        floors[f"n{n}"] = {
            "kernel_us": out,
            "fwd_floor_us": round(fwd_bytes / HBM_BYTES_PER_S * 1e6, 1),
            "bwd_floor_us": round(bwd_bytes / HBM_BYTES_PER_S * 1e6, 1),
            "fwd_share_of_floor": round(fwd_bytes / HBM_BYTES_PER_S * 1e3
                                        / s["rb_pair_loss_fwd"]["avg_ms"], 3),
            "bwd_share_of_floor": round(bwd_bytes / HBM_BYTES_PER_S * 1e3
                                        / s["rb_pair_loss_bwd"]["avg_ms"], 3)}

    def mm(k):
        return [round(min(times[k]), 3), round(max(times[k]), 3)]

    res = {"shape": {"batch": a.batch, "seq_len": a.seq_len, "hidden": a.hidden,
                     "items": a.items, "layers": a.layers, "ntok": ntok},
           "windows": a.windows, "steps_per_window": a.steps,
           "ms": {k: round(v, 3) for k, v in med.items()},
           "ms_min_max": {k: mm(k) for k in med},
           "kernels_vs_torch": {f"n{n}": round(med[f"loss_torch_n{n}"] / med[f"loss_kernels_n{n}"], 2)
                                for n in NEGATIVES},
           "pairs_step_vs_dense_ce_step": {f"n{n}": round(med["dense_ce"] / med[f"dense_pairs_n{n}"], 2)
                                           for n in NEGATIVES},
           "max_rel_diff_kernels_vs_torch_dh_dtable": check,
           "loss_kernels": floors,
           "peak_mem_gib": round(torch.cuda.max_memory_allocated(dev) / 2**30, 2)}
    if a.popularity:
        def versus(pop, uniform):
            gap = abs(med[pop] - med[uniform])
            own = max(max(times[k]) - min(times[k]) for k in (pop, uniform))
            return {"ratio": round(med[pop] / med[uniform], 3), "within_spread": gap <= own}

        sampler_us = {}
        for n in NEGATIVES:
            with kernels.kernel_timing(only={"rb_sample_negatives",
                                             "rb_sample_negatives_alias"}) as t:
                for _ in range(20):
                    sample(n, None)()
                    sample(n, model.neg_alias)()
            sampler_us[f"n{n}"] = {k: round(v["avg_ms"] * 1e3, 1) for k, v in t.summary().items()}
        res["popularity"] = {
            "counts": "zipf_counts(items): floor(1e5 / rank), alpha 0.75, smoothing 1",
            "dense_step": {f"n{n}": versus(f"dense_pairs_pop_n{n}", f"dense_pairs_n{n}")
                           for n in NEGATIVES},
            "sampler": {f"n{n}": versus(f"sample_pop_n{n}", f"sample_uniform_n{n}")
                        for n in NEGATIVES},
            "sampler_us": sampler_us}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

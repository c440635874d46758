#!/usr/bin/env python
"""Sampled softmax with negatives shared per sequence: the loss alone and the
dense training step, beside the pairwise loss and the full cross-entropy.

One run, the legs alternated window by window (tools/bench_dense.window_ms):

  * loss_kernels_n{n}   scoring.shared_softmax_loss, forward and backward
                        including the table gradient, on the dense step's own
                        rows h [ntok, d] (rb_shared_softmax_fwd / _bwd and the
                        two embedding applies), n in 16, 64, 128, 256;
  * loss_torch_n{n}     the same loss composed from torch ops
                        (scoring.shared_softmax_reference: gather table[neg],
                        padded batched product, logsumexp, autograd);
  * loss_pairs_n16      scoring.pair_loss at its largest n;
  * loss_ce_rows        the row-chunked full-vocabulary CE;
  * dense_ce, dense_pairs_n16, dense_sampled_n{n}
                        the whole dense training step with each loss.

Reported per leg: the median window, its min and max, and the repeat-to-repeat
spread (max - min) / median; kernels_vs_torch says whether the kernels' slowest
window still beats the composition's fastest one.

--popularity adds, in the same alternation, the popularity proposal's legs at
n in 16, 64, 256 (counts: zipf_counts, a Zipf-like synthetic distribution over
the items):

  * loss_kernels_pop_n{n}  the loss on lists drawn from the alias table, with
                           the per-item correction (rb_shared_softmax_fwd_items
                           / _bwd_items);
  * loss_kernels_poplists_n{n}, loss_kernels_items_n{n}
                           the two halves of that change alone: the popularity
                           lists with the scalar shift, and the uniform lists
                           with the per-item term;
  * dense_sampled_pop_n{n} the dense step of a dense_sampling 'popularity' model;
  * sample_uniform_n{n}, sample_pop_n{n}
                           the sampler alone, one list per row;

and "popularity" in the result: each leg's ratio to its uniform leg, whether the
difference is inside the two legs' own spreads, and the samplers by HIP events.

    python tools/bench_sampled.py [--batch 2048] [--seq-len 200] [--hidden 128]
                                  [--items 10544] [--windows 7] [--steps 3]
                                  [--popularity] [--out result.json]

Prints one JSON line.  Needs the GPU; there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_dense import window_ms  # noqa: E402
from datamining_recblr_amd import kernels, scoring  # noqa: E402
from datamining_recblr_amd.distributed import synthetic_interaction  # noqa: E402
from datamining_recblr_amd.model import RecBLR  # noqa: E402
from datamining_recblr_amd.optim import make_adam  # noqa: E402
from datamining_recblr_amd.recbole_compat import SyntheticDataset  # noqa: E402

NEGATIVES = (16, 64, 128, 256)
PAIRS_N = 16
POPULARITY_NEGATIVES = (16, 64, 256)


def zipf_counts(n_items: int, seed: int = 0, top: float = 1e5):
    """Zipf-like synthetic train counts [n_items]: the item of popularity rank
    r = 1, 2 ... has floor(top / r) occurrences, the ranks dealt to the ids 1 ..
    n_items - 1 by a seeded permutation (id 0, the padding id, has none)."""
    import numpy as np

    counts = np.zeros(n_items, dtype=np.int64)
    ranks = np.random.default_rng(seed).permutation(n_items - 1) + 1
    counts[1:] = np.floor(top / ranks).astype(np.int64)
    return counts


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--seq-len", type=int, default=200)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--items", type=int, default=10544)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup-windows", type=int, default=2)
    ap.add_argument("--popularity", action="store_true",
                    help="add the popularity proposal's legs beside the uniform ones")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampled needs a ROCm GPU")
    dev = torch.device("cuda:0")
    cfg = dict(hidden_size=a.hidden, loss_type="CE", num_layers=a.layers, dropout_prob=0.2,
               expand=2, d_conv=4, bd_lru_only=False, disable_conv1d=False, disable_ffn=False,
               MAX_ITEM_LIST_LENGTH=a.seq_len, train_all_positions=True)
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

    def with_n(method, n, sampling="uniform"):
        def loss(interaction):
            model.dense_negatives, model.dense_sampling = n, sampling
            return method(interaction)
        return loss

    legs = {"dense_ce": step(model.calculate_loss_dense),
            f"dense_pairs_n{PAIRS_N}": step(with_n(model.calculate_loss_pairs, PAIRS_N))}
    for n in NEGATIVES:
        legs[f"dense_sampled_n{n}"] = step(with_n(model.calculate_loss_sampled, n))
    if a.popularity:
        model.set_item_counts(zipf_counts(a.items))
        for n in POPULARITY_NEGATIVES:
            legs[f"dense_sampled_pop_n{n}"] = step(with_n(model.calculate_loss_sampled, n,
                                                          "popularity"))

    # ---- the loss alone on the dense step's rows (detached) -------------------------
    with torch.no_grad():
        h, seq = model.forward_all(inter["item_id_list"], inter["item_length"])
    ntok = seq.ntok
    rows = h.clone().requires_grad_()
    table = model.item_embedding.weight
    item_seq, lengths = inter["item_id_list"].to(torch.int64), inter["item_length"].to(torch.int64)
    pos_items = inter["item_id"].to(torch.int64)
    target = kernels.next_item_targets(seq.ids, seq.offsets, seq.order, pos_items)
    lists = {n: kernels.sample_negatives(item_seq, lengths, pos_items, n, 1, a.items, 1234 + n)
             for n in NEGATIVES}
    pair_negs = kernels.sample_negatives(item_seq, lengths, pos_items, PAIRS_N, 1, a.items, 99,
                                         seq.offsets, seq.inv, ntok)
    shifts = {n: math.log((a.items - 1) / n) for n in NEGATIVES}

    def loss_kernels(n):
        def run():
            rows.grad = table.grad = None
            scoring.shared_softmax_loss(rows, table, target, lists[n], seq.offsets, seq.order,
                                        shifts[n], max_len=a.seq_len).backward()
        return run

    def loss_torch(n):
        def run():
            rows.grad = table.grad = None
            scoring.shared_softmax_reference(rows, table, target, lists[n], seq.offsets,
                                             seq.order, shifts[n]).backward()
        return run

    def loss_pairs():
        rows.grad = table.grad = None
        scoring.pair_loss(rows, table, target, pair_negs).backward()

    m_pad = -(-ntok // 256) * 256
    ce_rows = torch.zeros((m_pad, a.hidden), device=dev)
    ce_rows[:ntok] = h
    ce_rows.requires_grad_()
    ce_tgt = F.pad(target, (0, m_pad - ntok), value=-1)

    def ce_only():
        ce_rows.grad = table.grad = None
        scoring.item_cross_entropy_rows(ce_rows, table, ce_tgt, n_live=ntok).backward()

    legs["loss_ce_rows"] = ce_only
    legs[f"loss_pairs_n{PAIRS_N}"] = loss_pairs
    for n in NEGATIVES:
        legs[f"loss_kernels_n{n}"] = loss_kernels(n)
        legs[f"loss_torch_n{n}"] = loss_torch(n)

    # ---- the popularity proposal: its lists, the per-item correction, the sampler ------
    if a.popularity:
        alias, item_shift = model.neg_alias, model.neg_item_shift
        pop_lists = {n: kernels.sample_negatives(item_seq, lengths, pos_items, n, 1, a.items,
                                                 1234 + n, alias=alias)
                     for n in POPULARITY_NEGATIVES}

        def loss_kernels_pop(n, lists_=pop_lists, shift_=item_shift):
            def run():
                rows.grad = table.grad = None
                scoring.shared_softmax_loss(rows, table, target, lists_[n], seq.offsets,
                                            seq.order, -math.log(n), max_len=a.seq_len,
                                            item_shift=shift_).backward()
            return run

        def sample(n, table_):
            def run():
                kernels.sample_negatives(item_seq, lengths, pos_items, n, 1, a.items, 77,
                                         alias=table_)
            return run

        for n in POPULARITY_NEGATIVES:
            legs[f"loss_kernels_pop_n{n}"] = loss_kernels_pop(n)
            # the two halves of the difference: the lists alone (scalar shift), the term alone
            legs[f"loss_kernels_poplists_n{n}"] = loss_kernels_pop(n, pop_lists, None)
            legs[f"loss_kernels_items_n{n}"] = loss_kernels_pop(n, lists, item_shift)
            legs[f"sample_uniform_n{n}"] = sample(n, None)
            legs[f"sample_pop_n{n}"] = sample(n, alias)

    # the two compositions compute the same thing
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

    # ---- the launches by HIP events ---------------------------------------------------
    names = {"rb_shared_softmax_fwd", "rb_shared_softmax_bwd", "rb_embedding_bwd_scaled",
             "rb_embedding_bwd"}
    launches = {}
    for n in NEGATIVES:
        with kernels.kernel_timing(only=names) as t:
            for _ in range(10):
                loss_kernels(n)()
        launches[f"n{n}"] = {k: round(v["avg_ms"] * 1e3, 1) for k, v in t.summary().items()}

    def mm(k):
        return [round(min(times[k]), 3), round(max(times[k]), 3)]

    def spread(k):
        return round((max(times[k]) - min(times[k])) / med[k], 3)

    res = {"shape": {"batch": a.batch, "seq_len": a.seq_len, "hidden": a.hidden,
                     "items": a.items, "layers": a.layers, "ntok": ntok},
           "windows": a.windows, "steps_per_window": a.steps,
           "ms": {k: round(v, 3) for k, v in med.items()},
           "ms_min_max": {k: mm(k) for k in med},
           "spread": {k: spread(k) for k in med},
           "kernels_vs_torch": {
               f"n{n}": {"ratio": round(med[f"loss_torch_n{n}"] / med[f"loss_kernels_n{n}"], 2),
                         "kernels_max_below_torch_min":
                             max(times[f"loss_kernels_n{n}"]) < min(times[f"loss_torch_n{n}"])}
               for n in NEGATIVES},
           "max_rel_diff_kernels_vs_torch_dh_dtable": check,
           "launch_us": launches,
           "peak_mem_gib": round(torch.cuda.max_memory_allocated(dev) / 2**30, 2)}
    if a.popularity:
        def versus(pop, uniform):
            """The popularity leg against the uniform one: the medians' ratio
            and whether the difference is inside the legs' own spreads."""
            gap = abs(med[pop] - med[uniform])
            own = max(max(times[k]) - min(times[k]) for k in (pop, uniform))
            return {"ratio": round(med[pop] / med[uniform], 3), "within_spread": gap <= own}

        pop_names = {"rb_shared_softmax_fwd_items", "rb_shared_softmax_bwd_items",
                     "rb_embedding_bwd_scaled", "rb_embedding_bwd", "rb_sample_negatives",
                     "rb_sample_negatives_alias"}
        pop_launches = {}
        for n in POPULARITY_NEGATIVES:
            with kernels.kernel_timing(only=pop_names) as t:
                for _ in range(10):
                    loss_kernels_pop(n)()
                    sample(n, None)()
                    sample(n, alias)()
            pop_launches[f"n{n}"] = {k: round(v["avg_ms"] * 1e3, 1)
                                     for k, v in t.summary().items()}
            for key, fn in (("popularity_lists_scalar_shift", loss_kernels_pop(n, pop_lists, None)),
                            ("uniform_lists_item_shift", loss_kernels_pop(n, lists, item_shift))):
                with kernels.kernel_timing(only=names | pop_names) as t:
                    for _ in range(10):
                        fn()
                pop_launches[f"n{n}_{key}"] = {k: round(v["avg_ms"] * 1e3, 1)
                                               for k, v in t.summary().items()}
        uniq = {f"n{n}": [int(torch.unique(lists[n]).numel()), int(torch.unique(pop_lists[n]).numel())]
                for n in POPULARITY_NEGATIVES}
        res["popularity"] = {
            "counts": "zipf_counts(items): floor(1e5 / rank), alpha 0.75, smoothing 1",
            "item_shift_min_max": [round(float(item_shift[1:].min()), 3),
                                   round(float(item_shift[1:].max()), 3)],
            "loss": {f"n{n}": versus(f"loss_kernels_pop_n{n}", f"loss_kernels_n{n}")
                     for n in POPULARITY_NEGATIVES},
            "loss_popularity_lists_scalar_shift": {
                f"n{n}": versus(f"loss_kernels_poplists_n{n}", f"loss_kernels_n{n}")
                for n in POPULARITY_NEGATIVES},
            "loss_uniform_lists_item_shift": {
                f"n{n}": versus(f"loss_kernels_items_n{n}", f"loss_kernels_n{n}")
                for n in POPULARITY_NEGATIVES},
            "dense_step": {f"n{n}": versus(f"dense_sampled_pop_n{n}", f"dense_sampled_n{n}")
                           for n in POPULARITY_NEGATIVES},
            "sampler": {f"n{n}": versus(f"sample_pop_n{n}", f"sample_uniform_n{n}")
                        for n in POPULARITY_NEGATIVES},
            "distinct_ids_uniform_vs_popularity": uniq,
            "launch_us": pop_launches}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

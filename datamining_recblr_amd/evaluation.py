"""Batched full-sort evaluation.

Two evaluators reduce the [B, n_items] full-sort scores of the reference to
the rank of each row's target (rb_item_rank, no score matrix):

  * ``full_sort_metrics`` — RecBole's full-sort Hit/NDCG/MRR@k for
    leave-one-out sequential batches (config.yaml: metrics Hit, NDCG, MRR,
    topk [10, 20]; item 0 masked as RecBole does).
  * ``evaluate_unseen`` — the unseen-user evaluation of
    run_with_unseen.py:209-265, which runs ``full_sort_predict`` once per user
    at batch size 1 on the unpadded sequence.  Here users are sorted by
    length and batched; ``RecBLR.forward(..., exact_lengths=True)`` gives each
    row the pad prefix of its own length, so every row equals its batch-1
    forward (up to fp32 reassociation in the GEMMs).  Metrics follow the
    reference: NDCG@k as sklearn.metrics.ndcg_score (tie-averaged) over
    scores[1:], Hit@k as "target among the k best of scores[1:]".

``recommend`` returns what a served model returns: each user's k best items
(rb_item_topk, again no score matrix), batched like ``evaluate_unseen``.
"""
from __future__ import annotations

import torch

from .scoring import rank_metrics, target_ranks, top_items

__all__ = ["unseen_inputs", "evaluate_unseen", "full_sort_metrics", "recommend"]


def unseen_inputs(sequences, pad_id: int = 0):
    """(item_id_lists, targets) from full per-user id sequences, as
    run_with_unseen.py:410-416 (mode "none"): inputs are seq[:-1], or the
    padding item alone for a one-item sequence; the target is seq[-1]."""
    lists, targets = [], []
    for seq in sequences:
        seq = list(seq)
        lists.append(seq[:-1] if len(seq) > 1 else [pad_id])
        targets.append(seq[-1] if len(seq) else -1)
    return lists, targets


@torch.no_grad()
def evaluate_unseen(model, item_id_lists, targets, topk=(10,), batch_size: int = 1024,
                    device=None, return_ranks: bool = False):
    """Batched run_with_unseen.evaluate_with_preprocessing.

    item_id_lists: per-user input id sequences (ints in [0, n_items));
    targets: per-user target ids, or -1 / None for a target the dataset does
    not know (such rows are skipped, as the reference's KeyError path does).
    Returns {"hit@k", "ndcg@k", "n_valid"} (+ per-user ranks)."""
    device = device or next(model.parameters()).device
    was_training = model.training
    model.eval()
    n = len(item_id_lists)
    lens = torch.tensor([max(1, len(x)) for x in item_id_lists], dtype=torch.int64)
    tg = torch.tensor([-1 if t is None else int(t) for t in targets], dtype=torch.int64)
    order = torch.argsort(lens, stable=True)
    n_gt = torch.full((n,), -1, dtype=torch.int64)
    n_eq = torch.full((n,), -1, dtype=torch.int64)
    table = model.item_embedding.weight
    for s in range(0, n, batch_size):
        idx = order[s:s + batch_size]
        L = int(lens[idx].max())
        seq = torch.zeros((len(idx), L), dtype=torch.int64)
        for r, u in enumerate(idx.tolist()):
            ids = item_id_lists[u] or [0]
            seq[r, :len(ids)] = torch.as_tensor(ids, dtype=torch.int64)
        seq = seq.to(device)
        ln = lens[idx].to(device)
        t = tg[idx].to(device)
        valid = t >= 1   # id 0 is padding: the reference's token2id(...) - 1 would be -1
        out = model.forward(seq, ln, exact_lengths=True)
        g, e = target_ranks(out, table, torch.where(valid, t, torch.zeros_like(t)), first_item=1)
        g = torch.where(valid, g, torch.full_like(g, -1))
        e = torch.where(valid, e, torch.full_like(e, -1))
        n_gt[idx] = g.cpu()
        n_eq[idx] = e.cpu()
    model.train(was_training)
    res = {}
    avg = rank_metrics(n_gt, n_eq, topk=topk, ties="average")
    opt = rank_metrics(n_gt, n_eq, topk=topk, ties="optimistic")
    for k in topk:
        res[f"hit@{k}"] = opt[f"hit@{k}"]
        res[f"ndcg@{k}"] = avg[f"ndcg@{k}"]
    res["n_valid"] = int((n_gt >= 0).sum())
    if return_ranks:
        res["n_greater"], res["n_equal"] = n_gt, n_eq
    return res


@torch.no_grad()
def full_sort_metrics(model, batches, topk=(10, 20), allow=None, allow_rows_key=None,
                      prior=None, prior_rows_key=None, prior_weight=None):
    """RecBole full-sort Hit/NDCG/MRR@k over leave-one-out batches
    (interaction dicts with ITEM_SEQ, ITEM_SEQ_LEN and POS_ITEM_ID).  allow
    (scoring.item_filters) ranks each target among the items of a catalogue
    filter only; allow_rows_key names the batches' entry that holds each row's
    filter index (None: filter 0 for every row).  A target that its row's
    filter does not allow is dropped, as an invalid target is.  prior
    (scoring.item_priors) ranks by score + weight * prior[item];
    prior_rows_key names the batches' entry that holds each row's prior index
    (None: prior 0 for every row), and prior_weight is a float (or None: 1.0)
    for all rows.  A target whose adjusted score is NaN is dropped."""
    if prior is None and (prior_rows_key is not None or prior_weight is not None):
        raise ValueError("prior_rows_key / prior_weight without prior")
    was_training = model.training
    model.eval()
    gts, eqs = [], []
    for inter in batches:
        if prior is not None:
            kw = {}
            if allow is not None:
                kw = dict(allow=allow, allow_rows=inter[allow_rows_key]
                          if allow_rows_key is not None else None)
            g, e = model.full_sort_rank(
                inter, prior=prior, prior_weight=prior_weight,
                prior_rows=inter[prior_rows_key] if prior_rows_key is not None else None, **kw)
        elif allow is None:
            g, e = model.full_sort_rank(inter)
        else:
            rows = inter[allow_rows_key] if allow_rows_key is not None else None
            g, e = model.full_sort_rank(inter, allow=allow, allow_rows=rows)
        gts.append(g.cpu())
        eqs.append(e.cpu())
    model.train(was_training)
    return rank_metrics(torch.cat(gts), torch.cat(eqs), topk=topk, ties="optimistic")


@torch.no_grad()
def recommend(model, item_id_lists, k: int = 10, batch_size: int = 1024,
              exclude_seen: bool = True, device=None, allow=None, allow_rows=None,
              groups=None, max_per_group=None, prior=None, prior_rows=None, prior_weight=None):
    """Each user's k best items from their input id sequence.

    item_id_lists: per-user id sequences (ints in [0, n_items)), batched by
    length with ``forward(..., exact_lengths=True)`` as evaluate_unseen does,
    so every row equals its batch-1 forward.  Item 0 (padding) is never
    recommended; exclude_seen also drops the user's own input items.  Returns
    (ids int64 [n, k], scores fp32 [n, k]) on the CPU in the callers' order,
    by (score descending, id ascending), id -1 / score -inf where fewer than k
    items are selectable (scoring.top_items).  The model's train/eval mode is
    left as found.

    allow (scoring.item_filters) restricts every list to a catalogue filter;
    allow_rows [n] names each user's filter in the callers' order (None:
    filter 0 for everyone, -1: no filter for that user) and follows the users
    through the length sort.  groups (scoring.item_groups) and max_per_group
    cap every list at that many items of one group; the groups are per item,
    so the length sort does not touch them.  prior (scoring.item_priors)
    ranks by score + weight * prior[item]: prior_rows [n] names each user's
    prior (None: prior 0 for everyone, -1: none for that user) and prior_weight
    is a float for everyone or a float [n] tensor with each user's strength;
    both are per user, in the callers' order, and follow the users through the
    length sort."""
    device = device or next(model.parameters()).device
    n_users = len(item_id_lists)
    if prior is None and (prior_rows is not None or prior_weight is not None):
        raise ValueError("prior_rows / prior_weight without prior")
    if prior is not None:
        prior = prior.to(device)
    if prior_rows is not None:
        prior_rows = torch.as_tensor(prior_rows, dtype=torch.int64).cpu()
        if prior_rows.shape != (n_users,):
            raise ValueError(f"prior_rows must be [{n_users}], got {tuple(prior_rows.shape)}")
    if isinstance(prior_weight, torch.Tensor):
        prior_weight = prior_weight.detach().to(dtype=torch.float32).cpu()
        if prior_weight.shape != (n_users,):
            raise ValueError(f"a tensor prior_weight must be [{n_users}], got "
                             f"{tuple(prior_weight.shape)}")
    if (groups is None) != (max_per_group is None):
        raise ValueError("groups and max_per_group are given together or not at all")
    if groups is not None:
        groups = groups.to(device)
    if allow_rows is not None:
        if allow is None:
            raise ValueError("allow_rows without allow")
        allow_rows = torch.as_tensor(allow_rows, dtype=torch.int64).cpu()
        if allow_rows.shape != (len(item_id_lists),):
            raise ValueError(f"allow_rows must be [{len(item_id_lists)}], got "
                             f"{tuple(allow_rows.shape)}")
    if allow is not None:
        allow = allow.to(device)
    was_training = model.training
    model.eval()
    n = len(item_id_lists)
    lens = torch.tensor([max(1, len(x)) for x in item_id_lists], dtype=torch.int64)
    order = torch.argsort(lens, stable=True)
    ids = torch.full((n, k), -1, dtype=torch.int64)
    scores = torch.full((n, k), float("-inf"), dtype=torch.float32)
    table = model.item_embedding.weight
    try:
        for s in range(0, n, batch_size):
            idx = order[s:s + batch_size]
            L = int(lens[idx].max())
            seq = torch.zeros((len(idx), L), dtype=torch.int64)
            for r, u in enumerate(idx.tolist()):
                row = item_id_lists[u] or [0]
                seq[r, :len(row)] = torch.as_tensor(row, dtype=torch.int64)
            seq = seq.to(device)
            out = model.forward(seq, lens[idx].to(device), exact_lengths=True)
            pkw = {}
            if prior is not None:
                pkw = dict(prior=prior,
                           prior_rows=prior_rows[idx] if prior_rows is not None else None,
                           prior_weight=prior_weight[idx]
                           if isinstance(prior_weight, torch.Tensor) else prior_weight)
            i, sc = top_items(out, table, k, first_item=1, exclude=seq if exclude_seen else None,
                              allow=allow,
                              allow_rows=allow_rows[idx] if allow_rows is not None else None,
                              groups=groups, max_per_group=max_per_group, **pkw)
            ids[idx] = i.cpu()
            scores[idx] = sc.cpu()
    finally:
        model.train(was_training)
    return ids, scores

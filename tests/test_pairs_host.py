"""The sampled pairwise (BPR) loss of all-position training, host side: the
sampler's host reference (its Philox, the rejection rule, exhaustion), the
torch restatement of the loss, the configuration errors and the loader's
negatives.  No GPU."""
import math

import numpy as np
import pytest
import torch

from datamining_recblr_amd import data as dp, kernels, scoring

from test_dense_host import _cfg, _toy_data

LENGTHS = (1, 12, 7, 3, 12)
L = 12
V = 50
SEED = 0x1234_5678_9ABC_DEF0


def sampler_case(lengths=LENGTHS, seq_len=L, n_items=V, seed=0):
    """item_seq [B, L] right-padded, lengths, pos_items and the packed plan
    (offsets, inv, ntok) as RecBLR.forward_all lays it out."""
    g = torch.Generator().manual_seed(seed)
    B = len(lengths)
    lens = torch.tensor(lengths)
    item_seq = torch.randint(1, n_items, (B, seq_len), generator=g)
    item_seq = item_seq * (torch.arange(seq_len)[None] < lens[:, None])
    pos_items = torch.randint(1, n_items, (B,), generator=g)
    order = torch.argsort(lens, descending=True, stable=True)
    offsets = torch.zeros(B + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(lens[order], 0)
    inv = torch.empty(B, dtype=torch.int64)
    inv[order] = torch.arange(B)
    return item_seq, lens, pos_items, offsets, inv, int(offsets[-1])


def exhaustion_case(n_items):
    """One row of 12 distinct items 1 .. 12 and the target 13: every id of
    [1, 14) is seen."""
    item_seq = torch.arange(1, 13)[None]
    lens, pos = torch.tensor([12]), torch.tensor([13])
    offsets, inv = torch.tensor([0, 12]), torch.tensor([0])
    return item_seq, lens, pos, offsets, inv, 12, n_items


# the seed of the exhaustion cases: at V = 15 (13 of 14 ids seen) it settles
# draws both inside the 16 attempts and by the walk (asserted below)
EXHAUSTION_SEED = 7


def test_philox_matches_the_published_vectors():
    """Random123's known-answer vectors for philox4x32-10."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2,
            (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = kernels.philox4x32_10([np.array([c]) for c in ctr], key)
        assert tuple(int(w[0]) for w in got) == want
    # vectorised: each element is its own counter
    ctrs = [np.array([k[0][i] for k in kat]) for i in range(4)]
    got = kernels.philox4x32_10(ctrs, kat[0][1])
    assert tuple(int(w[0]) for w in got) == kat[0][2]


@pytest.mark.parametrize("n", [1, 3])
def test_reference_sampler_properties(n):
    item_seq, lens, pos, offsets, inv, ntok = sampler_case()
    stats = {}
    dense = kernels.sample_negatives_reference(item_seq, lens, pos, n, 1, V, SEED, offsets, inv,
                                               ntok, stats=stats)
    assert dense.shape == (ntok, n) and dense.dtype == torch.int64
    assert stats["attempts"] + stats["walk"] == ntok * n and stats["exhausted"] == 0
    assert (dense >= 1).all() and (dense < V).all()
    for b in range(len(LENGTHS)):
        seen = set(item_seq[b, :lens[b]].tolist()) | {int(pos[b])}
        r0 = int(offsets[inv[b]])
        assert not seen & set(dense[r0:r0 + int(lens[b])].reshape(-1).tolist())
    # padding rows
    padded = kernels.sample_negatives_reference(item_seq, lens, pos, n, 1, V, SEED, offsets, inv,
                                                ntok, 64)
    assert torch.equal(padded[:ntok], dense) and (padded[ntok:] == -1).all()
    # the last-only call is the dense call's rows at each row's last position
    last = kernels.sample_negatives_reference(item_seq, lens, pos, n, 1, V, SEED)
    assert last.shape == (len(LENGTHS), n)
    assert torch.equal(last, dense[offsets[inv] + lens - 1])
    # another seed draws other ids
    other = kernels.sample_negatives_reference(item_seq, lens, pos, n, 1, V, SEED + 1)
    assert not torch.equal(other, last)
    # a row's draws depend on its batch index b and its content, not on the
    # rest of the batch or on where the packed plan puts it: the batch of
    # rows (1, 12, 7) alone, packed in its own order, gives those rows' ids
    sub = [0, 1, 2]
    lens2 = lens[sub]
    order2 = torch.argsort(lens2, descending=True, stable=True)
    offs2 = torch.zeros(4, dtype=torch.int64)
    offs2[1:] = torch.cumsum(lens2[order2], 0)
    inv2 = torch.empty(3, dtype=torch.int64)
    inv2[order2] = torch.arange(3)
    d2 = kernels.sample_negatives_reference(item_seq[sub], lens2, pos[sub], n, 1, V, SEED, offs2,
                                            inv2, int(offs2[-1]))
    for b in sub:
        a0, c0 = int(offsets[inv[b]]), int(offs2[inv2[b]])
        assert torch.equal(d2[c0:c0 + int(lens[b])], dense[a0:a0 + int(lens[b])])


def test_reference_sampler_exhaustion():
    item_seq, lens, pos, offsets, inv, ntok, _ = exhaustion_case(14)
    stats = {}
    out = kernels.sample_negatives_reference(item_seq, lens, pos, 3, 1, 14, EXHAUSTION_SEED,
                                             offsets, inv, ntok, stats=stats)
    assert (out == -1).all() and stats == {"attempts": 0, "walk": 0, "exhausted": 36}
    stats = {}
    out = kernels.sample_negatives_reference(item_seq, lens, pos, 3, 1, 15, EXHAUSTION_SEED,
                                             offsets, inv, ntok, stats=stats)
    assert (out == 14).all()                      # the single free id, for every draw
    assert stats["attempts"] > 0 and stats["walk"] > 0 and stats["exhausted"] == 0
    assert stats["attempts"] + stats["walk"] == 36


def pair_loss_by_hand(h, table, pos, neg, gamma):
    """The formula in fp64, pair by pair."""
    total, live = 0.0, 0
    for r in range(h.shape[0]):
        if pos[r] < 0:
            continue
        for j in range(neg.shape[1]):
            if neg[r, j] < 0:
                continue
            x = float(h[r].double() @ table[pos[r]].double()
                      - h[r].double() @ table[neg[r, j]].double())
            total += -math.log(gamma + 1.0 / (1.0 + math.exp(-x)))
            live += 1
    return total / max(live, 1), live


def test_pair_loss_reference_is_the_formula():
    g = torch.Generator().manual_seed(2)
    M, Vt, d, n = 23, 31, 24, 3
    h = torch.randn(M, d, generator=g, dtype=torch.float64)
    tab = torch.randn(Vt, d, generator=g, dtype=torch.float64)
    pos = torch.randint(0, Vt, (M,), generator=g)
    neg = torch.randint(0, Vt, (M, n), generator=g)
    pos[[0, 7]] = -1
    neg[3, 1] = neg[22, 2] = -1
    want, live = pair_loss_by_hand(h, tab, pos, neg, 1e-10)
    assert live == (M - 2) * n - 2
    hh, tt = h.clone().requires_grad_(), tab.clone().requires_grad_()
    got, n_live = scoring.pair_loss(hh, tt, pos, neg, return_live=True)   # CPU: the reference
    assert abs(float(got.detach()) - want) <= 1e-12 * abs(want) and int(n_live) == live
    got.backward()
    assert (hh.grad[[0, 7]] == 0).all() and torch.isfinite(tt.grad).all()
    # n = 1, all live: RecBole's BPRLoss on the pairs
    from datamining_recblr_amd.recbole_compat import BPRLoss
    p1, n1 = pos.clamp(min=0), neg[:, :1].clamp(min=0)
    bpr = BPRLoss()((h * tab[p1]).sum(-1), (h * tab[n1[:, 0]]).sum(-1))
    assert torch.allclose(scoring.pair_loss_reference(h, tab, p1, n1), bpr, rtol=1e-12, atol=0)
    # an id outside [-1, V) gives NaN; no live pair gives 0 and zero gradients
    bad = pos.clone()
    bad[5] = Vt
    assert torch.isnan(scoring.pair_loss(h, tab, bad, neg))
    hz = h.clone().requires_grad_()
    z = scoring.pair_loss(hz, tab, torch.full_like(pos, -1), neg)
    z.backward()
    assert float(z.detach()) == 0.0 and (hz.grad == 0).all()
    with pytest.raises(ValueError):
        scoring.pair_loss(h, tab, pos, neg[:, :0])
    with pytest.raises(ValueError):
        scoring.pair_loss(h, tab, pos[:-1], neg)


def test_dense_negatives_config():
    from datamining_recblr_amd.model import RecBLR
    from datamining_recblr_amd.recbole_compat import SyntheticDataset

    ds = SyntheticDataset(50)
    assert RecBLR(_cfg(), ds).dense_negatives == 0
    m = RecBLR(_cfg(train_all_positions=True, dense_negatives=4), ds)
    assert m.dense_negatives == 4 and m.train_all_positions and m.loss_type == "CE"
    with pytest.raises(ValueError, match="train_all_positions"):
        RecBLR(_cfg(dense_negatives=1), ds)
    with pytest.raises(ValueError, match="dense_negatives"):
        RecBLR(_cfg(train_all_positions=True, dense_negatives=17), ds)
    # the two refusals the dense CE pinned still hold
    with pytest.raises(ValueError, match="train_all_positions"):
        RecBLR(_cfg(train_all_positions=True, loss_type="BPR"), ds)
    with pytest.raises(ValueError, match="train_all_positions"):
        RecBLR(_cfg(train_all_positions=True, loss_type="BPR", dense_negatives=1), ds)
    with pytest.raises(ValueError):
        RecBLR(_cfg(loss_type="BPR"), ds).calculate_loss_dense({})


def test_loader_negatives_on_the_cpu():
    d = _toy_data(5)
    plain = dp.SequentialLoader(d, "train", batch_size=4, shuffle=False)
    assert all("neg_item_id" not in b for b in plain)
    loader = dp.SequentialLoader(d, "train", batch_size=4, shuffle=False, negatives=True)
    seen_any = []
    for batch in loader:
        seq, n, tgt, neg = (batch[k] for k in ("item_id_list", "item_length", "item_id",
                                               "neg_item_id"))
        assert neg.shape == tgt.shape and neg.dtype == torch.int64
        for r in range(seq.shape[0]):
            seen = set(seq[r, :n[r]].tolist()) | {int(tgt[r])}
            assert 1 <= int(neg[r]) < d.n_items and int(neg[r]) not in seen
        seen_any.append(neg)
    # reproducible from (seed, epoch, batch); another epoch draws again
    again = [b["neg_item_id"] for b in loader]
    assert all(torch.equal(a, b) for a, b in zip(seen_any, again))
    loader.set_epoch(1)
    assert any(not torch.equal(a, b["neg_item_id"]) for a, b in zip(seen_any, loader))

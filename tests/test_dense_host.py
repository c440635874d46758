"""All-position ("dense") training, host side: the per-position targets'
torch restatement, the dense loader's rows, the torch path of
item_cross_entropy_rows and the configuration errors.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from datamining_recblr_amd import _lib, data as dp, kernels, scoring

LENS = [1, 2, 7, 12, 12]
L = 12


def packed_case(lens=LENS, seq_len=L, n_items=77, seed=0):
    """item_seq [B, L] right-padded, pos_items [B] and the packed plan
    (ids, offsets, order) as RecBLR._forward_packed lays it out."""
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    lengths = torch.tensor(lens)
    item_seq = torch.randint(1, n_items, (B, seq_len), generator=g)
    item_seq = item_seq * (torch.arange(seq_len)[None] < lengths[:, None])
    pos_items = torch.randint(1, n_items, (B,), generator=g)
    order = torch.argsort(lengths, descending=True, stable=True)
    offsets = torch.zeros(B + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(lengths[order], 0)
    ids = torch.cat([item_seq[b, :lengths[b]] for b in order.tolist()])
    return item_seq, lengths, pos_items, ids, offsets, order


def targets_by_hand(item_seq, lengths, pos_items, order, m_pad):
    out = []
    for b in order.tolist():
        n = int(lengths[b])
        for t in range(n):
            out.append(int(item_seq[b, t + 1]) if t + 1 < n else int(pos_items[b]))
    return torch.tensor(out + [-1] * (m_pad - len(out)))


def test_next_item_targets_reference_matches_loop():
    item_seq, lengths, pos_items, ids, offsets, order = packed_case()
    assert ids.numel() == sum(LENS) == 34
    for m_pad in (34, 256):
        got = kernels.next_item_targets_reference(ids, offsets, order, pos_items, m_pad)
        want = targets_by_hand(item_seq, lengths, pos_items, order, m_pad)
        assert got.dtype == torch.int64 and torch.equal(got, want)
    assert torch.equal(kernels.next_item_targets_reference(ids, offsets, order, pos_items),
                       targets_by_hand(item_seq, lengths, pos_items, order, 34))


def test_dense_header_is_bound_with_the_product_library():
    names = {"rb_next_item_targets", "rb_item_ce_fwd_h_rows", "rb_item_ce_probs_h_rows",
             "rb_item_ce_probs_h_both_rows"}
    assert set(_lib.DENSE_SIGNATURES) == names
    assert not names & set(_lib.SIGNATURES)
    lib = _lib.load()
    f32, i64, p = ctypes.c_float, ctypes.c_int64, ctypes.c_void_p
    assert lib.rb_next_item_targets.argtypes == [p, p, p, p, i64, i64, i64, p, p]
    assert lib.rb_item_ce_probs_h_rows.argtypes[7] is f32
    # argument errors come back before any HIP call
    assert lib.rb_next_item_targets(16, 16, 16, 16, 4, 10, 8, 16, None) == _lib.RB_EINVAL
    assert b"m_pad" in lib.rb_last_error_string()
    assert lib.rb_item_ce_fwd_h_rows(16, 16, 16, 16, 16, 256, 8, 128, 0.0, 0, 16, 16, 16, 1 << 20,
                                     None) == _lib.RB_EINVAL
    assert b"inv_n" in lib.rb_last_error_string()
    assert lib.rb_item_ce_probs_h_both_rows(16, 16, 16, 16, 16, 16, 16, 2.0, 256, 8, 128, 0, 16, 8,
                                            16, 256, 16, 16, None) == _lib.RB_EINVAL
    assert {"rb_item_ce_fwd_h_rows", "rb_item_ce_probs_h_rows",
            "rb_item_ce_probs_h_both_rows"} <= set(kernels.FLOP_KERNELS)


def _toy_data(max_len):
    # users with 2, 3, 6 and 15 interactions: 1, 1, 3 and 12 train samples
    counts = {"a": 2, "b": 3, "c": 6, "d": 15}
    users = np.array(sum(([u] * n for u, n in counts.items()), []), dtype=object)
    g = np.random.default_rng(3)
    items = np.array([f"i{x}" for x in g.integers(0, 9, len(users))], dtype=object)
    cols = {"user_id": users, "item_id": items,
            "timestamp": np.arange(len(users), dtype=np.float64)}
    return dp.build_sequential(cols, max_len=max_len, min_user=1, min_item=1)


def test_dense_loader_rows_cover_exactly_the_train_samples():
    max_len = 5
    d = _toy_data(max_len)
    assert d.train.shape[0] == 1 + 1 + 3 + 12
    rows = dp.dense_windows(d.train, max_len)
    # user d: 12 train targets in windows of 5 counted from the end: 2 + 5 + 5
    s = int(d.train[-1, 0])
    t_last = int(d.train[-1, 1])
    assert t_last - s == 12
    assert [tuple(r) for r in rows.tolist() if r[0] >= s] == [
        (s, s + 2), (s + 2, s + 7), (s + 7, s + 12)]
    assert rows.shape[0] == 1 + 1 + 1 + 3

    loader = dp.SequentialLoader(d, "train", batch_size=4, shuffle=False, dense=True)
    assert len(loader) == 2 and torch.equal(loader.desc, rows)
    covered, i = [], 0
    for batch in loader:
        seq, n, tgt = batch["item_id_list"], batch["item_length"], batch["item_id"]
        assert seq.shape[1] == max_len
        assert torch.equal(getattr(n, "_recblr_host_lengths"), n.cpu())
        for r in range(seq.shape[0]):
            w0, t = rows[i].tolist()
            i += 1
            k = int(n[r])
            assert k == t - w0 <= max_len
            assert seq[r, :k].tolist() == d.items[w0:t].tolist() and (seq[r, k:] == 0).all()
            assert int(tgt[r]) == int(d.items[t])
            covered += [w0 + p + 1 for p in range(k)]   # position p trains on target w0 + p + 1
    assert i == rows.shape[0]
    assert sorted(covered) == sorted(d.train[:, 1].tolist())
    shuffled = dp.SequentialLoader(d, "train", batch_size=4, shuffle=True, seed=5, dense=True)
    assert sum(int(b["item_length"].sum()) for b in shuffled) == d.train.shape[0]
    with pytest.raises(ValueError):
        dp.SequentialLoader(d, "valid", dense=True)


def test_rows_ce_torch_path_equals_cross_entropy_with_ignore_index():
    g = torch.Generator().manual_seed(1)
    M, V, d = 23, 31, 24                      # d outside ITEM_DIMS, CPU: the torch path
    seq = torch.randn(M, d, generator=g, dtype=torch.float64)
    tab = torch.randn(V, d, generator=g, dtype=torch.float64)
    tgt = torch.randint(0, V, (M,), generator=g)
    tgt[[0, 1, 11, M - 1]] = -1
    s1, w1 = seq.clone().requires_grad_(), tab.clone().requires_grad_()
    s2, w2 = seq.clone().requires_grad_(), tab.clone().requires_grad_()
    a = scoring.item_cross_entropy_rows(s1, w1, tgt, chunk_rows=256)
    b = F.cross_entropy(s2 @ w2.t(), tgt, ignore_index=-1)
    a.backward()
    b.backward()
    assert torch.equal(a, b) and torch.equal(s1.grad, s2.grad) and torch.equal(w1.grad, w2.grad)
    assert (s1.grad[[0, 1, 11, M - 1]] == 0).all()
    # the host-known live count gives the same result
    a2 = scoring.item_cross_entropy_rows(seq, tab, tgt, n_live=M - 4)
    assert torch.equal(a2, b.detach())
    # no live row: 0 and zero gradients
    s3 = seq.clone().requires_grad_()
    z = scoring.item_cross_entropy_rows(s3, tab, torch.full((M,), -1))
    z.backward()
    assert float(z.detach()) == 0.0 and (s3.grad == 0).all()
    for bad in (0, 100, 257):
        with pytest.raises(ValueError):
            scoring.item_cross_entropy_rows(seq, tab, tgt, chunk_rows=bad)


def _cfg(**kw):
    cfg = dict(hidden_size=32, loss_type="CE", num_layers=1, dropout_prob=0.0, expand=2,
               d_conv=4, bd_lru_only=False, disable_conv1d=False, disable_ffn=False,
               MAX_ITEM_LIST_LENGTH=12)
    cfg.update(kw)
    return cfg


def test_train_all_positions_config():
    from datamining_recblr_amd.model import RecBLR
    from datamining_recblr_amd.recbole_compat import SyntheticDataset

    assert RecBLR(_cfg(), SyntheticDataset(50)).train_all_positions is False
    assert RecBLR(_cfg(train_all_positions=True), SyntheticDataset(50)).train_all_positions is True
    with pytest.raises(ValueError, match="train_all_positions"):
        RecBLR(_cfg(train_all_positions=True, loss_type="BPR"), SyntheticDataset(50))
    m = RecBLR(_cfg(loss_type="BPR"), SyntheticDataset(50))
    with pytest.raises(ValueError):
        m.calculate_loss_dense({})


def test_fit_dense_needs_the_model_switch():
    from datamining_recblr_amd import trainer
    from datamining_recblr_amd.model import RecBLR
    from datamining_recblr_amd.recbole_compat import SyntheticDataset

    with pytest.raises(ValueError, match="train_all_positions"):
        trainer.fit(RecBLR(_cfg(), SyntheticDataset(50)), None, None, dense=True)

"""The sampled pairwise (BPR) loss of all-position training on the GPU: the
sampler against its host reference bit for bit, the loss kernels against fp64,
the table gradient against the plain embedding backward bit for bit, the
equivalence that justifies the feature — calculate_loss_pairs on a batch
equals the reference's BPR calculate_loss on the batch expanded to one row
per prefix — and training through trainer.fit.

Tolerance: every comparison with a reference is max |got - ref| <= 1e-4 * max
|ref| (tests/test_gpu_dense.py's bar)."""
import math

import numpy as np
import pytest
import torch

from test_dense_host import L, LENS, packed_case
from test_gpu_dense import N_ITEMS, _batches, close
from test_pairs_host import (EXHAUSTION_SEED, LENGTHS, SEED, V, exhaustion_case, sampler_case)

pytestmark = pytest.mark.gpu

GAMMA = 1e-10


# ---- 1. the sampler ------------------------------------------------------------------
def _sample_both(case, n, first, num_items, seed, cuda, m_pad=None):
    from datamining_recblr_amd import kernels

    item_seq, lens, pos, offsets, inv, ntok = case
    dev = [t.to(cuda) for t in (item_seq, lens, pos, offsets, inv)]
    ref_d = kernels.sample_negatives_reference(item_seq, lens, pos, n, first, num_items, seed,
                                               offsets, inv, ntok, m_pad)
    ref_l = kernels.sample_negatives_reference(item_seq, lens, pos, n, first, num_items, seed)
    got_d = kernels.sample_negatives(dev[0], dev[1], dev[2], n, first, num_items, seed, dev[3],
                                     dev[4], ntok, m_pad)
    got_l = kernels.sample_negatives(dev[0], dev[1], dev[2], n, first, num_items, seed)
    again = kernels.sample_negatives(dev[0], dev[1], dev[2], n, first, num_items, seed, dev[3],
                                     dev[4], ntok, m_pad)
    assert got_d.dtype == torch.int64 and torch.equal(got_d, again)
    assert torch.equal(got_d.cpu(), ref_d), (got_d.cpu(), ref_d)
    assert torch.equal(got_l.cpu(), ref_l), (got_l.cpu(), ref_l)
    return got_d, got_l


@pytest.mark.parametrize("n", [1, 3])
def test_sampler_equals_host_reference(cuda, n):
    case = sampler_case()
    ntok = case[-1]
    got_d, got_l = _sample_both(case, n, 1, V, SEED, cuda, m_pad=64)
    assert got_d.shape == (64, n) and (got_d[ntok:] == -1).all() and (got_d[:ntok] >= 1).all()
    offsets, inv, lens = case[3].to(cuda), case[4].to(cuda), case[1].to(cuda)
    assert torch.equal(got_l, got_d[offsets[inv] + lens - 1])
    _sample_both(case, n, 1, V, SEED, cuda)                      # m_pad = ntok
    # 300 positions of one row: more draws than the workgroup has threads
    long_case = sampler_case(lengths=(300, 2), seq_len=300, n_items=400, seed=1)
    _sample_both(long_case, n, 1, 400, SEED + 3, cuda)


def test_sampler_exhaustion(cuda):
    *case, _ = exhaustion_case(14)
    got_d, got_l = _sample_both(tuple(case), 3, 1, 14, EXHAUSTION_SEED, cuda)
    assert (got_d == -1).all() and (got_l == -1).all()
    got_d, _ = _sample_both(tuple(case), 3, 1, 15, EXHAUSTION_SEED, cuda)   # attempts and the walk
    assert (got_d == 14).all()


# ---- 2. the loss against fp64 --------------------------------------------------------
def _case(M, Vt, d, n, cuda, seed, ignored_rows=(), ignored_pairs=(), one_negative=None):
    g = torch.Generator().manual_seed(seed)
    h = (0.5 * torch.randn(M, d, generator=g)).to(cuda)
    tab = (0.5 * torch.randn(Vt, d, generator=g)).to(cuda)
    pos = torch.randint(0, Vt, (M,), generator=g)
    neg = torch.randint(0, Vt, (M, n), generator=g)
    if one_negative is not None:
        neg[:] = one_negative
    pos[list(ignored_rows)] = -1
    for r, j in ignored_pairs:
        neg[r, j] = -1
    return h, tab, pos.to(cuda), neg.to(cuda)


def _run(h, tab, pos, neg, scale=0.7):
    from datamining_recblr_amd import scoring

    hh, tt = h.detach().requires_grad_(), tab.clone().requires_grad_()
    loss, n_live = scoring.pair_loss(hh, tt, pos, neg, GAMMA, return_live=True)
    (scale * loss).backward()
    return loss.detach(), hh.grad, tt.grad, int(n_live)


def _ref64(h, tab, pos, neg, scale=0.7):
    hh, tt = h.double().detach().requires_grad_(), tab.double().requires_grad_()
    live = (pos >= 0)[:, None] & (neg >= 0)
    ps = (hh * tt[pos.clamp(min=0)]).sum(-1)
    ns = (hh[:, None, :] * tt[neg.clamp(min=0)]).sum(-1)
    l = -torch.log(GAMMA + torch.sigmoid(ps[:, None] - ns))
    loss = torch.where(live, l, torch.zeros_like(l)).sum() / live.sum().clamp(min=1)
    (scale * loss).backward()
    return loss.detach(), hh.grad, tt.grad, int(live.sum())


def _check(h, tab, pos, neg, scale=0.7):
    with_kernels = []
    from datamining_recblr_amd import kernels
    with kernels.kernel_timing() as t:
        loss, dh, dt, n_live = _run(h, tab, pos, neg, scale)
    with_kernels = [r[0] for r in t.records]
    assert with_kernels == ["rb_pair_loss_fwd", "rb_pair_loss_bwd", "rb_embedding_bwd_scaled"], \
        with_kernels
    rl, rh, rt, rn = _ref64(h, tab, pos, neg, scale)
    assert n_live == rn
    assert torch.isfinite(loss) and torch.isfinite(dh).all() and torch.isfinite(dt).all()
    close(loss, rl, "loss")
    close(dh, rh, "dh")
    close(dt, rt, "dtable")
    return loss, dh, dt


@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("d", [128, 64, 16])
def test_pair_loss_vs_fp64(cuda, d, n):
    """M = 300: five workgroups of 64 rows, the last one partly filled; V = 77."""
    _check(*_case(300, N_ITEMS, d, n, cuda, 3))


def test_pair_loss_other_widths(cuda):
    """Every load count per lane (d <= 64, 128, 256, 512) and widths that are
    no multiple of 64."""
    for d in (4, 36, 200, 256, 388, 512):
        _check(*_case(70, N_ITEMS, d, 2, cuda, 4 + d))


@pytest.mark.parametrize("d", [128, 16])
def test_pair_loss_ignored_rows_and_pairs(cuda, d):
    rows = (0, 15, 16, 63, 64, 299)
    pairs = ((1, 0), (1, 3), (17, 2), (298, 1))
    h, tab, pos, neg = _case(300, N_ITEMS, d, 4, cuda, 5, rows, pairs)
    loss, dh, dt = _check(h, tab, pos, neg)
    assert (dh[list(rows)] == 0).all()
    # an ignored row's values change no output bit
    h2 = h.clone()
    h2[list(rows)] = 37.5 * torch.randn(len(rows), d, device=cuda)
    loss2, dh2, dt2, _ = _run(h2, tab, pos, neg)
    assert torch.equal(loss, loss2) and torch.equal(dh, dh2) and torch.equal(dt, dt2)
    # a row whose pairs are all ignored: zeros too
    neg3 = neg.clone()
    neg3[5] = -1
    assert (_run(h, tab, pos, neg3)[1][5] == 0).all()
    # a pos of V (and any id outside [-1, V)) gives NaN
    bad = pos.clone()
    bad[7] = N_ITEMS
    assert torch.isnan(_run(h, tab, bad, neg)[0])
    badn = neg.clone()
    badn[9, 2] = -2
    assert torch.isnan(_run(h, tab, pos, badn)[0])
    # no live pair: loss 0 and zero gradients
    z, dz, dtz, nz = _run(h, tab, torch.full_like(pos, -1), neg)
    assert float(z) == 0.0 and nz == 0 and (dz == 0).all() and (dtz == 0).all()


def test_pair_loss_one_negative_id_one_row_strided_rows(cuda):
    # every negative is id 5: one key with 300 * 4 positions, 19 chunks of 64
    _check(*_case(300, N_ITEMS, 128, 4, cuda, 6, one_negative=5))
    # M = 1
    _check(*_case(1, N_ITEMS, 64, 3, cuda, 7))
    # h a view with a row stride of d + 4 (read in place), and of d + 3 (copied)
    for extra in (4, 3):
        h, tab, pos, neg = _case(300, N_ITEMS, 64, 2, cuda, 8, (2,), ((3, 1),))
        wide = torch.zeros(300, 64 + extra, device=cuda)
        wide[:, :64] = h
        a = _check(wide[:, :64], tab, pos, neg)
        b = _run(h, tab, pos, neg)
        assert all(torch.equal(x, y) for x, y in zip(a, b[:3]))


def test_pair_loss_refused_width_takes_the_torch_path(cuda):
    from datamining_recblr_amd import kernels, scoring

    h, tab, pos, neg = _case(40, N_ITEMS, 30, 2, cuda, 9, (1,))
    assert not kernels.pair_loss_supported(h, tab)
    lib = kernels._lib.load()
    assert lib.rb_pair_loss_fwd(16, 32, 16, 16, 16, 40, 30, N_ITEMS, 2, 1e-10, 16, 16, 16, 16,
                                1 << 20, None) == kernels._lib.RB_EINVAL
    with kernels.kernel_timing() as t:
        loss = scoring.pair_loss(h, tab, pos, neg)
    assert not t.records
    close(loss, _ref64(h, tab, pos, neg)[0], "loss (torch path)")


@pytest.mark.parametrize("d", [4, 68, 132, 260])
def test_pair_diff_is_the_candidate_scores_difference_bit_for_bit(cuda, d):
    """The pairwise loss and the candidate kernels score a pair with one
    function (csrc/row_group.h): diff = score(pos) - score(neg) of
    rb_candidate_scores, one exact fp32 subtraction on both sides, so the
    comparison is of bits.  One d per count of 16-B loads per lane (1, 2, 4,
    8), each with lanes past d that load zeros; M = 70: two workgroups, the
    second partly empty; h read in place through a row stride of d + 4."""
    from datamining_recblr_amd import kernels

    M, Vt, n = 70, 50, 3
    h, tab, pos, neg = _case(M, Vt, d, n, cuda, 20 + d, (9,), ((33, 1),))
    wide = torch.zeros(M, d + 4, device=cuda)
    wide[:, :d] = h
    _, _, diff = kernels.pair_loss_fwd(wide[:, :d], tab, pos, neg, GAMMA)
    scores = kernels.candidate_scores(wide[:, :d], tab, torch.cat([pos[:, None], neg], 1))
    live = (pos >= 0)[:, None] & (neg >= 0)
    assert int(live.sum()) == M * n - n - 1
    assert torch.equal(diff[live], (scores[:, :1] - scores[:, 1:])[live])
    assert (diff[9] == 0).all() and diff[33, 1] == 0 and (diff[live] != 0).any()


def test_pair_loss_mean_over_more_than_256_workgroups(cuda):
    """258 workgroups: the last one to arrive re-reads the partials with a
    stride of 256, so its loop takes a second step.  The reference is the fp64
    mean of the per-pair terms of the kernel's own diff."""
    from datamining_recblr_amd import kernels

    M = 64 * 257 + 3
    h, tab, pos, neg = _case(M, 8, 4, 1, cuda, 13, (0, 64 * 256, M - 1), ((5, 0), (64 * 257, 0)))
    loss, n_live, diff = kernels.pair_loss_fwd(h, tab, pos, neg, GAMMA)
    again = kernels.pair_loss_fwd(h, tab, pos, neg, GAMMA)
    live = (pos >= 0)[:, None] & (neg >= 0)
    assert int(n_live) == int(live.sum()) == M - 5
    assert torch.equal(loss, again[0]) and torch.equal(n_live, again[1])
    terms = -torch.log(GAMMA + torch.sigmoid(diff.double()))
    close(loss, terms[live].mean(), "loss")


# ---- 3. saturation -------------------------------------------------------------------
def test_pair_loss_saturated(cuda):
    """|x| in [100, 104] on both signs: h_r = x_r (E[pos] - E[neg]) / |E[pos] -
    E[neg]|^2.  sigmoid(-100) = 3.7e-44 is below fp32's normal range: the loss
    there is -log(gamma), and the coefficient -s / (gamma + s) = -3.7e-34
    must keep its accuracy (at +100 it is e^-100 of that, i.e. 0 at the bar).
    The upstream gradient is 1024 so that the reference gradients (1e-34 *
    1024 / M times entries of E and h) stay in fp32's normal range: the test
    measures the kernel's arithmetic, not fp32 underflow of the result."""
    M, d = 96, 128
    h, tab, pos, neg = _case(M, N_ITEMS, d, 1, cuda, 10)
    neg[:, 0] = (pos + 1 + torch.arange(M, device=cuda) % 5) % N_ITEMS   # never the target
    delta = (tab[pos] - tab[neg[:, 0]]).double()
    x = torch.linspace(100.0, 104.0, M, device=cuda, dtype=torch.float64)
    x = x * (1 - 2 * (torch.arange(M, device=cuda) % 2))
    h = (x[:, None] * delta / (delta * delta).sum(-1, keepdim=True)).float()
    got = (h.double() * delta).sum(-1)
    assert (got.abs() >= 99.9).all() and (got > 0).sum() == M // 2
    loss, dh, dt = _check(h, tab, pos, neg, scale=1024.0)
    assert abs(float(loss) - 0.5 * -math.log(GAMMA)) < 1e-3


# ---- 4. the table gradient -----------------------------------------------------------
@pytest.mark.parametrize("Vt,d", [(N_ITEMS, 128), (N_ITEMS, 36), (20000, 16)])
def test_table_gradient_is_bitwise_the_embedding_backward(cuda, Vt, d):
    """rb_embedding_bwd_apply_scaled == rb_embedding_bwd on the materialised
    rows coef[p] * h[p mod M] (fp32, torch), -1 ids included; V = 77 plans by
    the counting sort, V = 20000 by the radix sort."""
    from datamining_recblr_amd import kernels

    M, n = 300, 4
    h, tab, pos, neg = _case(M, Vt, d, n, cuda, 11, (0, 17, 299), ((1, 0), (2, 3)))
    neg[40:140, 1] = 3                       # a key with more than one chunk of 64
    loss, n_live, diff = kernels.pair_loss_fwd(h, tab, pos, neg, GAMMA)
    dloss = torch.tensor(0.7, device=cuda)
    dh, coef = kernels.pair_loss_bwd(tab, pos, neg, diff, dloss, n_live, GAMMA)
    assert coef.shape == ((1 + n) * M,)
    assert (coef[:M][[0, 17, 299]] == 0).all() and coef[M + 1] == 0 and coef[4 * M + 2] == 0
    ids = torch.cat([pos, neg.t().reshape(-1)])
    plan = kernels.embedding_plan(ids, Vt, d)
    got = kernels.embedding_bwd_scaled(coef, h, Vt, plan)
    rows = coef[:, None] * h.repeat(1 + n, 1)
    want = kernels.embedding_bwd(ids, rows, Vt, padding_idx=None)
    assert torch.equal(got, want)
    assert torch.equal(got, kernels.embedding_bwd_scaled(coef, h, Vt, plan))
    live = ids >= 0
    ref = torch.zeros(Vt, d, device=cuda, dtype=torch.float64)
    ref.index_add_(0, ids[live], rows[live].double())
    close(got, ref, "dtable vs index_add in fp64")
    # and through the autograd function, run to run
    a, b = _run(h, tab, pos, neg), _run(h, tab, pos, neg)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
    assert torch.equal(a[2], got)


# ---- 5. the equivalence ----------------------------------------------------------------
def _model(cuda, packed=True, **kw):
    from datamining_recblr_amd.model import RecBLR
    from datamining_recblr_amd.recbole_compat import SyntheticDataset

    cfg = dict(hidden_size=128, loss_type="CE", num_layers=2, dropout_prob=0.0, expand=2,
               d_conv=4, bd_lru_only=False, disable_conv1d=False, disable_ffn=False,
               MAX_ITEM_LIST_LENGTH=L)
    cfg.update(kw)
    torch.manual_seed(11)
    m = RecBLR(cfg, SyntheticDataset(N_ITEMS)).to(cuda)
    m.pack_sequences = packed
    return m


@pytest.mark.parametrize("packed", [True, False])
def test_pairs_loss_equals_bpr_loss_on_expanded_batch(cuda, packed):
    dense_model = _model(cuda, packed, train_all_positions=True, dense_negatives=1).train()
    bpr_model = _model(cuda, packed, loss_type="BPR").train()
    bpr_model.load_state_dict(dense_model.state_dict())
    dense, expanded = _batches(cuda)
    order = packed_case(n_items=N_ITEMS)[5].tolist()
    starts = np.concatenate([[0], np.cumsum(LENS)])
    pick = torch.tensor([starts[b] + t for b in order for t in range(LENS[b])], device=cuda)
    g = torch.Generator().manual_seed(12)
    neg_expanded = torch.randint(1, N_ITEMS, (34,), generator=g).to(cuda)   # batch-row order
    expanded = dict(expanded, neg_item_id=neg_expanded)

    ref = bpr_model.calculate_loss(expanded)
    ref.backward()
    loss = dense_model.calculate_loss_pairs(dense, neg_expanded[pick][:, None])
    loss.backward()
    close(loss, ref, "loss")
    ref_grads = dict(bpr_model.named_parameters())
    for name, p in dense_model.named_parameters():
        assert p.grad is not None, name
        close(p.grad, ref_grads[name].grad, name)
    # padded negatives ([m_pad, n]) are accepted; the switch routes
    # calculate_loss to sampled negatives: finite, and seeded by torch
    padded = torch.cat([neg_expanded[pick][:, None], torch.full((30, 1), -1, device=cuda)])
    assert torch.equal(dense_model.calculate_loss_pairs(dense, padded).detach(), loss.detach())
    torch.manual_seed(5)
    a = dense_model.calculate_loss(dense).detach()
    torch.manual_seed(5)
    b = dense_model.calculate_loss(dense).detach()
    assert torch.isfinite(a) and torch.equal(a, b) and not torch.equal(a, loss.detach())


# ---- 6. training -----------------------------------------------------------------------
def _train_cfg(**kw):
    cfg = {"hidden_size": 32, "loss_type": "CE", "num_layers": 2, "dropout_prob": 0.1,
           "expand": 2, "d_conv": 4, "bd_lru_only": False, "disable_conv1d": False,
           "disable_ffn": False, "MAX_ITEM_LIST_LENGTH": 20}
    cfg.update(kw)
    return cfg


def test_fit_dense_with_sampled_negatives(cuda, tmp_path):
    from test_gpu_train import _toy_atomic
    from datamining_recblr_amd.distributed import DistEnv
    from datamining_recblr_amd.model import RecBLR
    from datamining_recblr_amd.recbole_compat import SyntheticDataset
    from datamining_recblr_amd.trainer import fit

    d = _toy_atomic(tmp_path, cuda)
    torch.manual_seed(0)
    model = RecBLR(_train_cfg(train_all_positions=True, dense_negatives=1),
                   SyntheticDataset(d.n_items, d.n_users)).to(cuda)
    losses = []
    inner = model.calculate_loss

    def recorded(interaction):
        loss = inner(interaction)
        losses.append(loss.detach())
        return loss

    model.calculate_loss = recorded
    # 400 users, one or two windows each: 7 steps per epoch at 64 rows
    fit(model, d, DistEnv(), epochs=5, batch_size=64, lr=1e-2, log=None, dense=True)
    steps = torch.stack(losses)[:30].cpu()
    assert steps.numel() == 30 and torch.isfinite(steps).all()
    first, last = float(steps[:5].mean()), float(steps[25:].mean())
    print(f"first 5 steps {first:.4f}, steps 26-30 {last:.4f}, ln 2 {math.log(2):.4f}")
    assert last < first and last < math.log(2)


def test_fit_bpr_model_gets_negatives_from_the_loader(cuda, tmp_path):
    from test_gpu_train import _toy_atomic
    from datamining_recblr_amd import data as dp
    from datamining_recblr_amd.distributed import DistEnv
    from datamining_recblr_amd.model import RecBLR
    from datamining_recblr_amd.recbole_compat import SyntheticDataset
    from datamining_recblr_amd.trainer import fit

    d = _toy_atomic(tmp_path, cuda)
    torch.manual_seed(0)
    model = RecBLR(_train_cfg(loss_type="BPR"), SyntheticDataset(d.n_items, d.n_users)).to(cuda)
    res = fit(model, d, DistEnv(), epochs=3, batch_size=512, lr=1e-2, log=None)
    losses = [h["train_loss"] for h in res["history"]]
    assert all(math.isfinite(x) for x in losses) and losses[-1] < losses[0]
    # the loader's device negatives are the host reference's, outside each row
    loader = dp.SequentialLoader(d, "train", batch_size=512, shuffle=False, negatives=True)
    batch = next(iter(loader))
    seq, n, tgt, neg = (batch[k] for k in ("item_id_list", "item_length", "item_id",
                                           "neg_item_id"))
    assert neg.is_cuda and neg.shape == tgt.shape
    assert not ((seq == neg[:, None]) & (torch.arange(seq.shape[1], device=cuda)[None] < n[:, None])
                ).any() and (neg != tgt).all() and (neg >= 1).all() and (neg < d.n_items).all()
    cpu = dp.SequentialLoader(d.to("cpu"), "train", batch_size=512, shuffle=False, negatives=True)
    assert torch.equal(next(iter(cpu))["neg_item_id"], neg.cpu())
    d.to(cuda)

"""Sampled softmax with negatives shared per sequence on the GPU: the kernels
against scoring.shared_softmax_reference in fp64, their rules, run-to-run
bits, the fallback, the model's calculate_loss_sampled and trainer.fit.

Bound of the fp64 comparisons (per compared tensor): the kernels' max error
may be at most 4x the max error of the same reference evaluated in fp32 on the
same inputs (torch's blocked sums against the MFMA's k chain), with a floor of
4 fp32 ulps of the reference's largest magnitude.  Both errors are printed.
The model-level comparison uses tests/test_gpu_dense.py's bar (1e-4 of the
largest reference entry)."""
import math

import pytest
import torch

from test_gpu_dense import close
from test_shared_softmax_host import plan

pytestmark = pytest.mark.gpu

V = 40
LENS = [1, 15, 16, 17, 48]          # tile edges, a one-row sequence, ntok = 97
SHIFT = 0.37
ULPS = 4 * 2.0 ** -23


def _case(d, n, cuda, seed=0, scale=0.5):
    g = torch.Generator().manual_seed(seed + 1000 * d + n)
    offsets, order = plan(LENS)
    M = int(offsets[-1])
    h = scale * torch.randn(M, d, generator=g)
    tab = 0.5 * torch.randn(V, d, generator=g)
    target = torch.randint(0, V, (M,), generator=g)
    neg = torch.randint(0, V, (len(LENS), n), generator=g)
    target[30] = -1                                  # an ignored row inside the 48-row sequence
    b48 = int(order[0])
    neg[b48, 0] = int(target[5])                     # a list holding one of its rows' targets
    if n >= 20:
        neg[b48, 3] = neg[b48, 17]                   # a repeated id
        neg[int(order[1]), 2] = -1                   # dead columns: in the first tile,
        neg[int(order[1]), n - 1] = -1               # and the list's last one
    return [t.to(cuda) for t in (h, tab, target, neg, offsets, order)]


def _grads(fn, h, tab, dtype, scale=0.7):
    hh = h.detach().to(dtype).requires_grad_()
    tt = tab.detach().to(dtype).requires_grad_()
    loss = fn(hh, tt)
    (scale * loss).backward()
    return loss.detach(), hh.grad, tt.grad


def _against_fp64(h, tab, target, neg, offsets, order, shift):
    from datamining_recblr_amd import kernels, scoring

    assert kernels.shared_softmax_supported(h, tab, neg.shape[1])
    ref = lambda a, b: scoring.shared_softmax_reference(a, b, target, neg, offsets, order, shift)
    with kernels.kernel_timing() as t:
        got = _grads(lambda a, b: scoring.shared_softmax_loss(a, b, target, neg, offsets, order,
                                                              shift), h, tab, torch.float32)
    assert [r[0] for r in t.records] == ["rb_shared_softmax_fwd", "rb_shared_softmax_bwd",
                                         "rb_embedding_bwd_scaled", "rb_embedding_bwd"]
    want = _grads(ref, h, tab, torch.float64)
    torch32 = _grads(ref, h, tab, torch.float32)
    for name, a, b, w in zip(("loss", "dh", "dtable"), got, torch32, want):
        assert torch.isfinite(a).all(), name
        err, err32 = (a.double() - w).abs().max().item(), (b.double() - w).abs().max().item()
        top = w.abs().max().item()
        bound = max(4 * err32, ULPS * top)
        print(f"{name}: kernel err {err:.3e}, fp32 torch err {err32:.3e}, max |ref| {top:.3e}, "
              f"bound {bound:.3e}")
        assert err <= bound, f"{name}: {err:.3e} > {bound:.3e}"
    return got


@pytest.mark.parametrize("n", [1, 20, 256])
@pytest.mark.parametrize("d", [64, 128])
def test_kernels_vs_fp64(cuda, d, n):
    h, tab, target, neg, offsets, order = _case(d, n, cuda)
    loss, dh, dt = _against_fp64(h, tab, target, neg, offsets, order, SHIFT)
    assert (dh[30] == 0).all() and (dh[29] != 0).any()          # the ignored row: exact zeros
    if n >= 20:
        # the dead columns' rows of dneg and the ignored row's coefficient: exact zeros
        from datamining_recblr_amd import kernels
        lse = kernels.shared_softmax_fwd(h, tab, target, neg, offsets, order, SHIFT, 48)[2]
        dl = torch.ones((), device=cuda)
        nl = torch.tensor(int((target >= 0).sum()), device=cuda)
        _, coef, dneg = kernels.shared_softmax_bwd(h, tab, target, neg, offsets, order, lse, dl,
                                                   nl, SHIFT, 48)
        b = int(order[1])
        assert (dneg[b, 2] == 0).all() and (dneg[b, n - 1] == 0).all() and (dneg[b, 1] != 0).any()
        assert coef[30] == 0 and coef[29] != 0


def test_kernels_large_scores(cuda):
    """Scores reaching +-80: finite, and the same bound."""
    d, n = 64, 20
    h, tab, target, neg, offsets, order = _case(d, n, cuda, seed=1)
    z = h @ tab.t()
    h = h * (80.0 / z.abs().max())
    assert 79.0 < (h @ tab.t()).abs().max() < 81.0
    _against_fp64(h, tab, target, neg, offsets, order, SHIFT)


def test_rules(cuda):
    from datamining_recblr_amd import scoring

    h, tab, target, neg, offsets, order = _case(64, 20, cuda)
    for bad_t, bad_n in ((V, None), (-2, None), (None, V), (None, -2)):
        t2, n2 = target.clone(), neg.clone()
        if bad_t is not None:
            t2[50] = bad_t
        if bad_n is not None:
            n2[2, 9] = bad_n                        # a column outside the first lanes' group
        assert torch.isnan(scoring.shared_softmax_loss(h, tab, t2, n2, offsets, order, SHIFT))
    none = torch.full_like(target, -1)
    loss, dh, dt = _grads(lambda a, b: scoring.shared_softmax_loss(a, b, none, neg, offsets,
                                                                   order, SHIFT),
                          h, tab, torch.float32)
    assert loss == 0 and (dh == 0).all() and (dt == 0).all()
    # a live row with no live column: loss 0, still counted
    loss, live = scoring.shared_softmax_loss(h, tab, target, torch.full_like(neg, -1), offsets,
                                             order, SHIFT, return_live=True)
    assert loss == 0 and int(live) == int((target >= 0).sum())
    # max_len sizes the launch only: an underestimate gives the same rows
    a = scoring.shared_softmax_loss(h, tab, target, neg, offsets, order, SHIFT, max_len=1)
    b = scoring.shared_softmax_loss(h, tab, target, neg, offsets, order, SHIFT, max_len=4096)
    c = scoring.shared_softmax_loss(h, tab, target, neg, offsets, order, SHIFT)
    assert torch.allclose(a, c, rtol=1e-6) and torch.allclose(b, c, rtol=1e-6)


@pytest.mark.parametrize("n", [20, 256])
def test_two_calls_give_the_same_bits(cuda, n):
    from datamining_recblr_amd import scoring

    h, tab, target, neg, offsets, order = _case(128, n, cuda)
    fn = lambda a, b: scoring.shared_softmax_loss(a, b, target, neg, offsets, order, SHIFT)
    one, two = _grads(fn, h, tab, torch.float32), _grads(fn, h, tab, torch.float32)
    assert all(torch.equal(x, y) for x, y in zip(one, two))


def test_mean_over_more_than_256_workgroups(cuda):
    """260 sequences of one and two rows, a workgroup each: the last one to
    arrive re-reads the partials with a stride of 256, so its loop takes a
    second step.  The reference is the fp64 mean of the kernel's own lse - z0
    over the live rows, under this file's bound."""
    from datamining_recblr_amd import kernels

    B, d = 260, 16
    g = torch.Generator().manual_seed(7)
    offsets, order = plan([1 + b % 2 for b in range(B)])
    M = int(offsets[-1])
    h, tab = 0.5 * torch.randn(M, d, generator=g), 0.5 * torch.randn(V, d, generator=g)
    target = torch.randint(0, V, (M,), generator=g)
    neg = torch.randint(0, V, (B, 1), generator=g)
    target[[0, 200, M - 1]] = -1
    args = [t.to(cuda) for t in (h, tab, target, neg, offsets, order)]
    loss, n_live, lse, z0 = kernels.shared_softmax_fwd(*args, SHIFT, 2)
    again = kernels.shared_softmax_fwd(*args, SHIFT, 2)
    live = args[2] >= 0
    assert int(n_live) == int(live.sum()) == M - 3
    assert torch.equal(loss, again[0]) and torch.equal(n_live, again[1])
    want = (lse.double() - z0.double())[live].mean()
    err, err32 = abs(float(loss) - float(want)), abs(float((lse - z0)[live].mean()) - float(want))
    bound = max(4 * err32, ULPS * abs(float(want)))
    print(f"loss: kernel err {err:.3e}, fp32 torch err {err32:.3e}, ref {float(want):.3e}, "
          f"bound {bound:.3e}")
    assert err <= bound, f"loss: {err:.3e} > {bound:.3e}"


def test_unsupported_shapes_take_the_reference(cuda):
    from datamining_recblr_amd import kernels, scoring

    for d, n in ((20, 8), (64, 300)):
        g = torch.Generator().manual_seed(d)
        offsets, order = (t.to(cuda) for t in plan(LENS))
        M = int(offsets[-1])
        h, tab = torch.randn(M, d, generator=g).to(cuda), torch.randn(V, d, generator=g).to(cuda)
        target = torch.randint(0, V, (M,), generator=g).to(cuda)
        neg = torch.randint(0, V, (len(LENS), n), generator=g).to(cuda)
        assert not kernels.shared_softmax_supported(h, tab, n)
        with kernels.kernel_timing() as t:
            loss = scoring.shared_softmax_loss(h, tab, target, neg, offsets, order, SHIFT)
        assert not t.records
        assert torch.equal(loss, scoring.shared_softmax_reference(h, tab, target, neg, offsets,
                                                                  order, SHIFT))
    assert kernels.shared_softmax_supported(torch.zeros(4, 64, device=cuda),
                                            torch.zeros(9, 64, device=cuda), 256)


# ---- the model -----------------------------------------------------------------------
L, N_ITEMS, N = 24, 77, 20
MODEL_LENS = [24, 1, 9, 17, 24, 3]


def _model(cuda, **kw):
    from datamining_recblr_amd.model import RecBLR
    from datamining_recblr_amd.recbole_compat import SyntheticDataset

    cfg = dict(hidden_size=64, loss_type="CE", num_layers=2, dropout_prob=0.0, expand=2,
               d_conv=4, bd_lru_only=False, disable_conv1d=False, disable_ffn=False,
               MAX_ITEM_LIST_LENGTH=L, train_all_positions=True, dense_loss="sampled_softmax",
               dense_negatives=N)
    cfg.update(kw)
    torch.manual_seed(11)
    return RecBLR(cfg, SyntheticDataset(N_ITEMS)).to(cuda).eval()


def _batch(cuda):
    g = torch.Generator().manual_seed(4)
    lens = torch.tensor(MODEL_LENS)
    seq = torch.randint(1, N_ITEMS, (len(MODEL_LENS), L), generator=g)
    seq = seq * (torch.arange(L)[None] < lens[:, None])
    pos = torch.randint(1, N_ITEMS, (len(MODEL_LENS),), generator=g)
    neg = torch.randint(1, N_ITEMS, (len(MODEL_LENS), N), generator=g)
    inter = {"item_id_list": seq.to(cuda), "item_length": lens.to(cuda), "item_id": pos.to(cuda)}
    return inter, neg.to(cuda)


def test_model_loss_equals_the_reference_on_its_rows(cuda):
    from datamining_recblr_amd import kernels, scoring

    inter, neg = _batch(cuda)
    model, twin = _model(cuda), _model(cuda)
    twin.load_state_dict(model.state_dict())
    loss = model.calculate_loss_sampled(inter, neg)
    loss.backward()
    h, seq = twin.forward_all(inter["item_id_list"], inter["item_length"])
    target = kernels.next_item_targets(seq.ids, seq.offsets, seq.order, inter["item_id"])
    ref = scoring.shared_softmax_reference(h, twin.item_embedding.weight, target, neg,
                                           seq.offsets, seq.order, math.log((N_ITEMS - 1) / N))
    ref.backward()
    close(loss, ref, "loss")
    want = dict(twin.named_parameters())
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        close(p.grad, want[name].grad, name)


def test_model_draws_its_lists_from_torchs_seed(cuda):
    from datamining_recblr_amd import kernels

    inter, _ = _batch(cuda)
    model = _model(cuda)
    torch.manual_seed(5)
    a = model.calculate_loss(inter).detach()
    torch.manual_seed(5)
    b = model.calculate_loss(inter).detach()
    assert torch.isfinite(a) and torch.equal(a, b)
    torch.manual_seed(5)
    seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64))
    cpu = [inter[k].cpu() for k in ("item_id_list", "item_length", "item_id")]
    lists = kernels.sample_negatives_reference(*cpu, N, 1, N_ITEMS, seed)
    assert lists.shape == (len(MODEL_LENS), N)
    drawn = kernels.sample_negatives(inter["item_id_list"], inter["item_length"],
                                     inter["item_id"], N, 1, N_ITEMS, seed)
    assert torch.equal(drawn.cpu(), lists)
    assert torch.equal(model.calculate_loss_sampled(inter, lists.to(cuda)).detach(), a)


def test_fit_dense_with_the_sampled_softmax(cuda, tmp_path):
    from test_gpu_train import _toy_atomic
    from datamining_recblr_amd.distributed import DistEnv
    from datamining_recblr_amd.model import RecBLR
    from datamining_recblr_amd.recbole_compat import SyntheticDataset
    from datamining_recblr_amd.trainer import fit

    d = _toy_atomic(tmp_path, cuda)
    torch.manual_seed(0)
    cfg = {"hidden_size": 32, "loss_type": "CE", "num_layers": 2, "dropout_prob": 0.1,
           "expand": 2, "d_conv": 4, "bd_lru_only": False, "disable_conv1d": False,
           "disable_ffn": False, "MAX_ITEM_LIST_LENGTH": 20, "train_all_positions": True,
           "dense_loss": "sampled_softmax", "dense_negatives": 32}
    model = RecBLR(cfg, SyntheticDataset(d.n_items, d.n_users)).to(cuda)
    res = fit(model, d, DistEnv(), epochs=2, batch_size=64, lr=1e-2, log=None, dense=True)
    losses = [h["train_loss"] for h in res["history"]]
    print("train loss per epoch", losses)
    assert len(losses) == 2 and all(math.isfinite(x) for x in losses) and losses[1] < losses[0]

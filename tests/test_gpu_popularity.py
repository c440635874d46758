"""Popularity-weighted negative sampling on the GPU: the alias sampler against
its host reference id for id, the sampled softmax kernels with the per-item
log-Q term against scoring.shared_softmax_reference in fp64, their launch
names and run-to-run bits, the model's two sampled losses and trainer.fit.

Bound of the fp64 comparisons (tests/test_gpu_shared_softmax.py's, per compared
tensor): the kernels' max error may be at most 4x the max error of the same
reference evaluated in fp32 on the same inputs, with a floor of 4 fp32 ulps of
the reference's largest magnitude.  Both errors are printed.  The model-level
comparison uses tests/test_gpu_dense.py's bar."""
import math

import pytest
import torch

from test_gpu_dense import close
from test_gpu_shared_softmax import LENS, SHIFT, ULPS, V, _case, _grads
from test_popularity_sampler_host import (FIRST_HIGH, FREQ_SEED, N, SEED, check_frequencies,
                                          counts, frequency_case, sampler_rows)

pytestmark = pytest.mark.gpu

ITEM_NAMES = ["rb_shared_softmax_fwd_items", "rb_shared_softmax_bwd_items",
              "rb_embedding_bwd_scaled", "rb_embedding_bwd"]
PLAIN_NAMES = ["rb_shared_softmax_fwd", "rb_shared_softmax_bwd", "rb_embedding_bwd_scaled",
               "rb_embedding_bwd"]


def _item_shift(cuda):
    """-log(q) of a skewed table over all 40 ids (the kernels' case draws its
    ids from [0, V)): about 0.5 for the heavy item to 8 for the items without
    a count."""
    from datamining_recblr_amd import kernels

    skewed = counts() * 6
    skewed[4] = 22000
    shift = kernels.negative_sampler(skewed, first_item=0).item_shift
    assert shift.shape == (V,) and 0.4 < float(shift.min()) < 0.7 and 7.5 < float(shift.max()) < 8.5
    return shift.to(cuda)


# ---- the sampler -----------------------------------------------------------------------
@pytest.mark.parametrize("first", [1, FIRST_HIGH])
def test_sampler_equals_the_host_reference(cuda, first):
    from datamining_recblr_amd import kernels

    item_seq, lens, pos, offsets, inv, ntok = sampler_rows()
    dev = [t.to(cuda) for t in (item_seq, lens, pos, offsets, inv)]
    table = kernels.negative_sampler(counts(), first_item=first)
    alias = table.alias.to(cuda)
    m_pad = 32
    for plan_h, plan_d in (((), ()), ((offsets, inv, ntok, m_pad), (*dev[3:], ntok, m_pad))):
        want = kernels.sample_negatives_reference(item_seq, lens, pos, N, first, V, SEED, *plan_h,
                                                  alias=table.alias)
        with kernels.kernel_timing() as t:
            got = kernels.sample_negatives(*dev[:3], N, first, V, SEED, *plan_d, alias=alias)
        assert [r[0] for r in t.records] == ["rb_sample_negatives_alias"]
        assert torch.equal(got.cpu(), want)
        if plan_h:
            assert got.shape == (m_pad, N) and (got[ntok:] == -1).all()
        # alias=None: the uniform sampler, unchanged
        with kernels.kernel_timing() as t:
            plain = kernels.sample_negatives(*dev[:3], N, first, V, SEED, *plan_d, alias=None)
        assert [r[0] for r in t.records] == ["rb_sample_negatives"]
        assert torch.equal(plain, kernels.sample_negatives(*dev[:3], N, first, V, SEED, *plan_d))
        assert torch.equal(plain.cpu(), kernels.sample_negatives_reference(
            item_seq, lens, pos, N, first, V, SEED, *plan_h))
    with pytest.raises(ValueError, match="alias"):
        kernels.sample_negatives(*dev[:3], N, first, V, SEED, alias=alias[:-1])


def test_sampler_frequencies(cuda):
    """The 16,384 draws of the host frequency test, on the device: the same
    ids, so the same statistic."""
    from datamining_recblr_amd import kernels

    table = kernels.negative_sampler(counts())
    item_seq, lens, pos = frequency_case()
    got = kernels.sample_negatives(item_seq.to(cuda), lens.to(cuda), pos.to(cuda), 256, 1, V,
                                   FREQ_SEED, alias=table.alias.to(cuda)).cpu()
    assert torch.equal(got, kernels.sample_negatives_reference(item_seq, lens, pos, 256, 1, V,
                                                               FREQ_SEED, alias=table.alias))
    check_frequencies(got, table.q.numpy())


# ---- the loss kernels ------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 20, 256])
@pytest.mark.parametrize("d", [64, 128])
def test_kernels_vs_fp64(cuda, d, n):
    from datamining_recblr_amd import kernels, scoring

    h, tab, target, neg, offsets, order = _case(d, n, cuda)
    item_shift = _item_shift(cuda)
    assert kernels.shared_softmax_supported(h, tab, n)
    ref = lambda a, b: scoring.shared_softmax_reference(a, b, target, neg, offsets, order, SHIFT,
                                                        item_shift=item_shift)
    with kernels.kernel_timing() as t:
        got = _grads(lambda a, b: scoring.shared_softmax_loss(a, b, target, neg, offsets, order,
                                                              SHIFT, item_shift=item_shift),
                     h, tab, torch.float32)
    assert [r[0] for r in t.records] == ITEM_NAMES
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
    # the term is there: the loss without it is another number
    plain = scoring.shared_softmax_loss(h, tab, target, neg, offsets, order, SHIFT)
    assert float(got[0]) - float(plain) > 1e-3       # every term is positive: a larger loss
    dh = got[1]
    assert (dh[30] == 0).all() and (dh[29] != 0).any()          # the ignored row: exact zeros
    if n >= 20:
        lse = kernels.shared_softmax_fwd(h, tab, target, neg, offsets, order, SHIFT, 48,
                                         item_shift)[2]
        dl = torch.ones((), device=cuda)
        nl = torch.tensor(int((target >= 0).sum()), device=cuda)
        _, coef, dneg = kernels.shared_softmax_bwd(h, tab, target, neg, offsets, order, lse, dl,
                                                   nl, SHIFT, 48, item_shift)
        b = int(order[1])
        assert (dneg[b, 2] == 0).all() and (dneg[b, n - 1] == 0).all() and (dneg[b, 1] != 0).any()
        assert coef[30] == 0 and coef[29] != 0


@pytest.mark.parametrize("n", [20, 256])
def test_launch_names_and_bits(cuda, n):
    from datamining_recblr_amd import kernels, scoring

    h, tab, target, neg, offsets, order = _case(128, n, cuda)
    item_shift = _item_shift(cuda)
    old = lambda a, b: scoring.shared_softmax_loss(a, b, target, neg, offsets, order, SHIFT)
    none = lambda a, b: scoring.shared_softmax_loss(a, b, target, neg, offsets, order, SHIFT,
                                                    item_shift=None)
    items = lambda a, b: scoring.shared_softmax_loss(a, b, target, neg, offsets, order, SHIFT,
                                                     item_shift=item_shift)
    with kernels.kernel_timing() as t:
        a = _grads(old, h, tab, torch.float32)
    assert [r[0] for r in t.records] == PLAIN_NAMES
    with kernels.kernel_timing() as t:
        b = _grads(none, h, tab, torch.float32)
    assert [r[0] for r in t.records] == PLAIN_NAMES
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with kernels.kernel_timing() as t:
        one = _grads(items, h, tab, torch.float32)
    assert [r[0] for r in t.records] == ITEM_NAMES
    two = _grads(items, h, tab, torch.float32)
    assert all(torch.equal(x, y) for x, y in zip(one, two))
    assert not torch.equal(one[0], a[0])
    # a zero item_shift is the plain path's arithmetic: (z + shift) + 0
    zero = _grads(lambda x, y: scoring.shared_softmax_loss(
        x, y, target, neg, offsets, order, SHIFT, item_shift=torch.zeros_like(item_shift)),
        h, tab, torch.float32)
    assert all(torch.equal(x, y) for x, y in zip(zero, a))
    # ids outside [-1, V) are never looked up in item_shift: NaN, as without it
    n2 = neg.clone()
    n2[2, 9] = V
    assert torch.isnan(scoring.shared_softmax_loss(h, tab, target, n2, offsets, order, SHIFT,
                                                   item_shift=item_shift))
    with pytest.raises(ValueError, match="item_shift"):
        kernels.shared_softmax_fwd(h, tab, target, neg, offsets, order, SHIFT, 48, item_shift[:-1])


def test_unsupported_shapes_take_the_reference(cuda):
    from datamining_recblr_amd import kernels, scoring
    from test_shared_softmax_host import plan

    d, n = 20, 8
    g = torch.Generator().manual_seed(d)
    offsets, order = (t.to(cuda) for t in plan(LENS))
    M = int(offsets[-1])
    h, tab = torch.randn(M, d, generator=g).to(cuda), torch.randn(V, d, generator=g).to(cuda)
    target = torch.randint(0, V, (M,), generator=g).to(cuda)
    neg = torch.randint(0, V, (len(LENS), n), generator=g).to(cuda)
    item_shift = _item_shift(cuda)
    with kernels.kernel_timing() as t:
        loss = scoring.shared_softmax_loss(h, tab, target, neg, offsets, order, SHIFT,
                                           item_shift=item_shift)
    assert not t.records
    assert torch.equal(loss, scoring.shared_softmax_reference(h, tab, target, neg, offsets, order,
                                                              SHIFT, item_shift=item_shift))


# ---- the model -------------------------------------------------------------------------
L = 48


def _model(cuda, **kw):
    from datamining_recblr_amd.model import RecBLR
    from datamining_recblr_amd.recbole_compat import SyntheticDataset

    cfg = dict(hidden_size=64, loss_type="CE", num_layers=2, dropout_prob=0.0, expand=2,
               d_conv=4, bd_lru_only=False, disable_conv1d=False, disable_ffn=False,
               MAX_ITEM_LIST_LENGTH=L, train_all_positions=True, dense_loss="sampled_softmax",
               dense_negatives=20, dense_sampling="popularity")
    cfg.update(kw)
    torch.manual_seed(11)
    return RecBLR(cfg, SyntheticDataset(V)).to(cuda).eval()


def _batch(cuda):
    g = torch.Generator().manual_seed(4)
    lens = torch.tensor(LENS)
    seq = torch.randint(1, V, (len(LENS), L), generator=g)
    seq = seq * (torch.arange(L)[None] < lens[:, None])
    pos = torch.randint(1, V, (len(LENS),), generator=g)
    return {"item_id_list": seq.to(cuda), "item_length": lens.to(cuda), "item_id": pos.to(cuda)}


def _next_seed(seed):
    torch.manual_seed(seed)
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64))   # blocks.draw_seed's draw


def test_model_sampled_softmax_with_the_popularity_proposal(cuda):
    from datamining_recblr_amd import kernels, scoring

    inter = _batch(cuda)
    model, twin = _model(cuda), _model(cuda)
    twin.load_state_dict(model.state_dict())
    keys = set(model.state_dict())
    with pytest.raises(RuntimeError, match="set_item_counts"):
        model.calculate_loss(inter)
    table = model.set_item_counts(torch.from_numpy(counts()).to(cuda))
    assert model.neg_alias.device.type == "cuda" and set(model.state_dict()) == keys
    cpu = [inter[k].cpu() for k in ("item_id_list", "item_length", "item_id")]
    lists = kernels.sample_negatives_reference(*cpu, 20, 1, V, _next_seed(5), alias=table.alias)
    assert not torch.equal(lists, kernels.sample_negatives_reference(*cpu, 20, 1, V,
                                                                     _next_seed(5)))
    torch.manual_seed(5)
    loss = model.calculate_loss(inter)
    loss.backward()
    h, seq = twin.forward_all(inter["item_id_list"], inter["item_length"])
    target = kernels.next_item_targets(seq.ids, seq.offsets, seq.order, inter["item_id"])
    ref = scoring.shared_softmax_reference(h, twin.item_embedding.weight, target, lists.to(cuda),
                                           seq.offsets, seq.order, -math.log(20),
                                           item_shift=table.item_shift.to(cuda))
    ref.backward()
    close(loss, ref, "loss")
    want = dict(twin.named_parameters())
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        close(p.grad, want[name].grad, name)
    # given the same lists the loss is the drawn one, bit for bit
    assert torch.equal(model.calculate_loss_sampled(inter, lists.to(cuda)).detach(), loss.detach())
    # sampled_softmax_correct: False drops both terms
    model.sampled_softmax_correct = False
    with torch.no_grad():
        h, seq = model.forward_all(inter["item_id_list"], inter["item_length"])
        plain = scoring.shared_softmax_loss(h, model.item_embedding.weight, target,
                                            lists.to(cuda), seq.offsets, seq.order, 0.0, max_len=L)
    assert torch.equal(model.calculate_loss_sampled(inter, lists.to(cuda)).detach(), plain)


def test_model_pairs_draw_from_the_table(cuda):
    from datamining_recblr_amd import kernels

    inter = _batch(cuda)
    model = _model(cuda, dense_loss="pairs", dense_negatives=3)
    with pytest.raises(RuntimeError, match="set_item_counts"):
        model.calculate_loss(inter)
    table = model.set_item_counts(counts())
    torch.manual_seed(7)
    drawn = model.calculate_loss(inter).detach()
    _, seq = model.forward_all(inter["item_id_list"], inter["item_length"])
    cpu = [inter[k].cpu() for k in ("item_id_list", "item_length", "item_id")]
    ids = kernels.sample_negatives_reference(*cpu, 3, 1, V, _next_seed(7), seq.offsets.cpu(),
                                             seq.inv.cpu(), seq.ntok, alias=table.alias)
    uniform = kernels.sample_negatives_reference(*cpu, 3, 1, V, _next_seed(7), seq.offsets.cpu(),
                                                 seq.inv.cpu(), seq.ntok)
    assert torch.isfinite(drawn) and not torch.equal(ids, uniform)
    assert torch.equal(model.calculate_loss_pairs(inter, ids.to(cuda)).detach(), drawn)
    assert not torch.equal(model.calculate_loss_pairs(inter, uniform.to(cuda)).detach(), drawn)


def test_fit_dense_with_the_popularity_proposal(cuda, tmp_path):
    from test_gpu_train import _toy_atomic
    from datamining_recblr_amd import data as dp, kernels
    from datamining_recblr_amd.distributed import DistEnv
    from datamining_recblr_amd.model import RecBLR
    from datamining_recblr_amd.recbole_compat import SyntheticDataset
    from datamining_recblr_amd.trainer import fit

    d = _toy_atomic(tmp_path, cuda)
    torch.manual_seed(0)
    cfg = {"hidden_size": 32, "loss_type": "CE", "num_layers": 2, "dropout_prob": 0.1,
           "expand": 2, "d_conv": 4, "bd_lru_only": False, "disable_conv1d": False,
           "disable_ffn": False, "MAX_ITEM_LIST_LENGTH": 20, "train_all_positions": True,
           "dense_loss": "sampled_softmax", "dense_negatives": 32,
           "dense_sampling": "popularity"}
    model = RecBLR(cfg, SyntheticDataset(d.n_items, d.n_users)).to(cuda)
    assert model.neg_alias is None
    res = fit(model, d, DistEnv(), epochs=2, batch_size=64, lr=1e-2, log=None, dense=True)
    # fit built the proposal from the train split's counts
    want = kernels.negative_sampler(dp.train_item_counts(d).cpu().numpy(), 0.75, 1.0, 1, d.n_items)
    assert torch.equal(model.neg_alias.cpu(), want.alias)
    losses = [h["train_loss"] for h in res["history"]]
    print("train loss per epoch", losses)
    assert len(losses) == 2 and all(math.isfinite(x) for x in losses) and losses[1] <= losses[0]

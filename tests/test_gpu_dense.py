"""All-position ("dense") training on the GPU: the target kernel, the
row-chunked CE with ignorable rows against fp64, and the equivalence that
justifies the feature — calculate_loss_dense on a batch equals calculate_loss
on the batch expanded to one right-padded row per prefix.

Tolerance: every comparison with a reference is max |got - ref| <= 1e-4 * max
|ref| (relative to the largest reference entry), the project's bar for the
timed step (tests/test_gpu_timed_step.py)."""
import pytest
import torch
import torch.nn.functional as F

from test_dense_host import L, LENS, packed_case, targets_by_hand

pytestmark = pytest.mark.gpu

TOL = 1e-4
N_ITEMS = 77


def close(got, ref, what, tol=TOL):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"{what}: max err {err:.3e}, largest reference entry {scale:.3e}")
    assert err <= tol * scale, f"{what}: max err {err:.3e} > {tol} * {scale:.3e}"


def test_next_item_targets_kernel(cuda):
    from datamining_recblr_amd import kernels

    item_seq, lengths, pos_items, ids, offsets, order = packed_case()
    want = targets_by_hand(item_seq, lengths, pos_items, order, 256)
    got = kernels.next_item_targets(ids.to(cuda), offsets.to(cuda), order.to(cuda),
                                    pos_items.to(cuda), 256)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)
    assert (got[34:] == -1).all()
    ref = kernels.next_item_targets_reference(ids.to(cuda), offsets.to(cuda), order.to(cuda),
                                              pos_items.to(cuda), 256)
    assert torch.equal(got, ref)
    # the packed plan of the model's own forward gives the same ids
    ids2, _, _, _ = kernels.pack_plan(item_seq.to(cuda), offsets.to(cuda), order.to(cuda), 34)
    assert torch.equal(ids2.cpu(), ids)


def _ce_case(M, V, d, cuda, seed, ignored):
    g = torch.Generator().manual_seed(seed)
    seq = (0.5 * torch.randn(M, d, generator=g)).to(cuda)
    tab = (0.5 * torch.randn(V, d, generator=g)).to(cuda)
    tgt = torch.randint(0, V, (M,), generator=g)
    tgt[list(ignored)] = -1
    return seq, tab, tgt.to(cuda)


def _run(seq, tab, tgt, scale=0.7, **kw):
    from datamining_recblr_amd import scoring

    s, w = seq.clone().requires_grad_(), tab.clone().requires_grad_()
    loss = scoring.item_cross_entropy_rows(s, w, tgt, **kw)
    (scale * loss).backward()
    return loss.detach(), s.grad, w.grad


def _ref64(seq, tab, tgt, scale=0.7):
    s, w = seq.double().requires_grad_(), tab.double().requires_grad_()
    loss = F.cross_entropy(s @ w.t(), tgt, ignore_index=-1)
    (scale * loss).backward()
    return loss.detach(), s.grad, w.grad


@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("M,ignored", [(300, (0, 5, 130, 255, 256, 299)), (40, (0, 17, 39))])
def test_rows_ce_vs_fp64(cuda, monkeypatch, M, ignored, d):
    """Two chunks (256 + 44 live rows) and one mostly padded chunk; V = 77 is
    no multiple of 32; d = 128 runs both products on rb_gemm_tn_h (no library
    GEMM), d = 64 the sliced path."""
    from datamining_recblr_amd import kernels

    seq, tab, tgt = _ce_case(M, N_ITEMS, d, cuda, 3, ignored)
    mm = []
    orig = torch.mm
    monkeypatch.setattr(torch, "mm", lambda *a, **k: mm.append(1) or orig(*a, **k))
    with kernels.kernel_timing() as t:
        loss, ds, dw = _run(seq, tab, tgt, chunk_rows=256)
    names = [r[0] for r in t.records]
    chunks = -(-M // 256)
    assert names.count("rb_item_ce_fwd_h_rows") == chunks, names
    if d == 128:
        assert names.count("rb_item_ce_probs_h_both_rows") == chunks and not mm, (names, len(mm))
    else:
        assert names.count("rb_item_ce_probs_h_rows") == chunks and mm, (names, len(mm))
    rl, rs, rw = _ref64(seq, tab, tgt)
    close(loss, rl, "loss")
    close(ds, rs, "dseq")
    close(dw, rw, "dtable")
    assert (ds[list(ignored)] == 0).all()


@pytest.mark.parametrize("d", [128, 64])
def test_rows_ce_ignored_rows(cuda, d):
    """An ignored row's dseq is exactly 0, and its (finite) values change
    neither the loss nor dtable by a bit."""
    ignored = (0, 31, 32, 200, 299)
    seq, tab, tgt = _ce_case(300, N_ITEMS, d, cuda, 4, ignored)
    loss, ds, dw = _run(seq, tab, tgt, chunk_rows=256)
    assert (ds[list(ignored)] == 0).all() and torch.isfinite(loss)
    seq2 = seq.clone()
    seq2[list(ignored)] = 37.5 * torch.randn(len(ignored), d, device=cuda)
    loss2, ds2, dw2 = _run(seq2, tab, tgt, chunk_rows=256)
    assert torch.equal(loss, loss2) and torch.equal(dw, dw2)
    assert torch.equal(ds, ds2)
    # an out-of-range target other than -1 still gives NaN
    bad = tgt.clone()
    bad[7] = N_ITEMS
    assert torch.isnan(_run(seq, tab, bad, chunk_rows=256)[0])
    # no live row at all: 0 and zero gradients
    z, dz, dwz = _run(seq, tab, torch.full_like(tgt, -1))
    assert float(z) == 0.0 and (dz == 0).all() and (dwz == 0).all()


def test_rows_ce_deterministic_and_chunk_independent(cuda):
    seq, tab, tgt = _ce_case(600, N_ITEMS, 128, cuda, 5, (3, 300, 599))
    a = _run(seq, tab, tgt, chunk_rows=256)
    b = _run(seq, tab, tgt, chunk_rows=256)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    c = _run(seq, tab, tgt, chunk_rows=512, n_live=597)
    for x, y, what in zip(a, c, ("loss", "dseq", "dtable")):
        close(x, y, f"{what} (chunks of 256 vs 512)")


# ---- the model ---------------------------------------------------------------------
def _model(cuda, dropout=0.0, packed=True, **kw):
    from datamining_recblr_amd.model import RecBLR
    from datamining_recblr_amd.recbole_compat import SyntheticDataset

    cfg = dict(hidden_size=128, loss_type="CE", num_layers=2, dropout_prob=dropout, expand=2,
               d_conv=4, bd_lru_only=False, disable_conv1d=False, disable_ffn=False,
               MAX_ITEM_LIST_LENGTH=L, **kw)
    torch.manual_seed(11)
    m = RecBLR(cfg, SyntheticDataset(N_ITEMS)).to(cuda)
    m.pack_sequences = packed
    return m


def _batches(cuda):
    """The 5 rows and their expansion: one right-padded row per prefix (34)."""
    item_seq, lengths, pos_items, _, _, _ = packed_case(n_items=N_ITEMS)
    rows, lens, tgts = [], [], []
    for b in range(len(LENS)):
        n = int(lengths[b])
        for t in range(n):
            r = torch.zeros(L, dtype=torch.int64)
            r[:t + 1] = item_seq[b, :t + 1]
            rows.append(r)
            lens.append(t + 1)
            tgts.append(int(item_seq[b, t + 1]) if t + 1 < n else int(pos_items[b]))

    def inter(s, n, p):
        return {"item_id_list": s.to(cuda), "item_length": n.to(cuda), "item_id": p.to(cuda)}

    return (inter(item_seq, lengths, pos_items),
            inter(torch.stack(rows), torch.tensor(lens), torch.tensor(tgts)))


@pytest.mark.parametrize("packed", [True, False])
def test_dense_loss_equals_loss_on_expanded_batch(cuda, packed):
    model = _model(cuda, packed=packed).train()
    dense, expanded = _batches(cuda)
    assert expanded["item_id_list"].shape[0] == 34

    model.zero_grad(set_to_none=True)
    ref = model.calculate_loss(expanded)
    ref.backward()
    ref_grads = {n: p.grad.clone() for n, p in model.named_parameters()}

    model.zero_grad(set_to_none=True)
    loss = model.calculate_loss_dense(dense)
    loss.backward()
    close(loss, ref, "loss")
    for n, p in model.named_parameters():
        assert p.grad is not None, n
        close(p.grad, ref_grads[n], n)

    with torch.no_grad():
        h, seq = model.forward_all(dense["item_id_list"], dense["item_length"])
        out = model.forward(dense["item_id_list"], dense["item_length"])
    assert h.shape == (34, 128) and seq.ntok == 34
    close(h[seq.last], out, "forward_all[seq.last] vs forward")
    # every row, not only the last: row offsets[s] + t is the expanded row's output
    with torch.no_grad():
        out_exp = model.forward(expanded["item_id_list"], expanded["item_length"])
    order = seq.order.tolist()
    starts = [0]
    for n in LENS:
        starts.append(starts[-1] + n)   # the expanded rows are in batch-row order
    pick = torch.tensor([starts[b] + t for b in order for t in range(LENS[b])], device=cuda)
    close(h, out_exp[pick], "forward_all vs forward on each prefix")

    # the config switch routes calculate_loss there
    model.train_all_positions = True
    assert torch.equal(model.calculate_loss(dense).detach(), loss.detach())


def test_dense_training_step_with_dropout(cuda):
    from datamining_recblr_amd.optim import make_adam

    model = _model(cuda, dropout=0.2, train_all_positions=True).train()
    dense, _ = _batches(cuda)
    opt = make_adam(model.parameters(), lr=1e-3, weight_decay=0.0)
    before = [p.detach().clone() for p in model.parameters()]
    loss = model.calculate_loss(dense)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    assert torch.isfinite(loss)
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    opt.step()
    torch.cuda.synchronize()
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    assert all(torch.isfinite(p).all() for p in model.parameters())

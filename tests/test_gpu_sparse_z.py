"""GPU tests of the last layer's sparse z: under gather_indexes on packed
sequences y = silu(z) * h is read only at each sequence's last row, so z is
computed, and dz is non-zero, only there (RecBLR.py:84,162,206).

  * the scan kernels' z_last / dz_last mode against the same kernels fed a
    dense z, bit for bit;
  * the split in-projection (linear.SplitInProjFn) against the one-GEMM xz
    path;
  * the model with the path on and off, and the fall-back under a hook."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _packed(lens, cuda):
    from datamining_recblr_amd import kernels

    lens = torch.tensor(sorted(lens, reverse=True))   # longest first, as the model packs
    offs = torch.zeros(lens.numel() + 1, dtype=torch.int64)
    torch.cumsum(lens, 0, out=offs[1:])
    ntok = int(offs[-1])
    return kernels.Packed(offs.to(cuda), 64, ntok), (offs[1:] - 1).to(cuda), ntok


# lengths around the RB_TILE = 16 boundaries; B = 5 leaves the middle sequence
# of the backward's long/short pairing on its own
LENS = {5: (50, 32, 17, 15, 1), 8: (50, 33, 32, 17, 16, 16, 15, 1)}


@pytest.mark.parametrize("permute", [False, True])
@pytest.mark.parametrize("H", [64, 256])
@pytest.mark.parametrize("B", [5, 8])
def test_scan_kernels_with_z_last_equal_dense_z(cuda, B, H, permute):
    """rb_gate_scan_fwd_last / _bwd_last given z_last / dz_last [B, H] == the
    same entry points given z / dz at every row: y_last, carries, drg, dxc,
    dh0, dlam and dgate_b bit for bit, dz_last == dz at the last rows — and
    the dense dz is exactly zero at every other row (the premise)."""
    from datamining_recblr_amd import kernels

    g = torch.Generator().manual_seed(100 * B + H + permute)
    seq, last, ntok = _packed(LENS[B], cuda)
    rg = torch.randn(ntok, 2 * H, generator=g).to(cuda)
    xz = torch.randn(ntok, 2 * H, generator=g).to(cuda)
    xc, z = xz[:, :H], xz[:, H:]
    lam = torch.linspace(-2.2, -6.9, H).to(cuda)
    gb = (0.1 * torch.randn(2 * H, generator=g)).to(cuda)
    h0 = torch.randn(H, generator=g).to(cuda)
    perm = torch.randperm(B, generator=g).to(cuda) if permute else None
    # row of sequence s in the [B, H] operands
    row = perm if permute else torch.arange(B, device=cuda)
    z_last = torch.empty(B, H, device=cuda)
    z_last[row] = z.index_select(0, last)
    kw = dict(gate_b=gb, seq=seq, last_only=True, batch_row=perm)

    y1, car1 = kernels.gate_scan_fwd(rg, xc, z, lam, h0, **kw)
    y2, car2 = kernels.gate_scan_fwd(rg, xc, None, lam, h0, z_last=z_last, **kw)
    assert torch.equal(y1, y2)
    for s, n in enumerate(sorted(LENS[B], reverse=True)):   # a sequence's own tiles
        nt = (n + kernels.RB_TILE - 1) // kernels.RB_TILE
        assert torch.equal(car1[s, :nt], car2[s, :nt]), s

    dyl = torch.randn(B, H, generator=g).to(cuda)
    dz = torch.full((ntok, H), float("nan"), device=cuda)
    dz_last = torch.full((B, H), float("nan"), device=cuda)
    r1 = kernels.gate_scan_bwd(rg, xc, z, lam, car1, dyl, dz, **kw)
    r2 = kernels.gate_scan_bwd(rg, xc, None, lam, car1, dyl, dz_last, z_last=z_last, **kw)
    for name, a, b in zip(("drg", "dxc", "dlam", "dgate_b", "dh0"), r1, r2):
        assert torch.equal(a, b), name
    assert torch.equal(dz_last[row], dz.index_select(0, last))
    other = torch.ones(ntok, dtype=torch.bool, device=cuda)
    other[last] = False
    assert other.any() and dz[other].abs().max().item() == 0.0


def _rel_err(y, ref):
    return ((y.double() - ref.double()).abs().max() / ref.double().abs().max()).item()


@pytest.mark.parametrize("d", [64, 128])
def test_split_in_projection_equals_one_gemm(cuda, d):
    """SplitInProjFn (x = X W[:H]^T, z_last = X[last] W[H:]^T and their
    gradients) against the one-GEMM xz path on the same inputs.  Each f16x3
    product is within 2e-6 of fp64 (tests/test_gpu_gemm_half.py, relative to
    the result's largest entry), so two of them differ by at most 4e-6."""
    from datamining_recblr_amd import linear

    g = torch.Generator().manual_seed(d)
    H, B = 2 * d, 8
    seq, last, ntok = _packed((150, 130, 110, 97, 80, 64, 50, 19), cuda)
    assert ntok == 700
    last = last[torch.randperm(B, generator=g).to(cuda)]   # batch order
    x0 = torch.randn(ntok, d, generator=g).to(cuda)
    w0 = (torch.randn(2 * H, d, generator=g) / d ** 0.5).to(cuda)
    gx = torch.randn(ntok, H, generator=g).to(cuda)
    gz = torch.randn(B, H, generator=g).to(cuda)

    x, w = x0.clone().requires_grad_(), w0.clone().requires_grad_()
    xh, z_last = linear.split_in_projection(x, w, last)
    assert xh.shape == (ntok, H) and xh.is_contiguous() and z_last.shape == (B, H)
    torch.autograd.backward((xh, z_last), (gx, gz))

    xr, wr = x0.clone().requires_grad_(), w0.clone().requires_grad_()
    xz = linear.LinearFn.apply(xr, wr, None)
    dxz = torch.zeros(ntok, 2 * H, device=cuda)
    dxz[:, :H] = gx
    dxz[last, H:] = gz
    xz.backward(dxz)

    bar = 4e-6
    assert _rel_err(xh, xz[:, :H]) < bar
    assert _rel_err(z_last, xz[last, H:]) < bar
    assert _rel_err(x.grad, xr.grad) < bar
    assert _rel_err(w.grad[:H], wr.grad[:H]) < bar
    assert _rel_err(w.grad[H:], wr.grad[H:]) < bar


CFG = dict(hidden_size=64, loss_type="CE", num_layers=2, dropout_prob=0.0, expand=2,
           d_conv=4, bd_lru_only=False, disable_conv1d=False, disable_ffn=False,
           MAX_ITEM_LIST_LENGTH=50)


def _model(cuda):
    from datamining_recblr_amd import model as M
    from datamining_recblr_amd.recbole_compat import SyntheticDataset

    torch.manual_seed(0)
    return M.RecBLR(CFG, SyntheticDataset(300)).to(cuda).train()


def test_model_sparse_z_equals_dense_z(cuda):
    """RecBLR.calculate_loss + backward with the last layer's sparse z on
    (threshold 0) and off, dropout 0: the loss within 1e-5 and every gradient
    within 1e-5 of its norm (the bar of tests/test_gpu_eval.py::
    test_gathered_last_layer_equals_full)."""
    from datamining_recblr_amd import model as M
    from datamining_recblr_amd.distributed import synthetic_interaction

    inter = synthetic_interaction(128, 50, 300, cuda, seed=4)
    res = []
    prev = M.set_sparse_z(True, 0)
    try:
        for on in (True, False):
            M.set_sparse_z(on)
            model = _model(cuda)
            taken = []
            layer = model.recurrent_layers[-1].behavior_modeling
            inner = layer._sparse_z
            layer._sparse_z = lambda *a: taken.append(inner(*a)) or taken[-1]
            loss = model.calculate_loss(inter)
            loss.backward()
            assert taken == [on]
            res.append((loss.detach(), {n: p.grad.clone() for n, p in model.named_parameters()
                                        if p.grad is not None}))
    finally:
        M.set_sparse_z(*prev)
    (l1, g1), (l2, g2) = res
    print("loss", l1.item(), l2.item())
    assert g1.keys() == g2.keys()
    errs = {n: ((g1[n].double() - g2[n].double()).norm()
                / max(g2[n].double().norm().item(), 1e-12)).item() for n in g1}
    for n, e in errs.items():
        print(f"{e:.3e}  {n}")
    assert abs(l1.item() - l2.item()) < 1e-5
    for n, e in errs.items():
        assert e < 1e-5, (n, e)


def test_forward_hook_on_the_in_projection_selects_the_dense_path(cuda):
    """A forward hook on the last layer's behavior_modeling.input sees the
    [ntok, 2H] in-projection output, so that call keeps the dense z."""
    from datamining_recblr_amd import model as M
    from datamining_recblr_amd.distributed import synthetic_interaction

    inter = synthetic_interaction(128, 50, 300, cuda, seed=4)
    prev = M.set_sparse_z(True, 0)
    try:
        model = _model(cuda)
        layer = model.recurrent_layers[-1].behavior_modeling
        seen = []
        handle = layer.input.register_forward_hook(lambda m, a, out: seen.append(tuple(out.shape)))
        loss = model.calculate_loss(inter)
        loss.backward()
        handle.remove()
        ntok = int(inter[model.ITEM_SEQ_LEN].sum())
        assert seen == [(ntok, 2 * layer.hidden)]
        assert layer.input.weight.grad is not None
    finally:
        M.set_sparse_z(*prev)

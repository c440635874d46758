"""The cross-entropy head (csrc/item_scores.hip, scoring.item_cross_entropy and
item_cross_entropy_rows) against an independent fp64 reference
(tests/item_ce_reference.py: a plain torch statement of the operation), not
against torch fp32 or one kernel against another.

Per output tensor the error is max |got - ref64| / scale and the bar
M * e32 + 4 * 2^-24, e32 the same error of the reference's own fp32 run on the
same inputs (gate_scan_reference.channel_error / judge).  lse is judged per row
at the row's logit summand scale, P per row in probability units, dseq per
sequence row and ditems per item row at their summand scales, the loss as the
sum of its rows' losses: item_ce_reference.judge_all says how and why.

Value regimes (item_ce_reference.make_inputs): "random" (0.5 * randn),
"peaked" (each row's target leads the rest by a margin of 2 .. 4 nats; the
range is narrowed until plain fp32 itself is within 1e-4: PEAKED_MARGIN_MAX),
"large" (logits past +-100, both signs), "scaled" (seq rows times 2^k, item
rows times 2^-k, k in 60, -60, 37, -23, an all-zero seq row and item row) and
"ties" (bit-equal item rows, some of them targets).  Targets stand on item 0,
item V - 1, both sides of a 32-item tile border and both ends of the ragged
last tile; one target is shared by many rows and one item is nobody's target.

Which loop geometry a shape runs (plan(): blocks x splits x per [tiles], the
last split's tiles; the sequence rows fixed / k_ce_bwd_item's item rows fixed):
    (1, 1) (5, 7) (33, 64) (130, 97)   per 1; V < 32, a ragged tile, idle waves
    (600, 4100)    5 x 65 x 2 [129], last 1     33 x 10 x 2 [19], last 1
    (1100, 5000)   9 x 53 x 3 [157], last 1     40 x 12 x 3 [35], last 2
    (2049, 3900)   17 x 31 x 4 [122], last 2    31 x 17 x 4 [65], last 1
    (2049, 4003)   17 x 26 x 5 [126], last 1    32 x 13 x 5 [65], last 5
test_item_ce_reference_host.py asserts from the restated plan() that these
reach every kind of `per`, a short last split, split counts that leave idle
placements, partial and idle waves.

Paths and the tests that run them:
    rb_item_ce_fwd, rb_item_ce_bwd (both, dseq only, ditems only),
    rb_item_ce_probs in two item slices into a view                test_fp32_pipe
    rb_item_split_h, rb_item_ce_fwd_h, rb_item_ce_probs_h (into a view),
    _h_t, _h_both(pad_to=256), the group maxima                     test_f16_pipe
    rb_item_ce_fwd_h_rows over two and three chunks (accumulate), rb_item_ce_
    probs_h_rows, _both_rows, ignored rows                          test_rows_forms
    scoring.item_cross_entropy under CE_PIPE x CE_BACKWARD          test_autograd_pipe_and_backward
    ... under CE_GRADS f16 / torch                                  test_autograd_ce_grads
    scoring.item_cross_entropy_rows, chunk_rows = 256, d 128 / 64   test_autograd_rows

M is twice the worst ratio error / max(e32, 4 * 2^-24) measured on an MI355X
over all cases and paths below, rounded up:

    tensor   worst ratio   path and case                              M
    lse      0.56          rows (two, three) peaked-600x97x128        2
    loss     0.49          fp32 and f16 large-33x64x64                1
    P        2.03          f16 random-5x7x256                         5
    dseq     2.20          fp32 random-5x7x256                        5
    ditems   2.47          fp32 random-5x7x256                        5

(loss_rows is not an output of any entry point; its M, for the host test's
planted errors, is lse's.)  The exp2-based exponential and the f16 split's
dropped x1.y1 term cost at most this factor 2.5 over plain fp32.

One path measured far above the rest and was fixed: scoring.item_cross_entropy
under CE_PIPE = f16 with CE_BACKWARD = fused took lse from the f16 pipe's
forward and recomputed the logits on the fp32 pipe in rb_item_ce_bwd, so P =
exp(x - lse) - onehot mixed two roundings of the same logits: ratio 9.51 in
dseq and 9.28 in ditems at peaked-600x4100x128 (1.1 on every other path of that
case), over the bar M = 5 gives.  The fused backward's forward now runs on the
fp32 pipe (test_autograd_pipe_and_backward[peaked-600x4100x128-f16-fused]).
"""
import functools

import pytest
import torch

import item_ce_reference as R

pytestmark = pytest.mark.gpu

M = {"lse": 2, "loss_rows": 2, "loss": 1, "P": 5, "dseq": 5, "ditems": 5}

DLOSS = 0.7
SENTINEL = 7.25


@functools.lru_cache(maxsize=3)
def _case(c, ignored=()):
    """(inputs, fp64 reference, fp32 run) of a case: computed once, shared and
    left unchanged by the tests that use it."""
    inp = R.case_inputs(c, ignored)
    r64, r32 = R.both(inp, DLOSS)
    return inp, r64, r32


def _dev(inp, cuda):
    return inp.seq.to(cuda), inp.table.to(cuda), inp.target.to(cuda)


def _judge(path, c, got, r64, r32):
    res = R.judge_all(got, r64, r32, M)
    bad = []
    for n, (ok, err, limit, ratio) in res.items():
        print(f"RATIO {n} {ratio:.3f} {path} {R.case_id(c)} err {err:.3e} bar {limit:.3e}")
        if not ok:
            bad.append(f"{n}: error {err:.3e} > bar {limit:.3e} (ratio {ratio:.2f})")
    assert not bad, f"{path} {R.case_id(c)}: " + "; ".join(bad)


def _view(cuda, rows, cols, pad=(1, 2, 5, 3)):
    """A [rows, cols] view into a sentinel-filled parent, and the parent."""
    top, bottom, left, right = pad
    parent = torch.full((rows + top + bottom, cols + left + right), SENTINEL, device=cuda)
    return parent[top:top + rows, left:left + cols], parent


def _intact(parent, rows, cols, pad=(1, 2, 5, 3)):
    top, bottom, left, right = pad
    mask = torch.ones_like(parent, dtype=torch.bool)
    mask[top:top + rows, left:left + cols] = False
    return bool((parent[mask] == SENTINEL).all())


def _group_max(x):
    """max |x| over each group of 32 rows of x [n, c] (a partial last group too)."""
    m = x.abs().amax(1)
    return torch.nn.functional.pad(m, (0, (-m.numel()) % 32)).view(-1, 32).amax(1)


def _dloss(cuda):
    return torch.full((), DLOSS, device=cuda)


# ---- the fp32 pipe -----------------------------------------------------------------
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_fp32_pipe(cuda, c):
    from datamining_recblr_amd import kernels

    inp, r64, r32 = _case(c)
    seq, W, tgt = _dev(inp, cuda)
    B, V = c[1], c[2]
    dl = _dloss(cuda)
    loss, lse = kernels.item_ce_fwd(seq, W, tgt)
    dseq, ditems = kernels.item_ce_bwd(seq, W, tgt, lse, dl)
    # P in two item slices (the cut inside a tile) into one sentinel-filled parent
    p, parent = _view(cuda, B, V)
    cut = V // 3
    for v0, v1 in ((0, cut), (cut, V)):
        if v1 > v0:
            out = kernels.item_ce_probs(seq, W[v0:v1], tgt, lse, dl, item_offset=v0, out=p[:, v0:v1])
            assert out.data_ptr() == p[:, v0:v1].data_ptr()
    assert _intact(parent, B, V)
    _judge("fp32", c, dict(lse=lse, loss=loss, P=p, dseq=dseq, ditems=ditems), r64, r32)
    only_seq, none1 = kernels.item_ce_bwd(seq, W, tgt, lse, dl, want_items=False)
    none2, only_items = kernels.item_ce_bwd(seq, W, tgt, lse, dl, want_seq=False)
    assert none1 is None and none2 is None
    assert torch.equal(only_seq, dseq) and torch.equal(only_items, ditems)


# ---- the f16 pipe ------------------------------------------------------------------
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_f16_pipe(cuda, c):
    from datamining_recblr_amd import kernels

    inp, r64, r32 = _case(c)
    seq, W, tgt = _dev(inp, cuda)
    B, V = c[1], c[2]
    dl = _dloss(cuda)
    ss, sw = kernels.item_split_h(seq), kernels.item_split_h(W)
    loss, lse = kernels.item_ce_fwd_h(ss, sw, tgt)
    p, parent = _view(cuda, B, V)
    kernels.item_ce_probs_h(ss, sw, tgt, lse, dl, out=p)
    assert _intact(parent, B, V)
    _judge("f16", c, dict(lse=lse, loss=loss, P=p), r64, r32)
    # the other layouts: the same bits, and the group maxima of those bits
    pt, gmax = kernels.item_ce_probs_h_t(ss, sw, tgt, lse, dl)
    assert torch.equal(pt, p.t())
    assert torch.equal(gmax, _group_max(p.t()))
    p2, pt2, bmax, gmax2 = kernels.item_ce_probs_h_both(ss, sw, tgt, lse, dl, pad_to=256)
    assert p2.shape == (B, -(-V // 256) * 256)
    assert torch.equal(p2[:, :V], p) and not p2[:, V:].any()
    assert torch.equal(pt2, p.t()) and torch.equal(gmax2, gmax)
    assert torch.equal(bmax, _group_max(p))


# ---- the rows forms ----------------------------------------------------------------
CHUNKINGS = {"two": ((0, 300), (300, 600)), "three": ((0, 256), (256, 456), (456, 600))}


def _rows_run(kernels, seq, W, tgt, inv_n, chunks, cuda, r64=None, r32=None, path=None, c=None):
    """The three rows kernels over `chunks`: (lse, loss, P, bmax, gmax), each
    output buffer a view into a sentinel-filled parent that is checked intact.
    With the reference runs, loss[0] is judged after every chunk against the
    sum of the rows so far."""
    n, V = seq.shape[0], W.shape[0]
    dl = _dloss(cuda)
    ss, sw = kernels.item_split_h(seq), kernels.item_split_h(W)
    lse_parent = torch.full((n + 5,), SENTINEL, device=cuda)
    loss_parent = torch.full((3,), SENTINEL, device=cuda)
    lse, loss = lse_parent[2:n + 2], loss_parent[1:2]
    p, parent = _view(cuda, n, V)
    bmaxes, gmaxes = [], []
    for k, (r0, r1) in enumerate(chunks):
        sr = ss.rows(r0, r1)
        before = loss.clone()
        kernels.item_ce_fwd_h_rows(sr, sw, tgt[r0:r1], inv_n, lse[r0:r1], loss, accumulate=k > 0)
        if r64 is not None:
            live = (tgt[r0:r1] >= 0).any()
            if k > 0 and not live:     # a wholly ignored chunk adds exactly nothing
                assert torch.equal(loss, before)
            terms64 = (r64.loss_rows[:r1] * r64.inv_n)[:, None]
            terms32 = (r32.loss_rows[:r1] * r32.inv_n)[:, None]
            ok, err, limit, ratio = R.judge(loss.reshape(1), terms64.sum().reshape(1),
                                            terms32.sum().reshape(1), M["loss"], scale=terms64,
                                            scale32=terms32)
            print(f"RATIO loss {ratio:.3f} {path}-after-chunk-{k} {R.case_id(c)} err {err:.3e} bar {limit:.3e}")
            assert ok, f"loss after chunk {k}: error {err:.3e} > bar {limit:.3e}"
        kernels.item_ce_probs_h_rows(sr, sw, tgt[r0:r1], lse[r0:r1], dl, inv_n, out=p[r0:r1])
        p2, pt2, bmax, gmax = kernels.item_ce_probs_h_both_rows(sr, sw, tgt[r0:r1], lse[r0:r1], dl,
                                                                inv_n, pad_to=256)
        assert torch.equal(p2[:, :V], p[r0:r1]) and not p2[:, V:].any()
        assert torch.equal(pt2, p[r0:r1].t())
        assert torch.equal(bmax, _group_max(p[r0:r1])) and torch.equal(gmax, _group_max(p[r0:r1].t()))
        bmaxes.append(bmax)
        gmaxes.append(gmax)
    assert _intact(parent, n, V)
    assert (lse_parent[:2] == SENTINEL).all() and (lse_parent[n + 2:] == SENTINEL).all()
    assert loss_parent[0] == SENTINEL and loss_parent[2] == SENTINEL
    return lse.clone(), loss.clone(), p.clone(), torch.cat(bmaxes), torch.stack(gmaxes)


@pytest.mark.parametrize("chunking", sorted(CHUNKINGS))
@pytest.mark.parametrize("c", R.ROWS_CASES, ids=R.case_id)
def test_rows_forms(cuda, c, chunking):
    """Ignored rows at 0, 31, 32, the whole tile 64 .. 95, rows 256 .. 455 (a
    whole chunk of the three-chunk run) and the last row."""
    from datamining_recblr_amd import kernels

    inp, r64, r32 = _case(c, R.ROWS_IGNORED)
    seq, W, tgt = _dev(inp, cuda)
    chunks = CHUNKINGS[chunking]
    path = f"rows-{chunking}"
    lse, loss, p, bmax, gmax = _rows_run(kernels, seq, W, tgt, r64.inv_n, chunks, cuda, r64, r32,
                                         path, c)
    ig = list(R.ROWS_IGNORED)
    assert not p[ig].any()
    _judge(path, c, dict(lse=lse, loss=loss, P=p), r64, r32)
    # large finite values in the ignored rows: no output bit moves (but those rows' own lse)
    g = torch.Generator().manual_seed(5)
    seq2 = seq.clone()
    seq2[ig] = (1e4 * torch.randn(len(ig), c[3], generator=g)).to(cuda)
    lse2, loss2, p2, bmax2, gmax2 = _rows_run(kernels, seq2, W, tgt, r64.inv_n, chunks, cuda)
    live = (tgt >= 0)
    assert torch.equal(loss2, loss) and torch.equal(lse2[live], lse[live])
    assert torch.isfinite(lse2).all()
    assert torch.equal(p2, p) and torch.equal(bmax2, bmax) and torch.equal(gmax2, gmax)


# ---- autograd ----------------------------------------------------------------------
def _backward(fn, seq, W):
    s, w = seq.clone().requires_grad_(), W.clone().requires_grad_()
    loss = fn(s, w)
    (DLOSS * loss).backward()
    return dict(loss=loss.detach(), dseq=s.grad, ditems=w.grad)


@pytest.mark.parametrize("backward", ["slices", "fused"])
@pytest.mark.parametrize("pipe", ["f16", "f32"])
@pytest.mark.parametrize("c", R.AUTOGRAD_CASES[1:], ids=R.case_id)
def test_autograd_pipe_and_backward(cuda, monkeypatch, c, pipe, backward):
    from datamining_recblr_amd import kernels, scoring

    monkeypatch.setattr(scoring, "CE_PIPE", pipe)
    monkeypatch.setattr(scoring, "CE_BACKWARD", backward)
    inp, r64, r32 = _case(c)
    seq, W, tgt = _dev(inp, cuda)
    with kernels.kernel_timing() as t:
        got = _backward(lambda s, w: scoring.item_cross_entropy(s, w, tgt), seq, W)
    names = {r[0] for r in t.records}
    # the fused backward recomputes the logits on the fp32 pipe, so its forward
    # runs there under either CE_PIPE: lse and P come from the same logits
    f16 = pipe == "f16" and backward == "slices"
    fwd = {"rb_item_split_h", "rb_item_ce_fwd_h"} if f16 else {"rb_item_ce_fwd"}
    bwd = "rb_item_ce_bwd" if backward == "fused" else \
        "rb_item_ce_probs_h" if f16 else "rb_item_ce_probs"
    assert fwd <= names and bwd in names, names
    assert not names & ({"rb_item_ce_fwd", "rb_item_ce_fwd_h", "rb_item_ce_bwd", "rb_item_ce_probs_h",
                         "rb_item_ce_probs", "rb_item_ce_probs_h_both"} - fwd - {bwd}), names
    _judge(f"autograd-{pipe}-{backward}", c, got, r64, r32)


@pytest.mark.parametrize("grads", ["f16", "torch"])
@pytest.mark.parametrize("c", R.AUTOGRAD_CASES[:2], ids=R.case_id)
def test_autograd_ce_grads(cuda, monkeypatch, tn_gemm_calls, c, grads):
    """(256, 515, 128) meets scoring._f16_grads_ok: under CE_GRADS = f16 both
    products run on rb_gemm_tn_h from rb_item_ce_probs_h_both; (130, 97, 128)
    does not and takes the sliced library path under either setting."""
    from datamining_recblr_amd import kernels, scoring

    monkeypatch.setattr(scoring, "CE_PIPE", "f16")
    monkeypatch.setattr(scoring, "CE_BACKWARD", "slices")
    monkeypatch.setattr(scoring, "CE_GRADS", grads)
    inp, r64, r32 = _case(c)
    seq, W, tgt = _dev(inp, cuda)
    with kernels.kernel_timing() as t:
        got = _backward(lambda s, w: scoring.item_cross_entropy(s, w, tgt), seq, W)
    names = {r[0] for r in t.records}
    if grads == "f16" and c[1] % 256 == 0:
        assert "rb_item_ce_probs_h_both" in names and "rb_item_ce_probs_h" not in names, names
        assert len(tn_gemm_calls) == 2, tn_gemm_calls
    else:
        assert "rb_item_ce_probs_h" in names and "rb_item_ce_probs_h_both" not in names, names
        assert not tn_gemm_calls, tn_gemm_calls
    _judge(f"autograd-grads-{grads}", c, got, r64, r32)


@pytest.mark.parametrize("c", R.ROWS_CASES[:3], ids=R.case_id)
def test_autograd_rows(cuda, tn_gemm_calls, c):
    """M = 600 rows in chunks of 256 (three chunks, the last padded by 168
    rows): d = 128 runs both products of every chunk on rb_gemm_tn_h, d = 64
    the library GEMM pair."""
    from datamining_recblr_amd import kernels, scoring

    inp, r64, r32 = _case(c, R.ROWS_IGNORED)
    seq, W, tgt = _dev(inp, cuda)
    with kernels.kernel_timing() as t:
        got = _backward(lambda s, w: scoring.item_cross_entropy_rows(s, w, tgt, chunk_rows=256),
                        seq, W)
    names = [r[0] for r in t.records]
    assert names.count("rb_item_ce_fwd_h_rows") == 3, names
    if c[3] == 128:
        assert names.count("rb_item_ce_probs_h_both_rows") == 3, names
        assert "rb_item_ce_probs_h_rows" not in names and len(tn_gemm_calls) == 6, (names, tn_gemm_calls)
    else:
        assert names.count("rb_item_ce_probs_h_rows") == 3, names
        assert "rb_item_ce_probs_h_both_rows" not in names and not tn_gemm_calls, (names, tn_gemm_calls)
    assert not got["dseq"][list(R.ROWS_IGNORED)].any()
    _judge("autograd-rows", c, got, r64, r32)

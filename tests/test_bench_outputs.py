"""bench.py's plain run, --full switch and --dump-outputs.

CPU: the snapshot that pins the timed steps' starting state (the settle runs
a clock-dependent number of steps in between) and the size cap of the dumped
arrays.  GPU: one small plain run end to end — the headline keys, nothing of
the --full measurements, and the last step's arrays on disk."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_bench_launch import BENCH, ROOT, _env, _import_bench

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
# what only --full measures: absent (None) from a plain run's line
FULL_ONLY_KEYS = ("gemm", "optimizer", "kernels", "fixed_length", "device_lengths", "fused_grl",
                  "ffn_act", "adam", "bwd_order", "nt_kernel", "ddp_overhead", "dense_batch",
                  "all_positions_tail", "scan_fwd_only", "long_seq_bf16", "cpu_baseline",
                  "host_enqueue_ms_per_step")


def _train(model, opt, xs):
    for x in xs:
        opt.zero_grad(set_to_none=True)
        (torch.nn.functional.dropout(model(x), 0.5) ** 2).sum().backward()
        opt.step()


@pytest.mark.parametrize("warm", [0, 2])
def test_restore_replays_the_same_steps(warm):
    """After any number of steps in between, _restore puts parameters,
    optimizer state and the default generator back: the next steps repeat bit
    for bit.  warm = 0: the optimizer state did not exist at the snapshot."""
    b = _import_bench()
    torch.manual_seed(3)
    model = torch.nn.Linear(5, 4)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    xs = [torch.randn(7, 5) for _ in range(6)]
    _train(model, opt, xs[:warm])
    snap = b._snapshot(model, opt)
    _train(model, opt, xs[:2])
    first = [p.detach().clone() for p in model.parameters()]
    _train(model, opt, xs)          # the "settle": any count
    b._restore(snap, model, opt)
    _train(model, opt, xs[:2])
    for p, q in zip(model.parameters(), first):
        assert torch.equal(p, q)


def test_dump_outputs_float32_and_capped(tmp_path, monkeypatch):
    b = _import_bench()
    g = torch.Generator().manual_seed(0)
    arrays = {"loss": torch.tensor(1.5, dtype=torch.float64),
              "grad.w": torch.randn(300, 7, generator=g),
              "param.w": torch.randn(1000, generator=g)}
    b.dump_outputs(str(tmp_path / "a"), arrays)
    for name, t in arrays.items():
        x = np.load(tmp_path / "a" / (name + ".npy"))
        assert x.dtype == np.float32 and x.shape == tuple(t.shape)
        assert np.array_equal(x, t.to(torch.float32).numpy())
    # over the limit: a fixed sample of every array, the same from call to call
    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", 4000)
    b.dump_outputs(str(tmp_path / "b"), arrays)
    b.dump_outputs(str(tmp_path / "c"), arrays)
    files = sorted(glob.glob(str(tmp_path / "b" / "*.npy")))
    assert [os.path.basename(f) for f in files] == ["grad.w.npy", "loss.npy", "param.w.npy"]
    assert sum(np.load(f).nbytes for f in files) <= 4000
    for f in files:
        x, y = np.load(f), np.load(str(tmp_path / "c" / os.path.basename(f)))
        assert x.dtype == np.float32 and x.size >= 1 and np.array_equal(x, y)
    flat = arrays["param.w"].numpy()
    assert set(np.load(tmp_path / "b" / "param.w.npy").tolist()) <= set(flat.tolist())


@pytest.mark.gpu
def test_plain_run_line_and_dump(cuda, tmp_path):
    """A small plain run: the headline keys, --steps timed steps, none of the
    --full measurements, and loss / gradients / parameters of the last timed
    step as float32 arrays."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--settle-seconds", "0.2", "--batch", "96", "--seq-len", "20",
                        "--hidden", "32", "--n-items", "203", "--dump-outputs", str(out)],
                       env=_env(), capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    for k in HEADLINE_KEYS:
        assert line[k] is not None, k
    assert line["full"] is False and line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - 96 / (line["ms_per_step"] * 1e-3)) <= 0.01 * line["value"]
    for k in FULL_ONLY_KEYS:
        assert line[k] is None, k
    names = {os.path.basename(f)[:-4] for f in glob.glob(str(out / "*.npy"))}
    assert "loss" in names and "grad.item_embedding.weight" in names
    assert {n[5:] for n in names if n.startswith("grad.")} == \
        {n[6:] for n in names if n.startswith("param.")}
    total = 0
    for n in names:
        x = np.load(out / (n + ".npy"))
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        total += x.nbytes
    assert total <= 64 * 1000 * 1000
    assert np.load(out / "param.item_embedding.weight.npy").shape == (203, 32)
    assert np.abs(np.load(out / "grad.item_embedding.weight.npy")).max() > 0

"""bench.py's multi-rank launcher on the CPU (VERDICT r2 "next" 1): ``python bench.py --gpus N``
outside a torchrun environment starts N ranks itself (torch.distributed.run as a child process),
and rank 0's one JSON line reports the world size the process group actually had. ``--dry-run``
replaces the training step by a gloo all-reduce so the launcher, the rank environment, the
barrier + max-over-ranks timing and the strong-scaling batch split run without a GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args, timeout=180):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    env.pop("LOCAL_RANK", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p.returncode, lines, p.stderr


@pytest.mark.parametrize("n", [2, 4, 8])
def test_gpus_n_launches_n_ranks(n):
    rc, lines, err = _run("--gpus", str(n), "--dry-run", "--steps", "3", "--warmup", "1")
    assert rc == 0, err[-2000:]
    assert len(lines) == 1, lines  # rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == n and out["steps"] == 3 and out["warmup"] == 1
    assert out["scaling"] == "weak" and out["config"]["global_batch"] == 128 * n
    assert out["config"]["backend"] == "gloo"


def test_global_batch_is_split_over_ranks():
    rc, lines, err = _run("--gpus", "4", "--dry-run", "--steps", "2", "--warmup", "0", "--global-batch", "128")
    assert rc == 0, err[-2000:]
    out = json.loads(lines[0])
    assert out["scaling"] == "strong" and out["n_gpus"] == 4
    assert out["config"]["per_gpu_batch"] == 32 and out["config"]["global_batch"] == 128
    assert out["config"]["bn"] == "sync"


def test_global_batch_must_divide():
    rc, lines, err = _run("--gpus", "3", "--dry-run", "--steps", "1", "--warmup", "0", "--global-batch", "128")
    assert rc != 0 and not lines
    assert "not divisible" in err


def test_full_and_dump_options_are_accepted():
    rc, lines, err = _run("--dry-run", "--full", "--dump-outputs", "unused", "--steps", "2", "--warmup", "0")
    assert rc == 0, err[-2000:]
    assert json.loads(lines[0])["steps"] == 2
    rc, lines, err = _run("--dry-run", "--steps", "0")
    assert rc != 0 and not lines


def test_dump_outputs_writes_float_arrays_within_budget(tmp_path, monkeypatch):
    """dump_outputs on stand-in host tensors: one .npy per output, float32 kept, integer exponents as
    float64 and only the quantisers' entries, an array over its share of the budget as the same fixed
    sample every time."""
    import types

    import numpy as np
    import torch

    import bench
    g = torch.Generator().manual_seed(3)
    w = torch.randn(5000, generator=g)
    trainer = types.SimpleNamespace(
        flat=types.SimpleNamespace(w=w, a=torch.randn(40, generator=g)),
        ctx=types.SimpleNamespace(exps=torch.arange(-8, 8, dtype=torch.int32), quantizers=[None] * 11))
    model = types.SimpleNamespace(loss=torch.tensor([2.5]), logits=torch.randn(4, 10, generator=g))
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 5 * 4000)  # 1000 float32 per array
    outs = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), trainer, model)
        outs.append({f[:-4]: np.load(str(tmp_path / d / f)) for f in sorted(os.listdir(str(tmp_path / d)))})
    a, b = outs
    assert sorted(a) == ["exponents", "logits", "loss", "momentum", "weights"]
    assert all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in a)
    assert a["loss"].dtype == np.float32 and a["loss"].tolist() == [2.5]
    assert a["logits"].dtype == np.float32 and np.array_equal(a["logits"], model.logits.numpy())
    assert a["exponents"].dtype == np.float64 and a["exponents"].tolist() == list(range(-8, 3))
    assert a["weights"].dtype == np.float32 and a["weights"].shape == (1000,)
    assert np.isin(a["weights"], w.numpy()).all() and len(set(a["weights"].tolist())) == 1000
    assert sum(v.nbytes for v in a.values()) <= 5 * 4000


def test_single_process_dry_run():
    rc, lines, err = _run("--dry-run", "--steps", "2", "--warmup", "0")
    assert rc == 0, err[-2000:]
    assert json.loads(lines[0])["n_gpus"] == 1

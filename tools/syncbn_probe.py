#!/usr/bin/env python
"""What the layer-wise SyncBN path costs at world 1 over RCCL: launch and collective overhead only.

    python tools/syncbn_probe.py [--batch 256] [--steps 30] [--rounds 3] [--out FILE.json]

One process forms a one-rank nccl group and builds two data-parallel trainers of ImageNet_Resnet50 (8 bits,
16-bit gradients: BASELINE configs[3]'s per-GPU shape) on the same synthetic batch: one as it is, one with
``sync_batchnorm(model, force=True)``. Both run the exact int64 exchange and capture their step, collectives
included, into ONE HIP graph. After a warm-up the arms alternate, ``rounds`` windows of ``steps`` steps each,
every window timed with a host clock around work that ends in a device synchronise. At world 1 no byte
crosses xGMI: the difference is what 2 x 53 lbt_sums_fold launches and 2 x 53 one-rank all-reduces cost inside
the graph. Prints ms/step per round, medians, run-to-run spread and the difference; the cost at N > 1 is not
measured by this (or any) tool here.
"""
import argparse
import json
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _spread(v):
    return (max(v) - min(v)) / statistics.median(v) if len(v) > 1 else 0.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.distributed as dist
    from lbt_amd.dfxp.layers import Normalization_q
    from lbt_amd.distributed import sync_batchnorm
    from lbt_amd.models import ImageNet_Resnet50
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    assert torch.cuda.is_available(), "the probe needs the GPU"
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))

    calls = []
    real = dist.all_reduce

    def counted(t, *args, **kw):
        calls.append(int(t.numel()))
        return real(t, *args, **kw)

    def make(sync):
        ctx = DfxpContext(seed=3, world_size=1)
        m = ImageNet_Resnet50(8, grad_bits=16, weight_decay=1e-4, image=a.image, ctx=ctx)
        if sync:
            sync_batchnorm(m, force=True)
        return Trainer(m, lr=1e-2, momentum=0.9, batch_size=a.batch, use_graph=True, exchange=True)

    try:
        rng = np.random.default_rng(3)
        X = torch.from_numpy(((rng.integers(0, 256, size=(a.batch, a.image, a.image, 3)) - 127.5) / 128)
                             .astype(np.float32)).cuda()
        y = torch.from_numpy(rng.integers(0, 1000, size=a.batch).astype(np.int32)).cuda()
        arms = {"plain": make(False), "sync_bn": make(True)}
        counts = {}
        for name, tr in arms.items():
            assert tr.dp and tr._lw_exact and tr.capture_comm, (name, tr.dp, tr._lw_exact, tr.capture_comm)
            # one eager step: the collectives and folds a step issues, counted where Python issues them
            dist.all_reduce = counted
            del calls[:]
            try:
                tr._eager(X, y)
            finally:
                dist.all_reduce = real
            counts[name] = {"collectives_per_step": len(calls), "int64_per_step": sum(calls)}
            for _ in range(5):  # captures the step, then replays it
                tr.step(X, y)
            assert tr._graphs is not None and tr._graphs[1] is None, "the step must be one graph"
        torch.cuda.synchronize()
        norms = [l for l in arms["sync_bn"].model._walk() if isinstance(l, Normalization_q)]

        def window(tr, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                tr.step(X, y)
            torch.cuda.synchronize()
            return 1000.0 * (time.perf_counter() - t0) / n

        rows = {k: [] for k in arms}
        for _ in range(a.rounds):
            for name, tr in arms.items():  # alternate the arms
                rows[name].append(window(tr, a.steps))
        report = {"host": socket.gethostname(), "device": torch.cuda.get_device_name(0), "batch": a.batch,
                  "image": a.image, "steps_per_window": a.steps, "rounds": a.rounds, "world": 1, "backend": "nccl",
                  "normalization_layers": len(norms), "bn_channels": sum(n.C for n in norms),
                  "fold_launches_per_step": 2 * len(norms), "arms": {}}
        for name, v in rows.items():
            report["arms"][name] = dict(counts[name], ms_per_step=v, median_ms=statistics.median(v), spread=_spread(v))
            print("%-8s ms/step %s   median %.4f   spread %.2f%%   collectives/step %d (%d int64)"
                  % (name, " ".join("%.4f" % t for t in v), statistics.median(v), 100 * _spread(v),
                     counts[name]["collectives_per_step"], counts[name]["int64_per_step"]), flush=True)
        d = report["arms"]["sync_bn"]["median_ms"] - report["arms"]["plain"]["median_ms"]
        report["sync_minus_plain_us_per_step"] = 1000.0 * d
        print("sync_bn - plain: %+.1f us per step (%d folds, %d statistics collectives; world 1: no bytes moved)"
              % (1000.0 * d, 2 * len(norms), counts["sync_bn"]["collectives_per_step"] - 1), flush=True)
        print(json.dumps(report), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(report, f, indent=1)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

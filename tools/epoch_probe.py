#!/usr/bin/env python
"""Time an epoch of ``Trainer.train()`` fed from host arrays against one fed from a ``DeviceDataset``
(lbt_amd/data.py), in one process on one GPU, and print JSON lines.

    python tools/epoch_probe.py [--samples 12800] [--batch 128] [--runs 3] [--captured-ms MS]

The workload is bench.py's: the ResNet-20 fused plan at B = 128, on a synthetic uint8 dataset of
CIFAR-shaped samples (12 800 = 100 steps an epoch). Each arm has a trainer of its own on its own copy of
the model; the host arm is the loop ``train()`` has always run (numpy gather, pageable upload,
``lbt_augment_flip_crop``), untouched. After one warm-up ``train()`` of each arm the arms alternate,
``--runs`` times each. A run is one ``train()`` call of two epochs: the first captures the step's graphs
again (``get_train_op`` resets the optimiser, as the reference does) and is not timed, the second is
timed between the two epochs' last batches -- ``train()``'s own logger line after batch 100 is the hook,
with a ``torch.cuda.synchronize()`` before each clock read. One line per run (ms per epoch and per step),
then a summary line with each arm's mean and spread, whether every device-resident run beat every host
run, and -- given ``--captured-ms``, the ms per step ``python bench.py`` printed at the same commit -- the
device arm's gap to the captured step alone.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


class EpochClock:
    """A Trainer logger that reads the clock at the epoch's last-batch line (device idle)."""

    def __init__(self):
        self.t = []

    def info(self, msg):
        if msg.startswith("Batch"):
            torch.cuda.synchronize()
            self.t.append(time.perf_counter())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=12800)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--captured-ms", type=float, default=None,
                    help="ms per step of the captured step alone (bench.py's ms_per_step at this commit)")
    args = ap.parse_args()
    steps = args.samples // args.batch
    if args.samples % args.batch or steps % 100:
        ap.error("--samples must be a multiple of 100 batches (the clock hook is the logger line every 100)")

    from lbt_amd.data import DeviceDataset
    from lbt_amd.fused import FusedResNet
    from lbt_amd.models import CIFAR10_Resnet20
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer

    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    rng = np.random.default_rng(0)
    Xu = rng.integers(0, 256, size=(args.samples, 32, 32, 3), dtype=np.uint8)
    y = rng.integers(0, 10, size=args.samples).astype(np.int32)
    ds = DeviceDataset(Xu, y, device=device)
    Xf = ds.host_float()

    def trainer(dataset):
        ctx = DfxpContext(device=device, seed=0)
        model = FusedResNet(CIFAR10_Resnet20(8, weight_decay=2e-4, ctx=ctx, grad_range=-6))
        tr = Trainer(model, dataset=dataset, lr=1e-2, momentum=0.9, batch_size=args.batch, n_epoch=2)
        tr.logger = EpochClock()
        return tr

    arms = {"host": trainer(((Xf, y), (Xf[:0], y[:0]))), "device": trainer((ds, None))}

    def run(name):
        tr = arms[name]
        tr.logger.t = []
        tr.train()
        t = tr.logger.t[-steps // 100 - 1:]  # the last batch of epoch 0 .. the last batch of epoch 1
        return 1000.0 * (t[-1] - t[0])

    for name in arms:  # warm-up: plans built, allocator and caches warm
        run(name)
    times = {name: [] for name in arms}
    for i in range(args.runs):
        for name in arms:
            ms = run(name)
            times[name].append(ms)
            print(json.dumps({"arm": name, "run": i, "steps": steps, "batch": args.batch,
                              "epoch_ms": round(ms, 3), "ms_per_step": round(ms / steps, 4)}), flush=True)
    out = {"summary": "train() epoch, host arrays vs DeviceDataset", "steps": steps, "batch": args.batch,
           "runs": args.runs}
    for name, ts in times.items():
        per = [t / steps for t in ts]
        out[name] = {"mean_ms_per_step": round(sum(per) / len(per), 4), "min": round(min(per), 4),
                     "max": round(max(per), 4)}
    out["every_device_run_faster"] = max(times["device"]) < min(times["host"])
    if args.captured_ms is not None:
        out["captured_step_ms"] = args.captured_ms
        out["device_gap_ms_per_step"] = round(out["device"]["mean_ms_per_step"] - args.captured_ms, 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

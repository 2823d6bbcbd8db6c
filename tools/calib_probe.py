#!/usr/bin/env python
"""Range calibration of a named model on one batch: per quantiser the default range, the calibrated range
(Trainer.calibrate) and the range after K ordinary steps from the defaults; the time of calibrate(); and the
scan kernel's time per tensor next to quantize_rows_kernel's on the same tensor.

    python tools/calib_probe.py --model CIFAR10_Resnet20 --batch 128 --steps 20
    python tools/calib_probe.py --model CIFAR10_Resnet20 --batch 128 --fused
    python tools/calib_probe.py --model ImageNet_Resnet50 --batch 256 --grad-bits 16 --steps 0 --largest 1
    python tools/calib_probe.py --model MNIST_Model --batch 128

Kernel times: device events around `--reps` back-to-back launches of one kernel on one tensor, the two
kernels alternating over `--rounds` rounds, the median round per launch. A tensor of a few thousand elements
measures the launch, not the kernel. One JSON line at the end (--table: the per-quantiser table before it).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def build(args, device, seed=0):
    from lbt_amd import models
    from lbt_amd.fused import FusedResNet
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    ctx = DfxpContext(device=device, seed=seed)
    if args.model.startswith("ImageNet"):
        model = getattr(models, args.model)(args.bits, grad_bits=args.grad_bits, weight_decay=args.weight_decay,
                                            image=args.image, ctx=ctx)
        classes = 1000
    else:
        kw = {} if "Resnet" in args.model else {"dropout": 0.5}
        model = getattr(models, args.model)(args.bits, weight_decay=args.weight_decay, ctx=ctx, **kw)
        classes = 10
    tr = Trainer(FusedResNet(model) if args.fused else model, lr=1e-2, momentum=0.9, batch_size=args.batch,
                 use_graph=True)
    return ctx, model, tr, classes


def batch(model, B, classes, device):
    g = torch.Generator().manual_seed(1000)
    x = ((torch.randint(0, 256, (B,) + tuple(model.input_shape[1:]), generator=g).float() - 127.5) / 128).to(device)
    y = torch.randint(0, classes, (B,), generator=g).to(torch.int32).to(device)
    return x.contiguous(), y


def fed_tensors(ctx, tr, X, y):
    """[(quantiser, tensor)] a calibration pass feeds, largest first (the layers' own reused buffers)."""
    seen = []
    feed = ctx.feed

    def spy(q, x):
        seen.append((q, x))
        return feed(q, x)
    ctx.feed = spy
    try:
        tr.calibrate(X, y)
    finally:
        del ctx.feed
    return sorted(seen, key=lambda qx: -qx[1].numel())


def kernel_times(q, x, reps, rounds):
    """(scan us, quantize us, the quantiser's kernel) per launch on tensor x."""
    from lbt_amd._lib import OUT_I8, OUT_I16, RANGE_BINS
    from lbt_amd.dfxp import ops
    table = torch.zeros(RANGE_BINS, dtype=torch.int64, device=x.device)
    kind = OUT_I8 if q.bits <= 8 else OUT_I16
    out = torch.empty(x.shape, dtype=ops.out_dtype(kind), device=x.device)
    rows, inner = ops.rows_inner(tuple(x.shape))
    name = "quantize_rows_kernel" if (inner % 4 == 0 and inner >= 64 and x.data_ptr() % 16 == 0) \
        else "quantize_generic_kernel"

    def run(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return 1000.0 * a.elapsed_time(b) / reps
    scan = lambda: ops.range_scan(x, table)  # noqa: E731
    quant = lambda: ops.quantize(x, q, kind, out=out)  # noqa: E731
    run(scan), run(quant)  # warm both
    ts, tq = [], []
    for _ in range(rounds):
        ts.append(run(scan))
        tq.append(run(quant))
    q.ctx.counts.zero_()
    return statistics.median(ts), statistics.median(tq), name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", required=True, help="a model builder of lbt_amd.models")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--bits", type=int, default=8)
    ap.add_argument("--grad-bits", type=int, default=None, help="ImageNet_Resnet*: the gradient quantisers' width")
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--weight-decay", type=float, default=2e-4)
    ap.add_argument("--fused", action="store_true", help="train through FusedResNet (CIFAR ResNets)")
    ap.add_argument("--steps", type=int, default=20, help="ordinary steps from the defaults (0: skip)")
    ap.add_argument("--largest", type=int, default=6, help="time the kernels on this many of the largest tensors")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--table", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("calib_probe needs the GPU: nothing is measured without one")
    device = torch.device("cuda", 0)

    ctx, model, tr, classes = build(args, device)
    X, y = batch(model, args.batch, classes, device)
    default = ctx.ranges()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = tr.calibrate(X, y)  # (ends in a device synchronise) first call: allocates the layers' buffers
    first = time.perf_counter() - t0
    t0 = time.perf_counter()
    tr.calibrate(X, y)
    again = time.perf_counter() - t0
    calibrated = ctx.ranges()

    after = None
    if args.steps > 0:  # the controller alone, from the defaults, on the same batch
        ctx2, _, tr2, _ = build(args, device)
        for _ in range(args.steps):
            tr2.step(X, y)
        torch.cuda.synchronize()
        after = ctx2.ranges()

    kernels = []
    for q, x in fed_tensors(ctx, tr, X, y)[: args.largest]:
        ts, tq, name = kernel_times(q, x, args.reps, args.rounds)
        kernels.append({"quantiser": q.name, "elements": x.numel(), "scan_us": round(ts, 2), "quantize_us": round(tq, 2),
                        "quantize_kernel": name, "scan_GBps": round(4e-3 * x.numel() / ts, 1)})

    if args.table:
        print("%-44s %8s %10s %s" % ("quantiser", "default", "calibrated", "after %d steps" % args.steps))
        for name in default:
            mark = "kept" if name in res["kept"] else ("unfed" if name in res["unfed"] else "")
            print("%-44s %8d %10d %s %s" % (name, default[name], calibrated[name],
                                            "" if after is None else "%6d" % after[name], mark))
    dist = [abs(after[k] - calibrated[k]) for k in res["set"]] if after is not None else []
    print(json.dumps({
        "model": args.model, "batch": args.batch, "bits": args.bits, "grad_bits": args.grad_bits, "fused": args.fused,
        "quantisers": len(default), "set": len(res["set"]), "kept": len(res["kept"]), "unfed": len(res["unfed"]),
        "calibrate_first_ms": round(1000 * first, 2), "calibrate_ms": round(1000 * again, 2),
        "grad_ranges": sorted({v for k, v in res["set"].items() if k.endswith("grad_range")}),
        "steps": args.steps, "after_steps_max_distance": max(dist) if dist else None,
        "after_steps_at_calibrated": sum(d == 0 for d in dist) if dist else None,
        "kernels": kernels, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()

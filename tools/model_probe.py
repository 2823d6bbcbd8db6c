#!/usr/bin/env python
"""Time one captured training step of a named model by graph replay (bench.py's method: W untimed
steps, then K steps between device synchronisations, one host clock around them), and print one JSON
line. For the models bench.py does not cover (the plain models of models.py:57-368).

    python tools/model_probe.py --model CIFAR10_VGG_Model --batch 128 --steps 40 --warmup 10
    LBT_DROPOUT_FUSE=0 python tools/model_probe.py --model CIFAR10_VGG_Model --batch 128   # the A/B's other arm
    python tools/model_probe.py --model CIFAR10_VGG_Model --batch 128 --layers            # + per-layer shares

--layers adds an eager pass after the timed region: device events around every top-level layer's
forward and backward (the launches of one layer, not a kernel trace), as milliseconds per step and
as a share of their sum.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def batches(n, B, shape, seed, device):
    g = torch.Generator().manual_seed(seed)
    xs = [((torch.randint(0, 256, (B,) + tuple(shape), generator=g).float() - 127.5) / 128).to(device)
          for _ in range(n)]
    ys = [torch.randint(0, 10, (B,), generator=g).to(torch.int32).to(device) for _ in range(n)]
    return xs, ys


def layer_times(model, x, y, reps):
    """[(label, ms per step)] of every top-level layer's forward and backward, eager."""
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    acc = {}

    def timed(label, fn, arg):
        a, b = ev(), ev()
        a.record()
        out = fn(arg)
        b.record()
        acc.setdefault(label, []).append((a, b))
        return out
    names = ["%02d %s" % (i, getattr(l, "name", type(l).__name__)) for i, l in enumerate(model.layers)]
    for _ in range(reps):
        model.ctx.zero_sums()
        model.ctx.fill_noise_tables()
        h = x
        for n, l in zip(names, model.layers):
            h = timed(n + " fwd", l.forward, h)
        model.logits = h
        model.compute_loss(y)
        g = model.dlogits
        for n, l in reversed(list(zip(names, model.layers))):
            g = timed(n + " bwd", l.backward, g)
        model.ctx.counts.zero_()  # no update runs here
    torch.cuda.synchronize()
    return [(k, sum(a.elapsed_time(b) for a, b in v) / reps) for k, v in acc.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", required=True, help="a model class or builder of lbt_amd.models")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--bits", type=int, default=8)
    ap.add_argument("--dropout", type=float, default=0.5)
    ap.add_argument("--weight-decay", type=float, default=2e-4)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--layers", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("model_probe needs the GPU: nothing is measured without one")

    from lbt_amd import models
    from lbt_amd.dfxp import layers
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    device = torch.device("cuda", 0)
    ctx = DfxpContext(device=device, seed=0)
    model = getattr(models, args.model)(args.bits, dropout=args.dropout, weight_decay=args.weight_decay, ctx=ctx)
    xs, ys = batches(4, args.batch, model.input_shape[1:], 1000, device)
    tr = Trainer(model, lr=1e-2, momentum=0.9, batch_size=args.batch, use_graph=not args.eager)
    tr.init_model()
    tr.prepare(xs[0], ys[0])
    for i in range(args.warmup):
        tr.step(xs[i % 4], ys[i % 4])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        tr.step(xs[i % 4], ys[i % 4])
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    out = {"model": args.model, "batch": args.batch, "bits": args.bits, "dropout": args.dropout,
           "dropout_fuse": int(layers.DROPOUT_FUSE), "graph": not args.eager, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": round(1000.0 * el / args.steps, 4),
           "samples_per_s": round(args.batch * args.steps / el, 1), "loss": float(model.loss.item()),
           "device": torch.cuda.get_device_name(0)}
    if args.layers:
        lt = layer_times(model, xs[0], ys[0], 5)
        total = sum(ms for _, ms in lt)
        out["eager_layers_ms"] = round(total, 4)
        out["layers"] = {k: [round(ms, 4), round(ms / total, 4)] for k, ms in lt}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

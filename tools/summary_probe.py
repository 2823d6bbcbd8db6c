#!/usr/bin/env python
"""What the device-recorded training summaries cost: a ResNet-20 trainer without them next to one with
``summary_every=100``, on synthetic batches at B = 128, in one process.

    python tools/summary_probe.py [--batch 128] [--steps 1000] [--rounds 3] [--every 100] [--out FILE.json]

Both trainers (same seed, same batch buffers) are warmed up until each holds every graph it replays; then
the two arms alternate, `rounds` windows of `steps` steps each, every window timed with a host clock
around work that ends in a device synchronise. The second arm's windows hold steps / every recording steps
(their share of the window is the amortised cost). A recording step alone is timed on a third trainer
with ``summary_every=1`` against the plain arm's step in the same way, and the two summary launches on
their own between device events (captured back to back into one graph). Prints per-arm ms/step per round,
medians and run-to-run spread ((max - min) / median), the recording step's time, and one decoded record.
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
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--every", type=int, default=100)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    from lbt_amd.fused import FusedResNet
    from lbt_amd.models import CIFAR10_Resnet20
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    assert torch.cuda.is_available(), "the probe needs the GPU"
    if a.steps % a.every:
        ap.error("--steps must be a multiple of --every (whole windows hold the same number of recording steps)")

    def make(every):
        ctx = DfxpContext(seed=3)
        return Trainer(FusedResNet(CIFAR10_Resnet20(8, weight_decay=2e-4, ctx=ctx)), lr=1e-2, momentum=0.9,
                       batch_size=a.batch, use_graph=True, summary_every=every)

    rng = np.random.default_rng(3)
    X = torch.from_numpy(((rng.integers(0, 256, size=(a.batch, 32, 32, 3)) - 127.5) / 128).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, 10, size=a.batch).astype(np.int32)).cuda()
    arms = {"plain": make(0), "summary_every=%d" % a.every: make(a.every), "summary_every=1": make(1)}
    early = []
    for tr in arms.values():  # every graph an arm replays is captured here, outside the timed windows
        tr.prepare(X, y)
        for _ in range(2 * a.every if tr.summary_every > 1 else 20):
            tr.step(X, y)
        early = tr.summaries() or early
    torch.cuda.synchronize()

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
            tr.summaries()  # (outside the window: the ring never overflows)
    report = {"host": socket.gethostname(), "device": torch.cuda.get_device_name(0), "batch": a.batch,
              "steps_per_window": a.steps, "rounds": a.rounds, "arms": {}}
    for name, v in rows.items():
        report["arms"][name] = {"ms_per_step": v, "median_ms": statistics.median(v), "spread": _spread(v)}
        print("%-20s ms/step %s   median %.4f   spread %.1f%%" % (name, " ".join("%.4f" % t for t in v),
                                                                 statistics.median(v), 100 * _spread(v)), flush=True)
    plain = report["arms"]["plain"]["median_ms"]
    rec = report["arms"]["summary_every=1"]["median_ms"]
    report["recording_step_ms"] = rec
    report["recording_step_extra_us"] = 1000.0 * (rec - plain)
    report["amortised_extra_us_per_step"] = 1000.0 * (rec - plain) / a.every
    print("a recording step: %.4f ms (plain %.4f ms, + %.1f us); amortised over %d steps: %.3f us per step"
          % (rec, plain, 1000.0 * (rec - plain), a.every, 1000.0 * (rec - plain) / a.every), flush=True)

    # the two launches alone: record + commit captured 20 times back to back, between device events
    tr = arms["summary_every=1"]
    rec_l, com_l = tr.model._summary_launches(tr._summary(tr.model))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(20):
                rec_l()
                com_l()
        for _ in range(3):
            g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(200):
            g.replay()
        e1.record(s)
        e1.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    report["record_plus_commit_us"] = 1000.0 * e0.elapsed_time(e1) / (20 * 200)
    print("lbt_summary_record + lbt_summary_commit, back to back in a graph: %.2f us per pair"
          % report["record_plus_commit_us"], flush=True)
    r = early[0]  # the first record of the warm-up (the same batch over and over soon stops being a sane run)
    brief = {k: r[k] for k in ("step", "batch", "loss", "accuracy")}
    tags = sorted(r["scalars"])
    brief["scalars"] = {t: r["scalars"][t] for t in tags[:12]}
    brief["n_scalars"] = len(tags)
    worst = max((v for v in r["overflow"].values() if v is not None), key=lambda v: v[2])
    brief["highest_overflow_rate"] = [k for k, v in r["overflow"].items() if v == worst][0], worst
    report["record"] = r
    print("one record (first 12 of %d scalars): %s" % (len(tags), json.dumps(brief)), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()

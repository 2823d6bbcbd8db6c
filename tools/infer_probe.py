#!/usr/bin/env python
"""Time the captured testing-mode forward of ResNet-20 against a training-mode forward.

    python tools/infer_probe.py --parent-tree DIR [--batches 128,1000] [--rounds 3] [--out FILE.json]

DIR is a checkout of the commit to compare with, built (its own ``lbt_amd/liblbt_dfxp.so``). For every batch
size the probe alternates child processes: this tree's ``FusedResNet(model, inference=True).forward`` and
DIR's training-mode ``FusedResNet(model).forward``, `rounds` times each. A child captures the whole forward
into one HIP graph and times replays between two device events (no host gaps in the window); it also times
the stage-1 (16 channels) and stage-3 (64 channels) ``lbt_conv_fwd_fused_i8`` launches on their own, each
captured `reps` times back to back into a graph. The report holds every round's figures, their medians and
the run-to-run spread of each configuration ((max - min) / median over its rounds): a difference between
the two configurations inside that spread is not a difference.

    python tools/infer_probe.py --child MODE --tree DIR --batch B     (one measurement; prints one JSON line)
"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fused_launches(plan):
    """{input channels: the first lbt_conv_fwd_fused_i8 launch of that stage} of a built plan."""
    out = {}
    for f in plan._fwd:
        if getattr(f, "kname", "") != "conv_fwd_fused_kernel":
            continue
        desc = f.__defaults__[1][0]._obj  # the launch's lbt_conv_fwd
        out.setdefault(int(desc.d.Cin), f)
    return out


def _time_graph(torch, run, reps, replays):
    """us per run(): run captured `reps` times into one HIP graph, replayed `replays` times between events."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(reps):
                run()
        for _ in range(3):
            g.replay()  # warm
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(replays):
            g.replay()
        e1.record(s)
        e1.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    return 1000.0 * e0.elapsed_time(e1) / (reps * replays)


def child(mode, tree, batch):
    sys.path.insert(0, os.path.abspath(tree))
    import numpy as np
    import torch
    from lbt_amd.fused import FusedResNet
    from lbt_amd.models import CIFAR10_Resnet20
    from lbt_amd.runtime import DfxpContext
    assert torch.cuda.is_available(), "the probe needs the GPU"
    ctx = DfxpContext(seed=3)
    gm = CIFAR10_Resnet20(8, weight_decay=2e-4, ctx=ctx)
    plan = FusedResNet(gm, inference=True) if mode == "inference" else FusedResNet(gm)
    rng = np.random.default_rng(3)
    x = torch.from_numpy(((rng.integers(0, 256, size=(batch, 32, 32, 3)) - 127.5) / 128).astype(np.float32)).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # builds the plan, allocates every buffer, loads the code objects
        for _ in range(3):
            plan.forward(x)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    res = {"mode": mode, "batch": batch, "host": socket.gethostname(), "device": torch.cuda.get_device_name(0),
           "launches": len(plan._fwd + plan._hfwd),
           "forward_us": _time_graph(torch, lambda: plan.forward(x), 4, 300)}
    for cin, f in sorted(_fused_launches(plan).items()):
        if cin in (16, 64):
            res["stage%d_fused_us" % (1 if cin == 16 else 3)] = _time_graph(torch, f, 20, 500)
    print(json.dumps(res), flush=True)


def _spread(v):
    return (max(v) - min(v)) / statistics.median(v) if len(v) > 1 else 0.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", choices=["inference", "training"])
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--parent-tree")
    ap.add_argument("--batches", default="128,1000")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per child process")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.tree, a.batch)
    if not a.parent_tree:
        ap.error("--parent-tree is required")
    configs = [("inference", ROOT), ("training (parent)", a.parent_tree)]
    report = {"batches": {}}
    for B in [int(b) for b in a.batches.split(",")]:
        rows = {name: [] for name, _ in configs}
        for _ in range(a.rounds):
            for name, tree in configs:  # alternate the two configurations
                cmd = [sys.executable, os.path.abspath(__file__), "--child", name.split()[0], "--tree", tree, "--batch", str(B)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
                if r.returncode != 0:  # nothing more is started on the GPU after a failed child
                    sys.stderr.write(r.stdout + r.stderr)
                    raise SystemExit("child %r failed with status %d" % (name, r.returncode))
                rows[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
                print("# %-17s %s" % (name, r.stdout.strip().splitlines()[-1]), flush=True)
        summary = {}
        for name, rs in rows.items():
            keys = [k for k in rs[0] if k.endswith("_us")]
            summary[name] = {"launches": rs[0]["launches"], "rounds": rs,
                             "median_us": {k: statistics.median(r[k] for r in rs) for k in keys},
                             "spread": {k: _spread([r[k] for r in rs]) for k in keys}}
        report["batches"][str(B)] = summary
        report["host"], report["device"] = rs[0]["host"], rs[0]["device"]
        for k in summary["inference"]["median_us"]:
            i, t = summary["inference"], summary["training (parent)"]
            print("B=%-5d %-16s inference %8.2f us (spread %4.1f%%)   parent training %8.2f us (spread %4.1f%%)   ratio %.3f"
                  % (B, k[:-3], i["median_us"][k], 100 * i["spread"][k], t["median_us"][k], 100 * t["spread"][k],
                     i["median_us"][k] / t["median_us"][k]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()

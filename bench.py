#!/usr/bin/env python
"""bench.py -- train-step samples/s of ResNet-20 / CIFAR-10, 8-bit DFXP, on 1..8 MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--global-batch B [--bn sync|local]]
                    [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps and prints the result line. ``--full`` adds what takes
runs of its own: the live roofline of the dominant kernel and the CPU baseline (the oracle's step on the
host). ``--dump-outputs DIR`` writes what the last timed step left (loss, logits, parameters, momentum,
DFXP exponents) as ``DIR/<name>.npy``; with the same arguments the inputs are the same from run to run.

A step is one ``Trainer.step`` (reference trainer.py:157): forward, mean softmax-CE, manual
backward through all 192 DFXP quantisers, MomentumOptimizer update and the update_range
collection, on a synthetic CIFAR-shaped batch already resident in HBM. Data parallel runs are
one process per GPU over RCCL: ``--gpus N`` without a torchrun environment starts the N rank
processes itself (torch.distributed.run as a child process, before this process touches the GPU).
Default: 128 images per GPU (weak scaling) and one RCCL all-reduce of the exact gradient
numerators + overflow counters per step, captured in the step's HIP graph. ``--global-batch B``:
strong scaling, B/N images per GPU; with ``--bn sync`` (its default) every BatchNorm takes the
whole-batch moments of the reference (dynamic_fixed_point.py:588) through exact all-reduces of the
integer statistics inside the step, so the N-GPU step computes the 1-GPU step on B images.
Rank 0 prints ONE JSON line (see DESIGN.md "Measurement").
"""
import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

METRIC = "train-step samples/sec, ResNet-20 CIFAR-10 8-bit DFP, 1/2/4/8 MI355X"
# BASELINE.json configs[3]: not the headline metric, a workload of its own
METRIC_R50 = "train-step samples/sec, ResNet-50 ImageNet-shape 8-bit W/A 16-bit grad DFP"
METRIC_W4 = "train-step samples/sec, ResNet-20 CIFAR-10 4-bit W / 8-bit A,G DFP"  # configs[4]


def synthetic_batches(n, B, seed, device):
    """x = (randint(0,256,[B,32,32,3]) - 127.5)/128 fp32 NHWC, labels randint(0,10)."""
    g = torch.Generator().manual_seed(seed)
    xs, ys = [], []
    for _ in range(n):
        x = ((torch.randint(0, 256, (B, 32, 32, 3), generator=g).float() - 127.5) / 128).to(device)
        y = torch.randint(0, 10, (B,), generator=g).to(torch.int32).to(device)
        xs.append(x.contiguous())
        ys.append(y)
    return xs, ys


def synthetic_imagenet(n, B, seed, device, image=224, classes=1000):
    g = torch.Generator().manual_seed(seed)
    xs, ys = [], []
    for _ in range(n):
        x = ((torch.randint(0, 256, (B, image, image, 3), generator=g).float() - 127.5) / 128).to(device)
        xs.append(x.contiguous())
        ys.append(torch.randint(0, classes, (B,), generator=g).to(torch.int32).to(device))
    return xs, ys


def cpu_baseline_r50(seconds=15.0, batch=1):
    """The oracle's ResNet-50 step (16-bit gradients) on the host, B=1 per step."""
    from oracle import resnet as oresnet
    try:
        from threadpoolctl import threadpool_info
        cores = max([i.get("num_threads", 1) for i in threadpool_info()] + [1])
    except Exception:  # pragma: no cover
        cores = os.cpu_count() or 1
    m = oresnet.build_resnet50(bits=8, grad_bits=16, weight_decay=1e-4)
    rng = np.random.default_rng(0)
    params = {}
    for name, owner in m.params():
        if name.endswith("/W"):
            shp = owner.ksize if hasattr(owner, "ksize") else (owner.in_units, owner.units)
            fan = float(np.prod(shp[:-1]))
            params[name] = rng.uniform(-np.sqrt(3 / fan), np.sqrt(3 / fan), size=shp).astype(np.float32)
        elif name.endswith("/g"):
            params[name] = np.ones(owner.C, np.float32)
        else:
            params[name] = np.zeros(owner.C, np.float32)
    state = dict(params=params, accum={k: np.zeros_like(v) for k, v in params.items()},
                 ranges=oresnet.init_ranges(m), step=0)
    x = ((rng.integers(0, 256, size=(batch, 224, 224, 3)) - 127.5) / 128).astype(np.float32)
    y = rng.integers(0, 1000, size=batch)
    n, t0 = 0, time.perf_counter()
    while True:
        _, state, _ = oresnet.train_step(m, state, x, y)
        n += 1
        el = time.perf_counter() - t0
        if el >= seconds:
            break
    return {"value": round(n * batch / el, 3), "unit": "samples/s", "cores": int(cores), "kind": "port",
            "sample": "%d oracle ResNet-50 train steps (numpy restatement), B=%d, 224x224, %.1f s" % (n, batch, el)}


def cpu_baseline(seconds=15.0, batch=128):
    """The oracle's ResNet-20 step (reference-semantics CPU restatement, numpy) on the host."""
    from oracle import resnet as oresnet
    try:
        from threadpoolctl import threadpool_info
        cores = max([i.get("num_threads", 1) for i in threadpool_info()] + [1])
    except Exception:  # pragma: no cover
        cores = os.cpu_count() or 1
    m = oresnet.build_resnet((3, 3, 3), 8, 2e-4)
    rng = np.random.default_rng(0)
    params = {}
    for name, owner in m.params():
        if name.endswith("/W"):
            shp = owner.ksize if hasattr(owner, "ksize") else (owner.in_units, owner.units)
            fan = float(np.prod(shp[:-1]))
            params[name] = rng.uniform(-np.sqrt(3 / fan), np.sqrt(3 / fan), size=shp).astype(np.float32)
        elif name.endswith("/g"):
            params[name] = np.ones(owner.C, np.float32)
        else:
            params[name] = np.zeros(owner.C, np.float32)
    state = dict(params=params, accum={k: np.zeros_like(v) for k, v in params.items()},
                 ranges=oresnet.init_ranges(m), step=0)
    x = ((rng.integers(0, 256, size=(batch, 32, 32, 3)) - 127.5) / 128).astype(np.float32)
    y = rng.integers(0, 10, size=batch)
    oresnet.train_step(m, state, x, y)  # warm-up
    n, t0 = 0, time.perf_counter()
    while True:
        _, state, _ = oresnet.train_step(m, state, x, y)
        n += 1
        el = time.perf_counter() - t0
        if el >= seconds:
            break
    return {"value": round(n * batch / el, 2), "unit": "samples/s", "cores": int(cores), "kind": "port",
            "sample": "%d oracle train steps (numpy restatement of dynamic_fixed_point/models/trainer), "
                      "ResNet-20 B=%d, %.1f s" % (n, batch, el)}


def _launch_ranks(n):
    """``--gpus N`` outside a torchrun environment: run this script under torch.distributed.run with
    N local ranks as a CHILD process and return its exit status (rank 0's JSON line goes to our
    stdout). Called before anything initialises the GPU, so no process that touched it execs."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC (RCCL peer buffers)
    return subprocess.call(cmd, env=env)


def _timed_region(step, steps, warmup, world, sync, device):
    """W untimed steps, then exactly K steps between barrier + synchronize on both sides; the MAX over
    ranks of the elapsed time."""
    for i in range(warmup):
        step(i)
    sync()
    if world > 1:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for i in range(steps):
        step(i)
    sync()
    if world > 1:
        dist.barrier()
    sync()
    el = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([el], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
    return el


def _exchange_report(trainer, model, world, reps=20):
    """The N>1 line's audit fields: the process group's size and backend, whether the
    collectives ran inside the step's graph, the exchange buffer's bytes, the collectives per step, and
    the exchange all-reduce timed EAGERLY, once, after the timed loop (reps back to back between a
    barrier and a synchronize, max over ranks) -- a cost estimate for the in-graph collective, which
    the timed steps include. The buffer is rewritten by the next step's backward, so summing it here
    changes nothing."""
    buf = trainer.xbuf if trainer.xbuf is not None else trainer.comm
    nsync = 0
    if getattr(model, "sync_bn", False):
        nsync = sum(1 for ops_ in (getattr(model, "_fwd", None), getattr(model, "_bwd", None)) if ops_
                    for op in ops_ if getattr(op, "kname", "") == "allreduce")
    rep = {"world_size": dist.get_world_size(), "backend": dist.get_backend(),
           "collectives_in_graph": bool(getattr(trainer, "capture_comm", False)),
           "bytes": int(buf.numel() * buf.element_size()) if buf is not None else 0,
           "dtype": str(buf.dtype).replace("torch.", "") if buf is not None else None,
           "collectives_per_step": 1 + nsync, "syncbn_collectives_per_step": nsync}
    if buf is not None:
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        for _ in range(reps):
            trainer._exchange()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        t = torch.tensor([el], dtype=torch.float64, device=buf.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        rep["eager_allreduce_us"] = round(float(t.item()) / reps * 1e6, 2)
        rep["eager_reps"] = reps
    return rep


DUMP_BUDGET_BYTES = 64 * 1000 * 1000  # --dump-outputs: the files' array data in all
DUMP_SAMPLE_SEED = 20


def dump_outputs(path, trainer, model):
    """--dump-outputs: what the last timed step left with its caller, one ``<name>.npy`` each: the loss and
    logits of that step's batch, the updated parameters and momentum accumulators (the flat buffers, in
    grads_and_vars order) and every quantiser's exponent. float32 as computed; the integer exponents as
    float64. An array over its share of the budget (ResNet-50's parameters) is written as a fixed sample:
    the elements at sorted indices drawn without replacement by numpy's PCG64 from DUMP_SAMPLE_SEED."""
    os.makedirs(path, exist_ok=True)
    arrays = {"loss": model.loss, "weights": trainer.flat.w, "momentum": trainer.flat.a,
              "exponents": trainer.ctx.exps[:len(trainer.ctx.quantizers)]}
    if getattr(model, "logits", None) is not None:
        arrays["logits"] = model.logits
    share = DUMP_BUDGET_BYTES // len(arrays)
    for name, t in arrays.items():
        a = t.detach().cpu().numpy()
        a = a.astype(np.float32 if a.dtype == np.float32 else np.float64, copy=False)
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(a.size, share // a.itemsize, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a))


def _dry_run(args, world, rank, backend, strong):
    if backend != "gloo":
        raise SystemExit("--dry-run runs on the gloo backend (CPU)")
    if world > 1:
        dist.init_process_group("gloo")
        world, rank = dist.get_world_size(), dist.get_rank()
    buf = torch.ones(1024, dtype=torch.int64)

    def step(i):
        if world > 1:
            dist.all_reduce(buf)
            buf.fill_(1)
    el = _timed_region(step, args.steps, args.warmup, world, lambda: None, "cpu")
    per = args.global_batch // world if strong else (args.batch or 128)
    if rank == 0:
        print(json.dumps({"metric": "dry-run (launcher plumbing, no measurement)", "value": None, "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1000.0 * el / args.steps, 4),
                          "scaling": "strong" if strong else "weak",
                          "config": {"global_batch": per * world, "per_gpu_batch": per, "backend": backend,
                                     "bn": args.bn or ("sync" if strong else "local"),
                                     }}), flush=True)
    if world > 1:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1,
                    help="GPUs (= ranks) of this node; without WORLD_SIZE in the environment the ranks are "
                         "launched by this script")
    ap.add_argument("--global-batch", type=int, default=None,
                    help="strong scaling: this many images per step over all GPUs (B/N per GPU)")
    ap.add_argument("--bn", choices=("sync", "local"), default=None,
                    help="BatchNorm statistics over the whole batch (sync, exact integer all-reduces inside "
                         "the step: the reference's semantics) or per GPU (local, standard DDP). Default: sync "
                         "with --global-batch, local otherwise")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=None,
                    help="images per GPU (default 128 = BASELINE configs[1]; resnet50: 256, the usual per-GPU "
                         "ImageNet batch -- configs[3] names none; measured 2.65K / 3.38K / 3.85K / 4.15K "
                         "samples/s at 32 / 64 / 128 / 256)")
    ap.add_argument("--eager", action="store_true", help="no HIP graph (diagnostics)")
    ap.add_argument("--layerwise", action="store_true", help="run the Layer_q path instead of the fused plan")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure what takes runs of its own: the live roofline of "
                         "the dominant kernel and the CPU baseline (one GPU only); off by default")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one left (loss, logits, parameters, momentum, "
                         "DFXP exponents) as DIR/<name>.npy, float32 / float64, at most 64 MB in all")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the roofline")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher / process-group plumbing only (CPU, gloo): each step is one all-reduce of a "
                         "small CPU tensor; used by the CPU tests, never a measurement")
    ap.add_argument("--grad-range", type=int, default=-6,
                    help="ResNet-20: the gradient quantisers' initial exponent I (the layers' grad_range argument, "
                         "dynamic_fixed_point.py:225,321,541,628). -6 (default): a run that trains; 2: the reference's "
                         "default, with which this random-label run diverges (DESIGN 4). The work per step is the same")
    ap.add_argument("--workload", choices=("resnet20", "resnet50", "resnet20w4"), default="resnet20",
                    help="resnet50: BASELINE configs[3], ImageNet-shape, 16-bit gradients (layer path); "
                         "resnet20w4: configs[4], 4-bit packed weights")
    args = ap.parse_args()
    r50 = args.workload == "resnet50"
    w4 = args.workload == "resnet20w4"
    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(_launch_ranks(args.gpus))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print("bench.py: --gpus %d but the launcher started %d ranks; reporting the ranks that ran"
              % (args.gpus, world), file=sys.stderr)
    strong = args.global_batch is not None
    if strong:
        if r50:
            ap.error("--global-batch: ResNet-20 workloads only")
        if args.global_batch % world:
            ap.error("--global-batch %d is not divisible by %d ranks" % (args.global_batch, world))
        args.batch = args.global_batch // world
    elif args.batch is None:
        args.batch = 256 if r50 else 128
    if args.bn == "sync" and args.layerwise:
        ap.error("--bn sync: the fused plan only (the layer-wise executor takes per-GPU statistics)")
    bn_mode = args.bn or ("sync" if strong and not args.layerwise else "local")
    if bn_mode == "sync" and r50:
        ap.error("--bn sync: ResNet-20 workloads only")
    # LBT_DIST_BACKEND=gloo + LBT_SHARE_GPU=1: a rehearsal of the N-rank path with every rank on the
    # box's GPUs round-robin (one-GPU boxes); the measured configuration is RCCL, one GPU per rank
    backend = os.environ.get("LBT_DIST_BACKEND", "gloo" if args.dry_run else "nccl")
    if args.dry_run:
        return _dry_run(args, world, rank, backend, strong)
    if os.environ.get("LBT_SHARE_GPU") == "1":
        local = local % max(1, torch.cuda.device_count())
    elif world > 1 and torch.cuda.device_count() < world:
        print("bench.py: %d ranks but %d visible GPUs (LBT_SHARE_GPU=1 rehearses on fewer)"
              % (world, torch.cuda.device_count()), file=sys.stderr)
        sys.exit(2)
    if world > 1:
        torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
        world = dist.get_world_size()
        rank = dist.get_rank()
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)

    from lbt_amd.models import CIFAR10_Resnet20
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer

    ctx = DfxpContext(device=device, seed=0, world_size=world)
    if r50:
        from lbt_amd.models import ImageNet_Resnet50
        model = ImageNet_Resnet50(8, grad_bits=16, weight_decay=1e-4, ctx=ctx)
        xs, ys = synthetic_imagenet(4, args.batch, 1000 + rank, device)
    else:
        model = CIFAR10_Resnet20(8, weight_decay=2e-4, ctx=ctx, weight_bits=4 if w4 else None,
                                 grad_range=args.grad_range)
        if not args.layerwise:
            from lbt_amd.fused import FusedResNet
            model = FusedResNet(model, sync_bn=bn_mode == "sync")
        if strong:  # every rank takes its shard of the same global batches
            gx, gy = synthetic_batches(4, args.global_batch, seed=1000, device="cpu")
            b = args.batch
            xs = [x[rank * b:(rank + 1) * b].contiguous().to(device) for x in gx]
            ys = [y[rank * b:(rank + 1) * b].contiguous().to(device) for y in gy]
        else:
            xs, ys = synthetic_batches(4, args.batch, seed=1000 + rank, device=device)
    trainer = Trainer(model, lr=1e-2, momentum=0.9, batch_size=args.batch, use_graph=not args.eager)
    trainer.init_model()
    for x_, y_ in zip(xs, ys):  # every batch buffer's graph captured before the warm-up and timed steps
        trainer.prepare(x_, y_)

    el = _timed_region(lambda i: trainer.step(xs[i % 4], ys[i % 4]), args.steps, args.warmup, world,
                       torch.cuda.synchronize, device)
    loss = float(model.loss.item())
    if args.dump_outputs and rank == 0:  # before anything below runs another step
        dump_outputs(args.dump_outputs, trainer, model)

    out = {
        "metric": METRIC_R50 if r50 else (METRIC_W4 if w4 else METRIC),
        "value": round(args.batch * world * args.steps / el, 2),
        "unit": "samples/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(1000.0 * el / args.steps, 4),
        "higher_is_better": True,
        "scaling": "strong" if strong else "weak",
        "vs_baseline": None,
        "dtype": "int8",
        "data": "synthetic CIFAR-10-shaped batches (uniform uint8 pixels, (p-127.5)/128), random-init weights",
        "config": {"workload": "ResNet-20 CIFAR-10 8-bit DFXP W/A/G train step (fwd+bwd+SGD-momentum+range update)",
                   "global_batch": args.batch * world, "per_gpu_batch": args.batch, "image": [32, 32, 3],
                   "parallelism": "dp%d" % world, "hip_graph": not args.eager,
                   "executor": "layerwise" if args.layerwise else "fused", "final_loss": round(loss, 4),
                   "grad_range": args.grad_range},
    }
    if world > 1 or strong:
        out["config"]["backend"] = backend if world > 1 else None
        out["config"]["bn"] = bn_mode if world > 1 else "local"
        out["config"]["collectives_in_graph"] = bool(getattr(trainer, "capture_comm", False))
        out["config"]["shared_gpu"] = os.environ.get("LBT_SHARE_GPU") == "1"
    if world > 1:
        out["config"]["exchange"] = _exchange_report(trainer, model, world)
    if w4:
        out["config"]["workload"] = "ResNet-20 CIFAR-10, 4-bit DFXP weights (packed, 2 per byte), 8-bit A/G, train step"
    if r50:
        out["data"] = "synthetic ImageNet-shaped batches (224x224x3 uniform uint8 pixels, (p-127.5)/128), random-init"
        out["config"] = {"workload": "ResNet-50 ImageNet-shape, 8-bit DFXP W/A, 16-bit DFXP gradients, train step",
                         "global_batch": args.batch * world, "per_gpu_batch": args.batch, "image": [224, 224, 3],
                         "classes": 1000, "parallelism": "dp%d" % world, "hip_graph": not args.eager,
                         "executor": "layerwise", "final_loss": round(loss, 4)}
    # the timed run trains on 4 synthetic batches from random init with the reference's default ranges;
    # it can diverge (identically in the oracle) without changing the work per step: flagged here
    ncls = 1000 if r50 else 10
    out["config"]["loss_diverged"] = bool(not math.isfinite(loss) or loss > 10 * math.log(ncls))
    if args.full and rank == 0 and world == 1 and not args.no_roofline:
        from lbt_amd.roofline import measure_dominant
        tf = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles",
                          "pmc_traffic_resnet50.json" if r50 else "pmc_traffic.json")
        out["roofline"] = measure_dominant(trainer, xs[0], ys[0], traffic_file=tf)
        sb = out["roofline"].get("step_algorithmic_bytes")
        if sb:  # the whole step against the same roofline: algorithmic bytes per step / step time
            gbs = sb / (el / args.steps) / 1e9
            out["roofline"]["step"] = {"achieved": round(gbs, 1), "frac": round(gbs / out["roofline"]["peak"], 4),
                                       "algorithmic_bytes": sb, "ms_per_step": out["ms_per_step"]}
            if not r50 and args.batch == 128:
                # the same step time against SURVEY 8(d)'s 1.09 GB model of a configs[1] step (GEMM
                # operands + every quantiser's fp32 read / code write): a different byte count
                from lbt_amd.roofline import SURVEY_STEP_BYTES_R20
                sg = SURVEY_STEP_BYTES_R20 / (el / args.steps) / 1e9
                out["roofline"]["step"]["frac_survey_model"] = round(sg / out["roofline"]["peak"], 4)
                out["roofline"]["step"]["survey_model_bytes"] = int(SURVEY_STEP_BYTES_R20)
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline_r50(args.cpu_seconds) if r50 else cpu_baseline(args.cpu_seconds, args.batch)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

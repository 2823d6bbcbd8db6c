#!/usr/bin/env python
"""Time the ImageNet input launch (``lbt_batch_resized_crop`` and, with colour jitter,
``lbt_batch_resized_crop_jitter``; lbt_amd/data.py) against a plain copy of its output and against the step it
feeds, in one process on one GPU.

    python tools/input_probe.py [--samples 1024] [--reps 20] [--iters 30] [--step-iters 10] [--no-step]
                                [--ragged] [--out profiles/input/resized_crop.json]

A synthetic uint8 store of ``--samples`` 256 x 256 x 3 images is resampled to 224 x 224. Per batch size
(256: one GPU's batch, 32: a rank's shard of it) and per mode (the training transform, the validation
transform), ``--reps`` launches -- each on another permutation slice and step counter -- are captured into
one HIP graph, so that the host's share of a launch (argument checks, ctypes) is not in the figure; after
warm-up replays, ``--iters`` replays are timed with device events, and the time per launch is a replay's
over ``--reps``; the median and the fastest are reported. The yardstick is ``copy_`` of as many fp32 bytes
as the launch writes, timed the same way: the launch stores what the copy stores and reads a quarter of
the bytes or fewer, so the ratio is what the resampling costs. Beside the training arm, in the same form: the
training transform with ``ColorJitter(0.4, 0.4, 0.4)`` (``jitter``: the statistics pass and the output pass) and
with contrast off (``jitter_no_contrast``: the output pass alone), each also as a ratio to the training arm of
this run. Then
``ImageNet_Resnet50`` at B = 256 (bench.py's ResNet-50 workload) is captured and ``--step-iters`` steps are
timed, for the launch's share of a step. One JSON document, printed and written to ``--out``.

``--ragged`` adds a store of images of their own sizes (``RaggedCropDataset``: short side 256, aspect ratios
uniform over [3/4, 16/9], as many images and the same labels and permutation) and times ``lbt_batch_ragged_crop``
-- training, validation, and training with ``ColorJitter(0.4, 0.4, 0.4)`` -- beside the uniform launch's same
three arms in the same run, each also as a ratio to its uniform arm. No step is timed; the default ``--out`` is
profiles/input/ragged_crop.json.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def timed(fn, iters, warmup=5):
    """ms of each of ``iters`` calls of fn(i), between device events around the call alone."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ms = []
    for i in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(warmup + i)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def timed_graph(fn, reps, iters, warmup=3):
    """ms per call of fn(i), i = 0 .. reps - 1, captured once into a graph and replayed."""
    fn(0)  # outside the capture first: code objects loaded
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(reps):
            fn(i)
    return [t / reps for t in timed(lambda i: g.replay(), iters, warmup)]


def stats(ms):
    return {"median_us": round(1000 * statistics.median(ms), 2), "min_us": round(1000 * min(ms), 2),
            "max_us": round(1000 * max(ms), 2), "n": len(ms)}


def ragged_images(rng, n):
    """n uint8 images of short side 256 with aspect ratios W / H uniform over [3/4, 16/9]: a store resized
    offline as the reference's validation transform resizes (short side to 256, aspect ratio kept)."""
    images = []
    for r in rng.uniform(3 / 4, 16 / 9, size=n):
        H, W = (int(round(256 / r)), 256) if r < 1 else (256, int(round(256 * r)))
        images.append(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8))
    return images


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--no-step", action="store_true", help="skip the ResNet-50 step")
    ap.add_argument("--ragged", action="store_true",
                    help="time lbt_batch_ragged_crop (+ _jitter) on images of short side 256 beside the uniform launch")
    ap.add_argument("--out", default=None, help="default: profiles/input/resized_crop.json, or ragged_crop.json")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join("profiles", "input", "ragged_crop.json" if args.ragged else "resized_crop.json")

    from lbt_amd.data import RaggedCropDataset, ResizedCropDataset

    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    rng = np.random.default_rng(0)
    X = rng.integers(0, 256, size=(args.samples, 256, 256, 3), dtype=np.uint8)
    y = rng.integers(0, 1000, size=args.samples).astype(np.int32)
    ds = ResizedCropDataset(X, y, MEAN, STD, 224, device=device)
    perm = ds.upload_index(torch.from_numpy(rng.permutation(args.samples)))
    arms = {"train": ds, "validation": ds}  # arm -> its dataset (the jitter arms hold the store again)
    jitter_arms = {"jitter": "train", "jitter_no_contrast": "train"}  # arm -> the arm it is a ratio to
    for name, cj in (("jitter", (0.4, 0.4, 0.4)), ("jitter_no_contrast", (0.4, 0.0, 0.4))):
        arms[name] = ResizedCropDataset(X, y, MEAN, STD, 224, device=device, color_jitter=cj)
    summary = "lbt_batch_resized_crop (+ _jitter), 256x256x3 uint8 store -> 224x224x3 fp32"
    if args.ragged:
        del arms["jitter_no_contrast"], jitter_arms["jitter_no_contrast"]
        images = ragged_images(rng, args.samples)
        rag = RaggedCropDataset(images, y, MEAN, STD, 224, device=device)
        arms.update({"ragged_train": rag, "ragged_validation": rag,
                     "ragged_jitter": RaggedCropDataset(images, y, MEAN, STD, 224, device=device,
                                                        color_jitter=(0.4, 0.4, 0.4))})
        jitter_arms["ragged_jitter"] = "ragged_train"
        summary += "; lbt_batch_ragged_crop (+ _jitter), short side 256, W / H in [3/4, 16/9], mean %d x %d" % tuple(
            np.rint(rag.shapes.mean(axis=0)))
        del images

    out = {"summary": summary, "samples": args.samples,
           "launches_per_graph": args.reps, "device": torch.cuda.get_device_name(0), "launch": {}}
    for B in (256, 32):
        oX = torch.empty((B,) + ds.sample_shape, dtype=torch.float32, device=device)
        oy = torch.empty(B, dtype=torch.int32, device=device)
        src = torch.empty_like(oX).normal_()
        slots = args.samples // B

        def launch(i, arm):
            lo = (i % slots) * B
            arms[arm].batch(oX, oy, idx=perm[lo:lo + B], augment=not arm.endswith("validation"), seed=1, counter=i,
                            check=False)

        row = {"output_bytes": oX.numel() * 4}
        for arm in arms:
            row[arm] = stats(timed_graph(lambda i: launch(i, arm), args.reps, args.iters))
        row["copy"] = stats(timed_graph(lambda i: oX.copy_(src), args.reps, args.iters))
        for mode in arms:
            row[mode]["ratio_to_copy"] = round(row[mode]["median_us"] / row["copy"]["median_us"], 3)
            row[mode]["output_GBps"] = round(row["output_bytes"] / row[mode]["median_us"] / 1000, 1)
        for mode, of in jitter_arms.items():
            row[mode]["ratio_to_train"] = round(row[mode]["median_us"] / row[of]["median_us"], 3)
        if args.ragged:
            for mode in ("train", "validation", "jitter"):
                row["ragged_" + mode]["ratio_to_uniform"] = round(row["ragged_" + mode]["median_us"] / row[mode]["median_us"], 3)
        out["launch"]["B%d" % B] = row
        del oX, src

    if not args.no_step and not args.ragged:
        from lbt_amd.models import ImageNet_Resnet50
        from lbt_amd.runtime import DfxpContext
        from lbt_amd.trainer import Trainer
        B = 256
        ctx = DfxpContext(device=device, seed=0)
        model = ImageNet_Resnet50(8, grad_bits=16, weight_decay=1e-4, ctx=ctx)
        tr = Trainer(model, lr=1e-2, momentum=0.9, batch_size=B, use_graph=True)
        tr.init_model()
        xb = torch.empty((B,) + ds.sample_shape, dtype=torch.float32, device=device)
        yb = torch.empty(B, dtype=torch.int32, device=device)
        ds.batch(xb, yb, idx=perm[:B], augment=True, seed=1, counter=0, check=False)
        tr.prepare(xb, yb)
        step = stats(timed(lambda i: tr.step(xb, yb), args.step_iters, warmup=3))
        out["step"] = {"workload": "ImageNet_Resnet50, B = 256, captured", **step}
        t = out["launch"]["B256"]["train"]["median_us"]
        out["step"]["input_share_of_step"] = round(t / (step["median_us"] + t), 5)
        for mode in jitter_arms:
            t = out["launch"]["B256"][mode]["median_us"]
            out["step"][mode + "_share_of_step"] = round(t / (step["median_us"] + t), 5)

    text = json.dumps(out, indent=1)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

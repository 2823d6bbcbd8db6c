"""The sharded test loop's metrics in numpy (test helper, CPU only).

Restates what include/lbt_dfxp.h documents next to ``lbt_eval_tally`` and what ``lbt_amd.trainer.decode_tally``
makes of its rows: the correct count is numpy's argmax (the first maximum, as tf.argmax / torch.argmax), a
batch's accuracy the fp32 quotient of two exactly represented integers, its loss the fixed-point sum times
2^-32 over the batch size in float64 rounded to fp32 once (lbt_step_finish), and the loop's result the
float64 mean of those fp32 values in batch order (trainer.py:166-190 as lbt_amd.trainer restates it).
"""
import numpy as np


def correct(logits, labels):
    """Samples whose first maximum is the label."""
    return int((np.argmax(np.asarray(logits), axis=1) == np.asarray(labels)).sum())


def decode(rows, sizes):
    """(mean accuracy, mean loss) from per-batch (correct, loss_fx) rows and batch sizes."""
    accs, losses = [], []
    for (c, fx), nb in zip(rows, sizes):
        accs.append(np.float32(c) / np.float32(nb))
        losses.append(np.float32(np.float64(fx) * np.float64(2.0) ** -32 / np.float64(nb)))
    if not sizes:
        return 0.0, 0.0
    a = l = np.float64(0.0)
    for x, z in zip(accs, losses):  # in batch order, one addition at a time
        a, l = a + np.float64(x), l + np.float64(z)
    return float(a / len(sizes)), float(l / len(sizes))


def shard(nb, world, rank):
    """Rows of a batch of nb that rank takes: equal contiguous shards in rank order."""
    assert nb % world == 0
    return list(range(nb))[rank * (nb // world):(rank + 1) * (nb // world)]

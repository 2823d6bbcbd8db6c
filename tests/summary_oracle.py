"""The training-summary record (lbt_summary_record + lbt_summary_commit) in numpy (test helper, CPU only).

Restates the layout documented next to ``lbt_summary`` in include/lbt_dfxp.h from the sources a step
holds: integers are exact, the parameter sums are ``math.fsum`` (the correctly rounded sum; a kernel's
double sum is compared with it inside the recursive-summation bound, ``sum_bound``), the accuracy count is
numpy's argmax (the first maximum, as tf.argmax / torch.argmax).
"""
import math

import numpy as np

NSHARD, CSTRIDE, HEADER = 32, 32, 32


def record_bytes(nslots, nparams):
    return HEADER + 16 * nslots + 8 * nparams


def scratch_bytes(nparams, max_seg, chunk):
    return 8 * nparams * max(1, (max_seg + chunk - 1) // chunk)


def shard_totals(counts, nslots):
    """(c1, c2) per slot from the counter array [slot][NSHARD][CSTRIDE] (int32 wrap-around, as the kernels')."""
    c = np.asarray(counts, dtype=np.int32).reshape(-1, NSHARD, CSTRIDE)[:nslots]
    with np.errstate(over="ignore"):
        return c[:, :, 0].sum(axis=1, dtype=np.int32), c[:, :, 1].sum(axis=1, dtype=np.int32)


def correct(logits, labels):
    """Samples whose lowest-index maximum is the label."""
    z = np.asarray(logits, dtype=np.float32)
    return int((np.argmax(z, axis=1).astype(np.int64) == np.asarray(labels, dtype=np.int64)).sum())


def segment_sums(w, seg_off):
    """math.fsum of every segment [seg_off[p], seg_off[p + 1]) of w."""
    w = np.asarray(w, dtype=np.float32)
    return [math.fsum(w[a:b].astype(np.float64).tolist()) for a, b in zip(seg_off[:-1], seg_off[1:])]


def sum_bound(w, seg_off):
    """n * 2^-53 * sum |w_i| per segment: the recursive-summation bound for double (any fixed order)."""
    w = np.abs(np.asarray(w, dtype=np.float32).astype(np.float64))
    return [(b - a) * 2.0 ** -53 * math.fsum(w[a:b].tolist()) for a, b in zip(seg_off[:-1], seg_off[1:])]


def record(step, exps, counts, nelem, sums, batch, n_correct, loss):
    """The bytes of one record from its fields (sums: the doubles to store)."""
    ns, npar = len(exps), len(sums)
    buf = np.zeros(record_bytes(ns, npar), dtype=np.uint8)
    buf[0:8] = np.array([step], dtype=np.uint64).view(np.uint8)
    buf[8:16] = np.array([batch, n_correct], dtype=np.int32).view(np.uint8)
    buf[16:20] = np.array([loss], dtype=np.float32).view(np.uint8)
    buf[20:32] = np.array([ns, npar, 0], dtype=np.int32).view(np.uint8)
    c1, c2 = shard_totals(counts, ns) if ns else (np.zeros(0, np.int32), np.zeros(0, np.int32))
    o = HEADER
    for arr, dt in ((exps, np.int32), (c1, np.int32), (c2, np.int32), (nelem, np.float32)):
        buf[o:o + 4 * ns] = np.asarray(arr, dtype=dt).view(np.uint8)
        o += 4 * ns
    buf[o:] = np.asarray(sums, dtype=np.float64).view(np.uint8)
    return buf


def fields(raw, nslots, nparams):
    """A record's raw fields (no names): dict of step, batch, correct, loss, exps, c1, c2, nelem, sums."""
    b = np.frombuffer(bytes(raw), dtype=np.uint8)
    assert b.size == record_bytes(nslots, nparams)
    o = HEADER
    return dict(step=int(b[0:8].view(np.uint64)[0]), batch=int(b[8:12].view(np.int32)[0]),
                correct=int(b[12:16].view(np.int32)[0]), loss=b[16:20].view(np.float32)[0],
                nslots=int(b[20:24].view(np.int32)[0]), nparams=int(b[24:28].view(np.int32)[0]),
                exps=b[o:o + 4 * nslots].view(np.int32), c1=b[o + 4 * nslots:o + 8 * nslots].view(np.int32),
                c2=b[o + 8 * nslots:o + 12 * nslots].view(np.int32),
                nelem=b[o + 12 * nslots:o + 16 * nslots].view(np.float32), sums=b[o + 16 * nslots:].view(np.float64))

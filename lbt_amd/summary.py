"""Training summaries recorded on the device (lbt_summary_record / lbt_summary_commit, csrc/summary.hip).

The reference gives every Conv2d_q / Dense_q / Normalization_q / Rescale_q a set of ``tf.summary.scalar``s
(``dynamic_fixed_point.py:180-190, 275-285, 372-382, 578-582, 667-675``) and fetches them with loss and
accuracy every 100th batch (``trainer.py:148-155``). Here a recording step writes one fixed-size record into
a ring in device memory from inside its captured graph; ``SummaryRing.drain`` copies the ring once and
``decode`` turns a record into a dict keyed by the reference's tags. The record layout is documented next
to ``lbt_summary`` in ``include/lbt_dfxp.h``; this module holds its host side only (numpy, no GPU call
outside ``SummaryRing``).
"""
import json
import os

import numpy as np

HEADER_BYTES = 32
# a parameter variable's summary tag (Rescale_q's gamma / beta are the reference's g / b)
MEAN_TAG = {"W": "W_mean", "b": "b_mean", "gamma": "g_mean", "beta": "b_mean"}


def record_bytes(nslots, nparams):
    """lbt_summary_record_bytes: header, four 4-byte arrays over the slots, one double per parameter."""
    return HEADER_BYTES + 16 * int(nslots) + 8 * int(nparams)


def scratch_bytes(nparams, max_seg, chunk=16384):
    """lbt_summary_scratch_bytes: one double per parameter and chunk of the longest segment."""
    return 8 * int(nparams) * max(1, -(-int(max_seg) // chunk))


def param_list(offsets):
    """[(layer name, variable, element count)] of FlatParams.offsets, the order of the record's sums."""
    return [(getattr(o, "name", ""), v, int(sz)) for o, v, _, sz in offsets]


def decode(raw, names, params):
    """One record (bytes / uint8 array of record_bytes(len(names), len(params))) as a dict.

    names: the quantisers' names in slot order (they are the reference's ``name_scope/var`` tags);
    params: ``param_list`` entries. Returns
      step, batch, correct, loss, accuracy (= correct / batch in fp32, as Model.accuracy),
      scalars     {tag: value}: every ``*_range`` -> int, ``<layer>/W_mean | b_mean | g_mean`` -> float32(sum / n)
      param_sums  {"<layer>/<variable>": the double sum}
      nelem       {quantiser name: elements seen this step}
      overflow    {quantiser name: (c1, c2, r1, r2)}, r = float32(c) / float32(nelem) as update_range
                  computes it; None for a slot that was not fed (nelem <= 0)."""
    buf = np.frombuffer(bytes(raw), dtype=np.uint8)
    ns, npar = len(names), len(params)
    if buf.size != record_bytes(ns, npar):
        raise ValueError("record of %d bytes, expected %d (%d slots, %d parameters)"
                         % (buf.size, record_bytes(ns, npar), ns, npar))
    step = int(buf[0:8].view(np.uint64)[0])
    batch, correct = (int(v) for v in buf[8:16].view(np.int32))
    loss = buf[16:20].view(np.float32)[0]
    rns, rnp = (int(v) for v in buf[20:28].view(np.int32))
    if (rns, rnp) != (ns, npar):
        raise ValueError("record holds %d slots / %d parameters, expected %d / %d" % (rns, rnp, ns, npar))
    o = HEADER_BYTES
    exps = buf[o:o + 4 * ns].view(np.int32)
    c1 = buf[o + 4 * ns:o + 8 * ns].view(np.int32)
    c2 = buf[o + 8 * ns:o + 12 * ns].view(np.int32)
    nelem = buf[o + 12 * ns:o + 16 * ns].view(np.float32)
    sums = buf[o + 16 * ns:].view(np.float64)
    scalars, overflow, nel = {}, {}, {}
    for i, name in enumerate(names):
        scalars[name] = int(exps[i])
        nel[name] = float(nelem[i])
        if nelem[i] > 0:
            r1, r2 = np.float32(c1[i]) / nelem[i], np.float32(c2[i]) / nelem[i]
            overflow[name] = (int(c1[i]), int(c2[i]), float(r1), float(r2))
        else:
            overflow[name] = None
    psums = {}
    for (layer, var, n), s in zip(params, sums):
        psums["%s/%s" % (layer, var)] = float(s)
        scalars["%s/%s" % (layer, MEAN_TAG[var])] = float(np.float32(s / n))
    acc = float(np.float32(correct) / np.float32(batch)) if batch > 0 else 0.0
    return {"step": step, "batch": batch, "correct": correct, "loss": float(loss), "accuracy": acc,
            "scalars": scalars, "param_sums": psums, "nelem": nel, "overflow": overflow}


def ring_slots(cursor, read, capacity):
    """The ring arithmetic: with `cursor` records committed and `read` of them handed out already, the
    ring slots of the unread records that still exist, oldest first, and how many were overwritten."""
    first = max(int(read), int(cursor) - int(capacity))
    return [k % capacity for k in range(first, int(cursor))], first - int(read)


def to_json(record):
    """One record as one JSON line (no newline); from_json restores it exactly (Python floats are written
    with repr precision; float32 values are exact doubles)."""
    return json.dumps(record, sort_keys=True)


def from_json(line):
    r = json.loads(line)
    r["overflow"] = {k: (None if v is None else (int(v[0]), int(v[1]), float(v[2]), float(v[3])))
                     for k, v in r["overflow"].items()}
    return r


def append_jsonl(path, records):
    """Append records to path (the reference's FileWriter(logdir + '/train'), trainer.py:72), one line each."""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "a") as f:
        for r in records:
            f.write(to_json(r) + "\n")


def read_jsonl(path):
    with open(path) as f:
        return [from_json(l) for l in f if l.strip()]


class SummaryRing:
    """The sink every plan of a Trainer records into: ring, cursor, chunk scratch and the parameter
    segment table in device memory (allocated once, outside any capture), and the host's read position."""

    def __init__(self, ctx, flat, capacity):
        import torch

        from . import _lib
        if int(capacity) <= 0:
            raise ValueError("summary_capacity must be positive, got %r" % (capacity,))
        self.ctx, self.capacity = ctx, int(capacity)
        self.names = [q.name for q in ctx.quantizers]
        self.params = param_list(flat.offsets)
        lib = _lib.load()
        ns, npar = len(self.names), len(self.params)
        self.max_seg = max([n for _, _, n in self.params] + [1])
        self.rec_bytes = int(lib.lbt_summary_record_bytes(ns, npar))
        dev = ctx.device
        self.ring = torch.zeros(self.capacity * self.rec_bytes, dtype=torch.uint8, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=dev)
        self.scratch = torch.zeros(max(1, int(lib.lbt_summary_scratch_bytes(npar, self.max_seg)) // 8),
                                   dtype=torch.float64, device=dev)
        offs = [off for _, _, off, _ in flat.offsets] + [flat.n]
        self.seg_off = torch.tensor(offs, dtype=torch.int64).to(dev)
        self.flat = flat
        self.read = 0
        self.dropped = 0

    def desc(self):
        """A lbt_summary with every shared field set; the plan fills logits / labels / batch / classes / loss."""
        from . import _lib
        c, s = self.ctx, _lib.Summary()
        s.exps, s.counts, s.nelem = c.exps.data_ptr(), c.counts.data_ptr(), c.nelem.data_ptr()
        s.nslots, s.nparams = len(self.names), len(self.params)
        s.w, s.seg_off, s.max_seg = self.flat.w.data_ptr(), self.seg_off.data_ptr(), self.max_seg
        s.step = c.step.data_ptr()
        s.ring, s.capacity = self.ring.data_ptr(), self.capacity
        s.cursor, s.scratch = self.cursor.data_ptr(), self.scratch.data_ptr()
        return s

    def drain(self):
        """Synchronise, copy the cursor and the ring once, decode the records committed since the last
        call (oldest first); those overwritten before being read are added to `dropped`."""
        import torch
        torch.cuda.synchronize(self.ctx.device)
        cursor = int(self.cursor.item())
        slots, lost = ring_slots(cursor, self.read, self.capacity)
        self.dropped += lost
        self.read = cursor
        if not slots:
            return []
        host = self.ring.cpu().numpy().reshape(self.capacity, self.rec_bytes)
        return [decode(host[k], self.names, self.params) for k in slots]

"""Training summaries recorded on the device: lbt_summary_record / lbt_summary_commit (csrc/summary.hip),
lbt_amd/summary.py and the Trainer's summary_every.

The yardstick is tests/summary_oracle.py (the record layout of include/lbt_dfxp.h restated in numpy).
Integers, exponents, element counts, the step, the loss and the accuracy count are compared exactly; a
parameter sum S against math.fsum F within |S - F| <= n * 2^-53 * sum |w_i| (recursive summation in double)."""
import ctypes
import logging
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import summary_oracle as SO
from lbt_amd import _lib
from lbt_amd import summary as S

F32 = np.float32
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = _lib.SUMMARY_CHUNK


# ------------------------------------------------------------------------------------ CPU
def test_summary_struct_layout_matches_c():
    """As tests/test_abi.py::test_struct_layouts_match_c, for lbt_summary."""
    fields = [f for f, _ in _lib.Summary._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lbt_dfxp.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(lbt_summary));', 'printf("chunk %d\\n", LBT_SUMMARY_CHUNK);']
    lines += ['printf("%s %%zu\\n", offsetof(lbt_summary, %s));' % (f, f) for f in fields]
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = dict(l.rsplit(" ", 1) for l in subprocess.check_output([exe], text=True).splitlines())
    assert int(out["size"]) == ctypes.sizeof(_lib.Summary)
    assert int(out["chunk"]) == CHUNK
    for f in fields:
        assert int(out[f]) == getattr(_lib.Summary, f).offset, f


def test_record_and_scratch_bytes_are_the_documented_formulas():
    lib = _lib.load()
    for ns, npar in ((0, 0), (1, 0), (0, 1), (70, 8), (161, 65), (1024, 500)):
        want = 32 + 16 * ns + 8 * npar
        assert lib.lbt_summary_record_bytes(ns, npar) == want == S.record_bytes(ns, npar) == SO.record_bytes(ns, npar)
    for npar, seg in ((0, 0), (3, 0), (3, 1), (8, CHUNK), (8, CHUNK + 1), (8, 70001), (161, 2359296)):
        want = 8 * npar * max(1, -(-seg // CHUNK))
        assert lib.lbt_summary_scratch_bytes(npar, seg) == want == S.scratch_bytes(npar, seg, CHUNK) \
            == SO.scratch_bytes(npar, seg, CHUNK)
    assert lib.lbt_summary_record_bytes(-1, 0) < 0 and lib.lbt_summary_scratch_bytes(-1, 5) < 0


def _fake_summary(**over):
    """A complete lbt_summary with fake non-NULL pointers (never dereferenced: rejected on the host first)."""
    p = 0x1000
    a = dict(exps=p, counts=p, nelem=p, nslots=4, nparams=2, w=p, seg_off=p, max_seg=100, logits=p, labels=p, batch=3,
             classes=10, loss=p, step=p, ring=p, capacity=3, cursor=p, scratch=p)
    a.update(over)
    s = _lib.Summary()
    for k, v in a.items():
        setattr(s, k, v)
    return s


EINVAL = [dict(capacity=0), dict(capacity=-3), dict(nslots=-1), dict(nparams=-1), dict(classes=0), dict(classes=-2),
          dict(ring=None), dict(cursor=None), dict(step=None), dict(batch=-1), dict(exps=None), dict(counts=None),
          dict(nelem=None), dict(w=None), dict(seg_off=None), dict(scratch=None), dict(max_seg=0), dict(logits=None),
          dict(labels=None), dict(nparams=1 << 20, max_seg=1 << 40)]


@pytest.mark.parametrize("over", EINVAL, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_summary_host_checks_return_einval(over):
    lib = _lib.load()
    s = _fake_summary(**over)
    assert lib.lbt_summary_record(ctypes.byref(s), None) == 1001
    assert lib.lbt_summary_commit(ctypes.byref(s), None) == 1001


def test_summary_null_descriptor_and_commit_without_loss():
    lib = _lib.load()
    assert lib.lbt_summary_record(None, None) == 1001 and lib.lbt_summary_commit(None, None) == 1001
    s = _fake_summary(loss=None)
    assert lib.lbt_summary_commit(ctypes.byref(s), None) == 1001


NAMES = ["conv1/W_range", "conv1/X_range", "conv1/grad_range", "bn/rescale/g_range", "bn/rescale/b_range", "fc/b_range"]


class _L:
    def __init__(self, name):
        self.name = name


def _hand_record():
    """A record assembled by hand from the header's layout (not through summary_oracle.record)."""
    exps = np.array([2, -3, 7, 0, -22, 1], dtype=np.int32)
    c1 = np.array([0, 5, (1 << 30) + 1, 7, 3, 9], dtype=np.int32)
    c2 = np.array([1, 50, (1 << 30) + 65, 8, 4, 9], dtype=np.int32)
    nelem = np.array([432, 49152, 3.0, 16, 0, 10], dtype=F32)
    sums = np.array([1.5, -0.001953125, 16.25, 1e-30, -3.0], dtype=np.float64)
    hdr = np.zeros(32, dtype=np.uint8)
    hdr[0:8] = np.array([(1 << 32) + 5], dtype=np.uint64).view(np.uint8)
    hdr[8:12] = np.array([37], dtype=np.int32).view(np.uint8)
    hdr[12:16] = np.array([11], dtype=np.int32).view(np.uint8)
    hdr[16:20] = np.array([2.302585], dtype=F32).view(np.uint8)
    hdr[20:24] = np.array([6], dtype=np.int32).view(np.uint8)
    hdr[24:28] = np.array([5], dtype=np.int32).view(np.uint8)
    raw = np.concatenate([hdr] + [a.view(np.uint8) for a in (exps, c1, c2, nelem, sums)])
    conv, resc, fc = _L("conv1"), _L("bn/rescale"), _L("fc")
    offsets = [(conv, "W", 0, 432), (resc, "gamma", 432, 16), (resc, "beta", 448, 16), (fc, "W", 464, 640),
               (fc, "b", 1104, 10)]
    return raw, S.param_list(offsets), (exps, c1, c2, nelem, sums)


def test_decode_of_a_hand_assembled_record():
    raw, params, (exps, c1, c2, nelem, sums) = _hand_record()
    assert raw.size == S.record_bytes(6, 5)
    r = S.decode(raw, NAMES, params)
    assert r["step"] == (1 << 32) + 5 and r["batch"] == 37 and r["correct"] == 11
    assert r["loss"] == float(F32(2.302585)) and r["accuracy"] == float(F32(11) / F32(37))
    for i, n in enumerate(NAMES):
        assert r["scalars"][n] == int(exps[i]) and isinstance(r["scalars"][n], int)
    # the overflow rates are float32 quotients of float32 operands (2^30 + 1 rounds before the division)
    assert r["overflow"]["conv1/grad_range"] == ((1 << 30) + 1, (1 << 30) + 65, float(F32((1 << 30) + 1) / F32(3.0)),
                                                  float(F32((1 << 30) + 65) / F32(3.0)))
    assert r["overflow"]["conv1/grad_range"][2] != ((1 << 30) + 1) / 3.0
    assert r["overflow"]["conv1/X_range"] == (5, 50, float(F32(5) / F32(49152)), float(F32(50) / F32(49152)))
    assert r["overflow"]["bn/rescale/b_range"] is None and r["nelem"]["bn/rescale/b_range"] == 0.0
    means = {"conv1/W_mean": (1.5, 432), "bn/rescale/g_mean": (-0.001953125, 16), "bn/rescale/b_mean": (16.25, 16),
             "fc/W_mean": (1e-30, 640), "fc/b_mean": (-3.0, 10)}
    for tag, (s, n) in means.items():
        assert r["scalars"][tag] == float(F32(s / n)), tag
    assert set(r["scalars"]) == set(NAMES) | set(means)
    assert r["param_sums"] == {"conv1/W": 1.5, "bn/rescale/gamma": -0.001953125, "bn/rescale/beta": 16.25,
                               "fc/W": 1e-30, "fc/b": -3.0}
    with pytest.raises(ValueError):
        S.decode(raw[:-8], NAMES, params)
    assert np.array_equal(SO.record((1 << 32) + 5, exps, _counts_with_totals(c1, c2), nelem, sums, 37, 11, 2.302585), raw)


def _counts_with_totals(c1, c2):
    """A counter array whose shard totals are c1 / c2 (everything in shard 5)."""
    c = np.zeros((len(c1), SO.NSHARD, SO.CSTRIDE), dtype=np.int32)
    c[:, 5, 0], c[:, 5, 1] = c1, c2
    return c


def test_ring_arithmetic():
    assert S.ring_slots(5, 0, 3) == ([2, 0, 1], 2)  # 5 commits into capacity 3: records 2, 3, 4; two lost
    assert S.ring_slots(5, 4, 3) == ([1], 0)
    assert S.ring_slots(5, 5, 3) == ([], 0)
    assert S.ring_slots(2, 0, 3) == ([0, 1], 0)
    assert S.ring_slots(3, 0, 3) == ([0, 1, 2], 0)
    assert S.ring_slots(1 << 40, (1 << 40) - 2, 1024) == ([1022, 1023], 0)
    assert S.ring_slots(0, 0, 1) == ([], 0)


def test_jsonl_round_trip(tmp_path):
    raw, params, _ = _hand_record()
    r = S.decode(raw, NAMES, params)
    path = str(tmp_path / "logs" / "train" / "summaries.jsonl")
    S.append_jsonl(path, [r])
    S.append_jsonl(path, [r, r])
    back = S.read_jsonl(path)
    assert len(back) == 3 and all(b == r for b in back)
    assert back[0]["overflow"]["bn/rescale/b_range"] is None and isinstance(back[0]["overflow"]["conv1/X_range"], tuple)


@pytest.fixture
def one_rank_group(tmp_path):
    import torch.distributed as dist
    own = not dist.is_initialized()
    if own:
        dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "pg"), rank=0, world_size=1)
    yield
    if own:
        dist.destroy_process_group()


def test_data_parallel_trainer_refuses_summaries_on_the_host(one_rank_group):
    from lbt_amd.models import MNIST_Model
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    with pytest.raises(NotImplementedError, match="summed across ranks"):
        Trainer(MNIST_Model(8, ctx=DfxpContext(device="cpu", world_size=1, rank=0)), exchange=True, summary_every=1)
    with pytest.raises(ValueError):
        Trainer(MNIST_Model(8, ctx=DfxpContext(device="cpu")), summary_every=-1)


# ------------------------------------------------------------------------------------ GPU, kernel level
class _Sink:
    """Ring, cursor, scratch and the per-launch sources of one lbt_summary on the device."""

    def __init__(self, nslots=0, nparams=0, max_seg=0, capacity=3):
        lib = _lib.load()
        self.ns, self.np, self.cap = nslots, nparams, capacity
        self.rb = lib.lbt_summary_record_bytes(nslots, nparams)
        self.ring = torch.full((capacity * self.rb,), 0xAB, dtype=torch.uint8, device=DEV)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.scratch = torch.full((max(1, lib.lbt_summary_scratch_bytes(nparams, max_seg) // 8),), float("nan"),
                                  dtype=torch.float64, device=DEV)
        self.step = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.loss = torch.zeros(1, dtype=torch.float32, device=DEV)
        s = self.s = _lib.Summary()
        s.nslots, s.nparams, s.max_seg, s.classes = nslots, nparams, max_seg, 1
        s.ring, s.capacity, s.cursor, s.scratch = self.ring.data_ptr(), capacity, self.cursor.data_ptr(), self.scratch.data_ptr()
        s.step, s.loss = self.step.data_ptr(), self.loss.data_ptr()

    def record(self):
        _lib.call("lbt_summary_record", ctypes.byref(self.s), _lib.stream())

    def commit(self):
        _lib.call("lbt_summary_commit", ctypes.byref(self.s), _lib.stream())

    def slot(self, k):
        torch.cuda.synchronize()
        return SO.fields(self.ring.cpu().numpy()[k * self.rb:(k + 1) * self.rb], self.ns, self.np)


@pytest.mark.gpu
def test_counters_are_summed_exactly_and_left_alone():
    """70 slots (more than one wave of slots, no multiple of 4 or 64), all 32 shards at random, the unused
    words of every shard's line filled too; slot 9 not fed (nelem = 0), slot 33's totals near 2^30 (odd: the
    float conversion of update_range rounds them, the record must not)."""
    ns = 70
    rng = np.random.default_rng(11)
    counts = rng.integers(0, 5000, size=(ns, SO.NSHARD, SO.CSTRIDE)).astype(np.int32)
    counts[33, :, 0] = (1 << 25) - 1 - rng.integers(0, 3, size=SO.NSHARD)
    counts[33, :, 1] = (1 << 25) - rng.integers(0, 2, size=SO.NSHARD)
    counts[33, 0, 0] -= (int(counts[33, :, 0].sum()) + 1) % 2  # an odd total near 2^30: no float32
    exps = rng.integers(-22, 8, size=ns).astype(np.int32)
    nelem = rng.integers(1, 1 << 22, size=ns).astype(F32)
    nelem[9] = 0
    k = _Sink(nslots=ns)
    d_counts, d_exps, d_nelem = (torch.from_numpy(a).to(DEV) for a in (counts, exps, nelem))
    k.s.counts, k.s.exps, k.s.nelem = d_counts.data_ptr(), d_exps.data_ptr(), d_nelem.data_ptr()
    k.step.fill_(12345678901)
    k.record()
    k.commit()
    f = k.slot(0)
    c1, c2 = SO.shard_totals(counts, ns)
    assert c1[33] % 2 == 1 and c1[33] > 1 << 29 and float(F32(c1[33])) != float(c1[33])
    assert np.array_equal(f["c1"], c1) and np.array_equal(f["c2"], c2)
    assert np.array_equal(f["exps"], exps) and np.array_equal(f["nelem"], nelem)
    assert (f["step"], f["batch"], f["correct"], f["nslots"], f["nparams"]) == (12345678901, 0, 0, ns, 0)
    assert np.array_equal(d_counts.cpu().numpy(), counts), "the record launch must not touch the counters"
    assert int(k.cursor.item()) == 1
    # the whole record against the oracle's bytes
    want = SO.record(12345678901, exps, counts, nelem, [], 0, 0, 0.0)
    assert np.array_equal(k.ring.cpu().numpy()[:k.rb], want)


SEG_SIZES = [1, 3, 16, 255, 256, 257, 4097, 70001]


def _param_values(seed):
    """Magnitudes 2^-20 .. 1 with both signs; the 256-element segment sums to nearly zero (pairs +v, -v in
    random positions, plus one tiny element)."""
    rng = np.random.default_rng(seed)
    n = sum(SEG_SIZES)
    w = (rng.choice([-1.0, 1.0], size=n) * rng.uniform(0.5, 1.0, size=n) * 2.0 ** rng.integers(-19, 1, size=n)).astype(F32)
    off = np.concatenate([[0], np.cumsum(SEG_SIZES)]).astype(np.int64)
    a = int(off[4])
    half = w[a:a + 127].copy()
    seg = np.concatenate([half, -half, np.array([2.0 ** -20, -(2.0 ** -21)], dtype=F32)])
    w[a:a + 256] = seg[rng.permutation(256)]
    return w, off


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_parameter_sums_within_the_double_bound_and_reproducible(shift):
    """Segments laid end to end (unaligned starts), the flat buffer itself starting `shift` floats past a
    16-byte boundary; 70001 elements span 5 chunks of LBT_SUMMARY_CHUNK."""
    assert CHUNK < 70001
    w, off = _param_values(3 + shift)
    store = torch.zeros(len(w) + 8, dtype=torch.float32, device=DEV)
    assert store.data_ptr() % 16 == 0
    dw = store[shift:shift + len(w)]
    dw.copy_(torch.from_numpy(w))
    d_off = torch.from_numpy(off).to(DEV)
    npar = len(SEG_SIZES)
    k = _Sink(nparams=npar, max_seg=max(SEG_SIZES))
    k.s.w, k.s.seg_off = dw.data_ptr(), d_off.data_ptr()
    k.record()
    k.commit()
    k.scratch.fill_(float("nan"))  # the second launch must rewrite every partial it folds
    k.record()
    k.commit()
    a, b = k.slot(0), k.slot(1)
    assert a["sums"].tobytes() == b["sums"].tobytes(), "two launches on the same data must give the same bits"
    F, bound = SO.segment_sums(w, off), SO.sum_bound(w, off)
    for p in range(npar):
        err = abs(float(a["sums"][p]) - F[p])
        print("segment %d n=%d sum=%r fsum=%r err=%.3e bound=%.3e" % (p, SEG_SIZES[p], a["sums"][p], F[p], err, bound[p]))
        assert err <= bound[p], (p, err, bound[p])
    # the CPU's own float64 sum stays inside the same bound (the bound is no artefact of the kernel's order)
    for p in range(npar):
        assert abs(float(w[off[p]:off[p + 1]].astype(np.float64).sum()) - F[p]) <= bound[p]
    assert abs(F[4]) < 1e-5 and np.array_equal(dw.cpu().numpy(), w)


def _accuracy_case(B, C, seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, C)).astype(F32)
    y = np.argmax(z, axis=1).astype(np.int32)
    hi = F32(9.5)
    # row 0: two maxima, lowest index wins -- the label is the lower one (correct)
    lo_i, hi_i = (3, C - 2) if C > 64 else (3, 7)
    z[0, lo_i] = z[0, hi_i] = hi
    y[0] = lo_i
    if B > 1:  # the same tie, labelled with the higher index (wrong)
        z[1] = z[0]
        y[1] = hi_i
    if B > 2:  # maximum at index 0, at the last index, and a tie inside one lane's stride (5 and 5 + 64)
        z[2, 0], y[2] = hi, 0
        z[3, C - 1], y[3] = hi, C - 1
        j = 69 if C > 69 else 6
        z[4, 5] = z[4, j] = hi
        y[4] = 5
    for b in range(5, B):  # the rest: about half of the labels wrong
        if b % 2:
            y[b] = (y[b] + 1 + b) % C
    return z, y


@pytest.mark.gpu
@pytest.mark.parametrize("B,C", [(1, 10), (37, 10), (5, 1000)])
def test_accuracy_count_takes_the_lowest_index_maximum(B, C):
    z, y = _accuracy_case(B, C, 100 + B)
    k = _Sink()
    dz, dy = torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV)
    k.s.logits, k.s.labels, k.s.batch, k.s.classes = dz.data_ptr(), dy.data_ptr(), B, C
    k.record()
    k.commit()
    f = k.slot(0)
    want = SO.correct(z, y)
    assert 0 < want <= B and (B < 2 or want < B)
    assert (f["batch"], f["correct"]) == (B, want)
    assert want == int((dz.argmax(dim=1).to(torch.int32) == dy).sum().item())  # Model.accuracy's count


@pytest.mark.gpu
def test_ring_wraps_and_the_loss_is_the_one_at_commit_time():
    k = _Sink(capacity=3)
    for i in range(5):
        k.step.fill_(i)
        k.loss.fill_(100.0 + i)
        k.record()
        k.loss.fill_(i + 0.5)  # (a fused plan's loss is written by the launch between the two)
        k.commit()
    assert int(k.cursor.item()) == 5
    for i in (2, 3, 4):
        f = k.slot(i % 3)
        assert f["step"] == i and f["loss"] == F32(i + 0.5)
    assert S.ring_slots(5, 0, 3) == ([2, 0, 1], 2)


# ------------------------------------------------------------------------------------ GPU, through the Trainer
B = 16


def _trainer(seed, fused=True, use_graph=True, **kw):
    """ResNet-20, 8 bits, as tests/test_device_data.py::_trainer."""
    from lbt_amd.fused import FusedResNet
    from lbt_amd.models import CIFAR10_Resnet20
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    ctx = DfxpContext(seed=seed)
    gm = CIFAR10_Resnet20(8, weight_decay=2e-4, ctx=ctx)
    return ctx, gm, Trainer(FusedResNet(gm) if fused else gm, lr=1e-2, momentum=0.9, batch_size=B, use_graph=use_graph,
                            **kw)


def _batches(n, seed=7, b=B):
    rng = np.random.default_rng(seed)
    xs = ((rng.integers(0, 256, size=(n, b, 32, 32, 3)) - 127.5) / 128).astype(F32)
    return torch.from_numpy(xs).to(DEV), torch.from_numpy(rng.integers(0, 10, size=(n, b)).astype(np.int32)).to(DEV)


def _bn_state(tr):
    return [t.cpu().numpy() for bn in tr._bn_layers() for t in (bn.X_mean_running, bn.X_var_running)]


def _assert_same_state(a, b):
    (ca, ta), (cb, tb) = a, b
    assert torch.equal(ta.flat.w, tb.flat.w) and torch.equal(ta.flat.a, tb.flat.a)
    assert ca.ranges() == cb.ranges() and torch.equal(ca.counts, cb.counts) and torch.equal(ca.step, cb.step)
    assert torch.equal(ca.nelem, cb.nelem)
    for x, y in zip(_bn_state(ta), _bn_state(tb)):
        assert np.array_equal(x, y)


MODES = [(True, True), (True, False), (False, True), (False, False)]
MODE_IDS = ["fused-graph", "fused-eager", "layerwise-graph", "layerwise-eager"]


@pytest.mark.gpu
@pytest.mark.parametrize("fused,graph", MODES, ids=MODE_IDS)
def test_recording_changes_nothing(fused, graph):
    xs, ys = _batches(5)
    ca, _, ta = _trainer(21, fused, graph)
    cb, _, tb = _trainer(21, fused, graph, summary_every=2)
    X, y = torch.empty_like(xs[0]), torch.empty_like(ys[0])  # one buffer pair: one graph per kind of step
    losses = []
    for tr in (ta, tb):
        ls = []
        for i in range(5):
            X.copy_(xs[i])
            y.copy_(ys[i])
            ls.append(tr.step(X, y).clone())
        losses.append(torch.cat(ls).cpu().numpy())
    assert losses[0].tobytes() == losses[1].tobytes()
    _assert_same_state((ca, ta), (cb, tb))
    recs = tb.summaries()
    assert [r["step"] for r in recs] == [1, 3] and tb.summary_dropped == 0  # the 2nd and 4th steps
    assert [r["loss"] for r in recs] == [float(losses[0][1]), float(losses[0][3])]
    assert ta.summaries() == [] and tb.summaries() == []
    if graph and fused:
        assert sorted(k[3] for k in tb._gcache) == [False, True] and len(ta._gcache) == 1


def _expected_tags(gm):
    """The reference's summary tags of this model's layers (dynamic_fixed_point.py:180-190, 275-285, 372-382,
    578-582, 667-675) without X_mean."""
    from lbt_amd import dynamic_fixed_point as L
    tags = set()
    for layer in gm._walk():
        if isinstance(layer, (L.Conv2d_q, L.Dense_q)):
            tags |= {layer.name + "/" + t for t in ("W_range", "X_range", "grad_range", "W_mean")}
            if layer.use_bias:
                tags |= {layer.name + "/b_range", layer.name + "/b_mean"}
        elif isinstance(layer, L.Normalization_q):
            tags |= {layer.name + "/" + t for t in ("X_range", "grad_range")}
        elif isinstance(layer, L.Rescale_q):
            tags |= {layer.name + "/" + t for t in ("g_range", "b_range", "X_range", "grad_range", "g_mean", "b_mean")}
    return tags


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused-graph", "layerwise-graph"])
def test_what_is_recorded_is_the_state_before_the_update(fused):
    """summary_every = 1 against a twin stepped by hand: forward + backward, read the state, update."""
    xs, ys = _batches(3, seed=8)
    ca, gm, ta = _trainer(22, fused, True, summary_every=1)
    cb, _, tb = _trainer(22, fused, False)
    X, y = torch.empty_like(xs[0]), torch.empty_like(ys[0])
    nq = len(cb.quantizers)
    off = [o for _, _, o, _ in tb.flat.offsets] + [tb.flat.n]
    want = []
    for i in range(3):
        X.copy_(xs[i])
        y.copy_(ys[i])
        tb._active = tb._plan(B)
        tb._sync_optimizer()
        assert not tb._fwd_bwd(X, y, update=False)
        torch.cuda.synchronize()
        m = tb._active
        w = tb.flat.w.cpu().numpy().copy()
        want.append(dict(ranges=cb.ranges(), counts=cb.counts_view().sum(dim=1, dtype=torch.int32).cpu().numpy(),
                         nelem=cb.nelem[:nq].cpu().numpy().copy(), step=int(cb.step.item()),
                         correct=int((m.logits.argmax(dim=1).to(torch.int32) == y).sum().item()),
                         F=SO.segment_sums(w, off), bound=SO.sum_bound(w, off)))
        tb._update()
        torch.cuda.synchronize()
        want[-1]["loss"] = float(m.loss.item())
        ta.step(X, y)
    recs = ta.summaries()
    assert len(recs) == 3
    _assert_same_state((ca, ta), (cb, tb))
    names = [q.name for q in cb.quantizers]
    for r, t in zip(recs, want):
        assert {n: r["scalars"][n] for n in names} == t["ranges"]
        c1 = np.array([0 if r["overflow"][n] is None else r["overflow"][n][0] for n in names])
        c2 = np.array([0 if r["overflow"][n] is None else r["overflow"][n][1] for n in names])
        fed = t["nelem"] > 0
        assert fed.sum() > 40 and t["counts"][:, 0].sum() > 0
        assert np.array_equal(c1[fed], t["counts"][fed, 0]) and np.array_equal(c2[fed], t["counts"][fed, 1])
        assert all((r["overflow"][n] is None) == (not f) for n, f in zip(names, fed))
        assert np.array_equal(np.array([r["nelem"][n] for n in names], dtype=F32), t["nelem"])
        assert r["step"] == t["step"] and r["batch"] == B and r["correct"] == t["correct"]
        assert r["accuracy"] == float(F32(t["correct"]) / F32(B))
        assert F32(r["loss"]).tobytes() == F32(t["loss"]).tobytes()
        sums = list(r["param_sums"].values())
        assert len(sums) == len(t["F"])
        for s, f, bnd in zip(sums, t["F"], t["bound"]):
            assert abs(s - f) <= bnd
        for n in names:  # r = float32(c) / float32(nelem), as range_apply
            if r["overflow"][n] is not None:
                c1n, c2n, r1, r2 = r["overflow"][n]
                assert r1 == float(F32(c1n) / F32(r["nelem"][n])) and r2 == float(F32(c2n) / F32(r["nelem"][n]))
    assert [r["step"] for r in recs] == [0, 1, 2]
    # tags: exactly the reference's for this model's layers, minus X_mean
    assert set(recs[0]["scalars"]) == _expected_tags(gm)
    for (o, v, _, sz), (key, s) in zip(tb.flat.offsets, recs[0]["param_sums"].items()):
        assert key == "%s/%s" % (o.name, v)
        assert recs[0]["scalars"]["%s/%s" % (o.name, S.MEAN_TAG[v])] == float(F32(s / sz))


@pytest.mark.gpu
def test_several_plans_share_one_ring(tmp_path):
    """train() over 40 samples: batches of 16, 16 and 8 -- the last on a plan of its own."""
    rng = np.random.default_rng(41)
    Xtr = ((rng.integers(0, 256, size=(40, 32, 32, 3)) - 127.5) / 128).astype(F32)
    ytr = rng.integers(0, 10, size=40).astype(np.int32)
    out = []
    for kw in (dict(), dict(summary_every=1, logdir=str(tmp_path))):
        c, _, tr = _trainer(23, True, True, **kw)
        tr.dataset, tr.n_epoch = ((Xtr, ytr), (None, None)), 1
        torch.manual_seed(5)
        tr.train()
        out.append((c, tr))
    (ca, ta), (cb, tb) = out
    _assert_same_state((ca, ta), (cb, tb))
    recs = tb.summaries()
    assert [r["batch"] for r in recs] == [16, 16, 8] and [r["step"] for r in recs] == [0, 1, 2]
    names = [q.name for q in cb.quantizers]
    for r, plan in zip(recs, (tb.model, tb.model, tb._plans[8])):
        got = np.array([r["nelem"][n] for n in names], dtype=F32)
        assert np.array_equal(got, plan._nelem[:len(names)].cpu().numpy())
    assert not np.array_equal(tb.model._nelem.cpu().numpy(), tb._plans[8]._nelem.cpu().numpy())
    assert not os.path.exists(str(tmp_path / "train"))  # three batches: the every-100-batches point never came


class _Log(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


@pytest.mark.gpu
def test_logging_point_drains_logs_and_writes_jsonl(tmp_path):
    """_log_batch (what both epoch loops call every 100 batches): the reference's line from the newest record,
    every record appended to logdir/train/summaries.jsonl; without summaries the line stays as it was."""
    xs, ys = _batches(2, seed=9)
    h = _Log()
    logger = logging.getLogger("test_summary")
    logger.setLevel(logging.INFO)
    logger.addHandler(h)
    try:
        _, _, tr = _trainer(24, True, True, summary_every=1, logger=logger, logdir=str(tmp_path))
        for i in range(2):
            loss = tr.step(xs[i], ys[i])
        tr._log_batch(100, loss)
        back = S.read_jsonl(str(tmp_path / "train" / "summaries.jsonl"))
        assert [r["step"] for r in back] == [0, 1] and tr.summaries() == []
        assert h.lines[-1] == "Batch 100 loss %f acc %f" % (back[-1]["loss"], back[-1]["accuracy"])
        assert back[-1]["loss"] == float(loss.item())
        _, _, t0 = _trainer(24, True, True, logger=logger)
        loss = t0.step(xs[0], ys[0])
        t0._log_batch(100, loss)
        assert h.lines[-1] == "Batch 100 loss %f" % loss.item()
    finally:
        logger.removeHandler(h)


@pytest.mark.gpu
def test_ring_overflow_is_counted_by_the_trainer():
    xs, ys = _batches(1, seed=10)
    _, _, tr = _trainer(25, True, True, summary_every=1, summary_capacity=2)
    for _ in range(5):
        tr.step(xs[0], ys[0])
    recs = tr.summaries()
    assert [r["step"] for r in recs] == [3, 4] and tr.summary_dropped == 3


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layerwise"])
def test_ordinary_steps_pay_nothing(fused):
    """summary_every = 3: the launches of the 1st and 2nd step, by kernel name, are those of a trainer without
    summaries; the 3rd has exactly two more. Counted where they are issued (the launch hook of dfxp.ops, eager
    steps), and for the fused plan also in the launch lists a captured step is built from."""
    from lbt_amd.dfxp import ops
    xs, ys = _batches(1, seed=11)

    def counts(tr):
        ops.PROFILE = {}
        try:
            tr.step(xs[0], ys[0])
            torch.cuda.synchronize()
            return {k: len(v) for k, v in ops.PROFILE.items()}
        finally:
            ops.PROFILE = None
    _, _, t0 = _trainer(26, fused, False)
    _, _, t3 = _trainer(26, fused, False, summary_every=3)
    base = [counts(t0) for _ in range(3)]
    got = [counts(t3) for _ in range(3)]
    assert base[1] == base[2] and sum(base[1].values()) > 20
    assert got[0] == base[0] and got[1] == base[1]
    extra = dict(base[2])
    extra.update(summary_record_kernel=1, summary_commit_kernel=1)
    assert got[2] == extra
    assert [r["step"] for r in t3.summaries()] == [2]
    if fused:
        m0, m3 = t0.model, t3.model
        plain = [f.kname for f in m0.step_launches(True)]
        assert [f.kname for f in m3.step_launches(True)] == plain
        rec = [f.kname for f in m3.step_launches(True, t3._summary(m3))]
        assert rec == plain[:-1] + ["summary_record_kernel", plain[-1], "summary_commit_kernel"]
        assert plain[-1] == "step_reduce_kernel"
        # graphs: a trainer with summaries holds one graph per kind of step and buffer pair, and replays the
        # plain one on ordinary steps
        _, _, tg = _trainer(26, True, True, summary_every=3)
        seen = []
        for _ in range(3):
            tg.step(xs[0], ys[0])
            seen.append(tg._graphs)
        keys = sorted(tg._gcache, key=lambda k: k[3])
        assert [k[3] for k in keys] == [False, True]
        assert seen[0] is seen[1] is tg._gcache[keys[0]] and seen[2] is tg._gcache[keys[1]]


@pytest.mark.gpu
def test_data_parallel_trainer_refuses_summaries(one_rank_group):
    from lbt_amd.fused import FusedResNet
    from lbt_amd.models import CIFAR10_Resnet20
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    ctx = DfxpContext(seed=1)
    m = FusedResNet(CIFAR10_Resnet20(8, weight_decay=2e-4, ctx=ctx))
    with pytest.raises(NotImplementedError, match="summed across ranks"):
        Trainer(m, batch_size=B, exchange=True, summary_every=1)
    assert m._shape is None  # nothing was built or captured
    assert Trainer(m, batch_size=B, exchange=True).dp  # the same trainer without summaries is accepted

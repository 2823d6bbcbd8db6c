"""The batched weight-gradient launch (lbt_conv_wgrad_many_i8 / lbt_conv_wgrad_many_stem_i8, conv_mfma.hip)
at the smallest shapes at which its staged body (wgrad_s1_body: 64-pixel chunks of whole output rows, one
workgroup per pixel split x ci slice x group of co slices; 3x3 convs of stride 1 and 2) can go wrong, against
the exact int64 sum
dW[kh, kw, ci, co] = sum_p X[p shifted by the tap][ci] * G[p][co]  (out-of-image taps = the fill code: -128
for the offset encoding x_u8off = 1, else 0). Every job's slab is compared summed over its shards; the sums
are integers, so the comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)

# the bench's block convs (ResNet-20 / CIFAR-10) as (H, W, Cin, Cout, k, s)
BENCH_CONVS = ([(32, 32, 16, 16, 3, 1)] * 6 + [(32, 32, 16, 32, 3, 2), (32, 32, 16, 32, 1, 2)] +
               [(16, 16, 32, 32, 3, 1)] * 5 + [(16, 16, 32, 64, 3, 2), (16, 16, 32, 64, 1, 2)] +
               [(8, 8, 64, 64, 3, 1)] * 5)


def _desc(N, H, W, Cin, Cout, k, s):
    from lbt_amd.dfxp import ops
    return ops.conv_desc(N, H, W, Cin, Cout, k, k, s, s, "SAME")


def _expected(x, g, d, fill):
    """Exact int64 sum_p X_tap (x) G of a TF-SAME conv (x, g: int8 NHWC codes) -> [taps * Cin, Cout]."""
    N, H, W, Cin = x.shape
    _, Ho, Wo, Cout = g.shape
    xp = np.full((N, H + d.PT + d.PB + 2 * d.SH, W + d.PL + d.PR + 2 * d.SW, Cin), fill, np.int64)
    xp[:, d.PT:d.PT + H, d.PL:d.PL + W] = x
    gg = g.reshape(-1, Cout).astype(np.int64)
    out = np.zeros((d.KH, d.KW, Cin, Cout), np.int64)
    for kh in range(d.KH):
        for kw in range(d.KW):
            xt = xp[:, kh:kh + d.SH * Ho:d.SH, kw:kw + d.SW * Wo:d.SW][:, :Ho, :Wo].reshape(-1, Cin)
            out[kh, kw] = xt.T @ gg
    return out.reshape(-1, Cout)


class _Jobs:
    """A list of weight-gradient jobs on random int8 operands, with their exact expected sums."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.jobs, self.slabs, self.want, self.tags, self.keep = [], [], [], [], []

    def add(self, case, x_u8off, nsplit=None, operands=None):
        from lbt_amd._lib import WgradJob
        from lbt_amd.dfxp import ops
        N, H, W, Cin, Cout, k, s = case
        d = _desc(*case)
        if operands is None:
            x = self.rng.integers(-128, 128, size=(N, H, W, Cin), dtype=np.int8)
            g = self.rng.integers(-128, 128, size=(N, d.Ho, d.Wo, Cout), dtype=np.int8)
            operands = (x, g, torch.from_numpy(x).to(DEV), torch.from_numpy(g).to(DEV),
                        _expected(x, g, d, -128 if x_u8off else 0))
        x, g, xq, gq, want = operands
        ns = ops.wgrad_nsplit_batched(d) if nsplit is None else nsplit
        nh = ops.wgrad_nshard(d, ns)
        slab = torch.zeros((nh, k * k * Cin, Cout), dtype=torch.int32, device=DEV)
        self.keep += [xq, gq]
        self.jobs.append(WgradJob(xq.data_ptr(), int(x_u8off), gq.data_ptr(), d, slab.data_ptr(), ns, nh))
        self.slabs.append(slab)
        self.want.append(want)
        self.tags.append((case, x_u8off, ns))
        return operands

    def array(self):
        from lbt_amd._lib import WgradJob
        return (WgradJob * len(self.jobs))(*self.jobs)

    def run(self):
        from lbt_amd.dfxp import ops
        for s in self.slabs:
            s.zero_()
        ops.call("lbt_conv_wgrad_many_i8", self.array(), len(self.jobs), ops.stream())
        torch.cuda.synchronize()

    def check(self):
        for slab, want, tag in zip(self.slabs, self.want, self.tags):
            got = slab.cpu().numpy().astype(np.int64).sum(0)
            assert np.array_equal(got, want), tag


def _divisors(n):
    return [k for k in range(1, n + 1) if n % k == 0]


# the three stages' shapes at N = 2 and N = 3: odd chunk counts (the split falls back to a divisor), the
# first and the last row block of every image (top halo, bottom halo, fill code)
STAGE = [(N, H, W, C, C, 3, 1) for N in (2, 3) for (H, W, C) in ((32, 32, 16), (16, 16, 32), (8, 8, 64))]
# Cin != Cout (3 x 12 x 8 has no whole-row chunks: the per-tap body with two ci slices), and on the staged
# body both ways round, with one and with two co slices per workgroup
CIN_COUT = [(3, 12, 8, 32, 16, 3, 1), (2, 8, 8, 16, 64, 3, 1), (2, 16, 8, 32, 16, 3, 1), (2, 16, 16, 64, 32, 3, 1)]
# narrow and wide rows: W = 4 (16 rows per chunk), W = 2 (three halo pieces), W = 32 with two co slices,
# W = 64 (one row per chunk: the per-tap body)
ROWS = [(2, 4, 64, 16, 32, 3, 1), (2, 16, 4, 16, 32, 3, 1), (1, 32, 2, 16, 16, 3, 1), (2, 32, 32, 16, 32, 3, 1)]
# 3x3 / 2 on the staged body: the bench's two (padding bottom / right only), an odd chunk count, an odd image
# (padding on all four sides), one ci slice with four co slices; and shapes it leaves to the per-tap body
# (output rows that tile no chunk, an odd number of co slices)
STRIDED = [(2, 32, 32, 16, 32, 3, 2), (3, 16, 16, 32, 64, 3, 2), (2, 31, 31, 16, 32, 3, 2), (2, 16, 16, 16, 64, 3, 2),
           (2, 8, 8, 16, 32, 3, 2), (2, 32, 32, 16, 16, 3, 2)]


@pytest.mark.parametrize("x_u8off", [0, 1])
@pytest.mark.parametrize("group", ["stage", "cin_cout", "rows", "strided"])
def test_shapes_exact(group, x_u8off):
    """One batched call per group of shapes, both fill codes."""
    cases = {"stage": STAGE, "cin_cout": CIN_COUT, "rows": ROWS, "strided": STRIDED}[group]
    jb = _Jobs(11 + x_u8off)
    for case in cases:
        jb.add(case, x_u8off)
        d = _desc(*case)
        if d.SH == 1 and 64 % d.W == 0 and d.H % (64 // d.W) == 0 and d.W < 64:  # whole-row chunks: the staged body
            assert (d.N * d.H * d.W // 64) % jb.tags[-1][2] == 0, case
    jb.run()
    jb.check()


@pytest.mark.parametrize("x_u8off", [0, 1])
def test_every_split_exact(x_u8off):
    """One conv per staged instance with every split that divides its chunk count, one split for the whole
    conv and one chunk per split included (then seven of a workgroup's eight waves have no chunk)."""
    jb = _Jobs(23 + x_u8off)
    for case in ((3, 32, 32, 16, 16, 3, 1), (2, 16, 16, 32, 32, 3, 1), (3, 8, 8, 64, 64, 3, 1),
                 (5, 16, 16, 16, 16, 3, 1), (2, 32, 32, 16, 32, 3, 2)):
        chunks = case[0] * (case[1] // case[6]) * (case[2] // case[6]) // 64
        operands = None
        for ns in _divisors(chunks):
            operands = jb.add(case, x_u8off, nsplit=ns, operands=operands)
    jb.run()
    jb.check()


MIXED = [(2, 32, 32, 16, 16, 3, 1), (2, 32, 32, 16, 32, 3, 2), (2, 32, 32, 16, 32, 1, 2), (2, 16, 16, 32, 32, 3, 1),
         (2, 16, 16, 32, 64, 3, 2), (2, 16, 16, 32, 64, 1, 2), (2, 8, 8, 64, 64, 3, 1)]


def test_mixed_list_with_and_without_stem():
    """Staged, 3x3/2 and 1x1/2 jobs in one call, exact; and the same list through
    lbt_conv_wgrad_many_stem_i8 (the stem's backward as workgroups of the same launch, N = 2) against
    lbt_conv_wgrad_many_i8 followed by lbt_conv_stem_bwd: the jobs' slabs exact, the stem's slab equal."""
    from lbt_amd.dfxp import ops
    from lbt_amd.fused import FusedResNet
    from lbt_amd.models import CIFAR10_Resnet20
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    jb = _Jobs(31)
    for case in MIXED:
        jb.add(case, 1)
    jb.run()
    jb.check()

    # the stem backward's own arguments come from a ResNet-20 plan at N = 2 after one step
    ctx = DfxpContext(seed=3)
    m = FusedResNet(CIFAR10_Resnet20(8, weight_decay=2e-4, ctx=ctx))
    tr = Trainer(m, lr=1e-2, momentum=0.9, batch_size=2, use_graph=False)
    rng = np.random.default_rng(4)
    x = ((rng.integers(0, 256, size=(2, 32, 32, 3)) - 127.5) / 128).astype(np.float32)
    y = rng.integers(0, 10, size=2).astype(np.int32)
    tr.step(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
    torch.cuda.synchronize()
    stem = [f for f in m._bwd if getattr(f, "kname", "") == "conv_wgrad_many_stem_kernel"]
    assert len(stem) == 1
    _, _, aB, ximg, dc, _, ns0 = stem[0].__defaults__[1]
    assert dc.N == 2
    slab0 = torch.zeros((ns0, dc.KH * dc.KW * dc.Cin, dc.Cout), dtype=torch.int32, device=DEV)
    p0 = ctypes.c_void_p(slab0.data_ptr())
    arr = jb.array()

    def zero():
        slab0.zero_()
        for s in jb.slabs:
            s.zero_()

    zero()
    ops.call("lbt_conv_wgrad_many_i8", arr, len(jb.jobs), ops.stream())
    ops.call("lbt_conv_stem_bwd", aB, ximg, dc, p0, ns0, ops.stream())
    torch.cuda.synchronize()
    jb.check()
    two_calls = slab0.cpu().numpy().astype(np.int64).sum(0)
    assert np.any(two_calls != 0)
    zero()
    ops.call("lbt_conv_wgrad_many_stem_i8", arr, len(jb.jobs), aB, ximg, dc, p0, ns0, ops.stream())
    torch.cuda.synchronize()
    jb.check()
    assert np.array_equal(slab0.cpu().numpy().astype(np.int64).sum(0), two_calls)


@pytest.mark.parametrize("B", [128, 64, 32, 16])
def test_planner(B):
    """The library's plan (lbt_conv_wgrad_many_nsplit / _blocks / _slots, through ops) for the bench's block
    convs: a staged job's split divides its chunk count, a wave's accumulator and a slab shard each cover at
    most 65536 pixels, and at B = 128 the whole launch (the stem's 256-pixel row blocks, two per workgroup,
    included) has at most as many workgroups as are resident at once."""
    from lbt_amd import _lib
    from lbt_amd.dfxp import ops
    total = B * 32 * 32 // 512
    for (H, W, Cin, Cout, k, s) in BENCH_CONVS:
        d = _desc(B, H, W, Cin, Cout, k, s)
        ns = ops.wgrad_nsplit_batched(d)
        nh = ops.wgrad_nshard(d, ns)
        P = d.N * d.Ho * d.Wo
        if k == 3:  # staged: whole 64-pixel chunks per split, at most 65536 pixels per wave
            assert (P // 64) % ns == 0, (B, H, Cin, Cout, s)
            assert -(-(P // 64 // ns) // 8) * 64 <= 65536
        assert 1 <= nh <= ns and -(-P // ns) * -(-ns // nh) <= 65536
        total += ops.wgrad_many_blocks(d, ns)
    slots = _lib.load().lbt_conv_wgrad_many_slots()
    assert slots >= 256
    print("B %d: %d workgroups, %d resident" % (B, total, slots))
    if B == 128:
        assert total <= slots, (total, slots)

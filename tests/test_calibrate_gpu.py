"""Range calibration on the GPU: the scan and pick kernels against numpy (tests/calib_oracle.py), and
``Trainer.calibrate`` against the calibration pass of the numpy model -- the same ranges for every quantiser,
nothing else moved, and the real (captured) step standing still on them.
"""
import ctypes

import numpy as np
import pytest
import torch

import calib_oracle as C
from lbt_amd import _lib
from oracle import nn as onn
from oracle import resnet as oresnet
from test_training import _batch, _oracle_params, _templates

pytestmark = pytest.mark.gpu
F32 = np.float32
DEV = "cuda:0"
BITS = (2, 4, 8, 9, 16, 20)
TARGETS = (0.0, 0.01, 0.3)
SUFFIX = {"W": "/W", "gamma": "/g", "beta": "/b"}


def _ops():
    from lbt_amd.dfxp import ops
    return ops


# ------------------------------------------------------------------------------------ scan kernel
def _crafted():
    pw = np.array([2.0 ** k for k in range(-31, 32)], F32)
    up, dn = np.nextafter(pw, F32(np.inf)), np.nextafter(pw, F32(0))
    denorm = np.array([0x007FFFFF], np.uint32).view(F32)
    return np.concatenate([pw, up, dn, -pw, -up, -dn, [0.0, -0.0, np.inf, -np.inf, np.nan], denorm, -denorm]).astype(F32)


def _fill(n, kind):
    rng = np.random.default_rng(n + 7)
    if kind == "normal":   # 3 to 8 neighbouring bins, as real tensors
        return (rng.standard_normal(n) * 3e-3).astype(F32)
    if kind == "one_bin":  # every element in [1, 2): one table entry from every lane, the contention case
        return rng.uniform(1.0, 1.999, n).astype(F32)
    if kind == "all_bins":
        return (rng.choice([-1.0, 1.0], n) * rng.uniform(1, 2, n) * np.exp2(rng.integers(-34, 34, n))).astype(F32)
    return np.resize(_crafted(), n).astype(F32)


def _scan(x, offset, table=None):
    """The kernel's table (a histogram: calib_oracle.hist) of x placed `offset` floats behind a 16-byte boundary."""
    buf = torch.zeros(x.size + offset + 8, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + x.size]
    view.copy_(torch.from_numpy(x))
    if table is None:
        table = torch.zeros(_lib.RANGE_BINS, dtype=torch.int64, device=DEV)
    _ops().range_scan(view, table)
    torch.cuda.synchronize()
    return table


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [0, 1, 3, 63, 64, 65, 255, 1027, 2 ** 20 + 3])
def test_scan_tables_are_bit_equal_to_numpy(n, offset):
    for kind in ("normal", "one_bin", "all_bins", "crafted"):
        x = _fill(n, kind)
        want = C.hist(x)
        got = _scan(x, offset).cpu().numpy()
        assert np.array_equal(got, want), (kind, np.flatnonzero(got != want)[:8] - 30)
        again = _scan(x, offset).cpu().numpy()  # integer sums commute: the same bits in every run
        assert np.array_equal(again, got), kind


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_scan_crafted_values_at_every_alignment(offset):
    x = _crafted()
    assert np.array_equal(_scan(x, offset).cpu().numpy(), C.hist(x))
    for k in range(1, 8):  # every head / tail split of a short tensor
        assert np.array_equal(_scan(x[:k], offset).cpu().numpy(), C.hist(x[:k])), k


def test_two_scans_on_one_table_add_up():
    a, b = _fill(1027, "normal"), _fill(65, "all_bins")
    t = _scan(a, 1)
    t = _scan(b, 0, table=t)
    assert np.array_equal(t.cpu().numpy(), C.hist(a) + C.hist(b))


# ------------------------------------------------------------------------------------ pick kernel
def _pick_cases():
    rng = np.random.default_rng(2)
    xs = [(rng.standard_normal(1025) * s).astype(F32)
          for s in (1e-8, 1e-6, 2e-5, 3e-4, 5e-3, 0.07, 1.0, 9.0, 40.0, 800.0, 3e5, 1e9)]
    xs += [_crafted(), np.zeros(64, F32), np.array([17.0] + [1e-3] * 999, F32), np.array([np.inf, 1.0], F32)]
    return [(x, bits, t) for x in xs for bits in BITS for t in TARGETS]


def test_pick_every_width_and_target_in_one_launch():
    cases = _pick_cases()
    cases.insert(5, (np.ones(10, F32) * 100, 32, 0.0))  # a 32-bit slot: left alone
    n = len(cases)
    assert n > 256  # more jobs than one launch carries
    tables = torch.from_numpy(np.stack([C.hist(x) for x, _, _ in cases])).to(DEV).contiguous()
    exps = torch.full((n,), 7, dtype=torch.int32, device=DEV)
    kept = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    bits = torch.tensor([b for _, b, _ in cases], dtype=torch.int32, device=DEV)
    target = torch.tensor([t for _, _, t in cases], dtype=torch.float32, device=DEV)
    nelem = torch.tensor([float(x.size) for x, _, _ in cases], dtype=torch.float32, device=DEV)
    slots = [s for s in range(n) if s % 7 != 3]  # some slots are no job: untouched
    _ops().range_pick(tables.view(-1), slots, exps, bits, target, nelem, kept)
    torch.cuda.synchronize()
    e, k = exps.cpu().tolist(), kept.cpu().tolist()
    nkept = 0
    for s, (x, b, t) in enumerate(cases):
        if s not in slots or b == 32:
            assert (e[s], k[s]) == (7, -1), s
            continue
        I, keep = C.pick(C.table(x), x.size, b, t)
        assert k[s] == int(keep), (s, b, t)
        assert e[s] == (7 if keep else I), (s, b, t, e[s], I)
        nkept += keep
    assert nkept >= 3 * len(BITS)  # the all-zero tensor at least


def test_host_checks_return_einval():
    lib = _lib.load()
    x = torch.zeros(8, dtype=torch.float32, device=DEV)
    tab = torch.zeros(2 * _lib.RANGE_BINS, dtype=torch.int64, device=DEV)
    i32 = torch.zeros(2, dtype=torch.int32, device=DEV)
    f32 = torch.ones(2, dtype=torch.float32, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.lbt_dfxp_range_scan(None, 8, P(tab), None) == 1001
    assert lib.lbt_dfxp_range_scan(P(x), 8, None, None) == 1001
    assert lib.lbt_dfxp_range_scan(P(x), -1, P(tab), None) == 1001
    assert lib.lbt_dfxp_range_scan(ctypes.c_void_p(x.data_ptr() + 2), 4, P(tab), None) == 1001
    assert lib.lbt_dfxp_range_scan(None, 0, None, None) == 0  # nothing to read: nothing launched
    ok = (ctypes.c_int32 * 2)(0, 1)
    args = [P(tab), ok, 2, P(i32), P(i32), P(f32), P(f32), 2, P(i32), None]
    for null in (0, 1, 3, 4, 5, 6, 8):
        a = list(args)
        a[null] = None
        assert lib.lbt_dfxp_range_pick(*a) == 1001, null
    for bad in (-1, 2):
        a = list(args)
        a[1] = (ctypes.c_int32 * 2)(0, bad)
        assert lib.lbt_dfxp_range_pick(*a) == 1001, bad
    a = list(args)
    a[2] = -1
    assert lib.lbt_dfxp_range_pick(*a) == 1001
    a = list(args)
    a[7] = -1
    assert lib.lbt_dfxp_range_pick(*a) == 1001
    a = list(args)
    a[2] = 0
    assert lib.lbt_dfxp_range_pick(*a) == 0
    torch.cuda.synchronize()
    assert int(tab.abs().sum().item()) == 0 and int(i32.abs().sum().item()) == 0  # a refused call writes nothing


# ------------------------------------------------------------------------------------ models
def _oracle_pass(om, ranges, x, y, seed, dz, monkeypatch):
    """The calibration pass of the numpy model (forward + backward of the injected dz: the softmax is the one
    op that is not bit-exact); returns the CalibCtx. ranges is calibrated in place."""
    def run():
        ctx = onn.Ctx(ranges, 0, seed)
        om.forward(np.asarray(x, F32), ctx)
        om.backward(np.asarray(dz, F32), ctx)
        return ctx
    return C.calibrate(run, monkeypatch)


def _resnet8(fused=False, blocks=(1, 1, 1), **ctx_kw):
    """The smallest CIFAR ResNet the models build (one block per stage; 32x32: its pool is 8x8), B = 16, with
    the oracle's parameters of test_default_grad_range_makes_first_update_noise."""
    from lbt_amd import dynamic_fixed_point as L
    from lbt_amd.fused import FusedResNet
    from lbt_amd.models import CIFAR10_Resnet
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    ctx = DfxpContext(device=DEV, seed=0, **ctx_kw)
    gm = CIFAR10_Resnet(8, list(blocks), L.ResidualBlock_q, weight_decay=2e-4, ctx=ctx)
    om = oresnet.build_resnet(tuple(blocks), 8, 2e-4)
    p = _oracle_params(om, 0)
    oresnet.set_params(om, p)
    for o, v, _ in gm.param_slots():
        getattr(o, v).copy_(torch.from_numpy(p[o.name + SUFFIX[v]]))
    tr = Trainer(FusedResNet(gm) if fused else gm, lr=1e-2, momentum=0.9, batch_size=16, use_graph=True,
                 **({"exchange": True} if ctx_kw else {}))
    rng = np.random.default_rng(3)
    x = ((rng.integers(0, 256, size=(16, 32, 32, 3)) - 127.5) / 128).astype(F32)
    y = rng.integers(0, 10, 16).astype(np.int32)
    return ctx, gm, om, tr, x, y, torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)


@pytest.fixture(scope="module")
def resnet8_reference():
    """Trainer.calibrate on the layer-wise ResNet-8 and the numpy calibration pass on the same batch, once."""
    ctx, gm, om, tr, x, y, X, Y = _resnet8()
    res = tr.calibrate(X, Y)
    dz = gm.dlogits.cpu().numpy().copy()
    ranges = oresnet.init_ranges(om)
    mp = pytest.MonkeyPatch()
    try:
        octx = _oracle_pass(om, ranges, x, y, ctx.seed, dz, mp)
    finally:
        mp.undo()
    return dict(res=res, set=dict(octx.set), kept=sorted(octx.kept))


def test_resnet8_ranges_equal_the_oracles(resnet8_reference):
    r = resnet8_reference
    assert r["res"]["unfed"] == []
    assert sorted(r["res"]["kept"]) == r["kept"] and r["kept"]
    assert r["res"]["set"] == r["set"]
    assert len({v for k, v in r["set"].items() if k.endswith("grad_range")}) > 1


def test_mnist_model_ranges_equal_the_oracles(monkeypatch):
    """Dropout (its unfused route), biases, dense layers and pools, against tests/plain_oracle.py."""
    import plain_oracle as P
    from lbt_amd.models import MNIST_Model
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    ctx = DfxpContext(device=DEV, seed=4)
    gm = MNIST_Model(8, ctx=ctx)
    tr = Trainer(gm, lr=1e-2, momentum=0.9, batch_size=8, use_graph=True)
    rng = np.random.default_rng(8)
    x = rng.uniform(-1, 1, size=(8, 28, 28, 1)).astype(F32)
    y = rng.integers(0, 10, 8).astype(np.int32)
    # a bias that is not zero gets a range; the others (fresh: zeros) keep theirs
    gm.layers[3].b.copy_(torch.from_numpy(rng.uniform(-0.1, 0.1, 16).astype(F32)))
    res = tr.calibrate(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
    om = P.mnist(8, 0.5)
    P.set_params(om, {o.name + {"W": "/W", "b": "/bias"}[v]: getattr(o, v).cpu().numpy() for o, v, _ in gm.param_slots()})
    ranges = P.init_ranges(om)
    octx = _oracle_pass(om, ranges, x, y, ctx.seed, gm.dlogits.cpu().numpy(), monkeypatch)
    assert res["unfed"] == []
    assert sorted(res["kept"]) == sorted(octx.kept) and "conv2/b_range" in res["set"] and "conv1/b_range" in res["kept"]
    assert res["set"] == octx.set
    assert ctx.ranges() == ranges


def test_bottleneck_model_with_16_bit_gradients_equals_the_oracles(monkeypatch):
    """ResidualBottleneck_q at the reduced widths of tests/test_dp_resnet50_gpu.py, grad_bits = 16: int16
    gradient codes, the max pool, the wide BN backward."""
    from lbt_amd.models import ImageNet_Resnet
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    blocks, width, image, classes, grad_bits = (1, 1, 1, 1), 8, 32, 16, 16
    ctx = DfxpContext(device=DEV, seed=1)
    gm = ImageNet_Resnet(8, blocks, grad_bits=grad_bits, width=width, classes=classes, image=image, weight_decay=1e-4,
                         ctx=ctx)
    tr = Trainer(gm, lr=1e-2, momentum=0.9, batch_size=8, use_graph=True)
    rng = np.random.default_rng(5)
    x = ((rng.integers(0, 256, size=(8, image, image, 3)) - 127.5) / 128).astype(F32)
    y = rng.integers(0, classes, size=8).astype(np.int32)
    res = tr.calibrate(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
    om = oresnet.build_resnet50(blocks, width, classes, 8, grad_bits, weight_decay=1e-4)
    oresnet.set_params(om, {o.name + SUFFIX[v]: getattr(o, v).cpu().numpy() for o, v, _ in gm.param_slots()})
    ranges = oresnet.init_ranges(om)
    octx = _oracle_pass(om, ranges, x, y, ctx.seed, gm.dlogits.cpu().numpy(), monkeypatch)
    assert res["unfed"] == []
    assert sorted(res["kept"]) == sorted(octx.kept)
    assert res["set"] == octx.set
    # ... and the real step stands still on them
    before = ctx.ranges()
    tr.step(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
    torch.cuda.synchronize()
    after = ctx.ranges()
    assert {k: after[k] - before[k] for k in before if after[k] != before[k]} == {k: -1 for k in res["kept"]}


@pytest.mark.parametrize("fused", [False, True], ids=["layerwise", "fused"])
def test_nothing_else_moved_and_the_captured_step_stands_still(fused, resnet8_reference):
    """The fused plan has no launch for a projection block behind a projection block (its transition kernel
    takes one BN branch in front), so it cannot run one block per stage: its case is two blocks per stage,
    the smallest it builds, against a layer-wise trainer of that model."""
    blocks = (2, 2, 2) if fused else (1, 1, 1)
    ctx, gm, om, tr, x, y, X, Y = _resnet8(fused, blocks)
    want = _resnet8(False, blocks)[3].calibrate(X, Y) if fused else resnet8_reference["res"]
    bns = tr._bn_layers()
    assert len(bns) == (15 if fused else 9)
    for bn in bns:  # (fresh running statistics are 0 / 1: make a restore visible)
        bn.X_mean_running.uniform_(-1, 1)
        bn.X_var_running.uniform_(0.5, 2)
    snap = lambda: dict(w=tr.flat.w.clone(), a=tr.flat.a.clone(), g=tr.flat.g.clone(), step=ctx.step.clone(),  # noqa: E731
                        nelem=ctx.nelem.clone(), bn=[(b.X_mean_running.clone(), b.X_var_running.clone()) for b in bns])
    tr.flat.g.normal_()
    before = snap()
    res = tr.calibrate(X, Y)
    after = snap()
    for k in ("w", "a", "g", "step", "nelem"):
        assert torch.equal(before[k].view(torch.int32) if before[k].is_floating_point() else before[k],
                           after[k].view(torch.int32) if after[k].is_floating_point() else after[k]), k
    for (m0, v0), (m1, v1) in zip(before["bn"], after["bn"]):
        assert torch.equal(m0, m1) and torch.equal(v0, v1)
    assert int(ctx.counts.abs().sum().item()) == 0
    assert tr.global_step == 0
    # the same ranges whichever trainer calibrates (a plan calibrates its layer-wise model)
    assert res == want and res["unfed"] == [] and res["kept"]
    assert {k: v for k, v in ctx.ranges().items() if k in res["set"]} == res["set"]
    # fixed point, through the real step: every counting kernel of the path agrees with the scan
    r0 = ctx.ranges()
    tr.step(X, Y)
    torch.cuda.synchronize()
    r1 = ctx.ranges()
    assert tr.global_step == 1
    assert {k: r1[k] - r0[k] for k in r0 if r1[k] != r0[k]} == {k: -1 for k in res["kept"]}
    # between steps: calibrating again on the graph's own batch changes nothing but the kept ranges back
    res2 = tr.calibrate(X, Y)
    assert res2["unfed"] == [] and tr.global_step == 1


# ------------------------------------------------------------------------------------ refusals
def test_a_quantiser_fed_twice_raises():
    from lbt_amd._lib import OUT_I8
    from lbt_amd.runtime import DfxpContext
    ctx = DfxpContext(device=DEV)
    q = ctx.quantizer("twice/X_range", 8)
    x = torch.randn(4, 64, device=DEV)
    with ctx.calibrating():
        _ops().quantize(x, q, OUT_I8)
        with pytest.raises(RuntimeError, match="twice/X_range"):
            _ops().quantize(x, q, OUT_I8)
    assert not ctx.calibrating_now
    _ops().quantize(x, q, OUT_I8)  # outside: the ordinary call
    _ops().quantize(x, q, OUT_I8)


@pytest.fixture
def one_rank_group(tmp_path):
    import torch.distributed as dist
    own = not dist.is_initialized()
    if own:
        dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "pg"), rank=0, world_size=1)
    yield
    if own:
        dist.destroy_process_group()


def test_one_rank_group_is_accepted_and_more_ranks_refused(one_rank_group, resnet8_reference, monkeypatch):
    import torch.distributed as dist
    ctx, gm, om, tr, x, y, X, Y = _resnet8(world_size=1, rank=0)
    assert tr.dp
    assert tr.calibrate(X, Y) == resnet8_reference["res"]
    before = ctx.ranges()
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="2 ranks"):
        tr.calibrate(X, Y)
    assert ctx.ranges() == before


# ------------------------------------------------------------------------------------ it learns
def test_resnet20_at_default_ranges_learns_after_calibration():
    """The template task of tests/test_training.py (B = 128, lr 1e-2, momentum 0.9, wd 2e-4, 150 steps, fused
    plan) with the model built at the DEFAULT ranges -- no grad_range argument -- and calibrated on the first
    batch. The criterion is that test's own."""
    from lbt_amd.fused import FusedResNet
    from lbt_amd.models import CIFAR10_Resnet20
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    B, seed = 128, 5
    ctx = DfxpContext(seed=seed)
    gm = CIFAR10_Resnet20(8, weight_decay=2e-4, ctx=ctx)
    assert set(ctx.ranges().values()) == {2}
    tr = Trainer(FusedResNet(gm), lr=1e-2, momentum=0.9, batch_size=B, use_graph=True)
    T = _templates(seed)
    rng = np.random.default_rng(seed)
    bufs = [(torch.empty((B, 32, 32, 3), device="cuda"), torch.empty((B,), dtype=torch.int32, device="cuda"))
            for _ in range(2)]
    losses = []
    for i in range(150):
        x, y = _batch(T, B, rng)
        X, Y = bufs[i % 2]
        X.copy_(torch.from_numpy(x))
        Y.copy_(torch.from_numpy(y))
        if i == 0:
            res = tr.calibrate(X, Y)
            assert res["unfed"] == []
        losses.append(float(tr.step(X, Y).item()))
    print("losses every 10 steps:", [round(v, 4) for v in losses[::10]], "last ten mean %.4f" % np.mean(losses[-10:]))
    assert np.mean(losses[-10:]) < 0.1 < losses[0] / 10, losses[::10]

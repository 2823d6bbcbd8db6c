"""Testing-mode BatchNorm (``Model.set_testing``, reference ``models.py:15``) on the fused kernels.

* the frozen ``lbt_conv_fwd_fused_i8`` / ``lbt_conv_fwd2_fused_i8`` against the existing two-launch
  sequences (``lbt_bn_chain_fwd`` with ``frozen = 1``, then ``lbt_conv_fwd_i8`` / ``lbt_conv_fwd_pair_i8``), bit
  for bit, at the smallest shapes that reach every tile height of ``lbt_conv_fused_tile_rows``;
* the argument checks of the frozen contract;
* ``FusedResNet(model, inference=True)`` against the layer-wise model after ``set_testing()`` and the oracle;
* the plan is read-only with respect to training (context, running statistics, a captured step);
* ``Trainer.evaluate(..., testing=True)``, fused against layer-wise;
* the forward-only surface.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import nn as onn
from oracle import resnet as oresnet

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
EINVAL = 1001


# ------------------------------------------------------------------------------ kernel level
class _Conv:
    """One conv's quantised weight images from random weights (bits = 4: the packed images too)."""

    def __init__(self, ctx, rng, name, kh, cin, cout, bits):
        from lbt_amd.dfxp import ops
        self.q = ctx.quantizer(name, bits, 0)
        w = torch.from_numpy((rng.standard_normal((kh, kh, cin, cout)) * 0.3).astype(F32)).to(DEV)
        self.ksf, ksd = ops.packed_slices(kh, kh, cin), ops.packed_slices(kh, kh, cout)
        self.w_hwio = torch.zeros((kh, kh, cin, cout), dtype=torch.int8, device=DEV)
        self.wf = torch.zeros((cout, self.ksf * 16), dtype=torch.int8, device=DEV)
        wd = torch.zeros((cin, ksd * 16), dtype=torch.int8, device=DEV)
        self.colsum = torch.zeros(cout, dtype=torch.int32, device=DEV)
        ops.quantize_weight(w, self.q, self.w_hwio, self.wf, self.ksf, wd, ksd, self.colsum)
        self.w4 = bits <= 4
        self.img = self.wf
        if self.w4:
            self.img = torch.zeros((cout, self.ksf * 8), dtype=torch.uint8, device=DEV)
            ops.pack_int4(self.wf, self.img)
        self.qw = self.q.desc_nostats()


class _Case:
    """Random operands of a frozen chain on [N, H, 512 / C, C]: int8 codes, running statistics, gamma /
    beta, residual and noise tables; the chain descriptor with no output pointer set."""

    def __init__(self, C, H, N, nb, res, seed, o2=False):
        from lbt_amd import _lib
        from lbt_amd.runtime import DfxpContext
        self.ctx = ctx = DfxpContext(seed=seed)
        self.rng = rng = np.random.default_rng(seed)
        self.C, self.H, self.N, self.W = C, H, N, 512 // C
        self.shp = shp = (N, H, self.W, C)
        self.inner = inner = H * self.W * C
        self.keep = []
        a = self.a = _lib.ChainFwd()
        for i in range(nb):
            br = a.b1 if i == 0 else a.b2
            q = self.dev(rng.integers(-128, 128, size=shp, dtype=np.int8))
            rm = self.dev((rng.standard_normal(C) * 0.5).astype(F32))
            rv = self.dev(rng.uniform(0.25, 2.0, C).astype(F32))
            gb = self.dev(np.concatenate([rng.uniform(0.5, 1.5, C), rng.standard_normal(C) * 0.3]).astype(F32))
            qn = ctx.quantizer("n%d/X_range" % i, 8, 2)
            br.nrm = _lib.BnNorm(q.data_ptr(), qn.desc_nostats(), None, N * H * self.W, 1e-5, 0.999, 0.001, None,
                                 rm.data_ptr(), rv.data_ptr(), 1, 0)
            br.qr = self.qd(ctx.quantizer("r%d/X_range" % i, 8, 2), inner)
            br.gb = gb.data_ptr()
        a.has_b2 = 1 if nb == 2 else 0
        if res:
            a.res = self.dev(rng.standard_normal(shp).astype(F32)).data_ptr()
        a.relu = 1
        a.o1_kind, a.qo1 = _lib.OUT_U8OFF, self.qd(ctx.quantizer("c1/X_range", 9, 2), inner)
        if o2:
            a.o2_kind, a.qo2 = _lib.OUT_U8OFF, self.qd(ctx.quantizer("cs/X_range", 9, 2), inner)
        a.rows, a.inner, a.C = N, inner, C

    def dev(self, x):
        t = torch.from_numpy(x).to(DEV)
        self.keep.append(t)
        return t

    def buf(self, shape, dtype):
        t = torch.full(tuple(shape), 77, dtype=dtype, device=DEV)
        self.keep.append(t)
        return t

    def qd(self, q, n):
        """q's descriptor without counters, its noise from a random table of n values in [0, 1)."""
        d = q.desc_nostats()
        d.noise = self.dev(self.rng.random(n, dtype=F32)).data_ptr()
        return d

    def chain(self, y, rout, o1, o2=False):
        """A copy of the chain with the chosen output buffers; returns (descriptor, buffers)."""
        from lbt_amd import _lib
        a = _lib.ChainFwd.from_buffer_copy(self.a)
        out = {}
        if y:
            out["y"] = self.buf(self.shp, torch.float32)
            a.y = out["y"].data_ptr()
        if rout:
            out["R1"] = self.buf(self.shp, torch.int8)
            a.b1.rout = out["R1"].data_ptr()
            if a.has_b2:
                out["R2"] = self.buf(self.shp, torch.int8)
                a.b2.rout = out["R2"].data_ptr()
        if o1:
            out["o1"] = self.buf(self.shp, torch.int8)
            a.o1 = out["o1"].data_ptr()
        if o2:
            out["o2"] = self.buf(self.shp, torch.int8)
            a.o2 = out["o2"].data_ptr()
        return a, out


def _st():
    from lbt_amd import _lib
    return _lib.stream()


def _fused(case, cv, y, opt=False):
    """The frozen lbt_conv_fwd_fused_i8 of conv cv on case's chain; opt: the optional outputs too."""
    from lbt_amd import _lib
    from lbt_amd.dfxp import ops
    C, H, N = case.C, case.H, case.N
    a, out = case.chain(y, opt, opt)
    cf = _lib.ConvFwd()
    cf.c = a
    cf.wf, cf.ksf, cf.w4, cf.wcolsum = cv.img.data_ptr(), cv.ksf, 1 if cv.w4 else 0, cv.colsum.data_ptr()
    cf.d = ops.conv_desc(N, H, case.W, C, C, 3, 3, 1, 1, "SAME")
    cf.qw = cv.qw
    out["yq"] = case.buf(case.shp, torch.int8)
    cf.yq = out["yq"].data_ptr()
    cf.qout = case.qd(case.ctx.quantizer("out%d/X_range" % len(case.ctx.quantizers), 8, 2), case.inner)
    return cf, out


def _two_launch(case, cv, cf, y):
    """lbt_bn_chain_fwd (frozen) + lbt_conv_fwd_i8 on the same operands: the expected values."""
    from lbt_amd import _lib
    a, out = case.chain(y, True, True)
    _lib.call("lbt_bn_chain_fwd", ctypes.byref(a), _st())
    out["yq"] = case.buf(case.shp, torch.int8)
    _lib.call("lbt_conv_fwd_i8w4" if cv.w4 else "lbt_conv_fwd_i8", _lib.ptr(out["o1"]), 1, _lib.ptr(cv.img), cv.ksf,
              _lib.ptr(cv.colsum), cf.d, a.qo1, cv.qw, None, _lib.ptr(out["yq"]), cf.qout, None, _st())
    return out


# (C, H, N, tile rows): the smallest batches that reach each tile height; 64 x 8 x 8 with an odd batch
SHAPES = [(16, 32, 2, 2), (16, 32, 32, 4), (16, 32, 64, 8), (32, 16, 2, 2), (32, 16, 64, 4), (64, 8, 3, 2),
          (64, 8, 128, 4)]
# (branches, residual, y): bn1's chain; a block end with the identity shortcut; with a projection shortcut
VARIANTS = [(1, False, False), (1, True, True), (2, False, True)]


@pytest.mark.parametrize("nb,res,y", VARIANTS)
@pytest.mark.parametrize("C,H,N,rows", SHAPES)
def test_frozen_fused_conv_equals_chain_then_conv(C, H, N, rows, nb, res, y):
    from lbt_amd import _lib
    lib = _lib.load()
    assert lib.lbt_conv_fused_tile_rows(C, N, H) == rows
    case = _Case(C, H, N, nb, res, seed=C + N + nb)
    cv = _Conv(case.ctx, case.rng, "c/W_range", 3, C, C, 8)
    cf, got = _fused(case, cv, y)
    want = _two_launch(case, cv, cf, y)
    assert lib.lbt_conv_fwd_fused_i8(ctypes.byref(cf), _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(got["yq"], want["yq"])
    if y:
        assert torch.equal(got["y"].view(torch.int32), want["y"].view(torch.int32))


@pytest.mark.parametrize("w4", [False, True])
def test_frozen_fused_conv_optional_outputs(w4):
    """With rout / o1 given the frozen launch also stores the chain's R and X codes; w4: the packed
    4-bit weight image."""
    from lbt_amd import _lib
    case = _Case(32, 16, 2, 2, False, seed=40 + w4)
    cv = _Conv(case.ctx, case.rng, "c/W_range", 3, 32, 32, 4 if w4 else 8)
    cf, got = _fused(case, cv, True, opt=True)
    want = _two_launch(case, cv, cf, True)
    assert _lib.load().lbt_conv_fwd_fused_i8(ctypes.byref(cf), _st()) == 0
    torch.cuda.synchronize()
    for k in ("yq", "R1", "R2", "o1"):
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got["y"].view(torch.int32), want["y"].view(torch.int32))


def _transition(C, w4, opt, seed):
    """The frozen lbt_conv_fwd2_fused_i8 descriptor of a C -> 2C transition at N = 2 (opt: with the optional
    outputs), its output buffers, and the expected values from lbt_bn_chain_fwd + lbt_conv_fwd_pair_i8."""
    from lbt_amd import _lib
    from lbt_amd.dfxp import ops
    H, N = 512 // C, 2
    case = _Case(C, H, N, 1, True, seed=seed, o2=True)
    bits = 4 if w4 else 8
    c1 = _Conv(case.ctx, case.rng, "c1/W_range", 3, C, 2 * C, bits)
    cs = _Conv(case.ctx, case.rng, "cs/W_range", 1, C, 2 * C, bits)
    d1 = ops.conv_desc(N, H, case.W, C, 2 * C, 3, 3, 2, 2, "SAME")
    ds = ops.conv_desc(N, H, case.W, C, 2 * C, 1, 1, 2, 2, "SAME")
    oshp = (N, d1.Ho, d1.Wo, 2 * C)
    inner_o = d1.Ho * d1.Wo * 2 * C
    q1 = case.qd(case.ctx.quantizer("n1/Xq_range", 8, 2), inner_o)
    qs = case.qd(case.ctx.quantizer("ns/Xq_range", 8, 2), inner_o)
    # expected: the chain's own launch, then the pair launch
    a, want = case.chain(True, True, True, o2=True)
    _lib.call("lbt_bn_chain_fwd", ctypes.byref(a), _st())
    jobs = []
    for cv, d, x, q, k in ((c1, d1, want["o1"], q1, "yq1"), (cs, ds, want["o2"], qs, "yqs")):
        want[k] = case.buf(oshp, torch.int8)
        jobs.append(_lib.ConvFwdJob(x.data_ptr(), 1, 1 if w4 else 0, cv.img.data_ptr(), cv.ksf, cv.colsum.data_ptr(), d,
                                    a.qo1 if cv is c1 else a.qo2, cv.qw, None, want[k].data_ptr(), q, None))
    _lib.call("lbt_conv_fwd_pair_i8", ctypes.byref(jobs[0]), ctypes.byref(jobs[1]), _st())
    # the frozen transition launch
    af, got = case.chain(True, opt, opt, o2=opt)
    cf = _lib.ConvFwd2()
    cf.c = af
    cf.wf1, cf.ksf1, cf.wcolsum1 = c1.img.data_ptr(), c1.ksf, c1.colsum.data_ptr()
    cf.wfs, cf.ksfs, cf.wcolsums = cs.img.data_ptr(), cs.ksf, cs.colsum.data_ptr()
    cf.w4, cf.d1, cf.ds, cf.qw1, cf.qws = 1 if w4 else 0, d1, ds, c1.qw, cs.qw
    got["yq1"], got["yqs"] = case.buf(oshp, torch.int8), case.buf(oshp, torch.int8)
    cf.yq1, cf.qout1, cf.yqs, cf.qouts = got["yq1"].data_ptr(), q1, got["yqs"].data_ptr(), qs
    return case, cf, got, want


@pytest.mark.parametrize("C,w4,opt", [(16, False, False), (32, False, True), (16, True, False)])
def test_frozen_transition_equals_chain_then_pair(C, w4, opt):
    """lbt_conv_fwd2_fused_i8 (frozen) against lbt_bn_chain_fwd + lbt_conv_fwd_pair_i8 on yq1, yqs and y."""
    from lbt_amd import _lib
    case, cf, got, want = _transition(C, w4, opt, seed=50 + C + w4)
    assert _lib.load().lbt_conv_fwd2_fused_i8(ctypes.byref(cf), _st()) == 0
    torch.cuda.synchronize()
    for k in ["yq1", "yqs"] + (["R1", "o1", "o2"] if opt else []):
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got["y"].view(torch.int32), want["y"].view(torch.int32))


def test_frozen_contract_refusals():
    """Mixed frozen / unfrozen branches, counters or channel sums on a frozen launch, and a training-mode
    launch without o1 all return LBT_EINVAL (host checks: nothing is launched)."""
    from lbt_amd import _lib
    lib = _lib.load()
    case = _Case(64, 8, 3, 2, False, seed=70)
    cv = _Conv(case.ctx, case.rng, "c/W_range", 3, 64, 64, 8)
    cf, _ = _fused(case, cv, True)
    sums = case.buf((_lib.NSHARD * 2 * 64,), torch.int64)
    counts = case.ctx.counts.data_ptr()

    def rc(edit):
        c = _lib.ConvFwd.from_buffer_copy(cf)
        edit(c)
        return lib.lbt_conv_fwd_fused_i8(ctypes.byref(c), _st())

    def mixed(c):
        c.c.b2.nrm.frozen = 0
        c.c.b2.nrm.chsum = sums.data_ptr()
    assert rc(mixed) == EINVAL
    assert rc(lambda c: setattr(c, "ychsum", sums.data_ptr())) == EINVAL
    assert rc(lambda c: setattr(c.qout, "counts", counts)) == EINVAL
    assert rc(lambda c: setattr(c.c.qo1, "counts", counts)) == EINVAL
    assert rc(lambda c: setattr(c.c.b1.qr, "counts", counts)) == EINVAL

    def training_without_o1(c):  # batch statistics, every other training-mode operand present
        for br in (c.c.b1, c.c.b2):
            br.nrm.frozen = 0
            br.nrm.chsum = sums.data_ptr()
            br.rout = case.buf(case.shp, torch.int8).data_ptr()
        c.ychsum = sums.data_ptr()
        c.c.o1 = None
    assert rc(training_without_o1) == EINVAL
    # the transition entry point: counters / channel sums on a frozen launch
    case2, cf2, _, _ = _transition(16, False, False, seed=71)

    def rc2(edit):
        c = _lib.ConvFwd2.from_buffer_copy(cf2)
        edit(c)
        return lib.lbt_conv_fwd2_fused_i8(ctypes.byref(c), _st())
    sums2 = case2.buf((_lib.NSHARD * 2 * 32,), torch.int64)
    assert rc2(lambda c: setattr(c.c.qo2, "counts", case2.ctx.counts.data_ptr())) == EINVAL
    assert rc2(lambda c: setattr(c.qouts, "counts", case2.ctx.counts.data_ptr())) == EINVAL
    assert rc2(lambda c: setattr(c, "ychsums", sums2.data_ptr())) == EINVAL
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ model level
def _batch(rng, B):
    x = ((rng.integers(0, 256, size=(B, 32, 32, 3)) - 127.5) / 128).astype(F32)
    return x, rng.integers(0, 10, B).astype(np.int32)


def _fused_trainer(seed, B=16, weight_bits=None, steps=2):
    """A graph-captured fused trainer after `steps` training steps at batch B (the running averages move)."""
    from lbt_amd.fused import FusedResNet
    from lbt_amd.models import CIFAR10_Resnet20
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    ctx = DfxpContext(seed=seed)
    gm = CIFAR10_Resnet20(8, weight_decay=2e-4, ctx=ctx, weight_bits=weight_bits)
    tr = Trainer(FusedResNet(gm), lr=1e-2, momentum=0.9, batch_size=B, use_graph=True)
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        x, y = _batch(rng, B)
        tr.step(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
    torch.cuda.synchronize()
    return ctx, gm, tr, rng


@pytest.fixture(scope="module")
def trained():
    return _fused_trainer(9)


def _layerwise_testing_logits(gm, x):
    gm.set_testing()
    try:
        return gm.forward(x).clone()
    finally:
        gm.set_training()


@pytest.mark.parametrize("B", [8, 3])
def test_inference_plan_matches_layerwise_and_oracle(trained, B):
    from lbt_amd.fused import FusedResNet
    ctx, gm, tr, _ = trained
    x, _ = _batch(np.random.default_rng(100 + B), B)
    xd = torch.from_numpy(x).to(DEV)
    got = FusedResNet(gm, inference=True).forward(xd).clone()
    assert torch.equal(got, _layerwise_testing_logits(gm, xd))
    om = oresnet.build_resnet((3, 3, 3), 8, 2e-4)
    oresnet.set_params(om, {o.name + {"W": "/W", "gamma": "/g", "beta": "/b"}[v]: getattr(o, v).cpu().numpy()
                            for o, v, _ in gm.param_slots()})
    for g_, o in zip(gm._norm_layers(), [l for l in oresnet._walk(om) if isinstance(l, onn.NormQ)]):
        o.mean_running = g_.X_mean_running.cpu().numpy().copy()
        o.var_running = g_.X_var_running.cpu().numpy().copy()
        o.train = False
    octx = onn.Ctx(ctx.ranges(), int(ctx.step.item()), 9)
    assert np.array_equal(got.cpu().numpy(), om.forward(x, octx))


@pytest.mark.parametrize("env", [{"LBT_FUSE_FWD": "0"}, {"LBT_FUSE_FWD": "0", "LBT_PAIR": "0"}, {"LBT_FUSE_FWD2": "0"}])
def test_inference_plan_fallback_launches(trained, env, monkeypatch):
    """Without the fused kernels the plan runs lbt_bn_chain_fwd (frozen) + lbt_conv_fwd_i8 / the pair launch:
    the same logits."""
    from lbt_amd.fused import FusedResNet
    ctx, gm, tr, _ = trained
    xd = torch.from_numpy(_batch(np.random.default_rng(108), 8)[0]).to(DEV)
    want = FusedResNet(gm, inference=True).forward(xd).clone()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plan = FusedResNet(gm, inference=True)
    got = plan.forward(xd)
    names = [f.kname for f in plan._fwd]
    assert ("conv_fwd_fused_kernel" in names) == ("LBT_FUSE_FWD" not in env) and "conv_fwd2_kernel" not in names
    assert torch.equal(got, want)


def test_inference_plan_w4_matches_layerwise():
    from lbt_amd.fused import FusedResNet
    ctx, gm, tr, rng = _fused_trainer(11, weight_bits=4)
    xd = torch.from_numpy(_batch(rng, 8)[0]).to(DEV)
    got = FusedResNet(gm, inference=True).forward(xd).clone()
    assert torch.equal(got, _layerwise_testing_logits(gm, xd))


def _state(ctx, gm):
    s = [ctx.exps, ctx.counts, ctx.step, ctx.nelem]
    for n in gm._norm_layers():
        s += [n.X_mean_running, n.X_var_running, n.ms]
    return s


def test_inference_forward_leaves_training_state(trained):
    from lbt_amd.fused import FusedResNet
    ctx, gm, tr, _ = trained
    xd = torch.from_numpy(_batch(np.random.default_rng(5), 8)[0]).to(DEV)
    before = [t.clone() for t in _state(ctx, gm)]
    nelem = [q._nelem for q in ctx.quantizers]
    plan = FusedResNet(gm, inference=True)
    a = plan.forward(xd).clone()
    b = plan.forward(xd).clone()
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    for t0, t1 in zip(before, _state(ctx, gm)):
        assert torch.equal(t0.view(torch.uint8), t1.view(torch.uint8))
    assert nelem == [q._nelem for q in ctx.quantizers]


def test_inference_forward_between_graph_replays():
    """Two graph-captured trainers from one seed take three steps; one runs an inference forward between
    steps 2 and 3: weights, exponents and running statistics end bit-equal."""
    from lbt_amd.fused import FusedResNet
    ctx_a, gm_a, tr_a, rng_a = _fused_trainer(13)
    ctx_b, gm_b, tr_b, rng_b = _fused_trainer(13)
    xe = torch.from_numpy(_batch(np.random.default_rng(6), 8)[0]).to(DEV)
    FusedResNet(gm_a, inference=True).forward(xe)
    for tr, rng in ((tr_a, rng_a), (tr_b, rng_b)):
        x, y = _batch(rng, 16)
        tr.step(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(tr_a.flat.w.view(torch.int32), tr_b.flat.w.view(torch.int32))
    assert torch.equal(ctx_a.exps, ctx_b.exps) and torch.equal(ctx_a.step, ctx_b.step)
    for na, nb in zip(gm_a._norm_layers(), gm_b._norm_layers()):
        assert torch.equal(na.X_mean_running.view(torch.int32), nb.X_mean_running.view(torch.int32))
        assert torch.equal(na.X_var_running.view(torch.int32), nb.X_var_running.view(torch.int32))


def test_evaluate_testing_fused_equals_layerwise():
    """40 samples at batch 16 (16, 16, 8): evaluate(testing=True) of the fused trainer equals the layer-wise
    trainer's with the same parameters, running statistics, exponents and step; the default evaluate
    returns what it returned before."""
    from lbt_amd.models import CIFAR10_Resnet20
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    ctx, gm, tr, rng = _fused_trainer(17)
    ctx_l = DfxpContext(seed=17)
    gm_l = CIFAR10_Resnet20(8, weight_decay=2e-4, ctx=ctx_l)
    tr_l = Trainer(gm_l, lr=1e-2, momentum=0.9, batch_size=16, use_graph=False)
    X = ((rng.integers(0, 256, size=(40, 32, 32, 3)) - 127.5) / 128).astype(F32)
    Y = rng.integers(0, 10, size=40).astype(np.int32)
    default = tr.evaluate(X, Y, batch_size=16)  # (training mode: it moves the running averages, as the reference's)
    tr_l.flat.w.copy_(tr.flat.w)
    ctx_l.exps.copy_(ctx.exps)
    ctx_l.step.copy_(ctx.step)
    for n, nl in zip(gm._norm_layers(), gm_l._norm_layers()):
        nl.X_mean_running.copy_(n.X_mean_running)
        nl.X_var_running.copy_(n.X_var_running)
    got = tr.evaluate(X, Y, batch_size=16, testing=True)
    want = tr_l.evaluate(X, Y, batch_size=16, testing=True)
    assert got == want
    assert sorted(k for k in tr._eval if isinstance(k, tuple)) == [("testing", 8), ("testing", 16)]
    assert tr.evaluate(X, Y, batch_size=16) == default
    assert gm_l.training and all(n.train for n in gm_l._norm_layers())


def test_inference_plan_is_forward_only(trained):
    from lbt_amd.fused import FusedResNet
    ctx, gm, tr, _ = trained
    x, y = _batch(np.random.default_rng(7), 8)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    plan = FusedResNet(gm, inference=True)
    plan.forward(xd)
    assert np.isfinite(plan.compute_loss(yd).item())
    with pytest.raises(RuntimeError, match="inference"):
        plan.backward()
    with pytest.raises(RuntimeError, match="inference"):
        plan.train_fwd_bwd(xd, yd)
    gm.set_testing()
    try:  # a testing-mode model without inference=True still refuses, naming the keyword
        with pytest.raises(NotImplementedError, match="inference=True"):
            FusedResNet(gm).forward(xd)
    finally:
        gm.set_training()

"""The whole ``--bits`` domain (``main.py:113``, ``1 <= bits <= 32``) against the numpy oracle.

The rest of the suite pins ``bits = 8`` (with ``weight_bits = 4`` or ``grad_bits = 16`` beside it) and
``bits >= 17``. Here: 3..7 bits (signed int8 X codes on the int8 kernels, no offset / column-sum
correction, the first conv as a generic conv) and 9..16 bits (float mode: the codes no longer fit the
int8 weight / BN images, so the layers contract the fake-quantised fp32 values, ``fp32.hip``).

CPU (unmarked): every model builder at every width -- the operand type each layer will ask a kernel
for can hold its quantiser's codes, and the int32 accumulators cannot overflow; the dispatch of the
layer cases below; the edge of the exponent domain; FusedResNet's refusal of widths its plan does not
hard-code.

GPU: one layer at a time and whole optimiser steps, by the method of ``tests/test_gpu_parity.py`` (the
GPU's d loss / d logits injected into the oracle, everything else equal).

Tolerance. Everything is asserted BIT-EXACT, the 9..16-bit float path included: its codes have at
most 17 bits, every product is below 2**33 and every sum here has fewer than 2**20 terms, so the
kernels' double accumulators and the oracle's int64 / float64 sums are both exact, and the power-of-
two scaling commutes with the one rounding to fp32. The softmax alone keeps the suite's bounds (loss
1e-5 relative; d loss / d logits rtol 1e-5, atol 1e-9).

Inputs and initial ranges are chosen so that low widths do not collapse everything to zero; each test
asserts on the ORACLE's records that it is not vacuous (share of non-zero codes, distinct codes,
overflow counters, gradients that differ from their weight-decay term, exponents that move).
"""
import numpy as np
import pytest
import torch

from lbt_amd import dynamic_fixed_point as D
from lbt_amd import models
from lbt_amd._lib import OUT_F32, OUT_I8, OUT_I16, OUT_U8OFF
from lbt_amd.dfxp import layers as L
from lbt_amd.runtime import DfxpContext
from oracle import dfxp as odfxp
from oracle import nn as onn
from oracle import resnet as oresnet

DEV = "cuda"
F32 = np.float32
WD = 2e-4


# =============================================================================== CPU: part 1
def _imagenet(bits, ctx, grad_bits=None):
    return models.ImageNet_Resnet(bits, (1, 1, 1, 1), grad_bits=grad_bits, width=8, image=32, classes=10, ctx=ctx)


BUILDERS = {
    "resnet20": lambda bits, ctx: models.CIFAR10_Resnet20(bits, ctx=ctx),
    "pi_mnist": lambda bits, ctx: models.PI_MNIST_Model(bits, ctx=ctx),
    "mnist": lambda bits, ctx: models.MNIST_Model(bits, ctx=ctx),
    "cifar10": lambda bits, ctx: models.CIFAR10_Model(bits, ctx=ctx),
    # the reference's widths where the accumulator bound depends on them (integer mode), a narrow
    # instance above (float mode is decided by the widths alone)
    "vgg": lambda bits, ctx: (models.CIFAR10_VGG_Model(bits, ctx=ctx) if bits <= 8 else
                              models.CIFAR10_VGG_Model(bits, ctx=ctx, width=16, dense_units=64)),
    "imagenet": _imagenet,
    "imagenet_g16": lambda bits, ctx: _imagenet(bits, ctx, 16),
}
QLAYERS = (L.Conv2d_q, L.Dense_q, L.Normalization_q, L.Rescale_q)


def _operand_errors(l):
    """What is wrong with the operand types layer `l` will ask its kernels for ([] = nothing)."""
    gemm = isinstance(l, (L.Conv2d_q, L.Dense_q))
    xb, gb = l.X_range.bits, l.grad_range.bits
    wb = l.W_range.bits if gemm else None
    # Normalization_q / Rescale_q have no x_kind: their integer paths write int8 codes (q, R)
    kind = l.x_kind if gemm else (OUT_F32 if l.fmode else OUT_I8)
    errs = []
    fits = l.bits <= 8 and (wb is None or wb <= 8) and gb <= 16
    if l.fmode != (not fits):
        errs.append("fmode=%s with bits=%d weight_bits=%s grad_bits=%d" % (l.fmode, l.bits, wb, gb))
    if l.fmode:
        if kind != OUT_F32:
            errs.append("float mode asks for operand kind %d" % kind)
        return errs
    if kind == OUT_I8:
        ok = xb <= 8
    elif kind == OUT_U8OFF:
        ok = xb <= 9 and l.input_nonnegative
    elif kind == OUT_I16:
        ok = xb <= 16
    else:
        ok = False
    if not ok:
        errs.append("X codes of %d bits in operand kind %d" % (xb, kind))
    if wb is not None and wb > 8:
        errs.append("%d-bit weight codes in the int8 weight images" % wb)
    # the layers pick int16 gradient codes when grad_bits > 8, int8 ones otherwise
    if gb > (16 if l.grad_bits > 8 else 8) or gb != l.grad_bits:
        errs.append("%d-bit gradient codes" % gb)
    if gemm:
        K = l.ksize[0] * l.ksize[1] * l.ksize[2] if isinstance(l, L.Conv2d_q) else l.in_units
        if K * 2 ** (xb - 1) * 2 ** (wb - 1) >= 2 ** 31:
            errs.append("int32 accumulator: K=%d, %d-bit X, %d-bit W" % (K, xb, wb))
    return errs


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_operand_types_hold_the_codes_at_every_width(name):
    """Every Conv2d_q / Dense_q / Normalization_q / Rescale_q of every model, nested blocks included,
    at every width 3..31 (the ImageNet model also with 16-bit gradients at bits <= 8): OUT_I8 needs
    X bits <= 8, OUT_U8OFF <= 9 and a non-negative input, OUT_I16 <= 16; int8 weight images need
    weight_bits <= 8; int8 / int16 gradient codes grad_bits <= 8 / 16; anything else is in float mode
    (and nothing that fits is); K * 2^(xbits-1) * 2^(wbits-1) < 2^31 for every integer conv / dense
    (the int32 accumulators of conv_fwd_generic_kernel and the MFMA kernels)."""
    bad = []
    for bits in (range(3, 9) if name == "imagenet_g16" else range(3, 32)):
        model = BUILDERS[name](bits, DfxpContext(device="cpu", seed=0))
        layers = [l for l in model._walk() if isinstance(l, QLAYERS)]
        assert len(layers) >= 3
        for l in layers:
            bad += ["bits %d, %s: %s" % (bits, l.name, e) for e in _operand_errors(l)]
    assert not bad, "%d operand errors, first: %s" % (len(bad), "; ".join(bad[:6]))


def test_exponent_domain_edge():
    """bits = 2 with the default initial range 2 is outside 0 <= bits - I - 1 <= 30 on both sides (so 3
    is the smallest width of a model with default ranges); bits = 2 with range 1 is inside."""
    ctx = DfxpContext(device="cpu", seed=0)
    with pytest.raises(ValueError):
        ctx.quantizer("a/X_range", 2, 2)
    with pytest.raises(ValueError):
        odfxp.frac_bits(2, 2)
    with pytest.raises(ValueError):
        models.MNIST_Model(2, ctx=DfxpContext(device="cpu", seed=0))
    assert ctx.quantizer("b/X_range", 2, 1).bits == 2
    assert odfxp.frac_bits(2, 1) == 0
    x = np.array([-1.6, -0.4, 0.4, 1.6], F32)
    assert list(odfxp.quantize_int(x, 2, 1, False)) == [-2, 0, 0, 1]  # codes -2..1 at 2**0


@pytest.mark.parametrize("bits,weight_bits", [(9, None), (12, None), (16, None), (20, None), (32, None), (8, 12)])
def test_fused_resnet_refuses_widths_its_plan_does_not_hold(bits, weight_bits):
    """FusedResNet's launches read int8 / offset-int8 / int16 codes only; a model with a float-mode
    layer is refused in the constructor, before anything is allocated or launched, naming the width."""
    from lbt_amd.fused import FusedResNet
    gm = models.CIFAR10_Resnet20(bits, ctx=DfxpContext(device="cpu", seed=0), weight_bits=weight_bits)
    with pytest.raises(NotImplementedError, match="bits=%d, weight_bits=%d" % (bits, weight_bits or bits)):
        FusedResNet(gm)


def test_fused_resnet_refuses_other_layouts():
    from lbt_amd.fused import FusedResNet
    with pytest.raises(NotImplementedError, match="CIFAR ResNet layout"):
        FusedResNet(models.MNIST_Model(8, ctx=DfxpContext(device="cpu", seed=0)))
    with pytest.raises(NotImplementedError, match="CIFAR ResNet layout"):
        FusedResNet(_imagenet(8, DfxpContext(device="cpu", seed=0)))


# =============================================================================== layer cases (part 3)
# (bits, grad_bits, weight_bits)
WIDTHS = [(3, None, None), (4, None, None), (6, None, None), (7, None, None), (9, None, None), (12, None, None),
          (15, None, None), (16, None, None), (6, 16, None), (4, 8, None), (12, None, 8)]
WIDTH_IDS = ["b%d%s%s" % (b, "-g%d" % g if g else "", "-w%d" % w if w else "") for b, g, w in WIDTHS]

# name -> (N, H, Cin, Cout, k, stride, padding, nonneg, bias)
CONVS = {
    "mfma_16_16": (4, 12, 16, 16, 3, 1, "SAME", False, False),
    "mfma_32_16_s2": (4, 9, 32, 16, 3, 2, "SAME", True, False),
    "igemm_128_192": (2, 9, 128, 192, 3, 1, "SAME", False, False),
    "igemm_64_256_1x1": (2, 8, 64, 256, 1, 1, "SAME", True, False),
    "first_3_32_s2": (5, 7, 3, 32, 3, 2, "SAME", False, False),
    "generic_6_10_5x5": (3, 6, 6, 10, 5, 1, "VALID", False, True),
}
DENSES = {"d64_10": (33, 64, 10, False), "d128_40": (7, 128, 40, True)}  # N, in, out, bias


def _is_float(bits, gb, wb):
    return bits > 8 or (wb or bits) > 8 or (gb or bits) > 16


def _conv_path(case, bits, gb, wb):
    """The dispatch a Conv2d_q case must take: dict of the layer attributes that select its kernels.
    Pinned, so that a later change of dispatch cannot empty a case."""
    if _is_float(bits, gb, wb):
        return dict(fmode=True, x_kind=OUT_F32, mfma=False, x_mfma=False, igemm_f=False, igemm_d=False, w4=False)
    g8 = (gb or bits) <= 8
    small = case.startswith("mfma")
    wide = case.startswith("igemm")
    # bits <= 7: signed int8 X codes whatever the sign of the input; no offset, no column sums
    return dict(fmode=False, x_kind=OUT_I8, mfma=small and g8, x_mfma=small and g8,
                igemm_f=wide, igemm_d=wide, igemm_w=False,
                w4=small and g8 and (wb or bits) <= 4)


def _check_path(gl, want):
    got = {k: getattr(gl, k) for k in want}
    assert got == want, (got, want)


@pytest.mark.parametrize("bits,gb,wb", WIDTHS, ids=WIDTH_IDS)
def test_layer_case_dispatch(bits, gb, wb):
    """CPU: which kernels every layer case of part 3 selects (the GPU tests assert the same)."""
    ctx = DfxpContext(device="cpu", seed=0)
    for case, (N, H, Cin, Cout, k, s, pad, nonneg, bias) in CONVS.items():
        gl = D.Conv2d_q(case, bits, [k, k, Cin, Cout], [1, s, s, 1], pad, use_bias=bias, input_nonnegative=nonneg,
                        grad_bits=gb, weight_bits=wb, ctx=ctx)
        _check_path(gl, _conv_path(case, bits, gb, wb))
        if not gl.fmode:
            d = D.ops.conv_desc(N, H, H, Cin, Cout, k, k, s, s, pad)
            assert not gl.stem(d) and not gl.stem_wide(d)  # below 8 bits the first conv is a generic conv
    for case, (N, i, o, bias) in DENSES.items():
        gl = D.Dense_q(case, bits, i, o, use_bias=bias, grad_bits=gb, weight_bits=wb, ctx=ctx)
        fl = _is_float(bits, gb, wb)
        assert (gl.fmode, gl.x_kind, gl.mfma) == (fl, OUT_F32 if fl else OUT_I8, case == "d128_40" and not fl)


def _ilog2_ceil(v):
    return int(np.ceil(np.log2(v)))


def _spread(rng, shape, I, nonneg=False):
    """Uniform in +-1.5 * 2**I (or [0, 1.5 * 2**I)): a third of it beyond the quantiser's range."""
    hi = 1.5 * 2.0 ** I
    return rng.uniform(0 if nonneg else -hi, hi, size=shape).astype(F32)


def _x_codes(gl, kind):
    a = gl.cpu().numpy()
    return a.astype(np.int32) + 128 if kind == OUT_U8OFF else a


def _same_codes(got, kind, rec, bits, I, what):
    """GPU operand (integer codes, or the fake-quantised fp32 values in float mode) == the oracle's codes."""
    if kind == OUT_F32:
        assert np.array_equal(got, odfxp.dequant(rec, odfxp.frac_bits(bits, I))), what
    else:
        assert np.array_equal(got.astype(np.int64), rec), what


def _not_vacuous(rec, bits, what, share=0.25):
    nz = np.count_nonzero(rec) / rec.size
    assert nz >= share, "%s: only %.1f%% of the codes are non-zero" % (what, 100 * nz)
    assert len(np.unique(rec)) >= min(3, 2 ** bits), what


X_I, G_I, B_I = 1, -4, -2  # initial ranges of the layer cases: X, gradient, bias


@pytest.mark.gpu
@pytest.mark.parametrize("bits,gb,wb", WIDTHS, ids=WIDTH_IDS)
@pytest.mark.parametrize("case", sorted(CONVS))
def test_conv_layer_across_widths(case, bits, gb, wb):
    """Conv2d_q against oracle.nn.Conv2dQ by the method of test_conv_layer_bitexact: X codes, y, gradient
    codes, dW, db, dX, then the exponent update -- all bit-exact, at every width and on every kernel
    family (register MFMA with signed / W4 operands, LDS-tiled igemm forward / dgrad, generic int8,
    int16-gradient generic kernels, the fp32 path)."""
    N, H, Cin, Cout, k, s, pad, nonneg, bias = CONVS[case]
    seed = 100 + bits
    rng = np.random.default_rng([bits, gb or 0, wb or 0, Cin, Cout])
    ctx = DfxpContext(seed=seed)
    W_I = _ilog2_ceil((3 / (k * k * Cin)) ** 0.5)  # the weights fill their range
    gl = D.Conv2d_q("c", bits, [k, k, Cin, Cout], [1, s, s, 1], pad, use_bias=bias, weight_decay=WD,
                    input_range=X_I, weight_range=W_I, bias_range=B_I, grad_range=G_I, input_nonnegative=nonneg,
                    grad_bits=gb, weight_bits=wb, ctx=ctx)
    _check_path(gl, _conv_path(case, bits, gb, wb))
    ol = onn.Conv2dQ("c", bits, [k, k, Cin, Cout], [1, s, s, 1], pad, WD, grad_bits=gb, weight_bits=wb, use_bias=bias)
    ol.W = gl.W.cpu().numpy().copy()
    ranges = {"c/W_range": W_I, "c/X_range": X_I, "c/grad_range": G_I}
    if bias:
        b = rng.uniform(-0.2, 0.2, size=Cout).astype(F32)
        gl.b.copy_(torch.from_numpy(b))
        ol.b = b.copy()
        ranges["c/b_range"] = B_I
    assert ctx.ranges() == ranges
    octx = onn.Ctx(dict(ranges), 0, seed)
    x = _spread(rng, (N, H, H, Cin), X_I, nonneg)
    y = gl.forward(torch.from_numpy(x).to(DEV))
    yr = ol.forward(x, octx)
    xrec = octx.record["c/X_range"]
    _not_vacuous(xrec, bits + 1, "X")
    c1, c2, _, _ = octx.counts["c/X_range"]
    assert c1 > 0 and c2 > c1, "both overflow counters of the X quantiser must count"
    assert len(np.unique(octx.record["c/W_range"])) >= 3
    _same_codes(_x_codes(gl.xq, gl.x_kind), gl.x_kind, xrec, bits + 1, X_I, "X codes")
    assert np.array_equal(y.cpu().numpy(), yr), "y"
    g = _spread(rng, yr.shape, G_I)
    dx = gl.backward(torch.from_numpy(g).to(DEV))
    dxr = ol.backward(g, octx)
    grec = octx.record["c/grad_range"]
    _not_vacuous(grec, gb or bits, "gradient")
    _same_codes(gl.gradq.cpu().numpy(), gl.x_kind if gl.fmode else OUT_I8, grec, gb or bits, G_I, "gradient codes")
    assert gl.gradq.dtype == (torch.float32 if gl.fmode else torch.int16 if (gb or bits) > 8 else torch.int8)
    assert np.array_equal(gl.dW.cpu().numpy(), ol.dW), "dW"
    assert not np.array_equal(ol.dW, (F32(2 * WD) * ol.W).astype(F32))
    if bias:
        assert np.array_equal(gl.db.cpu().numpy(), ol.db), "db"
    assert np.array_equal(dx.cpu().numpy(), dxr), "dX"
    assert np.count_nonzero(dxr) >= dxr.size // 4
    ctx.update_range_op()
    new = octx.new_ranges()
    assert ctx.ranges() == new
    assert new["c/X_range"] == min(X_I + 1, bits)  # the overflow moved it (clamped at bits + 1 - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("bits,gb,wb", WIDTHS, ids=WIDTH_IDS)
@pytest.mark.parametrize("case", sorted(DENSES))
def test_dense_layer_across_widths(case, bits, gb, wb):
    """Dense_q (generic int8 kernels at 64 -> 10, the int8-MFMA dense kernels at 128 -> 40 with a bias,
    int16 gradient codes, the fp32 path) against oracle.nn.DenseQ, bit-exact."""
    N, i, o, bias = DENSES[case]
    seed = 200 + bits
    rng = np.random.default_rng([bits, gb or 0, wb or 0, i, o])
    ctx = DfxpContext(seed=seed)
    W_I = _ilog2_ceil((6 / (i + o)) ** 0.5)
    gl = D.Dense_q("fc", bits, i, o, use_bias=bias, weight_decay=WD, input_range=X_I, weight_range=W_I,
                   bias_range=B_I, grad_range=G_I, grad_bits=gb, weight_bits=wb, ctx=ctx)
    fl = _is_float(bits, gb, wb)
    assert (gl.fmode, gl.x_kind, gl.mfma) == (fl, OUT_F32 if fl else OUT_I8, case == "d128_40" and not fl)
    ol = onn.DenseQ("fc", bits, i, o, WD, use_bias=bias, grad_bits=gb, weight_bits=wb)
    ol.W = gl.W.cpu().numpy().copy()
    ranges = {"fc/W_range": W_I, "fc/X_range": X_I, "fc/grad_range": G_I}
    if bias:
        b = rng.uniform(-0.2, 0.2, size=o).astype(F32)
        gl.b.copy_(torch.from_numpy(b))
        ol.b = b.copy()
        ranges["fc/b_range"] = B_I
    assert ctx.ranges() == ranges
    octx = onn.Ctx(dict(ranges), 0, seed)
    x = _spread(rng, (N, i), X_I)
    y = gl.forward(torch.from_numpy(x).to(DEV))
    yr = ol.forward(x, octx)
    xrec = octx.record["fc/X_range"]
    _not_vacuous(xrec, bits, "X")
    c1, c2, _, _ = octx.counts["fc/X_range"]
    assert c1 > 0 and c2 > c1
    _same_codes(gl.xq.cpu().numpy(), gl.x_kind, xrec, bits, X_I, "X codes")
    assert np.array_equal(y.cpu().numpy(), yr), "y"
    g = _spread(rng, (N, o), G_I)
    dx = gl.backward(torch.from_numpy(g).to(DEV))
    dxr = ol.backward(g, octx)
    grec = octx.record["fc/grad_range"]
    _not_vacuous(grec, gb or bits, "gradient")
    _same_codes(gl.gradq.cpu().numpy(), gl.x_kind if fl else OUT_I8, grec, gb or bits, G_I, "gradient codes")
    assert np.array_equal(gl.dW.cpu().numpy(), ol.dW), "dW"
    if bias:
        assert np.array_equal(gl.db.cpu().numpy(), ol.db), "db"
    assert np.array_equal(dx.cpu().numpy(), dxr), "dX"
    ctx.update_range_op()
    assert ctx.ranges() == octx.new_ranges()


BN_WIDTHS = [w for w in WIDTHS if w[2] is None]  # BatchNorm_q has no weight_bits


@pytest.mark.gpu
@pytest.mark.parametrize("bits,gb,wb", BN_WIDTHS, ids=[i for i, w in zip(WIDTH_IDS, WIDTHS) if w[2] is None])
@pytest.mark.parametrize("shape", [(6, 5, 7, 4), (16, 8, 8, 64)])
def test_batchnorm_across_widths(shape, bits, gb, wb):
    """BatchNorm_q (gamma and beta as in test_batchnorm_bitexact) against oracle.nn.BatchNormQ: the
    int8 chain kernels at <= 8 bits, the int16-gradient BN kernels at (6, 16), the fp32 BN at 9..16
    bits -- y, dgamma, dbeta, dX, the running averages and the exponent update, bit-exact."""
    seed = 300 + bits
    rng = np.random.default_rng([bits, gb or 0, shape[0]])
    C = shape[-1]
    ctx = DfxpContext(seed=seed)
    gbn = D.BatchNorm_q("bn", bits, C, weight_decay=WD, input_range=X_I, grad_range=G_I, grad_bits=gb, ctx=ctx)
    obn = onn.BatchNormQ("bn", bits, C, WD, grad_bits=gb)
    fl = _is_float(bits, gb, None)
    assert [l.fmode for l in gbn.layers] == [fl, fl]
    gam = (1 + 0.2 * rng.standard_normal(C)).astype(F32)
    bet = (0.2 * rng.standard_normal(C)).astype(F32)
    gbn.layers[1].gamma.copy_(torch.from_numpy(gam))
    gbn.layers[1].beta.copy_(torch.from_numpy(bet))
    obn.layers[1].gamma, obn.layers[1].beta = gam.copy(), bet.copy()
    ranges = {"bn-norm/X_range": X_I, "bn-norm/grad_range": G_I, "bn-rescale/g_range": 2, "bn-rescale/b_range": 2,
              "bn-rescale/X_range": 2, "bn-rescale/grad_range": G_I}
    assert ctx.ranges() == ranges
    octx = onn.Ctx(dict(ranges), 0, seed)
    x = (rng.standard_normal(shape) * 1.3 + 0.4).astype(F32)
    y = gbn.forward(torch.from_numpy(x).to(DEV))
    yr = obn.forward(x, octx)
    _not_vacuous(octx.record["bn-norm/X_range"], bits, "X")
    _not_vacuous(octx.record["bn-rescale/X_range"], bits, "rescale X")
    c1, c2, _, _ = octx.counts["bn-norm/X_range"]
    assert c1 > 0 and c2 > c1
    assert np.array_equal(y.cpu().numpy(), yr), "y"
    g = _spread(rng, shape, G_I)
    dx = gbn.backward(torch.from_numpy(g).to(DEV))
    dxr = obn.backward(g, octx)
    _not_vacuous(octx.record["bn-rescale/grad_range"], gb or bits, "rescale gradient")
    _not_vacuous(octx.record["bn-norm/grad_range"], gb or bits, "norm gradient")
    assert np.array_equal(gbn.layers[1].dgamma.cpu().numpy(), obn.layers[1].dgamma), "dgamma"
    assert np.array_equal(gbn.layers[1].dbeta.cpu().numpy(), obn.layers[1].dbeta), "dbeta"
    assert np.array_equal(dx.cpu().numpy(), dxr), "dX"
    assert np.array_equal(gbn.layers[0].X_mean_running.cpu().numpy(), obn.layers[0].mean_running)
    assert np.array_equal(gbn.layers[0].X_var_running.cpu().numpy(), obn.layers[0].var_running)
    ctx.update_range_op()
    assert ctx.ranges() == octx.new_ranges()


# =============================================================================== whole steps (part 4)
GRAD_I = -6  # every */grad_range of the ResNet step tests (the default 2 leaves low widths all-zero)
SUF = {"W": "/W", "gamma": "/g", "beta": "/b"}


def _resnet_pair(bits, seed):
    ctx = DfxpContext(seed=seed)
    gm = models.CIFAR10_Resnet20(bits, weight_decay=WD, ctx=ctx, grad_range=GRAD_I)
    om = oresnet.build_resnet((3, 3, 3), bits, WD)
    ranges = {r: (GRAD_I if r.endswith("/grad_range") else 2) for r in om.range_names()}
    return ctx, gm, om, ranges


def _batch(B, seed):
    rng = np.random.default_rng(seed)
    x = ((rng.integers(0, 256, size=(B, 32, 32, 3)) - 127.5) / 128).astype(F32)
    return x, rng.integers(0, 10, size=B).astype(np.int32)


def _flat(tr, buf):
    return {o.name + SUF[v]: buf[off:off + sz].view(getattr(o, v).shape).cpu().numpy().copy()
            for o, v, off, sz in tr.flat.offsets}


def _step_not_vacuous(octx, grads, params, moved, tag):
    for name, rec in octx.record.items():
        if name.endswith("/grad_range"):
            nz = np.count_nonzero(rec) / rec.size
            assert nz >= 0.01, "%s: %s has %.2f%% non-zero gradient codes" % (tag, name, 100 * nz)
    for k, g in grads.items():
        if k.endswith("/W"):
            assert not np.array_equal(g, (F32(2 * WD) * params[k]).astype(F32)), (tag, k)
    assert moved > 0, tag


def _two_steps(tr, ctx, om, ranges, model, B, seed):
    """Two optimiser steps against the oracle (the GPU's d loss / d logits injected): gradients,
    parameters, momentum, exponents and the step counter equal after each; the exponents moved by
    step 1 feed step 2. model: where dlogits lives (the layer-wise model or the fused plan)."""
    state = dict(params=_flat(tr, tr.flat.w), ranges=dict(ranges), step=0)
    state["accum"] = {k: np.zeros_like(v) for k, v in state["params"].items()}
    assert ctx.ranges() == ranges
    for i in range(2):
        x, y = _batch(B, seed=40 + 2 * seed + i)
        before = state
        loss = tr.step(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)).item()
        torch.cuda.synchronize()
        dz = model.dlogits.cpu().numpy()
        lref, state, octx = oresnet.train_step(om, state, x, y, lr=1e-2, momentum=0.9, seed=seed, dz=dz)
        assert abs(loss - lref) <= 1e-5 * abs(lref), (i, loss, lref)
        np.testing.assert_allclose(dz, octx.dz, rtol=1e-5, atol=1e-9)
        grads = oresnet.get_grads(om)
        moved = sum(state["ranges"][k] != before["ranges"][k] for k in state["ranges"])
        _step_not_vacuous(octx, grads, before["params"], moved, "step %d" % i)
        gg, gw, ga = _flat(tr, tr.flat.g), _flat(tr, tr.flat.w), _flat(tr, tr.flat.a)
        assert gw.keys() == state["params"].keys()
        for k in gw:
            assert np.array_equal(gg[k], grads[k]), (i, "grad", k)
            assert np.array_equal(gw[k], state["params"][k]), (i, "param", k)
            assert np.array_equal(ga[k], state["accum"][k]), (i, "momentum", k)
        assert ctx.ranges() == state["ranges"], i
        assert int(ctx.step.item()) == state["step"]


@pytest.mark.gpu
@pytest.mark.parametrize("bits,use_graph", [(4, False), (6, False), (6, True), (12, False), (16, False)])
def test_resnet20_two_steps_across_widths(bits, use_graph):
    """The layer-wise ResNet-20 at B = 4: 4 bits (W4 packed weights, signed int8 X codes), 6 bits (also
    through a captured graph), 12 and 16 bits (every layer in float mode)."""
    from lbt_amd.trainer import Trainer
    seed = bits
    ctx, gm, om, ranges = _resnet_pair(bits, seed)
    convs = [l for l in gm._walk() if isinstance(l, L.Conv2d_q)]
    assert all(c.fmode == (bits > 8) for c in convs)
    if bits <= 8:
        assert all(c.x_kind == OUT_I8 for c in convs) and all(c.mfma for c in convs[1:]) and not convs[0].mfma
        assert all(c.w4 == (bits <= 4) for c in convs[1:])
    tr = Trainer(gm, lr=1e-2, momentum=0.9, batch_size=4, use_graph=use_graph)
    _two_steps(tr, ctx, om, ranges, gm, 4, seed)
    assert (tr._graphs is not None) == use_graph


@pytest.mark.gpu
@pytest.mark.parametrize("bits,B", [(4, 4), (6, 4), (4, 32), (6, 32)])
def test_fused_resnet_below_8_bits(bits, B):
    """FusedResNet at 4 and 6 bits: its offset-int8 block inputs hold the (bits + 1)-bit codes of a post-
    ReLU tensor (0 .. 2**bits - 1), so the plan runs these widths. One forward / backward bit-identical
    to the layer-wise model (as test_fused_executor_bitidentical_to_layerwise), then two captured
    optimiser steps against the oracle."""
    from lbt_amd.fused import FusedResNet
    from lbt_amd.trainer import Trainer
    seed = 10 + bits
    x, y = _batch(B, seed=5)
    xt, yt = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    ctxA, A, _, _ = _resnet_pair(bits, seed)
    ctxB, gmB, _, _ = _resnet_pair(bits, seed)
    Bm = FusedResNet(gmB)
    assert np.array_equal(A.forward(xt).cpu().numpy(), Bm.forward(xt).cpu().numpy())
    assert A.compute_loss(yt).item() == Bm.compute_loss(yt).item()
    A.backward()
    Bm.backward()
    for (oa, va, ga), (ob, vb, gb_) in zip(A.param_slots(), gmB.param_slots()):
        assert np.array_equal(getattr(oa, ga).cpu().numpy(), getattr(ob, gb_).cpu().numpy()), oa.name + SUF[va]
    ctxA.update_range_op()
    ctxB.update_range_op()
    assert ctxA.ranges() == ctxB.ranges()
    ctx, gm, om, ranges = _resnet_pair(bits, seed)
    fm = FusedResNet(gm)
    tr = Trainer(fm, lr=1e-2, momentum=0.9, batch_size=B, use_graph=True)
    _two_steps(tr, ctx, om, ranges, fm, B, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("bits,gb", [(6, None), (6, 16), (12, None)])
def test_bottleneck_net_across_widths(bits, gb):
    """ImageNet_Resnet((1,1,1,1), width 8, 32x32, 10 classes) at B = 2 by the method of
    test_resnet50_layers_bitexact_vs_oracle: 6 bits (int8 everywhere, the 7x7 conv1 generic), 6 bits with
    16-bit gradients (int16 gradient codes on int8 X codes; the fused block path needs offset codes and
    is not taken), 12 bits (float mode)."""
    ctx = DfxpContext(seed=bits)
    gm = models.ImageNet_Resnet(bits, (1, 1, 1, 1), grad_bits=gb, width=8, classes=10, image=32, weight_decay=WD,
                                ctx=ctx)
    om = oresnet.build_resnet50((1, 1, 1, 1), 8, 10, bits, gb, WD)
    blocks = [l for l in gm.layers if isinstance(l, L.ResidualBottleneck_q)]
    assert len(blocks) == 4 and not any(b._fusable() for b in blocks)
    assert all(l.fmode == (bits > 8) for l in gm._walk() if isinstance(l, QLAYERS))
    grange = {q.name: GRAD_I for q in ctx.quantizers if q.name.endswith("/grad_range")}
    ctx.set_ranges(grange)
    ranges = dict(oresnet.init_ranges(om), **grange)
    assert ctx.ranges() == ranges
    oresnet.set_params(om, {o.name + SUF[v]: getattr(o, v).cpu().numpy() for o, v, _ in gm.param_slots()})
    x, y = _batch(2, seed=bits)
    octx = onn.Ctx(ranges, 0, ctx.seed)
    logits = gm.forward(torch.from_numpy(x).to(DEV))
    assert np.array_equal(logits.cpu().numpy(), om.forward(x, octx)), "forward"
    gm.compute_loss(torch.from_numpy(y).to(DEV))
    dz = gm.dlogits.cpu().numpy()
    gm.backward()
    om.backward(dz, octx)
    og = oresnet.get_grads(om)
    params = oresnet.get_params(om)
    for o, v, gname in gm.param_slots():
        k = o.name + SUF[v]
        assert np.array_equal(getattr(o, gname).cpu().numpy(), og[k]), k
    ctx.update_range_op()
    new = octx.new_ranges()
    assert ctx.ranges() == new
    _step_not_vacuous(octx, og, params, sum(new[k] != ranges[k] for k in new), "bottleneck")

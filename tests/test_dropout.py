"""Dropout_q: the mask definition on the oracle's Philox stream, the layer's
host-side contract, and -- on the GPU -- lbt_dropout_fwd / _bwd against the numpy oracle,
lbt_dropout_quantize against the two launches it replaces, and the fused wiring against the plain one."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import plain_oracle as P
from lbt_amd import _lib
from lbt_amd import dynamic_fixed_point as D
from lbt_amd._lib import OUT_F32, OUT_I8, OUT_I16, OUT_U8OFF
from lbt_amd.dfxp import layers, ops
from lbt_amd.runtime import DfxpContext, qid_of
from oracle import nn as onn

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda"


# ------------------------------------------------------------------------------ CPU
def test_mask_known_answers():
    kat = json.load(open(os.path.join(HERE, "golden", "dropout_kat.json")))["cases"]
    assert [(c["name"], c["step"], c["keep"], c["n"], c["kept"]) for c in kat] == \
        [("dropout1", 0, 0.5, 256, 120), ("dropout1", 3, 0.8, 70, 59)]
    for c in kat:
        m = P.dropout_mask(c["n"], c["name"], c["step"], c["seed"], c["keep"])
        assert "".join("1" if b else "0" for b in m) == c["mask"], c["name"]
        assert int(m.sum()) == c["kept"]


@pytest.mark.parametrize("keep", [0.3, 0.5, 0.8])
def test_keep_rate(keep):
    """The kept fraction of 2^20 elements is within 5 standard deviations of keep."""
    n = 1 << 20
    bound = 5 * np.sqrt(keep * (1 - keep) / n)
    for name in ("dropout1", "dropout2", "dropout5"):
        for step in (0, 1, 7):
            frac = P.dropout_mask(n, name, step, 0, keep).mean()
            print(keep, name, step, frac)
            assert abs(frac - keep) <= bound, (name, step, frac)


def test_mask_at_indices_is_the_same_stream():
    idx = np.concatenate([np.arange(0, 70), np.arange(4093, 4101)])
    full = P.dropout_mask(4101, "dropout2", 7, 3, 0.8)
    assert np.array_equal(P.dropout_mask_at(idx, "dropout2", 7, 3, 0.8), full[idx])


def test_oracle_dropout_forward_backward_share_the_mask():
    d = P.DropoutQ("dropout1", 0.5)
    ctx = onn.Ctx({}, 0, 0)
    x = np.arange(1, 257, dtype=F32).reshape(4, 64)
    y = d.forward(x, ctx)
    assert int((y != 0).sum()) == 120 and np.array_equal(y[y != 0], (x * 2)[y != 0])
    g = d.backward(np.ones_like(x), ctx)
    assert np.array_equal(g != 0, y != 0) and set(np.unique(g)) == {0.0, 2.0}


def test_keep_prob_validation_names_and_identity():
    ctx = DfxpContext(device="cpu")
    for bad in (0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            D.Dropout_q(bad, True, ctx=ctx)
    assert ctx.dropouts == {}
    a, b = D.Dropout_q(0.5, True, ctx=ctx), D.Dropout_q(1, True, ctx=ctx)
    c = D.Dropout_q(0.25, False, name="mine", ctx=ctx)
    assert (a.name, b.name, c.name) == ("dropout1", "dropout2", "mine")
    assert a.did == qid_of("dropout1") and c.did == qid_of("mine")
    with pytest.raises(ValueError):
        D.Dropout_q(0.5, True, name="dropout1", ctx=ctx)
    assert a.info() == "dropout: 0.500000"
    # keep_prob == 1 and testing mode: the identity, nothing launched (these are CPU tensors)
    x, g = torch.randn(3, 5), torch.randn(3, 5)
    for layer in (b, c):
        assert not layer.active
        assert layer.forward(x) is x and layer.backward(g) is g
    assert a.active and not a.fused and not a.folds_relu


def test_plain_model_layout_and_wiring():
    from lbt_amd.models import MNIST_Model
    ctx = DfxpContext(device="cpu")
    m = MNIST_Model(8, dropout=0.8, ctx=ctx)
    kinds = [type(l).__name__ for l in m.layers]
    assert kinds == ["Conv2d_q", "ReLU_q", "MaxPool_q", "Conv2d_q", "ReLU_q", "MaxPool_q", "Conv2d_q", "ReLU_q",
                     "Flatten_q", "Dropout_q", "Dense_q", "ReLU_q", "Dropout_q", "Dense_q"]
    d1, d2 = m.layers[9], m.layers[12]
    assert (d1.name, d2.name, d1.keep_prob, m.dropout) == ("dropout1", "dropout2", 0.8, 0.8)
    assert d1.feeds is m.layers[10] and m.layers[10].drop_in is d1 and d1.relu is m.layers[7]
    assert d2.feeds is m.layers[13] and d2.relu is m.layers[11] and m.layers[11].act_in_drop is d2
    assert [l.input_nonnegative for l in m.layers if isinstance(l, D.Conv2d_q)] == [False, True, True]
    assert all(l.use_bias for l in m.layers if isinstance(l, (D.Conv2d_q, D.Dense_q)))
    assert d1.fused == layers.DROPOUT_FUSE and d1.folds_relu == layers.DROPOUT_FUSE
    m.set_testing()
    assert not d1.train and not d2.train and not d1.fused and not d1.folds_relu
    m.set_training()
    assert d1.train and d2.train
    assert "dropout: 0.800000" in m.info()
    om = P.mnist(8, 0.8)
    assert [n for n, _ in om.params()] == [o.name + {"W": "/W", "b": "/bias"}[v] for o, v, _ in m.param_slots()]
    assert sorted(om.range_names()) == sorted(q.name for q in ctx.quantizers)


def test_data_parallel_trainer_rejects_dropout(tmp_path):
    import torch.distributed as dist
    from lbt_amd.models import MNIST_Model
    from lbt_amd.trainer import Trainer
    own = not dist.is_initialized()
    if own:
        dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "pg"), rank=0, world_size=1)
    try:
        ctx = DfxpContext(device="cpu", world_size=dist.get_world_size())
        with pytest.raises(NotImplementedError, match="Dropout_q"):
            Trainer(MNIST_Model(8, ctx=ctx), exchange=True)
    finally:
        if own:
            dist.destroy_process_group()


def test_abi_and_host_side_argument_checks():
    """ABI 24 exports the three entry points; each rejects on the host, before any HIP call (no GPU
    here): more than 2^34 elements, a keep outside (0, 1], and the fp32 output kind."""
    lib = _lib.load()
    assert _lib.ABI_VERSION == 24 == lib.lbt_abi_version()
    for name in ("lbt_dropout_fwd", "lbt_dropout_bwd", "lbt_dropout_quantize"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    p = ctypes.c_void_p(0x1000)  # never dereferenced: rejected first
    big = (1 << 34) + 1
    assert lib.lbt_dropout_fwd(p, p, big, 0.5, p, 0, 1, 0, None) == 1001
    assert lib.lbt_dropout_bwd(p, p, big, 0.5, p, 0, 1, None, None) == 1001
    for keep in (0.0, -1.0, 1.5, float("nan")):
        assert lib.lbt_dropout_fwd(p, p, 16, keep, p, 0, 1, 0, None) == 1001
        assert lib.lbt_dropout_bwd(p, p, 16, keep, p, 0, 1, None, None) == 1001
    q = _lib.QDesc()
    q.bits = 8
    assert lib.lbt_dropout_quantize(p, p, OUT_F32, 4, 64, 0.5, 1, 0, q, None) == 1001
    assert lib.lbt_dropout_quantize(p, p, OUT_I8, 1 << 20, (1 << 14) + 1, 0.5, 1, 0, q, None) == 1001
    assert lib.lbt_dropout_quantize(p, p, OUT_I8, 4, 64, 0.0, 1, 0, q, None) == 1001
    q.bits = 9
    assert lib.lbt_dropout_quantize(p, p, OUT_I8, 4, 64, 0.5, 1, 0, q, None) == 1001  # 9-bit codes in int8
    # nothing to do: success without a launch
    assert lib.lbt_dropout_fwd(p, p, 0, 0.5, p, 0, 1, 0, None) == 0
    assert lib.lbt_dropout_quantize(p, p, OUT_I16, 0, 64, 0.5, 1, 0, q, None) == 0


# ------------------------------------------------------------------------------ GPU
SHAPES = [(3, 5, 7, 6), (8, 4, 4, 16), (64, 1024), (1, 3)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_dropout_fwd_bwd_equal_oracle(shape):
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal(shape).astype(F32)
    g = (rng.standard_normal(shape) * 0.01).astype(F32)
    xr = np.maximum(x, F32(0))
    seed = 11
    ctx = DfxpContext(seed=seed)
    xt, gt = _dev(x), _dev(g)
    y, dx = torch.empty_like(xt), torch.empty_like(xt)
    for step in (0, 5):
        ctx.step.fill_(step)
        octx = onn.Ctx({}, step, seed)
        for keep in (0.5, 0.8):
            o = P.DropoutQ("dropout3", keep)
            for relu in (0, 1):
                want = o.forward(xr if relu else x, octx)
                ops.dropout_fwd(xt, y, keep, ctx, qid_of("dropout3"), relu=bool(relu))
                assert np.array_equal(y.cpu().numpy(), want), (step, keep, relu)
                want_dx = o.backward(g, octx)
                if relu:
                    want_dx = np.where(x > 0, want_dx, F32(0)).astype(F32)
                ops.dropout_bwd(gt, dx, keep, ctx, qid_of("dropout3"), relu_x=xt if relu else None)
                assert np.array_equal(dx.cpu().numpy(), want_dx), (step, keep, relu)
    assert int(ctx.step.item()) == 5  # the kernels only read the step


@pytest.mark.gpu
@pytest.mark.parametrize("table", [False, True], ids=["philox", "noise_table"])
@pytest.mark.parametrize("kind,bits,relu", [(OUT_I8, 8, 0), (OUT_U8OFF, 9, 1), (OUT_I16, 9, 0)],
                         ids=["i8", "u8off_relu", "i16"])
@pytest.mark.parametrize("shape", SHAPES[:3])
def test_dropout_quantize_equals_the_two_launches(shape, kind, bits, relu, table):
    """Codes bit-equal and every counter shard equal; rows >= 3, so the quantiser's noise index wraps
    where the dropout's does not; |x| reaches past 2^I = 4, so both overflow counters are non-zero."""
    rng = np.random.default_rng(sum(shape) + bits)
    x = _dev((rng.standard_normal(shape) * 2.5).astype(F32))
    ctx = DfxpContext(seed=7)
    q = ctx.quantizer("t/X_range", bits, 2)
    ctx.step.fill_(3)
    did, keep = qid_of("dropout2"), 0.5
    y = ops.dropout_fwd(x, torch.empty_like(x), keep, ctx, did, relu=bool(relu))
    ref = ops.quantize(y, q, kind).cpu().numpy()
    ref_counts = ctx.counts_view().cpu().numpy().copy()
    assert ref_counts[0, :, 0].sum() > 0 and ref_counts[0, :, 1].sum() > ref_counts[0, :, 0].sum()
    if shape == (64, 1024):
        assert (ref_counts[0, :, 1] > 0).all()  # 64 workgroups: every shard in use
    ctx.counts.zero_()
    desc = ctx.noise_table_desc(q, ops.rows_inner(shape)[1]) if table else None
    got = ops.dropout_quantize(x, keep, did, q, kind, relu=bool(relu), desc=desc)
    assert got.dtype == ops.out_dtype(kind)
    assert np.array_equal(got.cpu().numpy(), ref)
    assert np.array_equal(ctx.counts_view().cpu().numpy(), ref_counts)


@pytest.mark.gpu
def test_element_indices_past_2_31():
    """64-bit element indices and Philox block counters past 2^29: rows 0 and 2^15 of a [2^15 + 1, 2^16]
    tensor of ones (8.6 GB) through lbt_dropout_quantize (keep 0.5, nearest rounding at 2^-5: the
    code is 64 * mask) and through lbt_dropout_fwd (2 * mask)."""
    rows, inner = (1 << 15) + 1, 1 << 16
    ctx = DfxpContext(seed=5)
    q = ctx.quantizer("big/X_range", 8, 2, stochastic=False)
    ctx.step.fill_(1)
    x = torch.ones((rows, inner), dtype=torch.float32, device=DEV)
    want = {r: P.dropout_mask_at(np.arange(inner, dtype=np.uint64) + np.uint64(r * inner), "dropout1", 1, 5, 0.5)
            for r in (0, rows - 1)}
    out = ops.dropout_quantize(x, 0.5, qid_of("dropout1"), q, OUT_I8)
    for r, m in want.items():
        assert np.array_equal(out[r].cpu().numpy(), m.astype(np.int8) * 64), r
    del out
    y = ops.dropout_fwd(x, torch.empty_like(x), 0.5, ctx, qid_of("dropout1"))
    for r, m in want.items():
        assert np.array_equal(y[r].cpu().numpy(), m.astype(F32) * 2), r
    del x, y
    torch.cuda.empty_cache()  # 17 GB back to the device: other processes share it


def _conv_case(cin, cout, relu=False):
    """relu: ReLU_q -> Dropout_q -> a conv on unsigned codes (input_nonnegative), as the models have it."""
    def build(ctx):
        drop = D.Dropout_q(0.5, True, ctx=ctx)
        conv = D.Conv2d_q("c", 8, [3, 3, cin, cout], [1, 1, 1, 1], "SAME", weight_decay=1e-3,
                          input_nonnegative=relu, ctx=ctx)
        drop.feeds = conv
        if relu:
            drop.relu = D.ReLU_q()
        return ([drop.relu] if relu else []) + [drop, conv], conv

    def oracle():
        conv = onn.Conv2dQ("c", 8, [3, 3, cin, cout], [1, 1, 1, 1], "SAME", 1e-3, use_bias=True)
        return onn.SequentialQ(*([onn.ReluQ()] if relu else []), P.DropoutQ("dropout1", 0.5), conv), conv
    return build, oracle, (3, 6, 6, cin), (3, 6, 6, cout)


def _dense_case():
    def build(ctx):
        relu, drop = D.ReLU_q(), D.Dropout_q(0.5, True, ctx=ctx)
        dense = D.Dense_q("d", 8, 96, 40, weight_decay=1e-3, ctx=ctx)
        drop.feeds, drop.relu = dense, relu
        return [relu, drop, dense], dense

    def oracle():
        dense = onn.DenseQ("d", 8, 96, 40, 1e-3, use_bias=True)
        return onn.SequentialQ(onn.ReluQ(), P.DropoutQ("dropout1", 0.5), dense), dense
    return build, oracle, (5, 96), (5, 40)


LAYER_CASES = {"conv16x32": _conv_case(16, 32), "conv64x256_igemm": _conv_case(64, 256),
               "relu_conv64x256_u8off": _conv_case(64, 256, relu=True), "relu_dense96x40": _dense_case()}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(LAYER_CASES))
def test_fused_wiring_equals_plain_equals_oracle(case, monkeypatch):
    build, oracle, xs, gs = LAYER_CASES[case]
    rng = np.random.default_rng(len(case))
    x = rng.standard_normal(xs).astype(F32)
    g = (rng.standard_normal(gs) * 0.5).astype(F32)
    bias = (rng.standard_normal(gs[-1]) * 0.1).astype(F32)
    res = {}
    for fuse in (False, True):
        monkeypatch.setattr(layers, "DROPOUT_FUSE", fuse)
        ctx = DfxpContext(seed=9)
        ctx.step.fill_(2)
        ls, last = build(ctx)
        last.b.copy_(_dev(bias))
        h = _dev(x)
        for l in ls:
            h = l.forward(h)
        drop = [l for l in ls if isinstance(l, D.Dropout_q)][0]
        assert drop.fused == fuse and (drop.y is drop.X) == fuse  # fused: the input goes through untouched
        d = _dev(g)
        for l in reversed(ls):
            d = l.backward(d)
        res[fuse] = dict(y=h.cpu().numpy().copy(), dW=last.dW.cpu().numpy().copy(), db=last.db.cpu().numpy().copy(),
                         dx=d.cpu().numpy().copy(), W=last.W.cpu().numpy().copy())
        ctx.update_range_op()
        res[fuse]["ranges"] = ctx.ranges()
    om, olast = oracle()
    olast.W, olast.b = res[True]["W"], bias
    octx = onn.Ctx({r: 2 for r in om.range_names()}, 2, 9)
    want = dict(y=om.forward(x, octx))
    want["dx"] = om.backward(g, octx)
    want["dW"], want["db"] = olast.dW, olast.db
    for k in ("y", "dW", "db", "dx"):
        assert np.array_equal(res[False][k], res[True][k]), k
        assert np.array_equal(res[True][k], want[k]), k
    assert res[False]["ranges"] == res[True]["ranges"] == octx.new_ranges()

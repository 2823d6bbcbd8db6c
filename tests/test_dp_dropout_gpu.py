"""Data-parallel training of the Dropout_q models on the GPU.

Kernels: lbt_dropout_fwd_at / _bwd_at / _quantize_at against the numpy mask at global indices
(plain_oracle.dropout_mask_at), against the single launch over the concatenated tensor, and at base 0
against the entry points they generalise.

Models: N spawned ranks share cuda:0 over gloo (the one-GPU rehearsal of the RCCL path, as
tests/test_dp_resnet50_gpu.py), each with DfxpContext(world_size=N, rank=r) on its shard of a global
batch of 8. Two captured steps equal the numpy data-parallel oracle (tests/plain_dp_oracle.py, the ranks'
d loss / d logits injected) and a single-process Trainer step on the whole batch, bit for bit.
"""
import os
import queue
import socket
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
F32 = np.float32
DEV = "cuda"
SEED, STEP, KEEP = 7, 3, 0.5
NAME = "dropout2"


# ------------------------------------------------------------------------------ kernels
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ctx():
    from lbt_amd.runtime import DfxpContext
    ctx = DfxpContext(seed=SEED)
    ctx.step.fill_(STEP)
    return ctx


def _mask(base, n):
    import plain_oracle as P
    idx = np.uint64(base) + np.arange(n, dtype=np.uint64)
    return P.dropout_mask_at(idx, NAME, STEP, SEED, KEEP).astype(F32)


def _fwd_at(ctx, x, base, relu):
    from lbt_amd import _lib
    from lbt_amd.runtime import qid_of
    y = torch.empty_like(x)
    _lib.call("lbt_dropout_fwd_at", _lib.ptr(x), _lib.ptr(y), x.numel(), int(base), KEEP, _lib.ptr(ctx.step),
              ctx.seed, qid_of(NAME), int(relu), _lib.stream())
    return y


def _bwd_at(ctx, g, base, relu_x):
    from lbt_amd import _lib
    from lbt_amd.runtime import qid_of
    dx = torch.empty_like(g)
    _lib.call("lbt_dropout_bwd_at", _lib.ptr(g), _lib.ptr(dx), g.numel(), int(base), KEEP, _lib.ptr(ctx.step),
              ctx.seed, qid_of(NAME), _lib.ptr(relu_x), _lib.stream())
    return dx


# (rows, inner, bases): n = 15 at ranks 0..3 (base % 4 = 0, 3, 2, 1); n = 16 and 1030 at multiples of 4
# (the four-per-thread kernel without and with a tail; 1030 elements are 258 threads, two workgroups);
# 2^32 - 8: the indices of a 16-element window straddle 2^32
WINDOWS = [(3, 5, [0, 15, 30, 45]), (4, 4, [0, 16, 32]), (2, 515, [0, 1032, 4120]), (4, 4, [(1 << 32) - 8])]


@pytest.mark.parametrize("relu", [0, 1], ids=["plain", "relu"])
@pytest.mark.parametrize("rows,inner,bases", WINDOWS, ids=["n15", "n16", "n1030", "straddle_2_32"])
def test_fwd_bwd_at_equal_oracle_and_the_concatenated_launch(rows, inner, bases, relu):
    from lbt_amd.dfxp import ops
    from lbt_amd.runtime import qid_of
    n = rows * inner
    ctx = _ctx()
    rng = np.random.default_rng(n + relu)
    shards = len(bases)
    x = rng.standard_normal((shards, n)).astype(F32)
    g = (rng.standard_normal((shards, n)) * 0.01).astype(F32)
    xin = np.maximum(x, F32(0)) if relu else x
    ys, dxs = [], []
    for r, base in enumerate(bases):
        m = _mask(base, n)
        assert 0 < m.sum() < n
        xt, gt = _dev(x[r]), _dev(g[r])
        y = _fwd_at(ctx, xt, base, relu).cpu().numpy()
        assert np.array_equal(y, ((xin[r] / F32(KEEP)).astype(F32) * m).astype(F32)), base
        dx = _bwd_at(ctx, gt, base, xt if relu else None).cpu().numpy()
        want = ((g[r] / F32(KEEP)).astype(F32) * m).astype(F32)
        if relu:
            want = np.where(x[r] > 0, want, F32(0)).astype(F32)
        assert np.array_equal(dx, want), base
        ys.append(y)
        dxs.append(dx)
    if bases == [r * n for r in range(shards)]:  # equal shards of one tensor: the single launch over it
        xt, gt = _dev(x.reshape(-1)), _dev(g.reshape(-1))
        y = ops.dropout_fwd(xt, torch.empty_like(xt), KEEP, ctx, qid_of(NAME), relu=bool(relu))
        dx = ops.dropout_bwd(gt, torch.empty_like(gt), KEEP, ctx, qid_of(NAME), relu_x=xt if relu else None)
        assert np.array_equal(y.cpu().numpy(), np.concatenate(ys))
        assert np.array_equal(dx.cpu().numpy(), np.concatenate(dxs))
        assert not np.array_equal(ys[0] != 0, ys[1] != 0) or relu  # the shards' masks differ
    assert int(ctx.step.item()) == STEP


def _quantize_at(x, base, q, kind, relu):
    from lbt_amd import _lib
    from lbt_amd.dfxp import ops
    from lbt_amd.runtime import qid_of
    rows, inner = ops.rows_inner(tuple(x.shape))
    out = torch.empty(x.shape, dtype=ops.out_dtype(kind), device=x.device)
    q.observe(x.numel())
    _lib.call("lbt_dropout_quantize_at", _lib.ptr(x), _lib.ptr(out), kind, rows, inner, int(base), KEEP,
              qid_of(NAME), int(relu), q.desc, _lib.stream())
    return out


# inner 64: the vector threshold; 784: PI_MNIST's rows; 20: the generic kernel; (3, 64) at base 3*64 + 1..3:
# a base that is no multiple of 4 falls to the per-element kernel
QSHAPES = [((3, 64), [0, 192, 1 << 32]), ((2, 784), [0, 1568]), ((3, 20), [0, 60, 30]), ((3, 64), [193, 194, 195])]


@pytest.mark.parametrize("kind,bits,relu", [("I8", 8, 0), ("U8OFF", 9, 1), ("I16", 9, 0)],
                         ids=["i8", "u8off_relu", "i16"])
@pytest.mark.parametrize("shape,bases", QSHAPES, ids=["3x64", "2x784", "3x20_generic", "3x64_unaligned"])
def test_quantize_at_equals_fwd_at_then_quantize(shape, bases, kind, bits, relu):
    from lbt_amd import _lib
    from lbt_amd.dfxp import ops
    kind = getattr(_lib, "OUT_" + kind)
    rng = np.random.default_rng(sum(shape) + bits)
    x = _dev((rng.standard_normal(shape) * 2.5).astype(F32))  # |x| past 2^I = 4: both counters move
    ctx = _ctx()
    q = ctx.quantizer("t/X_range", bits, 2)
    for base in bases:
        ctx.counts.zero_()
        y = _fwd_at(ctx, x, base, relu)
        ref = ops.quantize(y, q, kind).cpu().numpy()
        ref_tot = ctx.counts_view().cpu().numpy().sum(axis=1)
        assert ref_tot[0, 1] > ref_tot[0, 0] > 0
        ctx.counts.zero_()
        got = _quantize_at(x, base, q, kind, relu)
        assert got.dtype == ops.out_dtype(kind)
        assert np.array_equal(got.cpu().numpy(), ref), base
        assert np.array_equal(ctx.counts_view().cpu().numpy().sum(axis=1), ref_tot), base


@pytest.mark.parametrize("shape", [(3, 5), (4, 4), (2, 515), (3, 64), (2, 784), (3, 20)])
def test_existing_entry_points_are_base_zero(shape):
    """Outputs bit-equal, and for lbt_dropout_quantize every counter shard."""
    from lbt_amd import _lib
    from lbt_amd.dfxp import ops
    from lbt_amd.runtime import qid_of
    rng = np.random.default_rng(sum(shape))
    x = _dev((rng.standard_normal(shape) * 2.5).astype(F32))
    g = _dev(rng.standard_normal(shape).astype(F32))
    ctx = _ctx()
    did = qid_of(NAME)
    for relu in (0, 1):
        y = ops.dropout_fwd(x, torch.empty_like(x), KEEP, ctx, did, relu=bool(relu))
        assert torch.equal(y, _fwd_at(ctx, x, 0, relu))
        dx = ops.dropout_bwd(g, torch.empty_like(g), KEEP, ctx, did, relu_x=x if relu else None)
        assert torch.equal(dx, _bwd_at(ctx, g, 0, x if relu else None))
    for i, (kind, bits) in enumerate(((_lib.OUT_I8, 8), (_lib.OUT_U8OFF, 9), (_lib.OUT_I16, 9))):
        q = ctx.quantizer("t%d/X_range" % i, bits, 2)
        ctx.counts.zero_()
        ref = ops.dropout_quantize(x, KEEP, did, q, kind)
        ref_counts = ctx.counts_view().cpu().numpy().copy()
        assert ref_counts[q.slot].sum() > 0
        ctx.counts.zero_()
        assert torch.equal(ref, _quantize_at(x, 0, q, kind, 0))
        assert np.array_equal(ctx.counts_view().cpu().numpy(), ref_counts)


def test_ops_route_by_the_contexts_switch():
    """ops.dropout_* on a context that declares rank 1 of 2: the shard's window inside shard_masks, the
    plain stream outside it (what Trainer.evaluate draws)."""
    from lbt_amd import _lib
    from lbt_amd.dfxp import ops
    from lbt_amd.runtime import DfxpContext, qid_of
    ctx = DfxpContext(seed=SEED, world_size=2, rank=1)
    ctx.step.fill_(STEP)
    x = _dev(np.arange(1, 3 * 64 + 1, dtype=F32).reshape(3, 64) / 64)
    did, n = qid_of(NAME), x.numel()
    q = ctx.quantizer("t/X_range", 8, 2, stochastic=False)
    plain = ops.dropout_fwd(x, torch.empty_like(x), KEEP, ctx, did).cpu().numpy()
    assert np.array_equal(plain != 0, _mask(0, n).reshape(3, 64) != 0)
    with ctx.shard_masks():
        y = ops.dropout_fwd(x, torch.empty_like(x), KEEP, ctx, did).cpu().numpy()
        dx = ops.dropout_bwd(x, torch.empty_like(x), KEEP, ctx, did).cpu().numpy()
        codes = ops.dropout_quantize(x, KEEP, did, q, _lib.OUT_I8).cpu().numpy()
    m = _mask(n, n).reshape(3, 64) != 0
    assert np.array_equal(y != 0, m) and np.array_equal(dx != 0, m) and np.array_equal(codes != 0, m)
    assert not np.array_equal(m, plain != 0)


# ------------------------------------------------------------------------------ models
STEPS, B = 2, 8
GRAD_I = -6  # initial */grad_range: the default 2 quantises these narrow gradients to zero
SUFFIX = {"W": "/W", "b": "/bias"}
CASES = {"mnist": ("MNIST_Model", "mnist", (28, 28, 1), {}),
         "pi_mnist": ("PI_MNIST_Model", "pi_mnist", (784,), {}),
         "vgg_w16": ("CIFAR10_VGG_Model", "cifar10_vgg", (32, 32, 3), dict(width=16, dense_units=64))}


def _lib_i16():
    from lbt_amd import _lib
    return _lib.OUT_I16


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _batches(shape):
    rng = np.random.default_rng(5)
    xs = [((rng.integers(0, 256, size=(B,) + shape) - 127.5) / 128).astype(F32) for _ in range(STEPS)]
    ys = [rng.integers(0, 10, size=B).astype(np.int32) for _ in range(STEPS)]
    return xs, ys


def _make(case, world, rank):
    from lbt_amd import models
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    gname, _, _, kw = CASES[case]
    ctx = DfxpContext(device="cuda:0", seed=1, world_size=world, rank=rank)
    gm = getattr(models, gname)(8, dropout=KEEP, weight_decay=1e-4, ctx=ctx, **kw)
    ctx.set_ranges({q.name: GRAD_I for q in ctx.quantizers if q.name.endswith("/grad_range")})
    return ctx, gm, Trainer(gm, lr=1e-2, momentum=0.9, batch_size=B // world, use_graph=True)


def _run_steps(ctx, gm, tr, xs, ys):
    rec = []
    for x, y in zip(xs, ys):
        tr.step(torch.from_numpy(x.copy()).cuda(), torch.from_numpy(y.copy()).cuda())
        torch.cuda.synchronize()
        assert tr._graphs is not None
        rec.append(dict(loss=float(gm.loss.item()), dz=gm.dlogits.cpu().numpy().copy(),
                        w=tr.flat.w.cpu().numpy().copy(), g=tr.flat.g.cpu().numpy().copy(),
                        a=tr.flat.a.cpu().numpy().copy(), ranges=ctx.ranges()))
    return rec


def _worker(rank, world, port, case, fuse, out_q):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if not fuse:
        os.environ["LBT_DROPOUT_FUSE"] = "0"  # read when lbt_amd.dfxp.layers is first imported (below)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from lbt_amd.dfxp import layers
        assert layers.DROPOUT_FUSE == fuse
        ctx, gm, tr = _make(case, world, rank)
        assert tr.dp and tr._lw_exact and tr.comm is None, "the exact layer-wise exchange must be the one in use"
        assert all(d.fused == fuse for d in ctx.dropouts.values())
        xs, ys = _batches(CASES[case][2])
        b = B // world
        rec = _run_steps(ctx, gm, tr, [x[rank * b:(rank + 1) * b] for x in xs], [y[rank * b:(rank + 1) * b] for y in ys])
        out_q.put((rank, rec))
    except Exception as e:  # pragma: no cover - surfaced by the parent
        out_q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def _run(case, world, fuse=True):
    """The ranks' records. Never retried; a rank that exits without reporting fails the test at once."""
    mctx = mp.get_context("spawn")
    q = mctx.Queue()
    port = _free_port()
    procs = [mctx.Process(target=_worker, args=(r, world, port, case, fuse, q)) for r in range(world)]
    for p in procs:
        p.start()
    res, deadline = [], time.monotonic() + 300
    try:
        while len(res) < world:
            try:
                res.append(q.get(timeout=2))
            except queue.Empty:
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                assert not dead, "a rank exited with %r before reporting" % dead
                assert time.monotonic() < deadline, "the ranks did not report within 300 s"
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0, p.exitcode
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    res.sort(key=lambda t: t[0])
    for _, rec in res:
        assert not isinstance(rec, str), rec
    return [rec for _, rec in res]


def _by_name(tr, flat):
    return {o.name + SUFFIX[v]: flat[off:off + sz].reshape(tuple(getattr(o, v).shape)) for o, v, off, sz in tr.flat.offsets}


def _check(case, world, fuse=True):
    import plain_dp_oracle as DP
    import plain_oracle as P
    ranks = _run(case, world, fuse)
    for r in ranks[1:]:  # one model on every rank
        for s0, s in zip(ranks[0], r):
            assert np.array_equal(s0["w"], s["w"]) and np.array_equal(s0["g"], s["g"]) and s0["ranges"] == s["ranges"]
    # the single process on the whole batch (same seed: the same initial parameters and flat layout)
    ctx1, gm1, tr1 = _make(case, 1, None)
    assert not tr1.dp
    w0 = tr1.flat.w.cpu().numpy().copy()
    xs, ys = _batches(CASES[case][2])
    one = _run_steps(ctx1, gm1, tr1, xs, ys)
    om = DP.shardable(getattr(P, CASES[case][1])(8, KEEP, 1e-4, **CASES[case][3]))
    params = _by_name(tr1, w0)
    assert list(params) == [n for n, _ in om.params()]
    ranges = {r: (GRAD_I if r.endswith("/grad_range") else 2) for r in om.range_names()}
    state = dict(params=params, accum={k: np.zeros_like(v) for k, v in params.items()}, ranges=ranges, step=0)
    b = B // world
    for i in range(STEPS):
        shards = [(xs[i][r * b:(r + 1) * b], ys[i][r * b:(r + 1) * b]) for r in range(world)]
        dzs = [ranks[r][i]["dz"] for r in range(world)]
        loss, state, octxs = DP.dp_train_step(om, state, shards, lr=1e-2, momentum=0.9, seed=1, dzs=dzs)
        for r, c in enumerate(octxs):  # each rank's rows of the GLOBAL-batch softmax gradient
            np.testing.assert_allclose(dzs[r], c.dz, rtol=1e-5, atol=1e-9)
        got = ranks[0][i]
        print(case, world, i, "loss", got["loss"], loss, one[i]["loss"])
        assert abs(got["loss"] - loss) <= 1e-5 * abs(loss), (i, got["loss"], loss)
        assert abs(got["loss"] - one[i]["loss"]) <= 1e-5 * abs(one[i]["loss"]), (i, got["loss"], one[i]["loss"])
        gw, ga = _by_name(tr1, got["w"]), _by_name(tr1, got["a"])
        for k in state["params"]:
            assert np.array_equal(gw[k], state["params"][k]), (i, "param", k)
            assert np.array_equal(ga[k], state["accum"][k]), (i, "momentum", k)
        assert got["ranges"] == state["ranges"], i
        # ... and bit-equal to the one-process step on the GPU, in weights, momentum and exponents
        assert np.array_equal(got["w"], one[i]["w"]) and np.array_equal(got["a"], one[i]["a"]), i
        assert got["ranges"] == one[i]["ranges"], i
        assert not np.array_equal(got["w"], w0 if i == 0 else ranks[0][i - 1]["w"])
        for name in octxs[0].masks:
            assert not np.array_equal(octxs[0].masks[name], octxs[1].masks[name]), name
            share = 1 - np.concatenate([c.masks[name].ravel() for c in octxs]).mean()
            assert 0.3 < share < 0.7, (name, share)
        assert len(octxs[0].masks) == len(DP.dropouts(om)) >= 2
        nz = [np.count_nonzero(c.record[n]) for c in octxs for n in c.record if n.endswith("/grad_range")]
        assert min(nz) > 0, "a gradient quantised to all zeros: the step would not see the masks"


@pytest.mark.parametrize("case,world", [("mnist", 2), ("mnist", 4), ("pi_mnist", 2), ("vgg_w16", 2)])
def test_ranks_equal_the_oracle_and_one_process_on_the_whole_batch(case, world):
    if case == "vgg_w16":  # what this case is for: the MFMA and stem convs, the MFMA dense
        from lbt_amd import models
        from lbt_amd.runtime import DfxpContext
        gm = models.CIFAR10_VGG_Model(8, ctx=DfxpContext(device="cpu"), width=16, dense_units=64)
        convs = [l for l in gm.layers if hasattr(l, "x_mfma")]
        assert any(l.x_mfma for l in convs) and not convs[0].x_mfma and convs[0].x_kind == _lib_i16()
        assert any(l.mfma for l in gm.layers if hasattr(l, "in_units"))
    _check(case, world)


def test_mnist_two_ranks_on_the_unfused_kernels(monkeypatch):
    from lbt_amd.dfxp import layers
    monkeypatch.setattr(layers, "DROPOUT_FUSE", False)
    _check("mnist", 2, fuse=False)

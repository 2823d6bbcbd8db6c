"""SyncBN for the layer-wise models (lbt_amd.distributed.sync_batchnorm): the switch, the lbt_sums_fold
kernel, and -- on a world of ONE rank, where every collective is the identity -- that the synchronised path
(fold -> all-reduce -> the unchanged consumers on the layer's own buffer and n * world) leaves what the plain
step leaves, bit for bit, eagerly over gloo and captured into one HIP graph over nccl (= RCCL).
Two ranks against one process: tests/test_syncbn_layerwise_dp_gpu.py.
"""
import ctypes
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, STEPS = 8, 3
# (blocks, width, image, classes, grad_bits) of ImageNet_Resnet -- the 8-bit chains, the wide (16-bit
# gradient) backward, and at width 64 the fused bottleneck schedule -- and the layer-wise CIFAR ResNet
CONFIGS = {"r50-g8": ((1, 1, 1, 1), 8, 32, 10, 8), "r50-g16": ((1, 1, 1, 1), 8, 32, 16, 16),
           "r50-w64-g16": ((1, 1, 1, 1), 64, 32, 16, 16), "cifar": "cifar"}


def make_model(cfg, ctx):
    """A reduced ImageNet_Resnet, or the layer-wise CIFAR ResNet with one block per stage."""
    from lbt_amd import dynamic_fixed_point as L
    from lbt_amd.models import CIFAR10_Resnet, ImageNet_Resnet
    if cfg == "cifar":
        return CIFAR10_Resnet(8, [1, 1, 1], L.ResidualBlock_q, weight_decay=1e-4, ctx=ctx)
    blocks, width, image, classes, grad_bits = cfg
    return ImageNet_Resnet(8, blocks, grad_bits=grad_bits, width=width, classes=classes, image=image,
                           weight_decay=1e-4, ctx=ctx)


def shape_of(cfg):
    return (32, 10) if cfg == "cifar" else (cfg[2], cfg[3])


def batches(cfg, steps=STEPS):
    """The global batches of tests/test_dp_resnet50_gpu.py: default_rng(5), B = 8."""
    image, classes = shape_of(cfg)
    rng = np.random.default_rng(5)
    xs = [((rng.integers(0, 256, size=(B, image, image, 3)) - 127.5) / 128).astype(np.float32) for _ in range(steps)]
    ys = [rng.integers(0, classes, size=B).astype(np.int32) for _ in range(steps)]
    return xs, ys


def norms(model):
    from lbt_amd.dfxp.layers import Normalization_q
    return [l for l in model._walk() if isinstance(l, Normalization_q)]


def snap(tr):
    """Everything a step leaves: parameters, momentum, gradients, exponents, step, BN statistics, loss."""
    m, ctx = tr.model, tr.ctx
    torch.cuda.synchronize()
    return dict(w=tr.flat.w.cpu().numpy().copy(), a=tr.flat.a.cpu().numpy().copy(), g=tr.flat.g.cpu().numpy().copy(),
                exps=ctx.exps.cpu().numpy().copy(), step=ctx.step.cpu().numpy().copy(),
                mean=[n.X_mean_running.cpu().numpy().copy() for n in norms(m)],
                var=[n.X_var_running.cpu().numpy().copy() for n in norms(m)],
                loss=m.loss.detach().cpu().numpy().copy())


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ------------------------------------------------------------------------------------------ CPU
def _cpu_model(cfg=((1, 1, 1, 1), 8, 32, 10, 8)):
    from lbt_amd.runtime import DfxpContext
    return make_model(cfg, DfxpContext(device="cpu"))


@pytest.mark.parametrize("cfg", [((1, 1, 1, 1), 8, 32, 10, 8), "cifar"], ids=["imagenet", "cifar"])
def test_sync_batchnorm_marks_every_normalization(cfg):
    from lbt_amd.distributed import sync_batchnorm
    m = _cpu_model(cfg)
    ns = norms(m)
    assert len(ns) == (17 if cfg != "cifar" else 9)
    assert m.sync_bn is False and all(n.sync is None for n in ns)
    assert sync_batchnorm(m, force=True) is m
    assert m.sync_bn is True
    assert all(n.sync == (None, 1) and n.synced for n in ns)
    # testing mode has no batch statistics: nothing is synchronised
    m.set_testing()
    assert not any(n.synced for n in ns)
    m.set_training()
    # the suspension clears and restores, also when its body raises
    with pytest.raises(ZeroDivisionError):
        with m.sync_suspended():
            assert m.sync_bn is False and all(n.sync is None for n in ns)
            1 / 0
    assert m.sync_bn is True and all(n.sync == (None, 1) for n in ns)


def test_world_one_without_force_changes_nothing():
    from lbt_amd.distributed import sync_batchnorm
    m = _cpu_model()
    before = {k: v for k, v in vars(m).items()}
    assert sync_batchnorm(m) is m
    assert m.sync_bn is False and all(n.sync is None and not n.synced for n in norms(m))
    assert vars(m) == before and "sync" not in vars(norms(m)[0])


def test_refusals():
    from lbt_amd.distributed import sync_batchnorm
    from lbt_amd.fused import FusedResNet
    from lbt_amd.models import CIFAR10_Resnet20
    from lbt_amd.runtime import DfxpContext
    fused = FusedResNet(CIFAR10_Resnet20(8, ctx=DfxpContext(device="cpu")))
    with pytest.raises(TypeError, match="sync_bn"):
        sync_batchnorm(fused, force=True)
    # a float-mode Normalization_q (bits > 8): fp32 partial sums, not integers -- named in the message
    from lbt_amd.models import ImageNet_Resnet
    fm = ImageNet_Resnet(12, (1, 1, 1, 1), width=8, classes=10, image=32, ctx=DfxpContext(device="cpu"))
    with pytest.raises(NotImplementedError, match="conv1-bn-norm"):
        sync_batchnorm(fm, force=True)
    assert all(n.sync is None for n in norms(fm)) and fm.sync_bn is False
    # world > 1 without an initialised process group
    m2 = make_model(((1, 1, 1, 1), 8, 32, 10, 8), DfxpContext(device="cpu", world_size=2))
    with pytest.raises(RuntimeError, match="process group"):
        sync_batchnorm(m2)
    assert all(n.sync is None for n in norms(m2))
    # a model that already ran a forward
    m3 = _cpu_model()
    m3.logits = torch.zeros(2, 10)
    with pytest.raises(RuntimeError, match="forward"):
        sync_batchnorm(m3, force=True)
    assert all(n.sync is None for n in norms(m3))


@pytest.fixture
def one_rank_group(tmp_path):
    import torch.distributed as dist
    own = not dist.is_initialized()
    if own:
        dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "pg"), rank=0, world_size=1)
    yield
    if own:
        dist.destroy_process_group()


def test_trainer_takes_syncbn_on_the_exact_exchange_only(one_rank_group, monkeypatch):
    """A data-parallel trainer of a layer-wise SyncBN model: the exact int64 exchange, or
    NotImplementedError before anything is allocated for the fp32 one (here: LBT_EXACT_LAYERWISE=0)."""
    from lbt_amd.distributed import sync_batchnorm
    from lbt_amd.trainer import Trainer
    tr = Trainer(sync_batchnorm(_cpu_model(), force=True), exchange=True)
    assert tr.dp and tr._lw_exact and tr.comm is None and tr.model.sync_bn
    assert all(n.sync == (None, 1) for n in norms(tr.model))
    monkeypatch.setenv("LBT_EXACT_LAYERWISE", "0")
    with pytest.raises(NotImplementedError, match="exact"):
        Trainer(sync_batchnorm(_cpu_model(), force=True), exchange=True)
    Trainer(_cpu_model(), exchange=True)  # without SyncBN the fp32 exchange stays available
    Trainer(sync_batchnorm(_cpu_model(), force=True), exchange=False)  # and no exchange: nothing to refuse


def test_sums_fold_is_declared_bound_and_checks_its_arguments():
    from lbt_amd import _lib
    header = open(os.path.join(ROOT, "include", "lbt_dfxp.h")).read()
    assert re.search(r"^int\s+lbt_sums_fold\s*\(const int64_t\* part, int32_t nshard, int64_t stride, int64_t\* total,"
                     r" void\* stream\);", header, flags=re.M)
    assert "lbt_sums_fold" in _lib.EXPORTED
    lib = _lib.load()
    p, t = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)  # never dereferenced: rejected on the host
    assert lib.lbt_sums_fold(None, 32, 8, t, None) == 1001
    assert lib.lbt_sums_fold(p, 32, 8, None, None) == 1001
    assert lib.lbt_sums_fold(p, 0, 8, t, None) == 1001
    assert lib.lbt_sums_fold(p, -1, 8, t, None) == 1001
    assert lib.lbt_sums_fold(p, _lib.NSHARD + 1, 8, t, None) == 1001
    assert lib.lbt_sums_fold(p, 32, 0, t, None) == 1001
    assert lib.lbt_sums_fold(p, 32, -4, t, None) == 1001


# ------------------------------------------------------------------------------------------ GPU: the kernel
@pytest.mark.gpu
@pytest.mark.parametrize("stride", [2, 6, 130, 4096, 8192])
def test_sums_fold_kernel(stride):
    """total[:stride] is numpy's exact sum over the 32 shards; nothing else of total and nothing of part is
    written. Values in +-2^50 (a sum of 32 stays below 2^56), two shards all zero, one value of each sign
    at the bound."""
    from lbt_amd.dfxp import ops
    rng = np.random.default_rng(stride)
    part = rng.integers(-(1 << 50), (1 << 50) + 1, size=(32, stride), dtype=np.int64)
    part[3] = 0
    part[31] = 0
    part[0, 0], part[7, stride - 1] = 1 << 50, -(1 << 50)
    sentinel = -0x0123456789ABCDEF
    d_part = torch.from_numpy(part).cuda()
    total = torch.full((32, stride), sentinel, dtype=torch.int64, device="cuda")
    ops.sums_fold(d_part, total)
    torch.cuda.synchronize()
    got = total.cpu().numpy().reshape(-1)
    assert np.array_equal(got[:stride], part.sum(axis=0, dtype=np.int64))
    assert np.all(got[stride:] == sentinel)
    assert np.array_equal(d_part.cpu().numpy(), part)


@pytest.mark.gpu
def test_sums_fold_wrapper_checks_shapes():
    from lbt_amd.dfxp import ops
    part = torch.zeros(32 * 4, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        ops.sums_fold(part, torch.zeros(3, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ops.sums_fold(part[:33], part.clone())
    with pytest.raises(ValueError):
        ops.sums_fold(part.to(torch.int32), part.clone())


# ------------------------------------------------------------------------------------------ GPU: world 1
def _trainer(cfg, mode, graph):
    """mode: 'plain' (never touched), 'noop' (sync_batchnorm at world 1 without force), 'sync' (force)."""
    from lbt_amd.distributed import sync_batchnorm
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    ctx = DfxpContext(device="cuda:0", seed=1, world_size=1)
    m = make_model(cfg, ctx)
    if mode != "plain":
        sync_batchnorm(m, force=(mode == "sync"))
    assert m.sync_bn == (mode == "sync")
    return Trainer(m, lr=1e-2, momentum=0.9, batch_size=B, use_graph=graph, exchange=True)


def _world1_worker(backend, port, out_q):
    import sys
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist

    from lbt_amd.dfxp import ops
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group(backend, rank=0, world_size=1)
    graph = backend == "nccl"
    real_allreduce, real_enter = dist.all_reduce, ops._Timed.__enter__
    reduced, kernels = [], []

    def counting_allreduce(t, *a, **kw):
        reduced.append(int(t.numel()))
        return real_allreduce(t, *a, **kw)

    def recording_enter(self):
        kernels.append(self.kernel)
        return real_enter(self)
    dist.all_reduce = counting_allreduce
    ops._Timed.__enter__ = recording_enter
    try:
        out = {}
        for name, cfg in CONFIGS.items():
            xs, ys = batches(cfg)
            xg = [torch.from_numpy(x).cuda() for x in xs]
            yg = [torch.from_numpy(y).cuda() for y in ys]
            rec = {}
            for mode in ("plain", "noop", "sync"):
                tr = _trainer(cfg, mode, graph)
                assert tr.dp and tr._lw_exact and tr.capture_comm == graph
                states, per_step = [], []
                for i in range(STEPS):
                    del reduced[:], kernels[:]
                    tr.step(xg[i], yg[i])
                    states.append(snap(tr))
                    per_step.append((list(reduced), list(kernels)))
                rec[mode] = dict(states=states, per_step=per_step, xbuf=int(tr.xbuf.numel()),
                                 channels=[n.C for n in norms(tr.model)],
                                 one_graph=(tr._graphs is not None and tr._graphs[1] is None) if graph else None)
            out[name] = rec
        out_q.put(out)
    except Exception as e:  # pragma: no cover - surfaced by the parent
        out_q.put(repr(e))
        raise
    finally:
        dist.all_reduce, ops._Timed.__enter__ = real_allreduce, real_enter
        dist.destroy_process_group()


def _spawn_world1(backend):
    """One spawned process runs every model in its three arms and sends back what they left."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_world1_worker, args=(backend, free_port(), q))
    p.start()
    res = q.get(timeout=300)
    p.join(timeout=120)
    assert p.exitcode == 0, p.exitcode
    assert not isinstance(res, str), res
    return res


@pytest.fixture(scope="module")
def world1_gloo():
    return _spawn_world1("gloo")


@pytest.fixture(scope="module")
def world1_nccl():
    return _spawn_world1("nccl")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("backend", ["gloo", "nccl"])
def test_world1_sync_path_is_the_identity(request, backend, name):
    """Three steps with sync_batchnorm(model, force=True) leave the parameters, momentum, gradients,
    exponents, step, BN running statistics and loss of the same model without it, bit for bit -- eagerly
    (gloo) and as ONE captured graph with the statistics collectives inside (nccl)."""
    rec = request.getfixturevalue("world1_" + backend)[name]
    for i in range(STEPS):
        ref, got = rec["plain"]["states"][i], rec["sync"]["states"][i]
        for k in ("w", "a", "g", "exps", "step", "loss"):
            assert np.array_equal(ref[k], got[k]), (backend, i, k)
        for k in ("mean", "var"):
            for j, (x, y) in enumerate(zip(ref[k], got[k])):
                assert np.array_equal(x, y), (backend, i, k, j)
    assert not np.array_equal(rec["plain"]["states"][0]["w"], rec["plain"]["states"][STEPS - 1]["w"])
    if backend == "nccl":
        assert rec["sync"]["one_graph"] is True  # g2 is None: folds and collectives captured with the step


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_world1_launches_and_collectives(world1_gloo, name):
    """Eager (gloo) steps, by _Timed kernel name and by dist.all_reduce call. Without sync -- never
    touched, or sync_batchnorm's world-1 no-op -- a step makes the same launches, no sums_fold_kernel, and
    one collective: the exchange. With sync it makes those launches plus two folds per Normalization_q, and
    at most 2 * (number of Normalization_q) + 1 collectives: the exchange, and per BN exactly 2C and 4C
    int64."""
    rec = world1_gloo[name]
    chans = rec["sync"]["channels"]
    for i in range(STEPS):
        (red_p, ker_p), (red_n, ker_n), (red_s, ker_s) = (rec[m]["per_step"][i] for m in ("plain", "noop", "sync"))
        assert ker_p == ker_n and len(ker_p) > 20
        assert "sums_fold_kernel" not in ker_p
        assert red_p == red_n == [rec["plain"]["xbuf"]]
        assert [k for k in ker_s if k != "sums_fold_kernel"] == ker_p
        assert ker_s.count("sums_fold_kernel") == 2 * len(chans)
        assert len(red_s) <= 2 * len(chans) + 1
        assert red_s[-1] == rec["sync"]["xbuf"]
        assert sorted(red_s[:-1]) == sorted([2 * c for c in chans] + [4 * c for c in chans])

"""Data-parallel epochs on the MI355X: Trainer.train() / evaluate() on two ranks against one process.

Two ranks are spawned ONCE as fresh processes on gloo sharing cuda:0 (as tests/test_dp_gpu.py does) and run
every data-parallel arm in the same order; the single-process arms run in this process. Each arm is the
same script -- the trainer's own train() and evaluate() -- so what is compared is what a user would run.

* case 1: ResNet-20 with SyncBN from a DeviceDataset (80 images, batch_size 32: global batches 32, 32, 16,
  shards 16, 16, 8; 2 epochs; a 40-image test set, so test shards of 20) == one process, bit for bit, with the
  evaluations that follow (test batches of 15 too: 15 runs redundantly, 10 splits into shards of 5).
* case 2: the same from host arrays (the path lbt_augment_flip_crop_at exists for).
* case 3: MNIST_Model on DfxpContext(world_size=2, rank=r) (Dropout_q, the layer-wise exact exchange).
* case 4: local BN: train() == a hand-written loop of tr.step() over the same shards, permutation and draws.
* case 5: one process, no group: the launches and results of the loops as they were.
"""
import collections
import datetime
import os
import queue
import socket
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
SEED = 20240607
WORLD = 2
N_TRAIN, N_TEST, BATCH = 80, 40, 32


# ---------------------------------------------------------------- the arms (run in the ranks and here)
def _cifar():
    rng = np.random.default_rng(42)
    return (rng.integers(0, 256, (N_TRAIN, 32, 32, 3), dtype=np.uint8), rng.integers(0, 10, N_TRAIN).astype(np.int32),
            rng.integers(0, 256, (N_TEST, 32, 32, 3), dtype=np.uint8), rng.integers(0, 10, N_TEST).astype(np.int32))


def _mnist():
    rng = np.random.default_rng(43)

    def images(n):
        return ((rng.integers(0, 256, (n, 28, 28, 1)) - 127.5) / 128).astype(np.float32)
    return images(48), rng.integers(0, 10, 48).astype(np.int32), images(24), rng.integers(0, 10, 24).astype(np.int32)


def _snap(tr):
    torch.cuda.synchronize()
    ctx = tr.ctx
    bn = [(b.X_mean_running.cpu().numpy().copy(), b.X_var_running.cpu().numpy().copy()) for b in tr._bn_layers()]
    return dict(w=tr.flat.w.cpu().numpy().copy(), a=tr.flat.a.cpu().numpy().copy(), exps=ctx.exps.cpu().numpy().copy(),
                step=ctx.step.cpu().numpy().copy(), bn=bn)


def _resnet_trainer(world, sync, dataset, **kw):
    from lbt_amd.fused import FusedResNet
    from lbt_amd.models import CIFAR10_Resnet20
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    ctx = DfxpContext(device="cuda:0", seed=0, world_size=world)
    m = FusedResNet(CIFAR10_Resnet20(8, weight_decay=2e-4, ctx=ctx), sync_bn=sync)
    return Trainer(m, dataset=dataset, lr=1e-2, momentum=0.9, batch_size=BATCH, n_epoch=2, **kw)


def _datasets(kind):
    """((train), (test)) as Trainer takes it, and the test set as evaluate()'s arguments."""
    from lbt_amd.data import DeviceDataset
    Xtr, ytr, Xte, yte = _cifar()
    ds = DeviceDataset(Xtr, ytr, device="cuda:0")
    ds_te = DeviceDataset(Xte, yte, mean=ds.mean, device="cuda:0")
    if kind == "device":
        return (ds, ds_te), (ds_te,)
    return ((ds.host_float(), ytr), (ds_te.host_float(), yte)), (ds_te.host_float(), yte)


def _launch_counts(fn):
    from lbt_amd.dfxp import ops
    ops.PROFILE = {}
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, {k: len(v) for k, v in ops.PROFILE.items()}
    finally:
        ops.PROFILE = None


def _epochs(tr, te, seed=SEED):
    """train() and the evaluations after it: the sequence every arm of cases 1 and 2 runs."""
    torch.manual_seed(seed)
    out = dict(history=tr.train(augment=True), sizes=list(tr.batch_sizes), global_step=tr.global_step)
    out["trained"] = _snap(tr)
    out["eval"], out["eval_launches"] = _launch_counts(lambda: tr.evaluate(*te))
    out["after_eval"] = _snap(tr)
    out["eval_testing"], out["testing_launches"] = _launch_counts(lambda: tr.evaluate(*te, testing=True))
    out["after_testing"] = _snap(tr)
    out["eval15"] = tr.evaluate(*te, batch_size=15)
    out["after15"] = _snap(tr)
    out["eval15_testing"] = tr.evaluate(*te, batch_size=15, testing=True)
    out["after15_testing"] = _snap(tr)
    out["plans"] = sorted(repr(k) for k in tr._eval)
    out["train_plans"] = sorted(tr._plans) + [tr.model._shape[0]]
    return out


def _arm_resnet(world, kind, seed=SEED):
    dataset, te = _datasets(kind)
    return _epochs(_resnet_trainer(world, True, dataset), te, seed)


def _arm_mnist(world, rank, seed=SEED):
    from lbt_amd.models import MNIST_Model
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    X, y, Xt, yt = _mnist()
    ctx = DfxpContext(device="cuda:0", seed=1, world_size=world, rank=rank if world > 1 else None)
    gm = MNIST_Model(8, dropout=0.5, weight_decay=1e-4, ctx=ctx)
    # (the default gradient range quantises these narrow gradients to zero: tests/test_dp_dropout_gpu.py)
    ctx.set_ranges({q.name: -6 for q in ctx.quantizers if q.name.endswith("/grad_range")})
    tr = Trainer(gm, dataset=((X, y), (Xt, yt)), lr=1e-2, momentum=0.9, batch_size=16, n_epoch=1)
    w0 = tr.flat.w.cpu().numpy().copy()
    torch.manual_seed(seed)
    out = dict(history=tr.train(augment=True), sizes=list(tr.batch_sizes), global_step=tr.global_step, w0=w0)
    out["trained"] = _snap(tr)
    out["eval"] = tr.evaluate(Xt, yt)
    out["after_eval"] = _snap(tr)
    out["exact"] = bool(tr.dp and tr._lw_exact and tr.comm is None)
    return out


def _arm_local_bn(world, rank):
    """Case 4: train() of a local-BN plan, and the same epochs written by hand around tr.step()."""
    from lbt_amd.dfxp import ops
    from lbt_amd.trainer import shard_rows
    dataset, _ = _datasets("host")
    (Xf, ytr), _ = dataset
    a = _resnet_trainer(world, False, ((Xf, ytr), (None, None)))
    torch.manual_seed(SEED)
    a.train(augment=True)
    b = _resnet_trainer(world, False, None)
    torch.manual_seed(SEED)  # every rank: the permutations rank 0 drew and broadcast above
    keep = {}
    for epoch in range(2):
        if epoch == 0:
            b.get_train_op()
        perm = torch.randperm(N_TRAIN).numpy()
        for s in range(0, N_TRAIN, BATCH):
            nb = min(BATCH, N_TRAIN - s)
            lo, hi = shard_rows(nb, world, rank)
            idx = perm[s + lo:s + hi]
            X = torch.from_numpy(Xf[idx]).to("cuda:0")
            y = torch.from_numpy(ytr[idx]).to("cuda:0")
            if hi - lo not in keep:  # one buffer pair per shard size: a captured graph reads it in place
                keep[hi - lo] = (torch.empty_like(X), torch.empty_like(y))
            Xs, ys = keep[hi - lo]
            ops.augment_flip_crop(X, 4, b.ctx.seed, b.global_step, out=Xs, base=lo)
            ys.copy_(y)
            b.step(Xs, ys)
    return dict(train=_snap(a), manual=_snap(b), steps=(a.global_step, b.global_step), sizes=list(a.batch_sizes))


def _rank_main(rank, world, port, out_q):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    # a rank whose peer is gone fails at its next collective instead of waiting for it
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        seed = SEED + 1000 * rank  # only rank 0 seeds as the single process does: its draws are the epoch's
        out = dict(device=_arm_resnet(world, "device", seed), host=_arm_resnet(world, "host", seed),
                   mnist=_arm_mnist(world, rank, seed), local=_arm_local_bn(world, rank))
        out_q.put((rank, out))
    except Exception as e:  # pragma: no cover - surfaced by the parent
        import traceback
        out_q.put((rank, repr(e) + "\n" + traceback.format_exc()))
        raise
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(world):
    """The ranks' results. Never retried; a rank that exits without reporting fails at once."""
    mctx = mp.get_context("spawn")
    q = mctx.Queue()
    port = _free_port()
    procs = [mctx.Process(target=_rank_main, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res, deadline = [], time.monotonic() + 420
    try:
        while len(res) < world:
            try:
                res.append(q.get(timeout=2))
            except queue.Empty:
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                assert not dead, "a rank exited with %r before reporting" % dead
                assert time.monotonic() < deadline, "the ranks did not report within 420 s"
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


@pytest.fixture(scope="module")
def ranks():
    return _run_ranks(WORLD)


@pytest.fixture(scope="module")
def one_resnet():
    return _arm_resnet(1, "device")


def _same(a, b, what):
    for k in ("w", "a", "exps", "step"):
        assert np.array_equal(a[k], b[k]), (what, k)
    assert len(a["bn"]) == len(b["bn"])
    for i, ((ma, va), (mb, vb)) in enumerate(zip(a["bn"], b["bn"])):
        assert np.array_equal(ma, mb) and np.array_equal(va, vb), (what, "bn", i)


STAGES = ("trained", "after_eval", "after_testing", "after15", "after15_testing")


def _check_resnet(got, ref, what):
    assert got["sizes"] == ref["sizes"] == [32, 32, 16]  # the global nb
    assert got["global_step"] == ref["global_step"] == 6
    assert got["history"] == ref["history"] and len(ref["history"]) == 2
    for stage in STAGES:
        _same(got[stage], ref[stage], (what, stage))
    for k in ("eval", "eval_testing", "eval15", "eval15_testing"):
        (acc, loss), (racc, rloss) = got[k], ref[k]
        print(what, k, "accuracy", acc, racc, "loss", loss, rloss)
        if k in ("eval", "eval_testing"):  # the 40-image batch: equal exactly
            assert acc == racc, (what, k)
        else:
            # a batch's sharded accuracy is the correctly rounded fp32 quotient correct / nb; one process takes
            # torch's mean(), which multiplies the count by the ROUNDED reciprocal of nb: for nb = 15 (1 / 15 is
            # no fp32 number) the two may differ by the product's two roundings, 2 * 2^-24 relative on a value
            # <= 1, and so may the mean over the batches
            assert abs(acc - racc) <= 2.0 ** -23, (what, k, acc, racc)
        assert abs(loss - rloss) <= 1e-6 * abs(rloss), (what, k, loss, rloss)  # the 2^-32 fixed-point loss sum


# ---------------------------------------------------------------- the cases
@pytest.mark.timeout(600)
def test_case1_syncbn_device_dataset_two_ranks_equal_one_process(ranks, one_resnet):
    ref = one_resnet
    assert ref["train_plans"] == [16, 32] and len(ref["trained"]["bn"]) > 10
    assert not np.array_equal(ref["trained"]["w"], ref["trained"]["a"])
    # the training-mode test loop moves the running statistics; the testing-mode loop moves nothing
    assert any(not np.array_equal(x[0], y[0]) for x, y in zip(ref["trained"]["bn"], ref["after_eval"]["bn"]))
    _same(ref["after_eval"], ref["after_testing"], "one process, testing mode")
    for r, rec in enumerate(ranks):
        got = rec["device"]
        assert got["train_plans"] == [8, 16]  # the shards' plans
        _check_resnet(got, ref, "device rank %d" % r)
        # the sharded test loop ran: a SyncBN eval plan and an inference plan per shard size, the batch of 15
        # redundantly; one tally launch per batch in place of the loss launch
        for key in ('("sync", 20)', '("sync", 5)', '("testing", 20)', '("testing", 5)', '("testing", 15)', "15"):
            assert key.replace('"', "'") in got["plans"], (key, got["plans"])
        for launches in (got["eval_launches"], got["testing_launches"]):
            assert launches.get("eval_tally_kernel") == 1 and not any("softmax" in k for k in launches), launches
    for stage in STAGES:
        _same(ranks[0]["device"][stage], ranks[1]["device"][stage], ("rank 0 / rank 1", stage))
    assert not any("tally" in k for k in list(ref["eval_launches"]) + list(ref["testing_launches"]))


@pytest.mark.timeout(600)
def test_case2_syncbn_host_arrays_two_ranks_equal_one_process(ranks, one_resnet):
    for r, rec in enumerate(ranks):
        _check_resnet(rec["host"], one_resnet, "host rank %d" % r)
        for stage in STAGES:
            _same(rec["host"][stage], rec["device"][stage], ("host / device", r, stage))
        for k in ("eval", "eval_testing", "eval15", "eval15_testing"):
            assert rec["host"][k] == rec["device"][k], (r, k)  # the same integers, decoded the same way
    for stage in STAGES:
        _same(ranks[0]["host"][stage], ranks[1]["host"][stage], ("rank 0 / rank 1", stage))


@pytest.mark.timeout(600)
def test_case3_dropout_model_on_ranked_contexts_equals_one_process(ranks):
    ref = _arm_mnist(1, None)
    assert ref["sizes"] == [16, 16, 16] and ref["global_step"] == 3 and not ref["exact"]
    assert not np.array_equal(ref["trained"]["w"], ref["w0"])
    for r, rec in enumerate(ranks):
        got = rec["mnist"]
        assert got["exact"], "the exact layer-wise exchange must be the one in use"
        assert got["sizes"] == ref["sizes"] and got["global_step"] == 3
        assert np.array_equal(got["w0"], ref["w0"])
        _same(got["trained"], ref["trained"], ("mnist trained", r))
        _same(got["after_eval"], ref["after_eval"], ("mnist evaluated", r))
        assert got["history"] == ref["history"] and len(ref["history"]) == 1
        print("mnist rank", r, got["eval"], ref["eval"])
        assert got["eval"][0] == ref["eval"][0]  # the redundant loop: the whole test set on every rank
        assert abs(got["eval"][1] - ref["eval"][1]) <= 1e-6 * abs(ref["eval"][1])
    _same(ranks[0]["mnist"]["after_eval"], ranks[1]["mnist"]["after_eval"], "rank 0 / rank 1")


@pytest.mark.timeout(600)
def test_case4_local_bn_train_is_the_hand_written_shard_loop(ranks):
    for r, rec in enumerate(ranks):
        got = rec["local"]
        assert got["steps"] == (6, 6) and got["sizes"] == [32, 32, 16]
        _same(got["train"], got["manual"], ("train() / tr.step() loop", r))
    # one model on both ranks: parameters, momentum, exponents (local BN: each rank its own running statistics)
    for k in ("w", "a", "exps", "step"):
        assert np.array_equal(ranks[0]["local"]["train"][k], ranks[1]["local"]["train"][k]), k
    # ... and sharding changes what is trained: local BN over 16 rows is not BN over 32
    assert not np.array_equal(ranks[0]["local"]["train"]["w"], ranks[0]["device"]["trained"]["w"])


@pytest.mark.timeout(600)
def test_case5_one_process_makes_the_launches_it_made():
    """No group: train() issues, by kernel name, the launches of the loop as it was written before sharding
    (restated here around tr.step()), and ends in the same state; evaluate() issues exactly its plans' forward
    and loss launches per batch -- no tally, no collective -- and returns what those launches give."""
    from lbt_amd.dfxp import ops
    dataset, te = _datasets("host")
    (Xf, ytr), (Xte, yte) = dataset
    a = _resnet_trainer(1, True, dataset, use_graph=False)
    assert not a._shard and a._shard_of(17) == (0, 17)
    torch.manual_seed(SEED)
    hist, la = _launch_counts(lambda: a.train(augment=True))

    b = _resnet_trainer(1, True, None, use_graph=False)
    torch.manual_seed(SEED)

    def old_loop():
        history = []
        for epoch in range(2):
            if epoch == 0:
                b.get_train_op()
            perm = torch.randperm(len(Xf))
            for s in range(0, len(Xf), BATCH):
                idx = perm[s:s + BATCH]
                X = torch.as_tensor(Xf[idx.numpy()], dtype=torch.float32).to("cuda:0").contiguous()
                y = torch.as_tensor(ytr[idx.numpy()], dtype=torch.int32).to("cuda:0")
                X = ops.augment_flip_crop(X, 4, b.ctx.seed, b.global_step)
                b.step(X, y)
            history.append(b.evaluate(Xte, yte)[0])
        return history
    hist_b, lb = _launch_counts(old_loop)
    assert la == lb and sum(la.values()) > 100
    assert hist == hist_b
    _same(_snap(a), _snap(b), "train() / the loop as it was")
    assert not any("tally" in k or k == "allreduce" for k in la)

    # evaluate(): per batch its plan's forward + loss launches, nothing else
    for testing, sizes in ((False, [40]), (True, [40]), (True, [15, 15, 10])):
        res, got = _launch_counts(lambda: a.evaluate(Xte, yte, batch_size=sizes[0], testing=testing))
        want = collections.Counter()
        for nb in sizes:
            p = a._eval[("testing", nb) if testing else nb]
            want.update(f.kname for f in p._fwd + p._hfwd + p._hloss)
        assert got == dict(want), (testing, sizes)
    # ... and the pair those launches give: torch's argmax / mean and the plan's loss, per batch
    acc_sum = loss_sum = 0.0
    for s in range(0, N_TEST, 15):
        Xb = torch.from_numpy(Xte[s:s + 15]).to("cuda:0")
        yb = torch.from_numpy(yte[s:s + 15]).to("cuda:0")
        p = a._eval[("testing", len(Xb))]
        logits = p.forward(Xb)
        loss_sum += float(p.compute_loss(yb).item())
        acc_sum += float((logits.argmax(dim=1).to(torch.int32) == yb).float().mean().item())
    assert res == (acc_sum / 3, loss_sum / 3)
    assert a.evaluate(*_datasets("device")[1], batch_size=15, testing=True) == res

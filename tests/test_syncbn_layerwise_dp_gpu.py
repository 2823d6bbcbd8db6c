"""SyncBN for the layer-wise models on two ranks: N ranks equal one process, bit for bit.

Two ranks are spawned once for the module; they share cuda:0 over gloo (the one-GPU rehearsal of the RCCL
path: the same Trainer and layer code, only the transport differs). Every rank takes 4 rows of the global
batch of 8 (default_rng(5), as tests/test_dp_resnet50_gpu.py), two steps, on the smallest models at which
each kernel path exists: the 8-bit chains, the wide (16-bit gradient) backward, at width 64 the fused
bottleneck schedule (quantising GEMM epilogue, dgrad + pass A, the bn3 entry), and the layer-wise CIFAR
ResNet with one block per stage.

Expected values: the ORACLE's one-process step on the whole batch (oracle.resnet.train_step, fed the two
ranks' d loss / d logits rows concatenated: the softmax is the one op that is not bit-exact), and a
one-process GPU trainer at B = 8 with the same seed. Against a vacuous pass the oracle's two-shard step with
local BN statistics (dp_train_step) must differ from its one-process step.
"""
import hashlib
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_syncbn_layerwise import B, CONFIGS, ROOT, batches, free_port, make_model, norms, shape_of

pytestmark = pytest.mark.gpu
STEPS = 2
N_TEST, TEST_BATCH = 12, 6
KEY = {"W": "/W", "gamma": "/g", "beta": "/b"}


def _digest(t):
    return hashlib.sha256(np.ascontiguousarray(t).tobytes()).hexdigest()


def _test_set(cfg):
    image, classes = shape_of(cfg)
    rng = np.random.default_rng(7)
    X = ((rng.integers(0, 256, size=(N_TEST, image, image, 3)) - 127.5) / 128).astype(np.float32)
    return X, rng.integers(0, classes, size=N_TEST).astype(np.int32)


def _make(world, cfg, sync):
    from lbt_amd.distributed import sync_batchnorm
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    ctx = DfxpContext(device="cuda:0", seed=1, world_size=world)
    gm = make_model(cfg, ctx)
    if sync:
        sync_batchnorm(gm)
    return ctx, gm, Trainer(gm, lr=1e-2, momentum=0.9, batch_size=B // world, use_graph=True)


def _bn(gm):
    return [(n.X_mean_running.cpu().numpy().copy(), n.X_var_running.cpu().numpy().copy()) for n in norms(gm)]


def _state(ctx, gm, tr, full):
    """What a step leaves. full: the parameters themselves (for the oracle's per-tensor comparison);
    everything else that is compared for bit-equality travels as a digest."""
    torch.cuda.synchronize()
    w = tr.flat.w.cpu().numpy()
    s = dict(loss=float(gm.loss.item()), dz=gm.dlogits.cpu().numpy().copy(), ranges=ctx.ranges(),
             exps=_digest(ctx.exps.cpu().numpy()), step=int(ctx.step.item()), w=_digest(w),
             a=_digest(tr.flat.a.cpu().numpy()), g=_digest(tr.flat.g.cpu().numpy()), bn=_bn(gm))
    if full:
        s["w_full"] = w.copy()
    return s


def _run_model(ctx, gm, tr, xs, ys, lo, hi, full):
    """STEPS training steps on rows [lo, hi) of every batch, then evaluate() on the test set."""
    xr = [torch.from_numpy(x[lo:hi].copy()).cuda() for x in xs]
    yr = [torch.from_numpy(y[lo:hi].copy()).cuda() for y in ys]
    steps = []
    for i in range(STEPS):
        tr.step(xr[i], yr[i])
        steps.append(_state(ctx, gm, tr, full))
    return steps


def _worker(rank, world, port, out_q):
    import sys
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out = {}
        b = B // world
        for name, cfg in CONFIGS.items():
            ctx, gm, tr = _make(world, cfg, True)
            assert gm.sync_bn and all(n.sync == (None, world) for n in norms(gm))
            assert tr.dp and tr._lw_exact and tr.comm is None, "the exact layer-wise exchange must be the one in use"
            xs, ys = batches(cfg, STEPS)
            steps = _run_model(ctx, gm, tr, xs, ys, rank * b, (rank + 1) * b, full=(rank == 0))
            ev = tr.evaluate(*_test_set(cfg), batch_size=TEST_BATCH)
            torch.cuda.synchronize()
            assert gm.sync_bn and all(n.sync == (None, world) for n in norms(gm))  # restored after the test loop
            out[name] = dict(steps=steps, eval=ev, eval_bn=_bn(gm), eval_exps=_digest(ctx.exps.cpu().numpy()))
        out_q.put((rank, out))
    except Exception as e:  # pragma: no cover - surfaced by the parent
        out_q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def ranks():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0, p.exitcode
    for _, rec in res:
        assert not isinstance(rec, str), rec
    return [rec for _, rec in res]


_ONE = {}


def _one_process(name):
    """The one-process GPU trainer on the whole batch (no SyncBN, no group), once per config."""
    if name not in _ONE:
        cfg = CONFIGS[name]
        ctx, gm, tr = _make(1, cfg, False)
        assert not gm.sync_bn and not tr.dp
        xs, ys = batches(cfg, STEPS)
        steps = _run_model(ctx, gm, tr, xs, ys, 0, B, full=True)
        ev = tr.evaluate(*_test_set(cfg), batch_size=TEST_BATCH)
        torch.cuda.synchronize()
        _ONE[name] = dict(steps=steps, eval=ev, eval_bn=_bn(gm), eval_exps=_digest(ctx.exps.cpu().numpy()),
                          offsets=[(o.name + KEY[v], off, sz, tuple(getattr(o, v).shape))
                                   for o, v, off, sz in tr.flat.offsets])
    return _ONE[name]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_two_ranks_agree(ranks, name):
    """One model on both ranks: parameters, momentum, gradients, exponents, BN running statistics."""
    r0, r1 = ranks[0][name], ranks[1][name]
    for i, (s0, s1) in enumerate(zip(r0["steps"], r1["steps"])):
        for k in ("w", "a", "g", "exps", "step", "ranges"):
            assert s0[k] == s1[k], (i, k)
        for j, ((m0, v0), (m1, v1)) in enumerate(zip(s0["bn"], s1["bn"])):
            assert np.array_equal(m0, m1) and np.array_equal(v0, v1), (i, j)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_two_ranks_equal_the_oracles_one_process_step(ranks, name):
    """Parameters and exponents after each step equal oracle.resnet.train_step on the WHOLE batch bit for bit
    (dz rows: rtol 1e-5 / atol 1e-9, loss: relative 1e-5 -- the softmax's bounds of
    tests/test_dp_resnet50_gpu.py); and the oracle's local-BN two-shard step on the same shards gives other
    parameters, so the equality is SyncBN's doing."""
    from oracle import resnet as oresnet
    cfg = CONFIGS[name]
    r0, r1 = ranks[0][name]["steps"], ranks[1][name]["steps"]
    _, gm, tr = _make(1, cfg, False)  # same seed: the same initial parameters and flat layout
    if cfg == "cifar":
        om = oresnet.build_resnet((1, 1, 1), 8, 1e-4)
    else:
        blocks, width, image, classes, grad_bits = cfg
        om = oresnet.build_resnet50(blocks, width, classes, 8, grad_bits, weight_decay=1e-4)
    params = {o.name + KEY[v]: getattr(o, v).detach().cpu().numpy() for o, v, _ in gm.param_slots()}
    state = dict(params=params, accum={k: np.zeros_like(v) for k, v in params.items()},
                 ranges=oresnet.init_ranges(om), step=0)
    xs, ys = batches(cfg, STEPS)
    b = B // 2
    for i in range(STEPS):
        dzs = [r0[i]["dz"], r1[i]["dz"]]
        if i == 0:  # against a vacuous pass: local BN statistics train another network
            shards = [(xs[i][r * b:(r + 1) * b], ys[i][r * b:(r + 1) * b]) for r in range(2)]
            _, local, _ = oresnet.dp_train_step(om, state, shards, seed=1, dzs=dzs)
        loss, new_state, octx = oresnet.train_step(om, state, xs[i], ys[i], seed=1, dz=np.concatenate(dzs))
        if i == 0:
            differ = [k for k in new_state["params"] if not np.array_equal(local["params"][k], new_state["params"][k])]
            assert differ, "local-BN shards gave the one-process parameters: the comparison shows nothing"
        np.testing.assert_allclose(np.concatenate(dzs), octx.dz, rtol=1e-5, atol=1e-9)
        assert abs(r0[i]["loss"] - loss) <= 1e-5 * abs(loss), (i, r0[i]["loss"], loss)
        got = {o.name + KEY[v]: r0[i]["w_full"][off:off + sz].reshape(getattr(o, v).shape)
               for o, v, off, sz in tr.flat.offsets}
        for k in new_state["params"]:
            assert np.array_equal(got[k], new_state["params"][k]), (i, k)
        assert r0[i]["ranges"] == new_state["ranges"], i
        state = new_state


@pytest.mark.parametrize("name", list(CONFIGS))
def test_two_ranks_equal_one_process_on_the_gpu(ranks, name):
    """A one-process trainer at B = 8 with the same seed: parameters, momentum, exponents, step and every BN
    running mean and variance bit for bit; the loss to 1e-6 (the 2^-32 fixed-point loss sum);
    each rank's dz rows are the one process's."""
    one = _one_process(name)
    for i in range(STEPS):
        ref = one["steps"][i]
        for r in range(2):
            s = ranks[r][name]["steps"][i]
            for k in ("w", "a", "exps", "step", "ranges"):
                assert s[k] == ref[k], (i, r, k)
            for j, ((ma, va), (mb, vb)) in enumerate(zip(s["bn"], ref["bn"])):
                assert np.array_equal(ma, mb) and np.array_equal(va, vb), (i, r, j)
            assert abs(s["loss"] - ref["loss"]) <= 1e-6 * abs(ref["loss"]), (i, r, s["loss"], ref["loss"])
        assert np.array_equal(np.concatenate([ranks[r][name]["steps"][i]["dz"] for r in range(2)]), ref["dz"]), i


@pytest.mark.parametrize("name", list(CONFIGS))
def test_evaluate_on_two_ranks_is_the_one_process_test_loop(ranks, name):
    """evaluate() of the synced model (12 images, batch_size 6: every rank runs each test batch whole, the
    synchronisation suspended) returns the one process's accuracy and loss on both ranks, and leaves its
    running statistics and exponents."""
    one = _one_process(name)
    for r in range(2):
        got = ranks[r][name]
        assert got["eval"][0] == one["eval"][0], r
        assert abs(got["eval"][1] - one["eval"][1]) <= 1e-6 * abs(one["eval"][1]), (r, got["eval"], one["eval"])
        for j, ((ma, va), (mb, vb)) in enumerate(zip(got["eval_bn"], one["eval_bn"])):
            assert np.array_equal(ma, mb) and np.array_equal(va, vb), (r, j)
        assert got["eval_exps"] == one["eval_exps"], r
    # the test loop moved the running statistics (training-mode forwards, trainer.py:164-190)
    last = one["steps"][-1]["bn"]
    assert any(not np.array_equal(m0, m1) for (m0, _), (m1, _) in zip(last, one["eval_bn"]))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_one_process_test_loop_is_the_oracles(name):
    """What the ranks are compared with is itself right: the one-process evaluate() after the two training
    steps equals the oracle's forwards of the two test batches -- each batch's own moments, not sums left
    over from the training step -- in accuracy, loss (1e-5: the softmax) and, bit for bit, in the running
    statistics it leaves."""
    from oracle import nn as onn
    from oracle import resnet as oresnet
    cfg = CONFIGS[name]
    one = _one_process(name)
    if cfg == "cifar":
        om = oresnet.build_resnet((1, 1, 1), 8, 1e-4)
    else:
        blocks, width, image, classes, grad_bits = cfg
        om = oresnet.build_resnet50(blocks, width, classes, 8, grad_bits, weight_decay=1e-4)
    trained = one["steps"][-1]
    oresnet.set_params(om, {k: trained["w_full"][off:off + sz].reshape(shape) for k, off, sz, shape in one["offsets"]})
    on = [l for l in oresnet._walk(om) if isinstance(l, onn.NormQ)]
    assert len(on) == len(trained["bn"])
    for o, (m, v) in zip(on, trained["bn"]):
        o.mean_running, o.var_running = m.copy(), v.copy()
    X, y = _test_set(cfg)
    accs, losses = [], []
    for b in range(0, N_TEST, TEST_BATCH):
        z = om.forward(X[b:b + TEST_BATCH], onn.Ctx(dict(trained["ranges"]), trained["step"], 1))
        l, _ = onn.softmax_xent(z, y[b:b + TEST_BATCH])
        accs.append(float(np.mean((np.argmax(z, 1) == y[b:b + TEST_BATCH]).astype(np.float32))))
        losses.append(l)
    acc, loss = one["eval"]
    assert acc == pytest.approx(sum(accs) / len(accs), abs=1e-7)
    assert abs(loss - sum(losses) / len(losses)) <= 1e-5 * abs(sum(losses) / len(losses))
    for j, (o, (m, v)) in enumerate(zip(on, one["eval_bn"])):
        assert np.array_equal(o.mean_running, m) and np.array_equal(o.var_running, v), j

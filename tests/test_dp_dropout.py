"""Data-parallel training of the Dropout_q models, host side (no GPU): the context's declared rank, the
Trainer's decisions, the four new entry points' ABI and host-side argument checks, and the numpy
data-parallel oracle (tests/plain_dp_oracle.py) against the one-process oracle on the whole batch."""
import ctypes

import numpy as np
import pytest
import torch.distributed as dist

import plain_dp_oracle as DP
import plain_oracle as P
from lbt_amd import _lib
from lbt_amd.runtime import DfxpContext

F32 = np.float32
NEW = ("lbt_dropout_fwd_at", "lbt_dropout_bwd_at", "lbt_dropout_quantize_at", "lbt_bias_grad_x")
MAXN = 1 << 34


@pytest.fixture
def one_rank_group(tmp_path):
    own = not dist.is_initialized()
    if own:
        dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "pg"), rank=0, world_size=1)
    yield
    if own:
        dist.destroy_process_group()


def test_context_rank_is_validated_and_defaults_to_none():
    assert DfxpContext(device="cpu").rank is None
    assert DfxpContext(device="cpu", world_size=4, rank=3).rank == 3
    for world, rank in ((1, 1), (4, 4), (2, -1)):
        with pytest.raises(ValueError):
            DfxpContext(device="cpu", world_size=world, rank=rank)


def test_mask_base_is_the_shard_offset_only_inside_the_training_step():
    ctx = DfxpContext(device="cpu", world_size=4, rank=3)
    assert ctx.mask_base(15) is None  # evaluation, plain forward: the masks one process draws
    with ctx.shard_masks():
        assert ctx.mask_base(15) == 45
        with ctx.shard_masks():
            assert ctx.mask_base(1 << 31) == 3 << 31
        assert ctx.mask_base(16) == 48
    assert ctx.mask_base(15) is None
    plain = DfxpContext(device="cpu", world_size=4)
    with plain.shard_masks():
        assert plain.mask_base(15) is None  # no declared rank: today's entry points


def test_trainer_with_a_declared_rank_takes_a_dropout_model(one_rank_group):
    from lbt_amd.models import MNIST_Model
    from lbt_amd.trainer import Trainer
    tr = Trainer(MNIST_Model(8, ctx=DfxpContext(device="cpu", world_size=1, rank=0)), exchange=True)
    assert tr.dp and tr._lw_exact and tr.comm is None and tr.xbuf is not None
    # one finish segment per parameter tensor; the biases dequantise as kind 2
    segs = (_lib.FSeg * len(tr.flat.offsets)).from_buffer_copy(tr._segs.numpy().tobytes())
    assert [s.kind for s in segs] == [2 if v == "b" else 0 for _, v, _, _ in tr.flat.offsets]
    assert {v for _, v, _, _ in tr.flat.offsets} == {"W", "b"}


def test_trainer_rejects_a_rank_that_is_not_the_process_groups(one_rank_group, monkeypatch):
    """The group answers as rank 0 of 2 (a one-process stand-in: the check comes before anything is
    exchanged); the context says rank 1."""
    from lbt_amd.models import MNIST_Model
    from lbt_amd.trainer import Trainer
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    with pytest.raises(ValueError, match=r"DfxpContext\.rank"):
        Trainer(MNIST_Model(8, ctx=DfxpContext(device="cpu", world_size=2, rank=1)))
    with pytest.raises(ValueError, match=r"DfxpContext\.rank"):  # without dropout too
        Trainer(MNIST_Model(8, dropout=1.0, ctx=DfxpContext(device="cpu", world_size=2, rank=1)))


def test_float_mode_model_with_dropout_is_refused_by_layer_name(one_rank_group):
    from lbt_amd.models import PI_MNIST_Model
    from lbt_amd.trainer import Trainer
    with pytest.raises(NotImplementedError, match="dense1"):
        Trainer(PI_MNIST_Model(16, ctx=DfxpContext(device="cpu", world_size=1, rank=0)), exchange=True)


def test_without_a_declared_rank_every_decision_is_unchanged(one_rank_group):
    from lbt_amd import distributed as D
    from lbt_amd.models import MNIST_Model
    m = MNIST_Model(8, dropout=1.0, ctx=DfxpContext(device="cpu"))
    assert not D.exact_layerwise_ok(m) and D.exact_layerwise_ok(m, biases=True)
    assert D.float_mode_layer(m) is None and D.float_mode_layer(m, biases=False) is m.layers[0]


def test_new_symbols_are_exported_under_abi_24():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 24 == lib.lbt_abi_version()
    for name in NEW:
        assert name in _lib.EXPORTED and hasattr(lib, name), name


def test_host_side_window_checks():
    """Rejected on the host before any HIP call (no GPU here; the pointers are never dereferenced):
    base < 0 and base + n > 2^34. base = 2^34 - n is the last accepted base: there a null step pointer
    is still what rejects the call."""
    lib = _lib.load()
    p = ctypes.c_void_p(0x1000)
    q = _lib.QDesc()
    q.bits = 8
    n = 16
    for base in (-1, -4, MAXN - n + 1, MAXN, MAXN + 4, 1 << 62):
        assert lib.lbt_dropout_fwd_at(p, p, n, base, 0.5, p, 0, 1, 0, None) == 1001, base
        assert lib.lbt_dropout_bwd_at(p, p, n, base, 0.5, p, 0, 1, None, None) == 1001, base
        assert lib.lbt_dropout_quantize_at(p, p, _lib.OUT_I8, 4, 4, base, 0.5, 1, 0, q, None) == 1001, base
    last = MAXN - n
    assert lib.lbt_dropout_fwd_at(p, p, n, last, 0.5, None, 0, 1, 0, None) == 1001
    assert lib.lbt_dropout_bwd_at(p, p, n, last, 0.5, None, 0, 1, None, None) == 1001
    # ... and with nothing to do the last base (and one past the end of an empty window) succeeds
    assert lib.lbt_dropout_fwd_at(p, p, 0, MAXN, 0.5, p, 0, 1, 0, None) == 0
    assert lib.lbt_dropout_quantize_at(p, p, _lib.OUT_I8, 0, 4, last, 0.5, 1, 0, q, None) == 0
    # the other argument checks of the plain entry points hold at a base too
    assert lib.lbt_dropout_fwd_at(p, p, n, 4, 0.0, p, 0, 1, 0, None) == 1001
    assert lib.lbt_dropout_quantize_at(p, p, _lib.OUT_F32, 4, 64, 4, 0.5, 1, 0, q, None) == 1001
    assert lib.lbt_dropout_quantize_at(p, p, _lib.OUT_I8, 1 << 20, 1 << 14, 4, 0.5, 1, 0, q, None) == 1001
    assert lib.lbt_bias_grad_x(None, 8, p, None) == 1001
    assert lib.lbt_bias_grad_x(p, 8, None, None) == 1001
    assert lib.lbt_bias_grad_x(p, 0, p, None) == 1001


# ---- the oracle: N shards at their global offsets are one process on the whole batch ------------------
B, STEPS = 8, 2
MODELS = {"mnist": (P.mnist, (28, 28, 1)), "pi_mnist": (P.pi_mnist, (784,))}


def _init(om, seed):
    rng = np.random.default_rng(seed)
    params = {}
    for name, owner in om.params():
        shape = owner.b.shape if name.endswith("/bias") else (
            owner.ksize if isinstance(owner, P.nn.Conv2dQ) else (owner.in_units, owner.units))
        fan = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
        scale = 0.05 if name.endswith("/bias") else (3.0 / fan) ** 0.5
        params[name] = (rng.uniform(-1, 1, size=shape) * scale).astype(F32)
    # gradient ranges low enough that the 8-bit gradient codes are not all zero
    ranges = {r: (-6 if r.endswith("/grad_range") else 2) for r in om.range_names()}
    return dict(params=params, accum={k: np.zeros_like(v) for k, v in params.items()}, ranges=ranges, step=0)


def _same(a, b):
    return (a["ranges"] == b["ranges"] and all(np.array_equal(a["params"][k], b["params"][k]) and
                                               np.array_equal(a["accum"][k], b["accum"][k]) for k in a["params"]))


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("case", sorted(MODELS))
def test_oracle_shards_at_global_offsets_equal_the_whole_batch(case, world):
    build, shape = MODELS[case]
    om = DP.shardable(build(8, 0.5, 1e-4))
    assert len(DP.dropouts(om)) == 2
    s_one = s_dp = s_zero = _init(om, 3)
    rng = np.random.default_rng(11)
    b = B // world
    for i in range(STEPS):
        x = ((rng.integers(0, 256, size=(B,) + shape) - 127.5) / 128).astype(F32)
        y = rng.integers(0, 10, size=B).astype(np.int32)
        shards = [(x[r * b:(r + 1) * b], y[r * b:(r + 1) * b]) for r in range(world)]
        l_one, s_one, c_one = P.train_step(om, s_one, x, y, seed=5)
        l_dp, s_dp, ctxs = DP.dp_train_step(om, s_dp, shards, seed=5)
        _, s_zero, zctxs = DP.dp_train_step(om, s_zero, shards, seed=5, global_masks=False)
        assert abs(l_dp - l_one) <= 1e-6 * abs(l_one)
        assert _same(s_dp, s_one), (case, world, i)
        assert not _same(s_zero, s_one), (case, world, i)  # ranks that ignore their position: another step
        assert any(not np.array_equal(g, F32(2e-4) * s_one["params"][k]) for k, g in c_one.grads.items()
                   if k.endswith("/W"))  # not vacuous: some data gradient is non-zero
        for name in ctxs[0].masks:
            assert not np.array_equal(ctxs[0].masks[name], ctxs[1].masks[name]), name
            assert np.array_equal(zctxs[0].masks[name], zctxs[1].masks[name]), name
            share = 1 - np.concatenate([c.masks[name].ravel() for c in ctxs]).mean()
            assert 0.3 < share < 0.7, (name, share)

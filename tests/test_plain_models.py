"""The reference's four plain models (models.py:57-368) on the HIP layers against the numpy oracle
(tests/plain_oracle.py): one training step each by the method of the ResNet-20 step tests (the GPU's
d loss / d logits injected into the oracle's backward; everything else bit-equal), two replays of
the captured step, and the testing-mode forward."""
import numpy as np
import pytest
import torch

import plain_oracle as P
from lbt_amd import models
from lbt_amd.runtime import DfxpContext
from lbt_amd.trainer import Trainer

pytestmark = pytest.mark.gpu
F32 = np.float32
DEV = "cuda"
SUFFIX = {"W": "/W", "b": "/bias"}

# name -> (GPU model, oracle builder, batch, input shape, extra constructor arguments)
CASES = {
    "mnist": (models.MNIST_Model, P.mnist, 4, (28, 28, 1), {}),
    "pi_mnist": (models.PI_MNIST_Model, P.pi_mnist, 8, (784,), {}),
    "cifar10": (models.CIFAR10_Model, P.cifar10, 2, (32, 32, 3), {}),
    "vgg_w16": (models.CIFAR10_VGG_Model, P.cifar10_vgg, 2, (32, 32, 3), dict(width=16, dense_units=64)),
    # 128 -> 256 and 256 -> 256 convs: the LDS-tiled igemm forward / dgrad (and, at 8 bits, the igemm
    # weight gradient on 8-bit gradient codes) in a whole model; vgg_w16 stays on the register kernels
    "vgg_w64": (models.CIFAR10_VGG_Model, P.cifar10_vgg, 2, (32, 32, 3), dict(width=64, dense_units=64)),
}
GRAD_I = -6  # initial */grad_range of the cases away from 8 bits (the default 2 quantises a narrow gradient to zero)


def _pair(case, keep, seed, bits=8):
    gcls, obuild, B, shape, kw = CASES[case]
    ctx = DfxpContext(seed=seed)
    gm = gcls(bits, dropout=keep, weight_decay=2e-4, ctx=ctx, **kw)
    om = obuild(bits, keep, 2e-4, **kw)
    return ctx, gm, om, B, shape


def _batch(B, shape, seed):
    rng = np.random.default_rng(seed)
    x = ((rng.integers(0, 256, size=(B,) + shape) - 127.5) / 128).astype(F32)
    return x, rng.integers(0, 10, size=B).astype(np.int32)


def _by_name(tr, flat):
    """{parameter name: its slice of a Trainer flat buffer (w / a / g)}."""
    return {o.name + SUFFIX[v]: flat[off:off + sz].view(getattr(o, v).shape).cpu().numpy().copy()
            for o, v, off, sz in tr.flat.offsets}


def _state(tr, om, ranges=None):
    p = _by_name(tr, tr.flat.w)
    assert list(p) == [n for n, _ in om.params()]
    return dict(params=p, accum={k: np.zeros_like(v) for k, v in p.items()}, ranges=ranges or P.init_ranges(om),
                step=0)


def _check_step(tr, ctx, gm, om, state, x, y, loss, seed, tag):
    torch.cuda.synchronize()
    dz = gm.dlogits.cpu().numpy()
    lref, state, octx = P.train_step(om, state, x, y, lr=1e-2, momentum=0.9, seed=seed, dz=dz)
    assert abs(loss - lref) <= 1e-5 * abs(lref), (tag, loss, lref)
    np.testing.assert_allclose(dz, octx.dz, rtol=1e-5, atol=1e-9)
    got_g, got_w, got_a = _by_name(tr, tr.flat.g), _by_name(tr, tr.flat.w), _by_name(tr, tr.flat.a)
    for k in got_w:
        assert np.array_equal(got_g[k], octx.grads[k]), (tag, "grad", k)
        assert np.array_equal(got_w[k], state["params"][k]), (tag, "param", k)
        assert np.array_equal(got_a[k], state["accum"][k]), (tag, "momentum", k)
    assert ctx.ranges() == state["ranges"], tag
    assert int(ctx.step.item()) == state["step"]
    _check_step.octx = octx  # the oracle's records of the step just checked
    return state


def _not_vacuous(octx, before, after, tag):
    """A narrow width must not pass by quantising everything to zero (asserted on the oracle alone)."""
    for name, rec in octx.record.items():
        if name.endswith("/grad_range"):
            nz = np.count_nonzero(rec) / rec.size
            assert nz >= 0.01, "%s: %s has %.2f%% non-zero gradient codes" % (tag, name, 100 * nz)
    for k, g in octx.grads.items():
        if k.endswith("/W"):
            assert not np.array_equal(g, (F32(2 * 2e-4) * before["params"][k]).astype(F32)), (tag, k)
    assert any(after["ranges"][k] != before["ranges"][k] for k in after["ranges"]), tag


@pytest.mark.parametrize("case,keep,bits", [
    pytest.param("mnist", 0.5, 8, id="mnist-0.5"), pytest.param("pi_mnist", 0.5, 8, id="pi_mnist-0.5"),
    pytest.param("cifar10", 0.5, 8, id="cifar10-0.5"), pytest.param("vgg_w16", 0.5, 8, id="vgg_w16-0.5"),
    pytest.param("mnist", 0.8, 8, id="mnist-0.8"),
    # away from 8 bits: 6 / 4 bits (signed int8 X codes, generic and igemm kernels, W4 packed weights on
    # the register kernels), 12 / 16 bits (every layer in float mode; the dropout applies its own mask)
    pytest.param("mnist", 0.5, 6, id="mnist-0.5-b6"), pytest.param("pi_mnist", 0.5, 16, id="pi_mnist-0.5-b16"),
    pytest.param("cifar10", 0.5, 4, id="cifar10-0.5-b4"), pytest.param("vgg_w16", 0.5, 12, id="vgg_w16-0.5-b12"),
    pytest.param("vgg_w64", 0.5, 8, id="vgg_w64-0.5"), pytest.param("vgg_w64", 0.5, 6, id="vgg_w64-0.5-b6")])
def test_training_step_equals_oracle(case, keep, bits):
    seed = 6
    ctx, gm, om, B, shape = _pair(case, keep, seed, bits)
    # the default wiring is the fused one (integer layers; a float-mode layer leaves the mask to the dropout)
    assert any(d.fused for d in ctx.dropouts.values()) == (bits <= 8)
    ranges = None
    if bits != 8 or case == "vgg_w64":
        ranges = {r: (GRAD_I if r.endswith("/grad_range") else 2) for r in om.range_names()}
        ctx.set_ranges({r: GRAD_I for r in ranges if r.endswith("/grad_range")})
        assert ctx.ranges() == ranges
    if case == "vgg_w64":
        wide = [l for l in gm.layers if getattr(l, "igemm_f", False)]
        assert [l.name for l in wide] == ["conv3-1", "conv3-2"]
        assert all(l.igemm_d and l.igemm_w == (bits == 8) for l in wide)
    tr = Trainer(gm, lr=1e-2, momentum=0.9, batch_size=B, use_graph=False)
    state = _state(tr, om, ranges)
    # the new cases run two steps: the exponents moved by step 1 feed step 2
    for i in range(1 if ranges is None else 2):
        x, y = _batch(B, shape, seed=1 + i)
        loss = tr.step(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)).item()
        before = state
        state = _check_step(tr, ctx, gm, om, state, x, y, loss, seed, "%s step %d" % (case, i))
        if ranges is not None:
            _not_vacuous(_check_step.octx, before, state, "%s step %d" % (case, i))


def test_mnist_graph_replays_draw_a_new_mask_each_step():
    """Two Trainer.step calls, both replays of the captured step, equal oracle steps 0 and 1: the mask
    is drawn on the device from the step counter, so a replay does not repeat the captured one."""
    seed = 8
    ctx, gm, om, B, shape = _pair("mnist", 0.5, seed)
    tr = Trainer(gm, lr=1e-2, momentum=0.9, batch_size=B, use_graph=True)
    state = _state(tr, om)
    masks = []
    for i in range(2):
        x, y = _batch(B, shape, seed=20 + i)
        loss = tr.step(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)).item()
        assert tr._graphs is not None
        state = _check_step(tr, ctx, gm, om, state, x, y, loss, seed, "replay %d" % i)
        masks.append([l.m.copy() for l in om.layers if isinstance(l, P.DropoutQ)])
    assert all(not np.array_equal(a, b) for a, b in zip(*masks))


def test_testing_mode_forward_is_the_model_without_dropout():
    seed = 3
    ctx, gm, om, B, shape = _pair("mnist", 0.5, seed)
    P.set_params(om, {o.name + SUFFIX[v]: getattr(o, v).cpu().numpy() for o, v, _ in gm.param_slots()})
    x, _ = _batch(B, shape, seed=2)
    xt = torch.from_numpy(x).to(DEV)
    train_logits = gm.forward(xt).cpu().numpy().copy()
    ctx.counts.zero_()
    gm.set_testing()
    logits = gm.forward(xt).cpu().numpy()
    octx = P.nn.Ctx(P.init_ranges(om), 0, seed)
    assert np.array_equal(logits, P.without_dropout(om).forward(x, octx))
    assert not np.array_equal(logits, train_logits)
    gm.set_training()
    assert np.array_equal(gm.forward(xt).cpu().numpy(), om.forward(x, P.nn.Ctx(P.init_ranges(om), 0, seed)))

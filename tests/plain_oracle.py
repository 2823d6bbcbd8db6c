"""Numpy oracle of ``Dropout_q`` and of the reference's four plain models (``models.py:57-368``),
on ``oracle.nn``'s layers (test helper; numpy only).

``DropoutQ`` restates DESIGN section 4's dropout: for the flat index i over the whole tensor,
``u_i`` = the Philox stream's i-th value of stream ``qid_of(name)`` at (step, seed),
``m_i = fl32(k + u_i) >= 1``, ``y_i = fl32(x_i / k) * m_i`` and ``dx_i = fl32(g_i / k) * m_i``
with ``k = float32(keep_prob)``.
"""
import numpy as np

from oracle import dfxp, nn
from oracle.nn import F32
from oracle.philox import philox4x32_10, uniform_noise
from oracle.resnet import sgd_momentum


def dropout_mask(n, name, step, seed, keep):
    """The n mask bits (bool) of the dropout layer `name` at (step, seed)."""
    u = uniform_noise(n, dfxp.qid_of(name), step, seed)
    return (F32(keep) + u).astype(F32) >= F32(1.0)


def dropout_mask_at(idx, name, step, seed, keep):
    """The mask bits of the elements with flat indices idx (any, < 2^34): the same stream as
    dropout_mask, evaluated at those counters only."""
    idx = np.asarray(idx, np.uint64)
    n = idx.size
    full = lambda v: np.full(n, v & 0xFFFFFFFF, np.uint32)  # noqa: E731
    r = philox4x32_10((idx >> np.uint64(2)).astype(np.uint32), full(dfxp.qid_of(name)), full(step), full(step >> 32),
                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    word = np.stack(r, axis=1)[np.arange(n), (idx & np.uint64(3)).astype(np.int64)]
    u = ((word >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)).astype(F32)
    return (F32(keep) + u).astype(F32) >= F32(1.0)


class DropoutQ(nn.LayerQ):
    def __init__(self, name, keep_prob, train=True):
        self.name, self.keep, self.train = name, keep_prob, train

    def _active(self):
        return self.train and self.keep < 1

    def forward(self, X, ctx):
        if not self._active():
            return X
        self.m = dropout_mask(X.size, self.name, ctx.step, ctx.seed, self.keep).reshape(X.shape).astype(F32)
        return ((np.asarray(X, F32) / F32(self.keep)).astype(F32) * self.m).astype(F32)

    def backward(self, g, ctx):
        if not self._active():
            return g
        return ((np.asarray(g, F32) / F32(self.keep)).astype(F32) * self.m.reshape(g.shape)).astype(F32)


class _Builder:
    """Layer constructors with the models' shared arguments; dropouts named in construction order."""

    def __init__(self, bits, keep, wd):
        self.bits, self.keep, self.wd, self.ndrop = bits, keep, wd, 0

    def conv(self, name, ksize, padding):
        return nn.Conv2dQ(name, self.bits, ksize, [1, 1, 1, 1], padding, self.wd, use_bias=True)

    def dense(self, name, i, o):
        return nn.DenseQ(name, self.bits, i, o, self.wd, use_bias=True)

    def drop(self):
        self.ndrop += 1
        return DropoutQ("dropout%d" % self.ndrop, self.keep)

    @staticmethod
    def pool(k, padding):
        return nn.MaxPoolQ([1, k, k, 1], [1, 2, 2, 1], padding)


def pi_mnist(bits=8, keep=0.5, wd=0.0):
    b = _Builder(bits, keep, wd)
    return nn.SequentialQ(b.dense("dense1", 784, 1024), nn.ReluQ(), b.drop(),
                          b.dense("dense2", 1024, 1024), nn.ReluQ(), b.drop(),
                          b.dense("softmax", 1024, 10))


def mnist(bits=8, keep=0.5, wd=0.0):
    b = _Builder(bits, keep, wd)
    return nn.SequentialQ(b.conv("conv1", [5, 5, 1, 6], "SAME"), nn.ReluQ(), b.pool(2, "VALID"),
                          b.conv("conv2", [5, 5, 6, 16], "VALID"), nn.ReluQ(), b.pool(2, "VALID"),
                          b.conv("conv3", [5, 5, 16, 120], "VALID"), nn.ReluQ(), nn.FlattenQ(120), b.drop(),
                          b.dense("dense1", 120, 84), nn.ReluQ(), b.drop(),
                          b.dense("softmax", 84, 10))


def cifar10(bits=8, keep=0.5, wd=0.0):
    b = _Builder(bits, keep, wd)
    return nn.SequentialQ(b.conv("conv1", [5, 5, 3, 64], "SAME"), nn.ReluQ(), b.pool(3, "SAME"),
                          b.drop(), b.conv("conv2", [5, 5, 64, 128], "SAME"), nn.ReluQ(), b.pool(3, "SAME"),
                          b.drop(), b.conv("conv3", [5, 5, 128, 128], "SAME"), nn.ReluQ(), b.pool(3, "SAME"),
                          nn.FlattenQ(128 * 4 * 4),
                          b.drop(), b.dense("dense1", 128 * 4 * 4, 400), nn.ReluQ(),
                          b.drop(), b.dense("softmax", 400, 10))


def cifar10_vgg(bits=8, keep=0.5, wd=0.0, width=128, dense_units=1024):
    b, w, u = _Builder(bits, keep, wd), width, dense_units
    return nn.SequentialQ(b.conv("conv1-1", [3, 3, 3, w], "SAME"), nn.ReluQ(),
                          b.conv("conv1-2", [3, 3, w, w], "SAME"), nn.ReluQ(), b.pool(3, "SAME"),
                          b.drop(), b.conv("conv2-1", [3, 3, w, 2 * w], "SAME"), nn.ReluQ(),
                          b.conv("conv2-2", [3, 3, 2 * w, 2 * w], "SAME"), nn.ReluQ(), b.pool(3, "SAME"),
                          b.drop(), b.conv("conv3-1", [3, 3, 2 * w, 4 * w], "SAME"), nn.ReluQ(),
                          b.conv("conv3-2", [3, 3, 4 * w, 4 * w], "SAME"), nn.ReluQ(), b.pool(3, "SAME"),
                          nn.FlattenQ(4 * w * 4 * 4),
                          b.drop(), b.dense("dense1", 4 * w * 4 * 4, u), nn.ReluQ(),
                          b.drop(), b.dense("dense2", u, u), nn.ReluQ(),
                          b.drop(), b.dense("softmax", u, 10))


def without_dropout(model):
    """The same layers (shared objects) with the dropout layers removed: the testing-mode model."""
    return nn.SequentialQ(*[l for l in model.layers if not isinstance(l, DropoutQ)])


# ---- parameters and gradients by name ("<layer>/W", "<layer>/bias": nn.*Q.params()) -------------
def _attr(name, grad):
    if name.endswith("/W"):
        return "dW" if grad else "W"
    if name.endswith("/bias"):
        return "db" if grad else "b"
    raise KeyError(name)


def get_params(model):
    return {name: getattr(owner, _attr(name, False)) for name, owner in model.params()}


def set_params(model, params):
    for name, owner in model.params():
        setattr(owner, _attr(name, False), np.asarray(params[name], F32).copy())


def get_grads(model):
    return {name: getattr(owner, _attr(name, True)) for name, owner in model.params()}


def init_ranges(model, initial=2):
    return {r: initial for r in model.range_names()}


def train_step(model, state, x, labels, lr=1e-2, momentum=0.9, seed=0, dz=None):
    """One training step (oracle.resnet.train_step's contract) on a plain model. state =
    dict(params, accum, ranges, step); dz: d loss / d logits to back-propagate in place of the
    oracle's own (the softmax is the one op of the step that is not bit-exact).
    Returns (loss, new_state, ctx); ctx.logits / ctx.dz hold the oracle's own."""
    set_params(model, state["params"])
    ctx = nn.Ctx(state["ranges"], state["step"], seed)
    logits = model.forward(np.asarray(x, F32), ctx)
    loss, dz_own = nn.softmax_xent(logits, np.asarray(labels))
    model.backward(dz_own if dz is None else np.asarray(dz, F32), ctx)
    ctx.logits, ctx.dz, ctx.grads = logits, dz_own, get_grads(model)
    params, accum = sgd_momentum(state["params"], ctx.grads, state["accum"], lr, momentum)
    return loss, dict(params=params, accum=accum, ranges=ctx.new_ranges(), step=state["step"] + 1), ctx

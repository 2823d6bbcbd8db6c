"""Numpy oracle of the data-parallel step of the plain models with ``Dropout_q`` (test helper; numpy
only, on ``plain_oracle`` and ``oracle.nn``).

A rank's shard of a dropout input has n = b * inner elements; local element i takes the mask bit of
element ``rank * n + i`` of the global [N*b, ...] tensor, so the shards of a batch
draw what one process draws on the whole batch. ``dp_train_step`` has the shape of
``oracle.resnet.dp_train_step``: per-shard forward and backward with the loss normalised by the global
batch, the integer numerators of every weight and bias gradient and the overflow counts summed over
the shards, dequantised once, then one SGD-momentum step and one range update.
"""
import numpy as np

import plain_oracle as P
from oracle import dfxp, nn
from oracle.nn import F32
from oracle.resnet import sgd_momentum


class DropoutQ(P.DropoutQ):
    """plain_oracle.DropoutQ on a window of the mask stream: ``offset`` is the global index of local
    element 0 (``None``: ``rank * X.size``, the shard of an equal split). Rank 0 is plain_oracle's."""

    def __init__(self, name, keep_prob, train=True):
        super().__init__(name, keep_prob, train)
        self.rank, self.offset = 0, None

    def forward(self, X, ctx):
        if not self._active():
            return X
        base = self.rank * X.size if self.offset is None else self.offset
        idx = np.uint64(base) + np.arange(X.size, dtype=np.uint64)
        self.m = P.dropout_mask_at(idx, self.name, ctx.step, ctx.seed, self.keep).reshape(X.shape).astype(F32)
        return ((np.asarray(X, F32) / F32(self.keep)).astype(F32) * self.m).astype(F32)


def shardable(model):
    """The same model with every plain_oracle.DropoutQ replaced by this module's (same names, keeps)."""
    return nn.SequentialQ(*[DropoutQ(l.name, l.keep, l.train) if isinstance(l, P.DropoutQ) else l
                            for l in model.layers])


def dropouts(model):
    return [l for l in model.layers if isinstance(l, DropoutQ)]


def _numerators(model):
    """{param name: (kind, int64 numerator, exponent, owner)} of the last backward."""
    out = {}
    for l in model.layers:
        if isinstance(l, (nn.Conv2dQ, nn.DenseQ)):
            out[l.name + "/W"] = ("w", l.acc_w, l.ew_grad, l)
            if l.use_bias:
                out[l.name + "/bias"] = ("b", l.db_int, l.ew_grad - l.ex, l)  # e_g
    return out


def dp_train_step(model, state, shards, lr=1e-2, momentum=0.9, seed=0, dzs=None, global_masks=True):
    """One data-parallel step over batch shards [(x_r, labels_r)] of equal size. dzs: per-shard injected
    d loss / d logits. global_masks=False: every shard at offset 0 (what ranks that do not know their
    position would draw). Returns (global loss, new_state, ctxs); ctxs[r].masks holds shard r's masks
    by dropout name, ctxs[r].dz the oracle's own rows of the global softmax gradient."""
    B = sum(len(y) for _, y in shards)
    num, counts, loss, ctxs = None, {}, 0.0, []
    for r, (x, y) in enumerate(shards):
        P.set_params(model, state["params"])
        for d in dropouts(model):
            d.rank, d.offset = (r, None) if global_masks else (0, 0)
        ctx = nn.Ctx(state["ranges"], state["step"], seed)
        logits = model.forward(np.asarray(x, F32), ctx)
        l, dz_own = nn.softmax_xent(logits, np.asarray(y), B)
        model.backward(dz_own if dzs is None else np.asarray(dzs[r], F32), ctx)
        ctx.logits, ctx.dz = logits, dz_own
        ctx.masks = {d.name: d.m.copy() for d in dropouts(model) if d._active()}
        loss += l
        ctxs.append(ctx)
        nr = _numerators(model)
        if num is None:
            num = {k: [kind, np.asarray(v, np.int64).copy(), e, owner] for k, (kind, v, e, owner) in nr.items()}
        else:
            for k, (_, v, e, _) in nr.items():
                assert e == num[k][2], k  # one set of exponents on every shard
                num[k][1] = num[k][1] + np.asarray(v, np.int64)
        for name, (c1, c2, n, bits) in ctx.counts.items():
            a = counts.get(name, (0, 0, 0, bits))
            counts[name] = (a[0] + c1, a[1] + c2, a[2] + n, bits)
    for d in dropouts(model):
        d.rank, d.offset = 0, None
    grads = {}
    for k, (kind, S, e, owner) in num.items():
        if kind == "w":
            grads[k] = (nn.scale_int(S, e) + (F32(2 * owner.wd) * owner.W).astype(F32)).astype(F32)
        else:  # nn._bias_bwd's formula on the summed integer
            grads[k] = (S.astype(np.float64) * 2.0 ** -e).astype(F32)
    params, accum = sgd_momentum(state["params"], grads, state["accum"], lr, momentum)
    ranges = dict(state["ranges"])
    for name, (c1, c2, n, bits) in counts.items():
        ranges[name] = dfxp.update_range_from_counts(c1, c2, n, 0.0, bits, state["ranges"][name])
    return loss, dict(params=params, accum=accum, ranges=ranges, step=state["step"] + 1), ctxs

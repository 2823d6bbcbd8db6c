"""Data-parallel exchange of the DFXP training step (torch.distributed: RCCL on MI355X, gloo on CPU).

The reference is single-process (trainer.py:69-71). The build shards the batch over ranks (one
process per GPU) and adds ONE collective per step. For the fused plans (the bench path) it is an
all-reduce SUM of the int64 exchange buffer

    [ every gradient element's integer numerator (272 464 for ResNet-20) | overflow counters
      (2 per quantiser) | loss-term sum in 2^-32 fixed point ]

written by lbt_step_reduce_x at the end of the backward: the weight gradient of :302 is
dequant(sum_pixels Xq * Gq) + 2*wd*W, so summing the integer sums over ranks and dequantising once
(lbt_step_finish) is EXACT -- the quantised-gradient exchange of SURVEY 8(e) -- and independent of
the order RCCL adds in. (2.2 MB; latency-bound on xGMI, one flat bucket.)

Layer-wise models whose trainable variables are all integer-coded (quantised conv / dense W, BN
gamma / beta: exact_layerwise_ok -- the ResNet-50 of configs[3]) use the SAME int64 exchange: while
the Trainer runs their forward / backward, ops.set_exchange_sink points every gradient reduction
(lbt_conv_wgrad_reduce(64)_x, lbt_dense_wgrad_x, lbt_bn_param_grads_x) at the gradient's slots of the
buffer, the softmax (lbt_softmax_xent_n) normalises by the global batch and leaves its loss sum in the
loss slot, and lbt_step_reduce_x's fold blocks add the counters: an N-rank step equals the oracle's
N-shard step bit for bit (tests/test_dp_resnet50_gpu.py).

A context that declares its rank (DfxpContext(world_size=N, rank=r)) extends this to the biased plain
models with Dropout_q: a bias gradient travels as its numerator too (lbt_bias_grad_x, an lbt_fseg of kind
2), and inside the training step each dropout layer draws the mask bits of its shard's elements of the
GLOBAL tensor (base = rank * n: lbt_dropout_*_at), so the N-rank step equals the one-process step on the
whole batch bit for bit (tests/test_dp_dropout_gpu.py).

The BatchNorm statistics of such a model stay per rank unless sync_batchnorm(model) switches them to the
global batch's: every Normalization_q then folds its exact int64 channel sums (forward) and pass-A sums
(backward) to their totals (lbt_sums_fold) and all-reduces those 2C / 4C integers before the kernel that
consumes them, and the N-rank step equals the ONE-process step on the whole batch bit for bit
(tests/test_syncbn_layerwise_dp_gpu.py).

Other layer-wise models (fp32-mode layers; biases without a declared rank) exchange dequantised
gradients instead, an all-reduce SUM of

    [ flat fp32 gradients | every quantiser's folded overflow counters ]

The gradient buffer IS the head of the comm buffer (the backward writes into it), and the counter
fold kernel (lbt_dfxp_counts_fold) writes each slot's totals into the tail as exact fp32 pairs
(c >> 12, c & 4095: every partial sum of the all-reduce stays below 2**24), so the exchange is one
in-place RCCL call on ~1.1 MB -- latency-bound on xGMI, so a single flat bucket beats bucketing. After it,
every rank applies the same averaged update (SGD gscale = 1/world) and the same range update
(nelem = per-rank elements x world), i.e. the DFXP exponents stay identical on all ranks without
any extra synchronisation. The rounding-noise key (seed, step, quantiser) does not involve the
rank, so activation noise (shape X.shape[1:]) is what a single process would draw.
"""
import torch
import torch.distributed as dist

FOLD = 4  # floats per quantiser slot in the comm buffer tail


def make_comm_buffer(n_grads, n_slots, device):
    """[grads | FOLD floats per quantiser slot] fp32."""
    return torch.zeros(n_grads + FOLD * n_slots, dtype=torch.float32, device=device)


def fold_host(c):
    """Host twin of lbt_dfxp_counts_fold's packing: int [slots, 2] -> fp32 [slots*4]."""
    c = torch.as_tensor(c, dtype=torch.int64).view(-1, 2)
    return torch.stack([c[:, 0] >> 12, c[:, 0] & 4095, c[:, 1] >> 12, c[:, 1] & 4095], 1).float().view(-1)


def unfold_host(f):
    """fp32 [slots*4] -> int64 [slots, 2] (what lbt_dfxp_range_update_folded decodes)."""
    f = f.view(-1, 4).to(torch.int64)
    return torch.stack([f[:, 0] * 4096 + f[:, 1], f[:, 2] * 4096 + f[:, 3]], 1)


def make_exchange(n_grads, n_slots, device):
    """The int64 exchange buffer [numerators | 2 counters per slot | loss] and its lbt_xchg
    descriptor (buf, cnt_off, loss_off, nslots set; the caller sets gbase / counts / pjob_scale)."""
    from . import _lib
    buf = torch.zeros(n_grads + 2 * n_slots + 1, dtype=torch.int64, device=device)
    x = _lib.Xchg()
    x.buf = buf.data_ptr()
    x.nslots = n_slots
    x.cnt_off = n_grads
    x.loss_off = n_grads + 2 * n_slots
    x.pjob_scale = 1
    return buf, x


def finish_segments(flat, device):
    """lbt_fseg per parameter tensor of a FlatParams (kind 0 conv / dense W, 1 gamma, 2 beta / bias) as a
    device array (raw bytes), and the finish kernel's block count."""
    from . import _lib
    from .dfxp import ops
    segs, blocks = [], 0
    for owner, var, off, sz in flat.offsets:
        if var == "W":
            kind, qx, qg = 0, owner.X_range.desc, owner.grad_range.desc
        elif var == "gamma":
            kind, qx, qg = 1, owner.X_range.desc, owner.grad_range.desc
        elif var in ("beta", "b"):  # a Conv2d_q / Dense_q bias: lbt_bias_grad's formula is beta's
            kind, qx, qg = 2, owner.X_range.desc, owner.grad_range.desc
        else:
            raise NotImplementedError("exact exchange of parameter %r" % var)
        segs.append(_lib.FSeg(off, sz, kind, qx, qg, ops.f32(2 * owner.weight_decay)))
        blocks += (sz + 255) // 256
    raw = bytes((_lib.FSeg * len(segs))(*segs))
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device), blocks


def exact_layerwise_ok(model, biases=False):
    """True when every trainable variable of a layer-wise model gets an INTEGER gradient numerator
    (quantised conv / dense W, BN gamma / beta; no fp32-mode layer, no bias): the models the exact
    int64 exchange (ops.set_exchange_sink) takes. biases=True also accepts Conv2d_q / Dense_q biases
    (lbt_bias_grad_x): what the Trainer asks when the context declares its rank."""
    return float_mode_layer(model, biases) is None


def float_mode_layer(model, biases=True):
    """The first parameter owner the exact exchange cannot take (a float-mode layer, a variable that is
    none of W / gamma / beta / -- with biases -- b), or None."""
    ok = ("W", "gamma", "beta") + (("b",) if biases else ())
    for owner, var, _ in model.param_slots():
        if var not in ok or getattr(owner, "fmode", False):
            return owner
    return None


def sync_batchnorm(model, process_group=None, force=False):
    """SyncBN for a layer-wise model: every Normalization_q takes the moments of the GLOBAL batch.

    Sets ``sync = (process_group, world)`` on every Normalization_q of ``model`` (Model._walk) and
    ``model.sync_bn = True``; returns ``model``. While such a layer trains, the exact int64 channel sums
    behind its moments and the exact int64 pass-A sums behind its input gradient are folded to their totals
    (lbt_sums_fold) and summed over the ranks (one all-reduce of 2C, one of 4C int64 per layer and step)
    before the kernel that consumes them -- so with the exact int64 exchange the same script on N ranks
    leaves the parameters, momentum, exponents and BN running statistics of one process on the whole
    batch, bit for bit. ``world`` is the group's size. At world 1 this is a no-op that leaves
    ``model.sync_bn`` False, unless ``force`` keeps the folds and collectives (tests of the path: a sum over
    one rank is the identity; without a process group only the folds run).

    Refused before anything is launched: a FusedResNet (TypeError: it has ``sync_bn=`` of its own), a
    float-mode Normalization_q (NotImplementedError: its statistics are fp32 partials, not integers),
    world > 1 without an initialised process group (RuntimeError), a model that already ran a forward
    (RuntimeError: captured graphs and warmed-up buffers would not hold the collectives)."""
    from .dfxp.layers import Normalization_q
    if hasattr(model, "set_exchange") or not hasattr(model, "_walk"):
        raise TypeError("sync_batchnorm takes a layer-wise Model; %s has sync_bn= of its own"
                        % type(model).__name__)
    norms = [l for l in model._walk() if isinstance(l, Normalization_q)]
    for n in norms:
        if n.fmode:
            raise NotImplementedError("SyncBN of the float-mode layer %r: its statistics are fp32 partial sums, "
                                      "not integers (bits <= 8 and grad_bits <= 16 run on integer sums)" % n.name)
    ready = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(process_group) if ready else 1
    if not ready and model.ctx.world_size > 1:
        raise RuntimeError("sync_batchnorm at world %d needs an initialised process group "
                           "(torch.distributed.init_process_group)" % model.ctx.world_size)
    if getattr(model, "logits", None) is not None or any(hasattr(n, "q") for n in norms):
        raise RuntimeError("sync_batchnorm after the model ran a forward: switch it before the first step")
    if world == 1 and not force:
        return model
    for n in norms:
        n.sync = (process_group, world)
    model.sync_bn = True
    return model


def allreduce_comm(comm, group=None):
    """The step's only collective: in-place SUM of [grads | folded counters] over the ranks."""
    dist.all_reduce(comm, op=dist.ReduceOp.SUM, group=group)

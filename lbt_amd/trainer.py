"""The timed training step of the reference (``trainer.py:109-162``) on the HIP path.

One ``Trainer.step(X, y)`` = ``sess.run([train_op, update_range_op])`` of ``trainer.py:157``:
forward, loss, manual backward, ``MomentumOptimizer.apply_gradients`` (``acc = mu*acc + g;
w -= lr*acc``, ``trainer.py:79-84``) and the ``'update_range'`` collection.

MI355X-native execution:
* all trainable variables live in ONE flat fp32 buffer (and their gradients / momentum in two
  more), so the optimiser is a single kernel and the data-parallel exchange is one all-reduce;
* after a warm-up step the whole step is captured into a HIP graph (``torch.cuda.CUDAGraph``)
  and replayed: ~300 kernel launches become one graph launch;
* data parallelism (``torch.distributed``, backend ``nccl`` = RCCL over xGMI): each rank runs
  the step on its own batch shard, with the loss a mean over the GLOBAL batch; between the
  backward graph and the update graph ONE all-reduce sums the step's gradients and the
  quantisers' overflow counters, so every rank applies identical updates and identical DFXP
  exponents. Noise keys (seed, step, quantiser) do not depend on the rank.
  - fused plans (FusedResNet): the gradients travel as their exact int64 numerators (the
    quantised-gradient exchange, lbt_step_reduce_x -> all-reduce -> lbt_step_finish): exact and
    order-independent, so the update is the single-process formula applied to the global sums;
    with ``FusedResNet(sync_bn=True)`` (global BatchNorm statistics) a step on N ranks of b
    samples is bit-identical to one process on the N*b batch.
  - layer-wise models: dequantised fp32 gradients + counters folded into exact fp32 pairs, one
    fp32 all-reduce (gscale = 1/world).
  - layer-wise models with ``lbt_amd.distributed.sync_batchnorm(model)``: every Normalization_q sums its
    exact integer statistics over the ranks (lbt_sums_fold + one small all-reduce, forward and backward), so
    on the exact int64 exchange -- required: the fp32 one is refused -- N ranks on the shards equal one
    process on the whole batch bit for bit. Those collectives sit inside the step: captured with it under
    RCCL, eager steps under gloo; ``evaluate()`` suspends them (every rank holds each test batch whole).
  - ``DfxpContext(world_size=N, rank=r)``: the plain models with ``Dropout_q`` train data-parallel on
    the exact int64 exchange (bias numerators included), each rank drawing its shard's bits of the
    global batch's dropout mask: N ranks on the shards equal one process on the whole batch.
* data-parallel epochs: under a process group ``train()`` shards every global batch of the epoch by rows
  (``shard_rows``; rank 0's permutation broadcast once per epoch; each row augmented with its draw of the global
  batch, ``lbt_batch_gather``'s / ``lbt_augment_flip_crop_at``'s ``base``), and ``evaluate()`` splits each test batch
  where that is exact -- a SyncBN-trained FusedResNet, or its inference plans -- summing ``lbt_eval_tally``'s
  integer rows with one all-reduce (``_evaluate_sharded``); elsewhere every rank runs the whole test loop. The
  same script on N ranks then leaves one process's parameters, exponents and BN statistics bit for bit. Not
  timed at N > 1 on hardware.
* the reference's training summaries (``trainer.py:148-155``: every layer's ``tf.summary.scalar``s with loss
  and accuracy, every 100th batch) are recorded on the device: ``Trainer(summary_every=K)`` replays, on every
  K-th step, a second captured graph of the step with ``lbt_summary_record`` between the backward and the
  update -- which zeroes the overflow counters that drove its range decisions -- and ``lbt_summary_commit``
  after it (``lbt_amd/summary.py``). Every other step replays the graph it replays without summaries.
"""
import contextlib
import os
import sys

import torch
import torch.distributed as dist

from . import _lib
from . import distributed as D
from .data import DEVICE_DATASETS
from .dfxp import ops


def shard_rows(nb, world, rank):
    """Rows [lo, hi) of a global batch of nb rows that rank ``rank`` of ``world`` takes: ``world`` equal
    shards in rank order, rank r rows [r * nb / world, (r + 1) * nb / world). ValueError when nb does
    not split evenly (uneven shards are not built)."""
    nb, world, rank = int(nb), int(world), int(rank)
    if world < 1 or not 0 <= rank < world:
        raise ValueError("rank %d is outside a world of %d" % (rank, world))
    if nb < 0 or nb % world:
        raise ValueError("a batch of %d rows does not split into %d equal shards" % (nb, world))
    s = nb // world
    return rank * s, (rank + 1) * s


def epoch_batch_sizes(n, batch_size):
    """Every batch size an epoch over n samples produces: batch_size (when a full batch fits) and the
    final partial batch n % batch_size (trainer.py:98), in that order."""
    n, batch_size = int(n), int(batch_size)
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1, got %d" % batch_size)
    return ([batch_size] if n >= batch_size else []) + ([n % batch_size] if n % batch_size else [])


def check_epoch_shards(n, batch_size, world):
    """The up-front check of a data-parallel epoch: every batch size it will produce splits into ``world``
    equal shards, or ValueError naming all three."""
    bad = [nb for nb in epoch_batch_sizes(n, batch_size) if nb % int(world)]
    if bad:
        raise ValueError("n = %d samples at batch_size = %d give a batch of %d rows, which does not split into "
                         "world = %d equal shards (batch_size is the GLOBAL batch; batch_size and n %% batch_size "
                         "must both be divisible by world)" % (n, batch_size, bad[0], world))


def decode_tally(rows, sizes):
    """(mean accuracy, mean loss) over the test batches from their lbt_eval_tally rows summed over the ranks:
    rows[i] = (correct predictions, loss-term sum in 2^-32 fixed point) of batch i, sizes[i] its rows.
    Per batch the accuracy is float32(correct) / float32(nb) -- what mean() of the 0 / 1 floats gives -- and
    the loss float32(sum * 2^-32 / nb) computed in double (lbt_step_finish's rounding); the fp32 values are
    added in double in batch order and divided by the number of batches, as the test loops do."""
    import numpy as np
    if len(rows) != len(sizes):
        raise ValueError("%d tally rows for %d batches" % (len(rows), len(sizes)))
    acc_sum = loss_sum = 0.0
    for (correct, loss_fx), nb in zip(rows, sizes):
        acc_sum += float(np.float32(int(correct)) / np.float32(int(nb)))
        loss_sum += float(np.float32(float(int(loss_fx)) * 2.0 ** -32 / float(int(nb))))
    return acc_sum / max(len(sizes), 1), loss_sum / max(len(sizes), 1)


class FlatParams:
    """Bind every (var, grad) of a model into contiguous flat buffers (grads_and_vars order)."""

    def __init__(self, model, grad_buffer=None):
        slots = model.param_slots()
        dev = model.ctx.device
        sizes = [getattr(o, v).numel() for o, v, _ in slots]
        n = sum(sizes)
        self.n = n
        self.w = torch.zeros(n, dtype=torch.float32, device=dev)
        self.g = grad_buffer[:n] if grad_buffer is not None else torch.zeros(n, dtype=torch.float32, device=dev)
        self.a = torch.zeros(n, dtype=torch.float32, device=dev)
        off = 0
        self.offsets = []
        for (o, v, gname), sz in zip(slots, sizes):
            t = getattr(o, v)
            wv = self.w[off:off + sz].view(t.shape)
            wv.copy_(t)
            setattr(o, v, wv)
            setattr(o, gname, self.g[off:off + sz].view(t.shape))
            self.offsets.append((o, v, off, sz))
            off += sz


class Trainer:
    def __init__(self, model, dataset=None, logger=None, logdir=None, lr=1e-2, lr_decay_factor=0.5,
                 lr_decay_epoch=50, momentum=0.95, n_epoch=5, batch_size=128, use_graph=True,
                 process_group=None, exchange=None, capture_comm=None, summary_every=0, summary_capacity=1024):
        """summary_every = K > 0: the K-th, 2K-th, ... steps of this trainer (counted from 1) record the
        reference's training summaries on the device (lbt_amd/summary.py; read them with summaries()):
        those steps replay a second captured graph of the same step with lbt_summary_record between the
        backward and the update and lbt_summary_commit after it; every other step replays the graph it
        replays without summaries. summary_capacity: records the device ring holds between two reads.
        0: off, nothing changes anywhere.
        batch_size: the reference's (trainer.py:34) -- under a process group the GLOBAL batch of train(), which
        every rank takes an equal shard of (step() itself takes whatever shard it is handed).
        exchange: run the data-parallel exchange (default: when the process group has > 1 rank;
        True at world 1 exercises the same path -- an all-reduce over one rank is the identity).
        capture_comm: put the step's collectives (the exchange, SyncBN's statistics) INSIDE the
        captured HIP graph, so a step is one graph launch (default: on for the nccl = RCCL backend,
        LBT_CAPTURE_COMM=0 turns it off; gloo collectives cannot be captured and run from the host
        between graph segments / eagerly)."""
        self.model = model
        self.dataset = dataset
        self.logger = logger
        self.lr, self.momentum = lr, momentum
        self.lr_decay_factor, self.lr_decay_epoch = lr_decay_factor, lr_decay_epoch
        self.n_epoch, self.batch_size = n_epoch, batch_size
        self.use_graph = use_graph
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        self.ctx = model.ctx
        if self.world != self.ctx.world_size:
            raise ValueError("DfxpContext.world_size (%d) must equal the process-group size (%d)"
                             % (self.ctx.world_size, self.world))
        # data-parallel exchange: int64 [numerators | counters | loss] (fused plans) or fp32
        # [grads | folded overflow counters] (layer-wise models) -> ONE in-place all-reduce per step
        self.comm = self.xbuf = None
        dist_on = dist.is_available() and dist.is_initialized()
        self.dp = (self.world > 1) if exchange is None else (bool(exchange) and dist_on)
        if capture_comm is None:
            capture_comm = (dist_on and dist.get_backend(process_group) == "nccl"
                            and os.environ.get("LBT_CAPTURE_COMM", "1") == "1")
        self.capture_comm = bool(capture_comm) and dist_on
        # the epoch loops under a process group of several ranks: each rank takes its shard of every global
        # batch (train) and, where that is exact, of every test batch (evaluate)
        self.rank = dist.get_rank(process_group) if dist_on else 0
        self._shard = self.dp and self.world > 1
        self.summary_every = int(summary_every)
        if self.summary_every < 0:
            raise ValueError("summary_every must be >= 0, got %r" % (summary_every,))
        if self.dp and self.summary_every > 0:
            raise NotImplementedError("summaries of a data-parallel trainer: the overflow counters are summed "
                                      "across ranks inside the exchange, so no rank holds the step's totals "
                                      "where lbt_summary_record reads them (summary_every must be 0)")
        # a context that declares its rank: shard-aware dropout masks and the exact exchange with biases
        ranked = self.ctx.rank is not None
        if ranked and dist_on and self.ctx.rank != dist.get_rank(process_group):
            raise ValueError("DfxpContext.rank (%d) must equal this process's rank in the group (%d)"
                             % (self.ctx.rank, dist.get_rank(process_group)))
        if self.dp and self._has_dropout(model):
            if not ranked:
                # every rank would draw the same mask (the noise keys do not depend on the rank): the
                # shards of one global batch need the context to say where its shard sits
                raise NotImplementedError("data-parallel training of a model with Dropout_q layers needs the "
                                          "shard position: DfxpContext(world_size=N, rank=r)")
            bad = D.float_mode_layer(model) if not hasattr(model, "set_exchange") else None
            if bad is not None:
                # bit-equality with the one-process step rests on integer numerators
                raise NotImplementedError("data-parallel training of a model with Dropout_q layers takes "
                                          "integer-coded layers only: %r is a float-mode layer (its gradients "
                                          "are no integer numerators)" % getattr(bad, "name", bad))
        exact = self.dp and hasattr(model, "set_exchange")
        # layer-wise models (ResNet-50, configs[3]): the same exact int64 exchange when every gradient
        # is an integer numerator (integer-coded W / gamma / beta, and with a declared rank biases;
        # LBT_EXACT_LAYERWISE=0: fp32 -- not with Dropout_q, whose guarantee is the exact exchange's)
        self._lw_exact = (self.dp and not exact and D.exact_layerwise_ok(model, biases=ranked)
                          and (os.environ.get("LBT_EXACT_LAYERWISE", "1") == "1"
                               or (ranked and self._has_dropout(model))))
        if self.dp and not exact and not self._lw_exact and getattr(model, "sync_bn", False):
            # global BN statistics promise one process's bits: dequantised fp32 gradients summed in the
            # collective's order cannot keep that promise
            raise NotImplementedError("a layer-wise model with sync_batchnorm trains data-parallel on the exact "
                                      "int64 exchange only (integer-coded parameters, no bias without a declared "
                                      "rank, LBT_EXACT_LAYERWISE not 0): the fp32 exchange cannot give SyncBN's "
                                      "bit-for-bit guarantee")
        if self.dp and not exact and not self._lw_exact:
            n = sum(getattr(o, v).numel() for o, v, _ in model.param_slots())
            self.comm = D.make_comm_buffer(n, len(self.ctx.quantizers), self.ctx.device)
        self.flat = FlatParams(model, self.comm)
        self._loss_n = 0
        if exact:
            self._setup_exchange()
        elif self._lw_exact:
            self._setup_exchange_layerwise()
        self.ctx.sums_managed = True
        # single process, fused plan: the optimiser + range update run inside the step's last launch
        # (FusedResNet.set_optimizer / lbt_step_reduce_update) instead of one more launch after it
        self._fused_update = hasattr(model, "set_optimizer") and not self.dp
        self._sync_optimizer()
        self.global_step = 0
        self._gflag = {}  # recording? -> captured graphs on the static inputs (models that bind none)
        self._graphs = None
        self._static = None
        self._gcache = {}  # (X ptr, y ptr, shape, recording?) -> captured graphs (models that bind inputs)
        # summaries: one ring / cursor for every plan, one lbt_summary per plan (its own logits, loss, labels)
        self.logdir = logdir
        self._sring = None
        self._sdesc = {}
        if self.summary_every > 0:
            from .summary import SummaryRing
            self._sring = SummaryRing(self.ctx, self.flat, summary_capacity)
        self._eval = {}
        self._plans = {}
        self._active = model
        self._aug = None
        self._inbuf = {}  # (batch size, sample shape) -> the (X, y) pair a DeviceDataset's batches are gathered into
        self._perm = None  # the epoch's permutation on the device (int32)
        if logger is not None:
            logger.info("Model info:\n" + model.info())

    @property
    def _graphs(self):
        """The graphs of the last captured or replayed step; None forgets every graph on the static inputs."""
        return self._glast

    @_graphs.setter
    def _graphs(self, g):
        self._glast = g
        if g is None:
            self._gflag = {}

    # -- summaries ---------------------------------------------------------------------------
    def _records(self):
        """Whether the step about to run records: the K-th, 2K-th, ... of this trainer, decided on the host."""
        return self.summary_every > 0 and (self.global_step + 1) % self.summary_every == 0

    def _summary(self, m):
        """Plan / model m's lbt_summary (the shared sink and sources; m's own pointers are set per step)."""
        s = self._sdesc.get(id(m))
        if s is None:
            s = self._sdesc[id(m)] = (m, self._sring.desc())
        return s[1]

    def _summary_call(self, name, m, y=None):
        """lbt_summary_record / _commit of a layer-wise model around Trainer._update: its logits, loss and
        the step's labels as they lie after the forward + backward (fixed buffers once warmed up)."""
        s = self._summary(m)
        if y is not None:
            s.logits, s.loss, s.labels = m.logits.data_ptr(), m.loss.data_ptr(), y.data_ptr()
            s.batch, s.classes = int(m.logits.shape[0]), int(m.logits.shape[1])
        with ops._Timed(name[4:] + "_kernel", 0):
            _lib.call(name, _lib.ctypes.byref(s), _lib.stream())

    def summaries(self):
        """The records committed since the last call, oldest first (lbt_amd.summary.decode's dicts: step,
        batch, loss, accuracy, scalars under the reference's tags, param_sums, overflow). Synchronises and
        copies the ring once; records overwritten before being read are counted in summary_dropped."""
        if self._sring is None:
            return []
        return self._sring.drain()

    @property
    def summary_dropped(self):
        return 0 if self._sring is None else self._sring.dropped

    def _log_batch(self, batch, loss):
        """The every-100-batches logging point of both epoch loops. With summaries: drain them, log the
        reference's line (trainer.py:155) from the newest record, append each to logdir/train/summaries.jsonl."""
        recs = self.summaries()
        if recs and self.logdir:
            from .summary import append_jsonl
            append_jsonl(os.path.join(self.logdir, "train", "summaries.jsonl"), recs)
        if self.logger is None:
            return
        if recs:
            self.logger.info("Batch %d loss %f acc %f" % (batch, recs[-1]["loss"], recs[-1]["accuracy"]))
        else:
            self.logger.info("Batch %d loss %f" % (batch, loss.item()))

    @staticmethod
    def _has_dropout(model):
        from .dfxp.layers import Dropout_q
        root = getattr(model, "model", model)
        return hasattr(root, "_walk") and any(isinstance(l, Dropout_q) for l in root._walk())

    def _setup_exchange(self):
        """The exact exchange of a fused plan: buffer, descriptor, and the finish kernel's segments."""
        m, ctx, flat = self.model, self.ctx, self.flat
        Q = len(ctx.quantizers)
        self.xbuf, x = D.make_exchange(flat.n, Q, ctx.device)
        x.gbase = flat.g.data_ptr()
        rank = dist.get_rank(self.pg)
        # SyncBN: the gamma / beta numerators come from pass-A sums that are already global
        x.pjob_scale = 1 if (not getattr(m, "sync_bn", False) or rank == 0) else 0
        x.counts = ctx.counts.data_ptr()
        self._xchg = x
        m.set_exchange(x)
        self._segs, self._seg_blocks = D.finish_segments(flat, ctx.device)

    def _setup_exchange_layerwise(self):
        """The exact exchange of a layer-wise model: every gradient reduction writes its integer
        numerator into the exchange buffer (ops.set_exchange_sink during the step), the counters are
        folded in by lbt_step_reduce_x's fold blocks; all-reduce, lbt_step_finish, range update."""
        ctx, flat = self.ctx, self.flat
        self.xbuf, x = D.make_exchange(flat.n, len(ctx.quantizers), ctx.device)
        x.gbase = flat.g.data_ptr()
        x.counts = ctx.counts.data_ptr()
        x.pjob_scale = 1
        self._xchg = x
        self._segs, self._seg_blocks = D.finish_segments(flat, ctx.device)

    def _sync_optimizer(self):
        """Hand the current lr / momentum and the flat buffers to every fused plan that applies the
        update itself (read when a step is captured or run eagerly)."""
        if self._fused_update:
            for p in [self.model] + list(getattr(self, "_plans", {}).values()):
                p.set_optimizer(self.flat, self.lr, self.momentum)

    # -- the reference's API ---------------------------------------------------------------
    def init_model(self):
        self.flat.a.zero_()

    def get_train_op(self):
        """Rebuilding MomentumOptimizer resets its accumulators (trainer.py:79-84)."""
        self.flat.a.zero_()
        self._graphs = None  # lr is baked into the captured optimiser kernel
        self._gcache = {}
        self._sync_optimizer()
        return self.step

    # -- the step ----------------------------------------------------------------------------
    def _plan(self, N):
        """The execution plan for a batch of N: a fused plan is built for one batch shape, so another
        N (the epoch's final partial batch, trainer.py:98) gets a plan of its own over the same
        layers, parameters and quantisers."""
        m = self.model
        if not hasattr(m, "set_exchange") or m._shape is None or m._shape[0] == N:
            return m
        p = self._plans.get(N)
        if p is None:
            from .fused import FusedResNet
            p = FusedResNet(m.model, sync_bn=m.sync_bn, process_group=m.pg, force_sync_bn=m.sync_bn)
            if self.xbuf is not None:
                p.set_exchange(self._xchg)
            if self._fused_update:
                p.set_optimizer(self.flat, self.lr, self.momentum)
            self._plans[N] = p
            # graphs captured while this was the only plan hold no per-step element-count copy
            # (_fwd_bwd adds one only once several plans exist): re-capture them with it, or they
            # would replay with the new plan's overflow-rate denominators
            self._gcache = {}
            self._graphs = None
        return p

    def _fwd_bwd(self, X, y, update=False, summary=False):
        """The step's forward + backward; update=True lets a fused plan apply the optimiser and the range
        update in its last launch. Returns whether it did (then _update must not run). summary: a fused
        plan records the step itself, around its tail (a layer-wise model's launches bracket _update)."""
        m = self._active = self._plan(X.shape[0])
        did = False
        nel = getattr(m, "_nelem", None)
        if nel is not None and self._plans:  # several plans: this one's per-step element counts
            self.ctx.nelem.copy_(nel)
        if not getattr(m, "zeroes_own_sums", False):
            self.ctx.zero_sums()
        if hasattr(m, "train_fwd_bwd"):
            if summary:
                did = bool(m.train_fwd_bwd(X, y, update=update and self._fused_update, summary=self._summary(m)))
            else:  # (a step that does not record makes the call it always made)
                did = bool(m.train_fwd_bwd(X, y, update=update and self._fused_update))
        elif self._lw_exact:
            x = self._xchg
            self._loss_n = int(X.shape[0]) * self.world
            ops.set_exchange_sink(self.flat.g, self.flat.n, self.xbuf, x.loss_off, self.world)
            try:
                with self.ctx.shard_masks():  # Dropout_q: this rank's bits of the global batch's mask
                    m.forward(X)
                    m.compute_loss(y)
                    m.backward()
            finally:
                ops.set_exchange_sink()
            # the overflow counters into the buffer (lbt_step_reduce_x with its fold blocks only)
            _lib.call("lbt_step_reduce_x", None, 0, 0, None, 0, 0, None, _lib.ctypes.byref(x), _lib.stream())
        else:
            m.forward(X)
            m.compute_loss(y)
            with ops.deferred_reductions():  # the backward's wgrad reduces / BN parameter grads: two launches at the end
                m.backward()
        if nel is None and hasattr(m, "set_exchange"):
            m._nelem = self.ctx.nelem.clone()  # what its build declared (Quantizer.observe)
        if self.comm is not None:
            self.ctx.fold_counts(self.comm[self.flat.n:])
        return did

    def _exchange(self):
        """Sum the step's gradients + overflow counters across ranks (one RCCL all-reduce;
        lbt_amd/distributed.py)."""
        D.allreduce_comm(self.xbuf if self.xbuf is not None else self.comm, self.pg)

    def _update(self):
        if self.xbuf is not None:  # exact exchange: dequantise the global sums, SGD, range update
            ctx, f = self.ctx, self.flat
            x = self._xchg
            _lib.call("lbt_step_finish", _lib.ptr(self._segs), len(self._segs) // _lib.ctypes.sizeof(_lib.FSeg),
                      self._seg_blocks, _lib.ptr(self.xbuf), _lib.ptr(f.w), _lib.ptr(f.a), _lib.ptr(f.g),
                      float(self.lr), float(self.momentum), _lib.ptr(self._active.loss), x.loss_off,
                      self._loss_n if self._lw_exact else int(self._active._head.loss_n), _lib.stream())
            _lib.call("lbt_dfxp_range_update_x", _lib.ptr(ctx.exps), _lib.ptr(self.xbuf), x.cnt_off,
                      _lib.ptr(ctx.bits), _lib.ptr(ctx.target), _lib.ptr(ctx.nelem), len(ctx.quantizers),
                      _lib.ptr(ctx.step), _lib.stream())
        elif self.comm is not None:
            ops.sgd_momentum(self.flat.w, self.flat.a, self.flat.g, self.lr, self.momentum, 1.0 / self.world)
            self.ctx.update_range_folded_op(self.comm[self.flat.n:])
        else:  # optimiser + range update in one launch
            self.ctx.update_range_op(sgd=(self.flat.w, self.flat.a, self.flat.g, self.lr, self.momentum, 1.0))

    def _update_recorded(self, y, rec):
        """_update, between lbt_summary_record and lbt_summary_commit when a layer-wise model's step records."""
        lw = rec and not hasattr(self._active, "train_fwd_bwd")
        if lw:
            self._summary_call("lbt_summary_record", self._active, y)
        self._update()
        if lw:
            self._summary_call("lbt_summary_commit", self._active)

    def _eager(self, X, y, rec=False):
        self._sync_optimizer()  # an assignment to self.lr / self.momentum takes effect on the fused update too
        did = self._fwd_bwd(X, y, update=not self.dp, summary=rec)
        if self.dp:
            self._exchange()
        if not did:
            self._update_recorded(y, rec)

    def _warmup(self, X, y):
        """One un-captured forward + backward that allocates every per-layer buffer before a capture.
        Its side effects are undone: the overflow counters (no update is applied) and the BN running
        statistics (the reference moves them once per step, dynamic_fixed_point.py:601-612)."""
        saved = [(bn.X_mean_running.clone(), bn.X_var_running.clone()) for bn in self._bn_layers()]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._fwd_bwd(X, y)
            if self.dp and self.capture_comm:
                # a collective must have run once (communicator set up) before one is captured; the
                # exchange buffer is rewritten by the next step's backward
                self._exchange()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self.ctx.counts.zero_()
        for bn, (m, v) in zip(self._bn_layers(), saved):
            bn.X_mean_running.copy_(m)
            bn.X_var_running.copy_(v)

    # -- range calibration -------------------------------------------------------------------
    @staticmethod
    def _param_quantizers(root):
        """[(quantiser, parameter tensor)] of every layer of the layer-wise model: what does not depend on
        the batch (Conv2d_q / Dense_q W and b, Rescale_q gamma and beta)."""
        out, seen = [], set()

        def walk(layer):
            if id(layer) in seen:
                return
            seen.add(id(layer))
            for rng, var in (("W_range", "W"), ("g_range", "gamma")):
                if hasattr(layer, rng) and hasattr(layer, var):
                    out.append((getattr(layer, rng), getattr(layer, var)))
            if hasattr(layer, "b_range"):
                out.append((layer.b_range, layer.beta if hasattr(layer, "beta") else layer.b))
            for attr in ("layers", "residual", "shortcut"):
                sub = getattr(layer, attr, None)
                for l in (sub if isinstance(sub, (list, tuple)) else [sub] if sub is not None else []):
                    walk(l)
        for layer in root.layers:
            walk(layer)
        return out

    def calibrate(self, X, y):
        """Set every quantiser's range from one batch (X, y: device tensors as step() takes them): one
        forward, loss and backward of the layer-wise model inside ``DfxpContext.calibrating`` -- a fused
        plan's ``model.model``, which shares every quantiser and parameter -- on a side stream outside any
        capture, as the warm-up runs. Each range lands where update_range leaves it on this batch, so the
        controller starts from its fixed point instead of the reference's I = 2. Everything else the pass
        touches is put back: overflow counters zeroed, the noise step, BN running statistics, element
        counts, parameters, accumulators, gradients, summaries and ``global_step`` as before; the next
        step draws the noise and masks this pass saw. Before the first step or between steps (captured
        graphs read the exponents from device memory). Returns {"set": {name: I}, "kept": [names],
        "unfed": [names]}: kept ranges were left (nothing of the tensor reaches the lowest range -- a
        zero beta or bias), unfed quantisers met no tensor."""
        world = dist.get_world_size(self.pg) if (dist.is_available() and dist.is_initialized()) else 1
        if max(world, self.world, self.ctx.world_size) > 1:
            raise NotImplementedError("calibrate() under a process group of %d ranks: each rank would set its own "
                                      "ranges from its shard (the ranks' tables are not summed yet)"
                                      % max(world, self.world, self.ctx.world_size))
        ctx = self.ctx
        root = getattr(self.model, "model", self.model)
        if not hasattr(root, "forward") or not hasattr(root, "backward"):
            raise TypeError("calibrate() needs a layer-wise model (or a plan over one)")
        torch.cuda.synchronize()
        bns = self._bn_layers()
        saved_bn = [(bn.X_mean_running.clone(), bn.X_var_running.clone()) for bn in bns]
        saved_nelem = ctx.nelem.clone()
        saved_qn = [q._nelem for q in ctx.quantizers]
        saved_g = self.flat.g.clone()
        saved_step = ctx.step.clone()
        own = root is not self.model
        had_prologue = getattr(root, "_pro", None) is not None
        if own:
            # a plan's step clears the arena it found when it was built: the layer-wise model's reduction
            # buffers live in an arena of this pass's own, so no step ever pays for them
            main = (ctx.sums_arena, ctx._sums_used, ctx._extra_arenas)
            if getattr(self, "_cal_arena", None) is None:
                self._cal_arena = (torch.zeros(1 << 20, dtype=torch.int64, device=ctx.device), 0, [])
            ctx.sums_arena, ctx._sums_used, ctx._extra_arenas = self._cal_arena
        params = self._param_quantizers(root)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        try:
            with torch.cuda.stream(s):
                ctx.zero_sums()  # (buffers carved later come from memory nothing has written: zeros)
                with ctx.calibrating(params) as cal:
                    root.forward(X)
                    root.compute_loss(y)
                    root.backward()
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
        finally:
            if own:
                self._cal_arena = (ctx.sums_arena, ctx._sums_used, ctx._extra_arenas)
                ctx.sums_arena, ctx._sums_used, ctx._extra_arenas = main
            ctx.counts.zero_()
            ctx.step.copy_(saved_step)
            ctx.nelem.copy_(saved_nelem)
            for q, n in zip(ctx.quantizers, saved_qn):
                q._nelem = n
            if not own and not had_prologue:
                # the parameter prologue this pass built declared its element counts once, and they were
                # just put back: the model's next forward builds it (and declares them) again
                root._pro = None
            self.flat.g.copy_(saved_g)
            for bn, (m, v) in zip(bns, saved_bn):
                bn.X_mean_running.copy_(m)
                bn.X_var_running.copy_(v)
            torch.cuda.synchronize()
        return cal.result()

    def _capture(self, X, y, rec=False):
        m = self.model
        fresh = not self._gflag or self._static is None or self._static[0].shape != X.shape
        if fresh:
            self._graphs = None  # another shape re-sizes the per-layer buffers: every graph on them goes
            if hasattr(m, "input_buffer") and hasattr(m, "label_buffer"):
                # capture on the model's own buffers: no copies inside the graph
                self._static = (m.input_buffer(X.shape), m.label_buffer(y.shape[0]))
            else:
                self._static = (torch.empty_like(X), torch.empty_like(y))
        sX, sy = self._static
        sX.copy_(X)
        sy.copy_(y)
        if fresh:  # (the other flag's graph of this shape left every buffer allocated)
            self._warmup(sX, sy)
        self._gflag[rec] = self._graphs = self._capture_step(sX, sy, rec)

    def _comm_capturable(self):
        """Capture the exchange ALONE into a throwaway graph (never replayed) once: whether this RCCL /
        runtime supports the collective inside a HIP graph. Only this probe may fail over to the
        host-issued exchange; any error while capturing the step itself is raised as it is."""
        if getattr(self, "_comm_probe", None) is None:
            g = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    self._exchange()
                self._comm_probe = True
            except RuntimeError:
                import traceback
                print("trainer: the collective cannot be captured in a HIP graph; the exchange runs from the "
                      "host between two graphs. The capture failed with:\n" + traceback.format_exc(),
                      file=sys.stderr)
                self._comm_probe = False
            del g
            torch.cuda.synchronize()
        return self._comm_probe

    def _capture_step(self, X, y, rec=False):
        """(g1, g2): the step as one graph (no exchange, or captured collectives), else the forward +
        backward and the update as two graphs with the host-issued exchange between them. When the
        exchange cannot be captured (``_comm_capturable``) it runs from the host, loudly (not for SyncBN
        plans, whose statistics collectives sit inside the forward)."""
        if self.dp and self.capture_comm and not getattr(self.model, "sync_bn", False):
            if not self._comm_capturable():
                self.capture_comm = False
        return self._capture_step_once(X, y, rec)

    def _capture_step_once(self, X, y, rec=False):
        one = not self.dp or self.capture_comm
        # thread-local capture: the process group's watchdog thread queries events meanwhile
        mode = "thread_local" if self.capture_comm else "global"
        g1 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g1, capture_error_mode=mode):
            did = self._fwd_bwd(X, y, update=not self.dp, summary=rec)
            if one:
                if self.dp:
                    self._exchange()
                if not did:
                    self._update_recorded(y, rec)
        g2 = None
        if not one:
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2):
                self._update()
        return g1, g2

    def _capture_bound(self, X, y, rec=False):
        """Capture the step reading (X, y) in place (models with binds_inputs): one graph per batch
        buffer pair (and per kind of step: recording or not), the first capture after a warm-up that
        allocates every per-layer buffer."""
        if getattr(self._plan(X.shape[0]), "_shape", 0) is None or not self._gcache:
            self._warmup(X, y)  # every plan's first run allocates its buffers outside a capture
        return self._capture_step(X, y, rec)

    def _bound_room(self, rec):
        """Whether one more bound buffer pair may get a graph: at most 8 per kind of step."""
        return sum(1 for k in self._gcache if k[3] == rec) < 8

    def prepare(self, X, y):
        """Build (capture) the step's graph for this batch buffer pair without running a step -- setup
        before a timed loop, so that no capture lands inside it whatever the warm-up count (a loader's
        ring of batch buffers gets one graph per buffer, on its first step otherwise)."""
        self._active = self._plan(X.shape[0])
        if not self.use_graph or (getattr(self.model, "sync_bn", False) and not self.capture_comm):
            return
        kinds = ([False] if self.summary_every != 1 else []) + ([True] if self.summary_every > 0 else [])
        for rec in kinds:  # both kinds of step a trainer with summaries replays
            key = (X.data_ptr(), y.data_ptr(), tuple(X.shape), rec)
            if getattr(self.model, "binds_inputs", False):
                if key not in self._gcache and self._bound_room(rec):
                    self._gcache[key] = self._capture_bound(X, y, rec)
            elif rec not in self._gflag or self._static is None or self._static[0].shape != X.shape:
                self._capture(X, y, rec)

    def step(self, X, y):
        """One training step on batch (X [B,32,32,3] fp32 NHWC, y [B] int32), device tensors.
        A SyncBN plan holds collectives inside the step: captured with them (RCCL), else eager."""
        self._active = self._plan(X.shape[0])
        rec = self._records()
        if not self.use_graph or (getattr(self.model, "sync_bn", False) and not self.capture_comm):
            self._eager(X, y, rec)
        else:
            key = (X.data_ptr(), y.data_ptr(), tuple(X.shape), rec)
            if getattr(self.model, "binds_inputs", False) and (key in self._gcache or self._bound_room(rec)):
                # the batch is read where it lies: a graph per buffer pair (a loader's ring of
                # batch buffers), no copy into static inputs inside the timed step
                if key not in self._gcache:
                    self._gcache[key] = self._capture_bound(X, y, rec)
                self._glast = self._gcache[key]
            elif rec not in self._gflag or self._static is None or self._static[0].shape != X.shape:
                self._capture(X, y, rec)
            else:
                self._static[0].copy_(X)
                self._static[1].copy_(y)
                self._glast = self._gflag[rec]
            g1, g2 = self._glast
            g1.replay()
            if g2 is not None:
                self._exchange()
                g2.replay()
        self.global_step += 1
        return self._active.loss

    # -- sharded epochs ----------------------------------------------------------------------
    def _check_epoch(self, n):
        """Before an epoch loop draws, allocates or launches anything: every batch size it will produce
        splits over the ranks (check_epoch_shards). One process: nothing to check."""
        if self._shard:
            check_epoch_shards(n, self.batch_size, self.world)

    def _shard_of(self, nb):
        """Rows [lo, hi) of a global batch of nb rows this rank takes: all of them in one process."""
        return shard_rows(nb, self.world, self.rank) if self._shard else (0, nb)

    def _epoch_perm(self, n):
        """The epoch's permutation (host int64): torch.randperm(n) where the single-process loop draws it;
        under sharding rank 0's draw, broadcast over the trainer's process group (the other ranks draw
        nothing: only rank 0's generator has to match the single process)."""
        if not self._shard:
            return torch.randperm(n)
        perm = torch.randperm(n) if self.rank == 0 else torch.empty(n, dtype=torch.int64)
        src = dist.get_global_rank(self.pg, 0) if self.pg is not None else 0
        if dist.get_backend(self.pg) == "nccl":  # RCCL moves device tensors
            t = perm.to(self.ctx.device)
            dist.broadcast(t, src=src, group=self.pg)
            return t.cpu()
        dist.broadcast(perm, src=src, group=self.pg)
        return perm

    def train(self, augment=True):
        """Epoch loop of trainer.py:117-192 over an in-memory dataset ((Xtr, ytr), (Xte, yte)):
        shuffled batches, preprocess_image on device (random flip + pad-4 random crop,
        lbt_augment_flip_crop), the lr schedule of :122-140, and the test loop after every epoch.
        Returns the per-epoch test accuracies.
        A dataset (DeviceDataset, DeviceDataset | None) (lbt_amd.data) runs the same epochs from device
        memory: see _train_device. A pair of ResizedCropDataset runs them with the ImageNet transforms
        (the random box and flip per training sample when augmenting, the centre crop for the test loop); a
        pair of RaggedCropDataset the same from images of their own sizes.
        Under a process group of ``world`` > 1 ranks (a data-parallel trainer) the epoch is sharded:
        ``batch_size`` stays the GLOBAL batch (trainer.py:34); rank 0 draws the epoch's permutation where
        the single process draws it and broadcasts it (one small collective per epoch, outside any
        capture); of every global batch of nb rows -- the final partial one too -- rank r gathers rows
        [r * nb / world, (r + 1) * nb / world) of the permuted batch (shard_rows) and augments them with
        THEIR draws of the global batch (lbt_augment_flip_crop_at / lbt_batch_gather's base). Both
        batch_size and n % batch_size must be divisible by world: checked before anything is drawn,
        allocated or launched (ValueError). With FusedResNet(sync_bn=True), or a ranked context's plain
        model, N ranks leave the parameters, momentum, exponents and BN statistics of one process with
        the same torch seed, bit for bit; batch_sizes records the global nb. No timing is claimed for it."""
        if isinstance(self.dataset[0], DEVICE_DATASETS):
            return self._train_device(augment)
        (Xtr, ytr), (Xte, yte) = self.dataset
        self._check_epoch(len(Xtr))
        dev = self.ctx.device
        history = []
        for epoch in range(self.n_epoch):
            if epoch == 0:
                self.get_train_op()
            elif epoch in (80, 120, 140):
                self.lr *= self.lr_decay_factor
                self.get_train_op()
            perm = self._epoch_perm(len(Xtr))
            self.batch_sizes = []
            for b in range(0, len(Xtr), self.batch_size):  # the final partial batch too (trainer.py:98)
                nb = min(self.batch_size, len(Xtr) - b)
                lo, hi = self._shard_of(nb)  # (one process: the whole batch)
                idx = perm[b + lo:b + hi]
                X = torch.as_tensor(Xtr[idx.numpy()], dtype=torch.float32).to(dev).contiguous()
                y = torch.as_tensor(ytr[idx.numpy()], dtype=torch.int32).to(dev)
                if augment:
                    if self._aug is None or self._aug.shape != X.shape:
                        self._aug = torch.empty_like(X)
                    X = ops.augment_flip_crop(X, 4, self.ctx.seed, self.global_step, out=self._aug, base=lo)
                loss = self.step(X, y)
                self.batch_sizes.append(nb)
                if (b // self.batch_size + 1) % 100 == 0 and (self.logger is not None or self._sring is not None):
                    self._log_batch(b // self.batch_size + 1, loss)
            if Xte is not None and len(Xte):
                acc, _ = self.evaluate(Xte, yte)
                history.append(acc)
                if self.logger is not None:
                    self.logger.info("Epoch %d test accuracy %f" % (epoch + 1, acc))
        return history

    # -- the same loops from a device-resident dataset (lbt_amd/data.py) ----------------------
    def _batch_buffers(self, ds, n):
        """The fixed (X, y) pair every batch of n samples is gathered into: a model that binds its inputs
        then holds one captured graph per batch size."""
        key = (n,) + tuple(ds.sample_shape)
        if key not in self._inbuf:
            dev = self.ctx.device
            self._inbuf[key] = (torch.empty(key, dtype=torch.float32, device=dev),
                                torch.empty(n, dtype=torch.int32, device=dev))
        return self._inbuf[key]

    def _train_device(self, augment):
        """train() over (DeviceDataset, DeviceDataset | None): the epoch's permutation is drawn on the host
        as in train() (the same torch seed gives the same order) and uploaded once; each step is one
        lbt_batch_gather launch -- gather, load_data's normalisation, preprocess_image with the draws
        lbt_augment_flip_crop makes at this step -- into the batch size's buffer pair, then the step, on
        one stream. No batch crosses PCIe and nothing synchronises inside the epoch (but the logger line
        every 100 batches). The gather is launched ahead of the step's graph, not captured into it: its
        arguments change every step. Bit for bit the host loop on ds.host_float(). (A ResizedCropDataset:
        the same loop with one lbt_batch_resized_crop (or, with color_jitter, _jitter) launch per step, through the classes' common
        train_batch / test_batch / sample_shape; a RaggedCropDataset: lbt_batch_ragged_crop / _jitter, likewise.)
        Sharded (see train()): every rank holds the whole dataset on its GPU and uploads the broadcast
        permutation; rank r's launch gathers idx = perm[b + r*s : b + (r+1)*s] with base = r*s into a
        buffer pair of the shard's size s = nb / world."""
        ds, ds_te = self.dataset
        n = len(ds)
        self._check_epoch(n)
        history = []
        for epoch in range(self.n_epoch):
            if epoch == 0:
                self.get_train_op()
            elif epoch in (80, 120, 140):
                self.lr *= self.lr_decay_factor
                self.get_train_op()
            perm = self._epoch_perm(n)
            if self._perm is None or self._perm.numel() != n:
                self._perm = torch.empty(n, dtype=torch.int32, device=self.ctx.device)
            ds.upload_index(perm, out=self._perm)
            self.batch_sizes = []
            for b in range(0, n, self.batch_size):  # the final partial batch too (trainer.py:98)
                nb = min(self.batch_size, n - b)
                lo, hi = self._shard_of(nb)  # (one process: the whole batch, base 0)
                X, y = self._batch_buffers(ds, hi - lo)
                ds.train_batch(X, y, idx=self._perm[b + lo:b + hi], augment=augment, base=lo, seed=self.ctx.seed,
                               counter=self.global_step)
                loss = self.step(X, y)
                self.batch_sizes.append(nb)
                if (b // self.batch_size + 1) % 100 == 0 and (self.logger is not None or self._sring is not None):
                    self._log_batch(b // self.batch_size + 1, loss)
            if ds_te is not None and len(ds_te):
                acc, _ = self.evaluate(ds_te)
                history.append(acc)
                if self.logger is not None:
                    self.logger.info("Epoch %d test accuracy %f" % (epoch + 1, acc))
        return history

    def _evaluate_device(self, ds, batch_size, testing):
        """evaluate() / evaluate(testing=True) over a DeviceDataset: the batches are first = b slices gathered
        on the device; each batch's accuracy and loss stay device tensors until one copy at the end, and
        are summed on the host in the order and type of the host loops (fp32 values added in double), so the
        returned pair and every side effect equal theirs."""
        from .fused import FusedResNet
        m = self.model
        fused = isinstance(m, FusedResNet)
        restore = not (testing and fused)  # inference plans touch neither the counters nor the element counts
        if restore:
            saved, saved_nelem = self.ctx.counts.clone(), self.ctx.nelem.clone()
        if testing and not fused:
            was_training = getattr(m, "training", True)
            m.set_testing()
        accs, losses, shared = [], [], not fused
        try:
            for b in range(0, len(ds), batch_size):
                nb = min(batch_size, len(ds) - b)
                Xb, yb = self._batch_buffers(ds, nb)
                ds.test_batch(Xb, yb, first=b)
                if not testing:
                    p, shared = self._eval_model(nb)
                elif fused:
                    key = ("testing", nb)
                    if key not in self._eval:
                        self._eval[key] = FusedResNet(m.model, inference=True)
                    p = self._eval[key]
                else:
                    p = m
                if not fused:  # (as evaluate: a layer-wise model's sums arena is this trainer's to clear)
                    self.ctx.zero_sums()
                logits = p.forward(Xb)
                loss = p.compute_loss(yb)
                accs.append((logits.argmax(dim=1).to(torch.int32) == yb).float().mean())
                losses.append(loss.detach().reshape(-1)[0].clone())  # the plan rewrites its loss buffer
        finally:
            if testing and not fused and was_training:
                m.set_training()
            if restore:
                self.ctx.counts.copy_(saved)
                self.ctx.nelem.copy_(saved_nelem)
                for q in self.ctx.quantizers:  # (as evaluate: the cached counts describe the test batches)
                    q._nelem = None
                if shared:
                    self._graphs = None
        if not accs:
            return 0.0, 0.0
        acc_sum = loss_sum = 0.0
        for a, l in zip(torch.stack(accs).cpu().tolist(), torch.stack(losses).cpu().tolist()):
            acc_sum += a
            loss_sum += l
        return acc_sum / len(accs), loss_sum / len(accs)

    # -- test loop and checkpoint (trainer.py:164-197) ----------------------------------------
    def _eval_model(self, n):
        """The model the test loop runs for a batch of n: a FusedResNet gets a plan of its own per
        test-batch size (its own buffers, so the captured training graph stays valid); a
        layer-wise model is shared (its per-layer buffers are re-sized by the test batch, so the
        training graph is re-captured afterwards)."""
        from .fused import FusedResNet
        m = self.model
        if isinstance(m, FusedResNet):
            if n not in self._eval:
                self._eval[n] = FusedResNet(m.model)
            return self._eval[n], False
        return m, True

    def _unsynced(self):
        """The context the whole-batch test loops run in: a layer-wise model with sync_batchnorm suspends
        its synchronisation (Model.sync_suspended, restored also when the loop raises), because every rank
        forwards every test batch whole -- a rank's moments of that batch are the one process's, and a sum
        over the ranks would count it world times. Anything else: nothing."""
        m = self.model
        if getattr(m, "sync_bn", False) and hasattr(m, "sync_suspended"):
            return m.sync_suspended()
        return contextlib.nullcontext()

    def _shards_eval(self, testing):
        """Whether evaluate() splits its test batches over the ranks: only where the rows a rank computes
        are the single process's -- a FusedResNet's inference plans (no batch coupling), or its training-
        mode plans when it was trained with sync_bn=True (whole-batch moments through SyncBN). Decided from
        what every rank shares (the trainer's world, the model's kind), so all ranks take the same path."""
        from .fused import FusedResNet
        m = self.model
        return bool(self._shard and isinstance(m, FusedResNet) and (testing or m.sync_bn))

    def _evaluate_sharded(self, X, y, batch_size, testing):
        """evaluate() with every test batch split by rows over the ranks (host arrays or a DeviceDataset):
        rank r forwards rows [r * nb / world, (r + 1) * nb / world) of each batch of nb -- training mode on a
        SyncBN eval plan per shard size (keys ("sync", s) of self._eval; its moments are the whole batch's, so
        logits rows and the running statistics each batch leaves are the single process's), testing mode on
        the inference plans -- and lbt_eval_tally (one launch, in place of the argmax / == / float / mean
        kernels and the loss launch) writes the shard's correct count and fixed-point loss sum into its row of
        one int64 tensor [nbatches, 2]. After the loop ONE all-reduce sums the rows over the ranks and one copy
        brings them to the host (decode_tally). A batch whose size is not divisible by world runs in the
        redundant form on every rank (whole batch, local-BN eval plan; rank 0's tally counts). The accuracy
        equals one process's exactly; the loss is the same fixed-point sum lbt_step_finish decodes. Counters
        and element counts are saved and restored as in the other loops."""
        from .fused import FusedResNet
        m, dev, ctx = self.model, self.ctx.device, self.ctx
        ds = X if isinstance(X, DEVICE_DATASETS) else None
        n = len(X)
        starts = list(range(0, n, batch_size))
        if not starts:
            return 0.0, 0.0
        rows = torch.zeros((len(starts), 2), dtype=torch.int64, device=dev)
        restore = not testing  # inference plans touch neither the counters nor the element counts
        if restore:
            saved, saved_nelem = ctx.counts.clone(), ctx.nelem.clone()
        sizes = []
        try:
            for i, b in enumerate(starts):
                nb = min(batch_size, n - b)
                sizes.append(nb)
                split = nb % self.world == 0  # (nb and world: the same on every rank)
                lo, hi = shard_rows(nb, self.world, self.rank) if split else (0, nb)
                if ds is not None:
                    Xb, yb = self._batch_buffers(ds, hi - lo)
                    ds.test_batch(Xb, yb, first=b + lo)
                else:
                    Xb = torch.as_tensor(X[b + lo:b + hi], dtype=torch.float32).to(dev).contiguous()
                    yb = torch.as_tensor(y[b + lo:b + hi], dtype=torch.int32).to(dev)
                if testing:
                    key = ("testing", hi - lo)
                    if key not in self._eval:
                        self._eval[key] = FusedResNet(m.model, inference=True)
                    p = self._eval[key]
                elif split:
                    key = ("sync", hi - lo)
                    if key not in self._eval:
                        self._eval[key] = FusedResNet(m.model, sync_bn=True, process_group=m.pg)
                    p = self._eval[key]
                else:
                    p, _ = self._eval_model(nb)
                logits = p.forward(Xb)
                if split or self.rank == 0:  # a redundant batch counts once in the sum over the ranks
                    ops.eval_tally(logits, yb, rows[i])
        finally:
            if restore:
                ctx.counts.copy_(saved)
                ctx.nelem.copy_(saved_nelem)
                for q in ctx.quantizers:  # (as evaluate: the cached counts describe the test batches)
                    q._nelem = None
        dist.all_reduce(rows, op=dist.ReduceOp.SUM, group=self.pg)
        return decode_tally(rows.cpu().tolist(), sizes)

    def _evaluate_testing(self, X, y, batch_size):
        """evaluate(testing=True): the test loop in testing mode (Model.set_testing, models.py:15) -- every
        BatchNorm normalises with its running averages and nothing moves. A FusedResNet runs one
        forward-only inference plan per test-batch size (keys ("testing", n) of self._eval), which
        touches neither the counters nor the element counts; a layer-wise model is wrapped in
        set_testing() / set_training() and its counters and element counts are restored."""
        from .fused import FusedResNet
        dev = self.ctx.device
        m = self.model
        fused = isinstance(m, FusedResNet)
        if not fused:
            was_training = getattr(m, "training", True)
            saved, saved_nelem = self.ctx.counts.clone(), self.ctx.nelem.clone()
            m.set_testing()
        acc_sum, loss_sum, nb = 0.0, 0.0, 0
        try:
            for b in range(0, len(X), batch_size):
                Xb = torch.as_tensor(X[b:b + batch_size], dtype=torch.float32).to(dev).contiguous()
                yb = torch.as_tensor(y[b:b + batch_size], dtype=torch.int32).to(dev)
                p = m
                if fused:
                    key = ("testing", len(Xb))
                    if key not in self._eval:
                        self._eval[key] = FusedResNet(m.model, inference=True)
                    p = self._eval[key]
                logits = p.forward(Xb)
                loss = p.compute_loss(yb)
                acc = (logits.argmax(dim=1).to(torch.int32) == yb).float().mean()
                acc_sum += float(acc.item())
                loss_sum += float(loss.item())
                nb += 1
        finally:
            if not fused:
                if was_training:
                    m.set_training()
                self.ctx.counts.copy_(saved)
                self.ctx.nelem.copy_(saved_nelem)
                for q in self.ctx.quantizers:  # (as evaluate: the cached counts describe the test batches)
                    q._nelem = None
                self._graphs = None
        return acc_sum / max(nb, 1), loss_sum / max(nb, 1)

    def evaluate(self, X, y=None, batch_size=1000, testing=False):
        """The reference's test loop (trainer.py:166-190): per batch of 1000 the forward pass in
        training mode (batch-statistic BN, stochastic quantisers, and Dropout_q still dropping, at the
        current step's mask -- the reference never runs set_testing, :164-165), loss and accuracy;
        returns (mean accuracy, mean loss) over the batches. The overflow counters these forwards accumulate are discarded (the loop does not
        fetch update_range_op); BN running statistics are updated, as the reference's are.
        testing=True: the same loop and return value in testing mode instead (running-average BN, Dropout_q
        the identity; what a trained network is deployed as): nothing is updated. A FusedResNet runs it on
        forward-only inference plans (FusedResNet(model, inference=True)), a layer-wise model between
        set_testing() and set_training().
        evaluate(ds) with a DeviceDataset (no y): the same loops on batches gathered on the device, the same
        return value and side effects (_evaluate_device).
        Under a process group of several ranks every rank runs the whole loop and gets the same result,
        except where a test batch can be split by rows exactly (_evaluate_sharded): the training-mode loop
        of a FusedResNet trained with sync_bn=True, and evaluate(testing=True) of a FusedResNet. A layer-wise
        model with sync_batchnorm runs the whole loop on every rank with its synchronisation suspended
        (_unsynced): a rank's moments of the whole test batch are the one process's.
        A layer-wise model's BN statistics are added into the context's sums arena, which this trainer
        clears once per training step: the loops clear it before each test batch's forward as well."""
        if isinstance(X, DEVICE_DATASETS) and y is not None:
            raise TypeError("a DeviceDataset carries its labels: evaluate(ds, batch_size=..., testing=...)")
        if self._shards_eval(testing):
            return self._evaluate_sharded(X, y, batch_size, testing)
        if isinstance(X, DEVICE_DATASETS):
            with self._unsynced():  # (a layer-wise SyncBN model: every rank holds the test batch whole)
                return self._evaluate_device(X, batch_size, testing)
        if testing:
            return self._evaluate_testing(X, y, batch_size)
        dev = self.ctx.device
        saved = self.ctx.counts.clone()
        saved_nelem = self.ctx.nelem.clone()  # an eval plan's build declares its own element counts
        acc_sum, loss_sum, nb, shared = 0.0, 0.0, 0, False
        with self._unsynced():  # (a layer-wise SyncBN model: every rank holds the test batch whole)
            for b in range(0, len(X), batch_size):
                Xb = torch.as_tensor(X[b:b + batch_size], dtype=torch.float32).to(dev).contiguous()
                yb = torch.as_tensor(y[b:b + batch_size], dtype=torch.int32).to(dev)
                m, shared = self._eval_model(len(Xb))
                if shared:
                    # a layer-wise model's BN channel sums are ADDED into the arena this trainer clears once
                    # per training step: each test batch starts from zeros too, not from the last step's sums
                    self.ctx.zero_sums()
                logits = m.forward(Xb)
                loss = m.compute_loss(yb)
                acc = (logits.argmax(dim=1).to(torch.int32) == yb).float().mean()
                acc_sum += float(acc.item())
                loss_sum += float(loss.item())
                nb += 1
        self.ctx.counts.copy_(saved)
        self.ctx.nelem.copy_(saved_nelem)
        # the quantisers' cached counts now describe the eval plan, not ctx.nelem: forget them so
        # the next plan build writes its own (Quantizer.observe skips a write that matches its cache)
        for q in self.ctx.quantizers:
            q._nelem = None
        if shared:
            self._graphs = None
        return acc_sum / max(nb, 1), loss_sum / max(nb, 1)

    def _bn_layers(self):
        out = []

        def walk(layers):
            for layer in layers:
                if hasattr(layer, "X_mean_running"):
                    out.append(layer)
                for attr in ("layers", "residual", "shortcut"):
                    sub = getattr(layer, attr, None)
                    if sub is None:
                        continue
                    walk(sub.layers if hasattr(sub, "layers") and not isinstance(sub, (list, tuple)) else sub)
        root = getattr(self.model, "model", self.model)
        walk(root.layers)
        return out

    def save_model(self, exp_path):
        """Checkpoint (trainer.py:189-192, tf.train.Saver): parameters, momentum accumulators, DFXP
        exponents + noise step, BN running statistics and the trainer's step / lr, as one
        safetensors file exp_path/model.safetensors (no pickled objects)."""
        import json
        import os

        from safetensors.torch import save_file
        os.makedirs(exp_path, exist_ok=True)
        t = {"w": self.flat.w, "a": self.flat.a, "exps": self.ctx.exps, "step": self.ctx.step}
        for i, bn in enumerate(self._bn_layers()):
            t["bn%d/mean" % i] = bn.X_mean_running
            t["bn%d/var" % i] = bn.X_var_running
        meta = {"global_step": str(self.global_step), "lr": repr(self.lr), "momentum": repr(self.momentum),
                "quantizers": json.dumps([q.name for q in self.ctx.quantizers]),
                "params": json.dumps([[o.name if hasattr(o, "name") else "", v, off, sz]
                                      for o, v, off, sz in self.flat.offsets])}
        path = os.path.join(exp_path, "model.safetensors")
        save_file({k: v.detach().contiguous().cpu() for k, v in t.items()}, path, metadata=meta)
        return path

    def load_model(self, path):
        """Restore a save_model checkpoint into this trainer (same model layout)."""
        import json

        from safetensors import safe_open
        with safe_open(path, framework="pt") as f:
            meta = f.metadata()
            if json.loads(meta["quantizers"]) != [q.name for q in self.ctx.quantizers]:
                raise ValueError("checkpoint quantiser layout differs from this model's")
            self.flat.w.copy_(f.get_tensor("w"))
            self.flat.a.copy_(f.get_tensor("a"))
            self.ctx.exps.copy_(f.get_tensor("exps"))
            self.ctx.step.copy_(f.get_tensor("step"))
            for i, bn in enumerate(self._bn_layers()):
                bn.X_mean_running.copy_(f.get_tensor("bn%d/mean" % i))
                bn.X_var_running.copy_(f.get_tensor("bn%d/var" % i))
        self.global_step = int(meta["global_step"])
        self.lr = float(meta["lr"])
        self.momentum = float(meta["momentum"])
        self._graphs = None  # lr is baked into the captured optimiser
        self._gcache = {}
        self._sync_optimizer()

"""The forward-only, testing-mode launch list of a ``FusedResNet(model, inference=True)``.

``Model.set_testing`` (reference ``models.py:15``) on the fused kernels: every ``Normalization_q``
normalises with its running averages (``dynamic_fixed_point.py:590-600``), so a launch needs no batch
statistics, no channel sums and -- nothing follows that would read them -- no overflow counters and
no R / X codes in memory. The plan reads ``ctx.exps`` / ``ctx.step`` / ``ctx.seed``, the parameters and the
running statistics; it writes its own buffers and the layers' forward weight images (the bytes a
training prologue writes from the same weights), and nothing else: no ``observe()``, every quantiser
descriptor with ``counts = NULL``, every BatchNorm descriptor frozen with ``ms = NULL``. Bit-identical
to the layer-wise model after ``set_testing()`` (tests/test_fused_inference.py).
"""
import ctypes
import math
import os

import torch

from . import _lib
from ._lib import OUT_I8, OUT_I16, OUT_U8OFF, BnNorm, ChainFwd, ConvFwd, NJob, QJob, WJob, ptr
from .dfxp import ops
from .fused import _dev_array


def build(plan, X):
    """Fill plan._fwd / _hfwd / _hloss for input batch X (FusedResNet._build's forward half, frozen)."""
    ctx = plan.ctx
    N, H, W, Cin0 = X.shape
    plan._X = plan._X_own = plan.input_buffer(X.shape)
    plan._labels = plan._labels_own = plan.label_buffer(N)
    lib = _lib.load()
    L = plan._launcher(lib)
    buf = plan._buf
    fwd, njobs = [], []
    plan._nd, plan._keep = {}, []
    fuse = plan.fuse_fwd
    fuse2 = fuse and plan.pair_launch and os.environ.get("LBT_FUSE_FWD2", "1") == "1"

    def qd(q, inner=0):
        """The plan's descriptor of quantiser q: no counters; inner > 0 gives a stochastic quantiser its
        per-step noise table of that many values (refreshed by the prologue)."""
        d = plan._nd.get(q)
        if d is None:
            d = q.desc_nostats()
            if inner and q.stochastic:
                tab = buf("noise:" + q.name, ((inner + 3) // 4 * 4,), torch.float32)
                d.noise = tab.data_ptr()
                njobs.append(NJob(ctx.step.data_ptr(), ctx.seed, q.qid, 0, inner, tab.data_ptr()))
            plan._nd[q] = d
        return d

    # ---- prologue jobs: weight, gamma / beta and input quantisers (forward images only)
    w4 = [c for c in plan.convs if c.mfma and c.w4]
    wimg = {}  # conv -> (entry point suffix, forward weight image pointer, bytes)
    if w4:  # own arena: one lbt_pack_int4 launch packs every 4-bit forward image
        total = sum(c.wf.numel() for c in w4)
        plan._w8 = torch.zeros(total, dtype=torch.int8, device=ctx.device)
        plan._w4 = torch.zeros(total // 2, dtype=torch.uint8, device=ctx.device)
        off = 0
        for c in w4:
            wimg[c] = ("w4", plan._w4.data_ptr() + off // 2, plan._w8.data_ptr() + off)
            off += c.wf.numel()
    wjobs = []
    for c in plan.convs:
        kh, kw, ci, co = c.ksize
        if c.mfma and c not in wimg:
            wimg[c] = ("", c.wf.data_ptr(), c.wf.data_ptr())
        wjobs.append(WJob(c.W.data_ptr(), kh, kw, ci, co, qd(c.W_range), c.w_hwio.data_ptr(),
                          wimg[c][2] if c.mfma else None, c.ksf, None, c.ksd, c.wcolsum.data_ptr() if c.mfma else None))
    d = plan.dense
    wjobs.append(WJob(d.W.data_ptr(), d.in_units, 1, 1, d.units, qd(d.W_range), d.w_hwio.data_ptr(), None, 0, None, 0,
                      None))
    qjobs = []
    for r in plan.rescales:
        C = r.C
        qjobs.append(QJob(r.gamma.data_ptr(), r.gb.data_ptr(), _lib.OUT_F32, C, 1, qd(r.g_range)))
        qjobs.append(QJob(r.beta.data_ptr(), r.gb.data_ptr() + 4 * C, _lib.OUT_F32, C, 1, qd(r.b_range)))

    def frozen(n, q):
        """Normalization_q n on codes q in testing mode: the running averages, nothing written."""
        C = q.shape[-1]
        return BnNorm(q.data_ptr(), qd(n.X_range), None, q.numel() // C, ops.f32(n.eps), ops.f32(n.momentum),
                      ops.f32(1 - n.momentum), None, n.X_mean_running.data_ptr(), n.X_var_running.data_ptr(), 1, 0)

    class Chain:
        """A forward chain not launched yet: the next conv launch absorbs it (its X codes then live in
        LDS only), or flush() gives it code buffers and its own lbt_bn_chain_fwd."""

        def __init__(self, key, br1, br2, y, res, q1, q2):
            qn = br1[1]
            self.key, self.shape = key, tuple(qn.shape)
            inner = qn.numel() // qn.shape[0]
            a = self.a = ChainFwd()
            for slot, br in ((a.b1, br1), (a.b2, br2)):
                if br is None:
                    continue
                n, q, r = br
                slot.nrm = frozen(n, q)
                slot.qr = qd(r.X_range, inner)
                slot.gb = r.gb.data_ptr()
            a.has_b2 = 1 if br2 is not None else 0
            a.res = res.data_ptr() if res is not None else None
            a.relu = 1
            a.y = y.data_ptr() if y is not None else None
            self.has_q1, self.has_q2 = q1 is not None, q2 is not None
            if q1 is not None:
                a.o1_kind, a.qo1 = OUT_U8OFF, qd(q1, inner)
            if q2 is not None:
                a.o2_kind, a.qo2 = OUT_U8OFF, qd(q2, inner)
            a.rows, a.inner, a.C = qn.shape[0], inner, qn.shape[-1]
            plan._keep.append(a)

        def flush(self):
            a = self.a
            o1 = o2 = None
            if self.has_q1:
                o1 = buf(self.key + "xa", self.shape, torch.int8)
                a.o1 = o1.data_ptr()
            if self.has_q2:
                o2 = buf(self.key + "xs", self.shape, torch.int8)
                a.o2 = o2.data_ptr()
            fwd.append(L("lbt_bn_chain_fwd", ctypes.byref(a), k="chain_fwd_kernel", nb=ops._chain_fwd_bytes(a)))
            return o1, o2

    def conv_plain(c, dd, xq, yq, qout):
        sfx, wf, _ = wimg[c]
        fwd.append(L("lbt_conv_fwd_i8" + sfx, ptr(xq), 1, ctypes.c_void_p(wf), c.ksf, ptr(c.wcolsum), dd, qd(c.X_range),
                     qd(c.W_range), None, ptr(yq), qout, None, k="conv_gemm_kernel<0> (fwd)",
                     nb=xq.numel() + c.wf.numel() + yq.numel()))

    def conv(c, dd, ch, yq, qout):
        """Conv c on pending chain ch's first output: one frozen lbt_conv_fwd_fused_i8, else the chain's
        own launch and lbt_conv_fwd_i8 (LBT_FUSE_FWD=0, or a shape the fused kernel does not tile)."""
        if fuse and not ch.has_q2 and plan._fusable_bwd(c, dd, flag=True):
            cf = ConvFwd()
            cf.c = ch.a
            cf.wf, cf.ksf, cf.w4 = wimg[c][1], c.ksf, 1 if wimg[c][0] else 0
            cf.wcolsum, cf.d, cf.qw = c.wcolsum.data_ptr(), dd, qd(c.W_range)
            cf.yq, cf.qout = yq.data_ptr(), qout
            a = ch.a
            nq = (2 if a.has_b2 else 1) + 2  # noise tables: R quantiser(s), X, output
            nb = (a.rows * a.inner * ((2 if a.has_b2 else 1) + (4 if a.res else 0) + (4 if a.y else 0))
                  + c.wf.numel() + yq.numel() + 4 * nq * a.inner)
            fwd.append(L("lbt_conv_fwd_fused_i8", ctypes.byref(cf), k="conv_fwd_fused_kernel", nb=nb))
            plan._keep.append(cf)
            return
        xq, _ = ch.flush()
        conv_plain(c, dd, xq, yq, qout)

    # ---- stem: conv1 on the signed 9-bit image, its epilogue = bn0's input quantiser (no sums)
    c = plan.conv1
    kh, kw, _, C0 = c.ksize
    dc = ops.conv_desc(N, H, W, Cin0, C0, kh, kw, c.strides[1], c.strides[2], c.padding)
    ximg = buf("ximg", (N, H, W, Cin0), torch.int16)
    plan._input_job = QJob(plan._X.data_ptr(), ximg.data_ptr(), OUT_I16, X.numel(), H * W * Cin0, qd(c.X_range))
    n0, r0 = plan.n0, plan.r0
    shp0 = (N, dc.Ho, dc.Wo, C0)
    numel0 = math.prod(shp0)
    inner0 = numel0 // N
    qn0 = buf("qn0", shp0, torch.int8)
    if c.stem(dc):
        fwd.append(L("lbt_conv_stem_fwd", ptr(ximg), ptr(c.w_hwio), dc, qd(c.X_range), qd(c.W_range), None, ptr(qn0),
                     qd(n0.X_range, inner0), None, k="stem_fwd_kernel", nb=ximg.numel() * 2 + c.w_hwio.numel() + numel0))
    else:
        y0 = buf("y0", shp0, torch.float32)
        fwd.append(L("lbt_conv_fwd_generic", ptr(ximg), 1, ptr(c.w_hwio), dc, qd(c.X_range), qd(c.W_range), ptr(y0),
                     k="conv_fwd_generic_kernel", nb=ximg.numel() * 2 + numel0 * 4))
        fwd.append(L("lbt_dfxp_quantize", ptr(y0), ptr(qn0), OUT_I8, N, inner0, qd(n0.X_range, inner0), None, C0,
                     k="quantize_rows_kernel", nb=numel0 * 5))
    X0 = buf("X0", shp0, torch.float32)
    b0 = plan.blocks[0]
    pending = Chain("s_", (n0, qn0, r0), None, X0, None, b0.c1.X_range, b0.cs.X_range if b0.cs is not None else None)

    # ---- residual blocks
    Xin = X0
    for i, b in enumerate(plan.blocks):
        nxt = plan.blocks[i + 1] if i + 1 < len(plan.blocks) else None
        Nb, Hb, Wb, Cin = Xin.shape
        c1, c2, cs = b.c1, b.c2, b.cs
        C = c1.ksize[3]
        s = c1.strides[1]
        d1 = ops.conv_desc(Nb, Hb, Wb, Cin, C, 3, 3, s, s, c1.padding)
        d2 = ops.conv_desc(Nb, d1.Ho, d1.Wo, C, C, 3, 3, 1, 1, c2.padding)
        shp = (Nb, d1.Ho, d1.Wo, C)
        inner = math.prod(shp[1:])
        k = "b%d_" % i
        qn1 = buf(k + "qn1", shp, torch.int8)
        q_n1 = qd(b.n1.X_range, inner)
        qns = None
        if cs is None:
            conv(c1, d1, pending, qn1, q_n1)
        else:
            ds = ops.conv_desc(Nb, Hb, Wb, Cin, C, 1, 1, s, s, cs.padding)
            qns = buf(k + "qns", shp, torch.int8)
            q_ns = qd(b.ns.X_range, inner)
            a = pending.a
            pair = (plan.pair_launch and not plan._fusable_bwd(c1, d1, flag=True) and (Cin, C) in ((16, 32), (32, 64))
                    and c1.mfma and cs.mfma)
            if (fuse2 and pair and not a.has_b2 and bool(a.res) and bool(a.y) and Wb * Cin == 512 and d1.Ho % 4 == 0
                    and (d1.PT, d1.PL, ds.PT, ds.PL) == (0, 0, 0, 0) and wimg[c1][0] == wimg[cs][0]):
                # the whole transition (the previous block's end chain + both strided convs): one launch
                cf2 = _lib.ConvFwd2()
                cf2.c = a
                cf2.wf1, cf2.ksf1, cf2.wcolsum1 = wimg[c1][1], c1.ksf, c1.wcolsum.data_ptr()
                cf2.wfs, cf2.ksfs, cf2.wcolsums = wimg[cs][1], cs.ksf, cs.wcolsum.data_ptr()
                cf2.w4 = 1 if wimg[c1][0] else 0
                cf2.d1, cf2.ds, cf2.qw1, cf2.qws = d1, ds, qd(c1.W_range), qd(cs.W_range)
                cf2.yq1, cf2.qout1 = qn1.data_ptr(), q_n1
                cf2.yqs, cf2.qouts = qns.data_ptr(), q_ns
                plan._keep.append(cf2)
                nb = (a.rows * a.inner * 9 + c1.wf.numel() + cs.wf.numel() + 2 * qn1.numel()
                      + 4 * (3 * a.inner + 2 * inner))
                fwd.append(L("lbt_conv_fwd2_fused_i8", ctypes.byref(cf2), k="conv_fwd2_kernel", nb=nb))
            else:
                xa, xs = pending.flush()
                if pair:  # conv-1 and the shortcut conv read the same pixels: one launch
                    jobs = [_lib.ConvFwdJob(x.data_ptr(), 1, 1 if wimg[cc][0] else 0, wimg[cc][1], cc.ksf,
                                            cc.wcolsum.data_ptr(), dd, qd(cc.X_range), qd(cc.W_range), None,
                                            yq.data_ptr(), qo, None)
                            for cc, dd, x, yq, qo in ((c1, d1, xa, qn1, q_n1), (cs, ds, xs, qns, q_ns))]
                    plan._keep += jobs
                    fwd.append(L("lbt_conv_fwd_pair_i8", ctypes.byref(jobs[0]), ctypes.byref(jobs[1]),
                                 k="conv_gemm2_kernel (fwd pair)",
                                 nb=xa.numel() + xs.numel() + c1.wf.numel() + cs.wf.numel() + 2 * qn1.numel()))
                else:
                    conv_plain(c1, d1, xa, qn1, q_n1)
                    conv_plain(cs, ds, xs, qns, q_ns)
        pending = Chain(k + "1", (b.n1, qn1, b.r1), None, None, None, c2.X_range, None)
        qn2 = buf(k + "qn2", shp, torch.int8)
        conv(c2, d2, pending, qn2, qd(b.n2.X_range, inner))
        Y = buf(k + "Y", shp, torch.float32)
        pending = Chain(k + "2", (b.n2, qn2, b.r2), (b.ns, qns, b.rs) if cs is not None else None, Y,
                        None if cs is not None else Xin, nxt.c1.X_range if nxt is not None else None,
                        nxt.cs.X_range if nxt is not None and nxt.cs is not None else None)
        Xin = Y
    pending.flush()  # the last block's end chain: the block output alone

    # ---- head: avg pool, Dense_q, logits (separate launches); compute_loss adds the softmax cross-entropy
    Nb, Hh, Wh, Ch = Xin.shape
    pooled = buf("pool", (Nb, Ch), torch.float32)
    hfwd = [L("lbt_avgpool_fwd", ptr(Xin), ptr(pooled), Nb, Hh * Wh, Ch)]
    dd = _lib.ConvDesc(Nb, 1, 1, d.in_units, d.units, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1)
    pq = buf("pq", (Nb, Ch), torch.int8)
    q_dx = qd(d.X_range, Ch)
    hfwd.append(L("lbt_dfxp_quantize", ptr(pooled), ptr(pq), OUT_I8, Nb, Ch, q_dx, None, 0))
    plan.logits = buf("logits", (Nb, d.units), torch.float32)
    hfwd.append(L("lbt_conv_fwd_generic", ptr(pq), 0, ptr(d.w_hwio), dd, q_dx, qd(d.W_range), ptr(plan.logits)))
    plan.loss = buf("loss", (1,), torch.float32)
    plan.dlogits = buf("dz", (Nb, d.units), torch.float32)  # lbt_softmax_xent writes it beside the loss
    hloss = [L("lbt_softmax_xent", ptr(plan.logits), ptr(plan._labels), Nb, d.units, ptr(plan.loss), ptr(plan.dlogits))]

    # ---- the prologue: this step's forward noise tables, every parameter quantiser and the input image
    plan._njobs = _dev_array(njobs, ctx.device)
    plan._wjobs = _dev_array(wjobs, ctx.device)
    plan._qjobs = _dev_array(qjobs, ctx.device)
    max_n = max(j.n for j in njobs)
    fwd.insert(0, L("lbt_step_prologue", ptr(plan._njobs), len(njobs), max_n, None, 0, ptr(plan._wjobs), len(wjobs),
                    max(j.Cout for j in wjobs), ptr(plan._qjobs), len(qjobs), ctypes.byref(plan._input_job), None, None,
                    0, k="step_prologue_kernel", nb=4 * sum(j.n for j in njobs) + 6 * X.numel()))
    if w4:  # the packed weight images need the quantised ones
        fwd.insert(1, L("lbt_pack_int4", ptr(plan._w8), ptr(plan._w4), plan._w8.numel(), k="pack_int4_kernel",
                        nb=plan._w8.numel() + plan._w4.numel()))
    plan._fwd, plan._hfwd, plan._hloss = fwd, hfwd, hloss

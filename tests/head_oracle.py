"""The classifier head (lbt_head_fwd_bwd + lbt_step_reduce's head block) in numpy (test helper, CPU only).

Composed from the oracle's pieces: ``AvgPoolQ`` (in-order fp32 sum), ``dfxp.quantize_int`` /
``overflow_counts``, the exact integer products of ``DenseQ`` with ``scale_int``, ``softmax_xent(norm=)``
and the ``NormQ`` / ``RescaleQ`` forward and backward arithmetic. Everything here is integer or in-order
fp32 arithmetic, so a kernel is compared with it bit for bit. The one transcendental step (``expf`` /
``logf``: dz and the loss terms) is not restated for the GPU tests: they feed ``backward`` with the
kernel's own dz (tests/test_head.py).

A quantiser is ``Q(bits, I, stochastic, noise)``: ``noise`` is the fp32 noise over the operand's
``shape[1:]`` (None for the nearest quantiser).
"""
import collections

import numpy as np

from oracle import dfxp
from oracle import nn as onn

F32 = np.float32
Q = collections.namedtuple("Q", "bits I stochastic noise")


def frac(q):
    return dfxp.frac_bits(q.bits, q.I)


def codes(x, q):
    with np.errstate(over="ignore", invalid="ignore"):
        u = None if not q.stochastic else np.asarray(q.noise, dtype=F32).reshape(np.asarray(x).shape[1:])
        return dfxp.quantize_int(x, q.bits, q.I, q.stochastic, u)


def counts(x, q):
    with np.errstate(over="ignore"):
        return dfxp.overflow_counts(x, q.bits, q.I)


def pool(x):
    """AvgPool_q over [N, HW, C]: the HW pixels added in order in fp32, times fl(1 / HW)."""
    N, HW, C = x.shape
    with np.errstate(over="ignore", invalid="ignore"):
        return onn.AvgPoolQ().forward(np.asarray(x, F32).reshape(N, HW, 1, C), None).reshape(N, C)


def forward(x, wq, qx, qw):
    """pooled, pq, logits and qx's counters."""
    pooled = pool(x)
    pq = codes(pooled, qx)
    acc = pq.astype(np.int64) @ np.asarray(wq).astype(np.int64)
    return dict(pooled=pooled, pq=pq, logits=onn.scale_int(acc, frac(qx) + frac(qw)), cx=counts(pooled, qx))


def softmax(logits, labels, norm=None):
    """(loss, dz) of oracle.nn.softmax_xent: the CPU tests' dz (the GPU tests take the kernel's)."""
    return onn.softmax_xent(np.asarray(logits, F32), np.asarray(labels), norm=norm)


def backward(fw, dz, wq, qx, qw, qg, HW, w=None, wd2=0.0):
    """Given dz [N, K]: gq, qg's counters, the integer sum_n pq^T gq, dW = fl(fl(S) 2^-(ex+eg)) + fl(wd2 w)
    (lbt_conv_wgrad_reduce's formula), the pooled gradient g = fl(S' 2^-(eg+ew)) fl(1/HW) and gx."""
    dz = np.asarray(dz, F32)
    gq = codes(dz, qg)
    dwi = fw["pq"].astype(np.int64).T @ gq.astype(np.int64)
    out = dict(gq=gq, cg=counts(dz, qg), dw_int=dwi)
    if w is not None:
        a = onn.scale_int(dwi, frac(qx) + frac(qg))
        out["dW"] = (a + (F32(wd2) * np.asarray(w, F32)).astype(F32)).astype(F32)
    s_dp = onn.scale_int(gq.astype(np.int64) @ np.asarray(wq).astype(np.int64).T, frac(qg) + frac(qw))
    g = (s_dp * F32(1.0 / HW)).astype(F32)
    out["g"] = g
    out["gx"] = np.broadcast_to(g[:, None, :], (g.shape[0], HW, g.shape[1])).copy()
    return out


def loss_from_terms(terms, norm):
    """loss[0] from the per-sample double terms in head_reduce's order: thread t adds rows t, t + 256, ...
    in order, then the tree s[t] += s[t + o], o = 128 .. 1; the total over norm, rounded to fp32."""
    terms = np.asarray(terms, np.float64)
    s = np.zeros(256, np.float64)
    for r in range(len(terms)):
        s[r % 256] = s[r % 256] + terms[r]
    o = 128
    while o:
        s[:o] = s[:o] + s[o:2 * o]
        o //= 2
    return F32(s[0] / float(norm)), int(np.rint(s[0] * 4294967296.0))


def pass_a(g, y_mask, R, qn, gamma_q, qrg, qng):
    """Pass A of the last block's output BatchNorm on the un-pooled gradient g[n][c] (every pixel of a
    sample gets it): ReLU mask y_mask > 0, the Rescale_q gradient quantiser (RescaleQ.backward: codes G2,
    sums G2 R and G2), times gamma_q, the Normalization_q gradient quantiser (NormQ.backward: codes G, sums G
    and G qn). y_mask / R / qn [N, HW, C]; noise over [HW, C]."""
    N, HW, C = y_mask.shape
    gfull = np.broadcast_to(np.asarray(g, F32)[:, None, :], (N, HW, C))
    gv = np.where(np.asarray(y_mask, F32) > 0, gfull, F32(0)).astype(F32)
    G2 = codes(gv, qrg)
    gh = (G2.astype(F32) * F32(2.0 ** -frac(qrg))).astype(F32)
    d = (gh * np.asarray(gamma_q, F32)).astype(F32)
    G = codes(d, qng)
    G2l, Gl = G2.reshape(-1, C).astype(np.int64), G.reshape(-1, C).astype(np.int64)
    Rl, ql = np.asarray(R).reshape(-1, C).astype(np.int64), np.asarray(qn).reshape(-1, C).astype(np.int64)
    sums = np.stack([(G2l * Rl).sum(0), G2l.sum(0), Gl.sum(0), (Gl * ql).sum(0)])
    return dict(gmask=gv, G2=G2, d=d, gout=G, sums=sums, crg=counts(gv, qrg), cng=counts(d, qng))


def moments(S1, S2, e, n, eps):
    """NormQ's batch moments from the exact integer sums: mu, var, sigma (fp32)."""
    s = 2.0 ** -e
    mean_d = np.asarray(S1, np.float64) * s / n
    var_d = np.asarray(S2, np.float64) * (s * s) / n - mean_d * mean_d
    mu, var = mean_d.astype(F32), var_d.astype(F32)
    return mu, var, np.sqrt((var + F32(eps)).astype(F32)).astype(F32)


def chain(q, e_n, gamma_q, beta_q, res, qr, eps=1e-5, momentum=0.999, one_minus=0.001, run_mean=None, run_var=None):
    """The end chain on int8 Normalization_q codes q [N, HW, C] (exponent e_n): NormQ.forward (moments of the
    whole batch), the Rescale_q quantiser qr, RescaleQ.forward, the residual add and ReLU. Returns y, the R
    codes, ms = [mu | sigma], the running statistics after ONE update and qr's counters."""
    N, HW, C = q.shape
    ql = np.asarray(q).reshape(-1, C).astype(np.int64)
    mu, var, sigma = moments(ql.sum(0), (ql * ql).sum(0), e_n, ql.shape[0], eps)
    xq = (np.asarray(q).astype(F32) * F32(2.0 ** -e_n)).astype(F32)
    xhat = ((xq - mu).astype(F32) / sigma).astype(F32)
    R = codes(xhat, qr)
    xr = (R.astype(F32) * F32(2.0 ** -frac(qr))).astype(F32)
    v = (((xr * np.asarray(gamma_q, F32)).astype(F32) + np.asarray(beta_q, F32)).astype(F32)
         + np.asarray(res, F32)).astype(F32)
    out = dict(y=np.where(v > 0, v, F32(0)).astype(F32), R=R, ms=np.concatenate([mu, sigma]), cr=counts(xhat, qr))
    if run_mean is not None:
        m, o = F32(momentum), F32(one_minus)
        out["run_mean"] = ((m * np.asarray(run_mean, F32)).astype(F32) + (o * mu).astype(F32)).astype(F32)
        out["run_var"] = ((m * np.asarray(run_var, F32)).astype(F32) + (o * var).astype(F32)).astype(F32)
    return out


# ------------------------------------------------------------------------------ wrong heads (teeth)
def wrong_pool_pairwise(x):
    """numpy's pairwise fp32 reduction instead of the in-order sum."""
    x = np.asarray(x, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.add.reduce(np.ascontiguousarray(x.transpose(0, 2, 1)), axis=-1, dtype=F32)
        return (s * F32(1.0 / x.shape[1])).astype(F32)


def wrong_mask_ge(g, y_mask):
    N, HW, C = y_mask.shape
    return np.where(np.asarray(y_mask, F32) >= 0, np.broadcast_to(np.asarray(g, F32)[:, None, :], (N, HW, C)),
                    F32(0)).astype(F32)


def wrong_counts_per_workgroup(c, S):
    """qx / qg counters added by each of a sample's S workgroups instead of the lead one."""
    return (c[0] * S, c[1] * S)


def wrong_reduce_pad(pq, gq, pad_pq, pad_gq):
    """A batch reduction whose pad mask lets sample N through (the record bytes pad_pq [C], pad_gq [K])."""
    return pq.astype(np.int64).T @ gq.astype(np.int64) + np.outer(pad_pq, pad_gq).astype(np.int64)

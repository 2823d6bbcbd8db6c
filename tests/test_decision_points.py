"""Every implementation of the quantiser's last steps at its decision points (tests/decision_points.py).

CPU part (unmarked): the crafted operands are non-vacuous on the oracle alone and four deliberately
wrong numpy quantisers each differ from the oracle on them. GPU part (``@pytest.mark.gpu``): the HIP
entry points reproduce the oracle's codes and overflow counters BIT-EXACTLY on the same operands.

Families: A a float given directly (quant1: lbt_dfxp_quantize, _many, the three weight quantisers,
lbt_dropout_quantize, lbt_grad_buffer_bwd); B the element chains (quant_w / quant_w2: lbt_bn_chain_fwd,
_bwd_a, _bwd_b, lbt_bn_bwd_a_wide, _masked, lbt_bn_bwd_b_wide_q); C the integer-accumulator epilogues
(lbt_conv_fwd_i8, lbt_conv_stem_fwd, lbt_conv_fwd_igemm_q on its three kernels, lbt_conv_dgrad_chain_i8,
lbt_conv_dgrad_igemm_bna); D the fused 3x3 kernels (lbt_conv_fwd_fused_i8, lbt_conv_bwd_fused_i8)
and the stage transitions lbt_conv_fwd2_fused_i8, lbt_conv_bwd2_fused_i8 (no add_src: grids and saturation
only, see _run_bwd2_fused). head.hip's quantisers: tests/test_head.py.
"""
import ctypes

import numpy as np
import pytest

import decision_points as DP
from oracle import dfxp as odfxp

SEED, STEP = 1234, 3
QNAME = "dp/X_range"
QID = odfxp.qid_of(QNAME)
INNER = 4096

# (bits, I) of the GPU cases and of the non-vacuity statement
WIDTHS = [(8, 2), (4, 1), (9, 2), (16, 2), (8, 7), (7, -24), (16, 15), (16, -15)]
CPU_WIDTHS = WIDTHS + [(8, -3), (2, -1)]


def _u(stoch, inner=INNER):
    return DP.noise(inner, stoch, SEED, QID, STEP)


def _sites(cls, bits, I, stoch, inner=INNER):
    return DP.sites(cls, bits, I, stoch, inner, SEED, QID, STEP)


# ------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("stoch", [True, False])
@pytest.mark.parametrize("bits,I", CPU_WIDTHS)
def test_rounding_sites_are_not_vacuous(bits, I, stoch):
    """At least 95 % of the rounding sites show two different oracle codes across their 7 rows (a
    condition on the sites, not a tolerance: a width that misses it needs a wider ulp span)."""
    x, ks = DP.rounding_sites(bits, I, stoch, INNER, SEED, QID, STEP)
    assert x.shape == (2 * DP.SPAN + 1, INNER)
    L = 1 << (bits - 1)
    lo, hi = (-L + 1, L - 1) if stoch else (-L, L - 2)
    if 2 * L <= INNER:
        assert set(ks.tolist()) == set(range(lo, hi + 1))
    else:
        assert set(range(lo, lo + 3)) | set(range(hi - 2, hi + 1)) <= set(ks.tolist())
        assert np.all(np.diff(ks) >= 0) and np.max(np.diff(ks)) <= (hi - lo) // (INNER - 7) + 1
    q = DP.oracle_codes(x, bits, I, stoch, _u(stoch))
    two = (q.min(0) != q.max(0)).mean()
    print("bits %d I %d %s: %.2f %% of %d sites change code within +-%d ulps"
          % (bits, I, "stochastic" if stoch else "nearest", 100 * two, INNER, DP.SPAN))
    assert two >= 0.95
    if not stoch:  # the middle row is an exact tie: half-even sends it to the even neighbour
        assert np.array_equal(q[DP.SPAN], np.clip(np.where(ks % 2 == 0, ks, ks + 1), -L, L - 1))


@pytest.mark.parametrize("bits,I", CPU_WIDTHS)
def test_threshold_classes_hold_counted_and_uncounted(bits, I):
    x = DP.threshold_sites(bits, I, INNER)
    f1, f2 = DP.oracle_element_flags(x, bits, I)
    for r, name in enumerate(DP.THRESHOLD_CLASSES):
        f = f1 if name in ("+L", "-L") else f2
        assert 0 < f[r].sum() < INNER, name
        # >= above, < below: the threshold itself counts on the positive side only
        assert f[r][1] == (1 if name[0] == "+" else 0)
        assert DP.oracle_row_counts(x, bits, I)[r] == (int(f1[r].sum()), int(f2[r].sum()))
    assert DP.oracle_counts(x, bits, I) == (int(f1.sum()), int(f2.sum()))


@pytest.mark.parametrize("bits,I", CPU_WIDTHS)
def test_clip_special_and_saturation_sites(bits, I):
    L = 1 << (bits - 1)
    u = _u(True)
    x = _sites("clip", bits, I, True)
    up = DP.find_round_up_to_L(bits, I, u)
    assert np.count_nonzero(~np.isnan(up)) > INNER // 8, "the noise admits too few round-up-to-L sites"
    q = DP.oracle_codes(x, bits, I, True, u)
    assert q.min() == -L and q.max() == L - 1
    hit = ~np.isnan(up)
    assert np.all(q[3][hit] == L - 1)  # fl(xm + u) == L there: only the clip keeps the code at L - 1
    for stoch in (True, False):
        s = _sites("saturation", bits, I, stoch)
        assert DP.oracle_counts(s, bits, I) == (s.size, s.size)
        qs = DP.oracle_codes(s, bits, I, stoch, _u(stoch))
        assert np.array_equal(qs, np.where(s > 0, L - 1, -L))
        sp = _sites("special", bits, I, stoch)
        qsp = DP.oracle_codes(sp, bits, I, stoch, _u(stoch))
        assert qsp.min() == -L and qsp.max() == L - 1 and np.all(qsp[np.isinf(sp)] == np.where(sp[np.isinf(sp)] > 0, L - 1, -L))


@pytest.mark.parametrize("stoch", [True, False])
@pytest.mark.parametrize("bits,I", CPU_WIDTHS)
def test_wrong_quantisers_differ_on_the_crafted_set(bits, I, stoch):
    """Teeth: half-away rounding, a symmetric |xm| >= T predicate, xm + u in exact arithmetic and a clip
    to L each disagree with the oracle somewhere on the crafted operands (rounding modes apart: half-away
    only exists for the nearest quantiser, the exact add only for the stochastic one)."""
    u = _u(stoch)
    diff = {name: [0, 0] for name in DP.WRONG}
    for cls in DP.ALL_CLASSES:
        x = _sites(cls, bits, I, stoch)
        ref = DP.oracle_codes(x, bits, I, stoch, u)
        cnt = DP.oracle_counts(x, bits, I)
        rq, rc = DP.right_quantiser(x, bits, I, stoch, u)
        assert np.array_equal(rq, ref) and rc == cnt
        for name, fn in DP.WRONG.items():
            wq, wc = fn(x, bits, I, stoch, u)
            diff[name][0] += int(np.count_nonzero(wq != ref))
            diff[name][1] += int(wc != cnt)
    print(bits, I, stoch, diff)
    assert diff["symmetric_counts"][1] > 0 and diff["clip_to_L"][0] > 0
    assert diff["half_away" if not stoch else "exact_add"][0] > 0


def test_u8off_rule():
    x = _sites("rounding", 9, 2, True)
    q = DP.oracle_codes(x, 9, 2, True, _u(True))
    assert q.min() < 0 and np.array_equal(DP.u8off(q), np.where(q < 0, 0, q)) and DP.u8off(q).max() == 255


# ------------------------------------------------------------------------------------------ GPU
import torch  # noqa: E402

from lbt_amd import _lib  # noqa: E402
from lbt_amd._lib import NSHARD, OUT_F32, OUT_I8, OUT_I16, OUT_U8OFF  # noqa: E402
from lbt_amd.dfxp import ops  # noqa: E402
from lbt_amd.runtime import DfxpContext  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda"
KIND_NAME = {OUT_I8: "I8", OUT_U8OFF: "U8OFF", OUT_I16: "I16", OUT_F32: "F32"}
# (bits, I, out_kind): the widths of the issue and the two ends of the exponent domain (e = 0, e = 30)
QCASES = [(8, 2, OUT_I8), (4, 1, OUT_I8), (9, 2, OUT_U8OFF), (16, 2, OUT_I16), (16, 2, OUT_F32),
          (8, 7, OUT_I8), (7, -24, OUT_I8), (16, 15, OUT_I16), (16, -15, OUT_I16)]
QIDS = ["b%d_I%d_%s" % (b, i, KIND_NAME[k]) for b, i, k in QCASES]
# rounding x noise source: nearest, stochastic with inline Philox, stochastic with the per-step noise table
MODES = [(False, False), (True, False), (True, True)]
MODE_IDS = ["nearest", "philox", "table"]


class Quant:
    """One quantiser of a fresh context at step STEP, with the descriptor the case asks for."""

    def __init__(self, bits, I, stoch, table=False, inner=INNER, name=QNAME):
        self.ctx = DfxpContext(seed=SEED, capacity=8, sums_capacity=64)
        self.ctx.step.fill_(STEP)
        self.bits, self.I, self.stoch, self.inner = bits, I, stoch, inner
        self.q = self.ctx.quantizer(name, bits, I, stochastic=stoch)
        self.desc = self.ctx.noise_table_desc(self.q, inner) if table else self.q.desc
        self.u = DP.noise(inner, stoch, SEED, odfxp.qid_of(name), STEP)

    def take_counts(self):
        c = tuple(self.ctx.counts_view()[self.q.slot].sum(0).cpu().tolist())
        self.ctx.counts.zero_()
        return c

    def sites(self, cls):
        return DP.sites(cls, self.bits, self.I, self.stoch, self.inner, SEED, self.q.qid, STEP).copy()  # writable


def decode(t, kind):
    a = t.cpu().numpy()
    if kind == OUT_U8OFF:
        return a.astype(np.int32) + 128
    return a if kind == OUT_F32 else a.astype(np.int32)


def expected_out(codes, kind, bits, I):
    if kind == OUT_U8OFF:
        return DP.u8off(codes)
    return odfxp.dequant(codes, odfxp.frac_bits(bits, I)) if kind == OUT_F32 else codes


def assert_same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    assert len(bad) == 0, "%s: %d of %d differ, first at %s: got %r, oracle %r" % (
        what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])])


def check_float_entry(Q, kind, run, classes=DP.ALL_CLASSES, operand=None, row_calls=True):
    """run(x [rows, inner] device fp32) -> output tensor in `kind`; the codes and the overflow counters must
    be the oracle's on every site class. operand: what the entry point does to x before its quantiser.
    The threshold class is also called one row (= one threshold class) at a time, so that a per-tensor
    counter identifies a wrong predicate."""
    for cls in classes:
        x = Q.sites(cls)
        xo = x if operand is None else operand(x)
        for what, rs in site_blocks(cls, x, row_calls):
            ref = DP.oracle_codes(xo[rs], Q.bits, Q.I, Q.stoch, Q.u)
            got = decode(run(torch.from_numpy(x[rs]).to(DEV)), kind)
            assert_same(got.reshape(ref.shape), expected_out(ref, kind, Q.bits, Q.I), what + " codes")
            assert Q.take_counts() == DP.oracle_counts(xo[rs], Q.bits, Q.I), what + " counters"
        if cls == "saturation" and operand is None:
            assert DP.oracle_counts(x, Q.bits, Q.I) == (x.size, x.size)


def channel_sums(chsum, C):
    s = chsum.view(NSHARD, 2 * C).sum(0).cpu().numpy()
    chsum.zero_()
    return s[:C], s[C:]


# ---- A. float operand given directly (quant1)
@gpu
@pytest.mark.parametrize("inner,C", [(4096, 16), (4096, 128), (4095, 15)], ids=["vec_C16", "vec_C128", "ragged"])
@pytest.mark.parametrize("stoch,table", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("bits,I,kind", QCASES, ids=QIDS)
def test_quantize(bits, I, kind, stoch, table, inner, C):
    """lbt_dfxp_quantize: the vector path (inner 4096) and the generic one (inner 4095), without and with
    channel sums; S1 = sum q and S2 = sum q^2 of the oracle's codes (lbt_dfxp.h), in int64."""
    Q = Quant(bits, I, stoch, table, inner)
    chsum = ops.new_sums(C, 2, DEV)

    def run(x, cs=None):
        out = torch.empty(x.shape, dtype=ops.out_dtype(kind), device=DEV)
        _lib.call("lbt_dfxp_quantize", _lib.ptr(x), _lib.ptr(out), kind, x.shape[0], x.shape[1], Q.desc,
                  _lib.ptr(cs), C if cs is not None else 0, _lib.stream())
        return out

    if C != 128:
        check_float_entry(Q, kind, run)
    for cls in DP.ALL_CLASSES:
        x = Q.sites(cls)
        ref = DP.oracle_codes(x, bits, I, stoch, Q.u)
        got = decode(run(torch.from_numpy(x).to(DEV), chsum), kind)
        assert_same(got, expected_out(ref, kind, bits, I), cls + " codes (with chsum)")
        assert Q.take_counts() == DP.oracle_counts(x, bits, I), cls
        s1, s2 = channel_sums(chsum, C)
        r = ref.reshape(-1, C).astype(np.int64)
        assert_same(s1, r.sum(0), cls + " S1")
        assert_same(s2, (r * r).sum(0), cls + " S2")


@gpu
@pytest.mark.parametrize("stoch,table", MODES, ids=MODE_IDS)
def test_quantize_many(stoch, table):
    """lbt_dfxp_quantize_many: every width as one job of a single launch per site class."""
    Qs = [Quant(b, i, stoch, table, name="dp%d/X_range" % n) for n, (b, i, _) in enumerate(QCASES)]
    for cls in DP.ALL_CLASSES:
        xs = [torch.from_numpy(Q.sites(cls)).to(DEV) for Q in Qs]
        outs = [torch.empty(x.shape, dtype=ops.out_dtype(k), device=DEV) for x, (_, _, k) in zip(xs, QCASES)]
        jobs = [_lib.QJob(x.data_ptr(), o.data_ptr(), k, x.numel(), x.shape[1], Q.desc)
                for x, o, Q, (_, _, k) in zip(xs, outs, Qs, QCASES)]
        buf = torch.frombuffer(bytearray(bytes((_lib.QJob * len(jobs))(*jobs))), dtype=torch.uint8).to(DEV)
        ops.quantize_many(buf, len(jobs))
        for x, o, Q, (b, i, k) in zip(xs, outs, Qs, QCASES):
            xn = x.cpu().numpy()
            ref = DP.oracle_codes(xn, b, i, stoch, Q.u)
            assert_same(decode(o, k), expected_out(ref, k, b, i), "%s bits %d I %d codes" % (cls, b, i))
            assert Q.take_counts() == DP.oracle_counts(xn, b, i), (cls, b, i)


WCASES = [(8, 2), (4, 1), (8, 7), (7, -24)]  # weight codes are int8: bits <= 8


@gpu
@pytest.mark.parametrize("entry", ["weight", "weights", "weights_flat"])
@pytest.mark.parametrize("stoch,table", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("bits,I", WCASES)
def test_quantize_weight(bits, I, stoch, table, entry):
    """lbt_dfxp_quantize_weight / _weights / _weights_flat on W [rows, 1, 64, 64] (noise over shape[1:] =
    4096 columns): the codes in w_hwio, then the packed images by test_weight_packing's method."""
    Cin = Cout = 64
    Q = Quant(bits, I, stoch, table, Cin * Cout, name="dp/W_range")
    for cls in DP.ALL_CLASSES:
        x = Q.sites(cls)
        KH, KW = x.shape[0], 1
        K = KH * KW * Cin
        ksf, ksd = ops.packed_slices(KH, KW, Cin), ops.packed_slices(KH, KW, Cout)
        w = torch.from_numpy(x).to(DEV)
        hwio = torch.zeros((KH, KW, Cin, Cout), dtype=torch.int8, device=DEV)
        wf = torch.zeros((Cout, ksf * 16), dtype=torch.int8, device=DEV)
        wd = torch.zeros((Cin, ksd * 16), dtype=torch.int8, device=DEV)
        cs = torch.zeros(Cout, dtype=torch.int32, device=DEV) if entry != "weights_flat" else None
        if entry == "weight":
            _lib.call("lbt_dfxp_quantize_weight", _lib.ptr(w), KH, KW, Cin, Cout, Q.desc, _lib.ptr(hwio), _lib.ptr(wf),
                      ksf, _lib.ptr(wd), ksd, _lib.ptr(cs), _lib.stream())
        else:
            job = _lib.WJob(w.data_ptr(), KH, KW, Cin, Cout, Q.desc, hwio.data_ptr(), wf.data_ptr(), ksf,
                            wd.data_ptr(), ksd, cs.data_ptr() if cs is not None else None)
            buf = torch.frombuffer(bytearray(bytes((_lib.WJob * 1)(job))), dtype=torch.uint8).to(DEV)
            if entry == "weights":
                _lib.call("lbt_dfxp_quantize_weights", _lib.ptr(buf), 1, Cout, _lib.stream())
            else:
                nb = _lib.load().lbt_flat_weight_blocks(w.numel())
                starts = torch.tensor([0, nb], dtype=torch.int32, device=DEV)
                ops.quantize_weights_flat(buf, starts, 1, nb)
        ref = DP.oracle_codes(x, bits, I, stoch, Q.u)
        assert_same(hwio.cpu().numpy().reshape(ref.shape), ref, cls + " w_hwio")
        assert Q.take_counts() == DP.oracle_counts(x, bits, I), cls
        r4 = ref.reshape(KH, KW, Cin, Cout)
        assert_same(wf.cpu().numpy()[:, :K], r4.reshape(K, Cout).T, cls + " wf")
        assert_same(wd.cpu().numpy()[:, :KH * KW * Cout], r4.transpose(2, 0, 1, 3).reshape(Cin, KH * KW * Cout),
                    cls + " wd")
        if cs is not None:
            assert_same(cs.cpu().numpy(), r4.reshape(K, Cout).sum(0), cls + " colsum")


DCASES = [c for c in QCASES if c[2] != OUT_F32]  # lbt_dropout_quantize writes integer codes only


@gpu
@pytest.mark.parametrize("inner", [4096, 4095], ids=["vec", "ragged"])
@pytest.mark.parametrize("stoch,table", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("bits,I,kind", DCASES, ids=[q for q, c in zip(QIDS, QCASES) if c[2] != OUT_F32])
def test_dropout_quantize(bits, I, kind, stoch, table, inner):
    """lbt_dropout_quantize through its ReLU variant at keep = 1 (the largest legal keep: the mask is all
    ones and x / 1 == x), so the quantiser's operand is exactly max(x, 0) of the crafted x."""
    Q = Quant(bits, I, stoch, table, inner)

    def run(x):
        out = torch.empty(x.shape, dtype=ops.out_dtype(kind), device=DEV)
        _lib.call("lbt_dropout_quantize", _lib.ptr(x), _lib.ptr(out), kind, x.shape[0], x.shape[1], 1.0, 77, 1,
                  Q.desc, _lib.stream())
        return out

    check_float_entry(Q, kind, run, operand=relu_np)


@gpu
@pytest.mark.parametrize("stoch,table", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("bits,I", WIDTHS)
def test_grad_buffer_bwd(bits, I, stoch, table):
    """lbt_grad_buffer_bwd with a zero buffer: total = g + 0 is the crafted g (a -0 becomes +0, which
    quantises alike); gq is the fake-quantised value, the new buffer g - gq."""
    Q = Quant(bits, I, stoch, table)

    def run(x):
        buf = torch.zeros_like(x)
        gq = ops.grad_buffer_bwd(x, buf, Q.desc, x.shape[1])
        fin = torch.isfinite(x)
        assert torch.equal(buf[fin], (x - gq)[fin])
        return gq

    check_float_entry(Q, OUT_F32, run)


# ---- B. chain kernels given a float (quant_w, quant_w2)
C_CHAIN = 64  # channels of the chain cases: inner 4096 = 64 positions x 64 channels


def site_blocks(cls, x, row_calls=True):
    """The whole class, and for the threshold class each row (= one threshold class) as a rows = 1 call."""
    blocks = [(cls, slice(0, len(x)))]
    if cls == "threshold" and row_calls:
        blocks += [("threshold %s" % DP.THRESHOLD_CLASSES[r], slice(r, r + 1)) for r in range(len(x))]
    return blocks


def expect(Q, operand, got, kind, what):
    """got (device tensor in `kind`) and Q's counters are the oracle's for this operand; returns the codes."""
    ref = DP.oracle_codes(operand, Q.bits, Q.I, Q.stoch, Q.u)
    assert_same(decode(got, kind).reshape(ref.shape), expected_out(ref, kind, Q.bits, Q.I), what + " codes")
    assert Q.take_counts() == DP.oracle_counts(operand, Q.bits, Q.I), what + " counters"
    return ref


def relu_np(x):
    return np.where(x > 0, x, np.float32(0)).astype(np.float32)


def shard_sums(t, per_shard):
    s = t.view(NSHARD, per_shard).sum(0).cpu().numpy()
    t.zero_()
    return s


def unit_gb(C):
    return torch.cat([torch.ones(C), torch.zeros(C)]).to(DEV)  # gamma_q = 1, beta_q = 0


@gpu
@pytest.mark.parametrize("with_y", [True, False], ids=["y", "no_y"])
@pytest.mark.parametrize("stoch,table", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("bits,I", WCASES)
def test_chain_fwd_into_qr(bits, I, stoch, table, with_y):
    """lbt_bn_chain_fwd with xin (nrm.q == NULL) into the Rescale_q quantiser qr; gamma_q = 1, beta_q = 0
    make y the dequantised code. Stochastic with y is the compiled variant (floor_i), the rest the run-time
    one (floorf / rintf). The R codes are int8, so bits <= 8."""
    Q = Quant(bits, I, stoch, table)
    gb = unit_gb(C_CHAIN)
    for cls in DP.ALL_CLASSES:
        xs = Q.sites(cls)
        for what, rs in site_blocks(cls, xs):
            x = torch.from_numpy(xs[rs]).to(DEV)
            rout = torch.empty(x.shape, dtype=torch.int8, device=DEV)
            y = torch.empty_like(x) if with_y else None
            a = _lib.ChainFwd()
            a.b1.xin, a.b1.qr, a.b1.rout, a.b1.gb = x.data_ptr(), Q.desc, rout.data_ptr(), gb.data_ptr()
            a.y = y.data_ptr() if with_y else None
            a.rows, a.inner, a.C = x.shape[0], x.shape[1], C_CHAIN
            ops.chain_fwd(a)
            ref = expect(Q, xs[rs], rout, OUT_I8, what)
            if with_y:
                assert_same(y.cpu().numpy(), odfxp.dequant(ref, odfxp.frac_bits(bits, I)), what + " y")


@gpu
@pytest.mark.parametrize("relu", [0, 1], ids=["linear", "relu"])
@pytest.mark.parametrize("stoch,table", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("bits,I", WCASES)
def test_chain_fwd_into_qo(bits, I, stoch, table, relu):
    """lbt_bn_chain_fwd with xin and qr.bits == 0: v = xin (or max(xin, 0)) into qo1 (int8 codes) and qo2
    (9-bit codes in the offset encoding: max(code, 0)). The compiled variants of this chain all take int8
    Normalization_q codes, so a float can only reach the run-time variant here."""
    Q1 = Quant(bits, I, stoch, table, name="dp/o1_range")
    Q2 = Quant(9, 2, stoch, table, name="dp/o2_range")
    for cls in DP.ALL_CLASSES:
        for Qs in (Q1, Q2):  # each quantiser's own sites (they depend on its noise), both outputs checked
            xs = Qs.sites(cls)
            for what, rs in site_blocks(cls, xs):
                x = torch.from_numpy(xs[rs]).to(DEV)
                o1 = torch.empty(x.shape, dtype=torch.int8, device=DEV)
                o2 = torch.empty(x.shape, dtype=torch.int8, device=DEV)
                a = _lib.ChainFwd()
                a.b1.xin, a.relu = x.data_ptr(), relu
                a.o1, a.o1_kind, a.qo1 = o1.data_ptr(), OUT_I8, Q1.desc
                a.o2, a.o2_kind, a.qo2 = o2.data_ptr(), OUT_U8OFF, Q2.desc
                a.rows, a.inner, a.C = x.shape[0], x.shape[1], C_CHAIN
                ops.chain_fwd(a)
                v = relu_np(xs[rs]) if relu else xs[rs]
                expect(Q1, v, o1, OUT_I8, what + " o1")
                expect(Q2, v, o2, OUT_U8OFF, what + " o2")


@gpu
@pytest.mark.parametrize("stoch,table", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("bits,I", WIDTHS)
def test_chain_bwd_a_into_qrg(bits, I, stoch, table):
    """lbt_bn_chain_bwd_a, no mask: g into the Rescale_q gradient quantiser qrg, qng off; with gamma_q = 1
    dout is the dequantised G2 code, and sums[C:2C) its per-channel sum (R codes = 1: sums[0:C) too)."""
    Q = Quant(bits, I, stoch, table)
    C = C_CHAIN
    gb = unit_gb(C)
    sums = ops.new_sums(C, 4, DEV)
    for cls in DP.ALL_CLASSES:
        xs = Q.sites(cls)
        for what, rs in site_blocks(cls, xs):
            x = torch.from_numpy(xs[rs]).to(DEV)
            R = torch.ones(x.shape, dtype=torch.int8, device=DEV)
            dout = torch.empty_like(x)
            a = _lib.ChainBwdA()
            a.g = x.data_ptr()
            a.b1 = _lib.BwdBranch(Q.desc, R.data_ptr(), _lib.NO_Q, gb.data_ptr(), _lib.NO_Q, None, None,
                                  dout.data_ptr(), sums.data_ptr())
            a.rows, a.inner, a.C = x.shape[0], x.shape[1], C
            ops.chain_bwd_a(a)
            ref = expect(Q, xs[rs], dout, OUT_F32, what)
            s = shard_sums(sums, 4 * C)
            per = ref.reshape(-1, C).astype(np.int64).sum(0)
            assert_same(s[:C], per, what + " S(G2 R)")
            assert_same(s[C:2 * C], per, what + " S(G2)")


@gpu
@pytest.mark.parametrize("stoch,table", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("bits,I", WCASES)
def test_chain_bwd_a_into_qng(bits, I, stoch, table):
    """lbt_bn_chain_bwd_a, no mask, qrg.bits == 0: g into the Normalization_q gradient quantiser qng (int8 G
    codes); sums[2C:3C) = S(G), sums[3C:4C) = S(G qn) with qn codes = 1."""
    Q = Quant(bits, I, stoch, table)
    C = C_CHAIN
    sums = ops.new_sums(C, 4, DEV)
    for cls in DP.ALL_CLASSES:
        xs = Q.sites(cls)
        for what, rs in site_blocks(cls, xs):
            x = torch.from_numpy(xs[rs]).to(DEV)
            qn = torch.ones(x.shape, dtype=torch.int8, device=DEV)
            G = torch.empty(x.shape, dtype=torch.int8, device=DEV)
            a = _lib.ChainBwdA()
            a.g = x.data_ptr()
            a.b1 = _lib.BwdBranch(_lib.NO_Q, None, _lib.NO_Q, None, Q.desc, qn.data_ptr(), G.data_ptr(), None,
                                  sums.data_ptr())
            a.rows, a.inner, a.C = x.shape[0], x.shape[1], C
            ops.chain_bwd_a(a)
            ref = expect(Q, xs[rs], G, OUT_I8, what)
            s = shard_sums(sums, 4 * C)
            per = ref.reshape(-1, C).astype(np.int64).sum(0)
            assert_same(s[2 * C:3 * C], per, what + " S(G)")
            assert_same(s[3 * C:], per, what + " S(G qn)")


@gpu
@pytest.mark.parametrize("table", [False, True], ids=["philox", "table"])
@pytest.mark.parametrize("bits,I", WCASES)
def test_chain_bwd_a_compiled_variant(bits, I, table):
    """The compiled pass A (both quantisers stochastic, y_mask, int8 G codes): y_mask = 1 keeps g, so qrg sees
    the crafted float; with gamma_q = 1 qng's operand is the dequantised G2 code -- analytically known."""
    Q = Quant(bits, I, True, table)
    Qn = Quant(8, 2, True, table, name="dp/ng_range")
    C = C_CHAIN
    gb = unit_gb(C)
    sums = ops.new_sums(C, 4, DEV)
    for cls in DP.ALL_CLASSES:
        xs = Q.sites(cls)
        x = torch.from_numpy(xs).to(DEV)
        ones8 = torch.ones(x.shape, dtype=torch.int8, device=DEV)
        ym = torch.ones_like(x)
        G = torch.empty(x.shape, dtype=torch.int8, device=DEV)
        a = _lib.ChainBwdA()
        a.g, a.y_mask = x.data_ptr(), ym.data_ptr()
        a.b1 = _lib.BwdBranch(Q.desc, ones8.data_ptr(), _lib.NO_Q, gb.data_ptr(), Qn.desc, ones8.data_ptr(),
                              G.data_ptr(), None, sums.data_ptr())
        a.rows, a.inner, a.C = x.shape[0], x.shape[1], C
        ops.chain_bwd_a(a)
        g2 = DP.oracle_codes(xs, bits, I, True, Q.u)
        assert Q.take_counts() == DP.oracle_counts(xs, bits, I), cls + " qrg counters"
        d = odfxp.dequant(g2, odfxp.frac_bits(bits, I))
        ref = expect(Qn, d, G, OUT_I8, cls + " qng")
        s = shard_sums(sums, 4 * C)
        assert_same(s[C:2 * C], g2.reshape(-1, C).astype(np.int64).sum(0), cls + " S(G2)")
        assert_same(s[2 * C:3 * C], ref.reshape(-1, C).astype(np.int64).sum(0), cls + " S(G)")


def grid_codes(bits, rows, inner, int8_operand=True):
    """Integer-grid codes [rows, inner]: every accumulator value of DP.integer_grid in every row, shifted
    from row to row so that a column sees different values."""
    g = DP.integer_grid(bits, int8_operand)
    r, c = np.indices((rows, inner))
    return g[(c + 37 * r) % len(g)]


# (qo bits, s): xm = G * 2^-s. 4 bits: the grid spans [-2L-2, 2L+2]; 8 bits: the int8 range of the G codes
GRID_CASES = [(4, 0), (4, 1), (8, 0), (8, 1)]


def _bwd_b_operands(qbits, s, rows, inner, C, int8_G, stoch, table):
    """Pass B with ms = [0 | 1] and zero sums: dx = G * 2^-e_g exactly, so qo's operand is the integer grid
    times 2^-s when e_o = e_g - s."""
    e_g = 5
    Qg = Quant(8 if int8_G else 16, (8 if int8_G else 16) - 1 - e_g, True, name="dp/ng_range")
    Qo = Quant(qbits, qbits - 1 - (e_g - s), stoch, table, inner, name="dp/o_range")
    Qx = Quant(8, 2, True, name="dp/nx_range")
    Gn = grid_codes(qbits, rows, inner, int8_G)
    dx = (Gn.astype(np.float32) * np.float32(2.0 ** -e_g)).astype(np.float32)
    ms = torch.cat([torch.zeros(C), torch.ones(C)]).to(DEV)
    sums = ops.new_sums(C, 4, DEV)
    return Qg, Qo, Qx, Gn, dx, ms, sums


@gpu
@pytest.mark.parametrize("stoch,table", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("qbits,s", GRID_CASES)
def test_chain_bwd_b_integer_grid(qbits, s, stoch, table):
    """lbt_bn_chain_bwd_b into qo on an integer grid (no float can be injected: dx is computed from codes):
    +-L, +-L/2, L-1 and -L exactly, and with s = 1 a tie on every odd G for the nearest quantiser."""
    rows, inner, C = 7, INNER, C_CHAIN
    Qg, Qo, Qx, Gn, dx, ms, sums = _bwd_b_operands(qbits, s, rows, inner, C, True, stoch, table)
    G = torch.from_numpy(Gn.astype(np.int8)).to(DEV)
    qn = torch.zeros((rows, inner), dtype=torch.int8, device=DEV)
    gq = torch.empty((rows, inner), dtype=torch.int8, device=DEV)
    gcol = ops.new_sums(C, 2, DEV)
    b = _lib.ChainBwdB(G.data_ptr(), Qg.desc, qn.data_ptr(), Qx.desc, ms.data_ptr(), sums.data_ptr(), rows * inner // C,
                       None, gq.data_ptr(), Qo.desc, gcol.data_ptr(), rows, inner, C)
    ops.chain_bwd_b(b)
    ref = expect(Qo, dx, gq, OUT_I8, "grid")
    s12 = shard_sums(gcol, 2 * C)
    r = ref.reshape(-1, C).astype(np.int64)
    assert_same(s12[:C], r.sum(0), "S1")
    assert_same(s12[C:], (r * r).sum(0), "S2")


WIDE_C = 64  # the wide kernels see [rows = samples * hw][C] with hw = inner / C positions per sample


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("stoch,table", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("bits,I", WIDTHS)
def test_bn_bwd_a_wide(bits, I, stoch, table, masked):
    """lbt_bn_bwd_a_wide / _masked (y_mask = 1): g into qrg (gamma_q = 1, dout the dequantised code), then with
    qrg.bits == 0 into qng (int16 G codes); one noise period per sample of 4096 elements."""
    Q = Quant(bits, I, stoch, table)
    C, hw = WIDE_C, INNER // WIDE_C
    gb = unit_gb(C)
    sums = ops.new_sums(C, 4, DEV)
    for cls in DP.ALL_CLASSES:
        xs = Q.sites(cls)
        for what, rs in site_blocks(cls, xs):
            x = torch.from_numpy(xs[rs]).to(DEV)
            n = x.shape[0]
            ones8 = torch.ones(x.shape, dtype=torch.int8, device=DEV)
            ym = torch.ones_like(x) if masked else None
            per = None
            for part in ("qrg", "qng"):
                dout = torch.empty_like(x) if part == "qrg" else None
                G = torch.empty(x.shape, dtype=torch.int16, device=DEV) if part == "qng" else None
                qrg, qng = (Q.desc, _lib.NO_Q) if part == "qrg" else (_lib.NO_Q, Q.desc)
                if masked:
                    _lib.call("lbt_bn_bwd_a_wide_masked", _lib.ptr(x), None, _lib.ptr(ym), None, 0, _lib.NO_Q,
                              _lib.ptr(gb), None, qrg, _lib.ptr(ones8), qng, _lib.ptr(ones8), _lib.ptr(G),
                              _lib.ptr(dout), _lib.ptr(sums), n * hw, INNER, C, _lib.stream())
                else:
                    ops.bn_bwd_a_wide(x, qrg, ones8, gb, qng, ones8, G, dout, sums, n * hw, INNER, C)
                ref = expect(Q, xs[rs], dout if part == "qrg" else G, OUT_F32 if part == "qrg" else OUT_I16,
                             "%s %s" % (what, part))
                s4 = shard_sums(sums, 4 * C)
                per = ref.reshape(-1, C).astype(np.int64).sum(0)
                lo = 0 if part == "qrg" else 2 * C
                assert_same(s4[lo:lo + C], per, what + " first sum of " + part)
                assert_same(s4[lo + C:lo + 2 * C], per, what + " second sum of " + part)


@gpu
@pytest.mark.parametrize("stoch,table", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("qbits,s", GRID_CASES + [(9, 0), (9, 1)])
def test_bn_bwd_b_wide_q_integer_grid(qbits, s, stoch, table):
    """lbt_bn_bwd_b_wide_q into qo on an integer grid of int16 G codes: the whole [-2L-2, 2L+2] at every
    width here (the codes are 16-bit), by the construction of test_chain_bwd_b_integer_grid."""
    rows, inner, C = 7, INNER, WIDE_C
    Qg, Qo, Qx, Gn, dx, ms, sums = _bwd_b_operands(qbits, s, rows, inner, C, False, stoch, table)
    G = torch.from_numpy(Gn.astype(np.int16)).to(DEV)
    qn = torch.zeros((rows, inner), dtype=torch.int8, device=DEV)
    gq = torch.empty((rows, inner), dtype=torch.int16, device=DEV)
    ops.bn_bwd_b_wide_q(G, Qg.desc, qn, Qx.desc, ms, sums, rows * inner // C, gq, Qo.desc, rows * (inner // C), inner, C)
    expect(Qo, dx, gq, OUT_I16, "grid")


# ---- C. integer-accumulator epilogues: integer grids through an identity conv
def _grid_quants(qbits, s, stoch, table, inner, e_x=5):
    """qx / qw with e_x + e_w = e_x (identity weight codes of value 1 at e_w = 0) and the output quantiser at
    e_out = e_x - s, so that its operand is acc * 2^-s. A stochastic epilogue reads the noise table."""
    Qx = Quant(9, 9 - 1 - e_x, True, name="dp/cx_range")
    Qw = Quant(8, 7, True, name="dp/cw_range")
    Qo = Quant(qbits, qbits - 1 - (e_x - s), stoch, table, inner, name="dp/co_range")
    return Qx, Qw, Qo


EPI_MODES = [(False, False), (True, True)]  # the quantising epilogues take nearest rounding or a noise table


@gpu
@pytest.mark.parametrize("stoch,table", EPI_MODES, ids=["nearest", "table"])
@pytest.mark.parametrize("qbits,s", GRID_CASES)
def test_conv_fwd_i8_epilogue_integer_grid(qbits, s, stoch, table):
    """lbt_conv_fwd_i8 with qout (conv_epilogue.h epi_quant): a 1x1 identity conv on int8 operand codes makes
    the accumulator the operand code, so qout sees acc * 2^-s; codes, counters and the channel sums."""
    N, H, C = 7, 16, 16
    inner = H * H * C
    Qx, Qw, Qo = _grid_quants(qbits, s, stoch, table, inner)
    acc = grid_codes(qbits, N, inner, True)
    xq = torch.from_numpy(acc.astype(np.int8).reshape(N, H, H, C)).to(DEV)
    ksf = ops.packed_slices(1, 1, C)
    wf = torch.zeros((C, ksf * 16), dtype=torch.int8, device=DEV)
    wf[:, :C] = torch.eye(C, dtype=torch.int8, device=DEV)
    d = ops.conv_desc(N, H, H, C, C, 1, 1, 1, 1, "SAME")
    yq = torch.empty((N, H, H, C), dtype=torch.int8, device=DEV)
    chsum = ops.new_sums(C, 2, DEV)
    ops.conv_fwd_i8(xq, 0, wf, ksf, None, d, Qx.desc, Qw.desc, yq=yq, qout=Qo.desc, ychsum=chsum)
    y = (acc.astype(np.float32) * np.float32(2.0 ** -5)).astype(np.float32)
    ref = expect(Qo, y, yq, OUT_I8, "grid")
    s1, s2 = channel_sums(chsum, C)
    r = ref.reshape(-1, C).astype(np.int64)
    assert_same(s1, r.sum(0), "S1")
    assert_same(s2, (r * r).sum(0), "S2")
    wide = Quant(9, 2, False, name="dp/wide_range")
    with pytest.raises(_lib.LbtError):  # int8 output codes: a wider quantiser is refused, not truncated
        ops.conv_fwd_i8(xq, 0, wf, ksf, None, d, Qx.desc, Qw.desc, yq=yq, qout=wide.desc, ychsum=chsum)


@gpu
@pytest.mark.parametrize("stoch,table", EPI_MODES, ids=["nearest", "table"])
@pytest.mark.parametrize("qbits,s", GRID_CASES)
def test_conv_stem_fwd_epilogue_integer_grid(qbits, s, stoch, table):
    """lbt_conv_stem_fwd with qout: 3x3 / SAME conv of int16 image codes [N, 16, 16, 3] whose centre tap
    copies input channel co % 3 to output channel co, so acc is the operand code: the whole [-2L-2, 2L+2]."""
    N, H, Cin, Cout = 7, 16, 3, 16
    inner = H * H * Cout
    Qx, Qw, Qo = _grid_quants(qbits, s, stoch, table, inner)
    xc = grid_codes(qbits, N, H * H * Cin, False).reshape(N, H, H, Cin)
    x = torch.from_numpy(xc.astype(np.int16)).to(DEV)
    w = np.zeros((3, 3, Cin, Cout), dtype=np.int8)
    for co in range(Cout):
        w[1, 1, co % Cin, co] = 1
    d = ops.conv_desc(N, H, H, Cin, Cout, 3, 3, 1, 1, "SAME")
    yq = torch.empty((N, H, H, Cout), dtype=torch.int8, device=DEV)
    chsum = ops.new_sums(Cout, 2, DEV)
    ops.conv_stem_fwd(x, torch.from_numpy(w).to(DEV), d, Qx.desc, Qw.desc, yq=yq, qout=Qo.desc, ychsum=chsum)
    acc = xc[..., np.arange(Cout) % Cin]
    y = (acc.astype(np.float32) * np.float32(2.0 ** -5)).astype(np.float32).reshape(N, inner)
    ref = expect(Qo, y, yq, OUT_I8, "grid")
    s1, s2 = channel_sums(chsum, Cout)
    rr = ref.reshape(-1, Cout).astype(np.int64)
    assert_same(s1, rr.sum(0), "S1")
    assert_same(s2, (rr * rr).sum(0), "S2")


# ---- D. the fused 3x3 forward (qfloor2, floor_i(fminf), ov_count2 / ov_count2_pos, packed lane counters)
E_N = 5  # exponent of the Normalization_q input codes of the fused cases


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _run_fwd_fused(N, H, C, qcodes, e_r, gamma, e_o1, e_out, res=None):
    """One training-mode lbt_conv_fwd_fused_i8 launch on [N, H, 512 / C, C] whose every quantiser operand is
    known analytically, checked against the oracle:

      * the channel sums are chosen as S1 = 0, S2 = n 4^E_N, eps = 0, so that by the moment formula of
        lbt_dfxp.h (mu = S1 s / n, var = S2 s^2 / n - mu^2, sigma = sqrtf(var + eps)) mu = 0 and sigma = 1:
        the Rescale_q quantiser sees q 2^-E_N (an integer grid);
      * gamma is a power of two or zero and beta = 0: v = (R 2^-e_r) gamma (+ res), ReLU, into the 9-bit X
        quantiser (offset encoding);
      * the conv copies through its centre tap (weight code 1 at e_w = 0): the accumulator is the X code, and
        the output quantiser sees X 2^-e_o1.

    Halo pixels are recomputed by the neighbouring tile; each counter must still count every element once.
    """
    W = 512 // C
    inner, n = H * W * C, N * H * W
    shp = (N, H, W, C)
    Qn = Quant(8, 8 - 1 - E_N, True, name="dp/fn_range")
    Qr = Quant(8, 8 - 1 - e_r, True, True, inner, name="dp/fr_range")
    Qx = Quant(9, 9 - 1 - e_o1, True, True, inner, name="dp/fx_range")
    Qw = Quant(8, 7, True, name="dp/fw_range")
    Qo = Quant(8, 8 - 1 - e_out, True, True, inner, name="dp/fo_range")
    q = torch.from_numpy(qcodes.astype(np.int8).reshape(shp)).to(DEV)
    chs = np.zeros((NSHARD, 2 * C), dtype=np.int64)
    chs[0, C:] = n * 4 ** E_N
    s = 2.0 ** -E_N  # the oracle's moment formula on these sums
    mu_d = chs.sum(0)[:C] * s / n
    var_d = chs.sum(0)[C:] * (s * s) / n - mu_d * mu_d
    assert np.all(_f32(mu_d) == 0) and np.all(np.sqrt(_f32(var_d) + np.float32(0)) == 1)
    chsum = torch.from_numpy(chs.reshape(-1)).to(DEV)
    ms = torch.full((2 * C,), 7.0, device=DEV)
    gb = torch.cat([torch.full((C,), float(gamma)), torch.zeros(C)]).to(DEV)
    rout = torch.empty(shp, dtype=torch.int8, device=DEV)
    o1 = torch.empty(shp, dtype=torch.int8, device=DEV)
    yq = torch.empty(shp, dtype=torch.int8, device=DEV)
    ychsum = ops.new_sums(C, 2, DEV)
    CS = C // 16
    ksf = ops.packed_slices(3, 3, C)
    wf = torch.zeros((C, ksf * 16), dtype=torch.int8, device=DEV)
    co = torch.arange(C, device=DEV)
    wf[co, (4 * CS + co // 16) * 16 + co % 16] = 1  # centre tap, ci = co
    colsum = torch.ones(C, dtype=torch.int32, device=DEV)
    cf = _lib.ConvFwd()
    a = cf.c
    a.b1.nrm = _lib.BnNorm(q.data_ptr(), Qn.q.desc_nostats(), chsum.data_ptr(), n, 0.0, 0.999, 0.001, ms.data_ptr(),
                           None, None, 0, 0)
    a.b1.qr, a.b1.rout, a.b1.gb = Qr.desc, rout.data_ptr(), gb.data_ptr()
    a.relu = 1
    a.o1, a.o1_kind, a.qo1 = o1.data_ptr(), OUT_U8OFF, Qx.desc
    a.rows, a.inner, a.C = N, inner, C
    y = None
    if res is not None:
        rt = torch.from_numpy(res.reshape(shp)).to(DEV)
        y = torch.empty(shp, dtype=torch.float32, device=DEV)
        a.res, a.y = rt.data_ptr(), y.data_ptr()
    cf.wf, cf.ksf, cf.w4, cf.wcolsum = wf.data_ptr(), ksf, 0, colsum.data_ptr()
    cf.d = ops.conv_desc(N, H, W, C, C, 3, 3, 1, 1, "SAME")
    cf.qw = Qw.q.desc_nostats()
    cf.yq, cf.qout, cf.ychsum = yq.data_ptr(), Qo.desc, ychsum.data_ptr()
    _lib.call("lbt_conv_fwd_fused_i8", ctypes.byref(cf), _lib.stream())
    assert_same(ms.cpu().numpy(), np.concatenate([np.zeros(C), np.ones(C)]).astype(np.float32), "ms")
    op_r = (qcodes.astype(np.float32) * np.float32(2.0 ** -E_N)).reshape(N, inner)
    R = expect(Qr, op_r, rout, OUT_I8, "R")
    v = (R.astype(np.float32) * np.float32(2.0 ** -e_r)) * np.float32(gamma) + np.float32(0)
    if res is not None:
        v = (v + res.reshape(N, inner)).astype(np.float32)
    v = relu_np(v)
    if y is not None:
        assert_same(y.cpu().numpy().reshape(N, inner), v, "y")
    X = DP.u8off(expect(Qx, v, o1, OUT_U8OFF, "X"))
    op_y = (X.astype(np.float32) * np.float32(2.0 ** -e_o1)).astype(np.float32)
    Y = expect(Qo, op_y, yq, OUT_I8, "yq")
    s1, s2 = channel_sums(ychsum, C)
    r = Y.reshape(-1, C).astype(np.int64)
    assert_same(s1, r.sum(0), "S1")
    assert_same(s2, (r * r).sum(0), "S2")
    return op_r, v, op_y


@gpu
def test_conv_fwd_fused_integer_grids():
    """lbt_conv_fwd_fused_i8 (64 channels, 2-row tiles, 7 samples): every int8 code into qr at xm = q (hits
    -L, +-L/2, L-1); X's operand 4 R (hits L/2, L and the clip at L-1 of the 9-bit quantiser; no lower clip
    exists after the ReLU); the output's operand the X code (hits L/2, L, the clip). A float cannot reach
    qr or the output quantiser, whose operands are computed from codes."""
    N, H, C = 7, 8, 64
    _run_fwd_fused(N, H, C, grid_codes(8, N, H * 512, True), e_r=5, gamma=1.0, e_o1=7, e_out=7)


@gpu
@pytest.mark.parametrize("cls", DP.ALL_CLASSES)
def test_conv_fwd_fused_float_residual(cls):
    """The residual variant with gamma = beta = 0: v = 0 + res, so the X quantiser (floor_i(fminf(xm + u,
    L - 1)) and the one-compare counters of conv_fused_fwd.h) sees max(res, 0) of the crafted float sites."""
    H, C = 8, 64
    Qx = Quant(9, 9 - 1 - 7, True, True, H * 512, name="dp/fx_range")  # the X quantiser of _run_fwd_fused
    res = Qx.sites(cls)
    if len(res) == 1:
        res = np.repeat(res, 2, axis=0)  # the noise is per column: a second sample sees the same sites
    N = res.shape[0]
    _run_fwd_fused(N, H, C, grid_codes(8, N, H * 512, True), e_r=5, gamma=0.0, e_o1=7, e_out=7, res=res)


@gpu
def test_conv_fwd_fused_saturation_largest_tile():
    """Saturation at the largest tile (16 channels, 64 samples of 32 rows: 8-row tiles), where the packed
    16-bit wave totals are largest: every element of every quantiser overflows both thresholds, so each
    counter equals the element count."""
    N, H, C = 64, 32, 16
    assert _lib.load().lbt_conv_fused_tile_rows(C, N, H) == 8
    r, c = np.indices((N, H * 512))
    q = 32 + (c + 5 * r) % 96  # 32 .. 127: 4 q >= L of the Rescale_q quantiser at e_r = E_N + 2
    op_r, v, op_y = _run_fwd_fused(N, H, C, q, e_r=E_N + 2, gamma=1024.0, e_o1=1, e_out=1)
    n = N * H * 512
    assert DP.oracle_counts(op_r, 8, 8 - 1 - (E_N + 2)) == (n, n)
    assert DP.oracle_counts(v, 9, 9 - 1 - 1) == (n, n)
    assert DP.oracle_counts(op_y, 8, 8 - 1 - 1) == (n, n)


# ---- D. the fused 3x3 backward (pass B + dgrad + pass A in one launch)
def _run_bwd_fused(N, H, C, Gcodes, e_o, qrg, qng, bits_o=8, add=None):
    """One lbt_conv_bwd_fused_i8 launch (y_mask = 1, masked gradient stored, no deferred wgrad) on
    [N, H, 512 / C, C] with analytically known operands, checked against the oracle:

      * pass B with ms = [0 | 1] and zero sums: dx = G 2^-E_N, an integer grid into the conv's gradient
        quantiser qo (as test_chain_bwd_b_integer_grid);
      * the dgrad copies through its centre tap (weight code 1 at e_w = 0): g = gq 2^-e_o (+ add_src);
      * pass A: g into the Rescale_q gradient quantiser (qrg = (bits, e)), then with gamma_q = 1 its
        dequantised code into the Normalization_q gradient quantiser (qng = (bits, e)).

    Halo pixels of pass B are recomputed by the neighbouring tile and must be counted once.
    """
    W = 512 // C
    inner, n = H * W * C, N * H * W
    shp = (N, H, W, C)
    Qg = Quant(8, 8 - 1 - E_N, True, name="dp/bg_range")
    Qx = Quant(8, 2, True, name="dp/bx_range")
    Qw = Quant(8, 7, True, name="dp/bw_range")
    Qo = Quant(bits_o, bits_o - 1 - e_o, True, True, inner, name="dp/bo_range")
    Qrg = Quant(qrg[0], qrg[0] - 1 - qrg[1], True, True, inner, name="dp/brg_range")
    Qng = Quant(qng[0], qng[0] - 1 - qng[1], True, True, inner, name="dp/bng_range")
    G = torch.from_numpy(Gcodes.astype(np.int8).reshape(shp)).to(DEV)
    zeros8 = torch.zeros(shp, dtype=torch.int8, device=DEV)
    ones8 = torch.ones(shp, dtype=torch.int8, device=DEV)
    ms = torch.cat([torch.zeros(C), torch.ones(C)]).to(DEV)
    bsums = ops.new_sums(C, 4, DEV)
    gq = torch.empty(shp, dtype=torch.int8, device=DEV)
    gcol = ops.new_sums(C, 2, DEV)
    CS = C // 16
    ksd = ops.packed_slices(3, 3, C)
    wd = torch.zeros((C, ksd * 16), dtype=torch.int8, device=DEV)
    ci = torch.arange(C, device=DEV)
    wd[ci, (4 * CS + ci // 16) * 16 + ci % 16] = 1  # centre tap, co = ci
    ym = torch.ones(shp, dtype=torch.float32, device=DEV)
    gmask = torch.empty(shp, dtype=torch.float32, device=DEV)
    Gout = torch.empty(shp, dtype=torch.int8, device=DEV)
    asums = ops.new_sums(C, 4, DEV)
    gb = unit_gb(C)
    addt = torch.from_numpy(add.reshape(shp)).to(DEV) if add is not None else None
    p = _lib.ConvBwd()
    p.b = _lib.ChainBwdB(G.data_ptr(), Qg.desc, zeros8.data_ptr(), Qx.desc, ms.data_ptr(), bsums.data_ptr(), n, None,
                         gq.data_ptr(), Qo.desc, gcol.data_ptr(), N, inner, C)
    p.wd, p.ksd, p.w4 = wd.data_ptr(), ksd, 0
    p.d = ops.conv_desc(N, H, W, C, C, 3, 3, 1, 1, "SAME")
    p.qw = Qw.q.desc_nostats()
    p.add_src = addt.data_ptr() if addt is not None else None
    p.a.y_mask, p.a.gmask_out = ym.data_ptr(), gmask.data_ptr()
    p.a.b1 = _lib.BwdBranch(Qrg.desc, ones8.data_ptr(), _lib.NO_Q, gb.data_ptr(), Qng.desc, ones8.data_ptr(),
                            Gout.data_ptr(), None, asums.data_ptr())
    p.a.rows, p.a.inner, p.a.C = N, inner, C
    _lib.call("lbt_conv_bwd_fused_i8", ctypes.byref(p), _lib.stream())
    dxb = (Gcodes.astype(np.float32) * np.float32(2.0 ** -E_N)).reshape(N, inner)
    gqr = expect(Qo, dxb, gq, OUT_I8, "gq")
    s12 = shard_sums(gcol, 2 * C)
    r = gqr.reshape(-1, C).astype(np.int64)
    assert_same(s12[:C], r.sum(0), "gq S1")
    assert_same(s12[C:], (r * r).sum(0), "gq S2")
    g = (gqr.astype(np.float32) * np.float32(2.0 ** -e_o)).astype(np.float32)
    if add is not None:
        g = (g + add.reshape(N, inner)).astype(np.float32)
    assert_same(gmask.cpu().numpy().reshape(N, inner), g, "masked gradient")
    G2 = DP.oracle_codes(g, Qrg.bits, Qrg.I, True, Qrg.u)
    assert Qrg.take_counts() == DP.oracle_counts(g, Qrg.bits, Qrg.I), "qrg counters"
    d = odfxp.dequant(G2, qrg[1])
    Gr = expect(Qng, d, Gout, OUT_I8, "G")
    s4 = shard_sums(asums, 4 * C)
    per2 = G2.reshape(-1, C).astype(np.int64).sum(0)
    perg = Gr.reshape(-1, C).astype(np.int64).sum(0)
    for k, want in enumerate((per2, per2, perg, perg)):
        assert_same(s4[k * C:(k + 1) * C], want, "pass A sum %d" % k)
    return dxb, g, d


@gpu
@pytest.mark.parametrize("bits_o,e_o,qrg,qng", [(8, 5, (4, 2), (3, 1)), (8, 4, (4, 1), (3, 0)), (4, 5, (8, 8), (8, 9))],
                         ids=["o8_rg4_ng3", "o8_halves", "o4_rg8_ng8"])
def test_conv_bwd_fused_integer_grids(bits_o, e_o, qrg, qng):
    """lbt_conv_bwd_fused_i8 (64 channels, 2-row tiles, 7 samples) on integer grids: qo sees G 2^(e_o - 5)
    (every int8 code, or [-2L-2, 2L+2] of the 4-bit quantiser; halves at e_o = 4), qrg sees gq 2^(e_rg - e_o)
    and qng G2 2^(e_ng - e_rg): each reaches its +-L/2, +-L and both clip limits in one of the cases."""
    N, H, C = 7, 8, 64
    _run_bwd_fused(N, H, C, grid_codes(bits_o, N, H * 512, True), e_o, qrg, qng, bits_o)


@gpu
@pytest.mark.parametrize("cls", DP.ALL_CLASSES)
def test_conv_bwd_fused_float_add_src(cls):
    """G = 0 makes pass B, its quantiser and the dgrad produce zeros, so g = 0 + add_src: the Rescale_q
    gradient quantiser of the fused pass A sees the crafted float sites (rounding, thresholds, clip,
    specials, saturation), and qng its dequantised codes."""
    H, C = 8, 64
    Qrg = Quant(8, 2, True, True, H * 512, name="dp/brg_range")  # the qrg of _run_bwd_fused below
    add = Qrg.sites(cls)
    if len(add) == 1:
        add = np.repeat(add, 2, axis=0)
    N = add.shape[0]
    _run_bwd_fused(N, H, C, np.zeros((N, H * 512), dtype=np.int64), 5, (8, 5), (8, 6), add=add)


@gpu
def test_conv_bwd_fused_saturation_largest_tile():
    """Saturation at the largest tile (16 channels, 64 samples of 32 rows: 8-row tiles): every element of
    all three quantisers overflows both thresholds, signs alternating; each counter equals the element count."""
    N, H, C = 64, 32, 16
    assert _lib.load().lbt_conv_fused_tile_rows(C, N, H) == 8
    r, c = np.indices((N, H * 512))
    G = (33 + (c + 5 * r) % 95) * np.where((r + c) % 2 == 0, 1, -1)  # 4 |G| > L (-L itself is not < -L)
    dxb, g, d = _run_bwd_fused(N, H, C, G, 7, (8, 9), (8, 11))
    n = N * H * 512
    assert DP.oracle_counts(dxb, 8, 0) == (n, n)
    assert DP.oracle_counts(g, 8, -2) == (n, n)
    assert DP.oracle_counts(d, 8, -4) == (n, n)


# ---- C. (continued) the wide forward's quantising epilogues and the GEMM-fused pass A
def _launches():
    return ops.igemm_tuning()["launches"]


# the 128-row kernel (igemm.h's epilogue); the 256-row kernel's LDS-staged quantiser (igemm_big.hip, quant4_w);
# the persistent one-k-block kernel (igemm_persist.hip, quant4_w on the accumulators)
IGEMM_PATHS = {"rows128": (dict(big=0), 0), "big_lds": (dict(big=1, min_tiles=1, fwdq_perm=1), 1),
               "persistent": (dict(big=1, min_tiles=1, fwdq_perm=2), 1)}


@gpu
@pytest.mark.parametrize("path", list(IGEMM_PATHS))
@pytest.mark.parametrize("stoch,table", EPI_MODES, ids=["nearest", "table"])
@pytest.mark.parametrize("qbits,s", GRID_CASES)
def test_conv_fwd_igemm_q_integer_grid(qbits, s, stoch, table, path):
    """lbt_conv_fwd_igemm_q: a 1x1 identity conv (64 -> 64 channels, 7 x 8 x 8 pixels: two 256-row tiles, the
    second ragged) makes the accumulator the int8 operand code; the dispatch is pinned as test_igemm_big does
    and checked by the 256-row launch counter."""
    N, H, C = 7, 8, 64
    inner = H * H * C
    Qx, Qw, Qo = _grid_quants(qbits, s, stoch, table, inner)
    acc = grid_codes(qbits, N, inner, True)
    xq = torch.from_numpy(acc.astype(np.int8).reshape(N, H, H, C)).to(DEV)
    ksf = ops.packed_slices(1, 1, C)
    wf = torch.zeros((C, ksf * 16), dtype=torch.int8, device=DEV)
    wf[:, :C] = torch.eye(C, dtype=torch.int8, device=DEV)
    d = ops.conv_desc(N, H, H, C, C, 1, 1, 1, 1, "SAME")
    yq = torch.full((N, H, H, C), 99, dtype=torch.int8, device=DEV)
    chsum = ops.new_sums(C, 2, DEV)
    forced, big_launches = IGEMM_PATHS[path]
    n0 = _launches()
    with ops.igemm_forced(**forced):
        ops.conv_fwd_igemm_q(xq, 0, wf, ksf, d, Qx.desc, Qw.desc, yq, Qo.q, chsum)
    assert _launches() == n0 + big_launches, "the call took another kernel than the case pins"
    y = (acc.astype(np.float32) * np.float32(2.0 ** -5)).astype(np.float32)
    ref = expect(Qo, y, yq, OUT_I8, "grid")
    s1, s2 = channel_sums(chsum, C)
    r = ref.reshape(-1, C).astype(np.int64)
    assert_same(s1, r.sum(0), "S1")
    assert_same(s2, (r * r).sum(0), "S2")


def _run_dgrad_chain(N, gcodes, e_g, qrg, qng, add=None):
    """lbt_conv_dgrad_chain_i8 on a 1x1 identity conv (16 channels, N x 16 x 16 pixels) with y_mask = 1:
    g = gq 2^-e_g (+ add_src) into the GEMM-fused pass A (conv_epilogue.h), gamma_q = 1."""
    H, C = 16, 16
    inner = H * H * C
    shp = (N, H, H, C)
    Qg = Quant(8, 8 - 1 - e_g, True, name="dp/dg_range")
    Qw = Quant(8, 7, True, name="dp/dw_range")
    Qrg = Quant(qrg[0], qrg[0] - 1 - qrg[1], True, True, inner, name="dp/drg_range")
    Qng = Quant(qng[0], qng[0] - 1 - qng[1], True, True, inner, name="dp/dng_range")
    gq = torch.from_numpy(gcodes.astype(np.int8).reshape(shp)).to(DEV)
    ksd = ops.packed_slices(1, 1, C)
    wd = torch.zeros((C, ksd * 16), dtype=torch.int8, device=DEV)
    wd[:, :C] = torch.eye(C, dtype=torch.int8, device=DEV)
    d = ops.conv_desc(N, H, H, C, C, 1, 1, 1, 1, "SAME")
    ones8 = torch.ones(shp, dtype=torch.int8, device=DEV)
    ym = torch.ones(shp, dtype=torch.float32, device=DEV)
    Gout = torch.empty(shp, dtype=torch.int8, device=DEV)
    asums = ops.new_sums(C, 4, DEV)
    gb = unit_gb(C)
    addt = torch.from_numpy(add.reshape(shp)).to(DEV) if add is not None else None
    a = _lib.ChainBwdA()
    a.y_mask = ym.data_ptr()
    a.b1 = _lib.BwdBranch(Qrg.desc, ones8.data_ptr(), _lib.NO_Q, gb.data_ptr(), Qng.desc, ones8.data_ptr(),
                          Gout.data_ptr(), None, asums.data_ptr())
    a.rows, a.inner, a.C = N, inner, C
    _lib.call("lbt_conv_dgrad_chain_i8", _lib.ptr(gq), _lib.ptr(wd), ksd, d, Qg.desc, Qw.desc, _lib.ptr(addt),
              ctypes.byref(a), _lib.stream())
    g = (gcodes.astype(np.float32) * np.float32(2.0 ** -e_g)).astype(np.float32).reshape(N, inner)
    if add is not None:
        g = (g + add.reshape(N, inner)).astype(np.float32)
    G2 = DP.oracle_codes(g, Qrg.bits, Qrg.I, True, Qrg.u)
    assert Qrg.take_counts() == DP.oracle_counts(g, Qrg.bits, Qrg.I), "qrg counters"
    Gr = expect(Qng, odfxp.dequant(G2, qrg[1]), Gout, OUT_I8, "G")
    s4 = shard_sums(asums, 4 * C)
    per2 = G2.reshape(-1, C).astype(np.int64).sum(0)
    perg = Gr.reshape(-1, C).astype(np.int64).sum(0)
    for k, want in enumerate((per2, per2, perg, perg)):
        assert_same(s4[k * C:(k + 1) * C], want, "pass A sum %d" % k)


@gpu
@pytest.mark.parametrize("qrg,qng", [((4, 2), (3, 1)), ((8, 5), (8, 6)), ((8, 6), (8, 6))])
def test_conv_dgrad_chain_i8_integer_grid(qrg, qng):
    """Every int8 gradient code through the identity dgrad: qrg sees gq 2^(e_rg - 5) -- gq / 8 on a 4-bit
    quantiser (+-L, +-L/2, both clip limits), gq and 2 gq on 8-bit ones -- and qng its dequantised codes."""
    _run_dgrad_chain(7, grid_codes(8, 7, 4096, True), 5, qrg, qng)


@gpu
@pytest.mark.parametrize("cls", DP.ALL_CLASSES)
def test_conv_dgrad_chain_i8_float_add_src(cls):
    """gq = 0: the dgrad is zero and g = 0 + add_src, so the fused pass A's qrg sees the crafted float sites."""
    Qrg = Quant(8, 2, True, True, 4096, name="dp/drg_range")  # the qrg of _run_dgrad_chain below
    add = Qrg.sites(cls)
    N = add.shape[0]
    _run_dgrad_chain(N, np.zeros((N, 4096), dtype=np.int64), 5, (8, 5), (8, 6), add=add)


@gpu
@pytest.mark.parametrize("big", [1, 0], ids=["epilogue", "unfused"])
@pytest.mark.parametrize("stoch,table", EPI_MODES, ids=["nearest", "table"])
@pytest.mark.parametrize("s", [0, 1])
def test_conv_dgrad_igemm_bna_integer_grid(s, stoch, table, big):
    """lbt_conv_dgrad_igemm_bna: int16 gradient codes through a 1x1 identity dgrad (64 channels) with the mask
    from R = 1, gamma_q = 1, beta_q = 0 (always open): the 8-bit qrg sees gq 2^-s over the whole
    [-2L-2, 2L+2] and qng twice its dequantised code. big = 1: pass A in the 256-row GEMM's epilogue (no
    dx stored); big = 0: the entry's own dgrad + lbt_bn_bwd_a_wide_masked fallback."""
    N, H, C, e_g = 7, 8, 64, 5
    inner = H * H * C
    shp = (N, H, H, C)
    Qg = Quant(16, 16 - 1 - e_g, True, name="dp/ag_range")
    Qw = Quant(8, 7, True, name="dp/aw_range")
    Qr = Quant(8, 2, True, name="dp/ar_range")
    e_rg = e_g - s
    Qrg = Quant(8, 8 - 1 - e_rg, stoch, table, inner, name="dp/arg_range")
    Qng = Quant(8, 8 - 1 - (e_rg + 1), stoch, table, inner, name="dp/ang_range")
    gcodes = grid_codes(8, N, inner, False)
    gq = torch.from_numpy(gcodes.astype(np.int16).reshape(shp)).to(DEV)
    ksd = ops.packed_slices(1, 1, C)
    wd = torch.zeros((C, ksd * 16), dtype=torch.int8, device=DEV)
    wd[:, :C] = torch.eye(C, dtype=torch.int8, device=DEV)
    d = ops.conv_desc(N, H, H, C, C, 1, 1, 1, 1, "SAME")
    ones8 = torch.ones(shp, dtype=torch.int8, device=DEV)
    Gout = torch.empty(shp, dtype=torch.int16, device=DEV)
    sums = ops.new_sums(C, 4, DEV)
    scratch = torch.full(shp, float("nan"), dtype=torch.float32, device=DEV)
    n0 = _launches()
    with ops.igemm_forced(big=big, min_tiles=1, fwdq_perm=1):
        ops.conv_dgrad_igemm_bna(gq, wd, ksd, d, Qg.desc, Qw.desc, Qr.desc, ones8, unit_gb(C), Qrg.q, Qng.q, ones8,
                                 Gout, sums, scratch, None)
    assert _launches() == n0 + big, "the call took another kernel than the case pins"
    gv = (gcodes.astype(np.float32) * np.float32(2.0 ** -e_g)).astype(np.float32)
    G2 = DP.oracle_codes(gv, 8, Qrg.I, stoch, Qrg.u)
    assert Qrg.take_counts() == DP.oracle_counts(gv, 8, Qrg.I), "qrg counters"
    Gr = expect(Qng, odfxp.dequant(G2, e_rg), Gout, OUT_I16, "G")
    s4 = shard_sums(sums, 4 * C)
    per2 = G2.reshape(-1, C).astype(np.int64).sum(0)
    perg = Gr.reshape(-1, C).astype(np.int64).sum(0)
    for k, want in enumerate((per2, per2, perg, perg)):
        assert_same(s4[k * C:(k + 1) * C], want, "pass A sum %d" % k)


# ---- D. (continued) the stage-transition launches: 3x3 / stride 2 + 1x1 / stride 2 shortcut, C -> 2C
def _transition_descs(N, H, C):
    W = 512 // C
    d1 = ops.conv_desc(N, H, W, C, 2 * C, 3, 3, 2, 2, "SAME")
    ds = ops.conv_desc(N, H, W, C, 2 * C, 1, 1, 2, 2, "SAME")
    return W, d1, ds


def _run_fwd2_fused(N, H, C, qcodes, e_r, gamma, e_o, e_out, res):
    """One training-mode lbt_conv_fwd2_fused_i8 launch on [N, H, 512 / C, C], by the construction of
    _run_fwd_fused (mu = 0, sigma = 1 from the chosen channel sums; gamma a power of two or zero, beta = 0;
    the chain always has a residual and y here). The two X quantisers (the 3x3 / 2 conv's input and the
    shortcut's) see the same v = max((R 2^-e_r) gamma + res, 0) with their own noise. Output channel co of
    the 3x3 / 2 conv copies channel co % C through the centre tap, i.e. X1[2 oy + 1, 2 ox + 1] (TF SAME pads
    0 / 1 at stride 2); the shortcut copies X2[2 oy, 2 ox]: each output quantiser sees an X code times
    2^-e_o."""
    W, d1, ds = _transition_descs(N, H, C)
    inner, n, Cq = H * W * C, N * H * W, 2 * C
    inner_o = d1.Ho * d1.Wo * Cq
    shp, oshp = (N, H, W, C), (N, d1.Ho, d1.Wo, Cq)
    Qn = Quant(8, 8 - 1 - E_N, True, name="dp/tn_range")
    Qr = Quant(8, 8 - 1 - e_r, True, True, inner, name="dp/tr_range")
    Qx1 = Quant(9, 9 - 1 - e_o, True, True, inner, name="dp/tx1_range")
    Qx2 = Quant(9, 9 - 1 - e_o, True, True, inner, name="dp/tx2_range")
    Qw = Quant(8, 7, True, name="dp/tw_range")
    Qo1 = Quant(8, 8 - 1 - e_out, True, True, inner_o, name="dp/to1_range")
    Qos = Quant(8, 8 - 1 - e_out, True, True, inner_o, name="dp/tos_range")
    q = torch.from_numpy(qcodes.astype(np.int8).reshape(shp)).to(DEV)
    chs = np.zeros((NSHARD, 2 * C), dtype=np.int64)
    chs[0, C:] = n * 4 ** E_N  # mu = S1 s / n = 0, var = S2 s^2 / n = 1 at s = 2^-E_N, eps = 0
    chsum = torch.from_numpy(chs.reshape(-1)).to(DEV)
    ms = torch.full((2 * C,), 7.0, device=DEV)
    gb = torch.cat([torch.full((C,), float(gamma)), torch.zeros(C)]).to(DEV)
    rout, o1, o2 = (torch.empty(shp, dtype=torch.int8, device=DEV) for _ in range(3))
    y = torch.empty(shp, dtype=torch.float32, device=DEV)
    rt = torch.from_numpy(np.ascontiguousarray(res, dtype=np.float32).reshape(shp)).to(DEV)
    yq1, yqs = (torch.empty(oshp, dtype=torch.int8, device=DEV) for _ in range(2))
    ych1, ychs = ops.new_sums(Cq, 2, DEV), ops.new_sums(Cq, 2, DEV)
    CS = C // 16
    ksf1, ksfs = ops.packed_slices(3, 3, C), ops.packed_slices(1, 1, C)
    co = torch.arange(Cq, device=DEV)
    ci = co % C
    wf1 = torch.zeros((Cq, ksf1 * 16), dtype=torch.int8, device=DEV)
    wf1[co, (4 * CS + ci // 16) * 16 + ci % 16] = 1  # centre tap, ci = co % C
    wfs = torch.zeros((Cq, ksfs * 16), dtype=torch.int8, device=DEV)
    wfs[co, ci] = 1
    colsum = torch.ones(Cq, dtype=torch.int32, device=DEV)
    cf = _lib.ConvFwd2()
    a = cf.c
    a.b1.nrm = _lib.BnNorm(q.data_ptr(), Qn.q.desc_nostats(), chsum.data_ptr(), n, 0.0, 0.999, 0.001, ms.data_ptr(),
                           None, None, 0, 0)
    a.b1.qr, a.b1.rout, a.b1.gb = Qr.desc, rout.data_ptr(), gb.data_ptr()
    a.res, a.relu, a.y = rt.data_ptr(), 1, y.data_ptr()
    a.o1, a.o1_kind, a.qo1 = o1.data_ptr(), OUT_U8OFF, Qx1.desc
    a.o2, a.o2_kind, a.qo2 = o2.data_ptr(), OUT_U8OFF, Qx2.desc
    a.rows, a.inner, a.C = N, inner, C
    cf.wf1, cf.ksf1, cf.wcolsum1 = wf1.data_ptr(), ksf1, colsum.data_ptr()
    cf.wfs, cf.ksfs, cf.wcolsums = wfs.data_ptr(), ksfs, colsum.data_ptr()
    cf.w4, cf.d1, cf.ds = 0, d1, ds
    cf.qw1 = cf.qws = Qw.q.desc_nostats()
    cf.yq1, cf.qout1, cf.ychsum1 = yq1.data_ptr(), Qo1.desc, ych1.data_ptr()
    cf.yqs, cf.qouts, cf.ychsums = yqs.data_ptr(), Qos.desc, ychs.data_ptr()
    _lib.call("lbt_conv_fwd2_fused_i8", ctypes.byref(cf), _lib.stream())
    assert_same(ms.cpu().numpy(), np.concatenate([np.zeros(C), np.ones(C)]).astype(np.float32), "ms")
    op_r = (qcodes.astype(np.float32) * np.float32(2.0 ** -E_N)).reshape(N, inner)
    R = expect(Qr, op_r, rout, OUT_I8, "R")
    v = (R.astype(np.float32) * np.float32(2.0 ** -e_r)) * np.float32(gamma) + np.float32(0)
    v = relu_np((v + np.asarray(res, dtype=np.float32).reshape(N, inner)).astype(np.float32))
    assert_same(y.cpu().numpy().reshape(N, inner), v, "y")
    ops_out = []
    for Qx, o, Qo, yq, ych, off, what in ((Qx1, o1, Qo1, yq1, ych1, 1, "conv-1"), (Qx2, o2, Qos, yqs, ychs, 0, "shortcut")):
        X = DP.u8off(expect(Qx, v, o, OUT_U8OFF, what + " X")).reshape(shp)
        acc = X[:, off::2, off::2, :][..., np.arange(Cq) % C]
        op_y = (acc.astype(np.float32) * np.float32(2.0 ** -e_o)).astype(np.float32).reshape(N, inner_o)
        Y = expect(Qo, op_y, yq, OUT_I8, what + " yq")
        s1, s2 = channel_sums(ych, Cq)
        r = Y.reshape(-1, Cq).astype(np.int64)
        assert_same(s1, r.sum(0), what + " S1")
        assert_same(s2, (r * r).sum(0), what + " S2")
        ops_out.append(op_y)
    return op_r, v, ops_out


@gpu
def test_conv_fwd2_fused_integer_grids():
    """lbt_conv_fwd2_fused_i8 (32 -> 64 channels, 16 x 16 pixels, 3 samples), zero residual: qr sees every
    int8 code, both X quantisers 4 R (L/2, L, the clip at L - 1), both output quantisers the X codes."""
    N, H, C = 3, 16, 32
    inner = H * 512
    _run_fwd2_fused(N, H, C, grid_codes(8, N, inner), 5, 1.0, 7, 7, np.zeros((N, inner), dtype=np.float32))


@gpu
@pytest.mark.parametrize("cls", DP.ALL_CLASSES)
def test_conv_fwd2_fused_float_residual(cls):
    """gamma = beta = 0: v = 0 + res, so both X quantisers of conv_fwd2_kernel (its own floor_i(fminf(xm + u,
    L - 1)) and one-compare counters) see max(res, 0) of the crafted float sites; the sites are built on the
    conv-1 quantiser's noise and the shortcut's quantiser is checked on the same floats with its own."""
    H, C = 16, 32
    Qx1 = Quant(9, 9 - 1 - 7, True, True, H * 512, name="dp/tx1_range")  # the conv-1 X quantiser below
    res = Qx1.sites(cls)
    if len(res) == 1:
        res = np.repeat(res, 2, axis=0)
    N = res.shape[0]
    _run_fwd2_fused(N, H, C, grid_codes(8, N, H * 512), 5, 0.0, 7, 7, res)


@gpu
def test_conv_fwd2_fused_saturation():
    """Saturation (16 -> 32 channels, 8 samples of 32 x 32 pixels; this kernel has one tile height): every
    element of all five quantisers overflows both thresholds, so each counter equals its element count."""
    N, H, C = 8, 32, 16
    inner = H * 512
    r, c = np.indices((N, inner))
    q = 32 + (c + 5 * r) % 96
    op_r, v, ops_out = _run_fwd2_fused(N, H, C, q, E_N + 2, 1024.0, 1, 1, np.zeros((N, inner), dtype=np.float32))
    assert DP.oracle_counts(op_r, 8, 8 - 1 - (E_N + 2)) == (op_r.size, op_r.size)
    assert DP.oracle_counts(v, 9, 9 - 1 - 1) == (v.size, v.size)
    for op_y in ops_out:
        assert DP.oracle_counts(op_y, 8, 8 - 1 - 1) == (op_y.size, op_y.size)


def _run_bwd2_fused(N, H, C, G1codes, Gscodes, e_o, qrg, qng, bits_o=8):
    """One lbt_conv_bwd2_fused_i8 launch (y_mask = 1, masked gradient stored): both pass-B chains on
    [N, H/2, W/2, 2C] as in _run_bwd_fused (integer grids into the two gradient quantisers), the two dgrads
    through identity-like weights -- conv-1's centre tap puts gq1[oy, ox, ci] on pixel (2 oy + 1, 2 ox + 1),
    the shortcut puts gqs[oy, ox, ci] on (2 oy, 2 ox), every other pixel gets 0 -- then pass A on their sum.

    This entry point has no add_src and its pass A sees only sums of dequantised codes, so the float site
    classes (rounding ulps, thresholds at +-1 ulp, specials) cannot be built for it; the integer grids and
    saturation are."""
    W, d1, ds = _transition_descs(N, H, C)
    Cq = 2 * C
    inner, inq, nq = H * W * C, d1.Ho * d1.Wo * Cq, N * d1.Ho * d1.Wo
    shp, oshp = (N, H, W, C), (N, d1.Ho, d1.Wo, Cq)
    Qg = Quant(8, 8 - 1 - E_N, True, name="dp/ug_range")
    Qx = Quant(8, 2, True, name="dp/ux_range")
    Qw = Quant(8, 7, True, name="dp/uw_range")
    Qrg = Quant(qrg[0], qrg[0] - 1 - qrg[1], True, True, inner, name="dp/urg_range")
    Qng = Quant(qng[0], qng[0] - 1 - qng[1], True, True, inner, name="dp/ung_range")
    zeros8 = torch.zeros(oshp, dtype=torch.int8, device=DEV)
    ms = torch.cat([torch.zeros(Cq), torch.ones(Cq)]).to(DEV)
    bsums = ops.new_sums(Cq, 4, DEV)
    CS = C // 16
    ksd1, ksds = ops.packed_slices(3, 3, Cq), ops.packed_slices(1, 1, Cq)
    ci = torch.arange(C, device=DEV)
    wd1 = torch.zeros((C, ksd1 * 16), dtype=torch.int8, device=DEV)
    wd1[ci, (4 * 2 * CS + ci // 16) * 16 + ci % 16] = 1  # centre tap, co = ci
    wds = torch.zeros((C, ksds * 16), dtype=torch.int8, device=DEV)
    wds[ci, ci] = 1
    p = _lib.ConvBwd2()
    keep, passb = [], []
    for name, codes in (("dp/uo1_range", G1codes), ("dp/uos_range", Gscodes)):
        Qo = Quant(bits_o, bits_o - 1 - e_o, True, True, inq, name=name)
        G = torch.from_numpy(codes.astype(np.int8).reshape(oshp)).to(DEV)
        gq = torch.empty(oshp, dtype=torch.int8, device=DEV)
        gcol = ops.new_sums(Cq, 2, DEV)
        b = _lib.ChainBwdB(G.data_ptr(), Qg.desc, zeros8.data_ptr(), Qx.desc, ms.data_ptr(), bsums.data_ptr(), nq, None,
                           gq.data_ptr(), Qo.desc, gcol.data_ptr(), N, inq, Cq)
        keep.append(G)
        passb.append((Qo, codes, gq, gcol, b))
    p.b1, p.bs = passb[0][4], passb[1][4]
    p.wd1, p.ksd1, p.wds, p.ksds, p.w4 = wd1.data_ptr(), ksd1, wds.data_ptr(), ksds, 0
    p.d1, p.ds = d1, ds
    p.qw1 = p.qws = Qw.q.desc_nostats()
    ones8 = torch.ones(shp, dtype=torch.int8, device=DEV)
    ym = torch.ones(shp, dtype=torch.float32, device=DEV)
    gmask = torch.empty(shp, dtype=torch.float32, device=DEV)
    Gout = torch.empty(shp, dtype=torch.int8, device=DEV)
    asums = ops.new_sums(C, 4, DEV)
    gb = unit_gb(C)
    p.a.y_mask, p.a.gmask_out = ym.data_ptr(), gmask.data_ptr()
    p.a.b1 = _lib.BwdBranch(Qrg.desc, ones8.data_ptr(), _lib.NO_Q, gb.data_ptr(), Qng.desc, ones8.data_ptr(),
                            Gout.data_ptr(), None, asums.data_ptr())
    p.a.rows, p.a.inner, p.a.C = N, inner, C
    _lib.call("lbt_conv_bwd2_fused_i8", ctypes.byref(p), _lib.stream())
    g = np.zeros(shp, dtype=np.float32)
    dxbs = []
    for (Qo, codes, gq, gcol, _), off, what in zip(passb, (1, 0), ("conv-1", "shortcut")):
        dxb = (codes.astype(np.float32) * np.float32(2.0 ** -E_N)).reshape(N, inq)
        gqr = expect(Qo, dxb, gq, OUT_I8, what + " gq")
        s12 = shard_sums(gcol, 2 * Cq)
        r = gqr.reshape(-1, Cq).astype(np.int64)
        assert_same(s12[:Cq], r.sum(0), what + " gq S1")
        assert_same(s12[Cq:], (r * r).sum(0), what + " gq S2")
        g[:, off::2, off::2, :] = gqr.reshape(oshp)[..., :C].astype(np.float32) * np.float32(2.0 ** -e_o)
        dxbs.append(dxb)
    g = g.reshape(N, inner)
    assert_same(gmask.cpu().numpy().reshape(N, inner), g, "masked gradient")
    G2 = DP.oracle_codes(g, Qrg.bits, Qrg.I, True, Qrg.u)
    assert Qrg.take_counts() == DP.oracle_counts(g, Qrg.bits, Qrg.I), "qrg counters"
    Gr = expect(Qng, odfxp.dequant(G2, qrg[1]), Gout, OUT_I8, "G")
    s4 = shard_sums(asums, 4 * C)
    per2 = G2.reshape(-1, C).astype(np.int64).sum(0)
    perg = Gr.reshape(-1, C).astype(np.int64).sum(0)
    for k, want in enumerate((per2, per2, perg, perg)):
        assert_same(s4[k * C:(k + 1) * C], want, "pass A sum %d" % k)
    return dxbs


@gpu
@pytest.mark.parametrize("bits_o,e_o,qrg,qng", [(8, 5, (4, 2), (3, 1)), (8, 4, (4, 1), (3, 0)), (4, 5, (8, 8), (8, 9))],
                         ids=["o8_rg4_ng3", "o8_halves", "o4_rg8_ng8"])
def test_conv_bwd2_fused_integer_grids(bits_o, e_o, qrg, qng):
    """lbt_conv_bwd2_fused_i8 (32 -> 64 channels, 16 x 16 pixels, 3 samples) on the integer grids of
    test_conv_bwd_fused_integer_grids, the two pass-B chains on differently shifted grids."""
    N, H, C = 3, 16, 32
    inq = (H // 2) * (512 // C // 2) * 2 * C
    G1 = grid_codes(bits_o, N, inq)
    _run_bwd2_fused(N, H, C, G1, np.roll(G1, 11, axis=1), e_o, qrg, qng, bits_o)


@gpu
def test_conv_bwd2_fused_saturation_largest_tile():
    """Saturation at the 16-channel stage's 8-row tiles (8 samples of 32 x 32 pixels): every element of both
    pass-B quantisers overflows both thresholds (counters = element count); pass A sees the saturated codes
    on a quarter of its pixels and zeros elsewhere, checked against the oracle's counts."""
    N, H, C = 8, 32, 16
    inq = (H // 2) * (512 // C // 2) * 2 * C
    r, c = np.indices((N, inq))
    G = (33 + (c + 5 * r) % 95) * np.where((r + c) % 2 == 0, 1, -1)
    for dxb in _run_bwd2_fused(N, H, C, G, -G, 7, (8, 9), (8, 11)):
        assert DP.oracle_counts(dxb, 8, 0) == (dxb.size, dxb.size)

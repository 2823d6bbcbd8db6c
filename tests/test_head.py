"""The fused classifier head (lbt_head_fwd_bwd, head.hip; head_reduce, head.h) on every kernel path and at
the quantisers' decision points, against the numpy head of tests/head_oracle.py.

CPU part (unmarked): the crafted inputs are not vacuous on the oracle alone, four deliberately wrong numpy
heads differ from it, and the path matrix reaches every path of the kernel. GPU part (``@pytest.mark.gpu``):
every output and counter of the head BIT FOR BIT against the oracle and against the separate launches the
head replaces. The one transcendental step is split off: dz and loss[0] must equal lbt_softmax_xent_n run
on the head's own logits, and everything downstream is checked against the oracle fed with the kernel's dz.

The entry point reads LBT_HEAD_SPLIT once per process, so the tests cannot steer the workgroups per sample
with it: S follows from the shape (``Case.split``), and the module is skipped when the variable is set.
"""
import ctypes
import os

import numpy as np
import pytest

if os.environ.get("LBT_HEAD_SPLIT"):
    pytest.skip("LBT_HEAD_SPLIT is set: the head's workgroups per sample no longer follow from the shape, which "
                "the path matrix of this module relies on", allow_module_level=True)

import decision_points as DP
import head_oracle as HO
from oracle import dfxp as odfxp
from test_decision_points import MODE_IDS, MODES, SEED, STEP, WCASES, Quant, site_blocks

F32 = np.float32
EINVAL = 1001


# ------------------------------------------------------------------------------ cases (no GPU needed)
class QS:
    """A quantiser of a case: what the oracle needs (``oracle()``) and, on the GPU, a ``Quant`` (``gpu()``)."""

    def __init__(self, name, bits, I, stoch=True, table=False, inner=1):
        self.name, self.bits, self.I, self.stoch, self.table, self.inner = name, bits, I, stoch, table, inner

    def oracle(self):
        return HO.Q(self.bits, self.I, self.stoch, DP.noise(self.inner, self.stoch, SEED, odfxp.qid_of(self.name), STEP))

    def gpu(self):
        return Quant(self.bits, self.I, self.stoch, self.table and self.stoch, self.inner, name=self.name)

    def sites(self, cls):
        return DP.sites(cls, self.bits, self.I, self.stoch, self.inner, SEED, odfxp.qid_of(self.name), STEP)


def ilog2(n):
    return int(n).bit_length() - 1


class Case:
    """One head problem: shapes, operands (numpy) and quantisers. pa: the fused pass A; chain: the end chain
    (with pa); table: noise tables (else inline Philox) for the stochastic quantisers; qx_table overrides it
    for qx alone. Any operand or quantiser can be replaced through ``over``."""
    EPS, MOM, OMM, E_N = 1e-5, 0.999, 0.001, 5

    def __init__(self, N, HW, C, K, pa=False, chain=False, table=True, qx_table=None, loss_n=0, seed=0, **over):
        self.N, self.HW, self.C, self.K, self.pa, self.chain, self.loss_n = N, HW, C, K, pa or chain, chain, loss_n
        rng = np.random.default_rng(1000 * N + 10 * HW + C + K + seed)
        # exponents that put each quantiser's operand around its thresholds (some counted at L / 2 and at L):
        # |pooled| ~ 4.5 / sqrt(HW) at most (the chain's block output: ~1.4), |dz| <= 1 / N, |sum gq wq| ~ 2^12
        ex = 7 if chain else 5 + (ilog2(HW) + 1) // 2
        eg = ilog2(N) + 8
        erg = eg + ilog2(HW) + 1
        self.q = dict(qx=QS("hd/X_range", 8, 7 - ex, True, table if qx_table is None else qx_table, C),
                      qw=QS("hd/W_range", 8, 1), qg=QS("hd/grad_range", 8, 7 - eg, True, table, K))
        if self.pa:
            self.q["qrg"] = QS("hb/rg_range", 8, 7 - erg, True, table, HW * C)
            self.q["qng"] = QS("hb/ng_range", 8, 7 - erg, True, table, HW * C)
            self.ym = rng.normal(0, 1, (N, HW, C)).astype(F32)
            self.R = rng.integers(-128, 128, (N, HW, C)).astype(np.int8)
            self.qn = rng.integers(-128, 128, (N, HW, C)).astype(np.int8)
            self.gamma = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(F32)
        if chain:
            self.q["qr"] = QS("hb/r_range", 8, 0, True, True, HW * C)  # e = 7: |xhat m| <= 222 (some overflow L)
            self.q["qn"] = QS("hb/n_range", 8, 8 - 1 - self.E_N)
            self.qn = rng.integers(-128, 128, (N, HW, C)).astype(np.int8)
            self.res = rng.normal(0, 1, (N, HW, C)).astype(F32)
            self.beta = rng.normal(0, 0.3, C).astype(F32)
            self.rm0, self.rv0 = rng.normal(0, 1, C).astype(F32), rng.uniform(0.5, 2, C).astype(F32)
        self.x = None if chain else rng.normal(0, 1.5, (N, HW, C)).astype(F32)
        self.wq = rng.integers(-20, 21, (C, K)).astype(np.int8)
        self.W = rng.normal(0, 0.3, (C, K)).astype(F32)
        self.wd2 = F32(4e-4)
        self.labels = rng.integers(0, K, N).astype(np.int32)
        for k, v in over.items():
            if k in self.q:
                self.q[k] = v
            else:
                assert hasattr(self, k), k
                setattr(self, k, v)
        self._fw = None

    @property
    def norm(self):
        return self.loss_n if self.loss_n > 0 else self.N

    # ---- which kernel paths the shape takes (head.hip's own rules)
    def split(self):
        smax = 4 if 2 * self.N < 256 else 2
        return max(s for s in range(1, smax + 1) if self.HW % s == 0 and (not self.chain or 4 % s == 0))

    def fast(self):
        q = self.q
        return bool(self.chain and self.C * self.K <= 1024 and all(q[k].stoch and q[k].table for k in ("qx", "qg")))

    def paths(self):
        N, HW, C, K, S = self.N, self.HW, self.C, self.K, self.split()
        P = 4096 // C
        p = {"S=%d" % S, "K=%d" % K if K in (1, 64) else "K", "chunks=%d" % -(-HW // P)}
        p.add("kernel:" + ("fast" if self.fast() else "chain" if self.chain else "plain"))
        if HW > P and HW % P:
            p.add("partial last chunk")
        if C & (C - 1):
            p.add("C not a power of two")
        if K == 64 and C == 256 and HW > P:
            p.add("K=64, C=256, chunks>1")
        if self.pa:
            p.add("pa:" + ("prefetch" if (HW // S) * C // 4 <= 1024 else "loop"))
            p.add("pa sums:" + ("scatter%d" % (C // 4) if C // 4 <= 16 else "butterfly%d" % (C // 4)))
            p.add("pa noise:" + ("table" if self.q["qrg"].table else "philox"))
        if self.chain:
            p.add("chain moments:" + ("head_stat_load" if C <= 64 else "bn_moments"))
            if C < 64:
                p.add("chain C<64")
            if not self.fast():
                p.add("chain not fast:" + ("philox" if not self.q["qx"].table else "C*K>1024"))
        return p

    # ---- the oracle
    def oq(self, k):
        return self.q[k].oracle()

    def forward(self):
        if self._fw is None:
            ch = None
            if self.chain:
                ch = HO.chain(self.qn, self.E_N, self.gamma, self.beta, self.res, self.oq("qr"), self.EPS, self.MOM,
                              self.OMM, self.rm0, self.rv0)
            fw = HO.forward(ch["y"] if ch else self.x, self.wq, self.oq("qx"), self.oq("qw"))
            fw["chain"] = ch
            self._fw = fw
        return self._fw

    def backward(self, dz):
        fw = self.forward()
        bw = HO.backward(fw, dz, self.wq, self.oq("qx"), self.oq("qw"), self.oq("qg"), self.HW, self.W, self.wd2)
        if self.pa:
            ch = fw["chain"]
            bw["pa"] = HO.pass_a(bw["g"], ch["y"] if ch else self.ym, ch["R"] if ch else self.R, self.qn, self.gamma,
                                 self.oq("qrg"), self.oq("qng"))
        return bw

    def oracle_dz(self):
        return HO.softmax(self.forward()["logits"], self.labels, self.norm)[1]


def case_id(cs):
    return "N%d_HW%d_C%d_K%d%s%s" % (cs.N, cs.HW, cs.C, cs.K, "_chain" if cs.chain else "_pa" if cs.pa else "",
                                      "" if cs.q["qg"].table and cs.q["qx"].table else "_philox")


# (a) the path matrix
PLAIN = [Case(3, 1, 8, 1), Case(5, 9, 24, 7), Case(17, 64, 128, 33), Case(2, 49, 256, 64), Case(130, 6, 72, 10),
         Case(130, 7, 40, 5, table=False)]
PASS_A = [Case(3, 4, 8, 10, pa=True), Case(3, 9, 16, 10, pa=True), Case(3, 49, 32, 10, pa=True),
          Case(130, 64, 64, 10, pa=True), Case(130, 64, 64, 10, pa=True, table=False), Case(2, 64, 128, 10, pa=True),
          Case(2, 25, 256, 10, pa=True), Case(130, 66, 256, 10, pa=True)]
CHAIN = [Case(3, 64, 64, 10, chain=True), Case(130, 64, 64, 10, chain=True), Case(3, 64, 64, 17, chain=True),
         Case(3, 64, 64, 10, chain=True, qx_table=False), Case(3, 32, 128, 10, chain=True),
         Case(3, 16, 256, 10, chain=True), Case(3, 128, 32, 10, chain=True), Case(3, 512, 8, 10, chain=True)]
MATRIX = PLAIN + PASS_A + CHAIN

# every path the issue names as never executed (and the one the older tests reach)
REQUIRED_PATHS = [
    "kernel:plain", "kernel:chain", "kernel:fast", "chain not fast:philox", "chain not fast:C*K>1024",
    "chain moments:bn_moments", "chain moments:head_stat_load", "chain C<64",
    "pa:loop", "pa:prefetch", "pa noise:philox", "pa noise:table",
    "pa sums:scatter2", "pa sums:scatter4", "pa sums:scatter8", "pa sums:scatter16", "pa sums:butterfly32",
    "pa sums:butterfly64",
    "S=1", "S=2", "S=3", "S=4", "chunks=2", "chunks=4", "partial last chunk", "C not a power of two", "K=1", "K=64",
    "K=64, C=256, chunks>1"]


# ------------------------------------------------------------------------------------------ CPU
def test_path_matrix_reaches_every_path():
    """The matrix of (a), by the entry point's own rules for S, the kernel, the pass-A operand path, the
    channel-sum reduction, the moments and the pooling chunks, reaches every path of the kernel."""
    reached = {}
    for cs in MATRIX:
        for p in cs.paths():
            reached.setdefault(p, []).append(case_id(cs))
    for p in sorted(reached):
        print("%-28s %s" % (p, " ".join(reached[p])))
    missing = [p for p in REQUIRED_PATHS if p not in reached]
    assert not missing, missing
    # the splits the issue states for its shapes
    S = {case_id(cs): cs.split() for cs in MATRIX}
    assert [cs.split() for cs in PLAIN] == [1, 3, 4, 1, 2, 1]
    assert [cs.split() for cs in PASS_A] == [4, 3, 1, 2, 2, 4, 1, 2]
    assert [cs.split() for cs in CHAIN] == [4, 2, 4, 4, 4, 4, 4, 4], S
    assert [cs.fast() for cs in CHAIN] == [True, True, False, False, False, False, True, True]
    # pass A with chains: own = 4 / S slots per thread
    assert 4 // CHAIN[0].split() == 1 and 4 // CHAIN[1].split() == 2


QX_CASES = [(b, i, s) for b, i in WCASES for s in (True, False)]


def qx_site_input(site, HW):
    """[N, HW, C]: the site (times HW) in pixel 0, zeros elsewhere: the in-order sum is HW site + 0 + .. and
    times 1 / HW (a power of two) gives the site back."""
    x = np.zeros((site.shape[0], HW, site.shape[1]), F32)
    with np.errstate(over="ignore"):
        x[:, 0, :] = (F32(HW) * site).astype(F32)
    return x


def pool_exact(site):
    """The bits of the site as the pooling returns it: the site's own, +0 for -0."""
    return np.where(site == 0, F32(0), site).astype(F32).view(np.uint32)


@pytest.mark.parametrize("C", [256, 8])
@pytest.mark.parametrize("bits,I,stoch", QX_CASES)
def test_qx_sites_reach_the_quantiser_exactly(bits, I, stoch, C):
    """The pooled value of the oracle IS the site, bit for bit (subnormals included), for every finite site below
    FLT_MAX / HW -- but for -0, which the in-order sum started from +0 turns into +0 (0 + -0 = +0; the two
    quantise alike); and the four wrong quantisers differ from the oracle on these sites."""
    qs = QS("hd/X_range", bits, I, stoch, False, C)
    q = qs.oracle()
    diff = {name: [0, 0] for name in DP.WRONG}
    for cls in DP.ALL_CLASSES:
        site = qs.sites(cls)
        for HW in (1, 4):
            pooled = HO.pool(qx_site_input(site, HW))
            ok = np.isfinite(site) & (np.abs(site) < DP.FLT_MAX / HW)
            assert ok.all() or cls == "special"  # all but the +-inf / +-FLT_MAX specials
            assert np.array_equal(pooled.view(np.uint32)[ok], pool_exact(site)[ok]), (cls, HW)
        ref, cnt = HO.codes(site, q), HO.counts(site, q)
        for name, fn in DP.WRONG.items():
            wq_, wc = fn(site, bits, I, stoch, q.noise)
            diff[name][0] += int(np.count_nonzero(wq_ != ref))
            diff[name][1] += int(wc != cnt)
    print(bits, I, stoch, C, diff)
    assert diff["symmetric_counts"][1] > 0 and diff["clip_to_L"][0] > 0
    assert diff["half_away" if not stoch else "exact_add"][0] > 0


def tie_case(N=4, bits=8):
    """wq = 0, K = 4, labels cycling: every logit is 0 and every p exactly 1 / 4, so with
    frac_bits(qg) = log2(N K) - 1 the operand dz m is +0.5 on the wrong classes and -1.5 on the right one."""
    K = 4
    e = ilog2(N * K) - 1
    return Case(N, 1, 8, K, wq=np.zeros((8, K), np.int8), labels=(np.arange(N) % K).astype(np.int32),
                qg=QS("hd/grad_range", bits, bits - 1 - e, False, False, K))


def test_all_zero_weights_tie_case():
    cs = tie_case()
    assert not np.any(cs.forward()["logits"])
    dz = cs.oracle_dz()
    onehot = np.arange(4)[None, :] == cs.labels[:, None]
    xm = dz.astype(np.float64) * 2.0 ** HO.frac(cs.oq("qg"))
    assert np.array_equal(xm, np.where(onehot, -1.5, 0.5))
    gq = cs.backward(dz)["gq"]
    assert np.array_equal(gq, np.where(onehot, -2, 0))                      # half-even
    away = np.sign(xm) * np.floor(np.abs(xm) + 0.5)
    up = np.floor(xm + 0.5)
    assert np.array_equal(away, np.where(onehot, -2, 1)) and np.array_equal(up, np.where(onehot, -1, 1))
    assert np.any(gq != away) and np.any(gq != up) and np.any(away != up)


def grid_case(C, table=True):
    """(d) The pass-A integer grid. x = 0 makes every logit 0 (pq = floor(0 + u) = 0), K = 4 every p = 1 / 4, and
    e_g = 6 with N = 4 the codes gq = 4 (wrong class) / -12 (right class) exactly. wq[c][0] = c - C / 2 (e_w = 0),
    the other classes 0: s_dp[c] = gq[0] (c - C / 2) 2^-6, g = s_dp / 4. With e_rg = 5 qrg's operand is
    g m = gq[0] (c - C / 2) / 8: steps of 1 / 2 over the channels where gq[0] = 4, of 3 / 2 where it is -12.
    gamma_q = 2 and e_ng = e_rg - 2 make qng's operand G2 / 2. Limits: L_rg = C / 8, L_ng = C / 32, so both
    operands pass +-L / 2 and +-L. The y mask holds 0.0, -0.0, 2^-149 and -1 at known places."""
    N, HW, K = 4, 4, 4
    brg, bng = ilog2(C) - 2, ilog2(C) - 4
    wq = np.zeros((C, K), np.int8)
    wq[:, 0] = np.arange(C) - C // 2
    rng = np.random.default_rng(C)
    ym = rng.uniform(0.5, 2, (N, HW, C)).astype(F32)
    ym[:, 0, 0::4], ym[:, 1, 1::4], ym[:, 2, 2::4], ym[:, 3, 3::4] = F32(0.0), F32(-0.0), F32(2.0 ** -149), F32(-1.0)
    return Case(N, HW, C, K, pa=True, table=table, x=np.zeros((N, HW, C), F32), wq=wq, ym=ym,
                labels=(np.arange(N) % K).astype(np.int32), gamma=np.full(C, 2.0, F32),
                qw=QS("hd/W_range", 8, 7), qg=QS("hd/grad_range", 8, 1, True, table, K),
                qrg=QS("hb/rg_range", brg, brg - 1 - 5, True, table, HW * C),
                qng=QS("hb/ng_range", bng, bng - 1 - 3, True, table, HW * C))


GRID_C = [256, 64]


@pytest.mark.parametrize("C", GRID_C)
def test_pass_a_integer_grid_is_not_vacuous(C):
    cs = grid_case(C)
    dz = cs.oracle_dz()
    bw = cs.backward(dz)
    assert np.array_equal(bw["gq"][:, 0], np.where(cs.labels == 0, -12, 4)) and cs.forward()["cx"] == (0, 0)
    pa = bw["pa"]
    for name, operand, key in (("qrg", pa["gmask"], "crg"), ("qng", pa["d"], "cng")):
        q = cs.oq(name)
        xm = operand.astype(np.float64) * 2.0 ** HO.frac(q)
        L = 2.0 ** (q.bits - 1)
        for v in (L, -L, L / 2, -L / 2):
            assert np.any(xm == v), (name, v)
        assert np.any(xm % 1 == 0.5), name
        f1, f2 = DP.oracle_element_flags(operand, q.bits, q.I)
        for f in (f1, f2):
            assert 0 < f.sum() < f.size, name
        assert (int(f1.sum()), int(f2.sum())) == pa[key]
    ym = cs.ym
    for v in (F32(0.0), F32(-0.0), F32(2.0 ** -149), F32(-1.0)):
        assert np.any(ym.view(np.uint32) == v.view(np.uint32))
    # the subnormal passes the gradient, both zeros and the negative stop it
    g = np.broadcast_to(bw["g"][:, None, :], ym.shape)
    live = g != 0
    assert np.all(pa["gmask"][live & (ym == F32(2.0 ** -149))] != 0) and not np.any(pa["gmask"][ym <= 0])
    # sums from codes of mixed sign
    assert np.any(cs.R > 0) and np.any(cs.R < 0) and np.any(pa["G2"] > 0) and np.any(pa["G2"] < 0)
    assert np.all(np.any(pa["sums"] != 0, axis=1))


def test_wrong_heads_differ():
    """Teeth of the inputs of the GPU tests: pairwise pooling, a >= 0 mask, qx / qg counters added once per
    workgroup and a pad mask that lets sample N through each differ from the oracle on them."""
    pooled = [cs for cs in PLAIN if cs.HW >= 49]
    assert pooled and all(np.any(HO.wrong_pool_pairwise(cs.x) != cs.forward()["pooled"]) for cs in pooled)
    for C in GRID_C:
        cs = grid_case(C)
        bw = cs.backward(cs.oracle_dz())
        assert np.any(HO.wrong_mask_ge(bw["g"], cs.ym) != bw["pa"]["gmask"])
    multi = [cs for cs in MATRIX if cs.split() > 1]
    assert len(multi) >= 12
    for cs in multi:
        fw = cs.forward()
        cg = cs.backward(cs.oracle_dz())["cg"]
        assert HO.wrong_counts_per_workgroup(fw["cx"], cs.split()) != fw["cx"], case_id(cs)
        assert HO.wrong_counts_per_workgroup(cg, cs.split()) != cg, case_id(cs)
    for N, C, K in REDUCE_CASES:
        if N % 16 == 0:
            continue  # no pad byte follows the last sample
        cs = reduce_case(N, C, K)
        bw = cs.backward(cs.oracle_dz())
        pad = np.full(C, 0x7f), np.full(K, 0x7f)
        assert np.any(HO.wrong_reduce_pad(cs.forward()["pq"], bw["gq"], *pad) != bw["dw_int"])


REDUCE_CASES = [(N, C, K) for N in (1, 15, 16, 17, 33) for C, K in ((8, 3), (8, 64), (96, 10), (256, 64))]


def reduce_case(N, C, K, loss_n=0):
    return Case(N, 1, C, K, loss_n=loss_n)


# ------------------------------------------------------------------------------------------ GPU
import torch  # noqa: E402

from lbt_amd import _lib  # noqa: E402
from lbt_amd._lib import NSHARD, OUT_I8  # noqa: E402
from lbt_amd.dfxp import ops  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda"
POISON = 0x7f


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def same(got, exp, what):
    """Bit for bit (the sign of a zero included); integers by value."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if got.dtype.kind == "f":
        assert got.dtype == exp.dtype, (what, got.dtype, exp.dtype)
        bad = np.argwhere(bits_of(got) != bits_of(exp))
    else:
        bad = np.argwhere(got.astype(np.int64) != exp.astype(np.int64))
    assert len(bad) == 0, "%s: %d of %d differ, first at %s: got %r, expected %r" % (
        what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])])


def poisoned(shape, dt=torch.float32):
    """A buffer whose every BYTE is POISON."""
    n = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
    return torch.full((n,), POISON, dtype=torch.uint8, device=DEV).view(dt).reshape(shape)


class Run:
    """The device side of a case: operands, output buffers, descriptors. head(): lbt_head_fwd_bwd +
    lbt_step_reduce; seq(): the separate launches the header names. Both return every output as numpy."""

    def __init__(self, cs):
        self.cs = cs
        N, HW, C, K = cs.N, cs.HW, cs.C, cs.K
        self.Q = {k: s.gpu() for k, s in cs.q.items()}
        self.wq, self.W, self.labels = dev(cs.wq), dev(cs.W), dev(cs.labels)
        self.x = None if cs.chain else dev(cs.x)
        e = poisoned
        self.pooled, self.pq = e((N, C)), e((N, C), torch.int8)
        self.logits, self.dz, self.gq = e((N, K)), e((N, K)), e((N, K), torch.int8)
        self.loss, self.dW = e((1,)), e((C, K))
        self.gx = None if cs.pa else e((N, HW, C))
        self.scratch = torch.full((_lib.load().lbt_head_scratch_bytes(N, C, K),), POISON, dtype=torch.uint8, device=DEV)
        self.keep = []
        if cs.pa:
            self.gamma = dev(np.concatenate([cs.gamma, cs.beta if cs.chain else np.zeros(C, F32)]))
            self.gmask, self.gout = e((N, HW, C)), e((N, HW, C), torch.int8)
            self.sums = ops.new_sums(C, 4, DEV)
            self.qn = dev(cs.qn)
        if cs.chain:
            ql = cs.qn.reshape(-1, C).astype(np.int64)
            S = np.stack([ql.sum(0), (ql * ql).sum(0)]).reshape(-1)  # [S1 | S2], spread over the shards
            rng = np.random.default_rng(7)
            parts = rng.integers(-1000, 1000, (NSHARD, 2 * C)).astype(np.int64)
            parts[-1] += S - parts.sum(0)
            self.chsum = dev(parts.reshape(-1))
            self.res = dev(cs.res)
            self.ms, self.rm, self.rv = e((2 * C,)), dev(cs.rm0), dev(cs.rv0)
            self.y, self.rout = e((N, HW, C)), e((N, HW, C), torch.int8)
        elif cs.pa:
            self.ym, self.R = dev(cs.ym), dev(cs.R)

    def head_desc(self):
        cs = self.cs
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return _lib.Head(p(self.x), cs.N, cs.HW, cs.C, cs.K, p(self.pooled), p(self.pq), self.Q["qx"].desc, p(self.wq),
                         self.Q["qw"].desc, p(self.labels), p(self.logits), p(self.loss), p(self.dz), p(self.gq),
                         self.Q["qg"].desc, p(self.W), float(cs.wd2), p(self.dW), p(self.gx), p(self.scratch), cs.loss_n)

    def pa_desc(self, g, ym, R):
        cs = self.cs
        a = _lib.ChainBwdA()
        a.g = None if g is None else g.data_ptr()
        a.y_mask, a.gmask_out = ym.data_ptr(), self.gmask.data_ptr()
        a.b1 = _lib.BwdBranch(self.Q["qrg"].desc, R.data_ptr(), _lib.NO_Q, self.gamma.data_ptr(), self.Q["qng"].desc,
                              self.qn.data_ptr(), self.gout.data_ptr(), None, self.sums.data_ptr())
        a.rows, a.inner, a.C = cs.N, cs.HW * cs.C, cs.C
        return a

    def chain_desc(self):
        cs = self.cs
        ch = _lib.ChainFwd()
        ch.b1.nrm = _lib.BnNorm(self.qn.data_ptr(), self.Q["qn"].q.desc_nostats(), self.chsum.data_ptr(), cs.N * cs.HW,
                                cs.EPS, cs.MOM, cs.OMM, self.ms.data_ptr(), self.rm.data_ptr(), self.rv.data_ptr(), 0, 0)
        ch.b1.qr, ch.b1.rout, ch.b1.gb = self.Q["qr"].desc, self.rout.data_ptr(), self.gamma.data_ptr()
        ch.res, ch.relu, ch.y = self.res.data_ptr(), 1, self.y.data_ptr()
        ch.rows, ch.inner, ch.C = cs.N, cs.HW * cs.C, cs.C
        return ch

    def collect(self):
        torch.cuda.synchronize()
        cs = self.cs
        out = {k: getattr(self, k).cpu().numpy() for k in ("pooled", "pq", "logits", "dz", "gq", "loss", "dW")}
        if cs.pa:
            out.update(gmask=self.gmask.cpu().numpy(), gout=self.gout.cpu().numpy(),
                       sums=self.sums.view(NSHARD, 4, cs.C).sum(0).cpu().numpy())
        else:
            out["gx"] = self.gx.cpu().numpy()
        if cs.chain:
            out.update(ms=self.ms.cpu().numpy(), run_mean=self.rm.cpu().numpy(), run_var=self.rv.cpu().numpy())
        out["counts"] = {k: q.take_counts() for k, q in self.Q.items()}
        return out

    def head(self, xchg=False):
        cs = self.cs
        st = _lib.stream()
        h = self.head_desc()
        if cs.pa:  # with a chain the mask / R / qn operands come from registers: poisoned buffers here
            poison = torch.full((cs.N, cs.HW, cs.C), -1.0, device=DEV), torch.zeros((cs.N, cs.HW, cs.C), dtype=torch.int8, device=DEV)
            a = self.pa_desc(None, poison[0] if cs.chain else self.ym, poison[1] if cs.chain else self.R)
            if cs.chain:
                a.b1.qn_codes = poison[1].data_ptr()
            h.pa = ctypes.addressof(a)
            self.keep += [a, poison]
        if cs.chain:
            ch = self.chain_desc()
            h.chain = ctypes.addressof(ch)
            self.keep.append(ch)
        _lib.call("lbt_head_fwd_bwd", ctypes.byref(h), st)
        _lib.call("lbt_step_reduce", None, 0, 0, None, 0, 0, ctypes.byref(h), st)
        out = self.collect()
        NP = (cs.N + 15) & ~15
        scr = self.scratch.cpu().numpy()
        out["terms"] = scr[(cs.C + 64) * NP:].view(np.float64).copy()
        out["scratch_pq"] = scr[:cs.C * NP].view(np.int8).reshape(cs.C, NP).copy()
        out["scratch_gq"] = scr[cs.C * NP:(cs.C + 64) * NP].view(np.int8).reshape(64, NP).copy()
        if cs.chain:  # the chain's y / R are not written by the head
            assert torch.all(self.rout == POISON) and torch.all(self.y.view(torch.uint8) == POISON)
        # the header's contract for the transcendental step: lbt_softmax_xent_n on the head's own logits
        dz2, loss2 = torch.empty_like(self.dz), torch.empty_like(self.loss)
        _lib.call("lbt_softmax_xent_n", _lib.ptr(self.logits), _lib.ptr(self.labels), cs.N, cs.K, cs.norm,
                  _lib.ptr(loss2), _lib.ptr(dz2), None, st)
        out["dz_ref"], out["loss_ref"] = dz2.cpu().numpy(), loss2.cpu().numpy()
        if xchg:  # lbt_step_reduce_x's head block: the integer numerators and the 2^-32 fixed-point loss
            n = cs.C * cs.K
            buf = torch.full((n + 1,), -77, dtype=torch.int64, device=DEV)
            xd = _lib.Xchg(buf.data_ptr(), self.dW.data_ptr(), 1, 0, None, 0, n)
            _lib.call("lbt_step_reduce_x", None, 0, 0, None, 0, 0, ctypes.byref(h), ctypes.byref(xd), st)
            torch.cuda.synchronize()
            out["xbuf"] = buf.cpu().numpy()
        return out

    def seq(self):
        cs = self.cs
        N, HW, C, K = cs.N, cs.HW, cs.C, cs.K
        st = _lib.stream()
        dx, dg, dw = self.Q["qx"].desc, self.Q["qg"].desc, self.Q["qw"].desc
        x = self.x
        if cs.chain:
            _lib.call("lbt_bn_chain_fwd", ctypes.byref(self.chain_desc()), st)
            x = self.y
        dd = _lib.ConvDesc(N, 1, 1, C, K, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1)
        _lib.call("lbt_avgpool_fwd", _lib.ptr(x), _lib.ptr(self.pooled), N, HW, C, st)
        _lib.call("lbt_dfxp_quantize", _lib.ptr(self.pooled), _lib.ptr(self.pq), OUT_I8, N, C, dx, None, 0, st)
        _lib.call("lbt_conv_fwd_generic", _lib.ptr(self.pq), 0, _lib.ptr(self.wq), dd, dx, dw, _lib.ptr(self.logits), st)
        _lib.call("lbt_softmax_xent_n", _lib.ptr(self.logits), _lib.ptr(self.labels), N, K, cs.norm, _lib.ptr(self.loss),
                  _lib.ptr(self.dz), None, st)
        _lib.call("lbt_dfxp_quantize", _lib.ptr(self.dz), _lib.ptr(self.gq), OUT_I8, N, K, dg, None, 0, st)
        ns = ops.wgrad_nsplit(dd, generic=True)
        slab = torch.empty((ns, C, K), dtype=torch.int32, device=DEV)
        _lib.call("lbt_conv_wgrad_generic", _lib.ptr(self.pq), 0, _lib.ptr(self.gq), dd, _lib.ptr(slab), ns, st)
        _lib.call("lbt_conv_wgrad_reduce", _lib.ptr(slab), ns, C, K, 0, None, dx, dg, _lib.ptr(self.W), float(cs.wd2),
                  _lib.ptr(self.dW), st)
        dp = torch.empty((N, C), device=DEV)
        _lib.call("lbt_conv_dgrad_generic", _lib.ptr(self.gq), _lib.ptr(self.wq), dd, dg, dw, _lib.ptr(dp), None, st)
        gx = self.gx if self.gx is not None else torch.empty((N, HW, C), device=DEV)
        _lib.call("lbt_avgpool_bwd", _lib.ptr(dp), _lib.ptr(gx), N, HW, C, st)
        if cs.pa:
            a = self.pa_desc(gx, self.y if cs.chain else self.ym, self.rout if cs.chain else self.R)
            _lib.call("lbt_bn_chain_bwd_a", ctypes.byref(a), st)
        return self.collect()


def check_oracle(cs, out, what=""):
    """Every output of a head run against the oracle: the forward outright, dz / loss against lbt_softmax_xent_n
    on the head's logits, and the backward against the oracle fed with the kernel's dz."""
    N, C, K = cs.N, cs.C, cs.K
    fw = cs.forward()
    w = (what + " ") if what else ""
    for k in ("pooled", "pq", "logits"):
        same(out[k], fw[k], w + k)
    assert out["counts"]["qx"] == fw["cx"], w + "qx counters"
    same(out["dz"], out["dz_ref"], w + "dz against lbt_softmax_xent_n")
    same(out["loss"], out["loss_ref"], w + "loss against lbt_softmax_xent_n")
    bw = cs.backward(out["dz"])
    same(out["gq"], bw["gq"], w + "gq")
    assert out["counts"]["qg"] == bw["cg"], w + "qg counters"
    assert out["counts"]["qw"] == (0, 0), w + "qw counters"
    same(out["dW"], bw["dW"], w + "dW")
    same(out["loss"].reshape(()), HO.loss_from_terms(out["terms"], cs.norm)[0], w + "loss from the terms")
    # the records: column n of pqT / gqT, pad bytes untouched
    same(out["scratch_pq"][:, :N], fw["pq"].T, w + "pqT")
    same(out["scratch_gq"][:K, :N], bw["gq"].T, w + "gqT")
    assert np.all(out["scratch_pq"][:, N:] == POISON) and np.all(out["scratch_gq"][:K, N:] == POISON), w + "record pads"
    if cs.pa:
        pa = bw["pa"]
        same(out["gmask"], pa["gmask"], w + "gmask_out")
        same(out["gout"], pa["gout"], w + "G codes")
        same(out["sums"], pa["sums"], w + "pass-A sums")
        assert out["counts"]["qrg"] == pa["crg"], w + "qrg counters"
        assert out["counts"]["qng"] == pa["cng"], w + "qng counters"
    else:
        same(out["gx"], bw["gx"], w + "gx")
    if cs.chain:
        ch = fw["chain"]
        for k in ("ms", "run_mean", "run_var"):  # ONE update: a second workgroup updating them would show
            same(out[k], ch[k], w + k)
        assert out["counts"]["qr"] == ch["cr"], w + "qr counters"
    return bw


def check_same_runs(a, b):
    for k, v in a.items():
        if k == "counts":
            assert v == b[k], (k, v, b[k])
        else:
            same(b[k], v, "head against the separate launches: " + k)


@gpu
@pytest.mark.parametrize("cs", MATRIX, ids=[case_id(c) for c in MATRIX])
def test_path_matrix(cs):
    """(a) Every shape of the path matrix against the oracle and against the separate launches."""
    print(case_id(cs), sorted(cs.paths()))
    head = Run(cs).head()
    check_oracle(cs, head)
    check_same_runs(Run(cs).seq(), head)


@gpu
@pytest.mark.parametrize("HW", [1, 4])
@pytest.mark.parametrize("C", [256, 8])
@pytest.mark.parametrize("stoch,table", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("bits,I", WCASES)
def test_qx_decision_points(bits, I, stoch, table, C, HW):
    """(b) The Dense_q X quantiser at its decision points: pooled, pq, the counters (HW = 4: S = 4, so only the lead
    workgroup may count) and dW after lbt_step_reduce."""
    qs = QS("hd/X_range", bits, I, stoch, table, C)
    for cls in DP.ALL_CLASSES:
        site = qs.sites(cls)
        for what, rs in site_blocks(cls, site):
            s = site[rs]
            cs = Case(len(s), HW, C, 4, table=table, x=qx_site_input(s, HW), qx=qs)
            assert cs.split() == (4 if HW == 4 else 1)
            out = Run(cs).head()
            check_oracle(cs, out, what)
            ok = np.isfinite(s) & (np.abs(s) < DP.FLT_MAX / HW)
            assert np.array_equal(out["pooled"].view(np.uint32)[ok], pool_exact(s)[ok]), what
            assert out["counts"]["qx"] == DP.oracle_counts(out["pooled"], bits, I), what


@gpu
def test_qg_tie_case():
    """(c) dz m = +0.5 / -1.5 exactly: half-even gives 0 / -2 (half-away 1 / -2, half-up 1 / -1)."""
    cs = tie_case()
    out = Run(cs).head()
    check_oracle(cs, out)
    onehot = np.arange(4)[None, :] == cs.labels[:, None]
    same(out["dz"], np.where(onehot, F32(-0.1875), F32(0.0625)).astype(F32), "dz")
    same(out["gq"], np.where(onehot, -2, 0), "gq")


@gpu
@pytest.mark.parametrize("stoch,table", MODES, ids=MODE_IDS)
def test_qg_saturation(stoch, table):
    """(c) e = 30: every |dz m| >= L, the codes clipped to -L / L - 1, both counters the element count."""
    N, K = 6, 5
    cs = Case(N, 2, 16, K, table=table, qg=QS("hd/grad_range", 8, 8 - 31, stoch, table, K))
    out = Run(cs).head()
    check_oracle(cs, out)
    assert np.all(np.abs(out["dz"]) * 2.0 ** 30 >= 128)
    same(out["gq"], np.where(out["dz"] > 0, 127, -128), "gq")
    assert out["counts"]["qg"] == (N * K, N * K)


@gpu
@pytest.mark.parametrize("table", [True, False], ids=["table", "philox"])
@pytest.mark.parametrize("C", GRID_C)
def test_pass_a_integer_grid(C, table):
    """(d) Pass A on an integer grid through both gradient quantisers (see grid_case): G codes, gmask_out, the four
    channel sums and both counter pairs, exactly; the y mask's special values on known places."""
    cs = grid_case(C, table)
    out = Run(cs).head()
    bw = check_oracle(cs, out)
    same(out["gq"][:, 0], np.where(cs.labels == 0, -12, 4), "gq[:, 0]")
    g = (np.where(cs.labels == 0, -12, 4)[:, None] * (np.arange(C) - C // 2)[None, :]).astype(F32) * F32(2.0 ** -8)
    same(bw["g"], g, "g")
    ym = np.broadcast_to(cs.ym, out["gmask"].shape)
    expect = np.where((ym > 0), np.broadcast_to(g[:, None, :], ym.shape), F32(0)).astype(F32)
    same(out["gmask"], expect, "gmask_out")
    assert np.all(out["gmask"][:, 0, 0::4] == 0) and np.all(out["gmask"][:, 1, 1::4] == 0)
    assert np.all(out["gmask"][:, 3, 3::4] == 0) and np.any(out["gmask"][:, 2, 2::4] != 0)


@gpu
@pytest.mark.parametrize("N,C,K", REDUCE_CASES)
def test_head_reduce(N, C, K):
    """(e) head_reduce on records whose pad bytes hold 0x7f (never written): dW from the exact integer pq^T gq by
    lbt_conv_wgrad_reduce's formula, the loss from the ordered double sum, and lbt_step_reduce_x's head block
    (integer numerators, the loss-term sum in 2^-32 fixed point)."""
    cs = reduce_case(N, C, K)
    out = Run(cs).head(xchg=True)
    bw = check_oracle(cs, out)
    same(out["xbuf"][:C * K].reshape(C, K), bw["dw_int"], "exchange numerators")
    assert out["xbuf"][C * K] == HO.loss_from_terms(out["terms"], cs.norm)[1]


@gpu
def test_head_reduce_global_loss_norm():
    """(e) loss_n = 4 N: dz and the loss are a shard's share of the global batch's."""
    cs = reduce_case(17, 96, 10, loss_n=68)
    out = Run(cs).head()
    check_oracle(cs, out)
    full = reduce_case(17, 96, 10)
    assert np.array_equal(full.forward()["logits"], cs.forward()["logits"])
    ref = Run(full).head()
    same(out["dz"], (ref["dz"] * F32(0.25)).astype(F32), "dz")  # 1 / 68 = (1 / 17) / 4: the scaling is exact


# ---- (f) rejections
def _reject_cases():
    def base(**kw):
        return dict(dict(N=3, HW=4, C=8, K=4, pa=False, chain=False), **kw)

    def chain(**kw):
        return base(**dict(dict(HW=64, C=64, K=10, chain=True), **kw))

    return [
        ("C=264", base(C=264)), ("C%8!=0", base(C=12)), ("K=0", base(), dict(K=0)), ("K=65", base(), dict(K=65)),
        ("HW=0", base(), dict(HW=0)), ("N=0", base(), dict(N=0)),
        ("x misaligned by 4", base(), dict(x=4)), ("wq misaligned by 1", base(), dict(wq=1)),
        ("scratch misaligned by 4", base(), dict(scratch=4)),
        ("pa with C=24", base(C=24, pa=True)), ("pa with has_b2", base(pa=True), dict(pa_has_b2=1)),
        ("pa with a nearest quantiser", base(pa=True), dict(pa_nearest=1)),
        ("pa with a zero-bit quantiser", base(pa=True), dict(pa_zero_bits=1)),
        ("chain without pa", chain(), dict(no_pa=1)), ("chain with inner != 4096", chain(HW=32)),
        ("chain with res misaligned", chain(), dict(res=4)), ("chain with the qr table misaligned", chain(), dict(qr_noise=4)),
        ("chain with an output quantiser", chain(), dict(chain_o1=1)), ("chain with frozen", chain(), dict(frozen=1))]


REJECT = _reject_cases()


@gpu
@pytest.mark.parametrize("case", REJECT, ids=[c[0] for c in REJECT])
def test_rejections(case):
    """(f) Every documented limit returns LBT_EINVAL and leaves the sentinel-filled outputs untouched."""
    kw = case[1]
    mut = case[2] if len(case) > 2 else {}
    C = kw["C"]
    legal_c = C if C % 8 == 0 and C <= 256 else 8  # operands of a legal size; the descriptor carries the illegal C
    cs = Case(kw["N"], kw["HW"], legal_c if not kw["pa"] else C, kw["K"], pa=kw["pa"] and 1024 % C == 0, chain=kw["chain"])
    r = Run(cs)
    if kw["pa"] and not cs.pa:  # pass A with C = 24: its operands built by hand (Case refuses nothing, Run needs them)
        rng = np.random.default_rng(0)
        shp = (cs.N, cs.HW, C)
        cs.q["qrg"], cs.q["qng"] = QS("hb/rg_range", 8, 0, True, True, cs.HW * C), QS("hb/ng_range", 8, 0, True, True, cs.HW * C)
        cs.ym, cs.R = rng.normal(0, 1, shp).astype(F32), rng.integers(-128, 128, shp).astype(np.int8)
        cs.qn, cs.gamma, cs.pa = cs.R.copy(), np.ones(C, F32), True
        r = Run(cs)
    h = r.head_desc()
    h.C = C
    keep = []
    if cs.pa:
        ym = r.ym if not cs.chain else torch.zeros((cs.N, cs.HW, cs.C), device=DEV)
        R = r.R if not cs.chain else torch.zeros((cs.N, cs.HW, cs.C), dtype=torch.int8, device=DEV)
        a = r.pa_desc(None, ym, R)
        a.has_b2 = mut.get("pa_has_b2", 0)
        if mut.get("pa_nearest"):
            a.b1.qng.stochastic = 0
        if mut.get("pa_zero_bits"):
            a.b1.qrg.bits = 0
        if not mut.get("no_pa"):
            h.pa = ctypes.addressof(a)
        else:  # a gx to write: only the chain's own demand for a pass A is left to refuse
            r.gx = poisoned((cs.N, cs.HW, cs.C))
            h.gx = r.gx.data_ptr()
        keep += [a, ym, R]
    if cs.chain:
        ch = r.chain_desc()
        if mut.get("res"):
            ch.res += mut["res"]
        if mut.get("qr_noise"):
            ch.b1.qr.noise += mut["qr_noise"]
        if mut.get("chain_o1"):
            o1 = torch.zeros((cs.N, cs.HW, cs.C), dtype=torch.int8, device=DEV)
            ch.o1, ch.o1_kind, ch.qo1 = o1.data_ptr(), OUT_I8, r.Q["qr"].desc
            keep.append(o1)
        ch.b1.nrm.frozen = mut.get("frozen", 0)
        h.chain = ctypes.addressof(ch)
        keep.append(ch)
    for k in ("K", "HW", "N"):
        if k in mut:
            setattr(h, k, mut[k])
    for k in ("x", "wq", "scratch"):
        if k in mut:
            setattr(h, k, getattr(h, k) + mut[k])
    rc = _lib.load().lbt_head_fwd_bwd(ctypes.byref(h), _lib.stream())
    torch.cuda.synchronize()
    assert rc == EINVAL, (case[0], rc)
    outs = [r.pooled, r.pq, r.logits, r.dz, r.gq, r.loss, r.dW, r.scratch] + ([r.gx] if r.gx is not None else [])
    if cs.pa:
        outs += [r.gmask, r.gout]
        assert not torch.any(r.sums)
    if cs.chain:
        outs += [r.ms, r.y, r.rout]
        same(r.rm.cpu().numpy(), cs.rm0, "running mean")
        same(r.rv.cpu().numpy(), cs.rv0, "running variance")
    for t in outs:
        assert torch.all(t.view(torch.uint8) == POISON), case[0]
    assert all(q.take_counts() == (0, 0) for q in r.Q.values())

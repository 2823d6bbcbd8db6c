"""The four fused 3x3 conv launches against the launches they replace, bit for bit, on inputs built for their
overflow counters (conv_fused.h ov_count2: lane masks counted on the scalar unit, one total per wave).

    lbt_conv_fwd_fused_i8   ==  lbt_bn_chain_fwd + lbt_conv_fwd_i8 (i8w4)
    lbt_conv_fwd2_fused_i8  ==  lbt_bn_chain_fwd + lbt_conv_fwd_pair_i8
    lbt_conv_bwd_fused_i8   ==  lbt_bn_chain_bwd_b + lbt_conv_dgrad_chain_i8 (i8w4)
    lbt_conv_bwd2_fused_i8  ==  lbt_bn_chain_bwd_b_pair + lbt_conv_dgrad2_chain_i8

Every output array, channel sum and counter of the fused launch must equal the unfused sequence's on the same
operands. The operands follow tests/test_decision_points.py: BN statistics that make mu = 0 and sigma = 1, so
that a quantiser fed from codes sees an integer grid, here 2 q: it holds T = L and L / 2 exactly, T + 2,
-T (not counted) and -T - 2 (counted). Only two quantisers take floats: the forward's X quantiser (through
the residual, with gamma = 0) and the backward's Rescale_q gradient quantiser (through add_src, with a zero
dgrad); those get T, T +- 1 ulp, -T, -T - 1 ulp, NaN and +-inf. `where` puts the values that can overflow on
every row ("owned") or only on the rows next to a tile boundary ("halo": rows that the neighbouring
workgroup also evaluates, as its halo, and must not count), everything else staying below L / 2.

Shapes: lbt_conv_fused_tile_rows picks the tile height from N * H, and the entry points take H % 8 == 0 at
16 channels and H % 4 == 0 at 32 / 64. So the 2-row tiles run at N = 2 with the smallest H (two tiles per
sample at 32 / 64 channels, four at 16: a sample of one 2-row tile does not exist); the 4-row tiles need
N * H >= 1024 (N = 256 at one tile per sample, N = 128 at two; at 16 channels only H = 8, two tiles); the
8-row tiles N * H >= 2048 (N = 256 at one tile, N = 64 at H = 32).
"""
import ctypes

import numpy as np
import pytest
import torch

import test_decision_points as TD
from lbt_amd import _lib
from lbt_amd._lib import NSHARD, OUT_U8OFF
from lbt_amd.dfxp import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
E_N = TD.E_N


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _buf(shape, dtype):
    return torch.full(tuple(shape), 77, dtype=dtype, device=DEV)


def _bits(t):
    """A tensor's bytes (NaNs compare equal)."""
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _sums(t, per_shard):
    return t.view(NSHARD, per_shard).sum(0)


def _stream():
    return _lib.stream()


def _boundary_rows(H, TH):
    """Rows of an H-row sample that lie in a neighbouring tile's halo."""
    return [y for y in range(H) if (y % TH == 0 and y > 0) or (y % TH == TH - 1 and y < H - 1)]


def _row_mask(N, H, rowlen, TH, where):
    """[N, H * rowlen] bool: the elements that may hold overflowing values."""
    m = np.ones((N, H, rowlen), dtype=bool)
    if where == "halo":
        m[:] = False
        m[:, _boundary_rows(H, TH), :] = True
        assert m.any(), "no halo row in this shape"
    return m.reshape(N, H * rowlen)


def _codes(rng, mask):
    """int8 codes: the whole range where mask, |q| < 16 elsewhere; 2 q hits 128, 130, -128, -130, 64, -66."""
    q = rng.integers(-128, 128, size=mask.shape)
    q[:, :12][mask[:, :12]] = np.resize([64, 65, -64, -65, 32, 33, -32, -33, 127, -128, 63, -63], mask[:, :12].sum())
    return np.where(mask, q, rng.integers(-15, 16, size=mask.shape)).astype(np.int8)


def _float_sites(rng, mask, T, lo):
    """fp32 operands of a quantiser whose thresholds are T and T / 2 (operand units): random values of which
    some overflow where mask (below lo * T elsewhere), and on the masked elements of every sample T, T / 2 and
    -T at -1, 0, +1 ulp, NaN and +-inf."""
    x = (rng.uniform(-1.3, 1.3, size=mask.shape) * T).astype(F32)
    x = np.where(mask, x, x * F32(lo / 1.3)).astype(F32)
    T = F32(T)
    sites = []
    for t in (T, T / 2, -T, -T / 2):
        sites += [np.nextafter(t, F32(0)), t, np.nextafter(t, F32(np.sign(t) * np.inf))]
    sites += [F32(np.nan), F32(np.inf), F32(-np.inf)]
    for n in range(x.shape[0]):
        idx = np.flatnonzero(mask[n])
        pick = idx[rng.permutation(len(idx))[:4 * len(sites)]]  # spread over lanes and waves
        x[n, pick] = np.resize(np.asarray(sites, dtype=F32), len(pick))
    return x


def _weights(rng, rows, cin, taps, zero=False):
    """A weight image [rows][slices * 16] of codes in [-2, 2] (slice = tap * cin / 16 + channel / 16, padded to 4
    slices), its column sums, and the slice count."""
    ks = ops.packed_slices(taps, 1, cin)
    w = np.zeros((rows, ks * 16), dtype=np.int8)
    if not zero:
        w[:, :taps * cin] = rng.integers(-2, 3, size=(rows, taps * cin))
    return _dev(w), _dev(w.astype(np.int32).sum(1).astype(np.int32)), ks


def _image(w, w4):
    if not w4:
        return w
    img = torch.zeros((w.shape[0], w.shape[1] // 2), dtype=torch.uint8, device=DEV)
    ops.pack_int4(w, img)
    return img


def _moment_sums(C, n):
    """Channel sums [NSHARD][2C] that give mu = 0 and sigma = 1 at eps = 0 for codes of exponent E_N."""
    chs = np.zeros((NSHARD, 2 * C), dtype=np.int64)
    chs[0, C:] = n * 4 ** E_N
    return _dev(chs.reshape(-1))


class _Quants:
    """Named quantisers (TD.Quant: one context each) and their counters after a launch."""

    def __init__(self):
        self.q, self.counted = {}, []

    def add(self, name, bits, e, inner=None):
        """inner: the quantiser rounds [rows, inner] operands with a noise table, and its counters are compared."""
        self.q[name] = TD.Quant(bits, bits - 1 - e, True, inner is not None, inner or TD.INNER, name="fc/%s_range" % name)
        if inner is not None:
            self.counted.append(name)
        return self.q[name]

    def take(self):
        torch.cuda.synchronize()
        return {k: self.q[k].take_counts() for k in self.counted}


def _assert_equal_runs(got, want, cnt_got, cnt_want, elems):
    for k in want:
        assert torch.equal(_bits(got[k]), _bits(want[k])), k
    assert cnt_got == cnt_want
    for k, (c1, c2) in cnt_want.items():  # not vacuous: both thresholds crossed, and not by everything
        assert 0 < c1 <= c2 < elems[k], (k, c1, c2, elems[k])


# ---------------------------------------------------------------------------------------- stride-1 forward
def _fwd_case(C, H, N, nb, res, w4, where, seed):
    TH = _lib.load().lbt_conv_fused_tile_rows(C, N, H)
    W, inner, n = 512 // C, H * 512, N * H * (512 // C)
    shp = (N, H, W, C)
    rng = np.random.default_rng(seed)
    mask = _row_mask(N, H, 512, TH, where)
    Q = _Quants()
    e_r, e_x, e_out = E_N + 1, 7, 5
    sh = 5 + (C == 64)  # the conv sum's deviation is about 2^(sh + 6) codes: the output quantiser sees about 64
    qw = Q.add("w", 4 if w4 else 8, sh + e_out - e_x)
    Q.add("x", 9, e_x, inner)
    Q.add("out", 8, e_out, inner)
    wf, colsum, ksf = _weights(rng, C, C, 9)
    img = _image(wf, w4)
    keep = [wf, colsum, img]
    cf = _lib.ConvFwd()
    a = cf.c
    for b in range(nb):
        br = a.b1 if b == 0 else a.b2
        q = _dev(_codes(rng, mask).reshape(shp))
        chsum = _moment_sums(C, n)
        # gamma = 0 with a residual: v = res exactly; else 4: the X quantiser sees 4 R (L / 2 at R = 32, L at 64)
        gb = _dev(np.concatenate([np.full(C, 0.0 if res else (4.0 if b == 0 else 2.0)), np.zeros(C)]).astype(F32))
        Q.add("n%d" % b, 8, E_N)
        Q.add("r%d" % b, 8, e_r, inner)
        br.nrm = _lib.BnNorm(q.data_ptr(), Q.q["n%d" % b].q.desc_nostats(), chsum.data_ptr(), n, 0.0, 0.999, 0.001, None,
                             None, None, 0, 0)
        br.qr, br.gb = Q.q["r%d" % b].desc, gb.data_ptr()
        keep += [q, chsum, gb]
    a.has_b2 = int(nb == 2)
    a.relu = 1
    a.o1_kind, a.qo1 = OUT_U8OFF, Q.q["x"].desc
    a.rows, a.inner, a.C = N, inner, C
    if res:
        rt = _dev(_float_sites(rng, mask, 256.0 * 2.0 ** -e_x, 0.45).reshape(shp))
        a.res = rt.data_ptr()
        keep.append(rt)
    cf.wf, cf.ksf, cf.w4, cf.wcolsum = img.data_ptr(), ksf, int(w4), colsum.data_ptr()
    cf.d = ops.conv_desc(N, H, W, C, C, 3, 3, 1, 1, "SAME")
    cf.qw, cf.qout = qw.q.desc_nostats(), Q.q["out"].desc

    def outputs(c):
        """Fresh output buffers into a copy of the descriptor."""
        c = _lib.ConvFwd.from_buffer_copy(c)
        out = {"yq": _buf(shp, torch.int8), "o1": _buf(shp, torch.int8), "ychsum": ops.new_sums(C, 2, DEV)}
        c.yq, c.c.o1, c.ychsum = out["yq"].data_ptr(), out["o1"].data_ptr(), out["ychsum"].data_ptr()
        for b in range(nb):
            br = c.c.b1 if b == 0 else c.c.b2
            out["R%d" % b], out["ms%d" % b] = _buf(shp, torch.int8), _buf((2 * C,), torch.float32)
            br.rout, br.nrm.ms = out["R%d" % b].data_ptr(), out["ms%d" % b].data_ptr()
        if res or nb == 2:
            out["y"] = _buf(shp, torch.float32)
            c.c.y = out["y"].data_ptr()
        return c, out

    elems = {k: N * inner for k in Q.q}
    return dict(cf=cf, outputs=outputs, Q=Q, keep=keep, TH=TH, tiles=N * H // TH, elems=elems, C=C, w4=w4, img=img,
                colsum=colsum, ksf=ksf)


def _run_fwd(case):
    Q = case["Q"]
    cf, got = case["outputs"](case["cf"])
    _lib.call("lbt_conv_fwd_fused_i8", ctypes.byref(cf), _stream())
    cnt_got = Q.take()
    cu, want = case["outputs"](case["cf"])
    _lib.call("lbt_bn_chain_fwd", ctypes.byref(cu.c), _stream())
    _lib.call("lbt_conv_fwd_i8w4" if case["w4"] else "lbt_conv_fwd_i8", _lib.ptr(want["o1"]), 1, _lib.ptr(case["img"]),
              case["ksf"], _lib.ptr(case["colsum"]), cu.d, cu.c.qo1, cu.qw, None, _lib.ptr(want["yq"]), cu.qout,
              _lib.ptr(want["ychsum"]), _stream())
    cnt_want = Q.take()
    for o in (got, want):
        o["ychsum"] = _sums(o["ychsum"], 2 * case["C"])
    _assert_equal_runs(got, want, cnt_got, cnt_want, case["elems"])


# (C, H, N, tile rows): one tile and two tiles per sample at every tile height the rule can select
S1_SHAPES = [(16, 8, 2, 2), (16, 8, 128, 4), (16, 8, 256, 8), (16, 32, 64, 8),
             (32, 4, 2, 2), (32, 4, 256, 4), (32, 8, 128, 4),
             (64, 4, 2, 2), (64, 4, 256, 4), (64, 8, 128, 4)]
S1_IDS = ["C%d_H%d_N%d_th%d" % s for s in S1_SHAPES]
TWO_TILE = [(16, 8, 2, 2), (32, 8, 128, 4), (64, 4, 2, 2), (16, 32, 64, 8)]


@pytest.mark.parametrize("C,H,N,rows", S1_SHAPES, ids=S1_IDS)
def test_fwd_fused_equals_chain_then_conv(C, H, N, rows):
    """The residual variant: float sites into the X quantiser, the integer grid into qr, conv sums into qout."""
    case = _fwd_case(C, H, N, 1, True, False, "owned", seed=C + H + N)
    assert case["TH"] == rows and case["tiles"] > 1
    _run_fwd(case)


@pytest.mark.parametrize("nb,res,w4", [(1, False, False), (2, False, False), (1, True, True)],
                         ids=["bn1", "two_branch", "w4"])
def test_fwd_fused_variants(nb, res, w4):
    case = _fwd_case(32, 4, 2, nb, res, w4, "owned", seed=7 + nb + w4)
    assert case["tiles"] > 1 and 4 // case["TH"] == 2  # interior halo present
    _run_fwd(case)


@pytest.mark.parametrize("C,H,N,rows", TWO_TILE, ids=["C%d_H%d_N%d_th%d" % s for s in TWO_TILE])
def test_fwd_fused_thresholds_on_halo_rows_only(C, H, N, rows):
    """Everything that can overflow lies on rows that two workgroups evaluate: a mask counted by the workgroup
    that does not own the row makes the totals differ from the unfused launches'."""
    case = _fwd_case(C, H, N, 1, True, False, "halo", seed=3 * C + H)
    assert case["TH"] == rows and H // rows >= 2
    _run_fwd(case)


# ---------------------------------------------------------------------------------------- stride-1 backward
def _bwd_case(C, H, N, nb, w4, where, seed, sites):
    TH = _lib.load().lbt_conv_fused_tile_rows(C, N, H)
    W, inner, n = 512 // C, H * 512, N * H * (512 // C)
    shp = (N, H, W, C)
    rng = np.random.default_rng(seed)
    mask = _row_mask(N, H, 512, TH, where)
    Q = _Quants()
    e_o, e_rg, e_ng = E_N + 1, 5, 6
    sh = 5 + (C == 64)
    Q.add("g", 8, E_N)
    Q.add("x", 8, 5)
    qw = Q.add("w", 4 if w4 else 8, sh + e_rg - e_o)
    Q.add("o", 8, e_o, inner)
    G = _dev(_codes(rng, mask).reshape(shp))
    zeros8 = torch.zeros(shp, dtype=torch.int8, device=DEV)
    ms = torch.cat([torch.zeros(C), torch.ones(C)]).to(DEV)
    bsums = ops.new_sums(C, 4, DEV)
    wd, _, ksd = _weights(rng, C, C, 9, zero=sites)  # sites: g = add_src exactly
    img = _image(wd, w4)
    # add_src: the float sites of qrg (thresholds L 2^-e_rg and half of it), or noise well below them
    add = _float_sites(rng, mask, 128.0 * 2.0 ** -e_rg, 0.45) if sites else (rng.uniform(-.2, .2, (N, inner))).astype(F32)
    addt = _dev(add.reshape(shp))
    ym = _dev((rng.random(shp) > 0.1).astype(F32))
    p = _lib.ConvBwd()
    p.b = _lib.ChainBwdB(G.data_ptr(), Q.q["g"].desc, zeros8.data_ptr(), Q.q["x"].desc, ms.data_ptr(), bsums.data_ptr(), n,
                         None, None, Q.q["o"].desc, None, N, inner, C)
    p.wd, p.ksd, p.w4 = img.data_ptr(), ksd, int(w4)
    p.d = ops.conv_desc(N, H, W, C, C, 3, 3, 1, 1, "SAME")
    p.qw = qw.q.desc_nostats()
    p.add_src = addt.data_ptr()
    p.a.y_mask = ym.data_ptr()
    keep = [G, zeros8, ms, bsums, wd, img, addt, ym]
    for b in range(nb):
        Q.add("rg%d" % b, 8, e_rg, inner)
        Q.add("ng%d" % b, 8, e_ng + b, inner)
        R = _dev(rng.integers(-128, 128, size=shp, dtype=np.int8))
        qn = _dev(rng.integers(-128, 128, size=shp, dtype=np.int8))
        gb = TD.unit_gb(C)
        br = _lib.BwdBranch(Q.q["rg%d" % b].desc, R.data_ptr(), _lib.NO_Q, gb.data_ptr(), Q.q["ng%d" % b].desc,
                            qn.data_ptr(), None, None, None)
        if b == 0:
            p.a.b1 = br
        else:
            p.a.b2 = br
        keep += [R, qn, gb]
    p.a.has_b2 = int(nb == 2)
    p.a.rows, p.a.inner, p.a.C = N, inner, C

    def outputs(c):
        c = _lib.ConvBwd.from_buffer_copy(c)
        out = {"gq": _buf(shp, torch.int8), "gcol": ops.new_sums(C, 2, DEV)}
        c.b.gq, c.b.gcolsum = out["gq"].data_ptr(), out["gcol"].data_ptr()
        if nb == 1:  # the two-branch instantiations store no masked gradient
            out["gmask"] = _buf(shp, torch.float32)
            c.a.gmask_out = out["gmask"].data_ptr()
        for b in range(nb):
            br = c.a.b1 if b == 0 else c.a.b2
            out["G%d" % b], out["asums%d" % b] = _buf(shp, torch.int8), ops.new_sums(C, 4, DEV)
            br.gout, br.sums = out["G%d" % b].data_ptr(), out["asums%d" % b].data_ptr()
        return c, out

    elems = {k: N * inner for k in Q.q}
    return dict(p=p, outputs=outputs, Q=Q, keep=keep, TH=TH, tiles=N * H // TH, elems=elems, C=C, w4=w4, img=img, ksd=ksd,
                addt=addt, nb=nb)


def _run_bwd(case):
    Q, C = case["Q"], case["C"]
    p, got = case["outputs"](case["p"])
    _lib.call("lbt_conv_bwd_fused_i8", ctypes.byref(p), _stream())
    cnt_got = Q.take()
    pu, want = case["outputs"](case["p"])
    _lib.call("lbt_bn_chain_bwd_b", ctypes.byref(pu.b), _stream())
    _lib.call("lbt_conv_dgrad_chain_i8w4" if case["w4"] else "lbt_conv_dgrad_chain_i8", _lib.ptr(want["gq"]),
              _lib.ptr(case["img"]), case["ksd"], pu.d, pu.b.qo, pu.qw, _lib.ptr(case["addt"]), ctypes.byref(pu.a), _stream())
    cnt_want = Q.take()
    for o in (got, want):
        o["gcol"] = _sums(o["gcol"], 2 * C)
        for b in range(case["nb"]):
            o["asums%d" % b] = _sums(o["asums%d" % b], 4 * C)
    _assert_equal_runs(got, want, cnt_got, cnt_want, case["elems"])


@pytest.mark.parametrize("C,H,N,rows", S1_SHAPES, ids=S1_IDS)
def test_bwd_fused_equals_chain_then_dgrad(C, H, N, rows):
    """Random dgrad weights: the integer grid into qo (halo included), the dgrad sums into qrg, its codes into qng."""
    case = _bwd_case(C, H, N, 1, False, "owned", seed=C + H + N + 1, sites=False)
    assert case["TH"] == rows and case["tiles"] > 1
    _run_bwd(case)


@pytest.mark.parametrize("nb,w4,sites", [(1, False, True), (2, False, False), (2, False, True), (1, True, False)],
                         ids=["float_sites", "two_branch", "two_branch_float_sites", "w4"])
def test_bwd_fused_variants(nb, w4, sites):
    case = _bwd_case(32, 4, 2, nb, w4, "owned", seed=11 + nb + w4 + sites, sites=sites)
    assert case["tiles"] > 1 and 4 // case["TH"] == 2
    _run_bwd(case)


@pytest.mark.parametrize("sites", [False, True], ids=["grid", "float_sites"])
@pytest.mark.parametrize("C,H,N,rows", TWO_TILE, ids=["C%d_H%d_N%d_th%d" % s for s in TWO_TILE])
def test_bwd_fused_thresholds_on_halo_rows_only(C, H, N, rows, sites):
    case = _bwd_case(C, H, N, 1, False, "halo", seed=5 * C + H + sites, sites=sites)
    assert case["TH"] == rows and H // rows >= 2
    _run_bwd(case)


# ---------------------------------------------------------------------------------------- the transitions
def _edge_mask(N, H, W, C, where):
    """Transition kernels: `edges` keeps the overflowing values on the last two input rows (the last output
    row reads the bottom padding row below them) and on columns 0, 1 and W - 1."""
    m = np.ones((N, H, W, C), dtype=bool)
    if where == "edges":
        m[:] = False
        m[:, H - 2:, :, :] = True
        m[:, :, [0, 1, W - 1], :] = True
    return m.reshape(N, H * W * C)


def _fwd2_case(C, N, w4, where, seed):
    H = 512 // C
    W, d1, ds = TD._transition_descs(N, H, C)
    Cq, inner, n = 2 * C, H * 512, N * H * W
    inner_o = d1.Ho * d1.Wo * Cq
    shp, oshp = (N, H, W, C), (N, d1.Ho, d1.Wo, Cq)
    rng = np.random.default_rng(seed)
    mask = _edge_mask(N, H, W, C, where)
    Q = _Quants()
    e_r, e_x, e_out, sh = E_N + 1, 7, 5, 5
    bits_w = 4 if w4 else 8
    Q.add("n", 8, E_N)
    Q.add("r", 8, e_r, inner)
    Q.add("x1", 9, e_x, inner)
    Q.add("x2", 9, e_x, inner)
    qw1, qws = Q.add("w1", bits_w, sh + e_out - e_x), Q.add("ws", bits_w, sh - 2 + e_out - e_x)
    Q.add("o1", 8, e_out, inner_o)
    Q.add("os", 8, e_out, inner_o)
    q = _dev(_codes(rng, mask).reshape(shp))
    chsum = _moment_sums(C, n)
    gb = _dev(np.zeros(2 * C, dtype=F32))  # gamma = beta = 0: v = res
    rt = _dev(_float_sites(rng, mask, 256.0 * 2.0 ** -e_x, 0.45).reshape(shp))
    wf1, col1, ksf1 = _weights(rng, Cq, C, 9)
    wfs, cols, ksfs = _weights(rng, Cq, C, 1)
    img1, imgs = _image(wf1, w4), _image(wfs, w4)
    cf = _lib.ConvFwd2()
    a = cf.c
    a.b1.nrm = _lib.BnNorm(q.data_ptr(), Q.q["n"].q.desc_nostats(), chsum.data_ptr(), n, 0.0, 0.999, 0.001, None, None, None,
                           0, 0)
    a.b1.qr, a.b1.gb = Q.q["r"].desc, gb.data_ptr()
    a.res, a.relu = rt.data_ptr(), 1
    a.o1_kind, a.qo1, a.o2_kind, a.qo2 = OUT_U8OFF, Q.q["x1"].desc, OUT_U8OFF, Q.q["x2"].desc
    a.rows, a.inner, a.C = N, inner, C
    cf.wf1, cf.ksf1, cf.wcolsum1 = img1.data_ptr(), ksf1, col1.data_ptr()
    cf.wfs, cf.ksfs, cf.wcolsums = imgs.data_ptr(), ksfs, cols.data_ptr()
    cf.w4, cf.d1, cf.ds = int(w4), d1, ds
    cf.qw1, cf.qws = qw1.q.desc_nostats(), qws.q.desc_nostats()
    cf.qout1, cf.qouts = Q.q["o1"].desc, Q.q["os"].desc
    keep = [q, chsum, gb, rt, wf1, col1, wfs, cols, img1, imgs]

    def outputs(c):
        c = _lib.ConvFwd2.from_buffer_copy(c)
        out = {"R": _buf(shp, torch.int8), "ms": _buf((2 * C,), torch.float32), "y": _buf(shp, torch.float32),
               "o1": _buf(shp, torch.int8), "o2": _buf(shp, torch.int8), "yq1": _buf(oshp, torch.int8),
               "yqs": _buf(oshp, torch.int8), "ych1": ops.new_sums(Cq, 2, DEV), "ychs": ops.new_sums(Cq, 2, DEV)}
        c.c.b1.rout, c.c.b1.nrm.ms, c.c.y = out["R"].data_ptr(), out["ms"].data_ptr(), out["y"].data_ptr()
        c.c.o1, c.c.o2 = out["o1"].data_ptr(), out["o2"].data_ptr()
        c.yq1, c.ychsum1, c.yqs, c.ychsums = (out[k].data_ptr() for k in ("yq1", "ych1", "yqs", "ychs"))
        return c, out

    elems = {k: N * (inner_o if k in ("o1", "os") else inner) for k in Q.q}
    cf, got = outputs(cf)
    _lib.call("lbt_conv_fwd2_fused_i8", ctypes.byref(cf), _stream())
    cnt_got = Q.take()
    cu, want = outputs(cf)
    _lib.call("lbt_bn_chain_fwd", ctypes.byref(cu.c), _stream())
    jobs = [_lib.ConvFwdJob(want[x].data_ptr(), 1, int(w4), im.data_ptr(), ks, col.data_ptr(), d, qx, qw, None,
                            want[y].data_ptr(), qo, want[s].data_ptr())
            for x, im, ks, col, d, qx, qw, y, qo, s in (
                ("o1", img1, ksf1, col1, d1, cu.c.qo1, cu.qw1, "yq1", cu.qout1, "ych1"),
                ("o2", imgs, ksfs, cols, ds, cu.c.qo2, cu.qws, "yqs", cu.qouts, "ychs"))]
    _lib.call("lbt_conv_fwd_pair_i8", ctypes.byref(jobs[0]), ctypes.byref(jobs[1]), _stream())
    cnt_want = Q.take()
    for o in (got, want):
        o["ych1"], o["ychs"] = _sums(o["ych1"], 2 * Cq), _sums(o["ychs"], 2 * Cq)
    assert N * d1.Ho // 4 > 1  # workgroups (4 output rows each)
    _assert_equal_runs(got, want, cnt_got, cnt_want, elems)
    del keep


@pytest.mark.parametrize("C,w4,where", [(16, False, "owned"), (32, False, "owned"), (16, True, "owned"),
                                        (16, False, "edges"), (32, False, "edges")],
                         ids=["C16", "C32", "C16_w4", "C16_edges", "C32_edges"])
def test_fwd2_fused_equals_chain_then_pair(C, w4, where):
    _fwd2_case(C, 2, w4, where, seed=60 + C + w4)


def _bwd2_case(C, N, w4, where, seed):
    H = 512 // C
    W, d1, ds = TD._transition_descs(N, H, C)
    Cq = 2 * C
    inner, inq, nq = H * 512, d1.Ho * d1.Wo * Cq, N * d1.Ho * d1.Wo
    shp, oshp = (N, H, W, C), (N, d1.Ho, d1.Wo, Cq)
    rng = np.random.default_rng(seed)
    mask = _edge_mask(N, d1.Ho, d1.Wo, Cq, where)
    Q = _Quants()
    e_o, e_rg, e_ng, sh = E_N + 1, 5, 6, 5
    bits_w = 4 if w4 else 8
    Q.add("g", 8, E_N)
    Q.add("x", 8, 5)
    qw1, qws = Q.add("w1", bits_w, sh + e_rg - e_o), Q.add("ws", bits_w, sh - 2 + e_rg - e_o)
    Q.add("rg", 8, e_rg, inner)
    Q.add("ng", 8, e_ng, inner)
    zeros8 = torch.zeros(oshp, dtype=torch.int8, device=DEV)
    ms = torch.cat([torch.zeros(Cq), torch.ones(Cq)]).to(DEV)
    bsums = ops.new_sums(Cq, 4, DEV)
    wd1, _, ksd1 = _weights(rng, C, Cq, 9)
    wds, _, ksds = _weights(rng, C, Cq, 1)
    img1, imgs = _image(wd1, w4), _image(wds, w4)
    p = _lib.ConvBwd2()
    keep = [zeros8, ms, bsums, wd1, wds, img1, imgs]
    for name in ("o1", "os"):
        Q.add(name, 8, e_o, inq)
        G = _dev(_codes(rng, mask).reshape(oshp))
        b = _lib.ChainBwdB(G.data_ptr(), Q.q["g"].desc, zeros8.data_ptr(), Q.q["x"].desc, ms.data_ptr(), bsums.data_ptr(), nq,
                           None, None, Q.q[name].desc, None, N, inq, Cq)
        if name == "o1":
            p.b1 = b
        else:
            p.bs = b
        keep.append(G)
    p.wd1, p.ksd1, p.wds, p.ksds, p.w4 = img1.data_ptr(), ksd1, imgs.data_ptr(), ksds, int(w4)
    p.d1, p.ds = d1, ds
    p.qw1, p.qws = qw1.q.desc_nostats(), qws.q.desc_nostats()
    R = _dev(rng.integers(-128, 128, size=shp, dtype=np.int8))
    qn = _dev(rng.integers(-128, 128, size=shp, dtype=np.int8))
    ym = _dev((rng.random(shp) > 0.1).astype(F32))
    gb = TD.unit_gb(C)
    p.a.y_mask = ym.data_ptr()
    p.a.b1 = _lib.BwdBranch(Q.q["rg"].desc, R.data_ptr(), _lib.NO_Q, gb.data_ptr(), Q.q["ng"].desc, qn.data_ptr(), None, None,
                            None)
    p.a.rows, p.a.inner, p.a.C = N, inner, C
    keep += [R, qn, ym, gb]

    def outputs(c):
        c = _lib.ConvBwd2.from_buffer_copy(c)
        out = {"gq1": _buf(oshp, torch.int8), "gqs": _buf(oshp, torch.int8), "gcol1": ops.new_sums(Cq, 2, DEV),
               "gcols": ops.new_sums(Cq, 2, DEV), "gmask": _buf(shp, torch.float32), "G": _buf(shp, torch.int8),
               "asums": ops.new_sums(C, 4, DEV)}
        c.b1.gq, c.b1.gcolsum, c.bs.gq, c.bs.gcolsum = (out[k].data_ptr() for k in ("gq1", "gcol1", "gqs", "gcols"))
        c.a.gmask_out, c.a.b1.gout, c.a.b1.sums = out["gmask"].data_ptr(), out["G"].data_ptr(), out["asums"].data_ptr()
        return c, out

    elems = {k: N * (inq if k in ("o1", "os") else inner) for k in Q.q}
    pf, got = outputs(p)
    _lib.call("lbt_conv_bwd2_fused_i8", ctypes.byref(pf), _stream())
    cnt_got = Q.take()
    pu, want = outputs(p)
    _lib.call("lbt_bn_chain_bwd_b_pair", ctypes.byref(pu.bs), ctypes.byref(pu.b1), _stream())
    _lib.call("lbt_conv_dgrad2_chain_i8", _lib.ptr(want["gq1"]), _lib.ptr(img1), ksd1, d1, pu.b1.qo, pu.qw1,
              _lib.ptr(want["gqs"]), _lib.ptr(imgs), ksds, ds, pu.bs.qo, pu.qws, int(w4), ctypes.byref(pu.a), _stream())
    cnt_want = Q.take()
    for o in (got, want):
        o["gcol1"], o["gcols"], o["asums"] = _sums(o["gcol1"], 2 * Cq), _sums(o["gcols"], 2 * Cq), _sums(o["asums"], 4 * C)
    _assert_equal_runs(got, want, cnt_got, cnt_want, elems)
    del keep


@pytest.mark.parametrize("C,w4,where", [(16, False, "owned"), (32, False, "owned"), (16, True, "owned"),
                                        (16, False, "edges"), (32, False, "edges")],
                         ids=["C16", "C32", "C16_w4", "C16_edges", "C32_edges"])
def test_bwd2_fused_equals_pair_then_dgrad2(C, w4, where):
    """No float reaches this entry point's quantisers (no add_src): integer grids into both gradient
    quantisers, the two dgrads' sums into qrg, its codes into qng."""
    _bwd2_case(C, 2, w4, where, seed=80 + C + w4)

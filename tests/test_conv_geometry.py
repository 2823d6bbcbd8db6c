"""Every conv kernel family on non-square geometry against the numpy oracle.

``Conv2d_q`` takes any ``ksize = [KH, KW, Cin, Cout]``, any ``strides = [1, SH, SW, 1]`` and ``SAME``,
``VALID`` or explicit padding, and picks its kernel family from channel counts and bit widths alone, so a
1x3 window, a (2, 1) stride or a ``VALID`` 3x3 / 2 conv reaches every hand-written kernel. The rest of the
suite runs them with ``KH == KW`` and ``SH == SW``, nearly always ``SAME``: a kernel that reads ``KH``
for ``KW``, ``PT`` for ``PL``, or swaps ``SH`` / ``SW`` in a parity class would pass it. The list in
``conv_geometry_cases.ROWS`` differs in every such pair of fields.

CPU (unmarked): the oracle's conv triple against a direct loop nest on every row (so the oracle is a
sound reference off the square diagonal), the resolved geometry and the unread rows / columns against
literals, ``ops.conv_desc`` against ``oracle.nn.conv_geometry``, that the list discriminates, and the
dispatch of every (family, row) pair -- fallbacks included -- pinned.

GPU: ``Conv2d_q`` against ``oracle.nn.Conv2dQ`` per (family, row) by the method of
``test_bit_widths.test_conv_layer_across_widths`` -- X codes, y, gradient codes, dW, db, dX and the
exponent update, all bit-exact (the 20-bit float mode: ``test_wide_bits``' 1-ulp ``F32_RTOL``); the wide
families again with the 256-row GEMM forced onto them; the ``_ws`` and quantising entry points and the
fused bottleneck's ``fwd_codes`` / ``bwd_codes16`` against the exact integer result; the pools, whose
descriptor and index code are of the same class, on non-square windows.
"""
import numpy as np
import pytest
import torch

import conv_geometry_cases as G
from lbt_amd import dynamic_fixed_point as D
from lbt_amd._lib import NSHARD, OUT_I8
from lbt_amd.dfxp import ops
from lbt_amd.runtime import DfxpContext
from oracle import dfxp as odfxp
from oracle import nn as onn
from test_bit_widths import B_I, G_I, WD, X_I, _check_path, _ilog2_ceil, _not_vacuous, _same_codes, _spread, _x_codes
from test_igemm_big import VARIANTS
from test_wide_bits import _close

DEV = "cuda"
F32 = np.float32


# =============================================================================== CPU: the list
@pytest.mark.parametrize("row", G.ROW_IDS)
def test_oracle_conv_triple_matches_loop_nest(row):
    """oracle.nn.conv_fwd_int / conv_dgrad_int / conv_wgrad_int == a loop nest over (n, oh, ow, kh, kw)
    with the (ci, co) contraction in int64, bit for bit, on int8-range operands (N = 2, 3 -> 4)."""
    H, W, KH, KW, SH, SW, pad = G.ROWS[row]
    Ho, Wo = G.geometry(row)[:2]
    rng = np.random.default_rng(G.ROW_IDS.index(row))
    x = rng.integers(-128, 128, size=(G.N, H, W, 3))
    w = rng.integers(-128, 128, size=(KH, KW, 3, 4))
    g = rng.integers(-128, 128, size=(G.N, Ho, Wo, 4))
    y, dx, dw = G.conv_loops(x, w, g, row)
    assert np.count_nonzero(y) and np.count_nonzero(dx) and np.count_nonzero(dw)
    assert np.array_equal(onn.conv_fwd_int(x, w, (SH, SW), pad), y)
    assert np.array_equal(onn.conv_dgrad_int(g, w, (SH, SW), pad, x.shape), dx)
    assert np.array_equal(onn.conv_wgrad_int(x, g, (SH, SW), pad, (KH, KW)), dw)
    rows, cols = G.unread(row)
    assert not dx[:, rows].any() and not dx[:, :, cols].any()


def test_geometry_literals_and_conv_desc():
    """The resolved geometry of every row and the unread rows / columns of rows f, i and n are the
    literals of the table (a change to conv_desc / conv_geometry must not quietly empty those cases);
    ops.conv_desc == oracle.nn.conv_geometry, field by field."""
    assert len(G.ROWS) >= 14 and set("abcdefghijklmn") <= set(G.ROWS)
    for row in G.ROW_IDS:
        H, W, KH, KW, SH, SW, pad = G.ROWS[row]
        want = G.GEOMETRY[row]
        assert G.geometry(row) == want, row
        assert tuple(onn.conv_geometry(H, W, KH, KW, SH, SW, pad)) == want, row
        d = ops.conv_desc(G.N, H, W, 3, 4, KH, KW, SH, SW, pad)
        assert (d.Ho, d.Wo, d.PT, d.PB, d.PL, d.PR) == want, row
        assert (d.N, d.H, d.W, d.Cin, d.Cout, d.KH, d.KW, d.SH, d.SW) == (G.N, H, W, 3, 4, KH, KW, SH, SW), row
        assert G.unread(row) == G.UNREAD.get(row, ([], [])), row
    assert G.UNREAD["f"] == ([7], [])
    assert G.UNREAD["i"] == ([1, 2, 4, 5, 7], [1, 3, 5])
    assert G.UNREAD["n"] == ([3, 7, 8], [3, 7, 8])
    assert G.GEOMETRY["g"][2:] == (0, 1, 0, 0) and G.GEOMETRY["h"][2:] == (1, 1, 0, 1)
    assert G.GEOMETRY["j"][2:] == (1, 1, 0, 0) and G.GEOMETRY["l"][:2] == (8, 5)


def test_list_discriminates():
    """At least two rows each differ in H / W, KH / KW, SH / SW, PT / PL and PT / PB; a VALID and an
    explicit-padding row exist."""
    rows = [G.ROWS[r] + G.GEOMETRY[r] for r in G.ROW_IDS]  # H W KH KW SH SW pad Ho Wo pt pb pl pr
    assert sum(r[0] != r[1] for r in rows) >= 2
    assert sum(r[2] != r[3] for r in rows) >= 2
    assert sum(r[4] != r[5] for r in rows) >= 2
    assert sum(r[9] != r[11] for r in rows) >= 2
    assert sum(r[9] != r[10] for r in rows) >= 2
    assert sum(r[7] != r[8] for r in rows) >= 2  # Ho != Wo: the noise index of the quantising epilogues
    assert any(r[6] == "VALID" for r in rows) and any(isinstance(r[6], tuple) for r in rows)


def _layer(family, row, ctx, name="c", ranges=True):
    bits, gb, wb, Cin, Cout, nonneg, bias = G.FAMILIES[family]
    H, W, KH, KW, SH, SW, pad = G.ROWS[row]
    kw = dict(input_range=X_I, weight_range=_w_range(family, row), bias_range=B_I, grad_range=G_I) if ranges else {}
    return D.Conv2d_q(name, bits, [KH, KW, Cin, Cout], [1, SH, SW, 1], pad, use_bias=bias, weight_decay=WD,
                      input_nonnegative=nonneg, grad_bits=gb, weight_bits=wb, ctx=ctx, **kw)


def _w_range(family, row):
    KH, KW = G.ROWS[row][2:4]
    return _ilog2_ceil((3 / (KH * KW * G.FAMILIES[family][3])) ** 0.5)  # the weights fill their range


def _desc(family, row):
    H, W, KH, KW, SH, SW, pad = G.ROWS[row]
    return ops.conv_desc(G.N, H, W, G.FAMILIES[family][3], G.FAMILIES[family][4], KH, KW, SH, SW, pad)


def _check_dispatch(gl, family, row):
    _check_path(gl, G.PATHS[family])
    d = _desc(family, row)
    got = dict(stem=bool(gl.stem(d)), stem_wide=bool(gl.stem_wide(d)), wgrad3=bool(ops.wgrad3_ok(d)),
               wgrad1=ops.wgrad1_wci(d))
    assert got == G.shape_path(family, row), (family, row, got)


@pytest.mark.parametrize("family", G.FAMILY_IDS)
def test_dispatch_is_pinned(family):
    """CPU: the kernels every (family, row) pair of the GPU tests selects -- the layer attributes and the
    shape predicates stem / stem_wide / wgrad3_ok / wgrad1_wci, the contract's fallbacks written down
    in conv_geometry_cases (the GPU tests assert the same and never skip)."""
    ctx = DfxpContext(device="cpu", seed=0)
    for row in G.ROW_IDS:
        _check_dispatch(_layer(family, row, ctx, name=row, ranges=False), family, row)
    # every family meets each asymmetry on a kernel of its own: the rows a pair falls back on are not all
    # of any class
    own = [r for r in G.ROW_IDS if family == "stem_wide" or r not in G.STEM_WIDE_ROWS.get(family, ())]
    rows = [G.ROWS[r] + G.GEOMETRY[r] for r in own]
    assert any(r[0] != r[1] for r in rows) and any(r[2] != r[3] for r in rows) and any(r[4] != r[5] for r in rows)
    assert any(r[6] == "VALID" and any(G.unread(o)) for r, o in zip(rows, own))
    assert any(isinstance(r[6], tuple) for r in rows)


def test_workspace_sizes_of_the_split_rows():
    """lbt_igemm_workspace_bytes at 64 -> 64: the forward splits K on rows j (nk = 8, two splits) and k
    (nk = 15, three); the dgrad on row k only (strided dgrads run as parity classes and never split)."""
    for row, fwd, dgrad8, dgrad16 in [("j", 2 * 32 * 64 * 4, 0, 0), ("k", 3 * 12 * 64 * 4, 3 * 12 * 64 * 4,
                                                                     2 * 3 * 12 * 64 * 4)]:
        d = _desc("igemm16_64_64", row)
        assert ops.igemm_workspace_bytes(d, 0, False) == fwd, row
        assert ops.igemm_workspace_bytes(d, 1, False) == dgrad8, row
        assert ops.igemm_workspace_bytes(d, 1, True) == dgrad16, row


# =============================================================================== GPU: the layer
def _launches():
    return ops.igemm_tuning()["launches"]


def _inputs(family, row):
    bits, gb, wb, Cin, Cout, nonneg, bias = G.FAMILIES[family]
    H, W = G.ROWS[row][:2]
    Ho, Wo = G.GEOMETRY[row][:2]
    rng = np.random.default_rng([G.FAMILY_IDS.index(family), G.ROW_IDS.index(row)])
    return dict(x=_spread(rng, (G.N, H, W, Cin), X_I, nonneg), g=_spread(rng, (G.N, Ho, Wo, Cout), G_I),
                b=rng.uniform(-0.2, 0.2, size=Cout).astype(F32) if bias else None)


def _gpu_step(family, row, inp, forced=None):
    """One forward / backward / exponent update of the layer on a fresh context; everything the oracle is
    compared with, and the 256-row GEMM launches the forward and the backward made."""
    bits, gb, wb, Cin, Cout, nonneg, bias = G.FAMILIES[family]
    ctx = DfxpContext(seed=100 + bits)
    gl = _layer(family, row, ctx)
    _check_dispatch(gl, family, row)
    if bias:
        gl.b.copy_(torch.from_numpy(inp["b"]))
    out = dict(W=gl.W.cpu().numpy().copy(), ranges0=ctx.ranges(), seed=ctx.seed)

    def run():
        n0 = _launches()
        y = gl.forward(torch.from_numpy(inp["x"]).to(DEV))
        n1 = _launches()
        dx = gl.backward(torch.from_numpy(inp["g"]).to(DEV))
        torch.cuda.synchronize()
        return y, dx, n1 - n0, _launches() - n1

    if forced is None:
        y, dx, nf, nb = run()
    else:
        with ops.igemm_forced(big=1, min_tiles=1, **forced):
            y, dx, nf, nb = run()
    out.update(y=y.cpu().numpy(), dx=dx.cpu().numpy(), dW=gl.dW.cpu().numpy(), nf=nf, nb=nb,
               xq=_x_codes(gl.xq, gl.x_kind), x_kind=gl.x_kind, fmode=gl.fmode, gq=gl.gradq.cpu().numpy(),
               gq_dtype=gl.gradq.dtype, db=gl.db.cpu().numpy() if bias else None)
    ctx.update_range_op()
    out["ranges"] = ctx.ranges()
    return out


def _oracle_step(family, row, inp, gpu):
    bits, gb, wb, Cin, Cout, nonneg, bias = G.FAMILIES[family]
    H, W, KH, KW, SH, SW, pad = G.ROWS[row]
    ol = onn.Conv2dQ("c", bits, [KH, KW, Cin, Cout], [1, SH, SW, 1], pad, WD, grad_bits=gb, weight_bits=wb,
                     use_bias=bias)
    ol.W = gpu["W"].copy()
    ranges = {"c/W_range": _w_range(family, row), "c/X_range": X_I, "c/grad_range": G_I}
    if bias:
        ol.b = inp["b"].copy()
        ranges["c/b_range"] = B_I
    assert gpu["ranges0"] == ranges
    octx = onn.Ctx(dict(ranges), 0, gpu["seed"])
    y = ol.forward(inp["x"], octx)
    dx = ol.backward(inp["g"], octx)
    return ol, octx, y, dx


def _read_mask(row):
    H, W = G.ROWS[row][:2]
    rows, cols = G.unread(row)
    m = np.ones((H, W), bool)
    m[rows] = False
    m[:, cols] = False
    return m


def _compare(family, row, inp, gpu, ol, octx, yr, dxr, tag=""):
    bits, gb, wb, Cin, Cout, nonneg, bias = G.FAMILIES[family]
    exact = bits <= 16  # float mode is bit-exact up to 16 bits (fp32.hip); above: 1 ulp of a double-accumulated sum

    def check(a, b, what):
        if exact:
            assert np.array_equal(a, b), "%s %s %s%s" % (family, row, what, tag)
        else:
            _close(a, b, what="%s %s %s%s" % (family, row, what, tag))

    xrec, grec = octx.record["c/X_range"], octx.record["c/grad_range"]
    _not_vacuous(xrec, bits + 1, "X")
    c1, c2, _, _ = octx.counts["c/X_range"]
    assert c1 > 0 and c2 > c1, "both overflow counters of the X quantiser must count"
    assert len(np.unique(octx.record["c/W_range"])) >= 3
    _same_codes(gpu["xq"], gpu["x_kind"], xrec, bits + 1, X_I, "X codes" + tag)
    check(gpu["y"], yr, "y")
    _not_vacuous(grec, gb or bits, "gradient")
    _same_codes(gpu["gq"], gpu["x_kind"] if gpu["fmode"] else OUT_I8, grec, gb or bits, G_I, "gradient codes" + tag)
    assert gpu["gq_dtype"] == (torch.float32 if gpu["fmode"] else torch.int16 if (gb or bits) > 8 else torch.int8)
    check(gpu["dW"], ol.dW, "dW")
    assert not np.array_equal(ol.dW, (F32(2 * WD) * ol.W).astype(F32))
    if bias:
        check(gpu["db"], ol.db, "db")
    check(gpu["dx"], dxr, "dX")
    read = _read_mask(row)
    assert np.count_nonzero(dxr[:, read]) >= dxr[:, read].size // 4
    if row in G.UNREAD:  # pixels no output window reads: exactly 0.0, whatever class or tile owns them
        assert (~read).sum() > 0
        assert np.all(gpu["dx"][:, ~read] == 0.0) and np.all(dxr[:, ~read] == 0.0), "unread dX" + tag
    new = octx.new_ranges()
    assert gpu["ranges"] == new, tag
    assert new["c/X_range"] == min(X_I + 1, bits)  # the overflow moved it (clamped at bits + 1 - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("row", G.ROW_IDS)
@pytest.mark.parametrize("family", G.FAMILY_IDS)
def test_conv_layer_matches_oracle(family, row):
    """Conv2d_q == oracle.nn.Conv2dQ on every (family, row) pair: X codes, y, gradient codes, dW, db, dX,
    the exponent update; dX exactly 0.0 where no window reads (rows f, i, n). A third of the operands lie
    beyond the range and at least a quarter of the codes are non-zero."""
    inp = _inputs(family, row)
    gpu = _gpu_step(family, row, inp)
    assert (gpu["nf"], gpu["nb"]) == (0, 0), "the default selection keeps these sizes off the 256-row kernel"
    _compare(family, row, inp, gpu, *_oracle_step(family, row, inp, gpu))


# (family, row, halo): every pair of the wide families, row a with the halo path off and on
FORCED = [(f, r, h) for f in G.IGEMM_FAMILIES for r in G.ROW_IDS for h in ((0, 3) if r == "a" else (None,))]


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(FORCED)), ids=["%s-%s%s" % (f, r, "" if h is None else "-halo%d" % h)
                                                       for f, r, h in FORCED])
def test_wide_layer_with_256_row_kernel_forced(i):
    """The wide families again under igemm_forced(big=1, min_tiles=1) with one (stages, max_bn) pair per
    case, rotating through test_igemm_big.VARIANTS: the forward runs on the 256-row kernel wherever it is
    an implicit GEMM, the dgrad on unit-stride rows only (strided ones stay parity classes on the
    128-row kernel); results identical to the unforced run and to the oracle."""
    family, row, halo = FORCED[i]
    stages, max_bn = VARIANTS[i % len(VARIANTS)]
    inp = _inputs(family, row)
    plain = _gpu_step(family, row, inp)
    forced = _gpu_step(family, row, inp, dict(stages=stages, max_bn=max_bn, **({} if halo is None else {"halo": halo})))
    assert (plain["nf"], plain["nb"]) == (0, 0)
    assert forced["nf"] == int(G.fwd_on_igemm(family, row)), "forward launches of the 256-row kernel"
    assert forced["nb"] == int(row in G.UNIT_STRIDE), "dgrad launches of the 256-row kernel"
    for k in ("xq", "y", "gq", "dW", "dx"):
        assert np.array_equal(plain[k], forced[k]), (k, stages, max_bn, halo)
    assert plain["ranges"] == forced["ranges"]
    _compare(family, row, inp, forced, *_oracle_step(family, row, inp, forced),
             tag=" (forced %d, %d)" % (stages, max_bn))


def test_forced_cases_use_every_variant():
    used = {VARIANTS[i % len(VARIANTS)] for i, (f, r, h) in enumerate(FORCED) if r in G.UNIT_STRIDE}
    assert used == set(VARIANTS)
    assert {r for f, r, h in FORCED if r in G.UNIT_STRIDE} == set("abckl")


# =============================================================================== GPU: entry points
XB, XI, WB, WI, GI = 9, 2, 8, 0, -3  # quantisers of the direct calls (as test_igemm_big._setup)


def _direct(row, Cin, Cout, seed, gbits=16):
    """Quantisers, descriptor, weight codes and their packed images for a direct call on `row`."""
    H, W, KH, KW, SH, SW, pad = G.ROWS[row]
    rng = np.random.default_rng(seed)
    ctx = DfxpContext(seed=seed)
    qx, qw, qg = ctx.quantizer("t/X", XB, XI), ctx.quantizer("t/W", WB, WI), ctx.quantizer("t/g", gbits, GI)
    d = ops.conv_desc(G.N, H, W, Cin, Cout, KH, KW, SH, SW, pad)
    Wt = torch.from_numpy(rng.uniform(-1, 1, size=(KH, KW, Cin, Cout)).astype(F32)).to(DEV)
    w_hwio = torch.empty((KH, KW, Cin, Cout), dtype=torch.int8, device=DEV)
    ksf, ksd = ops.packed_slices(KH, KW, Cin), ops.packed_slices(KH, KW, Cout)
    wf = torch.zeros((Cout, ksf * 16), dtype=torch.int8, device=DEV)
    wd = torch.zeros((Cin, ksd * 16), dtype=torch.int8, device=DEV)
    ops.quantize_weight(Wt, qw, w_hwio=w_hwio, wf=wf, ksf=ksf, wd=wd, ksd=ksd)
    wq = w_hwio.cpu().numpy().astype(np.int64)
    assert len(np.unique(wq)) > 100
    return rng, ctx, (qx, qw, qg), d, wq, (wf, ksf), (wd, ksd)


def _x_operand(rng, shape, a_kind):
    """(true codes int64, the operand the kernel reads) for a_kind 0 (int8), 1 (offset int8), 2 (int16)."""
    if a_kind == 2:
        x = rng.integers(-256, 256, size=shape)
        return x, torch.from_numpy(x.astype(np.int16)).to(DEV)
    if a_kind == 1:
        x = rng.integers(0, 256, size=shape)
        return x, torch.from_numpy((x - 128).astype(np.int8)).to(DEV)
    x = rng.integers(-128, 128, size=shape)
    return x, torch.from_numpy(x.astype(np.int8)).to(DEV)


def _ws(nbytes):
    return torch.empty(nbytes // 4, dtype=torch.int32, device=DEV) if nbytes else None


@pytest.mark.gpu
@pytest.mark.parametrize("a_kind", [0, 1, 2])
@pytest.mark.parametrize("row", ["j", "k"])
def test_fwd_igemm_ws_splits_k_exactly(row, a_kind):
    """lbt_conv_fwd_igemm_ws at 64 -> 64 on the rows whose forward splits K (4x2: two splits of four
    k-blocks; 3x5: three of five) == the exact integer conv scaled once."""
    H, W, KH, KW, SH, SW, pad = G.ROWS[row]
    rng, ctx, (qx, qw, _), d, wq, (wf, ksf), _ = _direct(row, 64, 64, 10 * a_kind + ord(row))
    nbytes = ops.igemm_workspace_bytes(d, 0, a_kind == 2)
    assert nbytes > 0
    x, xop = _x_operand(rng, (G.N, H, W, 64), a_kind)
    y = torch.full((G.N, d.Ho, d.Wo, 64), float("nan"), device=DEV)
    ops.conv_fwd_igemm_ws(xop, a_kind, wf, ksf, d, qx.desc, qw.desc, y, _ws(nbytes))
    e = odfxp.frac_bits(XB, XI) + odfxp.frac_bits(WB, WI)
    assert np.array_equal(y.cpu().numpy(), onn.scale_int(onn.conv_fwd_int(x, wq, (SH, SW), pad), e))


@pytest.mark.gpu
@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("g_i16", [0, 1])
@pytest.mark.parametrize("row", ["j", "k"])
def test_dgrad_igemm_ws_matches_integer_dgrad(row, g_i16, add):
    """lbt_conv_dgrad_igemm_ws at 64 -> 64: row k splits K (workspace > 0), row j is strided (parity
    classes, no workspace); 8- and 16-bit gradient codes, with and without add_src; dx pre-filled with NaN
    (a pixel no class writes is caught)."""
    H, W, KH, KW, SH, SW, pad = G.ROWS[row]
    gbits = 16 if g_i16 else 8
    rng, ctx, (_, qw, qg), d, wq, _, (wd, ksd) = _direct(row, 64, 64, 20 * g_i16 + ord(row) + int(add), gbits)
    nbytes = ops.igemm_workspace_bytes(d, 1, g_i16)
    assert (nbytes > 0) == (row == "k")
    lim = 32768 if g_i16 else 128
    g = rng.integers(-lim, lim, size=(G.N, d.Ho, d.Wo, 64))
    gop = torch.from_numpy(g.astype(np.int16 if g_i16 else np.int8)).to(DEV)
    addend = rng.normal(size=(G.N, H, W, 64)).astype(F32) if add else None
    dx = torch.full((G.N, H, W, 64), float("nan"), device=DEV)
    ops.conv_dgrad_igemm_ws(gop, g_i16, wd, ksd, d, qg.desc, qw.desc, dx, _ws(nbytes),
                            add_src=torch.from_numpy(addend).to(DEV) if add else None)
    e = odfxp.frac_bits(gbits, GI) + odfxp.frac_bits(WB, WI)
    ref = onn.scale_int(onn.conv_dgrad_int(g, wq, (SH, SW), pad, (G.N, H, W, 64)), e)
    if add:
        ref = (ref + addend).astype(F32)
    assert np.array_equal(dx.cpu().numpy(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("stochastic", [True, False])
@pytest.mark.parametrize("row", ["a", "d"])
def test_quantising_epilogue_where_ho_differs_from_wo(row, stochastic):
    """lbt_conv_fwd_igemm_q at 64 -> 128 on rows a (6 x 10 outputs) and d (4 x 10, stride (2, 1)): the noise
    index of its epilogue is (row % (Ho*Wo)) * Cout + col, so a kernel that decomposes rows with the wrong
    extent draws other noise. == lbt_conv_fwd_igemm (itself == the exact integer conv) followed by
    lbt_dfxp_quantize: codes, both overflow counters, exact channel sums -- on the 256-row kernel's
    row-major epilogue (every ring depth, halo off and on), its sample-blocked forms (fwdq_perm 1, 2, 8),
    and the 128-row kernel (big = 0)."""
    H, W, KH, KW, SH, SW, pad = G.ROWS[row]
    Cin, Cout = 64, 128
    for a_kind in (0, 1):
        rng, ctx, (qx, qw, _), d, wq, (wf, ksf), _ = _direct(row, Cin, Cout, 2 * ord(row) + a_kind + 7 * stochastic)
        assert d.Ho != d.Wo
        x, xop = _x_operand(rng, (G.N, H, W, Cin), a_kind)
        y = torch.empty((G.N, d.Ho, d.Wo, Cout), device=DEV)
        ops.conv_fwd_igemm(xop, a_kind, wf, ksf, d, qx.desc, qw.desc, y)
        e = odfxp.frac_bits(XB, XI) + odfxp.frac_bits(WB, WI)
        yr = onn.scale_int(onn.conv_fwd_int(x, wq, (SH, SW), pad), e)
        assert np.array_equal(y.cpu().numpy(), yr)
        # a range that puts a few percent of the outputs past the clip (both counters non-zero)
        qo = ctx.quantizer("t/bnX", 8, int(np.ceil(np.log2(np.abs(yr).max()))) - 2, stochastic=stochastic)
        cs_ref = torch.zeros(NSHARD * 2 * Cout, dtype=torch.int64, device=DEV)
        ctx.counts.zero_()
        q_ref = ops.quantize(y, qo, OUT_I8, chsum=cs_ref, C=Cout)
        cnt_ref = ctx.counts_view()[qo.slot].sum(0).cpu()
        assert cnt_ref[0] > 0 and cnt_ref[1] > cnt_ref[0]
        cases = [(1, v, h, 0) for v in VARIANTS[:-1:2] for h in (0, 3)]
        cases += [(1, (2, 64), 0, 1), (1, (2, 128), 0, 2), (1, (3, 64), 0, 8), (1, (4, 128), 0, 8), (0, (2, 128), 0, 2)]
        for big, (stages, max_bn), halo, perm in cases:
            ctx.counts.zero_()
            cs = torch.zeros_like(cs_ref)
            yq = torch.full(q_ref.shape, 99, dtype=torch.int8, device=DEV)
            n0 = _launches()
            with ops.igemm_forced(big=big, min_tiles=1, stages=stages, max_bn=max_bn, halo=halo, fwdq_perm=perm):
                ops.conv_fwd_igemm_q(xop, a_kind, wf, ksf, d, qx.desc, qw.desc, yq, qo, cs)
            what = (a_kind, big, stages, max_bn, halo, perm)
            assert _launches() == n0 + big, what
            assert torch.equal(yq, q_ref), what
            assert torch.equal(ctx.counts_view()[qo.slot].sum(0).cpu(), cnt_ref), what
            assert torch.equal(cs.view(NSHARD, -1).sum(0), cs_ref.view(NSHARD, -1).sum(0)), what


@pytest.mark.gpu
@pytest.mark.parametrize("add", [False, True])
def test_fused_block_conv_calls_on_row_k(add):
    """Conv2d_q.fwd_codes / bwd_codes16 (the fused bottleneck's conv calls: the _ws entry points with the
    layer's own workspace, the storing wide wgrad) at 64 -> 64 on the 3x5 window over a 2 x 3 map, from
    codes the caller quantised: y, dW and dX (+ add_src) == the exact integer results scaled once."""
    H, W, KH, KW, SH, SW, pad = G.ROWS["k"]
    rng = np.random.default_rng(50 + add)
    ctx = DfxpContext(seed=5)
    gl = _layer("igemm16_64_64", "k", ctx)
    d = _desc("igemm16_64_64", "k")
    assert gl._ws(d, 0, False) is not None and gl._ws(d, 1, True) is not None
    x, xop = _x_operand(rng, (G.N, H, W, 64), 1)
    y = gl.fwd_codes(xop, G.N, H, W)
    wq = gl.w_hwio.cpu().numpy().astype(np.int64)
    ex, ew, eg = odfxp.frac_bits(9, X_I), odfxp.frac_bits(8, _w_range("igemm16_64_64", "k")), odfxp.frac_bits(16, G_I)
    assert np.array_equal(y.cpu().numpy(), onn.scale_int(onn.conv_fwd_int(x, wq, (SH, SW), pad), ex + ew))
    g = rng.integers(-32768, 32768, size=(G.N, d.Ho, d.Wo, 64))
    addend = rng.normal(size=(G.N, H, W, 64)).astype(F32) if add else None
    dx = gl.bwd_codes16(torch.from_numpy(g.astype(np.int16)).to(DEV),
                        add_src=torch.from_numpy(addend).to(DEV) if add else None)
    torch.cuda.synchronize()
    ref = onn.scale_int(onn.conv_dgrad_int(g, wq, (SH, SW), pad, (G.N, H, W, 64)), eg + ew)
    if add:
        ref = (ref + addend).astype(F32)
    assert np.array_equal(dx.cpu().numpy(), ref)
    Wf = gl.W.cpu().numpy()
    dw = onn.scale_int(onn.conv_wgrad_int(x, g, (SH, SW), pad, (KH, KW)), ex + eg)
    assert np.array_equal(gl.dW.cpu().numpy(), (dw + (F32(2 * WD) * Wf).astype(F32)).astype(F32))


# =============================================================================== GPU: the pools
# (H, W, KH, KW, SH, SW, padding): rows d, g, m and a 3x2 window with stride (2, 3) on a 7 x 6 map
POOLS = {"d": G.ROWS["d"], "g": G.ROWS["g"], "m": G.ROWS["m"], "w3x2": (7, 6, 3, 2, 2, 3, "SAME")}


def _pool_input(rng, shape):
    x = rng.standard_normal(shape).astype(F32) - F32(0.3)
    x[:, : shape[1] // 3] = -np.abs(x[:, : shape[1] // 3])  # whole windows with max <= 0
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("C", [6, 8])
@pytest.mark.parametrize("case", sorted(POOLS))
def test_maxpool_non_square_windows(case, C):
    """MaxPool_q (C = 6: the scalar kernels, C = 8: the 4-wide ones) == oracle.nn.MaxPoolQ forward and
    backward, bit for bit; at C = 8 also lbt_maxpool_relu_fwd / _bwd, with and without y, ==
    relu_bwd(maxpool_bwd(g)) of the oracle on relu(x)."""
    H, W, KH, KW, SH, SW, pad = POOLS[case]
    rng = np.random.default_rng([C, sorted(POOLS).index(case)])
    x = _pool_input(rng, (G.N, H, W, C))
    layer = D.MaxPool_q([1, KH, KW, 1], [1, SH, SW, 1], pad)
    ref = onn.MaxPoolQ([1, KH, KW, 1], [1, SH, SW, 1], pad)
    yr = ref.forward(x, None)
    assert np.array_equal(layer.forward(torch.from_numpy(x).to(DEV)).cpu().numpy(), yr)
    g = rng.standard_normal(yr.shape).astype(F32)
    assert np.array_equal(layer.backward(torch.from_numpy(g).to(DEV)).cpu().numpy(), ref.backward(g, None))
    if C % 4:
        return
    d = ops.conv_desc(G.N, H, W, C, C, KH, KW, SH, SW, pad)
    xr = np.maximum(x, 0)
    yrr = ref.forward(xr, None)
    want = (ref.backward(g, None) * (x > 0)).astype(F32)
    xt, gt = torch.from_numpy(x).to(DEV), torch.from_numpy(g).to(DEV)
    y = torch.full(yr.shape, float("nan"), device=DEV)
    amax = torch.empty(yr.shape, dtype=torch.uint8, device=DEV)
    ops.maxpool_relu_fwd(xt, y, amax, d)
    assert np.array_equal(y.cpu().numpy(), yrr)
    empty = int((amax == 255).sum())  # windows the ReLU empties route nothing
    assert empty == int((yrr == 0).sum()) and (empty > 0 or case == "m")  # m: every 5x3 window reaches x > 0
    for with_y in (True, False):
        dx = torch.full(x.shape, float("nan"), device=DEV)
        ops.maxpool_relu_bwd(gt, amax, y if with_y else None, dx, d)
        assert np.array_equal(dx.cpu().numpy(), want), with_y
    # the unfused forward on the ReLU's output, the ReLU's backward folded into the pool's
    y2 = torch.empty_like(y)
    amax2 = torch.empty_like(amax)
    ops.maxpool_fwd(torch.from_numpy(xr).to(DEV), y2, amax2, d)
    assert np.array_equal(y2.cpu().numpy(), yrr)
    dx = torch.full(x.shape, float("nan"), device=DEV)
    ops.maxpool_relu_bwd(gt, amax2, y2, dx, d)
    assert np.array_equal(dx.cpu().numpy(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [6, 8])
@pytest.mark.parametrize("case", sorted(POOLS))
def test_avgpool_non_square_windows(case, C):
    """AvgPool_q == oracle.nn.AvgPoolQ forward and backward, bit for bit (sum / count of valid positions;
    the covering-window bounds of the backward divide by SH and SW separately)."""
    H, W, KH, KW, SH, SW, pad = POOLS[case]
    rng = np.random.default_rng([C, sorted(POOLS).index(case), 1])
    x = rng.standard_normal((G.N, H, W, C)).astype(F32)
    layer = D.AvgPool_q([1, KH, KW, 1], [1, SH, SW, 1], pad)
    ref = onn.AvgPoolQ([1, KH, KW, 1], [1, SH, SW, 1], pad)
    yr = ref.forward(x, None)
    assert np.array_equal(layer.forward(torch.from_numpy(x).to(DEV)).cpu().numpy(), yr)
    g = rng.standard_normal(yr.shape).astype(F32)
    assert np.array_equal(layer.backward(torch.from_numpy(g).to(DEV)).cpu().numpy(), ref.backward(g, None))

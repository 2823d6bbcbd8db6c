"""Operands that land on the DFXP quantiser's decision points (test helper, like plain_oracle.py).

A random float essentially never lands where two implementations of the quantiser's last steps can
differ: an exact rounding tie, ``fl(x*m + u)`` crossing an integer, the clip limits ``-L`` / ``L-1``
and the four counter thresholds ``+-L`` / ``+-L/2`` (``>=`` above, ``<`` below: oracle/dfxp.py
``overflow_counts``). This module builds fp32 operands ``[rows, inner]`` that sit exactly there, from
the oracle's own noise (``oracle.dfxp.noise_for`` is broadcast over dim 0: every row of a column shares
its ``u``), together with what the oracle says about them.

Site classes (each a function returning ``x`` fp32 ``[rows, inner]``):

* ``rounding_sites``   per column an integer k; x0 = fl((k - u)/m) (stochastic) or (k + 0.5)/m (nearest,
                       exact); the rows are x0 stepped by -span .. +span ulps (7 rows at span 3).
* ``threshold_sites``  one threshold class per row (+L, -L, +L/2, -L/2), columns cycle -1 / 0 / +1 ulp.
* ``clip_sites``       (L-1-u)/m, (L-u)/m, (-L-u)/m, (-L-1)/m at -1 / 0 / +1 ulp (rows), plus a row of
                       stochastic sites where fl(xm + u) rounds UP to exactly L although xm + u < L.
* ``special_sites``    +-0, +-inf, +-FLT_MAX, +-2^-126, +-2^-149, and -2^-149 on the smallest-u column.
* ``saturation_sites`` every element beyond +-4L/m, signs alternating.
* ``integer_grid``     the accumulator values for entry points whose operand is an integer times 2^-s.

NaN is out of scope: no integer code exists for it (the reference's cast of NaN is undefined), so no
site holds one.

The U8OFF rule, stated once: an offset-uint8 output stores ``max(code, 0)`` (``u8off``).
"""
import functools

import numpy as np

from oracle import dfxp as odfxp

SPAN = 3  # ulps either side of a rounding site: 2*SPAN + 1 = 7 rows

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def qparams(bits, I):
    """(e, m, L) of a quantiser: m = 2^e, L = 2^(bits-1), as float64 (all exact)."""
    e = odfxp.frac_bits(bits, I)
    return e, 2.0 ** e, 2.0 ** (bits - 1)


@functools.lru_cache(maxsize=64)
def _noise(inner, seed, qid, step):
    u = odfxp.noise_for((1, inner), qid, step, seed).astype(F32)
    u.setflags(write=False)
    return u


def noise(inner, stochastic, seed, qid, step):
    """The oracle's noise of a [rows, inner] operand (None for the nearest quantiser); cached, read-only."""
    return _noise(int(inner), int(seed), int(qid), int(step)) if stochastic else None


def ulp_step(x, n):
    """x stepped by n ulps (np.nextafter |n| times, towards +inf for n > 0)."""
    x = np.asarray(x, dtype=F32).copy()
    to = F32(np.inf) if n > 0 else F32(-np.inf)
    for _ in range(abs(int(n))):
        x = np.nextafter(x, to).astype(F32)
    return x


def _spread(lo, hi, inner):
    """inner integers from [lo, hi]: every one (tiled) when they fit, else spread evenly with the three
    lowest and the three highest always present."""
    count = hi - lo + 1
    if count <= inner:
        return (lo + np.arange(inner) % count).astype(np.int64)
    mid = np.rint(np.linspace(lo + 3, hi - 3, inner - 6)).astype(np.int64)
    return np.concatenate([np.arange(lo, lo + 3), mid, np.arange(hi - 2, hi + 1)]).astype(np.int64)


def rounding_ks(bits, stochastic, inner):
    L = 1 << (bits - 1)
    return _spread(-L + 1, L - 1, inner) if stochastic else _spread(-L, L - 2, inner)


def rounding_sites(bits, I, stochastic, inner, seed=0, qid=0, step=0, span=SPAN):
    """x [2*span+1, inner] and the k of each column."""
    _, m, _ = qparams(bits, I)
    ks = rounding_ks(bits, stochastic, inner)
    if stochastic:
        u = noise(inner, True, seed, qid, step).astype(np.float64)
        x0 = ((ks - u) / m).astype(F32)  # k - u is exact in float64; one rounding, to fp32
    else:
        x0 = ((ks + 0.5) / m).astype(F32)  # exact
        assert np.array_equal(x0.astype(np.float64) * m, ks + 0.5)
    return np.stack([ulp_step(x0, d) for d in range(-span, span + 1)]), ks


THRESHOLD_CLASSES = ("+L", "-L", "+L/2", "-L/2")


def threshold_sites(bits, I, inner):
    """x [4, inner]: row r holds class THRESHOLD_CLASSES[r] at -1, 0, +1 ulp (column % 3)."""
    _, m, L = qparams(bits, I)
    rows = []
    for t in (L, -L, L / 2, -L / 2):
        base = F32(t / m)
        three = np.array([ulp_step(base, d) for d in (-1, 0, 1)], dtype=F32)
        rows.append(three[np.arange(inner) % 3])
    return np.stack(rows)


def find_round_up_to_L(bits, I, u):
    """Per column: an fp32 x with x*m + u < L exactly but fl32(x*m + u) == L, or NaN where the column's u
    admits none (searched over the floats next to (L - u)/m)."""
    _, m, L = qparams(bits, I)
    u64 = np.asarray(u, dtype=np.float64)
    out = np.full(u64.shape, np.nan, dtype=F32)
    x0 = ((L - u64) / m).astype(F32)
    for d in range(-3, 4):
        x = ulp_step(x0, d)
        xm = (x * F32(m)).astype(F32)
        exact = xm.astype(np.float64) + u64  # exact: both addends have 24-bit significands within 2^40
        hit = (exact < L) & ((xm + np.asarray(u, dtype=F32)).astype(F32) == F32(L)) & np.isnan(out)
        out[hit] = x[hit]
    return out


def clip_sites(bits, I, stochastic, inner, seed=0, qid=0, step=0):
    """x [4, inner]: rows 0..2 = the four clip operands (column % 4) at -1, 0, +1 ulp; row 3 = the
    round-up-to-L site of every column that has one (stochastic), else row 1 again."""
    _, m, L = qparams(bits, I)
    u = noise(inner, stochastic, seed, qid, step)
    u64 = np.zeros(inner) if u is None else u.astype(np.float64)
    ops = np.stack([(L - 1 - u64) / m, (L - u64) / m, (-L - u64) / m, (-L - 1 + 0 * u64) / m]).astype(F32)
    base = ops[np.arange(inner) % 4, np.arange(inner)]
    rows = [ulp_step(base, d) for d in (-1, 0, 1)]
    last = rows[1].copy()
    if stochastic:
        up = find_round_up_to_L(bits, I, u)
        last = np.where(np.isnan(up), last, up).astype(F32)
    return np.stack(rows + [last])


SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, FLT_MAX, -FLT_MAX, 2.0 ** -126, -2.0 ** -126,
                     2.0 ** -149, -2.0 ** -149], dtype=F32)


def special_sites(bits, I, stochastic, inner, seed=0, qid=0, step=0):
    """x [1, inner]: SPECIALS tiled over the columns, -2^-149 on the column whose u is smallest."""
    x = SPECIALS[np.arange(inner) % len(SPECIALS)].copy()
    u = noise(inner, stochastic, seed, qid, step)
    x[int(np.argmin(u)) if u is not None else 0] = F32(-2.0 ** -149)
    return x.reshape(1, inner)


def saturation_sites(bits, I, rows, inner):
    """x [rows, inner]: |x*m| in {4, 5, 8, 1000} L, sign alternating along both axes."""
    _, m, L = qparams(bits, I)
    r, c = np.indices((rows, inner))
    mag = np.array([4.0, 5.0, 8.0, 1000.0])[(r + c // 2) % 4] * L / m
    return (np.where((r + c) % 2 == 0, mag, -mag)).astype(F32)


def integer_grid(bits, int8_operand=True):
    """Accumulator values for the integer-grid entry points: every integer in [-2L-2, 2L+2], or the
    whole int8 range where that is smaller."""
    L = 1 << (bits - 1)
    lo, hi = -2 * L - 2, 2 * L + 2
    if int8_operand:
        lo, hi = max(lo, -128), min(hi, 127)
    return np.arange(lo, hi + 1, dtype=np.int64)


ALL_CLASSES = ("rounding", "threshold", "clip", "special", "saturation")


def sites(cls, bits, I, stochastic, inner, seed=0, qid=0, step=0, rows=2 * SPAN + 1):
    """The operands of one site class (cached per argument tuple; the array is read-only)."""
    x = _sites(cls, int(bits), int(I), bool(stochastic), int(inner), int(seed), int(qid), int(step), int(rows))
    return x


@functools.lru_cache(maxsize=256)
def _sites(cls, bits, I, stochastic, inner, seed, qid, step, rows):
    x = _build_sites(cls, bits, I, stochastic, inner, seed, qid, step, rows)
    x.setflags(write=False)
    return x


def _build_sites(cls, bits, I, stochastic, inner, seed, qid, step, rows):
    if cls == "rounding":
        return rounding_sites(bits, I, stochastic, inner, seed, qid, step)[0]
    if cls == "threshold":
        return threshold_sites(bits, I, inner)
    if cls == "clip":
        return clip_sites(bits, I, stochastic, inner, seed, qid, step)
    if cls == "special":
        return special_sites(bits, I, stochastic, inner, seed, qid, step)
    if cls == "saturation":
        return saturation_sites(bits, I, rows, inner)
    raise ValueError(cls)


# ------------------------------------------------------------------------------ what the oracle says
def oracle_codes(x, bits, I, stochastic, u):
    with np.errstate(over="ignore", invalid="ignore"):
        return odfxp.quantize_int(x, bits, I, stochastic, u)


def oracle_counts(x, bits, I):
    with np.errstate(over="ignore"):
        return odfxp.overflow_counts(x, bits, I)


def oracle_row_counts(x, bits, I):
    """[(c1, c2)] per row of x."""
    return [oracle_counts(r, bits, I) for r in np.asarray(x, dtype=F32)]


def oracle_element_flags(x, bits, I):
    """overflow_counts per element: two 0/1/.. int arrays of x's shape (few distinct values: cached)."""
    x = np.asarray(x, dtype=F32)
    vals, inv = np.unique(x.view(np.uint32), return_inverse=True)
    per = np.array([oracle_counts(v.view(F32), bits, I) for v in vals], dtype=np.int64)
    return per[inv.reshape(-1), 0].reshape(x.shape), per[inv.reshape(-1), 1].reshape(x.shape)


def u8off(codes):
    """The U8OFF rule: an offset-uint8 output stores max(code, 0)."""
    return np.maximum(np.asarray(codes), 0)


# ------------------------------------------------------------------------------ wrong quantisers (teeth)
def _xm(x, bits, I):
    _, m, L = qparams(bits, I)
    with np.errstate(over="ignore"):
        return (np.asarray(x, dtype=F32) * F32(m)).astype(F32), F32(L)


def _codes(xm, L, stochastic, u, hi=None, exact_add=False, half_away=False):
    hi = L - F32(1) if hi is None else hi
    with np.errstate(over="ignore", invalid="ignore"):
        if stochastic:
            v = xm.astype(np.float64) + np.asarray(u, dtype=np.float64) if exact_add \
                else (xm + np.asarray(u, dtype=F32)).astype(F32)
            return np.floor(np.clip(v, -L, hi)).astype(np.int32)
        c = np.clip(xm, -L, hi)
        if half_away:
            return (np.sign(c) * np.floor(np.abs(c.astype(np.float64)) + 0.5)).astype(np.int32)
        return np.rint(c).astype(np.int32)


def _counts(xm, L, symmetric=False):
    if symmetric:
        a = np.abs(xm)
        return int(np.count_nonzero(a >= L)), int(np.count_nonzero(a >= L / F32(2)))
    return (int(np.count_nonzero(xm >= L) + np.count_nonzero(xm < -L)),
            int(np.count_nonzero(xm >= L / F32(2)) + np.count_nonzero(xm < -(L / F32(2)))))


def right_quantiser(x, bits, I, stochastic, u):
    """The oracle restated in this module's terms (checked equal to it by the CPU tests)."""
    xm, L = _xm(x, bits, I)
    return _codes(xm, L, stochastic, u), _counts(xm, L)


def wrong_half_away(x, bits, I, stochastic, u):
    xm, L = _xm(x, bits, I)
    return _codes(xm, L, stochastic, u, half_away=True), _counts(xm, L)


def wrong_symmetric_counts(x, bits, I, stochastic, u):
    xm, L = _xm(x, bits, I)
    return _codes(xm, L, stochastic, u), _counts(xm, L, symmetric=True)


def wrong_exact_add(x, bits, I, stochastic, u):
    xm, L = _xm(x, bits, I)
    return _codes(xm, L, stochastic, u, exact_add=True), _counts(xm, L)


def wrong_clip_to_L(x, bits, I, stochastic, u):
    xm, L = _xm(x, bits, I)
    return _codes(xm, L, stochastic, u, hi=L), _counts(xm, L)


WRONG = {"half_away": wrong_half_away, "symmetric_counts": wrong_symmetric_counts,
         "exact_add": wrong_exact_add, "clip_to_L": wrong_clip_to_L}

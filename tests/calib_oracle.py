"""Range calibration restated in numpy (test helper; include/lbt_dfxp.h "Range calibration").

``table(x)`` and ``pick(table, n, bits, t)`` are written from the definition alone: per element the largest
range it overflows at is read from its bit pattern, c1(I) counts the elements that overflow at I, and the
calibrated range is the lowest I of the controller's interval whose rate float32(c1) / float32(n) is within the
target. ``CalibCtx`` is ``oracle.nn.Ctx`` with that pick in front of every quantiser: substituted for
``onn.Ctx`` around a forward + backward it is the calibration pass of the numpy model.
"""
import numpy as np

from oracle import dfxp
from oracle import nn as onn

I_MIN, I_MAX = -30, 30
BINS = I_MAX - I_MIN + 1  # 61


def tops(x):
    """(top, counted): per element the largest I with x >= 2^I or x < -2^I, and whether there is one at all
    (+-0, denormals and NaN overflow nowhere; +-inf everywhere: top = 128)."""
    u = np.ascontiguousarray(np.asarray(x, np.float32)).reshape(-1).view(np.uint32)
    e = ((u >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64)
    man = u & np.uint32(0x7FFFFF)
    neg = (u >> np.uint32(31)).astype(bool)
    top = e - 127 - (neg & (man == 0)).astype(np.int64)  # x < -2^I is strict: a negative power of two sits one lower
    counted = (e != 0) & ~((e == 255) & (man != 0))
    return top, counted


def table(x):
    """int64 [61]: entry I + 30 = c1(I) = #{x >= 2^I} + #{x < -2^I}."""
    top, counted = tops(x)
    top = top[counted]
    return np.array([np.count_nonzero(top >= I) for I in range(I_MIN, I_MAX + 1)], dtype=np.int64)


def hist(x):
    """int64 [61], what lbt_dfxp_range_scan adds: entry I + 30 = the elements whose largest overflowing range
    is I (the last entry: 30 or above). table(x) is its sum from each entry up."""
    top, counted = tops(x)
    top = np.minimum(top[counted], I_MAX)
    return np.array([np.count_nonzero(top == I) for I in range(I_MIN, I_MAX + 1)], dtype=np.int64)


def pick(tab, n, bits, t):
    """(I*, kept): the calibrated range, or (None, True) when nothing reaches the lowest range."""
    lo, hi = bits - 31, bits - 1
    if tab[lo - I_MIN] == 0:
        return None, True
    for I in range(lo, hi + 1):
        if np.float32(tab[I - I_MIN]) / np.float32(n) <= np.float32(t):
            return I, False
    return hi, False


class CalibCtx(onn.Ctx):
    """oracle.nn.Ctx whose ``q`` first sets the quantiser's range from the tensor it is about to quantise."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.set, self.kept = {}, []

    def q(self, name, x, bits, stochastic=True):
        x = np.asarray(x, dtype=np.float32)
        if name in self.set or name in self.kept:
            raise RuntimeError("quantiser %r fed twice" % name)
        I, kept = pick(table(x), x.size, bits, self.target)
        if kept:
            self.kept.append(name)
        else:
            self.I[name] = I
            self.set[name] = I
        return super().q(name, x, bits, stochastic)


def calibrate(run, monkeypatch):
    """Run ``run()`` (a forward + backward that builds its context as ``onn.Ctx(...)`` and returns it, alone
    or last in a tuple) with CalibCtx in its place; returns what run returned."""
    with monkeypatch.context() as m:
        m.setattr(onn, "Ctx", CalibCtx)
        return run()


def iterate(x, t, bits, I, limit=80):
    """The controller on one tensor from range I until it stops moving."""
    for _ in range(limit):
        J = dfxp.update_range(x, t, bits, I)
        if J == I:
            return I
        I = J
    raise AssertionError("update_range did not settle")

"""Range calibration on the numpy oracle (no GPU): the definition of include/lbt_dfxp.h "Range calibration"
against the controller itself, and the calibration pass of a whole model.

* Pick: for random and crafted tensors, every width and target, ``table`` is the controller's own first
  overflow count at every range of its interval, the picked range is the one ``update_range`` leaves where it
  is, and the controller reaches it from the bottom, the top and the default 2. The keep rule fires for a
  tensor that reaches no range.
* Model: ResNet-8, B = 16, 16x16 images (the set-up of test_default_grad_range_makes_first_update_noise).
  After the calibration pass a training step on the same batch moves exactly the kept quantisers (zero
  betas), each by -1, and the first conv weight gradients are closer to the 20-bit gradient than with the
  hand-set grad_range = -6 (measured: defaults 15.4, -6 0.85, calibrated 0.34).
"""
import numpy as np
import pytest

import calib_oracle as C
from oracle import dfxp
from oracle import resnet as oresnet
from test_training import _oracle_params

F32 = np.float32
BITS = (2, 4, 8, 9, 16, 20)
TARGETS = (0.0, 0.01, 0.3)


def _tensors():
    rng = np.random.default_rng(11)
    out = {}
    for k, scale in enumerate((1e-6, 3e-4, 0.07, 1.0, 40.0, 3e5)):
        out["normal%d" % k] = (rng.standard_normal(4097) * scale).astype(F32)
    out["uniform"] = rng.uniform(-1, 1, 1000).astype(F32)
    out["outlier"] = np.concatenate([rng.standard_normal(999).astype(F32) * F32(1e-3), [F32(17.0)]]).astype(F32)
    out["neg_outlier"] = np.concatenate([rng.standard_normal(999).astype(F32) * F32(1e-3), [F32(-16.0)]]).astype(F32)
    pw = np.array([2.0 ** k for k in range(-31, 32)], F32)
    out["pow2"] = np.concatenate([pw, -pw, np.nextafter(pw, F32(np.inf)), np.nextafter(pw, F32(0)),
                                  -np.nextafter(pw, F32(np.inf)), -np.nextafter(pw, F32(0))]).astype(F32)
    out["neg_pow2_only"] = (-pw[20:40]).astype(F32)
    out["specials"] = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.1754942e-38, 0.5, -0.5], F32)
    out["one"] = np.array([0.75], F32)
    out["wide"] = (rng.standard_normal(2000) * np.exp2(rng.uniform(-32, 32, 2000))).astype(F32)
    return out


TENSORS = _tensors()


@pytest.mark.parametrize("name", sorted(TENSORS))
def test_table_and_pick_against_the_controller(name):
    x = TENSORS[name]
    tab = C.table(x)
    assert tab.shape == (C.BINS,)
    assert np.array_equal(np.cumsum(C.hist(x)[::-1])[::-1], tab)  # the scan kernel's histogram, summed from the top
    for bits in BITS:
        lo, hi = bits - 31, bits - 1
        for I in range(lo, hi + 1):
            c1, c2 = dfxp.overflow_counts(x, bits, I)
            assert tab[I + 30] == c1, (bits, I)
            if I > lo:
                assert tab[I - 1 + 30] == c2, (bits, I)  # the second count is c1(I - 1)
        for t in TARGETS:
            I, kept = C.pick(tab, x.size, bits, t)
            if kept:  # nothing of x reaches 2^lo: the controller would walk down to lo and stay
                assert dfxp.overflow_counts(x, bits, lo)[0] == 0
                assert C.iterate(x, t, bits, 2 if lo <= 2 <= hi else hi) == lo
                continue
            assert dfxp.update_range(x, t, bits, I) == I, (bits, t, I)
            fixed = [J for J in range(lo, hi + 1) if dfxp.update_range(x, t, bits, J) == J]
            assert fixed == [I], (bits, t, fixed)  # the only range the controller leaves alone
            for start in (lo, hi, 2 if lo <= 2 <= hi else hi):
                assert C.iterate(x, t, bits, start) == I, (bits, t, start)


@pytest.mark.parametrize("bits", BITS)
def test_keep_rule(bits):
    lo = bits - 31
    below = np.array([2.0 ** (lo - 1), -(2.0 ** lo), 0.0, 2.0 ** lo * (1 - 2.0 ** -24)], F32)  # none reaches 2^lo
    for x in (np.zeros(64, F32), below):
        for t in TARGETS:
            assert C.pick(C.table(x), x.size, bits, t) == (None, True)
    at = np.array([2.0 ** lo], F32)  # one element AT 2^lo overflows there: not kept
    assert C.pick(C.table(at), 1, bits, 1.0) == (lo, False)
    assert C.pick(C.table(at), 1, bits, 0.0) == (lo + 1, False)


def test_model_calibration_is_the_controllers_fixed_point(monkeypatch):
    rng = np.random.default_rng(3)
    x = ((rng.integers(0, 256, size=(16, 16, 16, 3)) - 127.5) / 128).astype(F32)
    y = rng.integers(0, 10, 16)

    def model(bits):
        om = oresnet.build_resnet((1, 1, 1), bits, 2e-4)
        oresnet.set_params(om, _oracle_params(om, 0))
        return om

    def grads(bits, grad_i0, other_i0):
        om = model(bits)
        r = {k: (grad_i0 if k.endswith("grad_range") else other_i0) for k in om.range_names()}
        return oresnet.forward_backward(om, r, x, y, 0, 0)[2]

    ref = grads(20, -2, 6)
    keys = ["conv1/W", "block16-1-1/W", "block32-1-1/W", "block64-1-2/W"]

    def rel(g):
        return min(np.linalg.norm(g[k] - ref[k]) / np.linalg.norm(ref[k]) for k in keys)

    om = model(8)
    ranges = oresnet.init_ranges(om)
    _, _, g_cal, ctx = C.calibrate(lambda: oresnet.forward_backward(om, ranges, x, y, 0, 0), monkeypatch)
    g_cal = {k: v.copy() for k, v in g_cal.items()}
    assert sorted(ctx.set) + sorted(ctx.kept) and set(ctx.set) | set(ctx.kept) == set(om.range_names())
    assert ctx.kept and all(k.endswith("/b_range") for k in ctx.kept), ctx.kept  # the zero betas
    assert all(ranges[k] == 2 for k in ctx.kept)
    # one ordinary step on the same batch: the calibrated ranges are where the controller stands still
    p = oresnet.get_params(om)
    state = dict(params=p, accum={k: np.zeros_like(v) for k, v in p.items()}, ranges=dict(ranges), step=0)
    _, new, _ = oresnet.train_step(om, state, x, y, lr=1e-2, momentum=0.9, seed=0)
    moved = {k: new["ranges"][k] - ranges[k] for k in ranges if new["ranges"][k] != ranges[k]}
    assert moved == {k: -1 for k in ctx.kept}, moved
    e_default, e_low, e_cal = rel(grads(8, 2, 2)), rel(grads(8, -6, 2)), rel(g_cal)
    print("relative error of the first conv weight gradients: defaults %.3g, grad_range=-6 %.3g, calibrated %.3g"
          % (e_default, e_low, e_cal))
    assert e_cal < e_low < e_default, (e_cal, e_low, e_default)
    grad_ranges = sorted({v for k, v in ctx.set.items() if k.endswith("grad_range")})
    assert len(grad_ranges) > 1, grad_ranges  # layer by layer: no single right constant

"""The fused conv kernels' in-image phase-1 enumeration at the smallest batches.

conv_fwd_fused_kernel / conv_bwd_kernel run their phase-1 element chain only over the halo rows inside
the image and the columns 0 .. W-1; the padding cells of the LDS halo image are filled by plain stores
(conv_fused.h halo_pad_fill). At B = 2 .. 6 every stage takes 2-row tiles (lbt_conv_fused_tile_rows), so one
launch holds tiles at the top edge (no row above), in the middle and at the bottom edge (no row below)
of one, two or three sample pairs, and an odd batch. The 4- and 8-row tiles run in
test_gpu_parity.py's B = 32 .. 128 cases.
"""
import numpy as np
import pytest
import torch

from lbt_amd.runtime import DfxpContext
from oracle import nn as onn
from oracle import resnet as oresnet

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _batch(B, seed):
    rng = np.random.default_rng(seed)
    x = ((rng.integers(0, 256, size=(B, 32, 32, 3)) - 127.5) / 128).astype(np.float32)
    y = rng.integers(0, 10, size=B).astype(np.int32)
    return torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)


def _params(gm):
    out = {}
    for owner, var, _ in gm.param_slots():
        out[owner.name + {"W": "/W", "gamma": "/g", "beta": "/b"}[var]] = getattr(owner, var).detach().cpu().numpy().copy()
    return out


def _two_steps(B, fused, graph):
    from lbt_amd.fused import FusedResNet
    from lbt_amd.models import CIFAR10_Resnet20
    from lbt_amd.trainer import Trainer
    ctx = DfxpContext(seed=4)
    m = FusedResNet(CIFAR10_Resnet20(8, weight_decay=2e-4, ctx=ctx))
    m.fuse_bwd = m.fuse_fwd = fused
    tr = Trainer(m, lr=1e-2, momentum=0.9, batch_size=B, use_graph=graph)
    for i in range(2):
        tr.step(*_batch(B, 30 + i))
    torch.cuda.synchronize()
    nb = sum(1 for f in m._bwd if getattr(f, "kname", "") == "conv_bwd_kernel")
    nf = sum(1 for f in m._fwd if getattr(f, "kname", "") == "conv_fwd_fused_kernel")
    assert (nb, nf) == ((16, 16) if fused else (0, 0)), (nb, nf)
    bn = [t.cpu().numpy() for l in tr._bn_layers() for t in (l.X_mean_running, l.X_var_running)]
    return (tr.flat.g.cpu().numpy(), tr.flat.a.cpu().numpy(), tr.flat.w.cpu().numpy(), ctx.ranges(), bn,
            m.loss.item())


@pytest.mark.parametrize("B,graph", [(2, False), (3, True), (4, True), (6, False)])
def test_fused_conv_small_batch_equals_launch_sequence(B, graph):
    """The fused conv launches (in-image phase 1) == the unfused launch sequence (fuse_bwd = fuse_fwd =
    False) after two optimiser steps: gradients, momentum, weights, exponents, BN running statistics
    and loss bit for bit; eager and graph replay."""
    a = _two_steps(B, False, False)
    b = _two_steps(B, True, graph)
    for i in range(3):
        assert np.array_equal(a[i], b[i]), i
    assert a[3] == b[3]
    assert len(a[4]) == len(b[4]) > 0
    for u, v in zip(a[4], b[4]):
        assert np.array_equal(u, v)
    assert a[5] == b[5]


def test_fused_conv_small_batch_bitexact_vs_oracle():
    """B = 4 on the fused plan with graph replay against the oracle for two optimiser steps (d loss /
    d logits injected): weights, exponents and BN running statistics bit-identical, loss at 1e-5."""
    from lbt_amd.dfxp.layers import Normalization_q
    from lbt_amd.fused import FusedResNet
    from lbt_amd.models import CIFAR10_Resnet20
    from lbt_amd.trainer import Trainer
    B = 4
    ctx = DfxpContext(seed=0)
    gm = CIFAR10_Resnet20(8, weight_decay=2e-4, ctx=ctx)
    om = oresnet.build_resnet((3, 3, 3), 8, 2e-4)
    fm = FusedResNet(gm)
    state = dict(params=_params(gm), accum=None, ranges=oresnet.init_ranges(om), step=0)
    state["accum"] = {k: np.zeros_like(v) for k, v in state["params"].items()}
    tr = Trainer(fm, lr=1e-2, momentum=0.9, batch_size=B, use_graph=True)
    gn = [l for l in gm._walk() if isinstance(l, Normalization_q)]
    on = [l for l in oresnet._walk(om) if isinstance(l, onn.NormQ)]
    assert len(gn) == len(on) == 21
    for i in range(2):
        x, y = _batch(B, 50 + i)
        loss = tr.step(x, y).item()
        torch.cuda.synchronize()
        dz = fm.dlogits.cpu().numpy()
        lref, state, octx = oresnet.train_step(om, state, x.cpu().numpy(), y.cpu().numpy(), lr=1e-2, momentum=0.9,
                                               seed=0, dz=dz)
        assert abs(loss - lref) <= 1e-5 * abs(lref), (i, loss, lref)
        gp = _params(gm)
        for k in gp:
            assert np.array_equal(gp[k], state["params"][k]), (i, k)
        assert ctx.ranges() == state["ranges"], i
        for g, o in zip(gn, on):
            assert np.array_equal(g.X_mean_running.cpu().numpy(), o.mean_running), (i, g.name)
            assert np.array_equal(g.X_var_running.cpu().numpy(), o.var_running), (i, g.name)

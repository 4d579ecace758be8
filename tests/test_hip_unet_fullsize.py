"""-m gpu: the U-Net's own kernels at the sizes of its 128^3 training step (NumChannel 16, 4 levels; profiles/unet_layer_table.txt):
the 3^3 instantiations of the fp32 MFMA convolution family, the 2x2x2 max-pooling streams past their grid cap, and ops.bn_concat on
its own.  On the pattern of tests/test_hip_fullsize.py, which does the same for the V-Net's 5^3 kernels:
(a) the oracle on crops of the full-size tensors (a 3^3 SAME convolution on a block depends on the block + 1 voxel of halo),
(b) integer-valued known answers, bit-exact in fp32,
(c) identities over all voxels with fp64 dot products,
and whole-volume oracle comparisons where the volume is small enough (32^3 and below).

Every bound is one the suite already holds: 2e-6 rel-L2 is the project's kernel bound (tests/test_hip_ops._conv_case, the 5^3
full-size test), 1e-5 linearity and 2e-6 |a||b| adjointness are test_conv_identities_full_resolution's, the batch-norm tolerances are
tests/test_hip_ops._bn_act_case's, the moment identities test_bn_and_loss_head_full_resolution's.  Pooling is compared bit for bit."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import vnet_oracle as O
from tests import unet_oracle as U
from tests.test_hip_fullsize import _crop_blocks, _dot, _oracle_block, _scale
from tests.test_hip_ops import _conv_case
from tests.test_hip_unet import epilogue_statistics_case
from tests.util import g, check_close, rel_l2

pytestmark = pytest.mark.gpu
P = 128


# ---- 1a. 3^3 convolutions against the oracle ---------------------------------------------------------------------------------------
def _blocks(dims):
    """(z0, y0, x0) of four 12^3 output blocks: a corner, an edge, the interior, the far corner (128^3: those of the 5^3 test)."""
    if tuple(dims) == (P, P, P):
        return _crop_blocks()
    D, H, W = dims
    return [(0, 0, 0), (0, H // 2 - 6, W - 12), (D // 2 - 7, H // 2 - 3, W // 2 - 14), (D - 12, H - 12, W - 12)]


def _conv3_tags(B, W, C0, C1, Co):
    shape = "%d^3x%d " % (W, B)
    return ["conv k3 s1 " + shape + "%d->%d" % (C0 + C1, Co), "conv k3 s1 " + shape + "%d->%d" % (Co, C0 + C1),
            "wgrad k3 s1 " + shape + "%d->%d" % (C0 + C1, Co)]


def _crop_case(dev, mode, B, D, H, W, C0, C1, Co):
    """Forward on four 12^3 blocks (1-voxel halo), then backward with dy supported on one 10^3 block that touches the high x face:
    dx on block + halo, exactly 0.0 outside block + 1 voxel, dw and db of the whole filter.  Returns (y, dx0, dx1, dw, db)."""
    from vnet_tensorflow_amd import ops
    dims = (D, H, W)
    gen = torch.Generator(device="cpu").manual_seed(4321 + D + H + W + C0 + C1 + Co)
    x0 = torch.randn(B, D, H, W, C0, generator=gen)
    x1 = torch.randn(B, D, H, W, C1, generator=gen) if C1 else None
    w = torch.randn(3, 3, 3, C0 + C1, Co, generator=gen) * 0.1
    b = torch.randn(Co, generator=gen)
    tx0 = x0.to(dev).requires_grad_(True)
    tx1 = x1.to(dev).requires_grad_(True) if C1 else None
    tw, tb = w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    xcat = x0.numpy() if x1 is None else np.concatenate((x0.numpy(), x1.numpy()), -1)
    tag = "conv3 %s [%d,%d,%d,%d] %d+%d->%d" % (mode, B, D, H, W, C0, C1, Co)
    bz, by, bx = D // 2 - 4, 3, W - 10                             # the dy block: x runs to the last voxel of a row
    dyb = torch.randn(B, 10, 10, 10, Co, generator=gen)
    ops.set_compute_dtype(mode)
    try:
        ops.profile_start()
        try:
            y = ops.conv(tx0, tw, tb, 3, 1, x1=tx1)
            dy = torch.zeros_like(y)
            dy[:, bz:bz + 10, by:by + 10, bx:bx + 10, :] = dyb.to(dev)
            y.backward(dy)
        finally:
            recs = ops.profile_stop()
    finally:
        ops.set_compute_dtype("fp32")
    assert sorted(r[0] for r in recs) == sorted(_conv3_tags(B, W, C0, C1, Co)), [r[0] for r in recs]
    for (z0, y0, xx0) in _blocks(dims):
        ref = _oracle_block(xcat, w.numpy(), z0, y0, xx0, halo=1, dims=dims) + b.numpy().astype(np.float64)
        r, m = check_close("%s block %s" % (tag, (z0, y0, xx0)), y[:, z0:z0 + 12, y0:y0 + 12, xx0:xx0 + 12, :], ref, 2e-6)
        print("%s fwd block %s rel-L2 %.2e" % (tag, (z0, y0, xx0), r))
    lo = [max(0, c - 1) for c in (bz, by, bx)]
    hi = [min(n, c + 11) for n, c in zip(dims, (bz, by, bx))]
    xc = xcat[:, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2], :].astype(np.float64)
    dyc = np.zeros(xc.shape[:-1] + (Co,))
    s = [c - l for c, l in zip((bz, by, bx), lo)]
    dyc[:, s[0]:s[0] + 10, s[1]:s[1] + 10, s[2]:s[2] + 10, :] = dyb.numpy()
    # the crop is zero-padded by the oracle where the volume continues: that is exact here because dy is zero there
    dx_ref, dw_ref = O.conv_nd_bwd(xc, w.numpy().astype(np.float64), dyc, 1)
    dxg = torch.cat((tx0.grad, tx1.grad), -1) if C1 else tx0.grad
    r1, _ = check_close(tag + " dx block", dxg[:, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2], :], dx_ref, 2e-6)
    outside = dxg.clone()
    outside[:, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2], :] = 0
    assert float(outside.abs().max()) == 0.0, tag                 # nothing leaks outside block + 1 voxel
    r2, _ = check_close(tag + " dw", tw.grad, dw_ref, 2e-6)
    r3, _ = check_close(tag + " db", tb.grad, dyb.numpy().reshape(-1, Co).sum(0), 2e-6)
    print("%s dx %.2e dw %.2e db %.2e" % (tag, r1, r2, r3))
    return y.detach(), tx0.grad, (tx1.grad if C1 else None), tw.grad, tb.grad


STEP_SHAPES = [
    # B, D, H, W, C0, C1, Cout                also under fp32_split3
    ((1, P, P, P, 1, 0, 16), True),           # first layer: scalar gather, Cin = 1
    ((1, P, P, P, 16, 0, 16), True),          # encoder level 1
    ((1, P, P, P, 16, 16, 16), True),         # decoder level 1, two sources
    ((1, P, P, P, 16, 0, 32), False),         # the backward-data launch of 32 -> 16 as the layer table lists it, run as a forward too
    ((2, 64, 64, 64, 32, 32, 32), False),     # batch 2 at a level with NS > 1
    ((1, 70, 100, 132, 16, 0, 16), False),    # ragged: bricks overhang all three axes, and there are many of them
]


@pytest.mark.parametrize("shape,both", STEP_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_conv3_step_shapes_against_oracle_crops(dev, shape, both):
    """fp32_split3 has no 3^3 form: the two modes launch the same kernels and must give the same bits."""
    a = _crop_case(dev, "fp32", *shape)
    if both:
        b = _crop_case(dev, "fp32_split3", *shape)
        for u, v in zip(a, b):
            assert (u is None and v is None) or torch.equal(u, v)


@pytest.mark.parametrize("shape", [(1, 32, 32, 32, 64, 0, 64), (1, 16, 16, 16, 128, 0, 128), (1, 16, 16, 16, 128, 128, 128)],
                         ids=lambda v: "x".join(map(str, v)))
def test_conv3_deep_levels_whole_volume(dev, shape):
    """Levels 3 and 4 of the step: the whole-volume oracle is affordable, so everything is compared (forward, dx, dw, db; 2e-6)."""
    from vnet_tensorflow_amd import ops
    ops.profile_start()
    try:
        _conv_case(dev, *shape, ks=3, stride=1, seed=sum(shape))
    finally:
        recs = ops.profile_stop()
    B, D, H, W, C0, C1, Co = shape
    assert sorted(r[0] for r in recs) == sorted(_conv3_tags(B, W, C0, C1, Co)), [r[0] for r in recs]


# ---- 1b. bit-exact known answers at 128^3 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C0,C1", [(16, 0), (16, 16)])
def test_conv3_full_resolution_exact_known_answers(dev, C0, C1):
    """Integer-valued cases are exact in fp32, so these are BIT-exact checks of the 3^3 index math at 128^3: ring of 3 slots, 27 taps
    on 32 tap slots, pad = 1.  Then the same two through the accumulating launch on a pre-filled output."""
    from vnet_tensorflow_amd import ops
    C, Co = C0 + C1, 16
    gen = torch.Generator(device="cpu").manual_seed(77 + C)
    xi = torch.randint(-8, 9, (1, P, P, P, C), generator=gen).float().to(dev)       # integers: x + b and prev + y are exact
    src = lambda t: (t[..., :C0].contiguous(), t[..., C0:].contiguous() if C1 else None)
    # delta filter: output channel o copies input channel o of the concat (two sources: o of the first, then of the second half)
    for half in range(2 if C1 else 1):
        w = torch.zeros(3, 3, 3, C, Co, device=dev)
        w[1, 1, 1, half * C0:half * C0 + Co] = torch.eye(Co, device=dev)
        b = torch.arange(Co, device=dev, dtype=torch.float32)
        x0, x1 = src(xi)
        y = ops.conv(x0, w, b, 3, 1, x1=x1)
        assert torch.equal(y, xi[..., half * C0:half * C0 + Co] + b)
    ones = torch.ones(1, P, P, P, C, device=dev)
    wo = torch.ones(3, 3, 3, C, Co, device=dev)
    x0, x1 = src(ones)
    y = ops.conv(x0, wo, torch.zeros(Co, device=dev), 3, 1, x1=x1)
    cnt1 = torch.tensor([2] + [3] * (P - 2) + [2], device=dev, dtype=torch.float32)              # taps inside per axis
    ref = (cnt1[:, None, None] * cnt1[None, :, None] * cnt1[None, None, :] * C)[None, ..., None].expand_as(y)
    assert torch.equal(y, ref)                                     # 8 C at the corners ... 27 C inside
    # y += conv(x) on a pre-filled output
    r = ops.route(ops.FWD, 3, 1, 0, False, False, C0, C1, Co, 1, (P, P, P), (P, P, P))
    prev = torch.randint(-100, 101, (1, P, P, P, Co), generator=gen).float().to(dev)
    wd = torch.zeros(3, 3, 3, C, Co, device=dev)
    wd[1, 1, 1, :Co] = torch.eye(Co, device=dev)
    for xin, wf, want in ((xi, wd, xi[..., :Co]), (ones, wo, ref)):
        x0, x1 = src(xin)
        yp = torch.empty_like(prev)
        ops._conv_launch(r, x0, x1, wf, None, yp)
        acc = prev.clone()
        ops._conv_launch(r, x0, x1, wf, None, acc, accum=True)
        assert torch.equal(yp, want) and torch.equal(acc, prev + yp)


# ---- 1c. identities over all voxels --------------------------------------------------------------------------------------------------
def test_conv3_identities_full_resolution(dev):
    """Linearity in x, adjointness of backward-data, and the filter gradient as the adjoint in w at 128^3, 16 + 16 -> 16, with fp64 dot
    products over all voxels (bounds of test_conv_identities_full_resolution)."""
    from vnet_tensorflow_amd import ops
    C0, C1, Co = 16, 16, 16
    rn = lambda *s: torch.randn(*s, device=dev)
    x0, x1, z0, z1 = (rn(1, P, P, P, c) for c in (C0, C1, C0, C1))
    w = (rn(3, 3, 3, C0 + C1, Co) * 0.1).requires_grad_(True)
    dw_dir = rn(3, 3, 3, C0 + C1, Co) * 0.1
    zero_b = torch.zeros(Co, device=dev)
    yv = rn(1, P, P, P, Co)
    a0, a1 = x0.clone().requires_grad_(True), x1.clone().requires_grad_(True)
    cx = ops.conv(a0, w, zero_b, 3, 1, x1=a1)
    cz = ops.conv(z0, w, zero_b, 3, 1, x1=z1)
    lin = ops.conv(2.0 * x0 - 0.5 * z0, w, zero_b, 3, 1, x1=2.0 * x1 - 0.5 * z1)
    want = (2.0 * cx - 0.5 * cz).detach().double()
    e = float((lin.detach().double() - want).norm() / want.norm())
    cx.backward(yv)
    lhs = _dot(cx.detach(), yv)
    e_adj = abs(lhs - _dot(x0, a0.grad) - _dot(x1, a1.grad)) / _scale(cx.detach(), yv)
    cdir = ops.conv(x0, dw_dir, zero_b, 3, 1, x1=x1)
    e_w = abs(_dot(cdir.detach(), yv) - _dot(dw_dir, w.grad)) / _scale(cdir.detach(), yv)
    print("conv3 identities 128^3 16+16->16: linearity %.2e adjoint %.2e filter adjoint %.2e" % (e, e_adj, e_w))
    assert e < 1e-5
    assert e_adj <= 2e-6                                           # <conv(x), y> = <x, conv^T(y)>
    assert e_w <= 2e-6                                             # <conv_dw(x), y> = <dw, wgrad(x, y)>


# ---- 1d. epilogue statistics at full size ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,Cin,Cout,residual", [((1, P, P, P), 16, 16, True), ((2, 64, 64, 64), 32, 32, False)])
def test_conv3_epilogue_statistics_full_size(dev, shape, Cin, Cout, residual):
    epilogue_statistics_case(dev, shape, Cin, Cout, residual)


# ---- 1e. max-pooling past the grid cap --------------------------------------------------------------------------------------------------
def _pool_cap():
    """Units one trip of the pooling kernels' grid-stride loops covers, read from the source so that a change of the cap is seen."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vnet_tensorflow_amd", "csrc", "pool.hip")).read()
    m = re.search(r"constexpr int POOL_BLOCK = (\d+), POOL_MAXBLK = (\d+);", src)
    assert m, "pool.hip no longer states POOL_BLOCK / POOL_MAXBLK in one line"
    return int(m.group(1)) * int(m.group(2))


def _pool_torch(x, dy=None):
    xc = x.clone().requires_grad_(True)
    yc = torch.nn.functional.max_pool3d(xc.permute(0, 4, 1, 2, 3), 2, 2).permute(0, 2, 3, 4, 1)
    if dy is None:
        return yc.detach()
    yc.backward(dy)
    return yc.detach(), xc.grad


@pytest.mark.parametrize("shape,fwd_trips", [
    ((1, P, P, P, 16), False),          # the step's level 1: the backward takes eight trips (the forward exactly one)
    ((1, P, P, P, 32), True),           # ... and a forward of two trips on the float4 path
    ((2, 64, 64, 64, 32), False),
    ((1, 127, 129, 130, 16), False),    # odd axes at size
    ((1, P, P, P, 6), True),            # scalar units
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_max_pool_past_the_grid_cap(dev, shape, fwd_trips):
    from vnet_tensorflow_amd import _lib, ops
    L = _lib.lib()
    B, D, H, W, C = shape
    cu = C // 4 if C % 4 == 0 else C
    cap = _pool_cap()
    assert B * D * H * W * cu > cap, "the backward no longer takes a second trip through its loop"
    assert not fwd_trips or B * (D // 2) * (H // 2) * (W // 2) * cu > cap, "the forward no longer takes a second trip"
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=gen)                              # tie-free
    dy = torch.randn(B, D // 2, H // 2, W // 2, C, generator=gen)
    yc, dxc = _pool_torch(x, dy)
    xg = x.to(dev).requires_grad_(True)
    y = ops.max_pool2(xg)
    assert tuple(y.shape) == tuple(yc.shape) and torch.equal(y.detach().cpu(), yc)
    y.backward(dy.to(dev))
    assert torch.equal(xg.grad.cpu(), dxc)
    prev = torch.randn(*shape, generator=gen).to(dev)
    acc = prev.clone()
    s = torch.cuda.current_stream().cuda_stream
    yd, dyd, xd = y.detach().contiguous(), dy.to(dev), xg.detach()
    assert L.vnet_maxpool2_bwd(dyd.data_ptr(), xd.data_ptr(), yd.data_ptr(), acc.data_ptr(), C, B, D, H, W, 1, s) == 0
    assert torch.equal(acc, prev + xg.grad)


@pytest.mark.parametrize("shape", [(1, 64, 64, 64, 32), (1, 33, 66, 35, 16)], ids=lambda v: "x".join(map(str, v)))
def test_max_pool_relu_ties_and_conservation(dev, shape):
    """The realistic tie case: x = relu(randn), about 1 window in 256 all zero.  Forward and backward bit-identical to the oracle
    (first maximum in scan order); exactly one winner per window; sum(dx) == sum(dy) per channel for integer dy."""
    from vnet_tensorflow_amd import ops
    B, D, H, W, C = shape
    d, h, w = D // 2, H // 2, W // 2
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.relu(torch.randn(*shape, generator=gen))
    win = U.max_pool2_fwd(x.numpy())[0]
    assert (win.max(0) == 0).mean() > 1.0 / 1024, "no all-zero windows in this draw"
    dy = torch.randint(-3, 4, (B, d, h, w, C), generator=gen).float()
    v = O.Var(x.numpy().astype(np.float64))
    yo = U.max_pool2(v)
    O.backward(yo, seed=dy.numpy().astype(np.float64))
    for dyt, ref in ((dy, v.g), (torch.ones_like(dy), None)):
        xg = x.to(dev).requires_grad_(True)
        y = ops.max_pool2(xg)
        assert np.array_equal(y.detach().cpu().numpy(), yo.v)
        y.backward(dyt.to(dev))
        dx = xg.grad
        if ref is not None:
            assert np.array_equal(dx.cpu().numpy(), ref)
            assert torch.equal(dx.double().sum((0, 1, 2, 3)).cpu(), dyt.double().sum((0, 1, 2, 3)))
        else:                                                      # dy = 1: every window has exactly one voxel with dx = 1
            inner = dx[:, :2 * d, :2 * h, :2 * w].reshape(B, d, 2, h, 2, w, 2, C)
            assert torch.equal(inner.sum((2, 4, 6)), torch.ones(B, d, h, w, C, device=dev))
            assert float(dx.max()) == 1.0 and float(dx.min()) == 0.0 and float(dx.sum()) == float(B * d * h * w * C)


def test_max_pool_scalar_kernel_through_a_misaligned_view(dev):
    """C % 4 == 0 takes the float4 kernels unless a pointer is not 16-byte aligned: a view offset by one float.  This reaches the
    scalar kernels only as long as ops.max_pool2 hands the view's own pointer to the library (its .contiguous() is a no-op on a
    contiguous view) -- the launch tag does not tell the two kernels apart, so the assertions on data_ptr below are what keeps the
    premise; a copy to an aligned buffer inside ops would need this test to call _lib directly."""
    from vnet_tensorflow_amd import ops
    shape = (2, 6, 10, 12, 8)
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(*shape, generator=gen)
    dy = torch.randn(2, 3, 5, 6, 8, generator=gen)
    yc, dxc = _pool_torch(x, dy)
    buf = torch.empty(x.numel() + 1, device=dev)
    xv = buf[1:].view(shape)
    xv.copy_(x)
    assert xv.data_ptr() % 16 == 4 and xv.is_contiguous()
    xg = xv.detach().requires_grad_(True)
    assert xg.data_ptr() == xv.data_ptr()
    y = ops.max_pool2(xg)
    assert torch.equal(y.detach().cpu(), yc)
    y.backward(dy.to(dev))
    assert torch.equal(xg.grad.cpu(), dxc)


# ---- 1f. ops.bn_concat on its own ---------------------------------------------------------------------------------------------------
def _bn_concat_oracle(x0, x1, gamma, beta, dy0, dy1):
    X0, X1, G_, B_ = O.Var(x0), O.Var(x1), O.Var(gamma), O.Var(beta)
    st = []
    y = O.batch_norm_train(O.concat_channels(X0, X1), G_, B_, stats_out=st)
    O.backward(y, np.concatenate((dy0, dy1), -1))
    return y.v, X0.g, X1.g, G_.g, B_.g, st[0]


@pytest.mark.parametrize("shp,C0,C1", [((2, 5, 9, 13), 4, 4), ((2, 5, 9, 13), 8, 24), ((1, 16, 16, 16), 32, 32)])
def test_bn_concat(dev, shp, C0, C1):
    """Against the fp64 batch-norm of the concatenated tensor, at the tolerances _bn_act_case holds ops.bn_act to.  Unequal halves:
    the op accepts them, the network never passes them."""
    from vnet_tensorflow_amd import ops
    rng = np.random.default_rng(C0 * 100 + C1)
    C = C0 + C1
    x0, x1 = rng.standard_normal(shp + (C0,)) * 3.0 + 1.5, rng.standard_normal(shp + (C1,)) * 0.7 - 2.0
    gamma, beta = rng.uniform(0.5, 1.5, C), rng.standard_normal(C)
    dy0, dy1 = rng.standard_normal(shp + (C0,)), rng.standard_normal(shp + (C1,))
    y_ref, dx0_ref, dx1_ref, dg_ref, db_ref, (mu, var) = _bn_concat_oracle(x0, x1, gamma, beta, dy0, dy1)
    tag = "bn_concat %s %d+%d" % (shp, C0, C1)

    def run(which):
        t0, t1, tg, tb = (g(a, dev).requires_grad_(True) for a in (x0, x1, gamma, beta))
        mm, mv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        y0, y1 = ops.bn_concat(t0, t1, tg, tb, mm, mv)
        outs = [(y0, g(dy0, dev)), (y1, g(dy1, dev))]
        torch.autograd.backward([outs[k][0] for k in which], [outs[k][1] for k in which])
        return y0, y1, t0, t1, tg, tb, mm, mv

    y0, y1, t0, t1, tg, tb, mm, mv = run((0, 1))
    check_close(tag + " y0", y0, y_ref[..., :C0], 5e-6)
    check_close(tag + " y1", y1, y_ref[..., C0:], 5e-6)
    check_close(tag + " dx0", t0.grad, dx0_ref, 5e-5, atol=1e-5)
    check_close(tag + " dx1", t1.grad, dx1_ref, 5e-5, atol=1e-5)
    for nm, got, ref in (("dgamma", tg.grad, dg_ref), ("dbeta", tb.grad, db_ref)):
        assert tuple(got.shape) == (C,)
        check_close(tag + " %s[:C0]" % nm, got[:C0], ref[:C0], 2e-5)
        check_close(tag + " %s[C0:]" % nm, got[C0:], ref[C0:], 2e-5)
    for sl in (slice(0, C0), slice(C0, C)):
        check_close(tag + " moving_mean", mm[sl], 0.01 * mu[sl], 1e-5, atol=1e-7)
        check_close(tag + " moving_var", mv[sl], 0.99 + 0.01 * var[sl], 1e-5)
    # one half alone: its slice of dgamma / dbeta as before (the halves of a batch-norm do not couple), the other slice exactly zero
    for k, (own, other) in enumerate(((slice(0, C0), slice(C0, C)), (slice(C0, C), slice(0, C0)))):
        _, _, h0, h1, hg, hb, _, _ = run((k,))
        for nm, got, ref in (("dgamma", hg.grad, dg_ref), ("dbeta", hb.grad, db_ref)):
            check_close(tag + " half %d %s own slice" % (k, nm), got[own], ref[own], 2e-5)
            assert float(got[other].abs().max()) == 0.0, (tag, k, nm)
        check_close(tag + " half %d dx" % k, (h0, h1)[k].grad, (dx0_ref, dx1_ref)[k], 5e-5, atol=1e-5)
        og = (h0, h1)[1 - k].grad
        assert og is None or float(og.abs().max()) == 0.0


@pytest.mark.parametrize("pool_first", [True, False])
def test_bn_concat_fork_with_max_pool(dev, pool_first):
    """The skip feature x1 feeds the concat batch-norm AND the max-pooling (ops.fork).  pool_first (the network's order: the encoder's
    pooling is recorded before the decoder's batch-norm, so the batch-norm's backward runs first and leaves its gradient in
    ctx.slot1, and the pooling kernel accumulates into it): x1's gradient is the oracle's sum of the two, either way."""
    from vnet_tensorflow_amd import ops
    rng = np.random.default_rng(5 + pool_first)
    shp, C0, C1 = (2, 6, 10, 12), 8, 8
    x0, x1 = rng.standard_normal(shp + (C0,)) * 2.0 + 0.5, rng.standard_normal(shp + (C1,)) * 1.5 - 1.0
    x0, x1 = x0.astype(np.float32).astype(np.float64), x1.astype(np.float32).astype(np.float64)
    gamma, beta = rng.uniform(0.5, 1.5, C0 + C1), rng.standard_normal(C0 + C1)
    dy0, dy1, dp = rng.standard_normal(shp + (C0,)), rng.standard_normal(shp + (C1,)), rng.standard_normal((2, 3, 5, 6, C1))
    _, dx0_ref, dx1_ref, dg_ref, db_ref, _ = _bn_concat_oracle(x0, x1, gamma, beta, dy0, dy1)
    v = O.Var(x1)
    O.backward(U.max_pool2(v), seed=dp)
    t0, t1, tg, tb = (g(a, dev).requires_grad_(True) for a in (x0, x1, gamma, beta))
    skip, down = ops.fork(t1 * 1.0)                                # (a non-leaf, as in the network)
    if pool_first:
        p = ops.max_pool2(down)
        y0, y1 = ops.bn_concat(t0, skip, tg, tb)
    else:
        y0, y1 = ops.bn_concat(t0, skip, tg, tb)
        p = ops.max_pool2(down)
    torch.autograd.backward([y0, y1, p], [g(dy0, dev), g(dy1, dev), g(dp, dev)])
    tag = "bn_concat fork pool_first=%s" % pool_first
    check_close(tag + " dx1 (batch-norm + pooling)", t1.grad, dx1_ref + v.g, 5e-5, atol=1e-5)
    check_close(tag + " dx0", t0.grad, dx0_ref, 5e-5, atol=1e-5)
    check_close(tag + " dgamma", tg.grad, dg_ref, 2e-5)
    check_close(tag + " dbeta", tb.grad, db_ref, 2e-5)


def test_bn_concat_full_resolution(dev):
    """(1, 128, 128, 128) 16 + 16: the moment identities of test_bn_and_loss_head_full_resolution for both halves (mean = beta,
    var = gamma^2 s^2 / (s^2 + eps); 1e-5), and the backward against the batch-norm formulas evaluated in float64 on the device from
    the same float32 operands, at _bn_act_case's tolerances."""
    from vnet_tensorflow_amd import ops
    C0 = C1 = 16
    gen = torch.Generator(device=dev).manual_seed(3)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)
    xs = [(rn(1, P, P, P, C0) * 3.0 + 1.5).requires_grad_(True), (rn(1, P, P, P, C1) * 0.5 - 1.0).requires_grad_(True)]
    gamma = (torch.rand(C0 + C1, device=dev, generator=gen) + 0.5).requires_grad_(True)
    beta = rn(C0 + C1).requires_grad_(True)
    dys = [rn(1, P, P, P, C0), rn(1, P, P, P, C1)]
    mm, mv = torch.zeros(C0 + C1, device=dev), torch.ones(C0 + C1, device=dev)
    ys = ops.bn_concat(xs[0], xs[1], gamma, beta, mm, mv)
    torch.autograd.backward(list(ys), dys)
    M = P ** 3
    for k, sl in enumerate((slice(0, C0), slice(C0, C0 + C1))):
        x = xs[k].detach().double().reshape(-1, C0)
        mu, var = x.mean(0), x.var(0, unbiased=False)
        gm, bt = gamma.detach().double()[sl], beta.detach().double()[sl]
        yd = ys[k].detach().double().reshape(-1, C0)
        assert float((yd.mean(0) - bt).abs().max()) < 1e-5
        ref_var = gm ** 2 * var / (var + 1e-3)
        assert float(((yd.var(0, unbiased=False) - ref_var) / ref_var).abs().max()) < 1e-5
        inv = 1.0 / torch.sqrt(var + 1e-3)
        xh = (x - mu) * inv
        dy = dys[k].double().reshape(-1, C0)
        dbeta, dgamma = dy.sum(0), (dy * xh).sum(0)
        dx = gm * inv * (dy - dbeta / M - xh * dgamma / M)
        tag = "bn_concat 128^3 half %d" % k
        check_close(tag + " dgamma", gamma.grad[sl], dgamma.cpu().numpy(), 2e-5)
        check_close(tag + " dbeta", beta.grad[sl], dbeta.cpu().numpy(), 2e-5)
        e = float((xs[k].grad.double().reshape(-1, C0) - dx).norm() / dx.norm())
        print("%s dx rel-L2 %.2e" % (tag, e))
        assert e < 5e-5
        check_close(tag + " moving_mean", mm[sl], (0.01 * mu).cpu().numpy(), 1e-5, atol=1e-7)
        check_close(tag + " moving_var", mv[sl], (0.99 + 0.01 * var).cpu().numpy(), 1e-5)

"""-m gpu: guard bands (tests/guard.py) around the entry points the U-Net adds or opens: the two max-pooling entry
points of include/vnet_hip_unet.h and the ks = 3 forward / statistics / accumulate / filter-gradient launches of vnet_hip.h.  Every
tensor of a launch is carved from a guarded arena, scratch has exactly the queried size; checked: (a) every guard byte intact and no
input modified, (b) every output byte written on the 0xFF pre-fill -- this is what catches a dx element the pooling backward left
unwritten -- (c) results against the fp64 oracle, (d) bit-identical results on a 0xFF and a 0x00 pre-fill.
CASES (entry points a case must reach, function) is what the ledger test in tests/test_abi_ledger.py reads."""
import numpy as np
import pytest
import torch

from oracle import vnet_oracle as O
from tests import guard, unet_oracle as U
from tests.util import check_close

pytestmark = pytest.mark.gpu


def _out(h, name, shape):
    return h.arena.tensor(name, shape, torch.float32, "out")


def _io(h, name, a):
    a = np.ascontiguousarray(a)
    return h.arena.tensor(name, a.shape, torch.float32, "inout", torch.as_tensor(a).to(torch.float32))


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _pool(B, D, H, W, C):
    def run(h):
        from vnet_tensorflow_amd import _lib, ops
        L = _lib.lib()
        rng = np.random.default_rng(B + D + H + W + C)
        x = rng.standard_normal((B, D, H, W, C)).astype(np.float32)
        win, y_ref = U.max_pool2_fwd(x.astype(np.float64))
        dy = rng.standard_normal(y_ref.shape).astype(np.float32)
        v = O.Var(x.astype(np.float64))
        O.backward(U.max_pool2(v), seed=dy.astype(np.float64))
        prev = rng.standard_normal(x.shape).astype(np.float32)
        tx, tdy = h.g(x), h.g(dy)
        y, dx, acc = _out(h, "y", y_ref.shape), _out(h, "dx", x.shape), _io(h, "acc", prev)
        s = ops._stream()
        assert L.vnet_maxpool2_fwd(tx.data_ptr(), y.data_ptr(), C, B, D, H, W, s) == 0
        assert L.vnet_maxpool2_bwd(tdy.data_ptr(), tx.data_ptr(), y.data_ptr(), dx.data_ptr(), C, B, D, H, W, 0, s) == 0
        assert L.vnet_maxpool2_bwd(tdy.data_ptr(), tx.data_ptr(), y.data_ptr(), acc.data_ptr(), C, B, D, H, W, 1, s) == 0
        assert np.array_equal(_np(y), y_ref) and np.array_equal(_np(dx), v.g)
        assert np.array_equal(acc.cpu().numpy(), prev + dx.cpu().numpy())
    return run


def _pool_autograd(h):
    """ops.max_pool2 as the network calls it: forward + backward through the autograd Function, tensors from the arena."""
    from vnet_tensorflow_amd import ops
    rng = np.random.default_rng(77)
    x = rng.standard_normal((2, 5, 6, 7, 8)).astype(np.float32)
    tx = h.g(x).requires_grad_(True)
    y = ops.max_pool2(tx)
    dy = rng.standard_normal(tuple(y.shape)).astype(np.float32)
    (dx,) = torch.autograd.grad(y, tx, h.g(dy))
    v = O.Var(x.astype(np.float64))
    yo = U.max_pool2(v)
    O.backward(yo, seed=dy.astype(np.float64))
    assert np.array_equal(_np(y), yo.v) and np.array_equal(_np(dx), v.g)


def _conv3(B, D, H, W, C0, C1, Co, stats):
    """3^3 forward (+ bias), with statistics rows of exactly Route.stats_rows where the shape has them, y += conv, the backward-data
    launch into two destinations and the filter gradient with scratch of exactly Route.ws."""
    def run(h):
        from vnet_tensorflow_amd import ops
        rng = np.random.default_rng(B + D + H + W + C0 + C1 + Co)
        x0 = rng.standard_normal((B, D, H, W, C0))
        x1 = rng.standard_normal((B, D, H, W, C1)) if C1 else None
        xc = x0 if x1 is None else np.concatenate((x0, x1), -1)
        w, b = rng.standard_normal((3, 3, 3, C0 + C1, Co)) * 0.1, rng.standard_normal(Co)
        prev, dy = rng.standard_normal((B, D, H, W, Co)), rng.standard_normal((B, D, H, W, Co))
        dims = (D, H, W)
        tx0, tx1, tw, tb, tdy = h.g(x0), (h.g(x1) if C1 else None), h.g(w), h.g(b), h.g(dy)
        conv = O.conv_nd_fwd(xc, w, 1)
        dx_ref, dw_ref = O.conv_nd_bwd(xc, w, dy, 1)
        r = ops.route(ops.FWD, 3, 1, 0, False, False, C0, C1, Co, B, dims, dims)
        assert r.family == "conv" and (r.stats_rows > 0) == stats, r
        y = _out(h, "y", (B, D, H, W, Co))
        if stats:
            st = _out(h, "stats", (r.stats_rows, 2 * Co))
            ops._conv_launch(r, tx0, tx1, tw, tb, y, stats=st)
            v = _np(y).reshape(-1, Co)
            part = _np(st).sum(0)
            np.testing.assert_allclose(part[:Co], v.sum(0), rtol=2e-5, atol=1e-6 * np.abs(v).sum(0).max())
            np.testing.assert_allclose(part[Co:], (v * v).sum(0), rtol=2e-5)
        else:
            ops._conv_launch(r, tx0, tx1, tw, tb, y)
        check_close("y", y, conv + b, 2e-6)
        acc = _io(h, "acc", prev)
        ops._conv_launch(r, tx0, tx1, tw, None, acc, accum=True)
        check_close("y += conv", acc, conv + prev, 2e-6)
        rb = ops.route(ops.BWD, 3, 1, 0, False, False, C0, C1, Co, B, dims, dims)
        dx0, dx1 = _out(h, "dx0", x0.shape), (_out(h, "dx1", x1.shape) if C1 else None)
        ops._conv_launch(rb, tdy, None, tw, None, dx0, dx1)
        check_close("dx0", dx0, dx_ref[..., :C0], 2e-6)
        if C1:
            check_close("dx1", dx1, dx_ref[..., C0:], 2e-6)
        rw = ops.route(ops.WGRAD, 3, 1, 0, False, False, C0, C1, Co, B, dims, dims)
        dw = _out(h, "dw", w.shape)
        n0 = len(h.ws_requests)
        ops._wgrad_launch(rw, tx0, tx1, tdy, dw)
        assert all(q <= rw.ws for q in h.ws_requests[n0:]), (rw.ws, h.ws_requests[n0:])
        check_close("dw", dw, dw_ref, 2e-6)
    return run


_CONV = ("vnet_pack_weights", "vnet_conv_fwd", "vnet_conv_fwd_acc", "vnet_conv_wgrad")
CASES = {
    "pool 8^3x1 c4": (("vnet_maxpool2_fwd", "vnet_maxpool2_bwd"), _pool(1, 8, 8, 8, 4)),
    "pool odd 5x7x9x2 c3 (scalar path)": (("vnet_maxpool2_fwd", "vnet_maxpool2_bwd"), _pool(2, 5, 7, 9, 3)),
    "pool odd 3x6x11x2 c20": (("vnet_maxpool2_fwd", "vnet_maxpool2_bwd"), _pool(2, 3, 6, 11, 20)),
    "pool through ops.max_pool2": (("vnet_maxpool2_fwd", "vnet_maxpool2_bwd"), _pool_autograd),
    "conv3 first layer 8^3x2 1->4": (_CONV + ("vnet_conv_fwd_stats",), _conv3(2, 8, 8, 8, 1, 0, 4, True)),
    "conv3 ragged 5x9x13 3->5": (_CONV, _conv3(1, 5, 9, 13, 3, 0, 5, False)),
    "conv3 two sources 16^3 16+16->16": (_CONV + ("vnet_conv_fwd_stats",), _conv3(1, 16, 16, 16, 16, 16, 16, True)),
    "conv3 split-K 8^3 64->64": (_CONV + ("vnet_conv_fwd_stats",), _conv3(1, 8, 8, 8, 64, 0, 64, True)),
    "conv3 4^3 bricks 4^3x2 64->32": (_CONV + ("vnet_conv_fwd_stats",), _conv3(2, 4, 4, 4, 64, 0, 32, True)),
    "conv3 direct filter gradient 32^3 16->16": (_CONV + ("vnet_conv_fwd_stats",), _conv3(1, 32, 32, 32, 16, 0, 16, True)),
}


@pytest.mark.parametrize("cid", sorted(CASES))
def test_unet_guard_bands(dev, cid):
    guard.check_case(CASES, cid, dev, need_output=False)

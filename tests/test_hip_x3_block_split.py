"""-m gpu: the two-cout-block form of the f32x3 convolution kernel (csrc/conv_x3.h, conv5_x3_kernel<STATS, 2, false>) against the
one-block form, bit for bit.

With two 16-cout blocks per item, wave group g takes cout block g of the pair on BOTH z-planes of the brick (one filter fragment set
feeds two plane walks); with one block per item (`X3_NB2 = 0`) group g takes plane g.  Every accumulator still receives the MFMA
sequence it receives in the one-block kernel and the epilogue's association does not move, so the results are `torch.equal` -- outputs,
statistics rows, accumulated outputs and both destinations of a backward-data launch.

Shapes: the smallest at which the plan rule `items * nks >= 2 * grid` (conv_x3.hip) still selects two blocks on a 256-CU part:
Cout = 32 needs 256 bricks of 2 x 8 x 16 (16 x 64 x 64), Cout = 64 needs 128 (32^3).  Each test asserts that rule for the device it
runs on, so a part with more CUs fails loudly instead of comparing the one-block kernel with itself.

A K-split launch (chunks of an item spread over several workgroups, partial slabs + reduce) never takes two blocks: `x3_plan_conv`
stops doubling `nks` as soon as `items * nks >= 256`, which is below `2 * grid`; there is nothing to test there.

One fp64-oracle check of the ragged case at the bound of tests/test_hip_x3.py (2e-6) keeps a fault that both forms share from hiding
behind the comparison."""
import numpy as np
import pytest
import torch

from oracle import vnet_oracle as O
from tests import util
from tests.util import g, check_close

pytestmark = pytest.mark.gpu

RAGGED = (1, 17, 60, 70)          # 9 x 8 x 5 bricks: the last brick in z (one plane), y (4 rows) and x (6 columns) is partial


@pytest.fixture
def split3():
    with util.split3(force=True) as ops:
        yield ops


def _assert_two_blocks(dev, B, D, H, W, Cin, Cout):
    """The launch takes conv5_x3_kernel<S, 2, false> when X3_NB2 = 1: the rule of conv_x3.hip, for this device."""
    from vnet_tensorflow_amd import _lib
    grid = torch.cuda.get_device_properties(dev).multi_processor_count // 8 * 8
    bricks = B * -(-D // 2) * -(-H // 8) * -(-W // 16)
    assert _lib.lib().vnet_conv_x3_ws_bytes(Cin, Cout, B, D, H, W) == 0, "a K-split launch: one block per item"
    assert Cout % 32 == 0 and W >= 16 and bricks * (Cout // 16) >= 2 * grid, ("one block per item on this device", bricks, Cout, grid)


def _with_nb2(fn):
    """fn() with two blocks per item and with one: (results of X3_NB2 = 1, results of X3_NB2 = 0)."""
    from vnet_tensorflow_amd import _lib
    out = []
    try:
        for v in (1, 0):
            _lib.set_option("X3_NB2", v)
            out.append(fn())
    finally:
        _lib.set_option("X3_NB2", 1)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("shape", [
    (1, 16, 64, 64, 16, 0, 32),      # whole bricks, one chunk: each wave group's block on both planes
    (1, 16, 64, 64, 16, 16, 32),     # two sources: the second chunk comes from x1 and runs negated
    (1, 16, 64, 64, 48, 0, 32),      # three chunks: the last one runs negated (`flip` in the epilogue), three rotations of the tap columns
    (2, 8, 64, 64, 32, 0, 32),       # batch 2
    (1, 32, 32, 32, 32, 0, 64),      # Cout = 64: two pairs per brick
    RAGGED + (32, 0, 32),            # partial last bricks, two chunks
])
def test_block_split_equals_plane_split(dev, split3, shape):
    ops = split3
    B, D, H, W, C0, C1, Co = shape
    _assert_two_blocks(dev, B, D, H, W, C0 + C1, Co)
    gen = torch.Generator(device="cpu").manual_seed(sum(shape))
    x0 = torch.randn((B, D, H, W, C0), generator=gen).to(dev)
    x1 = torch.randn((B, D, H, W, C1), generator=gen).to(dev) if C1 else None
    w = (torch.randn((5, 5, 5, C0 + C1, Co), generator=gen) * 0.05).to(dev)
    b = torch.randn(Co, generator=gen).to(dev)
    y2, y1 = _with_nb2(lambda: ops.conv(x0, w, b, 5, 1, x1=x1))
    assert torch.isfinite(y2).all() and float(y2.abs().max()) > 0
    assert torch.equal(y2, y1)


def test_block_split_ragged_against_the_fp64_oracle(dev, split3):
    """The ragged volume, 16 -> 32: bit-equal to the one-block kernel AND within 2e-6 of the fp64 oracle."""
    ops = split3
    B, D, H, W = RAGGED
    C, Co = 16, 32
    _assert_two_blocks(dev, B, D, H, W, C, Co)
    rng = np.random.default_rng(17)
    x = rng.standard_normal((B, D, H, W, C)); w = rng.standard_normal((5, 5, 5, C, Co)) * 0.1; b = rng.standard_normal(Co)
    y_ref = O.conv_nd_fwd(x, w, 1) + b
    tx, tw, tb = g(x, dev), g(w, dev), g(b, dev)
    y2, y1 = _with_nb2(lambda: ops.conv(tx, tw, tb, 5, 1))
    assert torch.equal(y2, y1)
    check_close("x3 block split, ragged 16->32", y2, y_ref, 2e-6)


def test_block_split_epilogue_statistics_accumulate_and_residual(dev, split3):
    """The epilogue on the ragged volume, built as test_hip_x3.py::test_x3_epilogue_statistics_accumulate_and_residual builds it: the
    residual in front of the batch-norm partial sums, the statistics rows themselves, and y += conv -- all bit-equal."""
    ops = split3
    from vnet_tensorflow_amd import _lib
    L = _lib.lib()
    B, D, H, W = RAGGED
    C, Co = 32, 32
    _assert_two_blocks(dev, B, D, H, W, C, Co)
    gen = torch.Generator(device="cpu").manual_seed(29)
    tx = torch.randn((B, D, H, W, C), generator=gen).to(dev)
    tw = (torch.randn((5, 5, 5, C, Co), generator=gen) * 0.1).to(dev)
    tb = torch.randn(Co, generator=gen).to(dev)
    tr = torch.randn((B, D, H, W, Co), generator=gen).to(dev)
    y_old = torch.randn((B, D, H, W, Co), generator=gen).to(dev)
    wp = ops.packed_weights(tw, ops.PACK_FWD_X3, 125, C, Co)
    rows = L.vnet_conv_x3_stats_rows(C, Co, B, D, H, W)
    assert rows == 9 * 8 * 5

    def run():
        stats = torch.full((rows, 2 * Co), float("nan"), device=dev)
        y = torch.empty((B, D, H, W, Co), device=dev)
        ops._conv_x3_call(tx, None, wp, tb, y, None, (D, H, W), stats=stats, res=tr)
        ty = y_old.clone()
        ops._conv_x3_call(tx, None, wp, tb, ty, None, (D, H, W), accum=True)
        return y, stats, ty

    (y2, s2, a2), (y1, s1, a1) = _with_nb2(run)
    assert torch.isfinite(s2).all()
    assert torch.equal(y2, y1)
    assert torch.equal(s2, s1)
    assert torch.equal(a2, a1)
    # (and the rows are the sums they claim to be: of y + res, over the volume)
    v = (y2 + tr).double().reshape(-1, Co)
    np.testing.assert_allclose(s2[:, :Co].double().sum(0).cpu().numpy(), v.sum(0).cpu().numpy(), rtol=0, atol=2e-5 * float(v.abs().sum(0).max()))
    np.testing.assert_allclose(s2[:, Co:].double().sum(0).cpu().numpy(), (v * v).sum(0).cpu().numpy(), rtol=2e-6)


def test_block_split_backward_data_into_two_destinations(dev, split3):
    """The backward-data launch of a (16 + 16) -> 16 layer through autograd: 16 -> 32 with Cy0 = Cy1 = 16, so the block pair of an item
    straddles the two destinations -- wave group 0 stores into dx0, group 1's block into dx1."""
    ops = split3
    B, D, H, W, C0, C1, Co = 1, 32, 32, 64, 16, 16, 16
    _assert_two_blocks(dev, B, D, H, W, Co, C0 + C1)
    gen = torch.Generator(device="cpu").manual_seed(41)
    x0 = torch.randn((B, D, H, W, C0), generator=gen).to(dev)
    x1 = torch.randn((B, D, H, W, C1), generator=gen).to(dev)
    w = (torch.randn((5, 5, 5, C0 + C1, Co), generator=gen) * 0.05).to(dev)
    b = torch.randn(Co, generator=gen).to(dev)
    dy = torch.randn((B, D, H, W, Co), generator=gen).to(dev)

    def run():
        t0, t1 = x0.clone().requires_grad_(True), x1.clone().requires_grad_(True)
        ops.profile_start()
        y = ops.conv(t0, w, b, 5, 1, x1=t1)
        y.backward(dy)
        recs = ops.profile_stop()
        assert sum(1 for r in recs if r[0].startswith("conv-x3")) == 2, [r[0] for r in recs]     # forward and backward-data
        return t0.grad, t1.grad

    (d0, d1), (e0, e1) = _with_nb2(run)
    assert float(d0.abs().max()) > 0 and float(d1.abs().max()) > 0
    assert torch.equal(d0, e0)
    assert torch.equal(d1, e1)

"""-m gpu: guard bands (tests/guard.py) around the two entry points of include/vnet_hip_resample.h, called the way the product
calls them (ops.resample inside guarded(): inputs, the divisor and the outputs are all carved from the arena).  Checked: (a) every guard
byte intact and no input modified, (b) every output element written on the 0xFF pre-fill -- the zeros of the samples outside the source
come from the kernel, not from a memset -- (c) results against the fp64 restatement (vnet_tensorflow_amd/resample.py), (d) bit-identical
results on a 0xFF and a 0x00 pre-fill.  CASES (entry points a case must reach, function) is what the ledger test in
tests/test_abi_ledger.py reads."""
import numpy as np
import pytest
import torch

from tests import guard

pytestmark = pytest.mark.gpu
UP = (0.7 / 0.5, 1.0 / 1.3, 2.5 / 1.0)                     # output spacing / source spacing of a 5x4x3 source
DOWN = tuple(1.0 / r for r in UP)


def _sizes(shape, ratio):
    """The Resample size formula for spacing ratio r: ceil(n / r) voxels."""
    from vnet_tensorflow_amd import resample as R
    return R.output_size(shape, (1.0, 1.0, 1.0), ratio)


def _linear(shape, C, ratio, divisor):
    def run(h):
        from vnet_tensorflow_amd import ops, resample as R
        rng = np.random.default_rng(sum(shape) + 10 * C)
        x = rng.normal(20.0, 30.0, size=tuple(shape) + (C,)).astype(np.float32)
        cnt = rng.integers(1, 9, size=shape).astype(np.float32) if divisor else None
        size = _sizes(shape, ratio)
        y = ops.resample(h.g(x), size, ratio, "linear", divisor=h.g(cnt) if divisor else None)
        ref = R.linear64(x, size, ratio, divisor=cnt)
        assert tuple(y.shape) == size + (C,)
        assert np.abs(y.cpu().numpy().astype(np.float64) - ref).max() <= 2.0 ** -23 * np.abs(x).max()
    return run


def _nearest(shape, ratio):
    def run(h):
        from vnet_tensorflow_amd import ops, resample as R
        lab = np.random.default_rng(sum(shape)).integers(1, 6, size=shape).astype(np.int32)
        size = _sizes(shape, ratio)
        y = ops.resample(h.g(lab, dtype=torch.int32), size, ratio, "nearest")
        assert y.dtype == torch.int32 and np.array_equal(y.cpu().numpy(), R.nearest(lab, size, ratio))
    return run


_LIN, _NEAR = ("vnet_resample_linear",), ("vnet_resample_nearest_i32",)
CASES = {
    "linear up 5x4x3 c4 (quads)": (_LIN, _linear((5, 4, 3), 4, DOWN, False)),
    "linear down 5x4x3 c8 (quads)": (_LIN, _linear((5, 4, 3), 8, UP, False)),
    "linear up 5x4x3 c3 (scalar)": (_LIN, _linear((5, 4, 3), 3, DOWN, False)),
    "linear down 5x4x3 c1 (scalar)": (_LIN, _linear((5, 4, 3), 1, UP, False)),
    "linear up 5x4x3 c4 divisor": (_LIN, _linear((5, 4, 3), 4, DOWN, True)),
    "linear down 5x4x3 c5 divisor": (_LIN, _linear((5, 4, 3), 5, UP, True)),
    "nearest up 5x4x3": (_NEAR, _nearest((5, 4, 3), DOWN)),
    "nearest down 5x4x3": (_NEAR, _nearest((5, 4, 3), UP)),
}


@pytest.mark.parametrize("cid", sorted(CASES))
def test_resample_guard_bands(dev, cid):
    guard.check_case(CASES, cid, dev, capacity=32 << 20)

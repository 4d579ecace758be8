"""-m gpu: guard bands (tests/guard.py) around the two entry points of include/vnet_hip_deform.h, called the way the product
calls them (ops.bspline_deform inside guarded(): the volume, the coefficient table and the output are all carved from the arena).
Checked: (a) every guard byte intact and no input modified, (b) every output element written on the 0xFF pre-fill -- the zeros of the
samples that leave the volume come from the kernel, not from a memset -- (c) results against the fp64 restatement
(vnet_tensorflow_amd/deform.py), (d) bit-identical results on a 0xFF and a 0x00 pre-fill.  CASES (entry points a case must reach,
function) is what the ledger test in tests/test_abi_ledger.py reads."""
import numpy as np
import pytest
import torch

from tests import guard

pytestmark = pytest.mark.gpu
SHAPE = (13, 10, 7)
SPACING = (1.0, 0.8, 1.25)


def _inputs(C, randomness):
    rng = np.random.default_rng(100 + 10 * C + int(randomness))
    x = rng.normal(20.0, 30.0, size=SHAPE + (C,)).astype(np.float32)
    lab = rng.integers(1, 6, size=SHAPE).astype(np.int32)        # (no zero in the input: a zero in the output is the default value)
    return x, lab, rng.random(3 * 13 ** 3) * randomness


def _image(C, randomness):
    def run(h):
        from vnet_tensorflow_amd import deform as D, ops
        x, _, coef = _inputs(C, randomness)
        y = ops.bspline_deform(h.g(x), h.g(coef, dtype=torch.float64), SPACING, "image")
        assert tuple(y.shape) == x.shape and y.dtype == torch.float32
        assert np.abs(y.cpu().numpy().astype(np.float64) - D.linear64(x, coef, SPACING)).max() <= (2.0 ** -23 + 6e-12) * np.abs(x).max()
    return run


def _label(randomness):
    def run(h):
        from vnet_tensorflow_amd import deform as D, ops
        _, lab, coef = _inputs(1, randomness)
        assert int(D.undecidable(SHAPE, SPACING, coef).sum()) == 0
        y = ops.bspline_deform(h.g(lab, dtype=torch.int32), h.g(coef, dtype=torch.float64), SPACING, "label")
        assert y.dtype == torch.int32 and np.array_equal(y.cpu().numpy(), D.label(lab, coef, SPACING))
    return run


_F32, _I32 = ("vnet_bspline_deform_f32",), ("vnet_bspline_deform_i32",)
CASES = {
    "image 13x10x7 c1 (scalar) r1.5": (_F32, _image(1, 1.5)),
    "image 13x10x7 c3 (scalar) r10": (_F32, _image(3, 10)),
    "image 13x10x7 c4 (quads) r1.5": (_F32, _image(4, 1.5)),
    "image 13x10x7 c4 (quads) r10": (_F32, _image(4, 10)),
    "label 13x10x7 r1.5": (_I32, _label(1.5)),
    "label 13x10x7 r10": (_I32, _label(10)),
}


@pytest.mark.parametrize("cid", sorted(CASES))
def test_deform_guard_bands(dev, cid):
    guard.check_case(CASES, cid, dev, capacity=32 << 20)

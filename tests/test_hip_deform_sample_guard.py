"""-m gpu: guard bands (tests/guard.py) around the entry point of include/vnet_hip_deform_sample.h, called the way the product
calls it (ops.bspline_deform of the label, then ops.deform_sample_patch, inside guarded(): the case, the coefficient table, the deformed
label and both slots are all carved from the arena).  Checked: (a) every guard byte intact and no input modified -- the gather reads the
resident image wherever a voxel's source position falls, never past it --, (b) every element of both slots written on the 0xFF pre-fill
(NaN / -1 poison): the zeros of the samples that leave the volume come from the kernel, (c) results against the windowed restatement
(vnet_tensorflow_amd/sample.py: deform_patch), (d) bit-identical results on a 0xFF and a 0x00 pre-fill.  CASES (entry points a case must
reach, function) is what the ledger test in tests/test_abi_ledger.py reads."""
import numpy as np
import pytest
import torch

from tests import guard

pytestmark = pytest.mark.gpu
SHAPE, SPACING, PATCH = (21, 18, 23), (1.0, 0.8, 1.25), (8, 6, 10)
SEED = 0xC0FFEE123456789


def _sample(C, start, patch, flip, sigma, coef_seed):
    def run(h):
        from vnet_tensorflow_amd import deform as D, ops, sample as S
        rng = np.random.default_rng(60 + C)
        img = rng.normal(100.0, 40.0, SHAPE + (C,)).astype(np.float32)
        lab = (rng.random(SHAPE) < 0.5).astype(np.int32)
        coef = np.random.default_rng(coef_seed).random(D.PARAMS) * 6.0
        assert not D.undecidable(SHAPE, SPACING, coef).any()
        dc = h.g(coef, dtype=torch.float64)
        yl = ops.bspline_deform(h.g(lab, dtype=torch.int32), dc, SPACING, "label")
        oi = h.arena.tensor("slot.image", tuple(patch) + (C,), torch.float32, "out")
        ol = h.arena.tensor("slot.label", tuple(patch) + (1,), torch.int32, "out")
        ops.deform_sample_patch(h.g(img), yl, dc, SPACING, start, patch, flip, sigma, SEED, oi, ol)
        ri, rl = S.deform_patch(img, lab, coef, SPACING, start, patch, flip, sigma, SEED)
        got = oi.cpu().numpy()
        assert np.array_equal(ol.cpu().numpy()[..., 0], rl) and set(np.unique(rl)) <= {0, 1}
        y64 = np.flip(D.linear64(img, coef, SPACING, (start, patch)), S.flip_axes(flip))
        # some voxels of the window sample inside the volume and -- the shifts are positive, so not from the window at the origin -- some
        # leave it: their zeros are written by the kernel
        assert (y64 != 0).any() and ((y64 == 0).any() or tuple(start) == (0, 0, 0) and tuple(patch) != SHAPE)
        bound = (2.0 ** -23 + 6e-12) * np.abs(img).max()
        if sigma == 0:
            assert np.abs(got.astype(np.float64) - y64).max() <= bound
        else:
            assert (np.abs(got.astype(np.float64) - ri) <= bound + 1e-5 * sigma + 2.0 ** -23 * np.abs(ri)).all()
    return run


_E = ("vnet_bspline_deform_i32", "vnet_deform_sample_patch")
FAR = tuple(n - p for n, p in zip(SHAPE, PATCH))
CASES = {
    "c1 (scalar) origin": (_E, _sample(1, (0, 0, 0), PATCH, 0, 0.0, 0)),
    "c3 (scalar) far corner flip5 noise": (_E, _sample(3, FAR, PATCH, 5, 5.0, 1)),
    "c4 (quads) mixed corner flip2": (_E, _sample(4, (FAR[0], 0, 5), PATCH, 2, 0.0, 2)),
    "c4 (quads) far corner flip7 noise": (_E, _sample(4, FAR, PATCH, 7, 5.0, 3)),
    "c8 (quads) whole volume flip3": (_E, _sample(8, (0, 0, 0), SHAPE, 3, 0.0, 4)),
}


@pytest.mark.parametrize("cid", sorted(CASES))
def test_deform_sample_guard_bands(dev, cid):
    guard.check_case(CASES, cid, dev, capacity=32 << 20)

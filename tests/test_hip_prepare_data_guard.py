"""-m gpu: guard bands (tests/guard.py) around the five entry points of csrc/vnet_tools.h, called the way the product calls them (the
ops of vnet_tensorflow_amd/morph.py inside guarded(arena, modules=(morph,)): inputs and outputs are carved from the arena; there is
no scratch).  Checked: (a) every guard byte intact and no input modified, (b) every output byte written, (c) results against the NumPy
rules (vnet_tensorflow_amd/prepare_data.py), (d) bit-identical results on a 0xFF and a 0x00 pre-fill of the outputs, (e) a case calls
its own entry point and no other.
On (b): an output element that is legitimately all 0xFF reads as "never written" (tests/test_hip_bbox_guard.py explains).  The cases keep
their outputs off it: no mask word here has all 64 bits set (sparse masks, rows of 65 voxels or of one), the box of a non-empty mask
holds no -1, the cropped int16 values are small and positive, unpacked bytes are 0 / 1.
CASES (entry points a case must reach, function) is what the ledger test in tests/test_abi_ledger.py reads."""
import numpy as np
import pytest
import torch

from tests import guard
from vnet_tensorflow_amd import morph, prepare_data as P

pytestmark = pytest.mark.gpu
SHAPES = {"5x7x65": (5, 7, 65), "1x1x1": (1, 1, 1)}


def _mask(shape):
    m = (np.random.default_rng(3).random(shape) < 0.05).astype(np.uint8)
    m[-1, -1, -1] = 1
    return m


def _select(shape):
    def run(h):
        label = np.random.default_rng(1).integers(0, 4, size=shape).astype(np.uint8)
        label[-1, -1, -1] = 2
        got = morph.select_bits(h.g(label, dtype=torch.uint8), [2, 3])
        assert np.array_equal(got.cpu().numpy(), P.pack_bits(P.select(label, [2, 3])))
        assert set(h.calls) == {"vnet_select_bits"}
    return run


def _dilate(shape):
    def run(h):
        m = np.zeros(shape, np.uint8)                      # two voxels: no dilated word has all 64 bits set, at either radius
        m[0, 0, 0] = m[-1, -1, -1] = 1
        for r in (1, 5):
            got = morph.dilate_bits(h.g(P.pack_bits(m), dtype=torch.int64), shape[2], r)
            assert np.array_equal(got.cpu().numpy(), P.pack_bits(P.dilate(m, r)))
        assert set(h.calls) == {"vnet_dilate_bits"}
    return run


def _bbox(shape):
    def run(h):
        m = _mask(shape)
        assert morph.bits_bbox(h.g(P.pack_bits(m), dtype=torch.int64), shape[2]) == (int(m.sum()),) + P.bounding_box(m)
        assert set(h.calls) == {"vnet_bits_bbox"}
    return run


def _crop(shape):
    def run(h):
        m = _mask(shape)
        src = np.random.default_rng(2).integers(1, 1000, size=shape).astype(np.int16)
        start = tuple(n // 3 for n in shape)
        size = tuple(n - s for n, s in zip(shape, start))
        w = tuple(slice(s, None) for s in start)
        t = h.g(src, dtype=torch.int16)
        got = morph.masked_crop(t, h.g(P.pack_bits(m), dtype=torch.int64), start, size)
        assert np.array_equal(got.cpu().numpy(), np.where(m != 0, src, 0)[w])
        assert np.array_equal(morph.masked_crop(t, None, start, size).cpu().numpy(), src[w])
        assert set(h.calls) == {"vnet_masked_crop"}
    return run


def _unpack(shape):
    def run(h):
        m = _mask(shape)
        assert np.array_equal(morph.unpack_bits(h.g(P.pack_bits(m), dtype=torch.int64), shape[2]).cpu().numpy(), m)
        assert set(h.calls) == {"vnet_unpack_bits"}
    return run


CASES = {}
for _name, _shape in SHAPES.items():
    CASES["select " + _name] = (("vnet_select_bits",), _select(_shape))
    CASES["dilate " + _name] = (("vnet_dilate_bits",), _dilate(_shape))
    CASES["bbox " + _name] = (("vnet_bits_bbox",), _bbox(_shape))
    CASES["crop " + _name] = (("vnet_masked_crop",), _crop(_shape))
    CASES["unpack " + _name] = (("vnet_unpack_bits",), _unpack(_shape))


@pytest.mark.parametrize("cid", sorted(CASES))
def test_prepare_data_guard_bands(dev, cid):
    guard.check_case(CASES, cid, dev, capacity=32 << 20, modules=(morph,))

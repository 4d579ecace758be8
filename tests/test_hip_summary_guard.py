"""-m gpu: guard bands (tests/guard.py) around the four entry points of include/vnet_hip_summary.h, called the way the product
calls them (ops.summary_slices_* inside guarded(): the input and the output are carved from the arena; there is no scratch).  Checked:
(a) every guard byte intact and no input modified, (b) every output byte written, (c) results against the NumPy restatements
(vnet_tensorflow_amd/summary.py), (d) bit-identical results on a 0xFF and a 0x00 pre-fill of the outputs.
On (b): an output byte here may legitimately be 0xFF, which arena.check_written() reads as "never written".  The intensity and index
cases keep their inputs off it (values below 255; factor 63 on classes 0 .. 3) and run check_written(); a rainbow pixel always has one
saturated channel (S = V = 1), so those cases rest on (c) under BOTH pre-fills -- a byte the kernel skipped would hold 0xFF in one run
and 0x00 in the other and cannot equal the restatement twice.
CASES (entry points a case must reach, function) is what the ledger test in tests/test_abi_ledger.py reads."""
import numpy as np
import pytest
import torch

from tests import guard

pytestmark = pytest.mark.gpu
SMALL, RAGGED, ONE = (2, 5, 7, 3, 3), (1, 33, 17, 65, 1), (1, 1, 1, 1, 1)


def _intensity(shape):
    def run(h):
        from vnet_tensorflow_amd import ops, summary as S
        x = (np.random.default_rng(1).random(shape, dtype=np.float32) * np.float32(260) - np.float32(5)).astype(np.float32)
        x = np.where(x >= 255, np.float32(254.5), x)                          # (no output byte 0xFF: see the module docstring)
        x.flat[0] = np.nan
        got = ops.summary_slices_intensity(h.g(x))
        assert np.array_equal(got.cpu().numpy(), S.slices_intensity(x)) and h.ws_requests == []
        return True
    return run


def _index(shape, dtype):
    def run(h):
        from vnet_tensorflow_amd import ops, summary as S
        npd = np.int32 if dtype == torch.int32 else np.int64
        x = np.random.default_rng(2).integers(0, 4, shape).astype(npd)
        got = ops.summary_slices_index(h.g(x, dtype=dtype), 63)
        assert np.array_equal(got.cpu().numpy(), S.slices_index(x, 63)) and h.ws_requests == []
        return True
    return run


def _rainbow(shape):
    def run(h):
        from vnet_tensorflow_amd import ops, summary as S
        x = np.random.default_rng(3).random(shape, dtype=np.float32)
        got = ops.summary_slices_rainbow(h.g(x))
        assert np.array_equal(got.cpu().numpy(), S.slices_rainbow(x)) and h.ws_requests == []
        return False
    return run


_F, _I32, _I64, _R = ("vnet_summary_slices_f32",), ("vnet_summary_slices_i32",), ("vnet_summary_slices_i64",), ("vnet_summary_rainbow_f32",)
CASES = {}
for _name, _shape in (("2x5x7x3x3", SMALL), ("1x33x17x65x1", RAGGED), ("1x1x1x1x1", ONE)):
    CASES["intensity " + _name] = (_F, _intensity(_shape))
    CASES["index i32 " + _name] = (_I32, _index(_shape, torch.int32))
    CASES["index i64 " + _name] = (_I64, _index(_shape, torch.int64))
    CASES["rainbow " + _name] = (_R, _rainbow(_shape))


@pytest.mark.parametrize("cid", sorted(CASES))
def test_summary_guard_bands(dev, cid):
    guard.check_case(CASES, cid, dev, capacity=48 << 20, written=guard.written_if_returned)

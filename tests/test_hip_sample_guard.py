"""-m gpu: guard bands (tests/guard.py) around the three entry points of include/vnet_hip_sample.h, called the way the product
calls them (ops.component_table / window_count / sample_patch inside guarded(): inputs, outputs and scratch are all carved from the arena,
the scratch of EXACTLY the queried size).  Checked: (a) every guard byte intact and no input modified, (b) every output element written
on the 0xFF pre-fill -- the zero rows past n, the two sums and every voxel of both slots come from a kernel, not from a memset --
(c) results against the NumPy restatements (vnet_tensorflow_amd/sample.py), (d) bit-identical results on a 0xFF and a 0x00 pre-fill of
outputs and scratch.  CASES (entry points a case must reach, function) is what the ledger test in tests/test_abi_ledger.py reads."""
import numpy as np
import pytest
import torch

from tests import guard

pytestmark = pytest.mark.gpu
NOISY, VOLUME, PATCH = (33, 31, 37), (40, 36, 44), (16, 12, 20)


def _noisy():
    return (np.random.default_rng(3).random(NOISY) < 0.35).astype(np.int32) * 2


def _table(cap):
    def run(h):
        from vnet_tensorflow_amd import _lib, ops, sample as S
        lab = _noisy()
        n, rows = ops.component_table(h.g(lab, dtype=torch.int32), cap)
        rn, rrows = S.component_table(lab)
        assert n == rn and n > 1000 and np.array_equal(rows, rrows[:cap])
        assert h.ws_requests == [_lib.lib().vnet_cc_table_ws_bytes(*NOISY)] and h.ws_requests[0] == 8 * lab.size + 4 * 4096
        # the rows past n (capacity above n) or none at all (capacity below): read the whole device table
        out = [e for e in h.arena.entries if e.role == "out"][-1].tensor.cpu().numpy()
        assert out[-1] == n and not out[min(n, cap) * 8:-1].any()
    return run


def _labels(shape, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < 0.3, rng.integers(1, 300, size=shape), 0).astype(np.int32)


def _window(start, size):
    def run(h):
        from vnet_tensorflow_amd import ops, sample as S
        lab = _labels(VOLUME, 8)
        assert ops.window_count(h.g(lab, dtype=torch.int32), start, size, 1, 255) == S.window_count(lab, start, size, 1, 255)
    return run


def _sample(C, flip, sigma):
    def run(h):
        from vnet_tensorflow_amd import ops, sample as S
        rng = np.random.default_rng(40 + C)
        img, lab = rng.normal(100.0, 40.0, VOLUME + (C,)).astype(np.float32), _labels(VOLUME, 9) + 1      # (no zero: a zero is unwritten)
        start = (VOLUME[0] - PATCH[0], 0, 7)
        oi = h.arena.tensor("slot.image", PATCH + (C,), torch.float32, "out")
        ol = h.arena.tensor("slot.label", PATCH + (1,), torch.int32, "out")
        ops.sample_patch(h.g(img), h.g(lab, dtype=torch.int32), start, PATCH, flip, sigma, 0xC0FFEE123456789, oi, ol)
        ri, rl = S.patch(img, lab, start, PATCH, flip, sigma, 0xC0FFEE123456789)
        got = oi.cpu().numpy()
        assert np.array_equal(ol.cpu().numpy()[..., 0], rl)
        if sigma == 0:
            assert np.array_equal(got, ri)
        else:
            assert (np.abs(got.astype(np.float64) - ri) <= 1e-5 * sigma + 2.0 ** -23 * np.abs(ri)).all()
    return run


_T, _W, _S = ("vnet_cc_table",), ("vnet_window_count",), ("vnet_sample_patch",)
CASES = {
    "table 33x31x37 p0.35 cap4096": (_T, _table(4096)),
    "table 33x31x37 p0.35 cap16": (_T, _table(16)),
    "window 40x36x44 whole": (_W, _window((0, 0, 0), VOLUME)),
    "window 40x36x44 high corner": (_W, _window((24, 24, 24), (16, 12, 20))),
    "sample c1 (scalar) crop": (_S, _sample(1, 0, 0.0)),
    "sample c3 (scalar) flip5 noise": (_S, _sample(3, 5, 5.0)),
    "sample c4 (quads) flip2 crop": (_S, _sample(4, 2, 0.0)),
    "sample c4 (quads) flip7 noise": (_S, _sample(4, 7, 5.0)),
}


@pytest.mark.parametrize("cid", sorted(CASES))
def test_sample_guard_bands(dev, cid):
    guard.check_case(CASES, cid, dev, capacity=48 << 20)

"""-m gpu: guard bands (tests/guard.py) around the two pointer-taking entry points of include/vnet_hip_score.h, called the way
the product calls them (ops.label_overlap / ops.component_shapes inside guarded(): inputs, outputs and scratch are all carved from the
arena, the scratch of EXACTLY the queried size).  Checked: (a) every guard byte intact and no input modified, (b) every output element
written on the 0xFF pre-fill -- the count table, the zero rows and zero sums past n come from a kernel, not from a memset --, (c) results
against the NumPy restatements (vnet_tensorflow_amd/score.py), (d) bit-identical results on a 0xFF and a 0x00 pre-fill of outputs and
scratch.  CASES (entry points a case must reach, function) is what the ledger test in tests/test_abi_ledger.py reads."""
import numpy as np
import pytest
import torch

from tests import guard

pytestmark = pytest.mark.gpu
SMALL, RAGGED = (5, 7, 9), (33, 17, 65)


def _overlap(shape, L):
    def run(h):
        from vnet_tensorflow_amd import ops, score as S
        rng = np.random.default_rng(L + shape[0])
        a = rng.integers(-1, L + 1, size=shape).astype(np.int32)
        b = np.where(rng.random(shape) < 0.6, a, rng.integers(-1, L + 1, size=shape)).astype(np.int32)
        a[0, 0, :3], b[0, 0, :3] = (-1, L, 0), (L, L, -5)
        got = ops.label_overlap(h.g(a, dtype=torch.int32), h.g(b, dtype=torch.int32), L)
        assert got.dtype == np.int64 and np.array_equal(got, S.label_overlap(a, b, L))
        assert got[L, 1] > 0 and got[L, 2] > 0 and h.ws_requests == []
    return run


def _shape(shape, density, cap):
    def run(h):
        from vnet_tensorflow_amd import _lib, ops, score as S
        lab = (np.random.default_rng(3).random(shape) < density).astype(np.int32) * 2
        n, rows, sums = ops.component_shapes(h.g(lab, dtype=torch.int32), cap)
        rn, rrows, rsums = S.component_shapes(lab, cap)
        assert n == rn and n > cap // 64 and np.array_equal(rows, rrows) and np.array_equal(sums, rsums) and sums.dtype == np.int64
        assert h.ws_requests == [_lib.lib().vnet_cc_shape_ws_bytes(*shape)] and h.ws_requests[0] == 8 * lab.size + 4 * 4096
        # the rows and sums past n (capacity above n) or none at all (capacity below): read the whole device tensors
        outs = [e for e in h.arena.entries if e.role == "out"]
        table, dsums = outs[-2].tensor.cpu().numpy(), outs[-1].tensor.cpu().numpy()
        m = min(n, cap)
        assert table[-1] == n and not table[m * 8:-1].any() and dsums.shape == (cap, 3) and not dsums[m:].any()
    return run


_O, _C = ("vnet_label_overlap",), ("vnet_cc_shape",)
CASES = {
    "overlap 5x7x9 L2": (_O, _overlap(SMALL, 2)),
    "overlap 5x7x9 L1024": (_O, _overlap(SMALL, 1024)),
    "overlap 33x17x65 L5": (_O, _overlap(RAGGED, 5)),
    "shape 5x7x9 p0.35 cap64": (_C, _shape(SMALL, 0.35, 64)),
    "shape 33x17x65 p0.35 cap4096": (_C, _shape(RAGGED, 0.35, 4096)),
    "shape 33x17x65 p0.35 cap16": (_C, _shape(RAGGED, 0.35, 16)),
}


@pytest.mark.parametrize("cid", sorted(CASES))
def test_score_guard_bands(dev, cid):
    guard.check_case(CASES, cid, dev, capacity=48 << 20)

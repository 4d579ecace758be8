"""-m gpu: guard bands (tests/guard.py) around the five pointer-taking entry points of csrc/vnet_surface.h, called the way the product
calls them (the ops of vnet_tensorflow_amd/surface.py inside guarded(arena, modules=(surface,)): inputs, outputs and scratch of
EXACTLY the queried size are carved from the arena).  Checked: (a) every guard byte intact and no input modified, (b) every output
byte written, (c) results against the NumPy rules (vnet_tensorflow_amd/score.py), (d) bit-identical results on a 0xFF and a 0x00
pre-fill of outputs and scratch, (e) a case calls its own entry point and no other.
On (b): an output element that is legitimately all 0xFF reads as "never written" (tests/test_hip_bbox_guard.py explains).  None occurs
here: no mask word has all 64 bits set (rows of 65 voxels or of one: the high bits are 0; the surfaces are sparse), a squared distance is
never a NaN pattern (+inf is 0x7FF0...), counts are >= 0, the selected elements and the sums are finite or +inf.
CASES (entry points a case must reach, function) is what the ledger test in tests/test_abi_ledger.py reads."""
import numpy as np
import pytest
import torch

from tests import guard
from vnet_tensorflow_amd import score as SC, surface

pytestmark = pytest.mark.gpu
SHAPES = {"5x7x65": (5, 7, 65), "1x1x1": (1, 1, 1)}
SP = (0.7, 0.7, 2.5)


def _mask(shape):
    m = np.random.default_rng(3).random(shape) < 0.05
    m[-1, -1, -1] = True
    return m


def _bits(shape):
    def run(h):
        label = np.random.default_rng(1).integers(0, 3, size=shape).astype(np.int32)
        label[-1, -1, -1] = 2
        t = h.g(label, dtype=torch.int32)
        for klass in (0, 2):
            assert np.array_equal(surface.surface_bits(t, klass).cpu().numpy(), SC.pack(SC.surface_mask(label, klass)))
        assert set(h.calls) == {"vnet_surface_bits"}
    return run


def _edt2(shape):
    def run(h):
        m = _mask(shape)
        got = surface.edt2(h.g(SC.pack(m), dtype=torch.int64), shape[2], SP)
        assert h.ws_requests == [12 * m.size + (4 * m.size) % 8]
        assert np.array_equal(got.cpu().numpy(), SC.edt2(m, SP))
        assert set(h.calls) == {"vnet_edt2"}
    return run


def _gather(shape):
    def run(h):
        m = _mask(shape)
        d2 = np.random.default_rng(2).random(shape) + 1.0
        want = SC.gather(d2, m)
        t, bits = h.g(d2, dtype=torch.float64), h.g(SC.pack(m), dtype=torch.int64)
        got, n = surface.gather(t, bits, shape[2])
        assert int(n) == len(want) and np.array_equal(got.cpu().numpy(), want)
        for cap in (max(1, len(want) - 2), len(want) + 3):                 # below n: the rest is dropped; above n: zeroed from n up
            out = surface.empty_list(cap, t.device)
            _, n = surface.gather(t, bits, shape[2], out=out)
            assert int(n) == len(want) and np.array_equal(out.cpu().numpy(), np.concatenate([want[:cap], np.zeros(max(0, cap - len(want)))]))
        assert set(h.calls) == {"vnet_surface_gather"}                     # (popcounts sizes the first list through it as well)
    return run


def _list(shape):
    v = np.random.default_rng(4).integers(0, 9, size=int(np.prod(shape)) + 2).astype(np.float64) * 0.49
    v[0] = np.inf
    return v


def _select(shape):
    def run(h):
        v = _list(shape)
        ranks = [0, len(v) - 1, SC.hd95_rank(len(v))]
        assert np.array_equal(surface.kth(h.g(v, dtype=torch.float64), ranks).cpu().numpy(), SC.kth(v, ranks))
        assert set(h.calls) == {"vnet_list_select"}
    return run


def _root_sum(shape):
    def run(h):
        v = _list(shape)[1:]
        got, want = surface.root_sum(h.g(v, dtype=torch.float64)).item(), np.sqrt(v).sum()
        assert abs(got - want) <= (len(v) + 2) * 2.0 ** -52 * want
        assert set(h.calls) == {"vnet_list_root_sum"}
    return run


CASES = {}
for _name, _shape in SHAPES.items():
    CASES["bits " + _name] = (("vnet_surface_bits",), _bits(_shape))
    CASES["edt2 " + _name] = (("vnet_edt2",), _edt2(_shape))
    CASES["gather " + _name] = (("vnet_surface_gather",), _gather(_shape))
    CASES["select " + _name] = (("vnet_list_select",), _select(_shape))
    CASES["root sum " + _name] = (("vnet_list_root_sum",), _root_sum(_shape))


@pytest.mark.parametrize("cid", sorted(CASES))
def test_surface_guard_bands(dev, cid):
    guard.check_case(CASES, cid, dev, capacity=64 << 20, modules=(surface,))

"""-m gpu: guard bands (tests/guard.py) around the pointer-taking entry points of csrc/vnet_bbox.h, called the way the
product calls them (ops.slice_stack / ops.plane_component_table / ops.bbox_render inside guarded(): inputs, outputs and scratch are
carved from the arena).  Checked: (a) every guard byte intact and no input modified, (b) every output byte written, (c) results
against the NumPy rules (vnet_tensorflow_amd/bounding_box.py), (d) scratch of exactly the queried size, (e) bit-identical results on a
0xFF and a 0x00 pre-fill of outputs and scratch.
On (b): an output element may legitimately be all 0xFF, which arena.check_written() reads as "never written".  The stack cases keep
their inputs off it (finite floats, labels >= 0) and the table holds no -1, so they run check_written(); a rendered byte is 255 wherever
the grey saturates or a colour channel is full, so the render cases rest on (c) under BOTH pre-fills -- a byte the kernel skipped
would hold 0xFF in one run and 0x00 in the other and cannot equal the rule twice.
CASES (entry points a case must reach, function) is what the ledger test in tests/test_abi_ledger.py reads."""
import numpy as np
import pytest
import torch

from tests import guard

pytestmark = pytest.mark.gpu
SMALL, RAGGED, ONE = (5, 7, 9), (33, 65, 17), (1, 1, 1)


def _label(shape, seed):
    return np.random.default_rng(seed).choice(4, size=shape, p=(0.4, 0.2, 0.2, 0.2)).astype(np.int32)


def _stack(shape, dtype):
    def run(h):
        from vnet_tensorflow_amd import bounding_box as B, ops
        x = np.random.default_rng(1).standard_normal(shape).astype(np.float32) if dtype == torch.float32 else _label(shape, 2)
        t = h.g(x, dtype=dtype)
        for axis in (0, 1, 2):
            got = ops.slice_stack(t, axis)
            assert np.array_equal(got.cpu().numpy(), B.stack(x, axis))
        assert h.ws_requests == []
        return True
    return run


def _table(shape):
    def run(h):
        from vnet_tensorflow_amd import _lib, bounding_box as B, ops
        stk = _label(shape, 3)
        want_n, want = B.plane_components(stk)
        n, rows, classes = ops.plane_component_table(h.g(stk, dtype=torch.int32), max_components=max(want_n, 1))
        assert n == want_n and np.array_equal(rows, want) and np.array_equal(classes, stk.reshape(-1)[want[:, 0]])
        assert h.ws_requests == [_lib.lib().vnet_plane_cc_table_ws_bytes(*shape)]          # scratch of exactly the queried size
        return True
    return run


def _render(shape):
    def run(h):
        from vnet_tensorflow_amd import bounding_box as B, ops
        rng = np.random.default_rng(4)
        label = _label(shape, 5)
        image = (rng.standard_normal(shape) * 700).astype(np.float32)
        image.flat[0] = np.nan
        boxes = B.slice_boxes(label)
        flat, first = B.box_arrays(boxes, shape[0])
        got = ops.bbox_render(h.g(image), h.g(label, dtype=torch.int32), h.g(flat, dtype=torch.int32), h.g(first, dtype=torch.int32),
                              -1024, 1024, 0.37)
        assert np.array_equal(got.cpu().numpy(), B.render(image, label, boxes, -1024, 1024, 0.37)) and h.ws_requests == []
        return False
    return run


_F, _I, _T, _R = ("vnet_slice_stack_f32",), ("vnet_slice_stack_i32",), ("vnet_plane_cc_table",), ("vnet_bbox_render",)
CASES = {}
for _name, _shape in (("5x7x9", SMALL), ("33x65x17", RAGGED), ("1x1x1", ONE)):
    CASES["stack f32 " + _name] = (_F, _stack(_shape, torch.float32))
    CASES["stack i32 " + _name] = (_I, _stack(_shape, torch.int32))
    CASES["table " + _name] = (_T, _table(_shape))
    CASES["render " + _name] = (_R, _render(_shape))


@pytest.mark.parametrize("cid", sorted(CASES))
def test_bbox_guard_bands(dev, cid):
    guard.check_case(CASES, cid, dev, capacity=64 << 20, written=guard.written_if_returned)

"""-m gpu: guard bands (tests/guard.py) around the five entry points of csrc/vnet_tools.h (libvnet_tools.so), called the way the
product calls them (the ops of vnet_tensorflow_amd/morph.py inside guarded(arena, modules=(morph,)): inputs and outputs are carved
from the arena; there is no scratch).  guard.run_case passes no modules and records libvnet_hip.so only, so the runner below does
its work for this library: morph.lib is wrapped to record the entry points called and to require every device pointer inside the arena.
Checked: (a) every guard byte intact and no input modified, (b) every output byte written, (c) results against the NumPy rules
(vnet_tensorflow_amd/prepare_data.py), (d) bit-identical results on a 0xFF and a 0x00 pre-fill of the outputs.
On (b): an output element that is legitimately all 0xFF reads as "never written" (tests/test_hip_bbox_guard.py explains).  The cases keep
their outputs off it: no mask word here has all 64 bits set (sparse masks, rows of 65 voxels or of one), the box of a non-empty mask
holds no -1, the cropped int16 values are small and positive, unpacked bytes are 0 / 1."""
import os

import numpy as np
import pytest
import torch

from tests import guard
from vnet_tensorflow_amd import morph, prepare_data as P

pytestmark = pytest.mark.gpu
SHAPES = {"5x7x65": (5, 7, 65), "1x1x1": (1, 1, 1)}
HOST_POINTERS = {("vnet_select_bits", "values")}


class _Recording(object):
    """Stands in for morph.lib(): records the entry points called; a device pointer outside the arena is an error."""

    def __init__(self, real, arena, calls):
        table = guard.pointer_entry_points(os.path.join(guard.ROOT, morph.HEADER))
        self.__dict__.update(_real=real, _arena=arena, _calls=calls, _table=table)

    def __getattr__(self, name):
        fn, params = getattr(self._real, name), self._table[name]

        def call(*args):
            self._calls.append(name)
            for (pname, ptr, _const, _typ), a in zip(params, args):
                if not ptr or pname == "stream" or (name, pname) in HOST_POINTERS or a is None:
                    continue
                if self._arena.find(a) is None:
                    raise guard.GuardError("%s: argument `%s` (0x%x) is not a tensor of the arena" % (name, pname, a))
            return fn(*args)
        return call


def _run(fn, dev, poison):
    """fn(h) inside a guarded arena pre-filled with `poison` -> (snapshot, entry points called)."""
    arena = guard.Arena(dev, capacity=32 << 20, poison=poison)
    calls = []
    real = morph.lib
    with guard.guarded(arena, modules=(morph,)) as h:
        rec = _Recording(real(), arena, calls)
        morph.lib = lambda: rec
        try:
            fn(h)
        finally:
            morph.lib = real
        arena.check()
        if poison == guard.GUARD:
            arena.check_written()
    return arena.snapshot(), calls


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
    return run


def _dilate(shape):
    def run(h):
        m = np.zeros(shape, np.uint8)                      # two voxels: no dilated word has all 64 bits set, at either radius
        m[0, 0, 0] = m[-1, -1, -1] = 1
        for r in (1, 5):
            got = morph.dilate_bits(h.g(P.pack_bits(m), dtype=torch.int64), shape[2], r)
            assert np.array_equal(got.cpu().numpy(), P.pack_bits(P.dilate(m, r)))
    return run


def _bbox(shape):
    def run(h):
        m = _mask(shape)
        assert morph.bits_bbox(h.g(P.pack_bits(m), dtype=torch.int64), shape[2]) == (int(m.sum()),) + P.bounding_box(m)
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
    return run


def _unpack(shape):
    def run(h):
        m = _mask(shape)
        assert np.array_equal(morph.unpack_bits(h.g(P.pack_bits(m), dtype=torch.int64), shape[2]).cpu().numpy(), m)
    return run


CASES = {}
for _name, _shape in SHAPES.items():
    CASES["select " + _name] = ("vnet_select_bits", _select(_shape))
    CASES["dilate " + _name] = ("vnet_dilate_bits", _dilate(_shape))
    CASES["bbox " + _name] = ("vnet_bits_bbox", _bbox(_shape))
    CASES["crop " + _name] = ("vnet_masked_crop", _crop(_shape))
    CASES["unpack " + _name] = ("vnet_unpack_bits", _unpack(_shape))


def test_every_entry_point_of_the_header_has_a_case():
    declared = set(guard.pointer_entry_points(os.path.join(guard.ROOT, morph.HEADER)))
    assert declared == set(morph.SIGNATURES_TOOLS) == {entry for entry, _ in CASES.values()}


@pytest.mark.parametrize("cid", sorted(CASES))
def test_prepare_data_guard_bands(dev, cid):
    entry, fn = CASES[cid]
    snap_ff, calls = _run(fn, dev, guard.GUARD)
    assert calls and set(calls) == {entry}, (cid, calls)
    assert snap_ff, "no output was carved from the arena"
    snap_00, _ = _run(fn, dev, 0x00)
    guard.assert_same_bits(snap_ff, snap_00)

"""-m gpu: guard bands (tests/guard.py) around the five pointer-taking entry points of csrc/vnet_post.h (libvnet_post.so), called the
way the product calls them (the ops of vnet_tensorflow_amd/postprocess.py inside guarded(arena, modules=(postprocess, morph)): inputs,
outputs and scratch of EXACTLY the queried size are carved from the arena).  guard.guarded records libvnet_hip.so only, so every case
wraps postprocess.lib in a recorder of its own: the entry points called go to the same list, and every device pointer must lie inside
the arena.  Checked by guard.check_case: (a) every guard byte intact and no input modified, (b) every output byte written, (c) results
against the NumPy rules (vnet_tensorflow_amd/postprocess.py), (d) bit-identical results on a 0xFF and a 0x00 pre-fill of outputs and
scratch.
On (b): an output element that is legitimately all 0xFF reads as "never written".  The representative map holds -1 where the class is
not selected, by contract: for it the elements still reading 0xFF must be exactly those voxels (tests/test_hip_components_guard.py does
the same for vnet_cc_roots; the 0x00 run, where an unwritten voxel would read 0, is held to the rule like every result).  Nothing else
here can be all ones: class values are positive, and no mask word has all 64 bits set (rows of 65 voxels or of one: the high bits of
the last word are 0, and the masks are about half full, so neither they nor their complements fill a word; the pipeline case
dilates the mask of a one-voxel class only -- vnet_post_not_bits has its own cases)."""
import os

import numpy as np
import pytest
import torch

from tests import guard
from vnet_tensorflow_amd import morph, postprocess as PP, prepare_data

pytestmark = pytest.mark.gpu
SHAPES = {"5x7x65": (5, 7, 65), "1x1x1": (1, 1, 1)}
HOST_POINTERS = {("vnet_post_class_roots", "values"), ("vnet_post_filter_components", "values")}
SP = (0.7, 0.7, 2.5)
CLASSES = [1, 2, 3]


class _Recording(object):
    """Stands in for postprocess.lib(): records the entry points called; a device pointer outside the arena is an error."""

    def __init__(self, real, arena, calls):
        table = guard.pointer_entry_points(os.path.join(guard.ROOT, PP.HEADER))
        self.__dict__.update(_real=real, _arena=arena, _calls=calls, _table=table)

    def __getattr__(self, name):
        fn, params = getattr(self._real, name), self._table.get(name)
        if params is None:                     # (a size query)
            return fn

        def call(*args):
            self._calls.append(name)
            for (pname, ptr, _const, _typ), a in zip(params, args):
                if not ptr or pname == "stream" or (name, pname) in HOST_POINTERS or a is None:
                    continue
                if self._arena.find(a) is None:
                    raise guard.GuardError("%s: argument `%s` (0x%x) is not a tensor of the arena" % (name, pname, a))
            return fn(*args)
        return call


def _recorded(fn):
    def run(h):
        real = PP.lib
        rec = _Recording(real(), h.arena, h.calls)
        PP.lib = lambda: rec
        try:
            return fn(h)
        finally:
            PP.lib = real
    return run


def _label(shape):
    rng = np.random.default_rng(sum(shape))
    lab = (rng.integers(1, 4, size=shape) * (rng.random(shape) < 0.6)).astype(np.int32)
    lab[-1, -1, -1] = 2
    if lab.size > 27:
        lab[1:4, 1:4, 1:4] = 1
        lab[2, 2, 2] = 0                        # a cavity of class 1
        lab[0, 0, 0] = 4                        # a class of one voxel: its mask and the mask's dilation stay far from a full word
    return lab


def _roots(shape, sizes):
    def run(h):
        lab = _label(shape)
        res = PP.class_roots_device(h.g(lab, dtype=torch.int32), [3, 1], sizes=sizes)
        ref_r, ref_s = PP.class_roots(lab, [3, 1])
        roots = res[0] if sizes else res
        assert np.array_equal(roots.cpu().numpy(), ref_r)
        if sizes:
            assert np.array_equal(res[1].cpu().numpy(), ref_s)
        return {roots.data_ptr(): int((ref_r == -1).sum())}      # the output whose -1 is a written value, and how many it holds
    return run


def _filter(shape, mode):
    def run(h):
        lab = _label(shape)
        got = PP.filter_components(h.g(lab, dtype=torch.int32), CLASSES, mode, 2.0, PP.voxel_volume(SP))
        want = PP.keep_largest(lab, CLASSES) if mode == 0 else PP.remove_small(lab, 2.0, SP, CLASSES)
        assert np.array_equal(got.cpu().numpy(), want)
        assert h.ws_requests == [128 + 128 * ((lab.size + 255) // 256) + 8 * lab.size]
        return {}
    return run


def _fill(shape):
    def run(h):
        lab = _label(shape)
        got = PP.fill_holes_class(h.g(lab, dtype=torch.int32), 1)
        want = PP.fill_holes(lab, [1])
        assert np.array_equal(got.cpu().numpy(), want) and (lab.size < 27 or (want != lab).any())
        assert h.ws_requests == [5 * lab.size]
        return {}
    return run


def _mask(shape):
    m = np.random.default_rng(3).random(shape) < 0.5
    m[-1, -1, -1] = True
    return m


def _not(shape):
    def run(h):
        m = _mask(shape)
        got = PP.not_bits(h.g(prepare_data.pack_bits(m), dtype=torch.int64), shape[2])
        assert np.array_equal(got.cpu().numpy(), prepare_data.pack_bits(~m))
        return {}
    return run


def _apply(shape):
    def run(h):
        lab, m = _label(shape), _mask(shape)
        got = PP.apply_bits(h.g(lab, dtype=torch.int32), h.g(prepare_data.pack_bits(m), dtype=torch.int64), 2)
        assert np.array_equal(got.cpu().numpy(), PP.apply_mask(lab, m, 2))
        return {}
    return run


def _pipeline(shape):
    def run(h):
        lab = _label(shape)
        steps = [PP.KeepLargestComponent(), PP.RemoveSmallComponents(2.0, [1, 3]), PP.FillHoles([1]), PP.Dilate(2, [4])]
        got = PP.run(steps, h.g(lab, dtype=torch.int32), SP, classes=5)
        assert np.array_equal(got.cpu().numpy(), PP.run(steps, lab, SP, classes=5))
        return {}
    return run


_ALL = ("vnet_post_filter_components", "vnet_post_fill_holes", "vnet_post_apply_bits")
CASES = {}
for _name, _shape in SHAPES.items():
    CASES["roots " + _name] = (("vnet_post_class_roots",), _recorded(_roots(_shape, False)))
    CASES["roots and sizes " + _name] = (("vnet_post_class_roots",), _recorded(_roots(_shape, True)))
    CASES["keep largest " + _name] = (("vnet_post_filter_components",), _recorded(_filter(_shape, 0)))
    CASES["remove small " + _name] = (("vnet_post_filter_components",), _recorded(_filter(_shape, 1)))
    CASES["fill holes " + _name] = (("vnet_post_fill_holes",), _recorded(_fill(_shape)))
    CASES["not bits " + _name] = (("vnet_post_not_bits",), _recorded(_not(_shape)))
    CASES["apply bits " + _name] = (("vnet_post_apply_bits",), _recorded(_apply(_shape)))
    CASES["pipeline " + _name] = (_ALL + ("vnet_select_bits", "vnet_dilate_bits"), _recorded(_pipeline(_shape)))


def _check_written(arena, minus_one):
    """arena.check_written(), with the representative maps held to their own rule."""
    bad = []
    seen = set()
    for e, n, first in arena.unwritten():
        want = minus_one.get(e.tensor.data_ptr())
        seen.add(e.tensor.data_ptr())
        if want is None or n != want:
            bad.append("%s: %d elements still 0xFF (first at %d), %s" % (e.describe(), n, first,
                                                                         "none may be" if want is None else "%d are not selected" % want))
    for ptr, want in minus_one.items():
        if want and ptr not in seen:
            bad.append("the representative map at 0x%x shows no -1 on its %d unselected voxels" % (ptr, want))
    if bad:
        raise guard.GuardError("\n".join(bad))


def test_every_entry_point_of_the_header_has_a_case():
    declared = set(guard.pointer_entry_points(os.path.join(guard.ROOT, PP.HEADER)))
    assert declared == {e for entries, _ in CASES.values() for e in entries if e.startswith("vnet_post_")} and len(declared) == 5
    assert declared == {n for n in PP.SIGNATURES_POST if not n.endswith("_ws_bytes")}


@pytest.mark.parametrize("cid", sorted(CASES))
def test_postprocess_guard_bands(dev, cid):
    guard.check_case(CASES, cid, dev, capacity=96 << 20, written=_check_written, modules=(PP, morph))

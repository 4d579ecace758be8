"""-m gpu: guard bands (tests/guard.py) around the two entry points of csrc/vnet_window.h (libvnet_window.so), called the way the
product calls them (the ops of vnet_tensorflow_amd/window.py inside guarded(arena, modules=(window,)): inputs, outputs and the running
sums are carved from the arena).  guard.guarded records libvnet_hip.so only, so every case wraps window.lib in a recorder of its own:
the entry points called go to the same list, and every device pointer must lie inside the arena.  Checked by guard.check_case: (a)
every guard byte intact and no input modified, (b) every byte of a crop's output written from the 0xFF poison -- also where the
window reaches past the volume and the word is a written 0 (no source word is all ones: the images are positive floats, the labels
positive integers), (c) results against the NumPy rules, which leave vol and cnt untouched outside the window, (d) bit-identical
results on a 0xFF and a 0x00 pre-fill of the outputs."""
import os

import numpy as np
import pytest
import torch

from tests import guard
from tests.test_window_host import asymmetric_weights, softmax_like
from vnet_tensorflow_amd import window as W

pytestmark = pytest.mark.gpu


class _Recording(object):
    """Stands in for window.lib(): records the entry points called; a device pointer outside the arena is an error."""

    def __init__(self, real, arena, calls):
        table = guard.pointer_entry_points(os.path.join(guard.ROOT, W.HEADER))
        self.__dict__.update(_real=real, _arena=arena, _calls=calls, _table=table)

    def __getattr__(self, name):
        fn, params = getattr(self._real, name), self._table[name]

        def call(*args):
            self._calls.append(name)
            for (pname, ptr, _const, _typ), a in zip(params, args):
                if not ptr or pname == "stream" or a is None:
                    continue
                if self._arena.find(a) is None:
                    raise guard.GuardError("%s: argument `%s` (0x%x) is not a tensor of the arena" % (name, pname, a))
            return fn(*args)
        return call


def _recorded(fn):
    def run(h):
        real = W.lib
        rec = _Recording(real(), h.arena, h.calls)
        W.lib = lambda: rec
        try:
            return fn(h)
        finally:
            W.lib = real
    return run


def _crop(vol, start, size, mask, label=False):
    def run(h):
        rng = np.random.default_rng(sum(vol))
        if label:
            src, dt = rng.integers(1, 9, size=vol[:3]).astype(np.int32), torch.int32
        else:
            src, dt = (rng.random(vol) + 0.5).astype(np.float32), torch.float32
        got = W.crop_flip(h.g(src, dtype=dt), start, size, mask)                       # (the output: window.torch.empty, from the arena)
        want = W.crop_flip_np(src, start, size, mask)
        assert np.array_equal(got.cpu().numpy(), want) and (want == 0).any() == any(s + p > n for s, p, n in zip(start, size, vol))
        return True
    return run


def _accumulate(P, D, K, origins, mask, weighted, with_cnt):
    def run(h):
        w = asymmetric_weights(P, 7) if weighted else None
        wd = None if w is None else tuple(h.g(v) for v in w)
        vol, cnt = softmax_like(D + (K,), seed=1), softmax_like(D, seed=2) if with_cnt else None
        tv = h.arena.tensor("vol", vol.shape, torch.float32, "inout", vol)
        tc = h.arena.tensor("cnt", cnt.shape, torch.float32, "inout", cnt) if with_cnt else None
        for n, origin in enumerate(origins):
            patch = softmax_like(P + (K,), seed=3 + n)
            W.accumulate(h.g(patch), tv, tc, origin, mask, wd)
            W.accumulate_np(patch, vol, cnt, origin, mask, w)
        assert np.array_equal(tv.cpu().numpy(), vol) and (cnt is None or np.array_equal(tc.cpu().numpy(), cnt))
        return True
    return run


_C, _A = ("vnet_window_crop_flip",), ("vnet_window_accumulate",)
CASES = {
    "crop C1 past the extent": (_C, _recorded(_crop((7, 6, 9, 1), (5, 3, 6), (4, 5, 6), 0))),
    "crop C3 mirrored past the extent": (_C, _recorded(_crop((7, 6, 9, 3), (5, 3, 6), (4, 5, 6), 7))),
    "crop C4 mirrored, 16-byte words": (_C, _recorded(_crop((7, 6, 9, 4), (5, 3, 6), (4, 5, 6), 5))),
    "crop C4 inside, rows of 65": (_C, _recorded(_crop((9, 8, 70, 4), (1, 2, 3), (8, 6, 65), 6))),
    "crop label mirrored": (_C, _recorded(_crop((7, 6, 9), (5, 3, 6), (4, 5, 6), 3, label=True))),
    "crop 1x1x1": (_C, _recorded(_crop((1, 1, 1, 1), (0, 0, 0), (1, 1, 1), 7))),
    "accumulate K2 weighted mirrored": (_A, _recorded(_accumulate((4, 5, 6), (7, 6, 9), 2, [(2, 1, 3), (5, 3, 6)], 7, True, True))),
    "accumulate K4 plain": (_A, _recorded(_accumulate((4, 5, 6), (7, 6, 9), 4, [(0, 0, 0), (5, 3, 6)], 0, False, True))),
    "accumulate K3 weighted, no count": (_A, _recorded(_accumulate((4, 5, 6), (7, 6, 9), 3, [(5, 3, 6), (3, 1, 3)], 2, True, False))),
    "accumulate K7 mirrored, rows of 65": (_A, _recorded(_accumulate((3, 4, 65), (5, 6, 70), 7, [(1, 1, 2), (3, 4, 60)], 4, False, True))),
    "accumulate K1 at the far corner": (_A, _recorded(_accumulate((4, 5, 6), (7, 6, 9), 1, [(6, 5, 8)], 7, True, True))),
    "accumulate K5 outside": (_A, _recorded(_accumulate((4, 5, 6), (7, 6, 9), 5, [(7, 0, 0), (0, 0, 9), (2, 2, 2)], 1, True, True))),
}


def test_every_entry_point_of_the_header_has_a_case():
    declared = set(guard.pointer_entry_points(os.path.join(guard.ROOT, W.HEADER)))
    assert declared == {e for entries, _ in CASES.values() for e in entries} == set(W.SIGNATURES_WINDOW) and len(declared) == 2


@pytest.mark.parametrize("cid", sorted(CASES))
def test_window_guard_bands(dev, cid):
    guard.check_case(CASES, cid, dev, capacity=64 << 20, modules=(W,))

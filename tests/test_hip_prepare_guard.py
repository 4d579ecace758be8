"""-m gpu: guard bands (tests/guard.py) around the four entry points of include/vnet_hip_prepare.h, called the way the product
calls them (ops.channel_stats / window_intensity / crop_window / argmax_label inside guarded(): inputs, parameter tables, outputs and
scratch are all carved from the arena, the scratch of EXACTLY the queried size).  Checked: (a) every guard byte intact and no input
modified, (b) every output element written on the 0xFF pre-fill -- the zero fill of a window that overhangs the volume comes from the
kernel, not from a memset -- (c) results against the NumPy restatements (vnet_tensorflow_amd/prepare.py), (d) bit-identical results on a
0xFF and a 0x00 pre-fill of outputs and scratch.  CASES (entry points a case must reach, function) is what the ledger test in
tests/test_abi_ledger.py reads."""
import numpy as np
import pytest
import torch

from tests import guard
from tests import prepare_data as D

pytestmark = pytest.mark.gpu
VOLUME, PATCH = (19, 21, 17), (16, 12, 20)


def _stats(C, n, with_pre):
    def run(h):
        from vnet_tensorflow_amd import _lib, ops, prepare as P
        x = D.tier_e(n, C, 3)
        pre = np.stack([np.arange(C) * 4.0 - 8.0, 2.0 ** np.arange(C)], axis=1) if with_pre else None      # (exact in double)
        got = ops.channel_stats(h.g(x), h.g(pre, dtype=torch.float64) if with_pre else None)
        assert h.ws_requests == [_lib.lib().vnet_channel_stats_ws_bytes(C)] and h.ws_requests[0] == 8 * C * (4 * ops.STATS_MAX_BLOCKS + 1)
        assert got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), P.channel_stats(x, pre))
    return run


def _window(C, in_place):
    def run(h):
        from vnet_tensorflow_amd import ops, prepare as P
        x = np.random.default_rng(C).normal(100.0, 60.0, VOLUME + (C,)).astype(np.float32)
        prm = np.array([[3.0 * c, 1.0 + c, -20.0 + c, 255.0 / (211.0 + c), float(c == 1)] for c in range(C)])
        src = h.arena.tensor("image", x.shape, torch.float32, "inout", x) if in_place else h.g(x)
        got = ops.window_intensity(src, h.g(prm, dtype=torch.float64), out=src if in_place else None)
        assert (got is src) == in_place and np.array_equal(got.cpu().numpy(), P.window_intensity(x, prm))
    return run


def _crop(C, start, misaligned=False, label=False):
    def run(h):
        from vnet_tensorflow_amd import ops, prepare as P
        rng = np.random.default_rng(10 + C)
        if label:
            x, dt = rng.integers(1, 300, size=VOLUME).astype(np.int32), torch.int32
        else:
            x, dt = rng.normal(100.0, 40.0, VOLUME + (C,)).astype(np.float32), torch.float32
        shape = PATCH + (() if label else (C,))
        if misaligned:          # a slot one word into its buffer: the one-word path whatever C is (the word in front stays poison)
            buf = h.arena.tensor("slots", (int(np.prod(shape)) + 1,), dt, "out", fill=np.full(int(np.prod(shape)) + 1, 7))
            out = buf[1:].view(shape)
        else:
            out = h.arena.tensor("slot", shape, dt, "out")
        assert ops.crop_window(h.g(x, dtype=dt), start, PATCH, out=out) is out
        assert np.array_equal(out.cpu().numpy(), P.crop_window(x, start, PATCH))
        if misaligned:
            assert int(buf[0]) == 7
    return run


def _argmax(K, n):
    def run(h):
        from vnet_tensorflow_amd import ops, prepare as P
        x = np.random.default_rng(K).integers(-3, 4, size=(n, K)).astype(np.float32)           # (many ties)
        got = ops.argmax_label(h.g(x))
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), P.argmax_label(x))
    return run


_ST, _W, _C, _A = ("vnet_channel_stats",), ("vnet_window_intensity",), ("vnet_crop_words",), ("vnet_argmax_label",)
CASES = {
    "stats c1 (scalar) n4099": (_ST, _stats(1, 4099, False)),
    "stats c3 (scalar) n4099 pre": (_ST, _stats(3, 4099, True)),
    "stats c4 (quads) n4099 pre": (_ST, _stats(4, 4099, True)),
    "window c3 (scalar) in place": (_W, _window(3, True)),
    "window c4 (quads)": (_W, _window(4, False)),
    "window c8 (quads) in place": (_W, _window(8, True)),
    "crop c1 (words) overhang xyz": (_C, _crop(1, (10, 12, 3))),
    "crop c4 (quads) overhang xyz": (_C, _crop(4, (10, 12, 3))),
    "crop c4 misaligned slot": (_C, _crop(4, (0, 20, 0), misaligned=True)),
    "crop int32 label": (_C, _crop(1, (18, 0, 16), label=True)),
    "argmax k2 (pairs)": (_A, _argmax(2, 4097)),
    "argmax k5 (scalar)": (_A, _argmax(5, 4097)),
    "argmax k32 (quads)": (_A, _argmax(32, 4097)),
}


@pytest.mark.parametrize("cid", sorted(CASES))
def test_prepare_guard_bands(dev, cid):
    guard.check_case(CASES, cid, dev, capacity=48 << 20)

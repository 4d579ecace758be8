"""-m gpu: guard bands (tests/guard.py) around the entry points of include/vnet_hip_components.h, called the way the product
calls them (ops.component_roots / largest_component / volume_threshold inside guarded(): the label, the outputs and the scratch -- of
EXACTLY the queried size -- are all carved from the arena).  Checked: (a) every guard byte intact and no input modified, (b) every
output element written on the 0xFF pre-fill, (c) results against the host, exactly, (d) bit-identical results on a 0xFF and a 0x00
pre-fill.  The representative map holds -1 on the background by contract, which guard.unwritten() cannot tell from the 0xFF poison: for
it the elements still reading 0xFF must be exactly the background voxels (the 0x00 run, where an unwritten background voxel would read
0 and not -1, closes the argument through (c) and (d)).  CASES (entry points a case must reach, function) is what the ledger test in
tests/test_abi_ledger.py reads."""
import numpy as np
import pytest
import torch

from tests import guard

pytestmark = pytest.mark.gpu
SHAPES = ((5, 4, 3), (9, 9, 9))


def _label(shape):
    rng = np.random.default_rng(sum(shape))
    return (rng.integers(1, 6, size=shape) * (rng.random(shape) < 0.4)).astype(np.int32)


def _roots(shape, sizes):
    def run(h):
        from tests.test_hip_components import host_roots
        from vnet_tensorflow_amd import ops
        lab = _label(shape)
        res = ops.component_roots(h.g(lab, dtype=torch.int32), sizes=sizes)
        ref_r, ref_s = host_roots(lab)
        roots = res[0] if sizes else res
        assert np.array_equal(roots.cpu().numpy(), ref_r)
        if sizes:
            assert np.array_equal(res[1].cpu().numpy(), ref_s)
        return {roots.data_ptr(): int((lab == 0).sum())}         # the output whose -1 is a written value, and how many it holds
    return run


def _largest(shape, min_volume):
    def run(h):
        from vnet_tensorflow_amd import model, ops
        lab = _label(shape)
        y = ops.largest_component(h.g(lab, dtype=torch.int32), classes=6, min_volume=min_volume, spacing=(0.5, 1.0, 1.5))
        ref = model.ExtractLargestConnectedComponents(lab)
        if min_volume is not None:
            ref = model.volume_threshold(ref, min_volume, (0.5, 1.0, 1.5))
        assert y.dtype == torch.uint8 and np.array_equal(y.cpu().numpy(), ref)
        assert h.ws_requests == [16 + 8 * lab.size]
        return {}
    return run


def _threshold(shape, volume):
    def run(h):
        from vnet_tensorflow_amd import model, ops
        lab = _label(shape)
        y = ops.volume_threshold(h.g(lab, dtype=torch.int32), volume, (0.5, 1.0, 1.5))
        assert y.dtype == torch.uint8 and np.array_equal(y.cpu().numpy(), model.volume_threshold(lab, volume, (0.5, 1.0, 1.5)))
        assert h.ws_requests == [16 + 8 * lab.size]
        return {}
    return run


_R, _L, _T = ("vnet_cc_roots",), ("vnet_cc_largest",), ("vnet_cc_volume_threshold",)
CASES = {}
for _s in SHAPES:
    _n = "%dx%dx%d" % _s
    CASES["roots %s" % _n] = (_R, _roots(_s, False))
    CASES["roots and sizes %s" % _n] = (_R, _roots(_s, True))
    CASES["largest %s" % _n] = (_L, _largest(_s, None))
    CASES["largest thresholded %s" % _n] = (_L, _largest(_s, 2.0))
    CASES["threshold %s" % _n] = (_T, _threshold(_s, 1.6))


def _check_written(arena, minus_one):
    """arena.check_written(), with the representative maps held to their own rule."""
    bad = []
    seen = set()
    for e, n, first in arena.unwritten():
        want = minus_one.get(e.tensor.data_ptr())
        seen.add(e.tensor.data_ptr())
        if want is None or n != want:
            bad.append("%s: %d elements still 0xFF (first at %d), %s" % (e.describe(), n, first,
                                                                         "none may be" if want is None else "%d are background" % want))
    for ptr, want in minus_one.items():
        if want and ptr not in seen:
            bad.append("the representative map at 0x%x shows no -1 on its %d background voxels" % (ptr, want))
    if bad:
        raise guard.GuardError("\n".join(bad))


@pytest.mark.parametrize("cid", sorted(CASES))
def test_components_guard_bands(dev, cid):
    guard.check_case(CASES, cid, dev, capacity=32 << 20, written=_check_written)

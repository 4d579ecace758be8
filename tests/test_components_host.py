"""Connected components, the parts that need no GPU: the claim about scipy's numbering that the device's tie rule rests on, the ledger of
include/vnet_hip_components.h, its error codes before any launch, and the wrappers' routes to the host functions (more than 255 classes,
a volume past the int32 index) through a stand-in library."""
import ctypes

import numpy as np
import pytest
import torch


def test_host_labels_are_numbered_by_first_voxel():
    """scipy.ndimage.label numbers the components in the C order of their first voxels, so the host function's "first label wins" on a
    tie in size IS "the smaller representative wins", the rule the device states (checked on random maps at and around the percolation
    threshold, and on a tie built by hand)."""
    from scipy import ndimage
    from vnet_tensorflow_amd import model
    for seed, p in enumerate((0.15, 0.3, 0.32, 0.5)):
        m = np.random.default_rng(seed).random((13, 9, 11)) < p
        cc, n = ndimage.label(m)
        flat = cc.ravel()
        first = [int(np.flatnonzero(flat == k)[0]) for k in range(1, n + 1)]
        assert n > 1 and first == sorted(first)
        sizes = np.bincount(flat)[1:]
        best = int(np.flatnonzero(sizes == sizes.max())[0])        # of the largest, the one whose first voxel comes first
        assert np.array_equal(model.ExtractLargestConnectedComponents(m.astype(np.int32)), (cc == best + 1).astype(np.uint8))
    lab = np.zeros((5, 6, 7), np.int32)
    lab[0, 0, 1:5] = 1
    lab[3:5, 3:5, 3] = 2
    assert model.ExtractLargestConnectedComponents(lab)[0, 0, 1:5].all()
    assert model.ExtractLargestConnectedComponents(lab[::-1, ::-1, ::-1].copy())[0:2, 1:3, 3].all()


def test_components_header_ledger():
    """include/vnet_hip_components.h beyond tests/test_abi_ledger.py: the guarded cases of tests/test_hip_components_guard.py run
    both shapes; the loaded library carries the table's argument types."""
    from vnet_tensorflow_amd import _lib
    from tests import test_hip_components_guard as TG
    for shape in ((5, 4, 3), (9, 9, 9)):
        assert any("%dx%dx%d" % shape in cid for cid in TG.CASES)
    bound = _lib.lib()
    assert bound.vnet_cc_largest.argtypes == _lib.SIGNATURES_COMPONENTS["vnet_cc_largest"][1]
    assert _lib.SIGNATURES_COMPONENTS["vnet_cc_ws_bytes"][0] is ctypes.c_size_t


def test_error_codes_need_no_device():
    """Before any launch: VNET_E_BADARG (-1) on null pointers, sizes < 1 and a volume or voxel volume that is not finite,
    VNET_E_UNSUPPORTED (-2) on a volume past the int32 index, VNET_E_WORKSPACE (-3) on a short ws; the size query answers 0 for what
    the entry points refuse."""
    from vnet_tensorflow_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)
    dims = (5, 4, 3)
    need = L.vnet_cc_ws_bytes(*dims)
    assert need == 16 + 8 * 60 and need <= 8 * 60 + 64
    assert L.vnet_cc_ws_bytes(1024, 1024, 512) == 16 + 8 * 2 ** 29 and L.vnet_cc_ws_bytes(1024, 1024, 1024) == 16 + 8 * 2 ** 30
    # null pointers
    assert L.vnet_cc_roots(None, one, None, *dims, None) == -1 and L.vnet_cc_roots(one, None, one, *dims, None) == -1
    for fn, mid in ((L.vnet_cc_largest, (0, 1.0, 1.0)), (L.vnet_cc_volume_threshold, (1.0, 1.0))):
        assert fn(None, one, *dims, *mid, one, need, None) == -1
        assert fn(one, None, *dims, *mid, one, need, None) == -1
        assert fn(one, one, *dims, *mid, None, need, None) == -1
        assert fn(one, one, *dims, *mid, ctypes.c_void_p(20), need, None) == -1          # ws not 8-byte aligned
        # sizes < 1
        for pos in range(3):
            for v in (0, -2):
                bad = list(dims)
                bad[pos] = v
                assert fn(one, one, *bad, *mid, one, need, None) == -1
                assert L.vnet_cc_roots(one, one, None, *bad, None) == -1 and L.vnet_cc_ws_bytes(*bad) == 0
        # volume, voxel_volume not finite
        for pos in (len(mid) - 2, len(mid) - 1):
            for v in (float("nan"), float("inf"), -float("inf")):
                bad = list(mid)
                bad[pos] = v
                assert fn(one, one, *dims, *bad, one, need, None) == -1
        # a short ws
        assert fn(one, one, *dims, *mid, one, need - 1, None) == -3 and fn(one, one, *dims, *mid, one, 0, None) == -3
        # past the index range: 2^31 voxels (2^31 - 1 is the last supported count)
        big = (2048, 2048, 512)
        assert fn(one, one, *big, *mid, one, 1 << 40, None) == -2
        assert fn(one, one, 1, 1, 2 ** 31 - 1, *mid, one, 8, None) == -3                 # supported, so the ws is looked at
    assert L.vnet_cc_roots(one, one, None, 2048, 2048, 512, None) == -2 and L.vnet_cc_ws_bytes(2048, 2048, 512) == 0
    assert L.vnet_cc_ws_bytes(1, 1, 2 ** 31 - 1) == 16 + 8 * (2 ** 31 - 1)


def test_ops_refuse_cpu_tensors():
    from vnet_tensorflow_amd import ops
    from vnet_tensorflow_amd._lib import VnetHipError
    lab = torch.ones(5, 4, 3, dtype=torch.int32)
    with pytest.raises(VnetHipError, match="component_roots: tensor on cpu"):
        ops.component_roots(lab)
    with pytest.raises(VnetHipError, match="largest_component: tensor on cpu"):
        ops.largest_component(lab, classes=3)
    with pytest.raises(VnetHipError, match="volume_threshold: tensor on cpu"):
        ops.volume_threshold(lab, 1.0, (1.0, 1.0, 1.0))
    with pytest.raises(VnetHipError, match=r"\[X,Y,Z\]"):
        ops.component_roots(torch.ones(5, 4, dtype=torch.int32))


class _NoKernels(object):
    """A library whose size query is scripted and whose kernels must not be reached."""

    def __init__(self, ws_bytes):
        self.ws_bytes, self.queries = ws_bytes, []

    def vnet_cc_ws_bytes(self, X, Y, Z):
        self.queries.append((X, Y, Z))
        return self.ws_bytes

    def __getattr__(self, name):
        raise AssertionError("the fallback must not launch %s" % name)


def _host_route(monkeypatch, ws_bytes):
    from vnet_tensorflow_amd import _lib, ops
    fake = _NoKernels(ws_bytes)
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(ops, "_need_gpu", lambda *a, **k: None)        # (the stand-in has no device either)
    return fake


def test_more_than_255_classes_take_the_host_function(monkeypatch):
    """The reference casts the label to uint8 before labelling: class 256 becomes background.  The device kernels see label != 0, so a
    class count past 255 goes to the host function, cast included -- whether the count is given or read from the label."""
    from vnet_tensorflow_amd import model, ops
    fake = _host_route(monkeypatch, 16 + 8 * 60)
    lab = np.zeros((5, 4, 3), np.int32)
    lab[0, 0, :] = 256                                          # three voxels the cast removes
    lab[3, 1:3, 1] = 7                                          # two voxels that stay
    ref = model.ExtractLargestConnectedComponents(lab)
    assert ref[3, 1:3, 1].all() and ref.sum() == 2
    for kw in ({"classes": 300}, {}):
        got = ops.largest_component(torch.from_numpy(lab), **kw)
        assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), ref)
    got = ops.largest_component(torch.from_numpy(lab), classes=300, min_volume=1.0, spacing=(0.5, 1.0, 1.0))
    assert np.array_equal(got.numpy(), model.volume_threshold(ref, 1.0, (0.5, 1.0, 1.0))) and not got.any()
    assert fake.queries == []                                    # decided before the library was asked anything
    # 255 classes or fewer reach the library (here: the stand-in refuses the launch)
    with pytest.raises(AssertionError, match="vnet_cc_largest"):
        ops.largest_component(torch.from_numpy(np.minimum(lab, 5)), classes=6)


def test_oversize_volumes_take_the_host_functions(monkeypatch):
    """vnet_cc_ws_bytes == 0 is the library's "an int32 cannot index this volume" (VNET_E_UNSUPPORTED at the entry points): both filters
    then run the host functions and no kernel is launched."""
    from vnet_tensorflow_amd import model, ops
    fake = _host_route(monkeypatch, 0)
    lab = (np.random.default_rng(0).random((6, 5, 4)) < 0.4).astype(np.int32) * 3
    sp = (0.5, 0.5, 1.5)
    t = torch.from_numpy(lab)
    assert np.array_equal(ops.largest_component(t, classes=4).numpy(), model.ExtractLargestConnectedComponents(lab))
    assert np.array_equal(ops.volume_threshold(t, 1.0, sp).numpy(), model.volume_threshold(lab, 1.0, sp))
    both = ops.largest_component(t, classes=4, min_volume=1.0, spacing=sp)
    assert np.array_equal(both.numpy(), model.volume_threshold(model.ExtractLargestConnectedComponents(lab), 1.0, sp))
    assert fake.queries == [(6, 5, 4)] * 3


def test_evaluate_single_3d_keeps_its_signature_defaults():
    import inspect
    from vnet_tensorflow_amd import model
    p = inspect.signature(model.image2label.evaluate_single_3D).parameters
    assert [p[k].default for k in ("back_size", "back_ratio", "largest_component", "volume_threshold", "spacing", "extent")] == \
        [None, None, False, None, None, None]

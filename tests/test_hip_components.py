"""-m gpu: connected components and the two label filters on the device (csrc/components.hip, include/vnet_hip_components.h).

Equality is exact everywhere.  The reference for the representative map is the host labelling (scipy.ndimage.label, default structure:
face connectivity) canonicalised to the smallest linear index per component; the reference for the two filters is the unchanged
model.ExtractLargestConnectedComponents and model.volume_threshold.  The shapes are the smallest at which each failure mode can show."""
import os
import re

import numpy as np
import pytest
import torch

from tests.util import g
from vnet_tensorflow_amd import data

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the references ------------------------------------------------------------------------------------------------------------------------
def host_roots(label):
    """(roots, sizes) as include/vnet_hip_components.h states them, from scipy's labelling."""
    from scipy import ndimage
    label = np.asarray(label)
    cc, n = ndimage.label(label != 0)
    flat = cc.ravel()
    first = np.full(n + 1, -1, dtype=np.int64)
    idx = np.nonzero(flat)[0]
    first[flat[idx][::-1]] = idx[::-1]                          # the smallest linear index of every component
    roots = first[flat].astype(np.int32).reshape(label.shape)
    sizes = np.zeros(flat.size, dtype=np.int32)
    sizes[first[1:]] = np.bincount(flat, minlength=n + 1)[1:]
    return roots, sizes.reshape(label.shape)


def check_all(label, dev, volumes=(0.5, 3.0), spacing=(1.0, 1.0, 1.0), classes=None):
    """Roots, sizes, the largest component, the thresholds and the chained pair against the host, exactly.  Returns the device results."""
    from vnet_tensorflow_amd import model, ops
    label = np.ascontiguousarray(label, dtype=np.int32)
    t = g(label, dev, torch.int32)
    roots, sizes = ops.component_roots(t, sizes=True)
    ref_r, ref_s = host_roots(label)
    assert roots.dtype == torch.int32 and tuple(roots.shape) == label.shape
    assert np.array_equal(roots.cpu().numpy(), ref_r), "roots differ at %d voxels" % int((roots.cpu().numpy() != ref_r).sum())
    assert np.array_equal(sizes.cpu().numpy(), ref_s)
    assert torch.equal(ops.component_roots(t), roots)
    kw = {} if classes is None else {"classes": classes}
    big = ops.largest_component(t, **kw)
    ref_big = model.ExtractLargestConnectedComponents(label)
    assert big.dtype == torch.uint8 and np.array_equal(big.cpu().numpy(), ref_big)
    out = [roots, sizes, big]
    for v in volumes:
        thr = ops.volume_threshold(t, v, spacing)
        assert thr.dtype == torch.uint8 and np.array_equal(thr.cpu().numpy(), model.volume_threshold(label, v, spacing)), v
        both = ops.largest_component(t, min_volume=v, spacing=spacing, **kw)
        assert np.array_equal(both.cpu().numpy(), model.volume_threshold(ref_big, v, spacing)), v
        assert torch.equal(ops.volume_threshold(big, v, spacing), both)            # (a uint8 map goes in as its mask)
        out += [thr, both]
    return out


def bernoulli(shape, p, seed):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.int32)


# ---- the cases of the issue ----------------------------------------------------------------------------------------------------------------
def test_degenerate_volumes(dev):
    from vnet_tensorflow_amd import ops
    check_all(np.ones((1, 1, 1)), dev)
    check_all(np.zeros((1, 1, 1)), dev)
    check_all(np.ones((7, 5, 3)), dev, volumes=(104.0, 105.0))
    zero = g(np.zeros((5, 4, 3)), dev, torch.int32)
    check_all(np.zeros((5, 4, 3)), dev)
    roots, sizes = ops.component_roots(zero, sizes=True)
    assert bool((roots == -1).all()) and not bool(sizes.any())
    assert not bool(ops.largest_component(zero).any()) and not bool(ops.volume_threshold(zero, -1.0).any())


def test_row_and_plane_wrap(dev):
    """Linear neighbours that are no face neighbours: (0,0,4) | (0,1,0) across a row end, (0,2,4) | (1,0,0) across a plane end."""
    from vnet_tensorflow_amd import ops
    for a, b in (((0, 0, 4), (0, 1, 0)), ((0, 2, 4), (1, 0, 0))):
        lab = np.zeros((4, 3, 5), np.int32)
        lab[a] = lab[b] = 1
        assert np.ravel_multi_index(b, lab.shape) - np.ravel_multi_index(a, lab.shape) == 1
        roots = check_all(lab, dev)[0].cpu().numpy()
        assert roots[a] != roots[b] and roots[a] == np.ravel_multi_index(a, lab.shape) and roots[b] == roots[a] + 1
    # and a full volume whose only gaps sit next to the wraps
    lab = np.ones((4, 3, 5), np.int32)
    lab[:, :, 1:4] = 0
    lab[1:3] = 0
    check_all(lab, dev)


def test_checkerboard_is_face_connectivity_only(dev):
    from vnet_tensorflow_amd import ops
    i, j, k = np.indices((6, 6, 6))
    lab = ((i + j + k) % 2 == 0).astype(np.int32)
    roots, sizes, big = check_all(lab, dev, volumes=(0.5, 1.0))[:3]
    assert int((sizes == 1).sum()) == 108 and int(sizes.sum()) == 108
    assert int(big.sum()) == 1 and int(big[0, 0, 0]) == 1              # the tie goes to the first voxel in C order
    t = g(lab, dev, torch.int32)
    assert int(ops.volume_threshold(t, 0.5).sum()) == 108 and int(ops.volume_threshold(t, 1.0).sum()) == 0


def _serpentine(n=9):
    """A one-voxel-wide path through n^3 (n odd): in every even plane x the rows along z at even y, joined alternately at z = n - 1 and
    z = 0, so a plane runs from (0, 0) to (n - 1, n - 1); the planes are joined alternately at that end and at that start.  One
    component, every voxel with at most two neighbours, the representative hundreds of links from the far end."""
    lab = np.zeros((n, n, n), np.int32)
    for x in range(0, n, 2):
        for y in range(0, n, 2):
            lab[x, y, :] = 1
            if y + 2 < n:
                lab[x, y + 1, (n - 1) if (y // 2) % 2 == 0 else 0] = 1
        if x + 2 < n:
            lab[(x + 1,) + ((n - 1, n - 1) if (x // 2) % 2 == 0 else (0, 0))] = 1
    return lab


def test_long_chain_both_ways(dev):
    from scipy import ndimage
    lab = _serpentine()
    assert ndimage.label(lab)[1] == 1 and lab.sum() > 200
    for m in (lab, lab[::-1, ::-1, ::-1], lab[:, ::-1, :], lab.transpose(2, 1, 0)):
        roots = check_all(m, dev, volumes=(float(lab.sum()) - 0.5, float(lab.sum())))[0]
        assert int(roots.max()) == int(np.flatnonzero(np.ascontiguousarray(m).ravel())[0])


def _combs(X=8):
    """Comb A: teeth (slabs over all z) at y = 0, 4, 8 for x < X - 2, joined by a spine in the plane x = 0; comb B: teeth at y = 2, 6 for
    x >= 2, joined by a spine in the LAST plane.  The teeth interleave and never touch; one voxel in front of B's spine joins the two."""
    sep = np.zeros((X, 9, 7), np.int32)
    sep[0:X - 2, 0::4, :] = 1
    sep[0, :, 0] = 1
    sep[2:X, 2::4, :] = 2
    sep[X - 1, :, 0] = 2
    joined = sep.copy()
    joined[X - 2, 0, 0] = 1
    return sep, joined


def test_late_merge_of_two_combs(dev):
    from scipy import ndimage
    sep, joined = _combs()
    assert ndimage.label(sep)[1] == 2 and ndimage.label(joined)[1] == 1
    assert int(check_all(sep, dev, volumes=(150.0, 200.0))[0].max()) == int(np.ravel_multi_index((2, 2, 0), sep.shape))
    for m in (joined, joined[::-1], joined[:, ::-1, ::-1]):
        assert int(check_all(m, dev)[1].max()) == int((joined != 0).sum()) == 224       # (voxels, not the sum of the classes)


def test_mixed_classes_are_one_mask(dev):
    from vnet_tensorflow_amd import ops
    rng = np.random.default_rng(5)
    lab = (rng.integers(1, 6, size=(11, 7, 9)) * (rng.random((11, 7, 9)) < 0.45)).astype(np.int32)
    roots = check_all(lab, dev, classes=6)[0]
    neg = lab.copy()
    neg[lab == 3] = -3                                          # a negative label is foreground
    assert torch.equal(ops.component_roots(g(neg, dev, torch.int32)), roots)
    two = np.zeros((3, 3, 3), np.int32)
    two[1, 1, 1], two[1, 1, 2] = 2, 5
    assert int(check_all(two, dev)[1].max()) == 2
    # other dtypes go in as their mask
    for dt in (torch.int64, torch.uint8, torch.float32):
        assert torch.equal(ops.component_roots(g(lab, dev, dt)), roots)


def test_ties_in_size(dev):
    """Two components of equal count; the later one is the compact one.  The host function's first-label-wins is the smaller first voxel."""
    lab = np.zeros((5, 6, 7), np.int32)
    lab[0, 0, 1:5] = 1                                          # 4 voxels, first voxel 1
    lab[3:5, 3:5, 3] = 2                                        # 4 voxels, first voxel later
    lab[2, 0, 0:3] = 1                                          # 3 voxels
    big = check_all(lab, dev, volumes=(3.5, 4.0))[2].cpu().numpy()
    assert big[0, 0, 1:5].all() and big.sum() == 4
    check_all(lab[::-1, ::-1, ::-1], dev, volumes=(3.5, 4.0))


def test_threshold_equality_is_strict(dev):
    from vnet_tensorflow_amd import ops
    lab = np.zeros((6, 6, 6), np.int32)
    lab[0:2, 0:2, 0:2] = 1                                      # 8 voxels: 8 * 0.125 == 1.0 exactly in double -> dropped
    lab[3:6, 3:6, 5] = 2                                        # 9 voxels: kept
    sp = (0.5, 0.5, 0.5)
    check_all(lab, dev, volumes=(1.0,), spacing=sp)
    thr = ops.volume_threshold(g(lab, dev, torch.int32), 1.0, sp).cpu().numpy()
    assert thr[3:6, 3:6, 5].all() and thr.sum() == 9
    # a spacing whose product rounds: the host's double decides, and the device forms the same one
    check_all(lab, dev, volumes=(8 * float(np.prod((0.3, 0.7, 1.1))),), spacing=(0.3, 0.7, 1.1))


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("p", [0.2, 0.32, 0.5, 0.8])
@pytest.mark.parametrize("shape", [(33, 17, 65), (64, 64, 40)], ids=["33x17x65", "64x64x40"])
def test_random_maps(dev, shape, p, seed):
    check_all(bernoulli(shape, p, 100 * seed + int(p * 100)), dev, volumes=(5.0,))


def _grid_cap():
    """Voxels one trip of the kernels' grid-stride loops covers, read from the source so that a change of the cap is seen."""
    src = open(os.path.join(ROOT, "vnet_tensorflow_amd", "csrc", "components.hip")).read()
    m = re.search(r"constexpr int CC_BLOCK = (\d+), CC_MAXBLK = (\d+);", src)
    assert m, "components.hip no longer states CC_BLOCK / CC_MAXBLK in one line"
    return int(m.group(1)) * int(m.group(2))


def test_volume_past_the_grid_cap(dev):
    shape = (112, 100, 104)
    assert shape[0] * shape[1] * shape[2] > _grid_cap()
    check_all(bernoulli(shape, 0.4, 7), dev, volumes=(40.0,))


def test_results_are_reproducible(dev):
    lab = bernoulli((64, 64, 40), 0.32, 3)
    a, b = check_all(lab, dev, volumes=(5.0,)), check_all(lab, dev, volumes=(5.0,))
    assert len(a) == len(b) == 5
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_error_codes_on_the_device(dev):
    from tests.test_components_host import test_error_codes_need_no_device
    from vnet_tensorflow_amd import _lib, ops
    from vnet_tensorflow_amd._lib import VnetHipError
    test_error_codes_need_no_device()
    L = _lib.lib()
    lab, out = torch.ones((5, 4, 3), dtype=torch.int32, device=dev), torch.zeros((5, 4, 3), dtype=torch.uint8, device=dev)
    need = L.vnet_cc_ws_bytes(5, 4, 3)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    assert L.vnet_cc_volume_threshold(lab.data_ptr(), out.data_ptr(), 5, 4, 3, 1.0, 1.0, ws.data_ptr(), need, ops._stream()) == 0
    assert L.vnet_cc_volume_threshold(lab.data_ptr(), out.data_ptr(), 5, 4, 3, 1.0, 1.0, ws.data_ptr(), need - 1, ops._stream()) == -3
    assert L.vnet_cc_largest(lab.data_ptr(), out.data_ptr(), 5, 4, 3, 1, float("inf"), 1.0, ws.data_ptr(), need, ops._stream()) == -1
    with pytest.raises(VnetHipError, match="VNET_E_BADARG"):
        ops.volume_threshold(lab, float("nan"))
    torch.cuda.synchronize()
    assert int(out.sum()) == 60


# ---- evaluate, end to end ------------------------------------------------------------------------------------------------------------------
K = 3
PIXDIM = (1.0, 0.8, 1.25)
VOLUME = (24, 20, 18)


@pytest.fixture(scope="module")
def small_model():
    from vnet_tensorflow_amd import model
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    cfg = {"TrainingSetting": {
        "Data": {"TrainingDataDirectory": ".", "TestingDataDirectory": ".", "ImageFilenames": ["image.nii"], "LabelFilename": "label.nii"},
        "BatchSize": 1, "PatchShape": [16, 16, 16], "SegmentationClasses": [0, 1, 2], "Epoches": 1,
        "Networks": {"Name": "VNet", "Dropout": 0.0, "NumChannel": 4, "NumLevels": 2, "NumCovolutions": [1, 1], "BottomConvolutions": 1},
        "Optimizer": {"Name": "Adam", "InitialLearningRate": 1e-2, "Decay": {"Factor": 0.99, "Steps": 100}},
        "Loss": {"Name": "sorensen"}},
        "EvaluationSetting": {"Data": {"EvaluateDataDirectory": ".", "ImageFilenames": ["image.nii"], "LabelFilename": "label_tf.nii"},
                              "CheckpointPath": "ckpt", "Stride": [8, 8, 8], "BatchSize": 4, "ProbabilityOutput": True}}
    torch.manual_seed(3)
    np.random.seed(3)
    m = model.image2label(None, cfg, device=torch.device("cuda", 0), verbose=False)
    m.read_config()
    m.build_model_graph()
    img, _ = data.synthetic_case(VOLUME, 1, K, 11)
    return m, img


def _host_filters(label, lcc, vt, spacing):
    from vnet_tensorflow_amd import model
    if lcc:
        label = model.ExtractLargestConnectedComponents(label, spacing)
    if vt is not None and vt > 0:
        label = model.volume_threshold(label, vt, spacing)
    return label


@pytest.mark.parametrize("branch", ["plain", "back"])
def test_evaluate_filters_on_the_device(dev, small_model, branch):
    """evaluate_single_3D with the filters on the device == the same call without them, then the host functions -- on the plain branch
    (cropped to the volume, and to a smaller `extent`) and on the back_size / back_ratio branch, with a non-unit spacing."""
    from vnet_tensorflow_amd import resample as R
    m, img = small_model
    kw, spacing = {}, PIXDIM
    if branch == "back":
        size = R.output_size(VOLUME, (1.0, 1.0, 1.0), (1.25, 0.8, 1.5))
        kw = dict(back_size=size, back_ratio=(1.25, 0.8, 1.5))
    plain, sm = m.evaluate_single_3D(img, **kw)
    again, sm2 = m.evaluate_single_3D(img, largest_component=False, volume_threshold=None, spacing=spacing, **kw)
    assert plain.dtype == again.dtype and plain.tobytes() == again.tobytes() and sm.tobytes() == sm2.tobytes()
    fg = float((plain != 0).sum()) * float(np.prod(spacing))
    print("%s: label %s, classes %s, foreground %.1f mm^3" % (branch, plain.shape, np.unique(plain).tolist(), fg))
    from scipy import ndimage
    counts = np.sort(np.bincount(ndimage.label(plain != 0)[0].ravel())[1:])
    # thresholds that cut between the components that are there (and one above everything)
    vts = [0.5 * float(np.prod(spacing)), 2.0 * fg] + ([(float(counts[-1]) - 0.5) * float(np.prod(spacing))] if counts.size else [])
    for lcc, vt in [(True, None), (False, vts[0])] + [(l, v) for l in (False, True) for v in vts[1:]] + [(True, vts[0])]:
        got, smf = m.evaluate_single_3D(img, largest_component=lcc, volume_threshold=vt, spacing=spacing, **kw)
        ref = _host_filters(plain, lcc, vt, spacing)
        assert got.shape == ref.shape and got.dtype == np.int64 and np.array_equal(got, ref), (lcc, vt)
        assert smf.tobytes() == sm.tobytes()
    if branch == "plain":
        ext = (20, 24, 11)                                      # the input file's size under a Padding transform: smaller on x and z
        got, _ = m.evaluate_single_3D(img, largest_component=True, volume_threshold=vts[0], spacing=spacing, extent=ext)
        cut = plain[:20, :20, :11]
        assert np.array_equal(got, _host_filters(cut, True, vts[0], spacing))

"""-m gpu: the post-processing pipeline on the device (csrc/postprocess.hip, csrc/vnet_post.h, libvnet_post.so) against the rules of
vnet_tensorflow_amd/postprocess.py.  Equality is exact everywhere: every entry point and every step `==` its NumPy / scipy restatement,
on a generated label with planted structure (tests/test_postprocess_host.planted), at the smallest shapes at which each failure mode
can show, past one trip of each capped grid, and on the adversarial union-find shapes of tests/test_hip_components.py re-stated with
two interleaved classes.  Then evaluate, end to end."""
import os
import re

import numpy as np
import pytest
import torch

from tests.test_hip_components import K, PIXDIM, VOLUME, _combs, _serpentine, small_model  # noqa: F401  (small_model: a fixture)
from tests.test_postprocess_host import SP, assert_not_vacuous, planted
from tests.util import g
from vnet_tensorflow_amd import morph, postprocess as PP, prepare_data

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOLUME_MM3 = 1.5 * float(np.prod(SP))              # between one voxel and two: drops the single voxels, keeps the pairs


def _np(t):
    return t.cpu().numpy()


def check_all(label, dev, classes=(1, 2, 3), radius=1, volume=VOLUME_MM3, spacing=SP):
    """Every entry point and every step against its rule, exactly.  Returns the device results."""
    label = np.ascontiguousarray(label, dtype=np.int32)
    classes = list(classes)
    Z = label.shape[2]
    t = g(label, dev, torch.int32)
    out = []
    # vnet_post_class_roots: all classes, a subset in another order, with and without sizes
    for vals in (classes, classes[::-1][:2]):
        roots, sizes = PP.class_roots_device(t, vals, sizes=True)
        ref_r, ref_s = PP.class_roots(label, vals)
        assert roots.dtype == torch.int32 and tuple(roots.shape) == label.shape
        assert np.array_equal(_np(roots), ref_r), "roots differ at %d voxels" % int((_np(roots) != ref_r).sum())
        assert np.array_equal(_np(sizes), ref_s)
        assert torch.equal(PP.class_roots_device(t, vals), roots)
        out += [roots, sizes]
    # vnet_post_filter_components
    for vals in (classes, classes[:1]):
        big = PP.filter_components(t, vals, 0)
        assert big.dtype == torch.int32 and np.array_equal(_np(big), PP.keep_largest(label, vals)), vals
        thr = PP.filter_components(t, vals, 1, volume, PP.voxel_volume(spacing))
        assert np.array_equal(_np(thr), PP.remove_small(label, volume, spacing, vals)), vals
        out += [big, thr]
    # vnet_post_fill_holes
    for c in classes:
        filled = PP.fill_holes_class(t, c)
        assert filled.dtype == torch.int32 and np.array_equal(_np(filled), PP.fill_holes(label, [c])), c
        out.append(filled)
    # vnet_post_not_bits, vnet_post_apply_bits
    bits = morph.select_bits(t, classes[:1])
    inv = PP.not_bits(bits, Z)
    assert np.array_equal(_np(inv), prepare_data.pack_bits(label != classes[0]))
    assert torch.equal(PP.not_bits(inv, Z), bits)
    other = prepare_data.pack_bits(np.random.default_rng(9).random(label.shape) < 0.5)
    applied = PP.apply_bits(t, g(other, dev, torch.int64), classes[0])
    assert np.array_equal(_np(applied), PP.apply_mask(label, prepare_data.unpack_bits(other, Z).astype(bool), classes[0]))
    out += [inv, applied]
    # the steps, through run()
    steps = [PP.KeepLargestComponent(), PP.RemoveSmallComponents(volume), PP.FillHoles(), PP.FillHoles(classes[::-1]),
             PP.Dilate(radius), PP.Erode(radius, classes[:1]), PP.Open(radius), PP.Close(radius)]
    for s in steps:
        got = PP.run([s], t, spacing, classes=classes)
        assert got.dtype == torch.int32 and got.device == t.device
        assert np.array_equal(_np(got), PP.run([s], label, spacing, classes=classes)), s
        out.append(got)
    chain = [PP.KeepLargestComponent([classes[0]]), PP.RemoveSmallComponents(volume), PP.FillHoles(), PP.Close(radius)]
    got = PP.run(chain, t, spacing, classes=classes)
    assert np.array_equal(_np(got), PP.run(chain, label, spacing, classes=classes))
    assert np.array_equal(_np(t), label)                                     # the input is not written
    return out + [got]


# ---- the generated label ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 4, 64), (5, 7, 65), (13, 17, 131)], ids=lambda s: "x".join(map(str, s)))
def test_every_entry_point_and_step(dev, shape):
    lab, inside = planted(shape, seed=0)
    if inside:
        assert_not_vacuous(lab, inside, VOLUME_MM3, SP)                      # before the device runs, from the rules alone
    check_all(lab, dev)
    dense, _ = planted(shape, seed=1, p=0.5)
    check_all(dense, dev, radius=2)
    if shape == (1, 1, 1):
        for v in (0, 1, 2):
            check_all(np.full(shape, v, np.int32), dev, classes=(1, 3))


def test_radii_up_to_eight_and_other_class_values(dev):
    lab, _ = planted((9, 10, 70), seed=5, p=0.1)
    lab = np.where(lab == 3, -7, np.where(lab == 2, 40000, lab)).astype(np.int32)
    t = g(lab, dev, torch.int32)
    for r in (3, 8):
        for step in (PP.Close(r, [40000, -7]), PP.Open(r, [1]), PP.Erode(r, [-7])):
            assert np.array_equal(_np(PP.run([step], t, SP)), PP.run([step], lab, SP)), step
    check_all(lab, dev, classes=(1, 40000, -7))


def _grid_cap():
    """Units one trip of the kernels' grid-stride loops covers, read from the source so that a change of the cap is seen."""
    src = open(os.path.join(ROOT, "vnet_tensorflow_amd", "csrc", "postprocess.hip")).read()
    m = re.search(r"constexpr int PP_BLOCK = (\d+), PP_MAXBLK = (\d+);", src)
    assert m, "postprocess.hip no longer states PP_BLOCK / PP_MAXBLK in one line"
    return int(m.group(1)) * int(m.group(2))


@pytest.mark.parametrize("shape, p", [((9, 251, 517), 0.04), ((1100, 1000, 1), 0.3)], ids=["per voxel 9x251x517", "per word 1100x1000x1"])
def test_volumes_past_the_grid_caps(dev, shape, p):
    """More than one trip of the 4096 x 256 grid: voxels for the per-voxel kernels, words (rows of one voxel) for the per-word ones."""
    assert (int(np.prod(shape)) if shape[2] > 1 else shape[0] * shape[1] * morph.words(shape[2])) > _grid_cap()
    lab, inside = planted(shape, seed=2, p=p)
    if inside:
        assert_not_vacuous(lab, inside, VOLUME_MM3, SP)
    check_all(lab, dev)


# ---- the adversarial union-find shapes, with two interleaved classes ---------------------------------------------------------------------------
def test_row_and_plane_wrap(dev):
    """Linear neighbours that are no face neighbours, (0,0,4) | (0,1,0) across a row end and (0,2,4) | (1,0,0) across a plane end, of
    the same class; the voxels between them in the other class."""
    for a, b in (((0, 0, 4), (0, 1, 0)), ((0, 2, 4), (1, 0, 0))):
        lab = np.full((4, 3, 5), 2, np.int32)
        lab[a] = lab[b] = 1
        assert np.ravel_multi_index(b, lab.shape) - np.ravel_multi_index(a, lab.shape) == 1
        roots = _np(check_all(lab, dev, classes=(1, 2))[0])
        assert roots[a] == np.ravel_multi_index(a, lab.shape) and roots[b] == roots[a] + 1
    lab = np.ones((4, 3, 5), np.int32)
    lab[:, :, 1:4] = 2
    lab[1:3] = 2
    check_all(lab, dev, classes=(1, 2))
    # a run of one class ends where the next class begins, in the middle of a wave and of a row
    lab = np.repeat(np.array([1, 1, 2, 2, 2, 1, 3, 3, 0, 3], np.int32), 13)[None, None, :] * np.ones((2, 3, 1), np.int32)
    roots = _np(check_all(lab, dev)[0])
    assert roots[0, 0, 26] == 26 and roots[0, 0, 65] == 65 and roots[1, 2, 129] == 117


def test_long_chain_both_ways(dev):
    from scipy import ndimage
    path = _serpentine()
    lab = np.where(path != 0, 1, 2).astype(np.int32)                          # the path in class 1, everything around it in class 2
    assert ndimage.label(lab == 1)[1] == 1 and int((lab == 1).sum()) > 200
    for m in (lab, lab[::-1, ::-1, ::-1], lab[:, ::-1, :], lab.transpose(2, 1, 0)):
        m = np.ascontiguousarray(m)
        roots = _np(check_all(m, dev, classes=(1, 2), volume=float((lab == 1).sum()) - 0.5, spacing=(1.0, 1.0, 1.0))[0])
        assert int(roots[m == 1].max()) == int(np.flatnonzero(m.ravel() == 1)[0])


def test_late_merge_of_two_combs(dev):
    from scipy import ndimage
    sep, joined = _combs()
    # both combs in class 1, the slabs between their teeth in class 2: the one voxel joins the combs through a wall of class 2
    for m, n in ((sep, 2), (joined, 1)):
        lab = np.where(m != 0, 1, 2).astype(np.int32)
        assert ndimage.label(lab == 1)[1] == n
        for v in (lab, lab[::-1], lab[:, ::-1, ::-1]):
            v = np.ascontiguousarray(v)
            sizes = _np(check_all(v, dev, classes=(1, 2))[1])
            if n == 1:
                assert int(sizes[v == 1].max()) == int((joined != 0).sum()) == 224
    # the combs as two classes: touching nowhere, and no merge where class 1 meets class 2
    roots = _np(check_all(sep, dev, classes=(1, 2))[0])
    assert len(np.unique(roots[sep == 1])) == 1 and len(np.unique(roots[sep == 2])) == 1


def test_checkerboard_of_two_classes(dev):
    i, j, k = np.indices((6, 6, 6))
    lab = (1 + (i + j + k) % 2).astype(np.int32)
    roots, sizes = check_all(lab, dev, classes=(1, 2), volume=0.5, spacing=(1.0, 1.0, 1.0))[:2]
    assert np.array_equal(_np(roots).ravel(), np.arange(216)) and bool((sizes == 1).all())          # every voxel its own component
    big = _np(PP.filter_components(g(lab, dev, torch.int32), [1, 2], 0))
    assert int((big != 0).sum()) == 2 and big[0, 0, 0] == 1 and big[0, 0, 1] == 2                    # each tie to the first voxel


def test_ties_in_size(dev):
    lab = np.zeros((5, 6, 7), np.int32)
    lab[0, 0, 1:5] = 3                                          # 4 voxels, first voxel 1
    lab[3:5, 3:5, 3] = 3                                        # 4 voxels, first voxel later
    lab[2, 0, 0:3] = 3                                          # 3 voxels
    lab[1, 1:3, 1:3] = 1                                        # another class with a larger count in between
    lab[4, 0, 0:4] = 1
    for m in (lab, np.ascontiguousarray(lab[::-1, ::-1, ::-1])):
        check_all(m, dev, classes=(1, 3), volume=3.5, spacing=(1.0, 1.0, 1.0))
        check_all(m, dev, classes=(1, 3), volume=4.0, spacing=(1.0, 1.0, 1.0))
    big = _np(PP.filter_components(g(lab, dev, torch.int32), [3, 1], 0))
    assert (big[0, 0, 1:5] == 3).all() and int((big == 3).sum()) == 4 and (big[1, 1:3, 1:3] == 1).all() and int((big == 1).sum()) == 4


def test_threshold_equality_is_strict(dev):
    lab = np.zeros((6, 6, 6), np.int32)
    lab[0:2, 0:2, 0:2] = 1                                      # 8 voxels: 8 * 0.125 == 1.0 exactly in double -> dropped
    lab[3:6, 3:6, 5] = 2                                        # 9 voxels: kept
    sp = (0.5, 0.5, 0.5)
    check_all(lab, dev, classes=(1, 2), volume=1.0, spacing=sp)
    thr = _np(PP.run([PP.RemoveSmallComponents(1.0)], g(lab, dev, torch.int32), sp, classes=3))
    assert not (thr == 1).any() and (thr[3:6, 3:6, 5] == 2).all()
    check_all(lab, dev, classes=(1, 2), volume=8 * float(np.prod((0.3, 0.7, 1.1))), spacing=(0.3, 0.7, 1.1))


def test_results_are_reproducible(dev):
    lab, _ = planted((13, 17, 131), seed=4, p=0.3)
    runs = [check_all(lab, dev) for _ in range(3)]
    for other in runs[1:]:
        assert len(other) == len(runs[0])
        for x, y in zip(runs[0], other):
            assert _np(x).tobytes() == _np(y).tobytes()


def test_error_codes_on_the_device(dev):
    from tests.test_postprocess_host import test_error_codes_need_no_device
    from vnet_tensorflow_amd import ops
    from vnet_tensorflow_amd._lib import VnetHipError
    test_error_codes_need_no_device()
    L = PP.lib()
    import ctypes
    vals = (ctypes.c_int * 2)(1, 2)
    lab = torch.ones((5, 4, 3), dtype=torch.int32, device=dev)
    out = torch.zeros((5, 4, 3), dtype=torch.int32, device=dev)
    need = L.vnet_post_filter_components_ws_bytes(5, 4, 3)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    st = ops._thread_stream(lab.device)
    assert L.vnet_post_filter_components(lab.data_ptr(), out.data_ptr(), vals, 2, 1, 1.0, 1.0, 5, 4, 3, ws.data_ptr(), need - 1, st) == -3
    assert L.vnet_post_filter_components(lab.data_ptr(), out.data_ptr(), vals, 2, 1, float("inf"), 1.0, 5, 4, 3, ws.data_ptr(), need, st) == -1
    assert L.vnet_post_fill_holes(lab.data_ptr(), out.data_ptr(), 1, 5, 4, 3, ws.data_ptr(), 5 * 60 - 1, st) == -3
    torch.cuda.synchronize()
    assert int(out.sum()) == 0                                                # nothing was launched
    assert L.vnet_post_filter_components(lab.data_ptr(), out.data_ptr(), vals, 2, 1, 1.0, 1.0, 5, 4, 3, ws.data_ptr(), need, st) == 0
    torch.cuda.synchronize()
    assert int(out.sum()) == 60
    with pytest.raises(VnetHipError, match="int32"):
        PP.run([PP.FillHoles()], lab.to(torch.int64), SP, classes=3)
    with pytest.raises(ValueError, match="class 0"):
        PP.fill_holes_class(lab, 0)


# ---- evaluate, end to end --------------------------------------------------------------------------------------------------------------------
def _steps(plain, spacing):
    from scipy import ndimage
    counts = np.sort(np.bincount(ndimage.label(plain == 1)[0].ravel())[1:])
    volume = (float(counts[len(counts) // 2]) if counts.size else 1.0) * float(np.prod(spacing))       # the median component of class 1 goes
    return [PP.KeepLargestComponent([2]), PP.RemoveSmallComponents(volume), PP.FillHoles(), PP.Close(2)]


@pytest.mark.parametrize("branch", ["plain", "back"])
def test_evaluate_postprocesses_on_the_device(dev, small_model, branch):
    """evaluate_single_3D with a pipeline == the same call without it, then the rules -- on the plain branch (cropped to the volume, and
    to a smaller `extent`) and on the back_size branch, for an array and for a case that lives on the device; on_label sees the same."""
    from vnet_tensorflow_amd import model, resample as R
    m, img = small_model
    kw, spacing = {}, PIXDIM
    if branch == "back":
        kw = dict(back_size=R.output_size(VOLUME, (1.0, 1.0, 1.0), (1.25, 0.8, 1.5)), back_ratio=(1.25, 0.8, 1.5))
    plain, sm = m.evaluate_single_3D(img, **kw)
    steps = _steps(plain, spacing)
    want = PP.run(steps, plain, spacing, classes=K)
    print("%s: label %s, classes %s, %d voxels changed by the pipeline" % (branch, plain.shape, np.unique(plain).tolist(), int((want != plain).sum())))
    for case in (img, torch.from_numpy(img).to(dev)):
        seen = []
        got, smf = m.evaluate_single_3D(case, postprocess=steps, spacing=spacing, on_label=lambda t: seen.append((t.dtype, t.device.type, _np(t))), **kw)
        assert got.shape == want.shape and got.dtype == np.int64 and np.array_equal(got, want)
        assert smf.tobytes() == sm.tobytes()
        assert len(seen) == 1 and seen[0][0] == torch.int32 and seen[0][1] == "cuda" and np.array_equal(seen[0][2], want)
        none, sm0 = m.evaluate_single_3D(case, postprocess=None, spacing=spacing, **kw)
        assert none.tobytes() == plain.tobytes() and sm0.tobytes() == sm.tobytes()
    # the legacy pair first (its 0/1 map), then the pipeline on it
    got, _ = m.evaluate_single_3D(img, largest_component=True, postprocess=steps, spacing=spacing, **kw)
    legacy = model.ExtractLargestConnectedComponents(plain, spacing)
    assert np.array_equal(got, PP.run(steps, legacy.astype(np.int64), spacing, classes=K))
    vt = 0.5 * float(np.prod(spacing))
    got, _ = m.evaluate_single_3D(img, volume_threshold=vt, postprocess=[PP.Dilate(1)], spacing=spacing, **kw)
    assert np.array_equal(got, PP.run([PP.Dilate(1)], model.volume_threshold(plain, vt, spacing).astype(np.int64), spacing, classes=K))
    if branch == "plain":
        ext = (20, 24, 11)                                      # the input file's size under a Padding transform: smaller on x and z
        got, _ = m.evaluate_single_3D(img, postprocess=steps, spacing=spacing, extent=ext)
        assert np.array_equal(got, PP.run(steps, plain[:20, :20, :11], spacing, classes=K))


def test_evaluate_case_reads_the_key(dev, small_model, tmp_path):
    m, img = small_model
    path = tmp_path / "post.yaml"
    path.write_text('postprocess:\n  evaluate:\n    3D:\n      - name: "KeepLargestComponent"\n      - name: "Close"\n        variables:\n          radius: 1\n')
    plain, _ = m.evaluate_case(img, PIXDIM, None, False)
    try:
        m.evaluate_postprocess = str(path)
        seen = []
        got, _ = m.evaluate_case(img, PIXDIM, None, False, on_label=lambda t: seen.append(_np(t)))
    finally:
        m.evaluate_postprocess = None
    want = PP.run(PP.build(str(path)), plain, PIXDIM, classes=K)
    assert np.array_equal(got, want) and len(seen) == 1 and np.array_equal(seen[0], want)
    assert m.evaluate_case(img, PIXDIM, None, False)[0].tobytes() == plain.tobytes()

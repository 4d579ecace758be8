"""BSplineDeformation, the parts that need no GPU: the fp64 restatement (vnet_tensorflow_amd/deform.py: the rules of
include/vnet_hip_deform.h, stated from knowledge of ITK) against known answers, the transform and what the pipeline, the dataset and the
op do with it up to the first launch, and the ledger of the new header."""
import ctypes
import os

import numpy as np
import pytest
import torch

from vnet_tensorflow_amd import data, deform as D, transforms as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "vnet_hip_deform.h")
SPACING = (1.0, 0.8, 1.25)


def _vol(shape, C=None, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(50.0, 20.0, size=tuple(shape) + ((C,) if C else ())).astype(np.float32)


def _x_shift(voxels, sx):
    """Every x coefficient `voxels * sx`, the others 0: a displacement of `voxels` voxels along x wherever the weights sum to 1."""
    coef = np.zeros((3, D.GRID, D.GRID, D.GRID))
    coef[0] = voxels * sx
    return coef.ravel()


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 10, 13, 64])
def test_weights_sum_to_one_and_stay_on_the_grid(n):
    for s in (1.0, 0.8, 1.25, 0.3):
        m, w, valid = D.weights(n, s)
        assert m.shape == (n,) and w.shape == (n, 4) and valid.all()
        assert np.abs(w.sum(axis=1) - 1.0).max() <= 4 * np.finfo(np.float64).eps
        assert (w >= 0).all() and m.min() >= 0 and m.max() + 3 <= D.GRID - 1


def test_constant_shift_known_answer():
    """All x coefficients 2.5 * s_x: image[i] -> (x[i+2] + x[i+3]) / 2, zeros where i + 2.5 >= n - 0.5.  Bound (derived): one float
    rounding, 2^-23 max|x|, plus the displacement's distance from 2.5 voxels (the weights sum to 1 within 4 ulp per axis: below 1e-12
    voxels) times a neighbour difference of at most 2 max|x|, with the same margin the kernel test takes: 6e-12 max|x|."""
    n, sx = 20, 1.25
    x = _vol((n, 5, 4), 2, seed=1) + 100.0
    coef = _x_shift(2.5, sx)
    d = D.displacement((n, 5, 4), (sx, 1.0, 1.0), coef)
    assert np.abs(d[..., 0] / sx - 2.5).max() < 1e-12 and not d[..., 1:].any()
    y = D.linear(x, coef, (sx, 1.0, 1.0))
    assert y.dtype == np.float32 and y.shape == x.shape
    ref = 0.5 * (x[2:n - 1].astype(np.float64) + x[3:].astype(np.float64))
    bound = (2.0 ** -23 + 6e-12) * np.abs(x).max()
    assert np.abs(y[:n - 3] - ref).max() <= bound
    assert not y[n - 3:].any() and (y[:n - 3] > 0).all()


def test_step_label_truncates_to_0_2_4():
    """A 0/4 step under the 2.5-voxel shift: the voxel whose two neighbours straddle the step blends to 0 + d * 4 with d = 0.5 and is
    truncated to 2.  The blend is TRUNCATED, so 2 against 1 hangs on the last bit of the displacement (the weights do not sum to 1
    exactly): the step is placed at a voxel whose displacement is at least 2.5 voxels in double, which this test asserts first."""
    n, sx = 20, 1.25
    coef = _x_shift(2.5, sx)
    c = D.source_index((n, 5, 4), (sx, 1.0, 1.0), coef)[:, 0, 0, 0]
    at = [i for i in range(3, n - 6) if c[i] - i >= 2.5]
    assert at, "no voxel with a displacement of at least 2.5 voxels"
    i = at[0]
    lab = np.zeros((n, 5, 4), dtype=np.int16)
    lab[i + 3:] = 4
    out = D.label(lab, coef, (sx, 1.0, 1.0))
    assert out.dtype == np.int16
    col = out[:, 2, 1]
    assert not col[:i].any() and col[i] == 2 and (col[i + 1:n - 3] == 4).all() and not col[n - 3:].any()
    assert np.array_equal(out, np.broadcast_to(col[:, None, None], out.shape))


def test_zero_coefficients_are_the_identity():
    x = _vol((9, 8, 7), 3, seed=2)
    lab = np.random.default_rng(3).integers(0, 6, size=(9, 8, 7)).astype(np.int32)
    zero = np.zeros(D.PARAMS)
    y = D.linear(x, zero, SPACING)
    assert y.dtype == np.float32 and np.array_equal(y, x)
    assert np.array_equal(D.label(lab, zero, SPACING), lab)
    assert np.array_equal(D.linear(x[..., 0], zero, SPACING), x[..., 0])


def test_truncated_label_never_gains_foreground_and_loses_some():
    """0/1 label, random draw: a voxel is 1 only where every tap with weight is 1, so the foreground is a subset of what rounding the
    same blend to nearest would give (never gains), and a strict one (the border erodes); nothing appears where the blend is 0."""
    shape = (24, 20, 18)
    g = np.ogrid[tuple(slice(0, s) for s in shape)]
    lab = (((g[0] - 12.0) ** 2 + (g[1] - 10.0) ** 2 + (g[2] - 9.0) ** 2) <= 36.0).astype(np.int32)
    coef = np.random.default_rng(5).random(D.PARAMS) * 1.5
    blend = D.linear64(lab, coef, SPACING)
    out = D.label(lab, coef, SPACING)
    assert set(np.unique(out)) == {0, 1}
    assert not (out[blend < 1.0]).any()
    rounded = blend >= 0.5
    assert not (out.astype(bool) & ~rounded).any()
    assert out.sum() < rounded.sum()
    assert out.sum() < lab.sum()                                   # (this draw: the sphere stays inside the volume)


def test_separable_evaluation_equals_the_plain_sum():
    shape = (9, 8, 7)
    coef = np.random.default_rng(7).random(D.PARAMS) * 10
    a, b = D.displacement(shape, SPACING, coef), D.displacement_direct(shape, SPACING, coef)
    assert a.shape == shape + (3,) and np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    # the layout: component a slowest, then z, y, x control indices -- a grid that is 1 in one component moves that component alone
    one = np.zeros((3, D.GRID, D.GRID, D.GRID))
    one[1] = 1.0
    d = D.displacement(shape, SPACING, one.ravel())
    assert np.abs(d[..., 1] - 1.0).max() < 1e-14 and not d[..., 0].any() and not d[..., 2].any()
    # ... and a grid that varies along its LAST index varies along array axis 0 (ITK's x)
    ramp = np.zeros((3, D.GRID, D.GRID, D.GRID))
    ramp[2] = np.arange(D.GRID, dtype=np.float64)[None, None, :]
    d = D.displacement(shape, SPACING, ramp.ravel())[..., 2]
    assert np.abs(d - d[:, :1, :1]).max() < 1e-13 and (np.diff(d[:, 0, 0]) > 0).all()


def test_argument_checks():
    with pytest.raises(ValueError, match="parameters"):
        D.displacement((4, 4, 4), SPACING, np.zeros(10))
    with pytest.raises(ValueError, match="spacing"):
        D.displacement((4, 4, 4), (1.0, 0.0, 1.0), np.zeros(D.PARAMS))
    with pytest.raises(ValueError, match="label"):
        D.label(np.zeros((4, 4, 4), dtype=np.float32), np.zeros(D.PARAMS), SPACING)


# ---- the transform ----------------------------------------------------------------------------------------------------------------------------
def _sample(shape=(12, 10, 9), C=2, seed=11):
    rng = np.random.default_rng(seed)
    return {'image': _vol(shape, C, seed), 'label': rng.integers(0, 3, size=shape).astype(np.int32)}


def test_transform_draws_from_the_generator_it_is_given():
    t = T.BSplineDeformation(randomness=1.5)
    assert t.name == 'BSpline Deformation' and t.device is None and t.loader_safe and T.BSplineDeformation().randomness == 10
    s = _sample()
    a, b, c = t(s, np.random.default_rng(4)), t(s, np.random.default_rng(4)), t(s, np.random.default_rng(5))
    assert np.array_equal(a['image'], b['image']) and np.array_equal(a['label'], b['label'])
    assert not np.array_equal(a['image'], c['image'])
    assert a['image'].dtype == np.float32 and a['image'].shape == s['image'].shape
    assert a['label'].dtype == np.int32 and a['label'].shape == s['label'].shape
    # the draw is rng.random(6591) * randomness, and nothing else is drawn
    rng = np.random.default_rng(4)
    coef = rng.random(D.PARAMS) * 1.5
    assert np.array_equal(a['image'], D.linear(s['image'], coef, (1.0, 1.0, 1.0)))
    assert np.array_equal(a['label'], D.label(s['label'], coef, (1.0, 1.0, 1.0)))
    used = np.random.default_rng(4)
    t(s, used)
    assert used.random() == rng.random()


@pytest.mark.parametrize("bad", [0, -1, 0.0, -2.5, "10", None])
def test_randomness_validation(bad):
    with pytest.raises(RuntimeError, match="Randomness should be non zero values"):
        T.BSplineDeformation(randomness=bad)


def test_randomness_accepts_int_and_float():
    assert T.BSplineDeformation(3).randomness == 3 and T.BSplineDeformation(0.25).randomness == 0.25


def test_spacing_is_read_and_carried_through_run_pipeline():
    s = dict(_sample(), spacing=SPACING)
    tf = [T.BSplineDeformation(2.0), T.Padding([16, 16, 16]), T.RandomCrop([8, 8, 8])]
    out = T.run_pipeline(tf, s, np.random.default_rng(0))
    assert out['spacing'] == SPACING and out['label'].shape == (8, 8, 8)
    one = T.BSplineDeformation(2.0)(s, np.random.default_rng(0))
    assert one['spacing'] == SPACING
    coef = np.random.default_rng(0).random(D.PARAMS) * 2.0
    assert np.array_equal(one['image'], D.linear(s['image'], coef, SPACING))          # the sample's spacing, not (1, 1, 1)
    assert not np.array_equal(one['image'], D.linear(s['image'], coef, (1.0, 1.0, 1.0)))


def test_deterministic_prefix_stops_in_front_of_it():
    tf = [T.StatisticalNormalization(2.5), T.Resample(0.5), T.BSplineDeformation(), T.Padding([16, 16, 16])]
    assert T.deterministic_prefix(tf) == 2
    assert T.deterministic_prefix([T.BSplineDeformation()]) == 0
    assert T.BSplineDeformation in T._RANDOM and T._REGISTRY["BSplineDeformation"] is T.BSplineDeformation


def test_build_pipeline_needs_to_be_asked(tmp_path):
    y = tmp_path / "deform.yaml"
    y.write_text("preprocess:\n  train:\n    3D:\n      - name: ManualNormalization\n        variables:\n          windowMin: 0\n"
                 "          windowMax: 255\n      - name: BSplineDeformation\n        variables:\n          randomness: 4\n"
                 "      - name: RandomCrop\n        variables:\n          output_size: [8, 8, 8]\n")
    for kw in ({}, {"geometry": True}, {"deformation": False}):
        with pytest.raises(NotImplementedError, match="BSplineDeformation"):
            T.build_pipeline(str(y), "train", **kw)
    tf = T.build_pipeline(str(y), "train", deformation=True)
    assert [t.name for t in tf] == ['ManualNormalization', 'BSpline Deformation', 'Random Crop']
    assert tf[1].randomness == 4 and tf[1].device is None
    assert T.build_pipeline(str(y), "train", geometry=True, deformation=True, device="cuda")[1].device == "cuda"
    assert "BSplineDeformation" in T._SITK_ONLY
    for name in ("Reorient", "Invert", "ConfidenceCrop"):
        z = tmp_path / (name + ".yaml")
        z.write_text("preprocess:\n  train:\n    3D:\n      - name: %s\n" % name)
        with pytest.raises(NotImplementedError, match=name):
            T.build_pipeline(str(z), "train", geometry=True, deformation=True)


def test_volume_dataset_accepts_it_on_a_device_and_nothing_else():
    syn = {"Cases": 2, "Shape": [12, 10, 9], "Spacing": list(SPACING)}
    args = ("synthetic", ["a.npy"], "l.npy", [0, 1], (8, 8, 8), 1)
    ds = data.VolumeDataset(*args, synthetic=syn, transforms=[T.BSplineDeformation(2.0, device="cuda"), T.RandomCrop([8, 8, 8])])
    assert ds.transforms[0].device == "cuda"
    with pytest.raises(ValueError, match="NumPy backend"):
        data.VolumeDataset(*args, synthetic=syn, transforms=[T.Resample(0.5, device="cuda")])
    with pytest.raises(ValueError, match="NumPy backend"):
        data.VolumeDataset(*args, synthetic=syn, transforms=[T.BSplineDeformation(2.0, device="cuda"), T.Resample(0.5, device="cuda")])
    # the NumPy backend through the dataset: the random transform is applied on every visit, behind the cached prefix
    ds = data.VolumeDataset(*args, synthetic=syn, seed=3, transforms=[T.ManualNormalization(0, 255), T.BSplineDeformation(2.0), T.RandomCrop([8, 8, 8])])
    (cases, seeds), = ds.epoch_plan()[:1]
    img, lab = ds.make_batch(cases, seeds)
    assert img.shape == (1, 8, 8, 8, 1) and lab.shape == (1, 8, 8, 8, 1) and lab.dtype == np.int32
    assert ds._prepared(cases[0])[1] == 1
    again = ds.make_batch(cases, seeds)
    assert np.array_equal(img, again[0]) and np.array_equal(lab, again[1])


# ---- the op up to the first launch ---------------------------------------------------------------------------------------------------------------
def test_op_shapes_meta_and_refuses_cpu_tensors():
    from vnet_tensorflow_amd import ops
    from vnet_tensorflow_amd._lib import VnetHipError
    coef = np.zeros(D.PARAMS)
    m = ops.bspline_deform(torch.zeros(5, 4, 3, 2, device="meta"), coef, SPACING)
    assert m.device.type == "meta" and tuple(m.shape) == (5, 4, 3, 2) and m.dtype == torch.float32
    m = ops.bspline_deform(torch.zeros(5, 4, 3, dtype=torch.int32, device="meta"), torch.zeros(D.PARAMS, dtype=torch.float64), SPACING, "label")
    assert m.device.type == "meta" and tuple(m.shape) == (5, 4, 3) and m.dtype == torch.int32
    with pytest.raises(VnetHipError, match="bspline_deform"):
        ops.bspline_deform(torch.zeros(5, 4, 3, 2), coef, SPACING)
    with pytest.raises(VnetHipError, match="bspline_deform"):
        ops.bspline_deform(torch.zeros(5, 4, 3, 2, dtype=torch.int32, device="meta"), coef, SPACING, "label")
    with pytest.raises(ValueError):
        ops.bspline_deform(torch.zeros(5, 4, 3, device="meta"), coef, SPACING, "cubic")
    with pytest.raises(ValueError, match="parameters"):
        ops.bspline_deform(torch.zeros(5, 4, 3, device="meta"), np.zeros(12), SPACING)
    with pytest.raises(VnetHipError, match="side_work"):
        with ops.side_work("cpu"):
            pass


def test_error_codes_need_no_device():
    """VNET_E_BADARG (-1) and VNET_E_UNSUPPORTED (-2) before any launch."""
    from vnet_tensorflow_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)
    ok = (5, 4, 3, 1)
    sp = (1.0, 0.8, 1.25)
    for fn in (L.vnet_bspline_deform_f32, L.vnet_bspline_deform_i32):
        assert fn(None, one, *ok, one, *sp, None) == -1 and fn(one, None, *ok, one, *sp, None) == -1 and fn(one, one, *ok, None, *sp, None) == -1
        for pos in range(4):
            for v in (0, -3):
                bad = list(ok)
                bad[pos] = v
                assert fn(one, one, *bad, one, *sp, None) == -1
        for pos in range(3):
            for v in (0.0, -1.0, float("nan"), float("inf")):
                bad = list(sp)
                bad[pos] = v
                assert fn(one, one, *ok, one, *bad, None) == -1
        # more voxels than an int32 index holds
        assert fn(one, one, 2048, 1024, 1024, 1, one, *sp, None) == -2
        assert fn(one, one, 65536, 65536, 1, 1, one, *sp, None) == -2
        assert fn(one, one, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 1, one, *sp, None) == -2
    assert L.vnet_bspline_deform_i32(one, one, 5, 4, 3, 2, one, *sp, None) == -1          # a label map has one channel


# ---- the ledger of include/vnet_hip_deform.h ---------------------------------------------------------------------------------------------------
def test_deform_header_ledger():
    """include/vnet_hip_deform.h beyond tests/test_abi_ledger.py: the loaded library carries the table's argument types; the size of
    the coefficient table is one number in the header and in deform.py."""
    from vnet_tensorflow_amd import _lib
    bound = _lib.lib()
    assert bound.vnet_bspline_deform_f32.argtypes == _lib.SIGNATURES_DEFORM["vnet_bspline_deform_f32"][1]
    assert D.GRID == 13 and D.PARAMS == 6591 and "VNET_BSPLINE_PARAMS (3 * 13 * 13 * 13)" in open(HEADER).read()

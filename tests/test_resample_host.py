"""Resample, the parts that need no GPU: known answers of the fp64 restatement (vnet_tensorflow_amd/resample.py: the rules of
include/vnet_hip_resample.h, stated from knowledge of ITK), the `Resample` transform and the spacing it carries, the reference's own
pipeline settings (tests/golden/pipeline3D_resample.yaml: pipeline/pipeline3D.yaml with voxel_size 0.25 -> 0.5, so that the test volume
stays small) through build_pipeline(geometry=True) and VolumeDataset, the ledger of the new header, and evaluate() over a config whose
pipeline resamples, on device "cpu" up to the first launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

from vnet_tensorflow_amd import data, resample as R, transforms as T

HERE = os.path.dirname(os.path.abspath(__file__))
PIPELINE = os.path.join(HERE, "golden", "pipeline3D_resample.yaml")


def _vol(shape, C=None, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(50.0, 20.0, size=tuple(shape) + ((C,) if C else ())).astype(np.float32)


# ---- restatement known answers -------------------------------------------------------------------------------------------------------
def test_equal_spacing_is_the_identity():
    x = _vol((5, 4, 3), 2)
    assert R.output_size((5, 4, 3), (0.7, 1.0, 2.5), (0.7, 1.0, 2.5)) == (5, 4, 3)
    assert R.ratios((0.7, 1.0, 2.5), (0.7, 1.0, 2.5)) == (1.0, 1.0, 1.0)
    y = R.linear(x, (5, 4, 3), (1.0, 1.0, 1.0))
    assert y.dtype == np.float32 and np.array_equal(y, x)
    lab = np.arange(60, dtype=np.int32).reshape(5, 4, 3)
    assert np.array_equal(R.nearest(lab, (5, 4, 3), (1.0, 1.0, 1.0)), lab)


def test_double_spacing_picks_every_other_voxel():
    x = _vol((8, 6, 4))
    size = R.output_size(x.shape, (1.0, 1.0, 1.0), (2.0, 2.0, 2.0))
    assert size == (4, 3, 2)
    assert np.array_equal(R.linear(x, size, (2.0, 2.0, 2.0)), x[::2, ::2, ::2])


def test_upsampling_clamps_the_upper_neighbour_then_goes_to_zero():
    """n = 4, s = 1, s' = 0.3: 14 outputs per axis; i = 11 (c = 3.3, in (n - 1, n - 0.5)) is x[3] alone, i = 12, 13 (c >= 3.5) are 0."""
    x = _vol((4, 4, 4)) + 100.0                                 # (no zero in the input: a zero in the output is the default value)
    size, r = R.output_size((4, 4, 4), (1.0,) * 3, (0.3,) * 3), R.ratios((1.0,) * 3, (0.3,) * 3)
    assert size == (14, 14, 14)
    y = R.linear(x, size, r)
    assert y[11, 11, 11] == x[3, 3, 3] and y[11, 0, 0] == x[3, 0, 0] and y[0, 11, 0] == x[0, 3, 0] and y[0, 0, 11] == x[0, 0, 3]
    assert not y[12:].any() and not y[:, 12:].any() and not y[:, :, 12:].any()
    assert (y[:12, :12, :12] > 0).all()
    c = 9 * 0.3                                                 # an interior sample, by hand along one axis: 2.6999999999999997
    assert y[9, 0, 0] == np.float32(x[2, 0, 0] + (c - 2.0) * (np.float64(x[3, 0, 0]) - np.float64(x[2, 0, 0])))
    assert y[10, 0, 0] == x[3, 0, 0]                            # 10 * 0.3 == 3.0 in double


def test_nearest_ties_go_up_and_the_last_sample_is_outside():
    """n = 4, s = 1, s' = 0.5: c = 0, 0.5, ..., 3.5 -> floor(c + 0.5) = 0, 1, 1, 2, 2, 3, 3 and c = 3.5 is outside."""
    lab = (np.arange(4, dtype=np.int32) + 1)[:, None, None] * np.ones((1, 4, 4), np.int32)
    size, r = R.output_size((4, 4, 4), (1.0,) * 3, (0.5,) * 3), R.ratios((1.0,) * 3, (0.5,) * 3)
    assert size == (8, 8, 8)
    y = R.nearest(lab, size, r)
    assert y.dtype == np.int32 and list(y[:, 0, 0]) == [1, 2, 2, 3, 3, 4, 4, 0]
    assert not y[:, 7].any() and not y[:, :, 7].any()


def test_linear_ramp_is_reproduced():
    """x = 3 i + 5 j - 2 k + 7 sampled at s' = s / 4 (dyadic: every product is exact): exactly the ramp wherever c <= n - 1."""
    i, j, k = np.meshgrid(np.arange(5), np.arange(4), np.arange(6), indexing="ij")
    x = (3.0 * i + 5.0 * j - 2.0 * k + 7.0).astype(np.float32)
    size = R.output_size(x.shape, (1.0, 2.0, 0.5), (0.25, 0.5, 0.125))
    assert size == (20, 16, 24)
    y = R.linear(x, size, R.ratios((1.0, 2.0, 0.5), (0.25, 0.5, 0.125)))
    ci, cj, ck = np.meshgrid(np.arange(20) * 0.25, np.arange(16) * 0.25, np.arange(24) * 0.25, indexing="ij")
    inside = (ci <= 4) & (cj <= 3) & (ck <= 5)
    assert inside.sum() == 17 * 13 * 21 and np.array_equal(y[inside], (3.0 * ci + 5.0 * cj - 2.0 * ck + 7.0)[inside].astype(np.float32))


def test_size_formula_on_non_integer_products():
    assert R.output_size((5, 4, 3), (0.5, 1.3, 1.0), (0.7, 1.0, 2.5)) == (4, 6, 2)       # 3.57.., 5.2, 1.2 -> ceil
    assert R.output_size((20, 18, 14), (1.0, 0.8, 1.25), (0.5, 0.5, 0.5)) == (40, 29, 35)    # 40, 28.8, 35
    assert R.output_size((3, 3, 3), (1.0, 1.0, 1.0), (3.0, 3.1, 2.9)) == (1, 1, 2)
    assert R.output_size((256, 256, 256), (0.5,) * 3, (0.25,) * 3) == (512, 512, 512)


def test_divisor_and_zero_count():
    vol, cnt = _vol((5, 4, 3), 3), np.random.default_rng(1).integers(1, 9, (5, 4, 3)).astype(np.float32)
    r = (1.4, 0.77, 2.5)
    size = (4, 6, 2)
    assert np.array_equal(R.linear64(vol, size, r, divisor=cnt), R.linear64(vol.astype(np.float64) / cnt[..., None], size, r))
    cnt[0, 0, 0] = 0.0
    y = R.linear64(vol, size, r, divisor=cnt)
    assert np.isfinite(y).all() and not y[0, 0, 0].any()        # output (0, 0, 0) reads the tap (0, 0, 0) alone (d = 0 on every axis)
    with pytest.raises(ValueError):
        R.linear(vol, size, (1.0, 0.0, 1.0))
    with pytest.raises(ValueError):
        R.nearest(cnt, (4, 0, 2), r)


# ---- the transform -----------------------------------------------------------------------------------------------------------------------
def test_resample_arguments_are_the_reference_s():
    assert T.Resample(0.5).voxel_size == (0.5, 0.5, 0.5) and T.Resample([0.25, 0.5, 1.0]).voxel_size == (0.25, 0.5, 1.0)
    assert T.Resample((1.0, 2.0, 3.0)).name == 'Resample'
    with pytest.raises(AssertionError):
        T.Resample(1)                                             # an int is neither float nor a sequence (NiftiDataset3D.py:359)
    with pytest.raises(AssertionError):
        T.Resample([1.0, 1.0])


def test_resample_transform_and_carried_spacing():
    img, lab = _vol((10, 9, 7), 2), np.zeros((10, 9, 7), np.int32)
    lab[3:6, 2:5, 1:4] = 2
    out = T.Resample([0.5, 0.5, 0.5])({'image': img, 'label': lab, 'spacing': (1.0, 0.8, 1.25)}, None)
    assert out['spacing'] == (0.5, 0.5, 0.5) and out['label'].shape == (20, 15, 18) and out['image'].shape == (20, 15, 18, 2)
    assert out['image'].dtype == np.float32 and out['label'].dtype == np.int32 and set(np.unique(out['label'])) == {0, 2}
    assert np.array_equal(out['image'][::2, 0, 0], img[:, 0, 0])
    # no spacing in the sample: (1, 1, 1)
    assert T.Resample(2.0)({'image': img, 'label': lab})['label'].shape == (5, 5, 4)
    # the spacing travels past the transforms that return image and label alone
    tf = [T.Resample(0.5), T.Padding([32, 32, 32]), T.ConfidenceCrop2([16, 16, 16], rand_range=1, probability=1.0)]
    s = T.run_pipeline(tf, {'image': img, 'label': lab, 'spacing': (1.0, 0.8, 1.25)}, np.random.default_rng(0))
    assert s['spacing'] == (0.5, 0.5, 0.5) and s['label'].shape == (16, 16, 16) and s['image'].shape == (16, 16, 16, 2)
    assert T.run_pipeline([T.Padding(4)], {'image': img, 'label': lab}, None)['spacing'] == (1.0, 1.0, 1.0)
    a, b = T.apply_pipeline(tf[:2], img, lab, None, spacing=(1.0, 0.8, 1.25))
    assert b.shape == (32, 32, 32) and np.array_equal(a[:20, :15, :18], out['image']) and not a[20:].any()
    assert T.deterministic_prefix(tf) == 2 and T.deterministic_prefix(tf[:2]) == 2 and T.deterministic_prefix([T.RandomNoise()]) == 0


# ---- the reference's pipeline ----------------------------------------------------------------------------------------------------------
def test_reference_pipeline_builds_and_yields_patchshape_samples():
    for phase, names in (("train", ['StatisticalNormalization', 'Resample', 'Padding', 'Confidence Crop 2', 'Random Noise']),
                         ("test", ['StatisticalNormalization', 'Resample', 'Padding', 'Confidence Crop 2']),
                         ("evaluate", ['StatisticalNormalization', 'Resample', 'Padding'])):
        with pytest.raises(NotImplementedError, match="Resample"):
            T.build_pipeline(PIPELINE, phase)                   # the two-argument call keeps refusing it by name
        assert [t.name for t in T.build_pipeline(PIPELINE, phase, geometry=True)] == names
    tf = T.build_pipeline(PIPELINE, "train", geometry=True)
    assert tf[1].voxel_size == (0.5, 0.5, 0.5) and tf[1].device is None
    syn = {"Cases": 2, "Shape": [20, 18, 14], "Spacing": [1.0, 0.8, 1.25]}
    ds = data.VolumeDataset("synthetic", ["a.npy"], "l.npy", [0, 1, 2], (128, 128, 128), 1, train=True, seed=1, synthetic=syn, transforms=tf)
    batches = list(ds)
    assert len(batches) == 2
    for img, lab in batches:
        assert img.shape == (1, 128, 128, 128, 1) and lab.shape == (1, 128, 128, 128, 1) and lab.dtype == np.int32 and img.dtype == np.float32
    # the deterministic prefix (normalisation, Resample, Padding) was applied once per case and cached on the resampled grid
    sample, n = ds._prepared(0)
    assert n == 3 and sample['spacing'] == (0.5, 0.5, 0.5) and sample['label'].shape == (128, 128, 128)
    assert sample['label'][40:].sum() == 0 and sample['label'][:, 29:].sum() == 0 and sample['label'][:, :, 35:].sum() == 0
    assert sample['label'][:40, :29, :35].any()
    # cached or not, the batches are the same
    ds2 = data.VolumeDataset("synthetic", ["a.npy"], "l.npy", [0, 1, 2], (128, 128, 128), 1, train=True, seed=1, synthetic=syn, transforms=tf,
                             cache=False)
    (cases, seeds), = ds2.epoch_plan()[:1]
    ds.epoch = 0
    ds.rng = np.random.default_rng(1)
    (cases1, seeds1), = ds.epoch_plan()[:1]
    assert (cases, seeds) == (cases1, seeds1)
    a, b = ds.make_batch(cases, seeds), ds2.make_batch(cases, seeds)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for bad in ("Reorient", "Invert", "BSplineDeformation", "ConfidenceCrop"):
        assert bad in T._SITK_ONLY
    with pytest.raises(ValueError, match="NumPy backend"):
        data.VolumeDataset("synthetic", ["a.npy"], "l.npy", [0, 1], (8, 8, 8), 1, synthetic=syn, transforms=[T.Resample(0.5, device="cuda")])


def test_out_of_scope_transforms_stay_refused(tmp_path):
    for name in ("Reorient", "Invert", "BSplineDeformation", "ConfidenceCrop"):
        y = tmp_path / (name + ".yaml")
        y.write_text("preprocess:\n  train:\n    3D:\n      - name: %s\n" % name)
        for geometry in (False, True):
            with pytest.raises(NotImplementedError, match=name):
                T.build_pipeline(str(y), "train", geometry=geometry)


def test_pipelines_without_resample_are_unchanged_by_the_cache():
    tf = [T.StatisticalNormalization(2.5), T.Padding([16, 16, 16]), T.ConfidenceCrop2([16, 16, 16], rand_range=2, probability=0.8), T.RandomNoise()]
    kw = dict(train=True, seed=1, synthetic={"Cases": 4, "Shape": [24, 20, 18]}, transforms=tf)
    ds = data.VolumeDataset("synthetic", ["a.npy"], "l.npy", [0, 1, 2], (16, 16, 16), 2, **kw)
    plan = ds.epoch_plan()
    for cases, seeds in plan:
        img, lab = ds.make_batch(cases, seeds)
        ref_i, ref_l = [], []
        for case, sd in zip(cases, seeds):                       # today's path: the whole pipeline on the raw case, every visit
            image, label = data.synthetic_case([24, 20, 18], 1, 3, 1000 + case)
            sample = {'image': image, 'label': label}
            rng = np.random.default_rng(sd)
            for t in tf:
                sample = t(sample, rng)
            ref_i.append(sample['image'])
            ref_l.append(sample['label'][..., None])
        assert np.array_equal(img, np.stack(ref_i)) and np.array_equal(lab, np.stack(ref_l))


# ---- the ledger of include/vnet_hip_resample.h -----------------------------------------------------------------------------------------
def test_resample_header_ledger():
    """include/vnet_hip_resample.h beyond tests/test_abi_ledger.py: the loaded library carries the table's argument types."""
    from vnet_tensorflow_amd import _lib
    bound = _lib.lib()
    assert bound.vnet_resample_linear.argtypes == _lib.SIGNATURES_RESAMPLE["vnet_resample_linear"][1]


def test_error_codes_need_no_device():
    """VNET_E_BADARG (-1) before any launch: null tensors, sizes < 1, C < 1, ratios that are not finite or not > 0."""
    from vnet_tensorflow_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)
    ok = (2, 3, 4, 5, 6, 7, 1.0, 0.5, 2.0)
    assert L.vnet_resample_linear(None, None, one, 1, *ok, None) == -1 and L.vnet_resample_linear(one, None, None, 1, *ok, None) == -1
    assert L.vnet_resample_nearest_i32(None, one, *ok, None) == -1 and L.vnet_resample_nearest_i32(one, None, *ok, None) == -1
    assert L.vnet_resample_linear(one, None, one, 0, *ok, None) == -1 and L.vnet_resample_linear(one, None, one, -4, *ok, None) == -1
    for pos in range(6):
        for v in (0, -3):
            bad = list(ok)
            bad[pos] = v
            assert L.vnet_resample_linear(one, None, one, 2, *bad, None) == -1 and L.vnet_resample_nearest_i32(one, one, *bad, None) == -1
    for pos in range(6, 9):
        for v in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            bad = list(ok)
            bad[pos] = v
            assert L.vnet_resample_linear(one, None, one, 2, *bad, None) == -1 and L.vnet_resample_nearest_i32(one, one, *bad, None) == -1


def test_op_refuses_cpu_tensors_and_shapes_meta():
    from vnet_tensorflow_amd import ops
    from vnet_tensorflow_amd._lib import VnetHipError
    x = torch.zeros(5, 4, 3, 2)
    with pytest.raises(VnetHipError, match="resample"):
        ops.resample(x, (4, 6, 2), (1.4, 0.77, 2.5))
    with pytest.raises(VnetHipError, match="resample"):
        ops.resample(torch.zeros(5, 4, 3, dtype=torch.int32), (4, 6, 2), (1.4, 0.77, 2.5), mode="nearest")
    with pytest.raises(ValueError):
        ops.resample(x, (4, 6, 2), (1.4, 0.77, 2.5), mode="cubic")
    m = ops.resample(torch.zeros(5, 4, 3, 2, device="meta"), (4, 6, 2), (1.4, 0.77, 2.5))
    assert m.device.type == "meta" and tuple(m.shape) == (4, 6, 2, 2) and m.dtype == torch.float32
    m = ops.resample(torch.zeros(5, 4, 3, dtype=torch.int32, device="meta"), (4, 6, 2), (1.4, 0.77, 2.5), mode="nearest")
    assert m.device.type == "meta" and tuple(m.shape) == (4, 6, 2) and m.dtype == torch.int32


# ---- evaluate over a pipeline that resamples ---------------------------------------------------------------------------------------------
def test_evaluate_config_with_resample_reaches_the_device(tmp_path):
    """evaluate() over the reference's pipeline settings: build_pipeline no longer refuses `Resample`; with the model on "cpu" the run
    gets as far as the first launch (ops.resample on the uploaded volume), which has no CPU fallback."""
    from vnet_tensorflow_amd import model
    from vnet_tensorflow_amd._lib import VnetHipError
    case = tmp_path / "eval" / "case0"
    case.mkdir(parents=True)
    img, _ = data.synthetic_case((10, 9, 7), 1, 2, 3)
    data.write_nifti(str(case / "image.nii"), img[..., 0], (1.0, 0.8, 1.25))
    cfg = {"TrainingSetting": {
        "Data": {"TrainingDataDirectory": str(tmp_path), "TestingDataDirectory": str(tmp_path), "ImageFilenames": ["image.nii"],
                 "LabelFilename": "label.nii"},
        "BatchSize": 1, "PatchShape": [16, 16, 16], "SegmentationClasses": [0, 1], "Epoches": 1, "Pipeline": PIPELINE,
        "Networks": {"Name": "VNet", "Dropout": 0.0, "NumChannel": 4, "NumLevels": 2, "NumCovolutions": [1, 1], "BottomConvolutions": 1},
        "Optimizer": {"Name": "Adam", "InitialLearningRate": 1e-2, "Decay": {"Factor": 0.99, "Steps": 100}},
        "Loss": {"Name": "sorensen"}},
        "EvaluationSetting": {"Data": {"EvaluateDataDirectory": str(tmp_path / "eval"), "ImageFilenames": ["image.nii"]},
                              "CheckpointPath": str(tmp_path / "ckpt"), "Stride": [8, 8, 8], "BatchSize": 1, "ProbabilityOutput": True,
                              "Pipeline": PIPELINE}}
    m = model.image2label(None, cfg, device="cpu", verbose=False)
    m.read_config()
    m.build_model_graph()
    torch.save({"variables": {k: v.detach().clone() for k, v in m.network.state_dict().items()}, "global_step": 0, "start_epoch": 0},
               str(tmp_path / "ckpt"))
    m2 = model.image2label(None, cfg, device="cpu", verbose=False)
    with pytest.raises(VnetHipError, match="resample: tensor on cpu"):
        m2.evaluate()
    # the training side builds the same settings for its loader threads: NumPy backend
    m2.synthetic = {"Cases": 1, "Shape": [10, 9, 7], "Spacing": [1.0, 0.8, 1.25]}
    m2.patch_shape, m2.batch_size = [128, 128, 128], 1
    ds = m2._dataset("synthetic", True)
    assert [t.name for t in ds.transforms][:3] == ['StatisticalNormalization', 'Resample', 'Padding'] and ds.transforms[1].device is None

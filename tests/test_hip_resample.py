"""-m gpu: the resampling kernels (csrc/resample.hip, include/vnet_hip_resample.h) against the fp64 restatement
(vnet_tensorflow_amd/resample.py), and evaluate() over a pipeline that resamples.

The bound of every linear comparison is DERIVED: the kernel blends in double and rounds once to float, so against the restatement's
double it is off by half a float ulp of the result, <= 2^-24 * max|x| (a blend is a convex combination of the taps); the test allows
2^-23 * max|x|.  The two double blends differ by a few 1e-16 relative (contraction of lo + d * (hi - lo) into an fma), far below that.
Nearest neighbour and the known answers are exact."""
import os
import re

import numpy as np
import pytest
import torch

from tests.util import g
from vnet_tensorflow_amd import data, resample as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP = (0.7 / 0.5, 1.0 / 1.3, 2.5 / 1.0)                     # output spacing / source spacing of the 5x4x3 source
DOWN = tuple(1.0 / r for r in UP)
SHAPE = (5, 4, 3)


def _size(shape, ratio):
    return R.output_size(shape, (1.0, 1.0, 1.0), ratio)


def _bound(x):
    return 2.0 ** -23 * float(np.abs(x).max())


def _err(y, ref):
    return float(np.abs(y.cpu().numpy().astype(np.float64) - ref).max())


def _misaligned(a, dev):
    """A contiguous device tensor of a's values whose first byte is 4 past a 16-byte boundary."""
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=dev)
    t = buf[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    return t


# ---- the kernels against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("ratio", [UP, DOWN], ids=["coarser", "finer"])
def test_linear_matches_the_restatement(dev, C, ratio):
    from vnet_tensorflow_amd import ops
    x = np.random.default_rng(C).normal(20.0, 30.0, size=SHAPE + (C,)).astype(np.float32)
    size = _size(SHAPE, ratio)
    ref = R.linear64(x, size, ratio)
    y = ops.resample(g(x, dev), size, ratio)
    assert tuple(y.shape) == size + (C,) and y.dtype == torch.float32
    e = _err(y, ref)
    print("C=%d ratio=%s: max|y - y64| = %.3e, bound %.3e" % (C, ratio, e, _bound(x)))
    assert e <= _bound(x)
    if C == 1:                                                  # a volume without a channel axis is one channel
        assert torch.equal(ops.resample(g(x[..., 0], dev), size, ratio), y[..., 0])


@pytest.mark.parametrize("ratio", [UP, DOWN], ids=["coarser", "finer"])
def test_misaligned_views_take_the_scalar_path(dev, ratio):
    """C = 4 from a base 4 bytes past a 16-byte boundary: not refused, and bit-identical to the aligned (quad) launch -- both paths do
    the same arithmetic per channel.  A misaligned OUTPUT goes through the C ABI (ops.resample allocates its own)."""
    from vnet_tensorflow_amd import _lib, ops
    x = np.random.default_rng(4).normal(20.0, 30.0, size=SHAPE + (4,)).astype(np.float32)
    cnt = np.random.default_rng(5).integers(1, 9, size=SHAPE).astype(np.float32)
    size = _size(SHAPE, ratio)
    aligned = ops.resample(g(x, dev), size, ratio)
    assert g(x, dev).data_ptr() % 16 == 0 and aligned.data_ptr() % 16 == 0
    assert _err(aligned, R.linear64(x, size, ratio)) <= _bound(x)
    assert torch.equal(ops.resample(_misaligned(x, dev), size, ratio), aligned)
    with_div = ops.resample(g(x, dev), size, ratio, divisor=g(cnt, dev))
    assert torch.equal(ops.resample(_misaligned(x, dev), size, ratio, divisor=_misaligned(cnt, dev)), with_div)
    out = _misaligned(np.full(size + (4,), np.nan, np.float32), dev)
    tx = g(x, dev)
    code = _lib.lib().vnet_resample_linear(tx.data_ptr(), None, out.data_ptr(), 4, *SHAPE, *size, *ratio, ops._stream())
    assert code == 0 and torch.equal(out, aligned)


def test_known_answers_on_the_device(dev):
    from vnet_tensorflow_amd import ops
    rng = np.random.default_rng(0)
    for C in (3, 4):                                            # scalar and quad path
        x = rng.normal(50.0, 20.0, size=(8, 6, 4, C)).astype(np.float32)
        assert torch.equal(ops.resample(g(x, dev), (8, 6, 4), (1.0, 1.0, 1.0)), g(x, dev))                     # equal spacing: identity
        assert torch.equal(ops.resample(g(x, dev), (4, 3, 2), (2.0, 2.0, 2.0)), g(x[::2, ::2, ::2], dev))     # s' = 2 s: x[2 i]
        # n = 4, s = 1, s' = 0.3: i = 11 (c = 3.3) is the last voxel alone, i = 12, 13 (c >= 3.5) are 0
        x = (rng.normal(50.0, 20.0, size=(4, 4, 4, C)) + 100.0).astype(np.float32)
        r = R.ratios((1.0,) * 3, (0.3,) * 3)
        y = ops.resample(g(x, dev), (14, 14, 14), r).cpu().numpy()
        assert np.array_equal(y[11, 11, 11], x[3, 3, 3]) and np.array_equal(y[11, 0, 0], x[3, 0, 0]) and np.array_equal(y[0, 0, 11], x[0, 0, 3])
        assert np.array_equal(y[10, 10, 10], x[3, 3, 3])                                                          # 10 * 0.3 == 3.0
        assert not y[12:].any() and not y[:, 12:].any() and not y[:, :, 12:].any() and (y[:12, :12, :12] > 0).all()
        assert np.abs(y - R.linear64(x, (14, 14, 14), r)).max() <= _bound(x)
    # a ramp on a dyadic grid: every product and sum is exact in float
    i, j, k = np.meshgrid(np.arange(5), np.arange(4), np.arange(6), indexing="ij")
    x = (3.0 * i + 5.0 * j - 2.0 * k + 7.0).astype(np.float32)
    assert np.array_equal(ops.resample(g(x, dev), (20, 16, 24), (0.25, 0.25, 0.25)).cpu().numpy(), R.linear(x, (20, 16, 24), (0.25, 0.25, 0.25)))


def test_nearest_equals_the_restatement_ties_included(dev):
    from vnet_tensorflow_amd import ops
    lab = (np.arange(4, dtype=np.int32) + 1)[:, None, None] * np.ones((1, 4, 4), np.int32)
    y = ops.resample(g(lab, dev, torch.int32), (8, 8, 8), (0.5, 0.5, 0.5), mode="nearest").cpu().numpy()
    assert list(y[:, 0, 0]) == [1, 2, 2, 3, 3, 4, 4, 0] and not y[:, 7].any() and not y[:, :, 7].any()        # ties go up, c = 3.5 is outside
    rng = np.random.default_rng(1)
    for shape, ratio in ((SHAPE, UP), (SHAPE, DOWN), ((7, 9, 11), (0.5, 0.25, 1.5)), ((7, 9, 11), (1.0 / 3.0, 2.0, 0.7))):
        lab = rng.integers(1, 7, size=shape).astype(np.int32)
        size = _size(shape, ratio)
        y = ops.resample(g(lab, dev, torch.int32), size, ratio, mode="nearest")
        assert y.dtype == torch.int32 and np.array_equal(y.cpu().numpy(), R.nearest(lab, size, ratio)), (shape, ratio)


@pytest.mark.parametrize("C", [2, 5, 8])
def test_divisor_is_the_count_map(dev, C):
    """resample(vol, divisor=cnt) against the restatement of vol / cnt in fp64 -- same bound: the quotient is formed in double and
    |vol / cnt| <= |vol| for counts >= 1.  A zero count makes the tap 0."""
    from vnet_tensorflow_amd import ops
    rng = np.random.default_rng(10 + C)
    vol = rng.uniform(0.0, 8.0, size=SHAPE + (C,)).astype(np.float32)
    cnt = rng.integers(1, 9, size=SHAPE).astype(np.float32)
    for ratio in (UP, DOWN):
        size = _size(SHAPE, ratio)
        ref = R.linear64(vol.astype(np.float64) / cnt[..., None].astype(np.float64), size, ratio)
        e = _err(ops.resample(g(vol, dev), size, ratio, divisor=g(cnt, dev)), ref)
        print("divisor C=%d ratio=%s: %.3e, bound %.3e" % (C, ratio, e, _bound(vol)))
        assert e <= _bound(vol)
    zero = cnt.copy()
    zero[0, 0, 0] = zero[4, 3, 2] = zero[2, 1, 1] = 0.0
    for ratio in (UP, DOWN):
        size = _size(SHAPE, ratio)
        y = ops.resample(g(vol, dev), size, ratio, divisor=g(zero, dev))
        assert bool(torch.isfinite(y).all()) and not bool(y[0, 0, 0].any())       # output (0, 0, 0) reads the tap (0, 0, 0) alone
        assert _err(y, R.linear64(vol, size, ratio, divisor=zero)) <= _bound(vol)
    allzero = ops.resample(g(vol, dev), _size(SHAPE, DOWN), DOWN, divisor=g(np.zeros(SHAPE, np.float32), dev))
    assert not bool(allzero.any())


def _grid_cap():
    """Units one trip of the kernels' grid-stride loops covers, read from the source so that a change of the cap is seen."""
    src = open(os.path.join(ROOT, "vnet_tensorflow_amd", "csrc", "resample.hip")).read()
    m = re.search(r"constexpr int RS_BLOCK = (\d+), RS_MAXBLK = (\d+);", src)
    assert m, "resample.hip no longer states RS_BLOCK / RS_MAXBLK in one line"
    return int(m.group(1)) * int(m.group(2))


def test_outputs_past_the_grid_cap(dev):
    """More output units than one trip of the grid-stride loop covers, on the quad, the scalar and the nearest kernel."""
    from vnet_tensorflow_amd import ops
    shape, ratio = (30, 28, 26), (0.25, 0.25, 0.25)
    size = _size(shape, ratio)
    assert size == (120, 112, 104) and size[0] * size[1] * size[2] > _grid_cap()
    rng = np.random.default_rng(2)
    for C in (4, 1):
        x = rng.normal(0.0, 100.0, size=shape + (C,)).astype(np.float32)
        assert _err(ops.resample(g(x, dev), size, ratio), R.linear64(x, size, ratio)) <= _bound(x)
    lab = rng.integers(1, 9, size=shape).astype(np.int32)
    assert np.array_equal(ops.resample(g(lab, dev, torch.int32), size, ratio, mode="nearest").cpu().numpy(), R.nearest(lab, size, ratio))


def test_error_codes(dev):
    """Zero or negative sizes, C < 1, a ratio that is not finite or not > 0: VNET_E_BADARG, with real device tensors as well."""
    from tests.test_resample_host import test_error_codes_need_no_device
    from vnet_tensorflow_amd import _lib, ops
    from vnet_tensorflow_amd._lib import VnetHipError
    test_error_codes_need_no_device()
    L = _lib.lib()
    x, y = torch.zeros(SHAPE + (2,), device=dev), torch.zeros((4, 6, 2, 2), device=dev)
    ok = SHAPE + (4, 6, 2) + UP
    assert L.vnet_resample_linear(x.data_ptr(), None, y.data_ptr(), 2, *ok, ops._stream()) == 0
    for pos, v in ((0, 0), (4, -1), (6, 0.0), (7, float("nan")), (8, float("inf")), (6, -1.5)):
        bad = list(ok)
        bad[pos] = v
        assert L.vnet_resample_linear(x.data_ptr(), None, y.data_ptr(), 2, *bad, ops._stream()) == -1
    assert L.vnet_resample_linear(x.data_ptr(), None, y.data_ptr(), 0, *ok, ops._stream()) == -1
    with pytest.raises(VnetHipError, match="VNET_E_BADARG"):
        ops.resample(x, (4, 6, 2), (1.0, float("nan"), 1.0))
    with pytest.raises(VnetHipError, match="expects"):
        ops.resample(x.to(torch.int32), (4, 6, 2), UP)
    torch.cuda.synchronize()


# ---- evaluate() over a pipeline that resamples -------------------------------------------------------------------------------------------------
K = 3
PIXDIM = (1.0, 0.8, 1.25)
VOLUME = (20, 18, 14)


def _evaluate_setup(tmp, pipeline_text, dev):
    from vnet_tensorflow_amd import model
    case = tmp / "eval" / "case0"
    case.mkdir(parents=True)
    img, _ = data.synthetic_case(VOLUME, 1, K, 11)
    data.write_nifti(str(case / "image.nii"), img[..., 0], PIXDIM)
    (tmp / "pipeline.yaml").write_text(pipeline_text)
    cfg = {"TrainingSetting": {
        "Data": {"TrainingDataDirectory": str(tmp), "TestingDataDirectory": str(tmp), "ImageFilenames": ["image.nii"], "LabelFilename": "label.nii"},
        "BatchSize": 1, "PatchShape": [16, 16, 16], "SegmentationClasses": [0, 1, 2], "Epoches": 1,
        "Networks": {"Name": "VNet", "Dropout": 0.0, "NumChannel": 4, "NumLevels": 2, "NumCovolutions": [1, 1], "BottomConvolutions": 1},
        "Optimizer": {"Name": "Adam", "InitialLearningRate": 1e-2, "Decay": {"Factor": 0.99, "Steps": 100}},
        "Loss": {"Name": "sorensen"}},
        "EvaluationSetting": {"Data": {"EvaluateDataDirectory": str(tmp / "eval"), "ImageFilenames": ["image.nii"], "LabelFilename": "label_tf.nii",
                                       "ProbabilityFilename": "probability_tf.nii"},
                              "CheckpointPath": str(tmp / "ckpt"), "Stride": [8, 8, 8], "BatchSize": 4, "ProbabilityOutput": True,
                              "Pipeline": str(tmp / "pipeline.yaml")}}
    torch.manual_seed(3)
    np.random.seed(3)
    m = model.image2label(None, cfg, device=dev, verbose=False)
    m.read_config()
    m.build_model_graph()
    torch.save({"variables": {k: v.detach().cpu().clone() for k, v in m.network.state_dict().items()}, "global_step": 0, "start_epoch": 0},
               str(tmp / "ckpt"))
    m2 = model.image2label(None, cfg, device=dev, verbose=False)
    m2.evaluate()
    label, hdr = data.read_nifti(str(case / "label_tf.nii"))
    probs = [data.read_nifti(str(case / ("probability_tf_%d.nii" % c))) for c in (0, 1, 2)]
    return m2, img, label, hdr, probs


def test_evaluate_resamples_there_and_back(dev, tmp_path):
    """Resample [0.5, 0.5, 0.5] -> Padding 16 on a 20x18x14 volume of spacing (1.0, 0.8, 1.25): the label and the K probability files
    come back on the input's grid with its pixdim, and equal the composition run in the same process on the same bits: the
    device-resampled image, downloaded -> evaluate_single_3D as it was -> the NumPy way back.  Both sides run the same launches, so
    the labels are equal; the composition's probabilities were rounded to float once per tap before its fp64 blend (vol / cnt on the
    host, <= 2^-24 relative) and the product rounds once after it: 2^-23 * max|p| in all."""
    from vnet_tensorflow_amd import transforms as T
    text = ("preprocess:\n  evaluate:\n    3D:\n      - name: Resample\n        variables: {voxel_size: [0.5, 0.5, 0.5]}\n"
            "      - name: Padding\n        variables: {output_size: [16, 16, 16]}\n")
    m, img, label, hdr, probs = _evaluate_setup(tmp_path, text, dev)
    assert label.shape == VOLUME and label.dtype == np.int16 and np.allclose(hdr["pixdim"], PIXDIM)
    for p, h in probs:
        assert p.shape == VOLUME and p.dtype == np.float32 and np.allclose(h["pixdim"], PIXDIM)
    # the composition, on the spacing the FILE carries: pixdim is float32, 0.8 reads back as 0.800000011920929, and with the double 0.8
    # the sample i = 28 of the y axis sits exactly on the tie c = 17.5 = n - 0.5 (outside) instead of just below it (inside)
    spacing = data.volume_spacing(str(tmp_path / "eval" / "case0" / "image.nii"))
    assert spacing == tuple(float(np.float32(v)) for v in PIXDIM)
    s = T.run_pipeline([T.Resample([0.5, 0.5, 0.5], device=dev), T.Padding(16)],
                       {'image': img, 'label': np.zeros(VOLUME, np.int32), 'spacing': spacing}, None)
    assert s['label'].shape == (40, 29, 35) and s['spacing'] == (0.5, 0.5, 0.5)
    lab_t, sm_t = m.evaluate_single_3D(s['image'])
    back = R.ratios(s['spacing'], spacing)
    lab_ref = R.nearest(lab_t, VOLUME, back)
    sm_ref = R.linear64(np.moveaxis(sm_t, 0, -1), VOLUME, back)
    got = np.stack([p for p, _ in probs], axis=-1).astype(np.float64)
    e = float(np.abs(got - sm_ref).max())
    differ = int((label != lab_ref).sum())
    print("evaluate there and back: %d of %d labels differ, max|p - p64| = %.3e, bound %.3e, classes present %s"
          % (differ, label.size, e, _bound(sm_t), np.unique(label).tolist()))
    assert differ == 0
    assert e <= _bound(sm_t)
    assert np.abs(got.sum(-1) - 1.0).max() < 1e-5               # inside the source every blend of softmaxes is a softmax
    # and against the NumPy Resample on the way in, the device one agrees to the kernel's bound
    host = T.Resample([0.5, 0.5, 0.5])({'image': img, 'label': np.zeros(VOLUME, np.int32), 'spacing': spacing})
    assert np.abs(s['image'][:40, :29, :35].astype(np.float64) - host['image']).max() <= _bound(img)


def test_evaluate_without_resample_is_unchanged(dev, tmp_path):
    """A pipeline without Resample takes the path it always took: build_pipeline's two-argument form, apply_pipeline, the window,
    crop to the input's size, vol / cnt on the host -- bit for bit."""
    from vnet_tensorflow_amd import transforms as T
    text = "preprocess:\n  evaluate:\n    3D:\n      - name: Padding\n        variables: {output_size: [24, 24, 24]}\n"
    m, img, label, hdr, probs = _evaluate_setup(tmp_path, text, dev)
    assert label.shape == VOLUME and np.allclose(hdr["pixdim"], PIXDIM)
    tf = T.build_pipeline(str(tmp_path / "pipeline.yaml"), "evaluate")
    image, _ = T.apply_pipeline(tf, img, np.zeros(VOLUME, np.int32), np.random.default_rng(0))
    assert image.shape == (24, 24, 24, 1)
    lab_t, sm_t = m.evaluate_single_3D(image)
    sl = tuple(slice(0, n) for n in VOLUME)
    assert np.array_equal(label, lab_t[sl].astype(np.int16))
    for c, (p, _) in enumerate(probs):
        assert np.array_equal(p, sm_t[c][sl])

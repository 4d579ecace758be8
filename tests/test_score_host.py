"""Scoring a label map against its ground truth, the parts that need no GPU: the NumPy restatements of include/vnet_hip_score.h against
brute force and scipy.ndimage, the rules of vnet_tensorflow_amd/score.py on hand-counted cases, `.nii.gz` on the way in, the ledger of the
header and its error codes before any launch, and Batch_Evaluate's own logic around a stand-in model on "cpu"."""
import csv
import ctypes
import gzip
import os

import numpy as np
import pytest

from vnet_tensorflow_amd import batch_evaluate as BE
from vnet_tensorflow_amd import data
from vnet_tensorflow_amd import score as SC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "vnet_hip_score.h")


# ---- the restatements ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 5, 1024])
def test_label_overlap_restatement_is_brute_force(L):
    rng = np.random.default_rng(L)
    a = rng.integers(-1, L + 1, size=(7, 6, 5)).astype(np.int32)
    b = np.where(rng.random(a.shape) < 0.5, a, rng.integers(-1, L + 1, size=a.shape)).astype(np.int32)
    a.flat[0], a.flat[1], b.flat[1], b.flat[2] = -1, L, L + 5, -7            # (out of range in both maps, once at one voxel)
    got = SC.label_overlap(a, b, L)
    assert got.dtype == np.int64 and got.shape == (L + 1, 3)
    for l in sorted(set(range(min(L, 7))) | {L - 1}):
        assert list(got[l]) == [int(((a == l) & (b == l)).sum()), int((a == l).sum()), int((b == l).sum())]
    assert list(got[L]) == [0, int(((a < 0) | (a >= L)).sum()), int(((b < 0) | (b >= L)).sum())]
    assert got[L, 1] > 0 and got[L, 2] > 0
    assert got[:, 1].sum() == a.size and got[:, 2].sum() == a.size
    with pytest.raises(ValueError):
        SC.label_overlap(a, b, 1025)
    with pytest.raises(ValueError):
        SC.label_overlap(a, b[:-1], L)


@pytest.mark.parametrize("density", [0.05, 0.35, 0.9])
def test_component_shapes_restatement_is_scipy(density):
    from scipy import ndimage
    lab = (np.random.default_rng(int(density * 100)).random((9, 11, 13)) < density).astype(np.int32) * 3
    n, rows, sums = SC.component_shapes(lab, 4096)
    cc, m = ndimage.label(lab != 0)
    assert n == m == len(rows) == len(sums) and rows.dtype == np.int32 and sums.dtype == np.int64
    boxes = ndimage.find_objects(cc)
    com = np.array(ndimage.center_of_mass(lab != 0, cc, np.arange(1, n + 1))).reshape(n, 3)
    for k in range(n):
        where = np.argwhere(cc == k + 1)
        assert rows[k, 1] == len(where) and list(sums[k]) == list(where.sum(0))
        assert list(rows[k, 2:5]) == [s.start for s in boxes[k]] and list(rows[k, 5:8]) == [s.stop - 1 for s in boxes[k]]
        assert np.array_equal(np.rint(com[k] * rows[k, 1]).astype(np.int64), sums[k])
    # a capacity below n: n stays true, the rows are the first ones
    if n > 3:
        n2, r2, s2 = SC.component_shapes(lab, 3)
        assert n2 == n and np.array_equal(r2, rows[:3]) and np.array_equal(s2, sums[:3])
    assert SC.component_shapes(np.zeros((3, 4, 5), np.int32))[0] == 0
    cen = SC.centroids((n, rows, sums), (0.5, 2.0, 1.0))
    assert np.allclose(cen, com * np.array([0.5, 2.0, 1.0]), rtol=0, atol=1e-12)


# ---- overlap measures, hand-counted ------------------------------------------------------------------------------------------------
def test_overlap_measures_hand_counted():
    a = np.zeros((4, 4, 4), np.int32)
    a[:2] = 1
    a[2, :2] = 2                                     # 32 voxels of label 1, 8 of label 2
    assert SC.overlap_measures(SC.label_overlap(a, a, 3)) == (1.0, 1.0)
    b = np.zeros_like(a)
    b[3] = 1                                         # disjoint from a's foreground
    assert SC.overlap_measures(SC.label_overlap(a, b, 3)) == (0.0, 0.0)
    # two labels with known counts: label 1: I = 16, A = 32, B = 24; label 2: I = 4, A = 8, B = 4
    c = np.zeros_like(a)
    c[0] = 1                                         # 16 voxels inside a's label 1
    c[3, :2] = 1                                     # 8 outside
    c[2, 0] = 2                                      # 4 inside a's label 2
    counts = SC.label_overlap(a, c, 3)
    assert counts.tolist() == [[16, 24, 36], [16, 32, 24], [4, 8, 4], [0, 0, 0]]
    dice, jac = SC.overlap_measures(counts)
    assert dice == 2.0 * 20 / (40 + 28) and jac == 20.0 / (40 + 28 - 20)
    # both maps empty: 0 and 0 by rule (ITK divides by zero)
    z = np.zeros_like(a)
    assert SC.overlap_measures(SC.label_overlap(z, z, 2)) == (0.0, 0.0)
    assert "0.0" in SC.overlap_measures.__doc__ and "divides by zero" in SC.overlap_measures.__doc__
    # a label outside [0, L) is foreground of the map that holds it
    d = a.copy()
    d[3] = 7
    dice_d, _ = SC.overlap_measures(SC.label_overlap(a, d, 3))
    assert dice_d == 2.0 * 40 / (40 + 56)


# ---- item scores, hand-placed boxes -------------------------------------------------------------------------------------------------
SHAPE = (24, 24, 32)


def _boxes(*boxes):
    lab = np.zeros(SHAPE, np.int32)
    for (x0, x1), (y0, y1), (z0, z1) in boxes:
        lab[x0:x1 + 1, y0:y1 + 1, z0:z1 + 1] = 1
    return SC.component_shapes(lab)


def test_item_scores_hand_placed():
    sp = (1.0, 1.0, 1.0)
    gt = _boxes(((4, 7), (4, 7), (4, 11)))                       # centroid (5.5, 5.5, 7.5)
    out = _boxes(((6, 9), (6, 9), (4, 11)))                      # centroid (7.5, 7.5, 7.5): distance sqrt(8) = 2.8284...
    hit = SC.item_scores(gt, out, sp, 2.83)
    assert hit == {"TP": 1, "FP": 0, "FN": 0, "Item Sensitivity": 1.0, "Item IoU": 1.0}
    miss = SC.item_scores(gt, out, sp, 2.82)
    assert miss == {"TP": 0, "FP": 1, "FN": 1, "Item Sensitivity": 0.0, "Item IoU": 0.0}
    # the spacing scales the centroids: the same boxes at (1, 1, 2) are no nearer, at (0.5, 0.5, 1) they are
    assert SC.item_scores(gt, out, (0.5, 0.5, 1.0), 1.42)["TP"] == 1 and SC.item_scores(gt, out, (0.5, 0.5, 1.0), 1.41)["TP"] == 0
    # a thin output item (z extent 5 < 6) is dropped, and so is one a single voxel wide in the plane
    thin = _boxes(((4, 7), (4, 7), (4, 8)))
    assert SC.item_scores(gt, thin, sp, 3) == {"TP": 0, "FP": 0, "FN": 1, "Item Sensitivity": 0.0, "Item IoU": 0.0}
    assert SC.item_scores(gt, thin, sp, 3, thickness_threshold=5)["TP"] == 1
    narrow = _boxes(((5, 5), (4, 7), (4, 11)))
    assert SC.item_scores(gt, narrow, sp, 3)["TP"] == 0 and SC.item_scores(gt, narrow, sp, 3, min_inplane=1)["TP"] == 1
    # two ground-truth items share one output item: FP = kept outputs - TP = -1, kept as the reference has it
    two = _boxes(((4, 7), (4, 7), (0, 5)), ((4, 7), (4, 7), (8, 13)))          # centroids z = 2.5 and 10.5
    one = _boxes(((4, 7), (4, 7), (3, 10)))                                      # centroid z = 6.5: 4 away from both
    shared = SC.item_scores(two, one, sp, 4.5)
    assert shared == {"TP": 2, "FP": -1, "FN": 0, "Item Sensitivity": 1.0, "Item IoU": 2.0}
    assert "NEGATIVE" in SC.item_scores.__doc__
    # no ground-truth item
    none = SC.component_shapes(np.zeros(SHAPE, np.int32))
    assert SC.item_scores(none, one, sp, 3) == {"TP": 0, "FP": 1, "FN": 0, "Item Sensitivity": 0.0, "Item IoU": 0.0}
    assert SC.item_scores(none, none, sp, 3) == {"TP": 0, "FP": 0, "FN": 0, "Item Sensitivity": 0.0, "Item IoU": 0.0}
    # min_physical_size drops components of either side: 128 voxels of 0.125 = 16.0
    assert SC.item_scores(gt, out, (0.5, 0.5, 0.5), 2, min_physical_size=16.0)["TP"] == 1
    assert SC.item_scores(gt, out, (0.5, 0.5, 0.5), 2, min_physical_size=16.5) == \
        {"TP": 0, "FP": 0, "FN": 0, "Item Sensitivity": 0.0, "Item IoU": 0.0}
    # an incomplete table is refused
    with pytest.raises(ValueError, match="max_components"):
        lab = np.zeros(SHAPE, np.int32)
        lab[::4, ::4, ::4] = 1
        SC.item_scores(gt, SC.component_shapes(lab, 5), sp, 3)


def test_accuracy_modes_on_arrays():
    rng = np.random.default_rng(2)
    gt = (rng.random((12, 12, 16)) < 0.2).astype(np.int32)
    out = np.where(rng.random(gt.shape) < 0.8, gt, 1 - gt).astype(np.int32)
    d = SC.Accuracy(gt, out)
    assert sorted(d) == ["DICE", "Jaccard"] and d == SC.Accuracy(gt, out, mode=["DICE"])
    i = SC.Accuracy(gt, out, spacing=(1, 1, 2), tolerence=2, mode=("ITEM",))
    assert sorted(i) == sorted(BE.ITEM_COLUMNS)
    both = SC.Accuracy(gt, out, spacing=(1, 1, 2), tolerence=2, mode=["DICE", "ITEM"])
    assert both == dict(d, **i)
    assert both["DICE"] == SC.overlap_measures(SC.label_overlap(gt, out, 2))[0]
    with pytest.raises(ValueError):
        SC.Accuracy(gt, out[:-1])


# ---- .nii.gz ---------------------------------------------------------------------------------------------------------------------------
def test_nii_gz_on_the_way_in(tmp_path):
    vol = np.random.default_rng(0).integers(0, 5, (6, 7, 8)).astype(np.int16)
    plain, packed = str(tmp_path / "label.nii"), str(tmp_path / "label.nii.gz")
    data.write_nifti(plain, vol, (0.5, 0.75, 2.0))
    raw = open(plain, "rb").read()
    with gzip.open(packed, "wb") as f:
        f.write(raw)
    got, ref = data.load_volume(packed), data.load_volume(plain)
    assert got.dtype == ref.dtype and np.array_equal(got, ref) and np.array_equal(got, vol)
    assert data.volume_spacing(packed) == data.volume_spacing(plain) == (0.5, 0.75, 2.0)
    arr, hdr = data.read_nifti(packed)
    assert np.array_equal(arr, vol) and hdr["dim"] == (6, 7, 8)
    # truncated: the compressed stream cut, and a whole stream whose voxel array is short
    cut = str(tmp_path / "cut.nii.gz")
    open(cut, "wb").write(open(packed, "rb").read()[:-40])
    with pytest.raises(ValueError):
        data.load_volume(cut)
    short = str(tmp_path / "short.nii.gz")
    with gzip.open(short, "wb") as f:
        f.write(raw[:-10])
    with pytest.raises(ValueError, match="truncated"):
        data.load_volume(short)
    head = str(tmp_path / "head.nii.gz")
    with gzip.open(head, "wb") as f:
        f.write(raw[:100])
    with pytest.raises(ValueError):
        data.volume_spacing(head)
    with pytest.raises(ValueError, match=r"\.nii\.gz"):
        data.load_volume(str(tmp_path / "label.mha"))


# ---- the ledger of include/vnet_hip_score.h ------------------------------------------------------------------------------------------
def test_score_header_ledger():
    """include/vnet_hip_score.h beyond tests/test_abi_ledger.py: the label cap is one number in the header and in score.py."""
    assert SC.MAX_LABELS == 1024 and "#define VNET_OVERLAP_MAX_LABELS 1024" in open(HEADER).read()


def test_error_codes_need_no_device():
    """VNET_E_BADARG (-1), VNET_E_UNSUPPORTED (-2), VNET_E_WORKSPACE (-3) before any launch, in that order."""
    from vnet_tensorflow_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)
    ok = (one, one, one, 60, 3, None)
    for pos in range(3):
        bad = list(ok)
        bad[pos] = None
        assert L.vnet_label_overlap(*bad) == -1
    assert L.vnet_label_overlap(one, one, one, 0, 3, None) == -1 and L.vnet_label_overlap(one, one, one, 60, 0, None) == -1
    assert L.vnet_label_overlap(one, one, one, 60, 1025, None) == -2 and L.vnet_label_overlap(one, one, one, 2 ** 31, 3, None) == -2
    assert L.vnet_label_overlap(None, one, one, 60, 1025, None) == -1                    # BADARG comes first
    assert L.vnet_cc_shape_ws_bytes(5, 4, 3) == L.vnet_cc_table_ws_bytes(5, 4, 3) == 8 * 60 + 4 * 4096
    assert L.vnet_cc_shape_ws_bytes(0, 4, 3) == 0 and L.vnet_cc_shape_ws_bytes(2048, 1024, 1024) == 0
    ok = (one, one, one, one, 16, 5, 4, 3, one, 1 << 20, None)
    for pos in (0, 1, 2, 3, 8):
        bad = list(ok)
        bad[pos] = None
        assert L.vnet_cc_shape(*bad) == -1
    for pos, v in ((4, 0), (4, -1), (5, 0), (6, -2), (7, 0), (8, ctypes.c_void_p(20))):
        bad = list(ok)
        bad[pos] = v
        assert L.vnet_cc_shape(*bad) == -1
    assert L.vnet_cc_shape(one, one, one, one, 16, 2048, 1024, 1024, one, 1 << 20, None) == -2
    assert L.vnet_cc_shape(one, one, one, one, 16, 5, 4, 3, one, 8 * 60 + 4 * 4096 - 1, None) == -3
    assert L.vnet_cc_shape(one, one, one, one, 16, 2048, 1024, 1024, one, 0, None) == -2      # UNSUPPORTED before WORKSPACE


def test_ops_refuse_cpu_tensors():
    import torch
    from vnet_tensorflow_amd import ops
    from vnet_tensorflow_amd._lib import VnetHipError
    lab = torch.zeros(5, 4, 3, dtype=torch.int32)
    with pytest.raises(VnetHipError, match="label_overlap"):
        ops.label_overlap(lab, lab, 2)
    with pytest.raises(VnetHipError, match="component_shapes"):
        ops.component_shapes(lab)


def test_evaluate_single_3d_takes_the_hook():
    import inspect
    from vnet_tensorflow_amd import model
    p = inspect.signature(model.image2label.evaluate_single_3D).parameters
    assert list(p)[-1] == "on_label" and p["on_label"].default is None


# ---- Batch_Evaluate around a stand-in model --------------------------------------------------------------------------------------------
class StandIn(object):
    """What Batch_Evaluate asks of a model, on "cpu": the label is a function of the image, the loaded checkpoint and the stride, handed
    to the hook as an int32 tensor."""

    def __init__(self, cfg):
        import torch
        self.device = torch.device("cpu")
        self.cfg = cfg
        self.label_classes = cfg["TrainingSetting"]["SegmentationClasses"]
        self.evaluate_image_filenames = ["image.npy"]
        self.loaded, self.calls, self.written = [], [], []
        self.step = None

    def evaluate_pipeline_transforms(self):
        return None, False

    def load_checkpoint(self, path, with_optimizer=True):
        assert with_optimizer is False
        self.loaded.append(path)
        self.step = int(path.rsplit("-", 1)[1])

    def label_of(self, image, step, stride):
        return (image[..., 0] > 0.3 + 0.01 * step + 0.002 * stride[0] - 0.003 * stride[2]).astype(np.int64)

    def evaluate_case(self, image, spacing, tf, regrid, on_label=None):
        import torch
        self.calls.append((self.step, tuple(self.evaluate_stride), self.evaluate_batch))
        label = self.label_of(image, self.step, self.evaluate_stride)
        on_label(torch.from_numpy(label.astype(np.int32)))
        return label, None

    def write_label(self, out, label, spacing):
        self.written.append(out)


def _sweep_folders(tmp_path):
    ck, dat, out = tmp_path / "ckpt", tmp_path / "data", tmp_path / "out"
    ck.mkdir()
    dat.mkdir()
    for name in ("checkpoint-5", "checkpoint-10", "checkpoint-20.index", "checkpoint-20.data-00000-of-00001", "checkpoint-30",
                 "checkpoint-latest", "checkpoint-12.meta", "events.log"):
        (ck / name).write_text("x")
    (ck / "checkpoint-40").mkdir()                    # a directory is no checkpoint
    rng = np.random.default_rng(9)
    for c in ("case_b", "case_a", "no_truth"):
        (dat / c).mkdir()
        img = rng.random((10, 9, 12)).astype(np.float32)
        np.save(str(dat / c / "image.npy"), img)
        if c != "no_truth":
            np.save(str(dat / c / "label.npy"), (img > 0.5).astype(np.int16) * 2)
    (dat / "stray.txt").write_text("x")
    return ck, dat, out


CFG = {"TrainingSetting": {"SegmentationClasses": [0, 2], "PatchShape": [16, 16, 8]}}


@pytest.mark.parametrize("mode", [["DICE"], ["DICE", "ITEM"], ["ITEM"]])
def test_batch_evaluate_around_a_stand_in_model(tmp_path, monkeypatch, capsys, mode):
    ck, dat, out = _sweep_folders(tmp_path)
    assert BE.list_checkpoints(str(ck)) == [(5, str(ck / "checkpoint-5")), (10, str(ck / "checkpoint-10")), (20, str(ck / "checkpoint-20")),
                                            (30, str(ck / "checkpoint-30"))]
    be = BE.Batch_Evaluate(config_json=CFG, model_folder=str(ck), output_folder=str(out), data_folder=str(dat),
                           ground_truth_filename="label.npy", evaluated_filename="label_vnet.npy", stride_layer_min=4, stride_layer_max=6,
                           stride_inplane_min=8, stride_inplane_max=13, patch_size=None, patch_layer=None, step=2, checkpoint_min=6,
                           checkpoint_max=25, batch_size=3, mode=mode, tolerance=2, write_labels=True)
    models = []
    monkeypatch.setattr(BE.Batch_Evaluate, "build_model", lambda self, cfg: models.append(StandIn(cfg)) or models[-1])
    best = be.Execute()
    m, = models                                                                       # built once
    assert m.cfg["TrainingSetting"]["PatchShape"] == [16, 16, 8]                      # None keeps the config's value
    assert [s for s, _ in be.checkpoints()] == [10, 20] and m.loaded == [str(ck / "checkpoint-10"), str(ck / "checkpoint-20")]
    strides = [(8, 4), (8, 6), (10, 4), (10, 6), (12, 4), (12, 6)]
    assert be.strides() == strides and be.cases() == ["case_a", "case_b"]
    assert m.calls == [(s, (a, a, b), 3) for s in (10, 20) for a, b in strides for _ in range(2)]
    assert len(m.written) == 24 and m.written[0] == str(dat / "case_a" / "label_vnet.npy")
    names = sorted(os.listdir(str(out)))
    assert names == sorted("result_checkpoint-%d_stride_inplane-%d_stride_layer-%d.csv" % (s, a, b) for s in (10, 20) for a, b in strides)
    cols = ["Case"] + (["DICE", "Jaccard"] if "DICE" in mode else []) + (BE.ITEM_COLUMNS if "ITEM" in mode else [])
    averages = {}
    for s in (10, 20):
        for a, b in strides:
            path = str(out / ("result_checkpoint-%d_stride_inplane-%d_stride_layer-%d.csv" % (s, a, b)))
            with open(path, newline="") as f:
                rd = csv.DictReader(f, delimiter=",", quotechar="|", quoting=csv.QUOTE_MINIMAL)
                rows = list(rd)
            assert rd.fieldnames == cols and [r["Case"] for r in rows] == ["case_a", "case_b", "average"]
            want = []
            for c in ("case_a", "case_b"):
                img = np.load(str(dat / c / "image.npy"))[..., None]
                gt = data.remap_labels(np.load(str(dat / c / "label.npy")), [0, 2])
                want.append(SC.Accuracy(gt, m.label_of(img, s, [a, a, b]).astype(np.int32), tolerence=2, mode=mode))
            for r, w in zip(rows, want):
                assert {k: float(v) for k, v in r.items() if k != "Case"} == {k: float(v) for k, v in w.items()}
            for k in cols[1:]:
                assert float(rows[2][k]) == float(np.mean([w[k] for w in want])), k
            averages[(s, a, b)] = {k: float(rows[2][k]) for k in cols[1:]}
    first = {"ckpt": "checkpoint-10", "stride_inplane": 8, "stride_layer": 4}
    want_best = []
    for key in ("DICE", "Jaccard"):
        top, res = 0, dict(first)
        if "DICE" in mode:
            for (s, a, b), avg in averages.items():
                if avg[key] > top:
                    top, res = avg[key], {"ckpt": "checkpoint-%d" % s, "stride_inplane": a, "stride_layer": b}
        want_best.append(res)
    assert list(best) == want_best
    printed = capsys.readouterr().out
    assert "Best DICE result: %s" % (want_best[0],) in printed and "Best Jaccard result: %s" % (want_best[1],) in printed
    if "DICE" in mode:
        assert want_best[0] != first                 # (the sweep tells combinations apart)


def test_batch_evaluate_arguments(tmp_path, monkeypatch):
    ck, dat, out = _sweep_folders(tmp_path)
    be = BE.Batch_Evaluate()
    assert (be.stride_layer_min, be.stride_layer_max, be.stride_inplane_min, be.stride_inplane_max, be.step) == (32, 64, 32, 64, 2)
    assert (be.patch_size, be.patch_layer, be.batch_size, be.mode, be.checkpoint_min) == (64, 64, 5, ["DICE"], 1)
    assert (be.ground_truth_filename, be.evaluated_filename) == ("label.nii.gz", "label_vnet.nii.gz")
    assert be.model_folder == os.path.abspath("./tmp/ckpt") and be.data_folder == os.path.abspath("./data")
    be.config_json = CFG
    assert be.config()["TrainingSetting"]["PatchShape"] == [64, 64, 64] and CFG["TrainingSetting"]["PatchShape"] == [16, 16, 8]
    be.patch_size, be.patch_layer = 32, None
    assert be.config()["TrainingSetting"]["PatchShape"] == [32, 32, 8]
    with pytest.raises(AssertionError):
        BE.Batch_Evaluate(step=0)
    # no checkpoint in range: said so, nothing written
    monkeypatch.setattr(BE.Batch_Evaluate, "build_model", lambda self, cfg: StandIn(cfg))
    with pytest.raises(FileNotFoundError, match="checkpoint"):
        BE.Batch_Evaluate(config_json=CFG, model_folder=str(ck), output_folder=str(out), data_folder=str(dat), checkpoint_min=100).Execute()
    # the flags of the reference's main.py, from a real argument list
    a = BE.get_args(["--checkpoint_dir", str(ck), "--data_dir", str(dat), "--output", str(tmp_path), "-cmin", "7", "-slmin", "4", "-slmax", "6",
                     "-spmin", "8", "-spmax", "12", "-ps", "16", "-pl", "8", "-b", "2", "-gt", "label.npy", "-e", "out.npy", "-c", "c.json",
                     "--mode", "DICE", "ITEM", "--tolerance", "2.5", "--gpu", "1"])
    assert (a.checkpoint_min, a.stride_layer_min, a.stride_layer_max, a.stride_inplane_min, a.stride_inplane_max) == (7, 4, 6, 8, 12)
    assert (a.patch_size, a.patch_layer, a.batch, a.mode, a.tolerance, a.gpu) == (16, 8, 2, ["DICE", "ITEM"], 2.5, 1)
    d = BE.get_args(["-cd", str(ck), "-d", str(dat), "-o", str(tmp_path)])
    assert (d.checkpoint_min, d.patch_size, d.batch, d.mode, d.gpu, d.ground_truth_filename) == (10000, 64, 5, ["DICE"], 0, "./3DRA_seg.nii.gz")
    with pytest.raises(SystemExit):
        BE.get_args([])                              # --checkpoint_dir is required, as in the reference

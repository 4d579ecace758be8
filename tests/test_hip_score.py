"""-m gpu: include/vnet_hip_score.h on the device, every output `==` its NumPy restatement (vnet_tensorflow_amd/score.py), then the product
around it: score.Accuracy on device tensors against the arrays, evaluate_single_3D's on_label hook, and one Batch_Evaluate.Execute()
whose CSVs equal the ones built from evaluate()'s written labels scored on the host.

Shapes: (5,7,9) and (33,17,65) are tails that are no multiple of a wave; (104,104,104) = 1 124 864 voxels is one trip past the
4096 x 256 grid cap of the streaming passes."""
import copy
import csv
import os

import numpy as np
import pytest
import torch

from vnet_tensorflow_amd import score as S

pytestmark = pytest.mark.gpu
SHAPES = [(5, 7, 9), (33, 17, 65), (104, 104, 104)]
CAP = 1 << 18                  # room for every component of the largest random mask (the rows past n are zero and read back as such)


def _ids(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


# ---- vnet_label_overlap --------------------------------------------------------------------------------------------------------------
def _overlap_raw(a, b, L, fill, dev):
    """The entry point on an `out` the test pre-fills: int64 [L + 1, 3]."""
    from vnet_tensorflow_amd import _lib
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    out = torch.full(((L + 1) * 3 * 8,), fill, dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().vnet_label_overlap(ta.data_ptr(), tb.data_ptr(), out.data_ptr(), a.size, L, None), "vnet_label_overlap")
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.int64).reshape(L + 1, 3)


@pytest.mark.parametrize("L", [1, 2, 5, 1024])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_label_overlap_is_the_restatement(dev, shape, L):
    from vnet_tensorflow_amd import ops
    rng = np.random.default_rng(L * 7 + shape[0])
    solid = np.full(shape, L - 1, np.int32)                                       # one run per wave: the register combination
    rand_a = rng.integers(0, L, size=shape).astype(np.int32)                      # every lane another label: the LDS counters
    rand_b = np.where(rng.random(shape) < 0.5, rand_a, rng.integers(0, L, size=shape)).astype(np.int32)
    out_a, out_b = rand_a.copy(), rand_b.copy()                                   # labels -1 and L present: row L
    out_a[rng.random(shape) < 0.1], out_b[rng.random(shape) < 0.1] = -1, L
    out_a.flat[0], out_b.flat[0], out_a.flat[-1], out_b.flat[-1] = -1, -1, L, L
    for name, a, b in (("solid", solid, solid), ("solid vs random", solid, rand_b), ("random", rand_a, rand_b), ("out of range", out_a, out_b)):
        want = S.label_overlap(a, b, L)
        got_ff, got_00 = _overlap_raw(a, b, L, 0xFF, dev), _overlap_raw(a, b, L, 0x00, dev)
        assert np.array_equal(got_ff, want), (name, np.argwhere(got_ff != want)[:4])
        assert np.array_equal(got_00, want), name
        assert np.array_equal(ops.label_overlap(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), L), want), name
        assert want[:, 1].sum() == a.size
    assert S.label_overlap(solid, solid, L)[L - 1].tolist() == [solid.size] * 3
    assert S.label_overlap(out_a, out_b, L)[L, 1] > 0


def test_label_overlap_refusals(dev):
    from vnet_tensorflow_amd import ops
    from vnet_tensorflow_amd._lib import VnetHipError
    a = torch.zeros((4, 4, 4), dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        ops.label_overlap(a, a, 1025)
    with pytest.raises(VnetHipError):
        ops.label_overlap(a, a[:2], 2)
    with pytest.raises(VnetHipError):
        ops.label_overlap(a, a.to(torch.int64), 2)


# ---- vnet_cc_shape --------------------------------------------------------------------------------------------------------------------
def _mask(shape, kind):
    if kind == "solid":
        return np.full(shape, 3, np.int32)
    if kind == "empty":
        return np.zeros(shape, np.int32)
    if kind == "comb":
        # teeth along z at every other y of every other plane, all standing on the plane z = 0: one component with voxels in every
        # workgroup's trips, whose runs within a wave are broken at every row
        m = np.zeros(shape, np.int32)
        m[::2, ::2, :] = 1
        m[:, :, 0] = 1
        return m
    return (np.random.default_rng(int(kind * 100) + shape[1]).random(shape) < kind).astype(np.int32) * 2


@pytest.mark.parametrize("kind", [0.05, 0.35, 0.9, "solid", "comb", "empty"], ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_component_shapes_is_the_restatement(dev, shape, kind):
    from vnet_tensorflow_amd import ops
    lab = _mask(shape, kind)
    t = torch.from_numpy(lab).to(dev)
    n, rows, sums = ops.component_shapes(t, CAP)
    wn, wrows, wsums = S.component_shapes(lab, CAP)
    assert n == wn <= CAP
    assert rows.dtype == np.int32 and sums.dtype == np.int64 and np.array_equal(rows, wrows)
    assert np.array_equal(sums, wsums), np.argwhere(sums != wsums)[:4]
    tn, trows = ops.component_table(t, CAP)                                      # the table is vnet_cc_table's, word for word
    assert tn == n and np.array_equal(trows, rows)
    if kind in ("solid", "comb"):
        assert n == 1 and rows[0, 1] == int((lab != 0).sum())
        if kind == "solid":
            assert sums[0].tolist() == [lab.size * (s - 1) // 2 for s in shape]
    if kind == "empty":
        assert n == 0 and rows.shape == (0, 8) and sums.shape == (0, 3)
    again = ops.component_shapes(t, CAP)                                         # integer atomics: identical from run to run
    assert again[0] == n and np.array_equal(again[1], rows) and np.array_equal(again[2], sums)


@pytest.mark.parametrize("shape", SHAPES[:2], ids=_ids)
def test_component_shapes_capacity_below_n(dev, shape):
    """max_components below n: n is still true, the rows are the first ones, and everything past the capacity's rows is zero on the
    device whatever it held before."""
    from vnet_tensorflow_amd import _lib, ops
    lab = _mask(shape, 0.35)
    wn, wrows, wsums = S.component_shapes(lab, 1 << 16)
    cap = 3
    assert wn > cap
    n, rows, sums = ops.component_shapes(torch.from_numpy(lab).to(dev), cap)
    assert n == wn and np.array_equal(rows, wrows[:cap]) and np.array_equal(sums, wsums[:cap])
    # capacity above n on poisoned outputs: the rows and sums past n are written zeros
    cap = wn + 5
    L = _lib.lib()
    X, Y, Z = shape
    need = L.vnet_cc_shape_ws_bytes(X, Y, Z)
    t = torch.from_numpy(lab).to(dev)
    for fill in (0xFF, 0x00):
        ws = torch.full((need,), fill, dtype=torch.uint8, device=dev)
        table = torch.full((cap * 8 * 4,), fill, dtype=torch.uint8, device=dev)
        dsums = torch.full((cap * 3 * 8,), fill, dtype=torch.uint8, device=dev)
        dn = torch.full((4,), fill, dtype=torch.uint8, device=dev)
        _lib.check(L.vnet_cc_shape(t.data_ptr(), dn.data_ptr(), table.data_ptr(), dsums.data_ptr(), cap, X, Y, Z, ws.data_ptr(), need, None),
                   "vnet_cc_shape")
        torch.cuda.synchronize()
        assert int(dn.cpu().numpy().view(np.int32)[0]) == wn
        assert np.array_equal(table.cpu().numpy().view(np.int32).reshape(cap, 8), np.concatenate([wrows, np.zeros((5, 8), np.int32)]))
        assert np.array_equal(dsums.cpu().numpy().view(np.int64).reshape(cap, 3), np.concatenate([wsums, np.zeros((5, 3), np.int64)]))


# ---- Accuracy --------------------------------------------------------------------------------------------------------------------------
def _blobs(shape, seed, n=6):
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape, np.int32)
    for _ in range(n):
        p = [int(rng.integers(0, s - 4)) for s in shape]
        e = [int(rng.integers(2, 5)) for _ in shape]
        lab[p[0]:p[0] + e[0], p[1]:p[1] + e[1], p[2]:p[2] + e[2] + 4] = int(rng.integers(1, 3))
    return lab


@pytest.mark.parametrize("mode", [("DICE",), ("ITEM",), ("DICE", "ITEM")], ids="+".join)
def test_accuracy_on_the_device_is_accuracy_on_the_arrays(dev, mode):
    shape = (33, 17, 65)
    gt = _blobs(shape, 1)
    out = np.roll(_blobs(shape, 1), 1, axis=0)                                   # the same items one voxel along x ...
    out[_blobs(shape, 2, 3) != 0] = 2                                            # ... and three that are not in the ground truth
    for sp, tol in (((1, 1, 1), 3), ((0.4, 0.4, 2.0), 0.5)):
        want = S.Accuracy(gt, out, spacing=sp, tolerence=tol, mode=mode)
        got = S.Accuracy(torch.from_numpy(gt).to(dev), torch.from_numpy(out).to(dev), spacing=sp, tolerence=tol, mode=mode)
        assert got == want and set(got) == ({"DICE", "Jaccard"} if "DICE" in mode else set()) | \
            ({"TP", "FP", "FN", "Item Sensitivity", "Item IoU"} if "ITEM" in mode else set())
    if "ITEM" in mode:
        assert want["TP"] + want["FN"] == S.component_shapes(gt)[0] > 1
    if "DICE" in mode:
        assert 0.0 < want["DICE"] < 1.0
    # more components than the default capacity: asked again with room for all
    many = np.zeros(shape, np.int32)
    many[::2, ::2, ::2] = 1
    assert S.shapes_of(torch.from_numpy(many).to(dev))[0] == 17 * 9 * 33 > S.DEFAULT_COMPONENTS
    if "ITEM" in mode:
        assert S.Accuracy(torch.from_numpy(many).to(dev), torch.from_numpy(gt).to(dev), mode=mode) == S.Accuracy(many, gt, mode=mode)


# ---- evaluate_single_3D(on_label=...) --------------------------------------------------------------------------------------------------
def _config(root=None, **evaluation):
    data = {"TrainingDataDirectory": "", "TestingDataDirectory": "", "ImageFilenames": ["image.npy"], "LabelFilename": "label.npy"}
    return {"TrainingSetting": {"Data": data, "SegmentationClasses": [0, 1], "BatchSize": 1, "PatchShape": [16, 16, 16],
                                "Networks": {"Name": "VNet", "Dropout": 0.0, "NumChannel": 4, "NumLevels": 2,
                                             "NumCovolutions": [1, 2], "BottomConvolutions": 1},
                                "Optimizer": {"Name": "Adam", "InitialLearningRate": 1e-3, "Decay": {"Factor": 0.99, "Steps": 100}},
                                "Loss": {"Name": "sorensen"}},
            "EvaluationSetting": dict({"Stride": [8, 12, 16], "BatchSize": 3}, **evaluation)}


def _model(dev, seed=5, **evaluation):
    from vnet_tensorflow_amd import model as M
    torch.manual_seed(seed)
    np.random.seed(seed)
    m = M.image2label(None, _config(**evaluation), device=dev, verbose=False)
    m.read_config()
    m.build_model_graph()
    return m


EVALUATE_KW = {
    "plain": {},
    "way back": {"back_size": (11, 13, 9), "back_ratio": (2.0, 1.7, 1.4)},
    "filters": {"largest_component": True, "volume_threshold": 3.0, "spacing": (1.0, 0.5, 2.0), "extent": (24, 20, 12)},
    "filters on the way back": {"back_size": (11, 13, 9), "back_ratio": (2.0, 1.7, 1.4), "largest_component": True, "volume_threshold": 3.0,
                                "spacing": (2.0, 1.7, 1.4)},
}


@pytest.mark.parametrize("probabilities", [False, True])
def test_evaluate_single_3d_hands_the_label_over(dev, probabilities):
    """On the array path and the device-case path, with and without the way back and the label filters: the hook sees, once, an int32
    device tensor equal to the returned label, and the returned values are those of a call without the hook."""
    m = _model(dev, ProbabilityOutput=probabilities)
    vol = np.random.default_rng(77).normal(100.0, 50.0, (24, 22, 12, 1)).astype(np.float32)
    for case in (vol, torch.from_numpy(vol).to(dev)):
        for name, kw in EVALUATE_KW.items():
            plain = m.evaluate_single_3D(case, **kw)
            seen = []
            hooked = m.evaluate_single_3D(case, on_label=lambda t: seen.append((t.dtype, t.device.type, t.is_contiguous(), t.cpu().numpy())), **kw)
            assert len(seen) == 1, name
            dtype, where, dense, label = seen[0]
            assert dtype == torch.int32 and where == "cuda" and dense, name
            assert label.shape == hooked[0].shape and np.array_equal(label, hooked[0]), name
            assert hooked[0].dtype == plain[0].dtype and hooked[0].tobytes() == plain[0].tobytes(), name
            assert (hooked[1] is None and plain[1] is None and not probabilities) or hooked[1].tobytes() == plain[1].tobytes(), name


# ---- Batch_Evaluate ----------------------------------------------------------------------------------------------------------------------
def test_batch_evaluate_is_evaluate_scored_on_the_host(dev, tmp_path, capsys):
    """Two checkpoints x two strides x two 24^3 cases, both modes: every CSV holds what evaluate() -- a model of its own per combination,
    the label through a file -- gives when its written labels are scored by the NumPy restatements."""
    from vnet_tensorflow_amd import batch_evaluate as BE, data, model as M
    ck, dat, out = tmp_path / "ckpt", tmp_path / "data", tmp_path / "out"
    ck.mkdir()
    dat.mkdir()
    for seed in (1, 2):
        m = _model(dev, seed=seed)
        torch.save({"variables": {k: v.detach().cpu().clone() for k, v in m.network.state_dict().items()}, "global_step": seed,
                    "start_epoch": 0}, str(ck / ("checkpoint-%d" % seed)))
    (ck / "checkpoint-latest").write_text('model_checkpoint_path: "checkpoint-2"\n')
    truth = {}
    for i, name in enumerate(("case_a", "case_b")):
        (dat / name).mkdir()
        img, lab = data.synthetic_case((24, 24, 24), 1, 2, 40 + i)
        np.save(str(dat / name / "image.npy"), img[..., 0])
        np.save(str(dat / name / "label.npy"), lab.astype(np.int16))
        truth[name] = data.remap_labels(lab, [0, 1])
    cfg = _config()
    mode = ["DICE", "ITEM"]
    be = BE.Batch_Evaluate(config_json=cfg, model_folder=str(ck), output_folder=str(out), data_folder=str(dat),
                           ground_truth_filename="label.npy", evaluated_filename="label_vnet.npy", stride_layer_min=16, stride_layer_max=16,
                           stride_inplane_min=8, stride_inplane_max=12, patch_size=None, patch_layer=None, step=4, checkpoint_min=1,
                           checkpoint_max=2, batch_size=3, mode=mode, tolerance=3, device=dev)
    best = be.Execute()
    assert not [f for f in os.listdir(str(dat / "case_a")) if f.startswith("label_vnet")]           # no file is needed for the score
    combos = [(s, a, 16) for s in (1, 2) for a in (8, 12)]
    assert sorted(os.listdir(str(out))) == sorted("result_checkpoint-%d_stride_inplane-%d_stride_layer-%d.csv" % c for c in combos)
    averages = {}
    for s, a, b in combos:
        ref = copy.deepcopy(cfg)
        ref["EvaluationSetting"].update({"CheckpointPath": str(ck / ("checkpoint-%d" % s)), "Stride": [a, a, b], "BatchSize": 3,
                                         "Data": {"EvaluateDataDirectory": str(dat), "ImageFilenames": ["image.npy"],
                                                  "LabelFilename": "label_tf.npy"}})
        M.image2label(None, ref, device=dev, verbose=False).evaluate()
        want = [S.Accuracy(truth[c], np.load(str(dat / c / "label_tf.npy")).astype(np.int32), tolerence=3, mode=mode) for c in ("case_a", "case_b")]
        with open(str(out / ("result_checkpoint-%d_stride_inplane-%d_stride_layer-%d.csv" % (s, a, b))), newline="") as f:
            rd = csv.DictReader(f, delimiter=",", quotechar="|", quoting=csv.QUOTE_MINIMAL)
            rows = list(rd)
        assert rd.fieldnames == ["Case", "DICE", "Jaccard", "TP", "FP", "FN", "Item Sensitivity", "Item IoU"]
        assert [r["Case"] for r in rows] == ["case_a", "case_b", "average"]
        for r, w in zip(rows, want):
            assert {k: float(v) for k, v in r.items() if k != "Case"} == {k: float(v) for k, v in w.items()}, (s, a, b)
        for k in rd.fieldnames[1:]:
            assert float(rows[2][k]) == float(np.mean([w[k] for w in want]))
        averages[(s, a, b)] = float(rows[2]["DICE"]), float(rows[2]["Jaccard"])
    for which in (0, 1):
        top, res = 0, {"ckpt": "checkpoint-1", "stride_inplane": 8, "stride_layer": 16}
        for (s, a, b), avg in averages.items():
            if avg[which] > top:
                top, res = avg[which], {"ckpt": "checkpoint-%d" % s, "stride_inplane": a, "stride_layer": b}
        assert best[which] == res
    assert "Best DICE result:" in capsys.readouterr().out
    # write_labels: the file evaluate() would write, under evaluated_filename
    be.write_labels, be.checkpoint_min, be.stride_inplane_min = True, 2, 12
    be.Execute()
    for c in ("case_a", "case_b"):
        assert (dat / c / "label_vnet.npy").read_bytes() == (dat / c / "label_tf.npy").read_bytes()

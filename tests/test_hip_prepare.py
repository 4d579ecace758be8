"""-m gpu: a case of evaluate prepared on the device (include/vnet_hip_prepare.h).  The four entry points through the C ABI, on tensors
carved from a guarded arena (tests/guard.py: guard bands checked after every group of launches), against NumPy:
  channel_stats    tier E (==): integer-valued inputs whose sums are exact in fp64 in any order (tests/prepare_data.py), every voxel count
                   and channel count at which the kernel takes another path, a base off a 16-byte boundary, more voxels than one trip of
                   the capped grid.  tier B: general data against math.fsum within the worst-case bound of ANY summation order,
                   (n - 1) * 2^-53 * sum |term|.
  window_intensity == the NumPy restatement for every element (NaN compared as NaN), in place and out of place.
  crop_words       == np.pad-then-slice on a 0xFF-poisoned output.
  argmax_label     == np.argmax.
Then the product: evaluate_single_3D on a device tensor against the same array (bit for bit), and evaluate() with
EvaluationSetting.PrepareOnDevice false and true (byte-identical label files)."""
import math

import numpy as np
import pytest
import torch

from tests import guard
from tests import prepare_data as D
from vnet_tensorflow_amd import prepare as P

pytestmark = pytest.mark.gpu
COUNTS = (1, 2, 63, 65, 257, 4099)
CHANNELS = (1, 2, 3, 4, 5, 8)


class _Abi(object):
    """The C ABI inside a guarded arena: every device pointer handed to the library lies in an arena tensor between two guards."""

    def __init__(self, dev, capacity=64 << 20):
        self.arena = guard.Arena(dev, capacity=capacity, min_guard=1 << 16)
        self.n = 0

    def __enter__(self):
        from vnet_tensorflow_amd import _lib
        self.ctx = guard.guarded(self.arena)
        self.h = self.ctx.__enter__()
        self.L = _lib.lib()
        return self

    def __exit__(self, *exc):
        self.ctx.__exit__(*exc)
        if exc[0] is None:
            self.arena.check()

    def put(self, a, dtype=torch.float32, offset=0, role="in"):
        """`a` as an arena tensor; offset: that many elements into its buffer (a base off the 16-byte boundary)."""
        a = np.ascontiguousarray(a)
        self.n += 1
        flat = np.concatenate([np.zeros(offset, a.dtype), a.reshape(-1)])
        t = self.arena.tensor("t%d" % self.n, flat.shape, dtype, role, torch.as_tensor(flat).to(dtype))
        return t[offset:].view(a.shape)

    def out(self, shape, dtype, offset=0):
        self.n += 1
        size = int(np.prod(shape)) + offset
        return self.arena.tensor("o%d" % self.n, (size,), dtype, "out")[offset:].view(tuple(shape))

    def stats(self, x, pre=None, offset=0):
        from vnet_tensorflow_amd import _lib
        n, C = x.shape
        need = self.L.vnet_channel_stats_ws_bytes(C)
        xt, out, ws = self.put(x, offset=offset), self.out((C, 4), torch.float64), self.h.workspace(need)
        pt = self.put(pre, torch.float64) if pre is not None else None
        _lib.check(self.L.vnet_channel_stats(xt.data_ptr(), pt.data_ptr() if pt is not None else None, out.data_ptr(), n, C, ws.data_ptr(),
                                             need, None), "vnet_channel_stats")
        return out.cpu().numpy()


# ---- channel_stats ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CHANNELS)
def test_channel_stats_tier_e(dev, C):
    with _Abi(dev) as abi:
        for n in COUNTS:
            x = D.tier_e(n, C, 1)
            want = P.channel_stats(x)
            for offset in (0, 1):                    # (one float off the boundary: the one-channel path whatever C is)
                got = abi.stats(x, offset=offset)
                assert np.array_equal(got, want), (n, C, offset, got, want)


def test_channel_stats_past_one_trip_of_the_grid(dev):
    from vnet_tensorflow_amd import ops
    n = ops.STATS_MAX_BLOCKS * 256 + 4099
    assert n <= 2 ** 21
    with _Abi(dev) as abi:
        for C in (1, 4):
            x = D.tier_e(n, C, 2)
            assert np.array_equal(abi.stats(x), P.channel_stats(x)), C


@pytest.mark.parametrize("mapped", [False, True])
def test_channel_stats_tier_b(dev, mapped):
    u = 2.0 ** -53
    with _Abi(dev) as abi:
        for n in (65, 4099):
            for C in (1, 3, 4):
                x = D.tier_b(n, C, 3)
                pre = np.array([[40.0 + c, 300.0 - 7.0 * c] for c in range(C)]) if mapped else None
                got = abi.stats(x, pre)
                mean_dev = got[:, 0] / np.float64(n)
                ref = D.fsum_stats(x, pre, mean=mean_dev)
                for c in range(C):
                    v = x[:, c].astype(np.float64)
                    if mapped:
                        v = (v - pre[c][0]) / pre[c][1]
                    b_sum, b_css = (n - 1) * u * math.fsum(np.abs(v)), (n - 1) * u * ref[c, 1]
                    e_sum, e_css = abs(got[c, 0] - ref[c, 0]), abs(got[c, 1] - ref[c, 1])
                    print("tier B n=%d C=%d c=%d mapped=%d: |sum err| %.3e (bound %.3e)  |css err| %.3e (bound %.3e)"
                          % (n, C, c, mapped, e_sum, b_sum, e_css, b_css))
                    assert e_sum <= b_sum and e_css <= b_css
                    assert got[c, 2] == ref[c, 2] and got[c, 3] == ref[c, 3]


# ---- window_intensity ---------------------------------------------------------------------------------------------------------------
def _window_case(n, C, seed):
    x = np.random.default_rng([seed, n, C]).normal(80.0, 120.0, (n, C)).astype(np.float32)
    prm = np.empty((C, 5))
    for c in range(C):
        a, b = ((0.0, 1.0), (12.5, 3.0))[c % 2]
        wmin = -20.0 + c
        wmax = wmin if c % 3 == 2 else 180.0 + c
        prm[c] = a, b, wmin, (0.0 if wmax == wmin else 255.0 / (wmax - wmin)), float(wmax == wmin)
        special = [wmin, wmax, wmin - 1, wmax + 1, wmin * b + a, wmax * b + a, 0.0, -0.0, 3e38, -3e38, np.nan, np.inf, -np.inf]
        k = min(n, len(special))
        x[:k, c] = np.roll(np.array(special, np.float32), c)[:k]
    return x, prm


@pytest.mark.parametrize("C", CHANNELS)
def test_window_intensity_is_the_restatement(dev, C):
    from vnet_tensorflow_amd import _lib
    with _Abi(dev) as abi:
        for n in COUNTS:
            x, prm = _window_case(n, C, 4)
            with np.errstate(all="ignore"):
                want = P.window_intensity(x, prm)
            pt = abi.put(prm, torch.float64)
            for offset, in_place in ((0, False), (0, True), (1, False), (1, True)):
                xt = abi.put(x, offset=offset, role="inout" if in_place else "in")
                out = xt if in_place else abi.out((n, C), torch.float32, offset)
                _lib.check(abi.L.vnet_window_intensity(xt.data_ptr(), out.data_ptr(), pt.data_ptr(), n, C, None), "vnet_window_intensity")
                got = out.cpu().numpy()
                assert np.array_equal(got, want, equal_nan=True), (n, C, offset, in_place)
                assert np.array_equal(np.signbit(got), np.signbit(want)), (n, C, offset, in_place)
            if n >= 13:
                assert np.isnan(want).any() == bool((prm[:, 4] == 0).any()) and (want == 255.0).any() and (want == 0.0).any()


# ---- crop_words ---------------------------------------------------------------------------------------------------------------------
VOL, PATCH = (7, 6, 9), (4, 3, 5)
WINDOWS = [((1, 2, 3), PATCH), ((5, 2, 3), PATCH), ((1, 4, 3), PATCH), ((1, 2, 6), PATCH), ((5, 4, 6), PATCH), ((6, 5, 8), PATCH),
           ((0, 0, 0), (7, 8, 16)), ((0, 0, 0), VOL)]


@pytest.mark.parametrize("C", [1, 3, 4, 8])
def test_crop_words_is_pad_then_slice(dev, C):
    from vnet_tensorflow_amd import _lib
    rng = np.random.default_rng(C)
    cases = [(rng.normal(0.0, 50.0, VOL + (C,)).astype(np.float32) + 1000.0, s, p) for s, p in WINDOWS]
    cases.append((rng.normal(0.0, 50.0, (3, 5, 2, C)).astype(np.float32) + 1000.0, (0, 0, 0), (4, 4, 4)))
    with _Abi(dev) as abi:
        for x, start, size in cases:
            want = P.crop_window(x, start, size)
            xt = abi.put(x)
            for offset in (0, 1):                    # (a slot one word off the boundary: the one-word path)
                out = abi.out(size + (C,), torch.float32, offset)
                _lib.check(abi.L.vnet_crop_words(xt.data_ptr(), out.data_ptr(), *x.shape, *start, *size, None), "vnet_crop_words")
                assert np.array_equal(out.cpu().numpy(), want), (x.shape, start, size, offset)
        assert not P.crop_window(cases[4][0], *cases[4][1:])[-1].any()           # (the overhang is really zeros in the yardstick)


def test_crop_words_int32_labels(dev):
    from vnet_tensorflow_amd import ops
    from tests.util import g
    lab = np.random.default_rng(0).integers(-5, 300, size=VOL).astype(np.int32)
    x = g(lab, dev, torch.int32)
    for start, size in WINDOWS:
        got = ops.crop_window(x, start, size)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), P.crop_window(lab, start, size)), (start, size)
    with pytest.raises(ValueError):
        ops.crop_window(x, (7, 0, 0), PATCH)
    with pytest.raises(Exception):
        ops.crop_window(x.to(torch.int64), (0, 0, 0), PATCH)


# ---- argmax_label -------------------------------------------------------------------------------------------------------------------
def _argmax_case(n, K, seed):
    rng = np.random.default_rng([seed, n, K])
    x = rng.integers(-3, 3, size=(n, K)).astype(np.float32)                         # small integers: ties in most rows, negatives
    x[rng.random((n, K)) < 0.1] = -0.0
    rows = rng.random(n)
    x[rows < 0.1] = np.float32(-7.25)                                                 # all-equal rows
    nan_rows = np.flatnonzero((rows >= 0.1) & (rows < 0.3))
    x[nan_rows, rng.integers(0, K, size=nan_rows.size)] = np.nan                     # one NaN ...
    x[nan_rows[::2], rng.integers(0, K, size=nan_rows[::2].size)] = np.nan           # ... or two: the first wins
    return x


@pytest.mark.parametrize("K", [1, 2, 3, 5, 32])
def test_argmax_label_is_numpy(dev, K):
    from vnet_tensorflow_amd import _lib
    with _Abi(dev) as abi:
        for n in (1, 63, 65, 4097):
            x = _argmax_case(n, K, 6)
            want = np.argmax(x, axis=-1).astype(np.int32)
            for offset in (0, 1):
                xt, out = abi.put(x, offset=offset), abi.out((n,), torch.int32)
                _lib.check(abi.L.vnet_argmax_label(xt.data_ptr(), out.data_ptr(), n, K, None), "vnet_argmax_label")
                assert np.array_equal(out.cpu().numpy(), want), (n, K, offset)
            if n == 4097 and K > 1:
                assert np.isnan(x).any() and len(np.unique(want)) > 1
                assert np.array_equal(torch.argmax(torch.from_numpy(x), -1).numpy(), want)


# ---- evaluate_single_3D on a device tensor ------------------------------------------------------------------------------------------
def _model(dev, **evaluation):
    from vnet_tensorflow_amd import model as M
    cfg = {"TrainingSetting": {"Data": {"TrainingDataDirectory": "", "TestingDataDirectory": "", "ImageFilenames": ["i.npy"],
                                        "LabelFilename": "l.npy"},
                               "SegmentationClasses": [0, 1], "BatchSize": 1, "PatchShape": [16, 16, 16],
                               "Networks": {"Name": "VNet", "Dropout": 0.0, "NumChannel": 4, "NumLevels": 2,
                                            "NumCovolutions": [1, 2], "BottomConvolutions": 1},
                               "Optimizer": {"Name": "Adam", "InitialLearningRate": 1e-3, "Decay": {"Factor": 0.99, "Steps": 100}},
                               "Loss": {"Name": "sorensen"}},
           "EvaluationSetting": dict({"Stride": [8, 12, 16], "BatchSize": 3, "ProbabilityOutput": True}, **evaluation)}
    torch.manual_seed(5)
    m = M.image2label(None, cfg, device=dev, verbose=False)
    m.read_config()
    m.build_model_graph()
    return m


def _same_bits(a, b):
    return all((x is None and y is None) or (x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()) for x, y in zip(a, b))


EVALUATE_KW = {
    "plain": {},
    "way back": {"back_size": (11, 13, 9), "back_ratio": (2.0, 1.7, 1.4)},
    "filters": {"largest_component": True, "volume_threshold": 3.0, "spacing": (1.0, 0.5, 2.0), "extent": (24, 20, 12)},
    "filters on the way back": {"back_size": (11, 13, 9), "back_ratio": (2.0, 1.7, 1.4), "largest_component": True, "volume_threshold": 3.0,
                                "spacing": (2.0, 1.7, 1.4)},
}


def test_evaluate_single_3d_on_a_device_tensor(dev, monkeypatch):
    """A 24x22x12 volume under a 16^3 patch, stride (8, 12, 16), batches of 3: the z axis is shorter than the patch (zero fill), the y
    axis is no multiple of the stride (a clamped last window), four windows leave a last batch of one, which is run twice.  The device
    tensor takes the same windows in the same batches through the same kernels: label and probabilities equal bit for bit -- after the
    array path has agreed with itself bit for bit."""
    from vnet_tensorflow_amd import model as M
    m = _model(dev)
    vol = np.random.default_rng(77).normal(100.0, 50.0, (24, 22, 12, 1)).astype(np.float32)
    on_dev = torch.from_numpy(vol).to(dev)
    for name, kw in EVALUATE_KW.items():
        first, again = m.evaluate_single_3D(vol, **kw), m.evaluate_single_3D(vol, **kw)
        assert _same_bits(first, again), "%s: the array path does not agree with itself bit for bit" % name

        def refuse(_):
            raise AssertionError("the device path cut a window on the host")
        with monkeypatch.context() as mp:
            mp.setattr(M, "prepare_batch", refuse)
            got = m.evaluate_single_3D(on_dev, **kw)
        assert isinstance(got[0], np.ndarray) and got[0].dtype == np.int64 and got[1].dtype == np.float32
        assert _same_bits(first, got), name
        assert first[0].shape == (kw.get("back_size") or ((24, 20, 12) if "extent" in kw else (24, 22, 12)))
    assert np.array_equal(on_dev.cpu().numpy(), vol)                                  # (the case itself is not written)
    m.evaluate_probability_output = False
    assert m.evaluate_single_3D(on_dev)[1] is None
    with pytest.raises(Exception, match="device case"):
        m.evaluate_single_3D(on_dev.to(torch.float64))


# ---- evaluate() with EvaluationSetting.PrepareOnDevice ------------------------------------------------------------------------------
CASE = (12, 10, 9)
PIPELINES = {
    "manual": ("      - name: ManualNormalization\n        variables: {windowMin: -50, windowMax: 250}\n"
               "      - name: Resample\n        variables: {voxel_size: [0.5, 0.5, 0.5]}\n"
               "      - name: Padding\n        variables: {output_size: [16, 24, 16]}\n"),
    "statistical": ("      - name: StatisticalNormalization\n        variables: {sigma: 2.5}\n"
                    "      - name: Resample\n        variables: {voxel_size: [0.5, 0.5, 0.5]}\n"
                    "      - name: Padding\n        variables: {output_size: [16, 24, 16]}\n"),
    "flip": ("      - name: ManualNormalization\n        variables: {windowMin: -50, windowMax: 250}\n"
             "      - name: RandomFlip\n        variables: {axes: [true, false, true]}\n"
             "      - name: Padding\n        variables: {output_size: [16, 24, 16]}\n"),
}


def _evaluate(tmp, name, image, on_device, dev):
    """evaluate() of a one-case directory of .npy files under a pipeline YAML written here: the bytes of the label file."""
    from vnet_tensorflow_amd import model
    root = tmp / ("%s_%d" % (name, on_device))
    case = root / "eval" / "case0"
    case.mkdir(parents=True)
    np.save(str(case / "image.npy"), image)
    (root / "pipeline.yaml").write_text("preprocess:\n  evaluate:\n    3D:\n" + PIPELINES[name])
    cfg = {"TrainingSetting": {
        "Data": {"TrainingDataDirectory": str(root), "TestingDataDirectory": str(root), "ImageFilenames": ["image.npy"], "LabelFilename": "label.npy"},
        "BatchSize": 1, "PatchShape": [16, 16, 16], "SegmentationClasses": [0, 1, 2], "Epoches": 1,
        "Networks": {"Name": "VNet", "Dropout": 0.0, "NumChannel": 4, "NumLevels": 2, "NumCovolutions": [1, 1], "BottomConvolutions": 1},
        "Optimizer": {"Name": "Adam", "InitialLearningRate": 1e-2, "Decay": {"Factor": 0.99, "Steps": 100}},
        "Loss": {"Name": "sorensen"}},
        "EvaluationSetting": {"Data": {"EvaluateDataDirectory": str(root / "eval"), "ImageFilenames": ["image.npy"], "LabelFilename": "label_tf.npy"},
                              "CheckpointPath": str(tmp / "ckpt"), "Stride": [8, 8, 8], "BatchSize": 3,
                              "Pipeline": str(root / "pipeline.yaml"), "PrepareOnDevice": bool(on_device)}}
    if not (tmp / "ckpt").exists():                  # one set of weights for every run of a test
        torch.manual_seed(3)
        np.random.seed(3)
        m = model.image2label(None, cfg, device=dev, verbose=False)
        m.read_config()
        m.build_model_graph()
        torch.save({"variables": {k: v.detach().cpu().clone() for k, v in m.network.state_dict().items()}, "global_step": 0,
                    "start_epoch": 0}, str(tmp / "ckpt"))
    model.image2label(None, cfg, device=dev, verbose=False).evaluate()
    label = np.load(str(case / "label_tf.npy"))
    assert label.shape == image.shape and label.dtype == np.int16
    return (case / "label_tf.npy").read_bytes()


@pytest.mark.parametrize("name", ["manual", "statistical"])
def test_evaluate_prepares_on_the_device(dev, tmp_path, monkeypatch, name):
    """The label file of evaluate() is the same bytes with PrepareOnDevice false and true: ManualNormalization needs no statistics, and
    on a tier-E volume the device's sums are NumPy's.  With the switch on nothing is cut, normalised or padded on the host."""
    from vnet_tensorflow_amd import model as M, ops, transforms as T
    if name == "manual":
        image = np.random.default_rng(1).normal(100.0, 80.0, CASE).astype(np.float32)
    else:
        image = D.tier_e(int(np.prod(CASE)), 1, 9).reshape(CASE)
    host = _evaluate(tmp_path, name, image, False, dev)
    calls = []
    for fn in ("channel_stats", "window_intensity", "crop_window", "argmax_label"):
        real = getattr(ops, fn)
        monkeypatch.setattr(ops, fn, lambda *a, _r=real, _n=fn, **k: (calls.append(_n), _r(*a, **k))[1])

    def refuse(*a, **k):
        raise AssertionError("PrepareOnDevice: host work on the volume")
    monkeypatch.setattr(M, "prepare_batch", refuse)
    monkeypatch.setattr(T, "_window", refuse)
    monkeypatch.setattr(T.Padding, "__call__", refuse)
    assert _evaluate(tmp_path, name, image, True, dev) == host
    assert calls.count("channel_stats") == (1 if name == "statistical" else 0) and calls.count("window_intensity") == 1
    assert calls.count("argmax_label") == 1 and calls.count("crop_window") >= 9          # Padding + 8 windows + the duplicated batch


def test_evaluate_keeps_the_host_path_for_other_pipelines(dev, tmp_path, monkeypatch):
    """A RandomFlip in the pipeline: prepare_on_device declines, the switch changes nothing."""
    from vnet_tensorflow_amd import ops
    image = np.random.default_rng(2).normal(100.0, 80.0, (18, 17, 12)).astype(np.float32)
    host = _evaluate(tmp_path, "flip", image, False, dev)
    monkeypatch.setattr(ops, "crop_window", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device path taken")))
    assert _evaluate(tmp_path, "flip", image, True, dev) == host

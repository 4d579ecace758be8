"""The training pipeline's random tail on device-resident cases, the parts that need no GPU: the index methods of the two crops against
their __call__ (same generator, same window), plan_tail, the Philox restatement against the published known-answer vectors, the
statistics of the restated noise, the ledger of include/vnet_hip_sample.h and its error codes before any launch."""
import ctypes
import os

import numpy as np
import pytest

from vnet_tensorflow_amd import sample as S
from vnet_tensorflow_amd import transforms as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "vnet_hip_sample.h")
SHAPE = (40, 36, 44)
SEEDS = 200


def blob_and_islands(shape=SHAPE, seed=5, islands=12):
    """One solid blob (off centre, small enough to leave windows without any label) plus small islands, labels 1..3."""
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape, np.int32)
    g = np.ogrid[tuple(slice(0, s) for s in shape)]
    c = [s * 0.6 for s in shape]
    lab[sum((a - b) ** 2 for a, b in zip(g, c)) <= (min(shape) / 6.0) ** 2] = 1
    for _ in range(islands):
        p = [int(rng.integers(0, s - 2)) for s in shape]
        lab[p[0]:p[0] + int(rng.integers(1, 3)), p[1]:p[1] + int(rng.integers(1, 3)), p[2]:p[2] + int(rng.integers(1, 3))] = int(rng.integers(2, 4))
    return lab


def _labels():
    return {"blob": blob_and_islands(), "empty": np.zeros(SHAPE, np.int32), "full": np.ones(SHAPE, np.int32)}


LABELS = _labels()
IMAGE = np.random.default_rng(11).normal(100.0, 30.0, SHAPE + (2,)).astype(np.float32)
TABLES = {k: S.component_table(v) for k, v in LABELS.items()}


def _same_window(t, name, seed):
    lab = LABELS[name]
    calls = []

    def table():
        calls.append("t")
        return TABLES[name]
    ref = t({'image': IMAGE, 'label': lab}, np.random.default_rng(seed))
    rng = np.random.default_rng(seed)
    start = t.start_index(lab.shape, rng, table, lambda s, n, lo, hi: S.window_count(lab, s, n, lo, hi))
    sl = tuple(slice(a, a + n) for a, n in zip(start, t.output_size))
    assert np.array_equal(ref['image'], IMAGE[sl]) and ref['image'].dtype == np.float32, (name, seed, start)
    assert np.array_equal(ref['label'], lab[sl]), (name, seed, start)
    # the generator stands where __call__ left it: whatever follows the crop in the pipeline draws the same
    again = np.random.default_rng(seed)
    t({'image': IMAGE, 'label': lab}, again)
    assert rng.integers(0, 2 ** 62) == again.integers(0, 2 ** 62), (name, seed)
    return start


@pytest.mark.parametrize("name", sorted(LABELS))
@pytest.mark.parametrize("empty_region", [False, True])
@pytest.mark.parametrize("probability", [0.0, 0.5, 1.0])
def test_confidence_crop2_start_index_is_call(name, empty_region, probability):
    if empty_region and name == "full" and probability < 1.0:
        return          # RandomEmptyRegion never ends on a map without an empty window (the reference's loop, kept)
    t = T.ConfidenceCrop2([16, 12, 20], rand_range=[5, 3, 32], probability=probability, random_empty_region=empty_region)
    starts = set()
    for seed in range(SEEDS):
        starts.add(tuple(_same_window(t, name, seed)))
    assert len(starts) > 20 or (name == "full" and probability == 1.0 and len(starts) > 5)


@pytest.mark.parametrize("name", sorted(LABELS))
def test_random_crop_start_index_is_call(name):
    for t in (T.RandomCrop([16, 12, 20], drop_ratio=0.1, min_pixel=1), T.RandomCrop([16, 12, 20], drop_ratio=0.5, min_pixel=40),
              T.RandomCrop([16, 12, 20], drop_ratio=0.0, min_pixel=0)):
        if name == "empty" and t.drop_ratio == 0.0 and t.min_pixel > 0:
            continue
        for seed in range(SEEDS):
            _same_window(t, name, seed)


def test_tail_draw_follows_the_transforms():
    """crop, flip and the draw in front of the noise: the same generator state as the NumPy transforms up to RandomNoise."""
    lab = LABELS["blob"]
    crop, flip = T.ConfidenceCrop2([16, 12, 20], 4, 0.5), T.RandomFlip([True, False, True])
    plan = T.plan_tail([crop, flip, T.RandomNoise(3)])
    flips = set()
    for seed in range(60):
        ref = flip(crop({'image': IMAGE, 'label': lab}, a := np.random.default_rng(seed)), a)
        start, mask, sigma, nseed = plan.draw(lab.shape, b := np.random.default_rng(seed), lambda: TABLES["blob"],
                                              lambda s, n, lo, hi: S.window_count(lab, s, n, lo, hi))
        img, l = S.patch(IMAGE, lab, start, crop.output_size, mask)
        assert mask in (0, 5) and sigma == 3.0 and 0 <= nseed < 2 ** 64
        assert np.array_equal(ref['image'], img) and np.array_equal(ref['label'], l)
        assert nseed == int(a.integers(0, 2 ** 64, dtype=np.uint64))
        flips.add(mask)
    assert flips == {0, 5}


def test_plan_tail():
    crop2, crop, flip, noise = T.ConfidenceCrop2(8, 32, 0.8), T.RandomCrop(8), T.RandomFlip([True]), T.RandomNoise()
    p = T.plan_tail([crop2, noise])                           # the reference's train tail (pipeline3D.yaml)
    assert p.crop is crop2 and p.flip is None and p.noise is noise
    p = T.plan_tail([crop2])                                  # its test tail
    assert p.crop is crop2 and p.flip is None and p.noise is None
    p = T.plan_tail([crop, flip, noise])
    assert p.crop is crop and p.flip is flip and p.noise is noise
    assert T.plan_tail([crop, flip]).flip is flip
    for bad in ([], [noise, crop2], [flip, crop2], [crop2, noise, flip], [crop2, crop], [crop2, flip, flip], [noise],
                [T.BSplineDeformation(), crop2, noise], [crop2, noise, T.Padding(8)]):
        assert T.plan_tail(bad) is None, bad
    # through the reference's own YAML schema
    full = [T.StatisticalNormalization(2.5), T.Padding(8), crop2, noise]
    n = T.deterministic_prefix(full)
    assert n == 2 and T.plan_tail(full[n:]).noise is noise


def test_philox_known_answers():
    """Philox4x32-10 known-answer vectors of Random123 (Salmon et al., SC'11; kat_vectors): zeros, ones, digits of pi."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = tuple(int(v[0]) for v in S.philox4x32_10(ctr, key))
        assert got == want, (ctr, [hex(v) for v in got])
    # vectorised over the counter: the same words as one call each
    many = S.philox4x32_10((np.arange(5, dtype=np.uint32), np.zeros(5, np.uint32), np.zeros(5, np.uint32), np.zeros(5, np.uint32)), (7, 9))
    for i in range(5):
        assert tuple(int(v[0]) for v in S.philox4x32_10((i, 0, 0, 0), (7, 9))) == tuple(int(w[i]) for w in many)


def test_restated_noise_statistics():
    N = 1 << 20
    z = S.normal(0x1234567890ABCDEF, N)
    assert z.shape == (N,) and np.isfinite(z).all()
    assert abs(z.mean()) <= 5.0 / np.sqrt(N)
    assert abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / N)
    assert np.abs(z).max() <= np.sqrt(2 * 24 * np.log(2.0))
    # a function of (seed, element index) alone
    assert np.array_equal(S.normal(0x1234567890ABCDEF, 37, first=1001), z[1001:1038])
    assert not np.array_equal(S.normal(0x1234567890ABCDEE, 64), z[:64])
    assert not np.array_equal(S.normal(0x1234567890ABCDEF ^ (1 << 40), 64), z[:64])            # the key's upper half counts


def test_component_table_restatement():
    from scipy import ndimage
    lab = LABELS["blob"]
    n, rows = TABLES["blob"]
    cc, m = ndimage.label(lab != 0)
    assert n == m == rows.shape[0] and n > 5 and rows.dtype == np.int32
    for k in (0, n // 2, n - 1):
        where = np.argwhere(cc == k + 1)
        assert rows[k, 0] == np.flatnonzero(cc.ravel() == k + 1)[0] and rows[k, 1] == len(where)
        assert list(rows[k, 2:5]) == list(where.min(0)) and list(rows[k, 5:8]) == list(where.max(0))
    assert np.all(np.diff(rows[:, 0]) > 0)
    assert TABLES["empty"][0] == 0 and TABLES["empty"][1].shape == (0, S.ROW)
    assert TABLES["full"][0] == 1 and list(TABLES["full"][1][0]) == [0, lab.size, 0, 0, 0] + [s - 1 for s in SHAPE]


def test_dataset_keeps_the_loader_path_for_other_tails(capsys):
    from vnet_tensorflow_amd import data
    syn = {"Cases": 2, "Shape": [12, 10, 9]}
    args = ("synthetic", ["a.npy"], "l.npy", [0, 1], (8, 8, 8), 1)
    ds = data.VolumeDataset(*args, synthetic=syn, transforms=[T.Padding(8), T.RandomNoise(), T.RandomCrop(8)], device_tail="cuda")
    assert ds.device_tail is None and "loader path" in capsys.readouterr().out
    (cases, seeds), = ds.epoch_plan()[:1]
    img, lab = ds.make_batch(cases, seeds)
    assert isinstance(img, np.ndarray) and img.shape == (1, 8, 8, 8, 1)
    ds = data.VolumeDataset(*args, synthetic=syn, transforms=[T.Padding(8), T.RandomCrop(8)])
    assert ds.device_tail is None and capsys.readouterr().out == ""
    with pytest.raises(ValueError, match="PatchShape"):
        data.VolumeDataset(*args, synthetic=syn, transforms=[T.Padding(8), T.RandomCrop(6)], device_tail="cuda")


def _stand_ins(monkeypatch):
    """ops.side_work / component_table / window_count / sample_patch on CPU tensors through the restatements: the dataset's own logic
    (plan, cache, evictions, slots) without a device."""
    import contextlib
    import torch
    from vnet_tensorflow_amd import ops

    @contextlib.contextmanager
    def side_work(device):
        yield None

    def component_table(label, max_components=4096, ws=None):
        n, rows = S.component_table(label.numpy())
        return n, rows[:max_components]

    def sample_patch(image, label, start, patch, flip, sigma, seed, out_image, out_label):
        img, lab = S.patch(image.numpy(), label.numpy(), start, patch, flip, sigma, seed)
        out_image.copy_(torch.from_numpy(img.astype(np.float32)))
        out_label.copy_(torch.from_numpy(lab.reshape(tuple(out_label.shape)).copy()))
    monkeypatch.setattr(ops, "side_work", side_work)
    monkeypatch.setattr(ops, "component_table", component_table)
    monkeypatch.setattr(ops, "window_count", lambda label, s, n, lo, hi: S.window_count(label.numpy(), s, n, lo, hi))
    monkeypatch.setattr(ops, "sample_patch", sample_patch)
    monkeypatch.setattr(ops._lib, "lib", lambda: type("L", (), {"vnet_cc_table_ws_bytes": staticmethod(lambda X, Y, Z: 8 * X * Y * Z + 16384)})())


@pytest.mark.parametrize("crop", ["confidence", "random"])
def test_dataset_device_path_is_the_numpy_dataset_through_stand_ins(monkeypatch, crop):
    """VolumeDataset(device_tail=...) with the device entry points replaced by their restatements: the batches of the two paths are equal
    bit for bit (no noise in the tail), with room for every case and with a budget of one case (evictions); and a Prefetcher hands the
    batches on as they are."""
    import torch
    from vnet_tensorflow_amd import data
    _stand_ins(monkeypatch)

    def make(**kw):
        first = T.ConfidenceCrop2([8, 8, 8], rand_range=3, probability=0.5) if crop == "confidence" else T.RandomCrop([8, 8, 8], 0.2, 30)
        tf = [T.ManualNormalization(0, 255), first, T.RandomFlip([True, False, True])]
        return data.VolumeDataset("synthetic", ["a.npy", "b.npy"], "l.npy", [0, 1], (8, 8, 8), 2, train=True, seed=5,
                                  synthetic={"Cases": 6, "Shape": [20, 18, 22]}, transforms=tf, **kw)
    case_bytes = 20 * 18 * 22 * 4 * 3
    for budget in (16 << 30, case_bytes * 3 // 2):
        host, on_dev = make(), make(device_tail="cpu", device_cache_bytes=budget)
        assert on_dev.device_tail == torch.device("cpu") and on_dev._tail_at == 1
        for epoch in range(2):
            ref = list(host)
            got = list(data.Prefetcher(on_dev, depth=2, workers=2)) if epoch else list(on_dev)
            assert len(ref) == len(got) == 3
            for (ri, rl), (gi, gl) in zip(ref, got):
                assert isinstance(gi, torch.Tensor) and gi.dtype == torch.float32 and gl.dtype == torch.int32 and not gi.is_pinned()
                assert gi.numpy().tobytes() == ri.tobytes() and np.array_equal(gl.numpy(), rl)
        st = on_dev.device_stats
        if budget < 16 << 30:
            assert st["evictions"] >= 6 and len(on_dev._dev_cache) == 1 and st["host_samples"] == 0
        else:
            assert st["uploads"] == 6 and st["evictions"] == 0 and st["host_samples"] == 0
    # a budget below one case, a table capacity below a case's components: the NumPy path, into the same batch
    for kw in ({"device_cache_bytes": 100}, {"max_components": 0}):
        host, on_dev = make(), make(device_tail="cpu", **kw)
        (ri, rl), (gi, gl) = next(iter(host)), next(iter(on_dev))
        if crop == "confidence" or "device_cache_bytes" in kw:
            assert on_dev.device_stats["host_samples"] == 2 and on_dev.device_stats["uploads"] == 0
        assert gi.numpy().tobytes() == ri.tobytes() and np.array_equal(gl.numpy(), rl)


def test_config_switch_is_off_by_default(tmp_path):
    from tests.test_host import _config
    from vnet_tensorflow_amd.model import image2label
    m = image2label(None, _config(tmp_path), device="cpu", verbose=False)
    m.read_config()
    assert m.sample_on_device is False and m.device_cache_gb == 16.0
    m = image2label(None, _config(tmp_path, SampleOnDevice=True, DeviceCacheGB=0.5), device="cpu", verbose=False)
    m.read_config()
    assert m.sample_on_device is True and m.device_cache_gb == 0.5


# ---- the op up to the first launch, error codes ---------------------------------------------------------------------------------------
def test_ops_refuse_cpu_tensors():
    import torch
    from vnet_tensorflow_amd import ops
    from vnet_tensorflow_amd._lib import VnetHipError
    lab = torch.zeros(5, 4, 3, dtype=torch.int32)
    with pytest.raises(VnetHipError, match="component_table"):
        ops.component_table(lab)
    with pytest.raises(VnetHipError, match="window_count"):
        ops.window_count(lab, (0, 0, 0), (1, 1, 1), 1, 255)
    with pytest.raises(VnetHipError, match="sample_patch"):
        ops.sample_patch(torch.zeros(5, 4, 3, 1), lab, (0, 0, 0), (2, 2, 2), 0, 0.0, 0, torch.zeros(2, 2, 2, 1), torch.zeros(2, 2, 2, dtype=torch.int32))


def test_error_codes_need_no_device():
    """VNET_E_BADARG (-1), VNET_E_UNSUPPORTED (-2), VNET_E_WORKSPACE (-3) before any launch, in that order."""
    from vnet_tensorflow_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)
    assert L.vnet_cc_table_ws_bytes(5, 4, 3) == 8 * 60 + 4 * 4096 and L.vnet_cc_table_ws_bytes(0, 4, 3) == 0
    assert L.vnet_cc_table_ws_bytes(2048, 1024, 1024) == 0
    ok = (one, one, one, 16, 5, 4, 3, one, 1 << 20, None)
    for pos in (0, 1, 2, 7):
        bad = list(ok)
        bad[pos] = None
        assert L.vnet_cc_table(*bad) == -1
    for pos, v in ((3, 0), (3, -1), (4, 0), (5, -2), (6, 0), (7, ctypes.c_void_p(20))):
        bad = list(ok)
        bad[pos] = v
        assert L.vnet_cc_table(*bad) == -1
    assert L.vnet_cc_table(one, one, one, 16, 2048, 1024, 1024, one, 1 << 20, None) == -2
    assert L.vnet_cc_table(one, one, one, 16, 5, 4, 3, one, 8 * 60 + 4 * 4096 - 1, None) == -3
    w = (one, one, 5, 4, 3, 1, 1, 1, 2, 2, 2, 1, 255, None)
    assert L.vnet_window_count(None, *w[1:]) == -1 and L.vnet_window_count(one, None, *w[2:]) == -1
    for pos, v in ((2, 0), (5, -1), (5, 4), (8, 0), (8, 5), (9, 4), (10, 3)):
        bad = list(w)
        bad[pos] = v
        assert L.vnet_window_count(*bad) == -1, (pos, v)
    assert L.vnet_window_count(one, one, 2048, 1024, 1024, 0, 0, 0, 1, 1, 1, 1, 255, None) == -2
    s = (one, one, one, one, 5, 4, 3, 2, 1, 1, 1, 4, 3, 2, 0, 1.0, 7, None)
    for pos in range(4):
        bad = list(s)
        bad[pos] = None
        assert L.vnet_sample_patch(*bad) == -1
    for pos, v in ((4, 0), (7, 0), (8, -1), (8, 2), (11, 5), (12, 0), (14, 8), (14, -1), (15, -1.0), (15, float("nan")), (15, float("inf"))):
        bad = list(s)
        bad[pos] = v
        assert L.vnet_sample_patch(*bad) == -1, (pos, v)
    assert L.vnet_sample_patch(one, one, one, one, 2048, 1024, 1024, 1, 0, 0, 0, 1, 1, 1, 0, 0.0, 0, None) == -2


# ---- the ledger of include/vnet_hip_sample.h ----------------------------------------------------------------------------------------------
def test_sample_header_ledger():
    """include/vnet_hip_sample.h beyond tests/test_abi_ledger.py: the width of a table row is one number in the header and in sample.py."""
    assert S.ROW == 8 and "#define VNET_CC_ROW 8" in open(HEADER).read()

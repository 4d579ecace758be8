"""-m gpu: the training pipeline's random tail on device-resident cases (include/vnet_hip_sample.h) against its NumPy restatements
(vnet_tensorflow_amd/sample.py): the component table exactly, window counts exactly, the sample bit for bit without noise and within the
derived bound with it; VolumeDataset(device_tail=...) against the NumPy dataset bit for bit, evictions included; and
image2label.train() with TrainingSetting.SampleOnDevice from two loader threads across the capture of the step graph."""
import threading

import numpy as np
import pytest
import torch

from tests.test_sample_host import blob_and_islands
from tests.util import g

pytestmark = pytest.mark.gpu
VOLUME, PATCH = (40, 36, 44), (16, 12, 20)
SEED = 0x9E3779B97F4A7C15


def _bernoulli():
    return (np.random.default_rng(3).random((33, 31, 37)) < 0.35).astype(np.int32)


def _past_one_grid():
    """112x96x100 = 1 075 200 voxels, more than the 4096 x 256 threads of a full grid: 512-voxel chunks.  Every fourth z-row is solid and
    the plane z = 0 ties the rows together: ONE component with voxels in every chunk; isolated single voxels sit in the rows between."""
    lab = np.zeros((112, 96, 100), np.int32)
    lab[:, ::4, :] = 1
    lab[:, :, 0] = 1
    pick = np.random.default_rng(6).random((56, 24, 49)) < 0.02
    lab[::2, 2::4, 2::2][pick] = 3
    return lab


TABLE_CASES = {
    "bernoulli 33x31x37": (_bernoulli, 4096),
    "bernoulli 33x31x37 cap16": (_bernoulli, 16),
    "blob and islands 40x36x44": (blob_and_islands, 4096),
    "empty": (lambda: np.zeros(VOLUME, np.int32), 64),
    "full": (lambda: np.full(VOLUME, 7, np.int32), 64),
    "past one grid 112x96x100": (_past_one_grid, 4096),
}


@pytest.mark.parametrize("cid", sorted(TABLE_CASES))
def test_component_table_is_the_restatement(dev, cid):
    from vnet_tensorflow_amd import ops, sample as S
    make, cap = TABLE_CASES[cid]
    lab = make()
    rn, rrows = S.component_table(lab)
    x = g(lab, dev, torch.int32)
    n, rows = ops.component_table(x, cap)
    assert n == rn, (n, rn)
    assert rows.shape == (min(rn, cap), 8) and np.array_equal(rows, rrows[:cap])
    if cid == "bernoulli 33x31x37":
        assert lab.size % 64 and n > 100
    if cid == "bernoulli 33x31x37 cap16":
        assert n > 16
    if cid.startswith("past"):
        assert lab.size > 4096 * 256 and rows[0, 1] > lab.size // 4 and n > 500 and (rows[1:, 1] == 1).all()
    n2, rows2 = ops.component_table(x, cap)
    assert n2 == n and rows2.tobytes() == rows.tobytes()


def test_component_table_zeroes_the_rows_past_n(dev):
    """The device table itself, through the C ABI: n, the rows, and zeros up to the capacity on a 0xFF pre-fill."""
    from vnet_tensorflow_amd import _lib, sample as S
    lab = blob_and_islands()
    rn, rrows = S.component_table(lab)
    cap = rn + 9
    L = _lib.lib()
    x = g(lab, dev, torch.int32)
    need = L.vnet_cc_table_ws_bytes(*lab.shape)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    out = torch.full((cap * 8 + 1,), -1, dtype=torch.int32, device=dev)
    _lib.check(L.vnet_cc_table(x.data_ptr(), out.data_ptr() + 32 * cap, out.data_ptr(), cap, *lab.shape, ws.data_ptr(), need, None), "vnet_cc_table")
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert host[-1] == rn and np.array_equal(host[:rn * 8].reshape(-1, 8), rrows) and not host[rn * 8:-1].any()


WINDOWS = [((0, 0, 0), VOLUME), ((0, 5, 7), (1, 12, 20)), ((39, 5, 7), (1, 12, 20)), ((3, 0, 7), (16, 1, 20)), ((3, 35, 7), (16, 1, 20)),
           ((3, 5, 0), (16, 12, 1)), ((3, 5, 43), (16, 12, 1)), ((24, 24, 24), PATCH), ((0, 0, 0), PATCH), ((11, 13, 17), (9, 7, 5))]


def test_window_count_is_numpy(dev):
    from vnet_tensorflow_amd import ops, sample as S
    rng = np.random.default_rng(8)
    lab = np.where(rng.random(VOLUME) < 0.3, rng.integers(1, 300, size=VOLUME), 0).astype(np.int32)
    x = g(lab, dev, torch.int32)
    for start, size in WINDOWS:
        for lo, hi in ((1, 255), (2, 2), (0, 1000)):
            assert ops.window_count(x, start, size, lo, hi) == S.window_count(lab, start, size, lo, hi), (start, size, lo, hi)
    empty = g(np.zeros(VOLUME, np.int32), dev, torch.int32)
    assert ops.window_count(empty, (0, 0, 0), VOLUME, 1, 255) == (0, 0)
    with pytest.raises(Exception):
        ops.window_count(x, (30, 0, 0), PATCH, 1, 255)


def _volume(C, seed=40):
    rng = np.random.default_rng(seed + C)
    img = rng.normal(100.0, 40.0, VOLUME + (C,)).astype(np.float32)
    img[0, 0, 0, 0] = -0.0
    lab = rng.integers(0, 5, size=VOLUME).astype(np.int32)
    return img, lab


def _misaligned(a, dev, dtype=torch.float32):
    """A dense device copy of `a` that starts 4 bytes off a 16-byte boundary."""
    buf = torch.empty(a.size + 4, dtype=dtype, device=dev)
    off = 1 if buf.data_ptr() % 16 == 0 else 0
    t = buf[off:off + a.size].view(a.shape)
    t.copy_(torch.as_tensor(np.ascontiguousarray(a)).to(dtype))
    assert t.data_ptr() % 16 != 0 and t.is_contiguous()
    return t


CORNERS = [(0, 0, 0), (VOLUME[0] - PATCH[0], VOLUME[1] - PATCH[1], VOLUME[2] - PATCH[2]), (VOLUME[0] - PATCH[0], 0, 9), (5, VOLUME[1] - PATCH[1], 0)]


def _run_sample(dev, img_t, lab_t, C, start, flip, sigma, out_i=None):
    from vnet_tensorflow_amd import ops
    oi = out_i if out_i is not None else torch.full(PATCH + (C,), float("nan"), dtype=torch.float32, device=dev)
    ol = torch.full(PATCH + (1,), -1, dtype=torch.int32, device=dev)
    ops.sample_patch(img_t, lab_t, start, PATCH, flip, sigma, SEED, oi, ol)
    return oi.cpu().numpy(), ol.cpu().numpy()[..., 0]


@pytest.mark.parametrize("C", [1, 3, 4])
def test_sample_patch_crop_and_flip_bit_for_bit(dev, C):
    from vnet_tensorflow_amd import sample as S
    img, lab = _volume(C)
    ti, tl = g(img, dev), g(lab, dev, torch.int32)
    for k, start in enumerate(CORNERS):
        for flip in range(8):
            gi, gl = _run_sample(dev, ti, tl, C, start, flip, 0.0)
            ri, rl = S.patch(img, lab, start, PATCH, flip)
            assert gi.tobytes() == ri.tobytes() and np.array_equal(gl, rl), (start, flip)


@pytest.mark.parametrize("C", [1, 3, 4])
def test_sample_patch_noise_is_the_restatement(dev, C):
    """|device - restatement| <= 1e-5 sigma + 2^-23 |y|: r <= sqrt(2 * 24 ln 2) = 5.77, the float angle is within 2^-22 of 2 pi u2, logf,
    sinf and cosf within 2 ulp -- together |dz| < 5e-6 --, plus the one rounding of x + sigma z."""
    from vnet_tensorflow_amd import sample as S
    img, lab = _volume(C)
    ti, tl = g(img, dev), g(lab, dev, torch.int32)
    sigma = 5.0
    for start, flip in ((CORNERS[1], 0), (CORNERS[2], 5), (CORNERS[0], 7)):
        gi, gl = _run_sample(dev, ti, tl, C, start, flip, sigma)
        ri, rl = S.patch(img, lab, start, PATCH, flip, sigma, SEED)
        err = np.abs(gi.astype(np.float64) - ri)
        print("C=%d flip=%d: max |device - restatement| = %.3e (bound at 0: %.3e)" % (C, flip, err.max(), 1e-5 * sigma))
        assert (err <= 1e-5 * sigma + 2.0 ** -23 * np.abs(ri)).all(), err.max()
        assert np.array_equal(gl, rl)
        crop = S.patch(img, lab, start, PATCH, flip)[0]
        z = (gi.astype(np.float64) - crop) / sigma
        assert abs(z.mean()) < 5.0 / np.sqrt(z.size) and abs(z.var() - 1.0) < 5.0 * np.sqrt(2.0 / z.size)


def test_sample_patch_quads_and_scalars_agree(dev):
    """C = 4 through the 16-byte path (aligned) and through the one-channel path (a view 4 bytes off, source and slot): the same bits,
    with and without noise."""
    from vnet_tensorflow_amd import sample as S
    img, lab = _volume(4)
    tl = g(lab, dev, torch.int32)
    aligned = g(img, dev)
    assert aligned.data_ptr() % 16 == 0
    off_src = _misaligned(img, dev)
    for sigma in (0.0, 5.0):
        for flip in (0, 3, 6):
            a, la = _run_sample(dev, aligned, tl, 4, CORNERS[2], flip, sigma)
            b, lb = _run_sample(dev, off_src, tl, 4, CORNERS[2], flip, sigma)
            slot = _misaligned(np.zeros(PATCH + (4,), np.float32), dev)
            c, lc = _run_sample(dev, aligned, tl, 4, CORNERS[2], flip, sigma, out_i=slot)
            assert a.tobytes() == b.tobytes() == c.tobytes() and np.array_equal(la, lb) and np.array_equal(la, lc), (sigma, flip)
            if sigma == 0.0:
                assert a.tobytes() == S.patch(img, lab, CORNERS[2], PATCH, flip)[0].tobytes()


# ---- the dataset --------------------------------------------------------------------------------------------------------------------
def _datasets(dev, cin, budget=None):
    from vnet_tensorflow_amd import data, transforms as T

    def make(**kw):
        tf = [T.ManualNormalization(0, 255), T.ConfidenceCrop2([16, 16, 16], rand_range=4, probability=0.5), T.RandomFlip([True, False, True])]
        return data.VolumeDataset("synthetic", ["c%d.npy" % i for i in range(cin)], "label.npy", [0, 1], (16, 16, 16), 2, train=True, seed=5,
                                  synthetic={"Cases": 6, "Shape": [40, 40, 40]}, transforms=tf, **kw)
    kw = {"device_tail": dev}
    if budget is not None:
        kw["device_cache_bytes"] = budget
    return make(), make(**kw)


@pytest.mark.parametrize("cin", [1, 4])
@pytest.mark.parametrize("one_case", [False, True])
def test_dataset_on_the_device_is_the_numpy_dataset(dev, cin, one_case):
    case_bytes = 40 ** 3 * 4 * (cin + 1)
    host, on_dev = _datasets(dev, cin, budget=case_bytes * 3 // 2 if one_case else None)
    assert on_dev.device_tail == dev and on_dev._tail_at == 1
    flips = 0
    for epoch in range(2):
        ref = list(host)
        got = list(on_dev)
        assert len(ref) == len(got) == 3
        for (ri, rl), (gi, gl) in zip(ref, got):
            assert gi.is_cuda and gl.is_cuda and gi.dtype == torch.float32 and gl.dtype == torch.int32
            assert tuple(gi.shape) == ri.shape and tuple(gl.shape) == rl.shape
            assert gi.cpu().numpy().tobytes() == ri.tobytes() and np.array_equal(gl.cpu().numpy(), rl)
    st = on_dev.device_stats
    if one_case:
        assert st["evictions"] >= 6 and len(on_dev._dev_cache) == 1 and st["host_samples"] == 0
    else:
        assert st["uploads"] == 6 and st["evictions"] == 0 and st["host_samples"] == 0


def test_dataset_takes_the_numpy_path_where_it_must(dev):
    """A budget below one case, and a table capacity below a case's component count: every sample comes from the NumPy transforms, into
    the same device batch."""
    from vnet_tensorflow_amd import data, transforms as T
    for kw in ({"device_cache_bytes": 1000}, {"max_components": 1}):
        def make(**k):
            tf = [T.ConfidenceCrop2([16, 16, 16], rand_range=4, probability=1.0)]
            return data.VolumeDataset("synthetic", ["image.npy"], "label.npy", [0, 1, 2], (16, 16, 16), 2, train=True, seed=9,
                                      synthetic={"Cases": 2, "Shape": [40, 40, 40]}, transforms=tf, **k)
        host, on_dev = make(), make(device_tail=dev, **kw)
        (ri, rl), = list(host)
        (gi, gl), = list(on_dev)
        if "max_components" in kw and on_dev.device_stats["host_samples"] == 0:
            pytest.fail("the synthetic cases were expected to hold two components (two spheres)")
        assert on_dev.device_stats["host_samples"] >= 1
        assert gi.cpu().numpy().tobytes() == ri.tobytes() and np.array_equal(gl.cpu().numpy(), rl)


# ---- the training loop ----------------------------------------------------------------------------------------------------------------
PIPELINE = """preprocess:
  train:
    3D:
      - name: "Padding"
        variables:
          output_size: [24, 24, 24]
      - name: "ConfidenceCrop2"
        variables:
          output_size: [16, 16, 16]
          rand_range: 3
          probability: 0.8
      - name: "RandomNoise"
  test:
    3D:
      - name: "Padding"
        variables:
          output_size: [24, 24, 24]
      - name: "ConfidenceCrop2"
        variables:
          output_size: [16, 16, 16]
          rand_range: 3
          probability: 0.8
"""


def test_train_samples_on_the_device_across_the_capture(dev, tmp_path):
    """image2label.train() with SampleOnDevice on the reference's tail (Padding, ConfidenceCrop2, RandomNoise): two loader threads make
    the batches in device memory while the main thread runs two eager steps, captures the step graph and replays it.  The capture
    succeeded, the losses are finite, and the samples were written by loader threads, never by the main one."""
    from vnet_tensorflow_amd import ops
    from vnet_tensorflow_amd.model import image2label
    from tests.test_hip_train_loop import _cfg
    y = tmp_path / "pipeline.yaml"
    y.write_text(PIPELINE)
    cfg = _cfg(tmp_path, Pipeline=str(y), SampleOnDevice=True, DeviceCacheGB=1, LoaderThreads=2, Epoches=3)
    np.random.seed(3)
    m = image2label(None, cfg, device=dev, verbose=False)
    losses, names, real = [], set(), ops.sample_patch
    step = m.train_step

    def spy(*a, **kw):
        names.add(threading.current_thread().name)
        return real(*a, **kw)

    def record(*a, **kw):
        out = step(*a, **kw)
        losses.append(out)
        return out
    ops.sample_patch = spy
    m.train_step = record
    try:
        m.train()
    finally:
        ops.sample_patch = real
    torch.cuda.synchronize()
    assert m.global_step == 6 and len(losses) == 6
    assert all(np.isfinite(float(v)) for v in losses) and np.isfinite(m.last_loss)
    assert m._graphs is not None and not getattr(m, "_graph_failed", False)
    assert names and threading.current_thread().name not in names

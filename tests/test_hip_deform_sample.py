"""-m gpu: a training sample cut from a device-resident case through the free-form deformation (csrc/deform_sample.hip,
include/vnet_hip_deform_sample.h).

Fused == composition.  The rule of the header is bit equality with vnet_sample_patch(vnet_bspline_deform_f32(image), deformed label) for the
same window, flip, sigma and seed: both sides run the same device functions in the same order, so tobytes() must be equal -- no bound.
Against fp64.  Image: |y - y64| <= 2^-23 max|x| + 6e-12 max|x| (the derived bound of tests/test_hip_deform.py: one rounding to float plus the
summation-order distance of the displacement); with noise, on top of it, 1e-5 sigma + 2^-23 |y| (the derived bound of
tests/test_hip_sample.py).  Label: equality -- every test asserts first that its coefficients leave no voxel undecidable.

Inputs: volumes (21, 18, 23) at spacing (1.0, 0.8, 1.25) and (24, 20, 28) at (1, 1, 1), coefficients default_rng(seed).random(6591) * 6.0
for seeds 0..11 (shifts of 5 to 6 voxels, about 40 % of the voxels sample outside the volume; tests/test_deform_sample_host.py checks
that on the CPU), labels in {0, 1}."""
import threading

import numpy as np
import pytest
import torch

from tests.util import g

pytestmark = pytest.mark.gpu
VOLUMES = [((21, 18, 23), (1.0, 0.8, 1.25)), ((24, 20, 28), (1.0, 1.0, 1.0))]
PATCH = (8, 6, 10)
SEED = 0x9E3779B97F4A7C15
_REF = {}


def _inputs(shape, C, seed):
    """(image, label, coef) of a case: computed once and shared, never modified."""
    key = (shape, C, seed)
    if key not in _REF:
        rng = np.random.default_rng(1000 + 10 * sum(shape) + C)
        out = (rng.normal(20.0, 30.0, size=tuple(shape) + (C,)).astype(np.float32), (rng.random(shape) < 0.5).astype(np.int32),
               np.random.default_rng(seed).random(3 * 13 ** 3) * 6.0)
        for a in out:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _decidable(shape, spacing, coef):
    from vnet_tensorflow_amd import deform as D
    key = ("undecidable", shape, spacing, coef.tobytes()[:64])
    if key not in _REF:
        _REF[key] = int(D.undecidable(shape, spacing, coef).sum())
    assert _REF[key] == 0, "the seeded coefficients leave %d undecidable voxels: pick another seed" % _REF[key]


def _windows(shape, patch=PATCH):
    far = tuple(n - p for n, p in zip(shape, patch))
    return [((0, 0, 0), patch), (far, patch), ((far[0], 0, 5), patch), ((3, far[1], 0), patch), ((0, 0, 0), tuple(shape))]


def _misaligned(a, dev, dtype=torch.float32):
    """A dense device copy of `a` that starts 4 bytes off a 16-byte boundary."""
    buf = torch.empty(a.size + 4, dtype=dtype, device=dev)
    off = 1 if buf.data_ptr() % 16 == 0 else 0
    t = buf[off:off + a.size].view(a.shape)
    t.copy_(torch.as_tensor(np.ascontiguousarray(a)).to(dtype))
    assert t.data_ptr() % 16 != 0 and t.is_contiguous()
    return t


def _slots(dev, patch, C):
    return (torch.full(tuple(patch) + (C,), float("nan"), dtype=torch.float32, device=dev),
            torch.full(tuple(patch) + (1,), -1, dtype=torch.int32, device=dev))


def _fused(dev, ti, yl, dc, spacing, start, patch, flip, sigma, out_i=None):
    from vnet_tensorflow_amd import ops
    oi, ol = _slots(dev, patch, int(ti.shape[3]))
    if out_i is not None:
        oi = out_i
    ops.deform_sample_patch(ti, yl, dc, spacing, start, patch, flip, sigma, SEED, oi, ol)
    return oi.cpu().numpy(), ol.cpu().numpy()[..., 0]


def _composition(dev, yi, yl, start, patch, flip, sigma):
    from vnet_tensorflow_amd import ops
    oi, ol = _slots(dev, patch, int(yi.shape[3]))
    ops.sample_patch(yi, yl, start, patch, flip, sigma, SEED, oi, ol)
    return oi.cpu().numpy(), ol.cpu().numpy()[..., 0]


def _reads_past_the_window(shape, spacing, coef, start, patch):
    """From the restatement: (voxels of the window that sample outside the volume, voxels inside it with a tap outside the window)."""
    from vnet_tensorflow_amd import deform as D
    c = D.source_index(shape, spacing, coef, (start, patch))
    outside, leaves = np.zeros(patch, bool), np.zeros(patch, bool)
    for a, n in enumerate(shape):
        outside |= ~((c[..., a] >= -0.5) & (c[..., a] < n - 0.5))
        leaves |= (np.floor(c[..., a]) < start[a]) | (np.floor(c[..., a]) + 1 > start[a] + patch[a] - 1)
    return int(outside.sum()), int((leaves & ~outside).sum())


@pytest.mark.parametrize("sigma", [0.0, 5.0])
@pytest.mark.parametrize("C", [1, 3, 4, 8])
@pytest.mark.parametrize("vol", [0, 1])
def test_fused_is_deform_then_sample_bit_for_bit(dev, vol, C, sigma):
    from vnet_tensorflow_amd import ops
    shape, spacing = VOLUMES[vol]
    seed = (vol * 8 + [1, 3, 4, 8].index(C) * 2 + int(sigma > 0)) % 12
    img, lab, coef = _inputs(shape, C, seed)
    _decidable(shape, spacing, coef)
    ti, tl, dc = g(img, dev), g(lab, dev, torch.int32), torch.from_numpy(coef).to(dev)
    assert ti.data_ptr() % 16 == 0
    yi, yl = ops.bspline_deform(ti, dc, spacing, "image"), ops.bspline_deform(tl, dc, spacing, "label")
    past = [0, 0]
    for start, patch in _windows(shape):
        if patch != tuple(shape):
            o, t = _reads_past_the_window(shape, spacing, coef, start, patch)
            past[0] += o
            past[1] += t
        for flip in range(8):
            fi, fl = _fused(dev, ti, yl, dc, spacing, start, patch, flip, sigma)
            ci, cl = _composition(dev, yi, yl, start, patch, flip, sigma)
            assert fi.tobytes() == ci.tobytes() and fl.tobytes() == cl.tobytes(), (start, patch, flip)
            assert np.isfinite(fi).all() and set(np.unique(fl)) <= {0, 1}
    # a kernel that read only the window could not have passed: voxels of the small windows sample outside the volume, others inside it
    # take taps outside their window
    assert past[0] > 0 and past[1] > 0, past
    assert float((yi == 0).float().mean()) > 0.2


@pytest.mark.parametrize("sigma", [0.0, 5.0])
def test_quads_and_scalars_agree(dev, sigma):
    """C = 4 through the 16-byte path (aligned) and through the one-channel path (source, then slot, 4 bytes off): the same bits."""
    from vnet_tensorflow_amd import ops
    shape, spacing = VOLUMES[0]
    img, lab, coef = _inputs(shape, 4, 5)
    _decidable(shape, spacing, coef)
    tl, dc = g(lab, dev, torch.int32), torch.from_numpy(coef).to(dev)
    aligned, off_src = g(img, dev), _misaligned(img, dev)
    assert aligned.data_ptr() % 16 == 0
    yl = ops.bspline_deform(tl, dc, spacing, "label")
    yi = ops.bspline_deform(aligned, dc, spacing, "image")
    start = _windows(shape)[2][0]
    for flip in (0, 3, 6):
        a, la = _fused(dev, aligned, yl, dc, spacing, start, PATCH, flip, sigma)
        b, lb = _fused(dev, off_src, yl, dc, spacing, start, PATCH, flip, sigma)
        c, lc = _fused(dev, aligned, yl, dc, spacing, start, PATCH, flip, sigma, out_i=_misaligned(np.zeros(PATCH + (4,), np.float32), dev))
        assert a.tobytes() == b.tobytes() == c.tobytes() and np.array_equal(la, lb) and np.array_equal(la, lc), (sigma, flip)
        assert a.tobytes() == _composition(dev, yi, yl, start, PATCH, flip, sigma)[0].tobytes()


# (volume, patch, start, C): rows longer than a chunk of 1024 voxels (one row per chunk, four trips of the 256 threads and a tail); three
# rows per chunk with 10 rows in all (the last chunk holds one); 4160 chunks of one row, past the grid cap of 4096 workgroups.  X and Y are
# small in the first two, where a shift of 5 voxels would push every voxel outside: the spacing (6, 6, 1) makes it about half a voxel there
EDGES = {
    "rows longer than a chunk": ((3, 2, 1100), (2, 2, 1030), (1, 0, 35), 1),
    "rows longer than a chunk c4": ((3, 2, 1100), (2, 2, 1030), (0, 0, 70), 4),
    "row-count tail": ((6, 4, 310), (5, 2, 300), (1, 1, 7), 3),
    "past the grid cap": ((66, 65, 1100), (65, 64, 1030), (1, 0, 35), 1),
}
EDGE_SPACING = (6.0, 6.0, 1.0)


def test_edge_shapes_are_what_they_say():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vnet_tensorflow_amd", "csrc", "deform_sample.hip")).read()
    rows, chunk, cap = (int(re.search(r"\b%s\s*=\s*(\d+)" % n, src).group(1)) for n in ("DS_ROWS", "DS_CHUNK", "DS_MAXBLK"))

    def per_chunk(P2):
        return max(1, min(rows, chunk // P2))
    _, p, _, _ = EDGES["rows longer than a chunk"]
    assert p[2] > chunk and per_chunk(p[2]) == 1
    _, p, _, _ = EDGES["row-count tail"]
    assert per_chunk(p[2]) == 3 and (p[0] * p[1]) % 3 == 1
    _, p, _, _ = EDGES["past the grid cap"]
    assert per_chunk(p[2]) == 1 and cap < p[0] * p[1] < 2 * cap
    assert per_chunk(PATCH[2]) == rows and (PATCH[0] * PATCH[1]) % rows == 0 and (21 * 18) % rows != 0


@pytest.mark.parametrize("cid", sorted(EDGES))
def test_shape_edges_equal_the_composition(dev, cid):
    from vnet_tensorflow_amd import ops
    shape, patch, start, C = EDGES[cid]
    img, lab, coef = _inputs(shape, C, 7)
    _decidable(shape, EDGE_SPACING, coef)
    ti, tl, dc = g(img, dev), g(lab, dev, torch.int32), torch.from_numpy(coef).to(dev)
    yi, yl = ops.bspline_deform(ti, dc, EDGE_SPACING, "image"), ops.bspline_deform(tl, dc, EDGE_SPACING, "label")
    for flip, sigma in ((0, 0.0), (7, 5.0)):
        fi, fl = _fused(dev, ti, yl, dc, EDGE_SPACING, start, patch, flip, sigma)
        ci, cl = _composition(dev, yi, yl, start, patch, flip, sigma)
        assert fi.tobytes() == ci.tobytes() and fl.tobytes() == cl.tobytes(), (cid, flip, sigma)
        if sigma == 0.0:
            zero = float((fi == 0).mean())
            print("%s: %.0f%% of the window samples outside the volume" % (cid, 100.0 * zero))
            # (a property of the inputs, not of the kernel: both branches of the inside test are taken.  The shifts are positive, so only
            # voxels within a shift of the high faces leave: about one x-plane in two of the 66 in the largest volume, under 1 %)
            assert 0.001 < zero < 0.98


@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("vol", [0, 1])
def test_against_fp64(dev, vol, C):
    from vnet_tensorflow_amd import deform as D, ops, sample as S
    shape, spacing = VOLUMES[vol]
    img, lab, coef = _inputs(shape, C, 8 + vol * 2 + (C == 4))
    _decidable(shape, spacing, coef)
    ti, tl, dc = g(img, dev), g(lab, dev, torch.int32), torch.from_numpy(coef).to(dev)
    yl = ops.bspline_deform(tl, dc, spacing, "label")
    bound = (2.0 ** -23 + 6e-12) * np.abs(img).max()
    for (start, patch), flip in zip(_windows(shape), (0, 5, 3, 6, 7)):
        y64 = np.flip(D.linear64(img, coef, spacing, (start, patch)), S.flip_axes(flip))
        lref = np.flip(D.label(lab, coef, spacing)[tuple(slice(s, s + n) for s, n in zip(start, patch))], S.flip_axes(flip))
        fi, fl = _fused(dev, ti, yl, dc, spacing, start, patch, flip, 0.0)
        err = np.abs(fi.astype(np.float64) - y64).max()
        diff = int((fl != lref).sum())
        print("vol %d c%d window %s+%s flip %d: image max error %.3e (bound %.3e), %d label voxels differ" % (vol, C, start, patch, flip, err, bound, diff))
        assert err <= bound and diff == 0
        sigma = 5.0
        ni, nl = _fused(dev, ti, yl, dc, spacing, start, patch, flip, sigma)
        n64 = y64.astype(np.float32).astype(np.float64) + sigma * S.normal(SEED, y64.size).reshape(y64.shape)
        nerr = np.abs(ni.astype(np.float64) - n64)
        print("    with noise: max error %.3e (bound at 0: %.3e)" % (nerr.max(), bound + 1e-5 * sigma))
        assert (nerr <= bound + 1e-5 * sigma + 2.0 ** -23 * np.abs(n64)).all() and np.array_equal(nl, lref)
        z = (ni.astype(np.float64) - fi) / sigma
        assert abs(z.mean()) < 5.0 / np.sqrt(z.size) and abs(z.var() - 1.0) < 5.0 * np.sqrt(2.0 / z.size)


# ---- the dataset --------------------------------------------------------------------------------------------------------------------
DS_SPACING = (1.0, 0.8, 1.25)


def _datasets(dev, crop, cin, classes=(0, 1), cases=6, **kw):
    from vnet_tensorflow_amd import data, transforms as T

    def make(**k):
        first = T.ConfidenceCrop2([16, 16, 16], rand_range=4, probability=0.5) if crop == "confidence" else T.RandomCrop([16, 16, 16], 0.2, 30)
        tf = [T.ManualNormalization(0, 255), T.BSplineDeformation(4), first, T.RandomFlip([True, False, True])]
        return data.VolumeDataset("synthetic", ["c%d.npy" % i for i in range(cin)], "label.npy", list(classes), (16, 16, 16), 2, train=True, seed=5,
                                  synthetic={"Cases": cases, "Shape": [40, 40, 40], "Spacing": list(DS_SPACING)}, transforms=tf, **k)
    return make(), make(device_tail=dev, **kw), make()


def _compare(host, on_dev, probe, epochs, batches):
    from vnet_tensorflow_amd import deform as D
    for epoch in range(epochs):
        for _, seeds in probe.epoch_plan():
            for sd in seeds:
                coef = np.random.default_rng(sd).random(D.PARAMS) * 4
                assert int(D.undecidable((40, 40, 40), DS_SPACING, coef).sum()) == 0
        ref, got = list(host), list(on_dev)
        assert len(ref) == len(got) == batches
        for (ri, rl), (gi, gl) in zip(ref, got):
            assert gi.is_cuda and gl.is_cuda and gi.dtype == torch.float32 and gl.dtype == torch.int32
            assert tuple(gi.shape) == ri.shape and tuple(gl.shape) == rl.shape
            # equal deformed labels give equal tables and counts, hence equal windows: the label patches are equal
            assert np.array_equal(gl.cpu().numpy(), rl)
            # each side is half a float ulp away from its fp64 blend; the normalised volumes lie in [0, 255]
            bound = 2.0 ** -23 * np.abs(ri).max() + 6e-12 * 255.0
            assert np.abs(gi.cpu().numpy().astype(np.float64) - ri.astype(np.float64)).max() <= bound


@pytest.mark.parametrize("crop,cin", [("confidence", 1), ("random", 4)])
@pytest.mark.parametrize("one_case", [False, True])
def test_dataset_through_the_deformation_is_the_numpy_dataset(dev, crop, cin, one_case):
    case_bytes = 40 ** 3 * 4 * (cin + 1)
    kw = {"device_cache_bytes": case_bytes * 3 // 2} if one_case else {}
    host, on_dev, probe = _datasets(dev, crop, cin, **kw)
    assert on_dev.device_tail == dev and on_dev._tail_at == 1 and on_dev._deformed
    _compare(host, on_dev, probe, epochs=2, batches=3)
    st = on_dev.device_stats
    if one_case:
        assert st["evictions"] >= 6 and len(on_dev._dev_cache) == 1 and st["host_samples"] == 0
    else:
        assert st["uploads"] == 6 and st["evictions"] == 0 and st["host_samples"] == 0


def test_dataset_takes_the_numpy_tail_past_max_components(dev):
    """Two spheres per case: a deformed label with two components is beyond max_components = 1 and takes the NumPy tail on a fresh
    generator, into the same device batch."""
    host, on_dev, probe = _datasets(dev, "confidence", 1, classes=(0, 1, 2), cases=4, max_components=1)
    _compare(host, on_dev, probe, epochs=1, batches=2)
    assert on_dev.device_stats["host_samples"] >= 1 and on_dev.device_stats["uploads"] == 4


# ---- the training loop ----------------------------------------------------------------------------------------------------------------
PIPELINE = """preprocess:
  train:
    3D:
      - name: "Padding"
        variables:
          output_size: [24, 24, 24]
      - name: "BSplineDeformation"
        variables:
          randomness: 4
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


def test_train_samples_through_the_deformation_across_the_capture(dev, tmp_path, capsys):
    """image2label.train() with SampleOnDevice on a pipeline that holds a BSplineDeformation: two loader threads deform the label, table
    its components and write the samples in device memory while the main thread runs two eager steps, captures the step graph and
    replays it.  The dataset served the tail on the device (every sample came from ops.deform_sample_patch, on a loader thread), the
    capture succeeded and the losses are finite."""
    from vnet_tensorflow_amd import ops
    from vnet_tensorflow_amd.model import image2label
    from tests.test_hip_train_loop import _cfg
    y = tmp_path / "pipeline.yaml"
    y.write_text(PIPELINE)
    cfg = _cfg(tmp_path, Pipeline=str(y), SampleOnDevice=True, DeviceCacheGB=1, LoaderThreads=2, Epoches=3)
    np.random.seed(3)
    m = image2label(None, cfg, device=dev, verbose=False)
    losses, names, real, plain = [], [], ops.deform_sample_patch, ops.sample_patch
    step = m.train_step

    def spy(*a, **kw):
        names.append(threading.current_thread().name)
        return real(*a, **kw)

    def undeformed(*a, **kw):
        raise AssertionError("the deformed tail must not go through sample_patch")

    def record(*a, **kw):
        out = step(*a, **kw)
        losses.append(out)
        return out
    ops.deform_sample_patch, ops.sample_patch = spy, undeformed
    m.train_step = record
    try:
        m.train()
    finally:
        ops.deform_sample_patch, ops.sample_patch = real, plain
    torch.cuda.synchronize()
    assert m.global_step == 6 and len(losses) == 6
    assert all(np.isfinite(float(v)) for v in losses) and np.isfinite(m.last_loss)
    assert m._graphs is not None and not getattr(m, "_graph_failed", False)
    assert "loader path" not in capsys.readouterr().out
    assert len(names) == 12 and threading.current_thread().name not in names

"""-m gpu: the free-form deformation kernels (csrc/deform.hip, include/vnet_hip_deform.h) against the fp64 restatement
(vnet_tensorflow_amd/deform.py), the transform's device path against its NumPy backend, and loader threads that deform on the device
while the main thread trains.

Bounds.  Image: |y - y64| <= 2^-23 max|x| + 6e-12 max|x| -- one rounding to float, plus a summation-order difference of the displacement of
at most 1e-12 voxels, times three axes, times a neighbour difference of at most 2 max|x|.  Label: equality.  A label depends on floor(c)
and on a truncation, so a voxel whose source index lies within 1e-9 of an integer or of n - 0.5 is not decidable across summation
orders: every case asserts that its seeded inputs have no such voxel (deform.undecidable), then demands equality everywhere."""
import os
import re
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SPACING = (1.0, 0.8, 1.25)

# (shape, C, view offset in floats): one channel and three (scalar path), four aligned (quads) and the same through a view that starts
# 4 bytes into its buffer (scalar path on C = 4); 128x96x96 is the issue's large case, 192x172x16 the one whose 4128 chunks of 8 rows
# pass the kernel's grid cap of 4096 workgroups
SMALL = [((13, 10, 7), 1, 0), ((13, 10, 7), 3, 0), ((12, 9, 8), 4, 0), ((12, 9, 8), 4, 1)]
LARGE = [((128, 96, 96), 1, 0), ((192, 172, 16), 1, 0)]
# (shape, C, view offset, z-rows per chunk): every shape above has Z <= 96, so its chunks are DF_ROWS = 8 whole z-rows.  These reach the other
# values of clamp(DF_CHUNK / Z, 1, DF_ROWS): 3 rows of 300 voxels (20 rows in all: the last chunk holds 2, and a chunk's voxel loop takes
# four trips of the 256 threads), one row per chunk (Z = 600), and a row longer than DF_CHUNK (Z = 1100: the quotient 0 is clamped to 1).
# X and Y stay at 3 to 5, where a randomness of 10 would push every voxel outside the volume: 1.5 leaves about half of them inside.
CHUNKS = [((5, 4, 300), 1, 0, 3), ((5, 4, 300), 4, 0, 3), ((3, 5, 600), 1, 0, 1), ((4, 3, 1100), 1, 0, 1)]
CASES = ([(s, C, off, r) for s, C, off in SMALL for r in (1.5, 10)] + [(s, C, off, 10) for s, C, off in LARGE] +
         [(s, C, off, 1.5) for s, C, off, _ in CHUNKS])
_REF = {}


def _chunk_rows(Z):
    """z-rows per chunk, as df_launch computes them from the constants of csrc/deform.hip."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vnet_tensorflow_amd", "csrc", "deform.hip")).read()
    rows, chunk = (int(re.search(r"\b%s\s*=\s*(\d+)" % n, src).group(1)) for n in ("DF_ROWS", "DF_CHUNK"))
    return max(1, min(rows, chunk // Z)), chunk


def test_chunk_shapes_reach_every_row_count():
    """The shapes of CHUNKS are what their comment says under the kernel's present constants (a change of DF_ROWS / DF_CHUNK shows up here,
    not as a case that silently tests the 8-row path again)."""
    got = set()
    for (X, Y, Z), _, _, want in CHUNKS:
        rows, chunk = _chunk_rows(Z)
        assert rows == want, ((X, Y, Z), rows, want)
        got.add((rows, (X * Y) % rows != 0, rows * Z > 256, Z > chunk))
    assert (3, True, True, False) in got and (1, False, True, False) in got and (1, False, True, True) in got
    assert all(_chunk_rows(s[2])[0] == 8 for s, _, _ in SMALL + LARGE)


def _inputs(shape, C, randomness):
    seed = sum(shape) + 10 * C + int(randomness * 2)
    rng = np.random.default_rng(seed)
    x = rng.normal(20.0, 30.0, size=tuple(shape) + (C,)).astype(np.float32)
    lab = rng.integers(0, 6, size=shape).astype(np.int32)
    coef = rng.random(3 * 13 ** 3) * randomness
    return x, lab, coef


def _reference(shape, C, randomness):
    """(x, lab, coef, y64, label, undecidable count): computed once per case and shared, never modified."""
    from vnet_tensorflow_amd import deform as D
    key = (shape, C, randomness)
    if key not in _REF:
        x, lab, coef = _inputs(shape, C, randomness)
        out = (x, lab, coef, D.linear64(x, coef, SPACING), D.label(lab, coef, SPACING), int(D.undecidable(shape, SPACING, coef).sum()))
        for a in out[:5]:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _device_view(a, off, dev):
    """`a` on the device, `off` elements into a larger buffer (off = 1: a float32 view that is 4-byte but not 16-byte aligned)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("shape,C,off,randomness", CASES)
def test_kernels_against_the_restatement(dev, shape, C, off, randomness):
    from vnet_tensorflow_amd import ops
    x, lab, coef, y64, lref, undecided = _reference(shape, C, randomness)
    assert undecided == 0, "the seeded inputs have %d undecidable voxels: pick another seed" % undecided
    dc = torch.from_numpy(coef).to(dev)
    xd = _device_view(x, off, dev)
    assert xd.data_ptr() % 16 == (4 * off) % 16
    y = ops.bspline_deform(xd, dc, SPACING, "image")
    assert y.dtype == torch.float32 and tuple(y.shape) == x.shape
    err = np.abs(y.cpu().numpy().astype(np.float64) - y64).max()
    bound = (2.0 ** -23 + 6e-12) * np.abs(x).max()
    print("image %s c%d r%s: max error %.3e, bound %.3e, outside %.0f%%" % (shape, C, randomness, err, bound, 100.0 * (y64 == 0).mean()))
    assert err <= bound
    yl = ops.bspline_deform(torch.from_numpy(lab).to(dev), dc, SPACING, "label")
    assert yl.dtype == torch.int32
    diff = int((yl.cpu().numpy() != lref).sum())
    print("label %s r%s: %d voxels differ, %d non-zero" % (shape, randomness, diff, int((lref != 0).sum())))
    assert diff == 0
    # a second run gives the same bits, and a 3-d image is the one-channel case
    assert torch.equal(ops.bspline_deform(xd, dc, SPACING, "image"), y)
    assert torch.equal(ops.bspline_deform(torch.from_numpy(lab).to(dev), dc, SPACING, "label"), yl)
    if C == 1:
        assert torch.equal(ops.bspline_deform(xd[..., 0].contiguous(), dc, SPACING), y[..., 0])
    if randomness == 10 and max(shape) <= 13:
        assert (y64 == 0).mean() > 0.5                             # most taps leave the small volume
    # host coefficients are uploaded by the op
    assert torch.equal(ops.bspline_deform(xd, coef, SPACING), y)


def test_zero_grid_is_the_identity(dev):
    from vnet_tensorflow_amd import ops
    x, lab, _, _, _, _ = _reference((13, 10, 7), 3, 1.5)
    zero = torch.zeros(3 * 13 ** 3, dtype=torch.float64, device=dev)
    xd, ld = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
    assert torch.equal(ops.bspline_deform(xd, zero, SPACING), xd)
    assert torch.equal(ops.bspline_deform(ld, zero, SPACING, "label"), ld)


@pytest.mark.parametrize("randomness", [1.5, 10])
def test_transform_device_path_equals_its_numpy_backend(dev, randomness):
    from vnet_tensorflow_amd import deform as D, transforms as T
    rng = np.random.default_rng(41)
    sample = {'image': rng.normal(20.0, 30.0, size=(13, 10, 7, 3)).astype(np.float32),
              'label': rng.integers(0, 6, size=(13, 10, 7)).astype(np.int16), 'spacing': SPACING}
    coef = np.random.default_rng(9).random(D.PARAMS) * randomness
    assert int(D.undecidable((13, 10, 7), SPACING, coef).sum()) == 0
    host = T.run_pipeline([T.BSplineDeformation(randomness)], sample, np.random.default_rng(9))
    on_dev = T.run_pipeline([T.BSplineDeformation(randomness, device=dev)], sample, np.random.default_rng(9))
    assert on_dev['spacing'] == host['spacing'] == SPACING
    assert on_dev['image'].dtype == np.float32 and on_dev['label'].dtype == np.int16
    # both are one rounding away from the same fp64 blend, up to the displacement's summation order
    y64 = D.linear64(sample['image'], coef, SPACING)
    bound = (2.0 ** -23 + 6e-12) * np.abs(sample['image']).max()
    assert np.abs(on_dev['image'].astype(np.float64) - y64).max() <= bound
    assert np.abs(host['image'].astype(np.float64) - y64).max() <= bound
    assert np.array_equal(on_dev['label'], host['label'])
    # the staging buffers are reused: an earlier result must not change under a later call
    keep = on_dev['image'].copy()
    T.run_pipeline([T.BSplineDeformation(randomness, device=dev)], sample, np.random.default_rng(10))
    assert np.array_equal(on_dev['image'], keep)


def test_loader_threads_deform_on_the_device_while_the_main_thread_trains(dev, tmp_path):
    """Two loader threads make 6 batches from a 24x20x18 synthetic set through BSplineDeformation(device=...) while the main thread runs 6
    training steps of the smallest network of the system tests (two eager steps, the capture of the step graph, three replays).  The
    batches equal those of the same dataset on the NumPy backend -- images within the image bound, labels equal -- and the step graph was
    captured, not abandoned."""
    from vnet_tensorflow_amd import data, deform as D, transforms as T
    from vnet_tensorflow_amd.model import image2label
    from tests.test_hip_train_loop import _cfg

    def dataset(device):
        tf = [T.BSplineDeformation(1.5, device=device), T.RandomCrop([16, 16, 16])]
        return data.VolumeDataset("synthetic", ["image.npy"], "label.npy", [0, 1], (16, 16, 16), 2, train=True, seed=5,
                                  synthetic={"Cases": 12, "Shape": [24, 20, 18], "Spacing": list(SPACING)}, transforms=tf)
    ref = list(dataset(None))
    assert len(ref) == 6
    probe = dataset(None)
    for cases, seeds in probe.epoch_plan():
        for sd in seeds:
            coef = np.random.default_rng(sd).random(D.PARAMS) * 1.5
            assert int(D.undecidable((24, 20, 18), SPACING, coef).sum()) == 0

    np.random.seed(3)
    m = image2label(None, _cfg(tmp_path), device=dev, verbose=False)
    m.read_config()
    m.build_model_graph()
    m._setup_training()
    assert m._graph_mode() == "whole"
    got, losses = [], []
    loader = data.Prefetcher(dataset(dev), depth=4, workers=2)
    names = set()
    real = T.BSplineDeformation._on_device

    def spy(self, *a):
        names.add(threading.current_thread().name)
        return real(self, *a)
    T.BSplineDeformation._on_device = spy
    try:
        for ti, tl in loader:
            got.append((ti.numpy().copy(), tl.numpy().copy()))
            losses.append(float(m.train_step(ti.to(dev, non_blocking=True), tl.to(dev, non_blocking=True), dropout=0.0)))
    finally:
        T.BSplineDeformation._on_device = real
    torch.cuda.synchronize()
    assert len(got) == 6 and all(np.isfinite(losses)), losses
    assert m._graphs is not None and not getattr(m, "_graph_failed", False)
    assert names and threading.current_thread().name not in names
    for (gi, gl), (ri, rl) in zip(got, ref):
        # the image bound: each side is half a float ulp away from its fp64 blend; the synthetic volumes are clipped to [0, 255]
        bound = 2.0 ** -23 * np.abs(ri).max() + 6e-12 * 255.0
        assert np.abs(gi.astype(np.float64) - ri.astype(np.float64)).max() <= bound
        assert np.array_equal(gl, rl)

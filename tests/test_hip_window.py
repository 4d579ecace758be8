"""-m gpu: mirrored crops and mirrored, weighted accumulation on the device (csrc/window.hip, csrc/vnet_window.h, libvnet_window.so)
against the rules of vnet_tensorflow_amd/window.py, then evaluate end to end.  Equality is exact everywhere.  It can be: the unit is
built without contraction, every operation of the rules is one float32 operation, the patches are softmax-like values in [2^-20, 1] or
exactly 0 and the weights are >= 2^-100, so no product is subnormal and the NumPy restatement rounds like the device; and the forward
kernels give the same bits from launch to launch (tests/test_hip_determinism.py), so the end-to-end loop written here, which runs the
model's own _infer on torch.flip-ped batches, reproduces the sums bit for bit.
Shapes: the smallest at which each path can go wrong -- every mask, K on every template (1 .. 5) and on the generic loop (7), float2 /
float4 and the one-word paths (bases off their alignment), windows partly and wholly outside the volume, rows of 5, 6, 33 and 65
voxels (several rows per wave, one row per wave, a second step along the row), and past one trip of the capped grid in both layouts
(csrc/vnet_window.h: 2048 blocks * 4 waves * (64 / L) rows)."""
import numpy as np
import pytest
import torch

from tests.test_hip_components import K, PIXDIM, VOLUME, small_model  # noqa: F401  (small_model: a fixture)
from tests.test_window_host import BATCH, PATCH, STRIDE, asymmetric_weights, softmax_like, windows
from tests.util import g
from vnet_tensorflow_amd import ops, window as W

pytestmark = pytest.mark.gpu
ROWS_PER_TRIP = lambda P2: 2048 * 4 * (64 >> min(6, max(0, int(P2 - 1).bit_length())))          # noqa: E731


def _np(t):
    return t.cpu().numpy()


def _off16(shape, dtype, dev, fill=None):
    """A dense tensor whose first byte is 4 bytes past a 16-byte boundary."""
    n = int(np.prod(shape))
    buf = torch.zeros(n + 8, dtype=dtype, device=dev)
    lead = ((4 - buf.data_ptr() % 16) % 16) // 4
    t = buf[lead:lead + n].view(shape)
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    if fill is not None:
        t.copy_(torch.from_numpy(np.ascontiguousarray(fill)).to(dtype))
    return t


# ---- crop_flip --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 4, None], ids=lambda c: "label" if c is None else "C%d" % c)
def test_crop_flip_is_the_rule(dev, C):
    rng = np.random.default_rng(3 if C is None else C)
    if C is None:
        src, dt = rng.integers(1, 9, size=(7, 6, 9)).astype(np.int32), torch.int32
    else:
        src, dt = (rng.random((7, 6, 9, C)) + 0.5).astype(np.float32), torch.float32
    t = g(src, dev, dt)
    for mask in range(8):
        for start, size in (((5, 3, 6), (4, 5, 6)), ((0, 0, 0), (7, 6, 9)), ((1, 2, 3), (3, 2, 5)), ((6, 5, 8), (1, 1, 1))):
            want = W.crop_flip_np(src, start, size, mask)
            got = W.crop_flip(t, start, size, mask)
            assert got.dtype == dt and np.array_equal(_np(got), want), (mask, start, size)
            # a poisoned slot off a 16-byte boundary: the one-word path, the same values, every word written
            slot = _off16(want.shape, dt, dev)
            slot.view(torch.int32).fill_(-1)
            assert W.crop_flip(t, start, size, mask, out=slot) is slot and np.array_equal(_np(slot), want), (mask, start, size)
        if mask == 0:
            assert _np(W.crop_flip(t, (5, 3, 6), (4, 5, 6), 0)).tobytes() == _np(ops.crop_window(t, (5, 3, 6), (4, 5, 6))).tobytes()
    assert not W.crop_flip_np(src, (5, 3, 6), (4, 5, 6), 7)[:2].any()               # (mirrored, the overhang comes first: really zeros)
    assert np.array_equal(_np(t), src)                                              # the input is not written


@pytest.mark.parametrize("vol, start, size, C", [((70, 66, 67, 4), (3, 2, 1), (64, 64, 65, 4), 4),        # 64x64x65x4 words
                                                 ((100, 90, 40, 1), (2, 1, 3), (96, 96, 33, 1), 1),       # 9216 rows, one per wave
                                                 ((262, 262, 6, 1), (1, 2, 0), (260, 260, 5, 1), 1)],     # 67600 rows, eight per wave
                         ids=["64x64x65x4", "96x96x33", "260x260x5"])
def test_crop_flip_past_one_grid_trip(dev, vol, start, size, C):
    if size[2] != 65:
        assert size[0] * size[1] > ROWS_PER_TRIP(size[2])
    src = np.arange(int(np.prod(vol)), dtype=np.int64).astype(np.float32).reshape(vol) + 1
    t = g(src, dev)
    for mask in (0, 5, 7):
        assert np.array_equal(_np(W.crop_flip(t, start, size[:3], mask)), W.crop_flip_np(src, start, size[:3], mask)), mask
    if C == 4:
        slot = _off16(size, torch.float32, dev)
        assert np.array_equal(_np(W.crop_flip(t, start, size[:3], 6, out=slot)), W.crop_flip_np(src, start, size[:3], 6))
    assert _np(W.crop_flip(t, start, size[:3], 0)).tobytes() == _np(ops.crop_window(t, start, size[:3])).tobytes()


# ---- accumulate -------------------------------------------------------------------------------------------------------------------------------
def _weights(kind, P, seed=0):
    return {"null": None, "gaussian": W.weight_vectors("gaussian", P, 0.25), "asymmetric": asymmetric_weights(P, seed)}[kind]


def _dev_weights(w, dev):
    return None if w is None else tuple(g(v, dev) for v in w)


@pytest.mark.parametrize("K_", [1, 2, 3, 4, 5, 7])
def test_accumulate_is_the_rule(dev, K_):
    P, D = (4, 5, 6), (7, 6, 9)
    for mask in range(8):
        for kind in ("null", "gaussian", "asymmetric"):
            w = _weights(kind, P, mask)
            wd = _dev_weights(w, dev)
            # inside, partly outside on every axis, outside on one axis only, wholly outside
            for origin in ((2, 1, 3), (5, 3, 6), (0, 0, 8), (7, 0, 0)):
                patch = softmax_like(P + (K_,), seed=10 * K_ + mask)
                vol, cnt = softmax_like(D + (K_,), seed=mask, zeros=0.5), softmax_like(D, seed=mask + 1, zeros=0.5)
                tv, tc = g(vol, dev), g(cnt, dev)
                W.accumulate(g(patch, dev), tv, tc, origin, mask, wd)
                W.accumulate_np(patch, vol, cnt, origin, mask, w)
                assert np.array_equal(_np(tv), vol) and np.array_equal(_np(tc), cnt), (mask, kind, origin)
    # cnt null; the bases off their alignment (K = 2, 4: the one-word path of the same template)
    for mask, kind in ((0, "null"), (6, "asymmetric"), (7, "gaussian")):
        w = _weights(kind, P, 5)
        patch, vol = softmax_like(P + (K_,), seed=7), softmax_like(D + (K_,), seed=8)
        tv = _off16(vol.shape, torch.float32, dev, vol)
        W.accumulate(_off16(patch.shape, torch.float32, dev, patch), tv, None, (5, 3, 6), mask, _dev_weights(w, dev))
        W.accumulate_np(patch, vol, None, (5, 3, 6), mask, w)
        assert np.array_equal(_np(tv), vol), (mask, kind)


@pytest.mark.parametrize("kind", ["null", "gaussian", "asymmetric"])
def test_overlapping_windows_in_order(dev, kind):
    """The windows of a small case, each with its own mask, on the same sums, in order -- twice: the same bits on the second run; with
    null weights and mask 0 the bytes of ops.accumulate_patch."""
    P, D, K_ = (6, 5, 33), (11, 9, 40), 2
    w = _weights(kind, P, 1)
    wd = _dev_weights(w, dev)
    origins = [(i, j, k) for i in (0, 3, 5, 7) for j in (0, 4, 6) for k in (0, 7, 12)]         # the last of each axis reaches past the volume
    patches = [softmax_like(P + (K_,), seed=n) for n in range(len(origins))]
    runs = []
    for _ in range(2):
        tv, tc = torch.zeros(D + (K_,), device=dev), torch.zeros(D, device=dev)
        for n, (at, p) in enumerate(zip(origins, patches)):
            W.accumulate(g(p, dev), tv, tc, at, n % 8, wd)
        runs.append((_np(tv), _np(tc)))
    vol, cnt = np.zeros(D + (K_,), np.float32), np.zeros(D, np.float32)
    for n, (at, p) in enumerate(zip(origins, patches)):
        W.accumulate_np(p, vol, cnt, at, n % 8, w)
    assert np.array_equal(runs[0][0], vol) and np.array_equal(runs[0][1], cnt) and cnt.min() > 0
    assert runs[1][0].tobytes() == runs[0][0].tobytes() and runs[1][1].tobytes() == runs[0][1].tobytes()
    if kind == "null":
        tv, tc = torch.zeros(D + (K_,), device=dev), torch.zeros(D, device=dev)
        ov, oc = torch.zeros(D + (K_,), device=dev), torch.zeros(D, device=dev)
        for at, p in zip(origins, patches):
            W.accumulate(g(p, dev), tv, tc, at, 0, None)
            ops.accumulate_patch(g(p, dev), ov, oc, at)
        assert _np(tv).tobytes() == _np(ov).tobytes() and _np(tc).tobytes() == _np(oc).tobytes() and _np(tc).max() > 2


@pytest.mark.parametrize("P, D, origin, K_", [((96, 96, 33), (100, 100, 40), (3, 2, 5), 2), ((260, 260, 5), (262, 258, 8), (1, 0, 4), 3),
                                              ((64, 64, 65), (70, 66, 67), (3, 2, 1), 4)], ids=["96x96x33", "260x260x5", "64x64x65"])
def test_accumulate_past_one_grid_trip(dev, P, D, origin, K_):
    if P[2] != 65:
        assert P[0] * P[1] > ROWS_PER_TRIP(P[2])
    patch = softmax_like(P + (K_,), seed=3)
    tp = g(patch, dev)
    for mask, kind in ((0, "null"), (7, "asymmetric")):
        w = _weights(kind, P, 2)
        vol, cnt = softmax_like(D + (K_,), seed=4), softmax_like(D, seed=5)
        tv, tc = g(vol, dev), g(cnt, dev)
        W.accumulate(tp, tv, tc, origin, mask, _dev_weights(w, dev))
        W.accumulate_np(patch, vol, cnt, origin, mask, w)
        assert np.array_equal(_np(tv), vol) and np.array_equal(_np(tc), cnt), (mask, kind)
    ov, oc, tv, tc = (torch.zeros(D + (K_,), device=dev), torch.zeros(D, device=dev), torch.zeros(D + (K_,), device=dev),
                      torch.zeros(D, device=dev))
    ops.accumulate_patch(tp, ov, oc, origin)
    W.accumulate(tp, tv, tc, origin, 0, None)
    assert _np(tv).tobytes() == _np(ov).tobytes() and _np(tc).tobytes() == _np(oc).tobytes()


def test_ops_refuse_mixed_devices(dev):
    from vnet_tensorflow_amd._lib import VnetHipError
    P, D = (4, 5, 6), (7, 6, 9)
    with pytest.raises(VnetHipError, match="patch is on cpu"):
        W.accumulate(torch.zeros(P + (2,)), torch.zeros(D + (2,), device=dev), None, (0, 0, 0), 0, None)
    with pytest.raises(VnetHipError, match="w1 is on cpu"):
        W.accumulate(torch.zeros(P + (2,), device=dev), torch.zeros(D + (2,), device=dev), None, (0, 0, 0), 0,
                     (torch.ones(4, device=dev), torch.ones(5), torch.ones(6, device=dev)))
    with pytest.raises(VnetHipError, match="crop_flip: out"):
        W.crop_flip(torch.zeros(D + (1,), device=dev), (0, 0, 0), P, 0, out=torch.zeros(P + (1,)))


# ---- evaluate, end to end ---------------------------------------------------------------------------------------------------------------------
def _sums(m, img, dev, masks, weights, accumulate):
    """The loop written here: the reference's windows in their batches, the last batch once more; per batch one pass per mask, identity
    first, through the model's own _infer on the torch.flip-ped batch; accumulate(window softmax, origin, mask)."""
    dims = tuple(max(s, p) for s, p in zip(img.shape[:3], PATCH))
    padded = np.zeros(dims + img.shape[3:], np.float32)
    padded[:img.shape[0], :img.shape[1], :img.shape[2]] = img
    for batch in windows(dims, PATCH, STRIDE, BATCH):
        x = torch.from_numpy(np.stack([padded[tuple(slice(s, s + p) for s, p in zip(at, PATCH))] for at in batch])).to(dev)
        for mask in masks:
            axes = [1 + a for a in range(3) if mask >> a & 1]
            sm = m._infer(torch.flip(x, dims=axes).contiguous() if axes else x)
            for at, p in zip(batch, sm):
                accumulate(p, at, mask)
    return dims


def _reference(m, img, dev, mirror, kind, sigma=0.125):
    masks, weights = W.flip_sets(mirror), W.weight_vectors(kind, PATCH, sigma)
    dims = tuple(max(s, p) for s, p in zip(img.shape[:3], PATCH))
    vol, cnt = np.zeros(dims + (K,), np.float32), np.zeros(dims, np.float32)
    _sums(m, img, dev, masks, weights, lambda p, at, mask: W.accumulate_np(_np(p), vol, cnt, at, mask, weights))
    return vol, cnt


def _set(m, mirror, kind, sigma=0.125):
    m.evaluate_mirror, m.evaluate_window_weights, m.evaluate_window_sigma = mirror, kind, sigma


@pytest.mark.parametrize("mirror, kind", [([0, 2], "gaussian"), ([[0, 1]], "uniform")], ids=["02-gaussian", "joint01-uniform"])
def test_evaluate_with_mirrors_and_weights(dev, small_model, mirror, kind):
    """evaluate_single_3D == the loop written here (accumulate_np on the host), label and probabilities, for an array and for a case
    that lives on the device; on_label sees the same label; once each the back_size branch and a label filter."""
    from vnet_tensorflow_amd import model, resample as R
    m, img = small_model
    plain, plain_sm = m.evaluate_single_3D(img)
    vol, cnt = _reference(m, img, dev, mirror, kind)
    sl = tuple(slice(0, s) for s in VOLUME)
    want, want_sm = np.argmax(vol, -1)[sl], (np.moveaxis(vol, -1, 0) / cnt)[(slice(None),) + sl]
    print("%s %s: %d of %d voxels differ from the plain label, max |dp| %.3g" % (mirror, kind, int((want != plain).sum()), plain.size,
                                                                                float(np.abs(want_sm - plain_sm).max())))
    assert (want_sm != plain_sm).any()
    size = R.output_size(VOLUME, (1.0, 1.0, 1.0), (1.25, 0.8, 1.5))
    back = dict(back_size=size, back_ratio=(1.25, 0.8, 1.5))
    tv, tc = torch.from_numpy(vol).to(dev), torch.from_numpy(cnt).to(dev)
    want_back = _np(ops.resample(ops.argmax_label(tv), size, (1.25, 0.8, 1.5), "nearest")).astype(np.int64)
    want_back_sm = np.moveaxis(_np(ops.resample(tv, size, (1.25, 0.8, 1.5), "linear", divisor=tc)), -1, 0)
    try:
        _set(m, mirror, kind)
        for case in (img, torch.from_numpy(img).to(dev)):
            seen = []
            got, sm = m.evaluate_single_3D(case, on_label=lambda t: seen.append((t.dtype, t.device.type, _np(t))))
            assert got.dtype == np.int64 and got.shape == VOLUME and np.array_equal(got, want)
            assert sm.dtype == np.float32 and np.array_equal(sm, want_sm)
            assert len(seen) == 1 and seen[0][0] == torch.int32 and seen[0][1] == "cuda" and np.array_equal(seen[0][2], want)
            got, sm = m.evaluate_single_3D(case, **back)
            assert np.array_equal(got, want_back) and np.array_equal(sm, want_back_sm)
            got, sm = m.evaluate_single_3D(case, largest_component=True, spacing=PIXDIM)
            assert np.array_equal(got, model.ExtractLargestConnectedComponents(want, PIXDIM)) and np.array_equal(sm, want_sm)
    finally:
        _set(m, [], "uniform")
    again, again_sm = m.evaluate_single_3D(img)
    assert again.tobytes() == plain.tobytes() and again_sm.tobytes() == plain_sm.tobytes()


def test_evaluate_with_the_feature_off_is_the_plain_loop(dev, small_model):
    """Mirror [] and "uniform": == a loop over ops.accumulate_patch, on both paths, and libvnet_window.so's ops are not called."""
    m, img = small_model
    dims = tuple(max(s, p) for s, p in zip(img.shape[:3], PATCH))
    vol, cnt = torch.zeros(dims + (K,), device=dev), torch.zeros(dims, device=dev)
    _sums(m, img, dev, [0], None, lambda p, at, mask: ops.accumulate_patch(p, vol, cnt, at))
    sl = tuple(slice(0, s) for s in VOLUME)
    want, want_sm = np.argmax(_np(vol), -1)[sl], (np.moveaxis(_np(vol), -1, 0) / _np(cnt))[(slice(None),) + sl]
    called = []
    real = W.lib
    W.lib = lambda: called.append(1) or real()
    try:
        for setting in (([], "uniform"), (None, None)):
            _set(m, *setting)
            for case in (img, torch.from_numpy(img).to(dev)):
                got, sm = m.evaluate_single_3D(case)
                assert np.array_equal(got, want) and np.array_equal(sm, want_sm)
    finally:
        W.lib = real
        _set(m, [], "uniform")
    assert not called

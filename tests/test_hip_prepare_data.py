"""-m gpu: the kernels of csrc/morph.hip through vnet_tensorflow_amd/morph.py, every comparison `==` against the
NumPy rules of vnet_tensorflow_amd/prepare_data.py, and the two device tools end to end on a case written to a temporary directory.
Shapes: the smallest at which a kernel can go wrong -- one voxel, less than a word, 63 / 64 / 65 voxels per row, (19,37,130) which
crosses the dilation's 8 x 32 tile in A and B and has three words with a ragged last one, (9,9,200) narrower than the ball of radius 8,
and PAST_CAPS = (16390,2,65): 4098 dilation tiles (cap 4096), 65560 words (bounding-box cap 65536 threads, selection cap 16384 waves),
2.1 M voxels (crop and unpack cap 1 M threads), so every kernel takes a second trip of its loop."""
import ctypes
import os

import numpy as np
import pytest
import torch

from vnet_tensorflow_amd import data, morph, prepare_data as P

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1), (3, 2, 5), (5, 7, 63), (5, 7, 64), (5, 7, 65), (19, 37, 130), (9, 9, 200)]
PAST_CAPS = (16390, 2, 65)
RADII = (1, 2, 5, 8)
BALL_COUNT = {1: 19, 2: 81, 5: 739, 8: 2553}
LABEL_DTYPES = [np.uint8, np.int8, np.int16, np.uint16, np.int32]


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(mask, dev):
    return _up(P.pack_bits(mask), dev)


def _random(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def _high_bits_zero(bits, C):
    return C % 64 == 0 or not (bits[:, :, -1].view(np.uint64) >> np.uint64(C % 64)).any()


# ---- select -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", LABEL_DTYPES, ids=lambda d: np.dtype(d).name)
def test_select_bits(dev, dtype):
    info = np.iinfo(dtype)
    rng = np.random.default_rng(5)
    pool = np.array(sorted({info.min, info.min + 1, -1 if info.min < 0 else 3, 0, 1, 2, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41,
                            info.max - 1, info.max}), dtype=np.int64)
    sixteen = [int(info.min), int(info.max)] + [int(v) for v in pool if v not in (info.min, info.max)][:14]
    assert len(set(sixteen)) == 16
    for shape in SHAPES + [PAST_CAPS]:
        label = pool[rng.integers(0, pool.size, size=shape)].astype(dtype)
        for c in (shape[2] - 1, 63, 64):
            if c < shape[2]:
                label[-1, -1, c] = info.max                           # a set voxel at the row's end and on both sides of a word boundary
        t = _up(label, dev)
        assert t.dtype == {np.uint8: torch.uint8, np.int8: torch.int8, np.int16: torch.int16, np.uint16: torch.uint16,
                           np.int32: torch.int32}[dtype]
        for values in ([int(info.max)], [int(info.min)], sixteen):
            got = morph.select_bits(t, values).cpu().numpy()
            want = P.select(label, values)
            assert got.dtype == np.int64 and np.array_equal(got, P.pack_bits(want)), (shape, values)
            assert _high_bits_zero(got, shape[2])
            assert np.array_equal(P.unpack_bits(got, shape[2]), want)


def test_select_bits_refuses(dev):
    t = torch.zeros((2, 3, 4), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        morph.select_bits(t, [1, 1])
    with pytest.raises(ValueError):
        morph.select_bits(t, list(range(17)))
    with pytest.raises(ValueError):
        morph.select_bits(t, [256])
    with pytest.raises(morph.VnetHipError):
        morph.select_bits(t.to(torch.float32), [1])
    L = morph.lib()
    bits = torch.zeros((2, 3, 1), dtype=torch.int64, device=dev)
    vals = (ctypes.c_longlong * 1)(1)
    st = morph._stream(dev)
    assert L.vnet_select_bits(None, 0, vals, 1, bits.data_ptr(), 2, 3, 4, st) == -1                       # VNET_E_BADARG
    assert L.vnet_select_bits(t.data_ptr(), 5, vals, 1, bits.data_ptr(), 2, 3, 4, st) == -1
    assert L.vnet_select_bits(t.data_ptr(), 0, vals, 1, bits.data_ptr(), 2048, 2048, 2048, st) == -2      # VNET_E_UNSUPPORTED, no launch
    assert L.vnet_dilate_bits(bits.data_ptr(), bits.data_ptr(), 2, 3, 4, 1, st) == -1                     # in place
    assert L.vnet_masked_crop(t.data_ptr(), None, t.data_ptr(), 2, 3, 4, 1, 1, 0, 0, 2, 3, 4, st) == -1   # window past the volume
    assert L.vnet_masked_crop(t.data_ptr(), None, t.data_ptr(), 2, 3, 4, 3, 0, 0, 0, 2, 3, 4, st) == -1   # 3-byte elements
    torch.cuda.synchronize(dev)


# ---- dilate -------------------------------------------------------------------------------------------------------------------------
def _dilated(mask, r, dev):
    C = mask.shape[2]
    got = morph.dilate_bits(_bits(mask, dev), C, r).cpu().numpy()
    assert _high_bits_zero(got, C)
    return got


@pytest.mark.parametrize("r", RADII)
def test_dilate_single_voxels(dev, r):
    n = 2 * r + 3
    mask = np.zeros((n, n, n), np.uint8)
    mask[r + 1, r + 1, r + 1] = 1
    got = P.unpack_bits(_dilated(mask, r, dev), n)
    assert int(got.sum()) == BALL_COUNT[r] and np.array_equal(got, np.pad(P.ball(r), 1).astype(np.uint8))
    for shape in ((n, n, n), (19, 37, 130), (9, 9, 200)):
        for at in ((0, 0, 0), tuple(s - 1 for s in shape)):                          # the ball clipped by a corner
            mask = np.zeros(shape, np.uint8)
            mask[at] = 1
            assert np.array_equal(_dilated(mask, r, dev), P.pack_bits(P.dilate(mask, r))), (shape, at)
    for c in (63, 64):                                                               # the carry into the next word and into the previous
        mask = np.zeros((5, 7, 130), np.uint8)
        mask[2, 3, c] = 1
        got = _dilated(mask, r, dev)
        assert np.array_equal(got, P.pack_bits(P.dilate(mask, r))) and got[2, 3, 0] != 0 and got[2, 3, 1] != 0


@pytest.mark.parametrize("r", RADII)
def test_dilate_random_zeros_ones(dev, r):
    for k, shape in enumerate(SHAPES):
        for density in (0.01, 0.5):
            mask = _random(shape, density, 100 * r + k)
            assert np.array_equal(_dilated(mask, r, dev), P.pack_bits(P.dilate(mask, r))), (shape, density)
        zeros, ones = np.zeros(shape, np.uint8), np.ones(shape, np.uint8)
        assert not _dilated(zeros, r, dev).any()
        assert np.array_equal(_dilated(ones, r, dev), P.pack_bits(ones))


@pytest.mark.parametrize("r", (1, 5))
def test_dilate_past_the_grid_cap(dev, r):
    mask = _random(PAST_CAPS, 0.002, 9)
    mask[-1, -1, -1] = mask[0, 0, 0] = 1
    assert np.array_equal(_dilated(mask, r, dev), P.pack_bits(P.dilate(mask, r)))


def test_dilate_refuses(dev):
    bits = torch.zeros((2, 3, 1), dtype=torch.int64, device=dev)
    for r in (0, 9):
        with pytest.raises(ValueError):
            morph.dilate_bits(bits, 4, r)
    with pytest.raises(ValueError):
        morph.dilate_bits(bits, 65, 1)                     # two words per row would be needed
    with pytest.raises(morph.VnetHipError):
        morph.dilate_bits(bits.to(torch.int32), 4, 1)


# ---- bounding box, unpack -----------------------------------------------------------------------------------------------------------
def test_bits_bbox(dev):
    for k, shape in enumerate(SHAPES + [PAST_CAPS]):
        A, B, C = shape
        assert morph.bits_bbox(_bits(np.zeros(shape, np.uint8), dev), C) == (0, None, None)
        masks = []
        for at in ((0, 0, 0), (A - 1, B - 1, C - 1), (A // 2, B // 2, C // 2)):      # (the last valid bit of the last word)
            m = np.zeros(shape, np.uint8)
            m[at] = 1
            masks.append(m)
        masks += [_random(shape, 0.02, k), _random(shape, 0.5, 50 + k), np.ones(shape, np.uint8)]
        for m in masks:
            if not m.any():
                continue
            count, lo, hi = morph.bits_bbox(_bits(m, dev), C)
            assert count == int(m.sum()) and (lo, hi) == P.bounding_box(m), shape


def test_unpack_bits(dev):
    for k, shape in enumerate(SHAPES + [PAST_CAPS]):
        m = _random(shape, 0.3, k)
        m[-1, -1, -1] = 1
        got = morph.unpack_bits(_bits(m, dev), shape[2])
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), m)


# ---- masked crop --------------------------------------------------------------------------------------------------------------------
def _windows(shape):
    A, B, C = shape
    out = [((0, 0, 0), (max(A // 2, 1), max(B // 2, 1), max(C // 2, 1))),                    # at the origin
           ((A - max(A // 2, 1), B - max(B // 2, 1), C - max(C // 3, 1)), (max(A // 2, 1), max(B // 2, 1), max(C // 3, 1))),   # far corner
           ((A - 1, B // 2, C - 1), (1, 1, 1)), ((0, 0, 0), (1, 1, 1)), ((0, 0, 0), shape)]
    for c0, n in ((1, 63), (63, 2), (65, 64), (3, 125)):                                      # start and size on c off every multiple of 64
        if c0 + n <= C:
            out.append(((A // 3, B // 4, c0), (A - A // 3, B - B // 4, n)))
    return out


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_masked_crop(dev, dtype):
    eb = np.dtype(dtype).itemsize
    as_uint = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[eb]
    rng = np.random.default_rng(eb)
    for k, shape in enumerate([(1, 1, 1), (5, 7, 65), (19, 37, 130)]):
        raw = rng.integers(0, 256, size=shape + (eb,), dtype=np.uint8)                        # random bytes: NaN patterns among them
        src = raw.view(dtype).reshape(shape)
        if dtype == np.float32:
            patterns = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0x80000000, 0x7F800000], dtype=np.uint32).view(np.float32)
            src.reshape(-1)[:min(src.size, 5)] = patterns[:min(src.size, 5)]                  # quiet / signalling NaN, -0.0, inf
        mask = _random(shape, 0.5, 70 + k)
        t, bits = _up(src, dev), _bits(mask, dev)
        masked = np.where(mask != 0, src.view(as_uint), as_uint(0))
        for start, size in _windows(shape):
            w = tuple(slice(s, s + n) for s, n in zip(start, size))
            got = morph.masked_crop(t, bits, start, size)
            assert got.dtype == t.dtype and tuple(got.shape) == tuple(size)
            assert np.array_equal(got.cpu().numpy().view(as_uint), masked[w]), (shape, start, size)
            plain = morph.masked_crop(t, None, start, size)
            assert np.array_equal(plain.cpu().numpy().view(as_uint), src.view(as_uint)[w]), (shape, start, size)


def test_masked_crop_past_the_grid_cap_and_refusals(dev):
    A, B, C = PAST_CAPS
    src = np.random.default_rng(1).integers(-3000, 3000, size=PAST_CAPS).astype(np.int16)
    mask = _random(PAST_CAPS, 0.5, 2)
    start, size = (1, 0, 1), (A - 1, B, C - 1)
    got = morph.masked_crop(_up(src, dev), _bits(mask, dev), start, size).cpu().numpy()
    assert np.array_equal(got, np.where(mask != 0, src, 0)[1:, :, 1:])
    t = torch.zeros((2, 3, 4), dtype=torch.int16, device=dev)
    for start, size in (((0, 0, 0), (3, 3, 4)), ((0, 0, 1), (2, 3, 4)), ((0, 0, 0), (2, 0, 4)), ((-1, 0, 0), (2, 3, 4))):
        with pytest.raises(ValueError):
            morph.masked_crop(t, None, start, size)
    with pytest.raises(ValueError):
        morph.masked_crop(t, torch.zeros((2, 2, 1), dtype=torch.int64, device=dev), (0, 0, 0), (1, 1, 1))


# ---- the tools, file to file --------------------------------------------------------------------------------------------------------
def test_fit_label_and_binarize_end_to_end(dev, tmp_path, monkeypatch):
    shape = (40, 48, 70)
    rng = np.random.default_rng(21)
    image = rng.integers(-1000, 1000, size=shape).astype(np.int16)
    label = np.zeros(shape, np.uint8)
    label[9:30, 11:20, 3:66] = 1
    label[14:22, 12:17, 58:70] = 2                                   # reaches the far face in z: the window is one voxel short there
    label[33, 40, 30] = 1                                            # a stray voxel: it stretches the box, the mask around it is a ball
    spacing = (0.75, 0.75, 2.5)
    src, fit, binz = (str(tmp_path / n) for n in ("src", "fit", "bin"))
    os.makedirs(os.path.join(src, "case_a"))
    data.write_nifti(os.path.join(src, "case_a", "image.nii"), image, spacing)
    data.write_nifti(os.path.join(src, "case_a", "label.nii"), label, spacing)
    uploads = []
    real = P._upload

    def counted(arr, device):
        uploads.append(tuple(arr.shape))
        return real(arr, device)
    monkeypatch.setattr(P, "_upload", counted)

    assert P.FitLabel(src, fit, device=dev).run() == [("case_a", "done")]
    assert len(uploads) == 2                                          # the label and the image, once each
    want_image, want_label = P.fit_label(image, label, [1, 2])
    got_image, hdr = data.read_nifti(os.path.join(fit, "case_a", "image_cropped.nii"))
    got_label, _ = data.read_nifti(os.path.join(fit, "case_a", "label_cropped.nii"))
    assert got_image.dtype == np.int16 and got_label.dtype == np.uint8 and np.allclose(hdr["pixdim"], spacing)
    assert np.array_equal(got_image, want_image) and np.array_equal(got_label, want_label)
    assert (want_image == 0).any() and want_image.shape != image.shape

    del uploads[:]
    assert P.Binarize(fit, binz, select_label=(2,), mask_label=(1, 2), mask_dilation=5, device=dev).run() == [("case_a", "done")]
    assert len(uploads) == 2
    want_out, want_masked = P.binarize(want_image, want_label, [2], mask_labels=[1, 2], dilation=5)
    got_out, _ = data.read_nifti(os.path.join(binz, "case_a", "label_masked.nii"))
    got_masked, _ = data.read_nifti(os.path.join(binz, "case_a", "image_masked.nii"))
    assert got_out.dtype == np.uint8 and got_masked.dtype == np.int16
    assert np.array_equal(got_out, want_out) and np.array_equal(got_masked, want_masked) and want_out.any()

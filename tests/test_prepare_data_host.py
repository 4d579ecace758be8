"""The data-preparation tools without a GPU: the NumPy rules of vnet_tensorflow_amd/prepare_data.py (the ball against its known
counts, the dilation against scipy, the crop window by hand, the composed rules against their steps written out), what
csrc/vnet_tools.h alone has to say beside its row of tests/test_abi_ledger.py (needs the built library), and the command line on a
temporary directory with the device ops replaced by the rules."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

from tests import guard
from tests.test_abi_ledger import _result_types
from vnet_tensorflow_amd import _lib, data, morph, prepare_data as P

ROOT = guard.ROOT


# ---- the rules ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,count", [(1, 19), (2, 81), (5, 739), (8, 2553)])
def test_ball_counts_and_symmetry(r, count):
    b = P.ball(r)
    assert b.shape == (2 * r + 1,) * 3 and b.dtype == bool and int(b.sum()) == count
    assert b[r, r, r] and b[0, r, r] and not b[0, 0, 0]
    for perm in itertools.permutations(range(3)):
        assert np.array_equal(b, b.transpose(perm))
    for axis in range(3):
        assert np.array_equal(b, np.flip(b, axis))


@pytest.mark.parametrize("r", [1, 2, 5])
def test_dilate_is_scipy_binary_dilation_with_the_ball(r):
    from scipy import ndimage
    mask = (np.random.default_rng(7).random((33, 65, 70)) < 0.01).astype(np.uint8)
    want = ndimage.binary_dilation(mask, structure=P.ball(r), border_value=0)
    got = P.dilate(mask, r)
    assert got.dtype == np.uint8 and np.array_equal(got, want.astype(np.uint8))


def test_dilate_and_select_refuse_what_the_kernels_refuse():
    mask = np.zeros((3, 3, 3), np.uint8)
    for r in (0, 9):
        with pytest.raises(ValueError):
            P.dilate(mask, r)
    with pytest.raises(ValueError):
        P.select(mask, [1, 1])
    with pytest.raises(ValueError):
        P.select(mask, range(17))
    assert P.select(np.array([[[0, 1, 2, 3]]]), [1, 3]).tolist() == [[[0, 1, 0, 1]]]


def test_fit_window_by_hand():
    # both axes of interest in dims
    start, size = P.fit_window((3, 6, 0), (5, 9, 0), (10, 10, 10), buffer=2, dims=(0, 1))
    assert (start[0], size[0]) == (1, 7)              # end = 3 + 3 + 2 = 8 < 10
    assert (start[1], size[1]) == (4, 5)              # end = 6 + 4 + 2 = 12 -> 9: one voxel short, as the reference
    assert (start[2], size[2]) == (0, 9)              # an axis not in dims: start 0, end n - 1
    assert P.fit_window((0, 0, 0), (9, 9, 9), (10, 10, 10), 2, (0, 1, 2)) == ((0, 0, 0), (9, 9, 9))


def test_bounding_box_rule():
    m = np.zeros((4, 5, 6), np.uint8)
    assert P.bounding_box(m) is None
    m[1, 2, 3] = m[3, 2, 5] = 1
    assert P.bounding_box(m) == ((1, 2, 3), (3, 2, 5))


def test_partition_rule():
    assert P.partition(130, 64) == [(0, 64), (64, 64), (128, 2)]
    assert P.partition(128, 64) == [(0, 64), (64, 64)]
    assert P.partition(5, 64) == [(0, 5)]


def test_pack_bits_layout():
    rng = np.random.default_rng(3)
    for shape in ((1, 1, 1), (2, 3, 63), (2, 3, 64), (2, 3, 130)):
        m = (rng.random(shape) < 0.5).astype(np.uint8)
        m[-1, -1, -1] = 1
        bits = P.pack_bits(m)
        assert bits.dtype == np.int64 and bits.shape == shape[:2] + ((shape[2] + 63) // 64,)
        a, b, c = shape[0] - 1, shape[1] - 1, shape[2] - 1
        assert (int(bits[a, b, c // 64]) >> (c % 64)) & 1 == 1
        if shape[2] % 64:
            assert not (bits[:, :, -1].view(np.uint64) >> np.uint64(shape[2] % 64)).any()          # the unused high bits
        assert np.array_equal(P.unpack_bits(bits, shape[2]), m)


def _case(shape=(20, 24, 30), seed=11):
    """A small synthetic case [X,Y,Z]: int16 image, uint8 label with a block of 1 and, inside it, a block of 2."""
    rng = np.random.default_rng(seed)
    image = rng.integers(-1000, 1000, size=shape).astype(np.int16)
    image[image == 0] = 7
    label = np.zeros(shape, np.uint8)
    label[6:12, 9:15, 14:27] = 1
    label[8:10, 10:13, 18:22] = 2
    return image, label


def test_fit_label_against_its_steps_written_out():
    image, label = _case()
    got_image, got_label = P.fit_label(image, label, [1, 2], buffer=2, mask_image=True, dilation=2, dims=(0, 1, 2))
    # the steps: selection, its box, the window by the reference's arithmetic, the dilated mask
    sel = ((label == 1) | (label == 2)).astype(np.uint8)
    assert P.bounding_box(sel) == ((6, 9, 14), (11, 14, 26))
    # x: start 4, end 6 + 6 + 2 = 14; y: start 7, end 9 + 6 + 2 = 17; z: start 12, end 14 + 13 + 2 = 29 -> stays 29 (< 30)
    window = (slice(4, 14), slice(7, 17), slice(12, 29))
    mask = P.dilate(sel, 2)
    masked = image.copy()
    masked[mask == 0] = 0
    assert got_image.dtype == np.int16 and got_label.dtype == np.uint8
    assert np.array_equal(got_image, masked[window]) and np.array_equal(got_label, label[window])
    assert (got_image == 0).any() and (got_image != 0).any()
    # crop only: the image keeps its voxels; an axis outside dims keeps start 0 and loses its last voxel
    plain, _ = P.fit_label(image, label, [2], buffer=1, mask_image=False, dims=(0, 2))
    assert np.array_equal(plain, image[7:11, 0:23, 17:23])
    with pytest.raises(ValueError):
        P.fit_label(image, label, [5])


def test_binarize_against_its_steps_written_out():
    image, label = _case()
    label_out, none = P.binarize(image, label, [2])
    assert none is None and label_out.dtype == np.uint8 and np.array_equal(label_out, (label == 2).astype(np.uint8))
    label_out, masked = P.binarize(image, label, [2], mask_labels=[1, 2], dilation=5)
    keep = P.dilate(((label == 1) | (label == 2)).astype(np.uint8), 5) != 0
    assert masked.dtype == np.int16 and np.array_equal(masked, np.where(keep, image, 0)) and np.array_equal(label_out, label == 2)
    _, undilated = P.binarize(image, label, [2], mask_labels=[1], dilation=0)
    assert np.array_equal(undilated, np.where(label == 1, image, 0))


# ---- csrc/vnet_tools.h beside its ledger row (tests/test_abi_ledger.py) -------------------------------------------------------------
def test_tools_header_ledger():
    path = os.path.join(ROOT, morph.HEADER)
    fns = guard.header_functions(path)
    assert set(_result_types(path).values()) == {"int"}
    assert all(params[-1][0] == "stream" for params in fns.values())
    assert not [n for n in fns if n.endswith("_ws_bytes")]
    assert set(guard.pointer_entry_points(path)) == set(fns) and len(fns) == 5
    # the one HOST pointer of the header: the values of vnet_select_bits, copied into the kernel's arguments
    host = {(n, p[0]) for n, ps in fns.items() for p in ps if guard._is_buffer(p) and p[3].replace(" ", "") == "constlonglong*"
            and p[0] == "values"}
    assert host == {("vnet_select_bits", "values")} and host <= guard.HOST_POINTERS


def test_tools_live_in_the_one_library():
    assert morph.HEADER in [h for h, _ in _lib.HEADERS]
    names = set(guard.header_functions(os.path.join(ROOT, morph.HEADER)))
    assert len(names) == 5 and names <= set(_lib.all_signatures())
    main = ctypes.CDLL(_lib.LIB_PATH)
    assert not [n for n in names if not hasattr(main, n)]
    assert not morph.HEADER.startswith("include/") and not os.path.exists(os.path.join(ROOT, "include", "vnet_tools.h"))
    assert not hasattr(morph, "LIB_PATH")
    mk = open(os.path.join(ROOT, "vnet_tensorflow_amd", "csrc", "Makefile")).read()
    assert "libvnet_tools" not in mk and "TOOLS_" not in mk


def test_device_ops_refuse_cpu_tensors_and_bad_arguments():
    x = torch.zeros((2, 3, 4), dtype=torch.uint8)
    with pytest.raises(morph.VnetHipError, match="no CPU path"):
        morph.select_bits(x, [1])
    with pytest.raises(morph.VnetHipError):
        morph.unpack_bits(torch.zeros((2, 3, 1), dtype=torch.int64), 4)
    with pytest.raises(morph.VnetHipError):
        morph.select_bits(torch.zeros((2, 3), dtype=torch.uint8), [1])


# ---- the command line, the device ops replaced by the rules ------------------------------------------------------------------------
class _RuleOps(object):
    """morph's five ops on CPU tensors, by the NumPy rules."""

    def __init__(self):
        self.calls = []

    def select_bits(self, label, values, dtype_code=None):
        self.calls.append("select_bits")
        return torch.from_numpy(P.pack_bits(P.select(label.numpy(), values)))

    def dilate_bits(self, bits, C, r):
        self.calls.append("dilate_bits")
        return torch.from_numpy(P.pack_bits(P.dilate(P.unpack_bits(bits.numpy(), C), r)))

    def bits_bbox(self, bits, C):
        self.calls.append("bits_bbox")
        m = P.unpack_bits(bits.numpy(), C)
        box = P.bounding_box(m)
        return (0, None, None) if box is None else (int(m.sum()), box[0], box[1])

    def masked_crop(self, src, bits, start, size):
        self.calls.append("masked_crop")
        x = src.numpy()
        if bits is not None:
            x = np.where(P.unpack_bits(bits.numpy(), x.shape[2]) != 0, x, np.zeros((), x.dtype))
        return torch.from_numpy(np.ascontiguousarray(x[tuple(slice(s, s + n) for s, n in zip(start, size))]))

    def unpack_bits(self, bits, C):
        self.calls.append("unpack_bits")
        return torch.from_numpy(P.unpack_bits(bits.numpy(), C))


@pytest.fixture
def rule_ops(monkeypatch):
    ops = _RuleOps()
    for name in ("select_bits", "dilate_bits", "bits_bbox", "masked_crop", "unpack_bits"):
        monkeypatch.setattr(morph, name, getattr(ops, name))
    monkeypatch.setattr(P._Tool, "_device", lambda self: torch.device("cpu"))
    return ops


def _write_cases(src):
    image, label = _case()
    spacing = (0.7, 0.8, 2.5)
    for case, lab in (("case_a", label), ("case_empty", np.zeros_like(label))):
        os.makedirs(os.path.join(src, case))
        data.write_nifti(os.path.join(src, case, "image.nii"), image, spacing)
        data.write_nifti(os.path.join(src, case, "label.nii"), lab, spacing)
    open(os.path.join(src, "notes.txt"), "w").close()                        # not a case
    os.makedirs(os.path.join(src, "no_files"))                               # a directory without the files
    return image, label, spacing


def test_command_line_fit_label_binarize_partition(tmp_path, rule_ops, capsys):
    src, fit, binz, part = (str(tmp_path / n) for n in ("src", "fit", "bin", "part"))
    os.makedirs(src)
    image, label, spacing = _write_cases(src)

    assert P.main(["fit-label", src, fit, "-v"]) == 0
    out = capsys.readouterr().out
    assert "case_empty: skipped" in out and "case_a:" in out and "2 cases, 1 skipped" in out
    assert sorted(os.listdir(fit)) == ["case_a"]                              # the empty case writes nothing
    assert sorted(os.listdir(os.path.join(fit, "case_a"))) == ["image_cropped.nii", "label_cropped.nii"]      # .gz dropped
    want_image, want_label = P.fit_label(image, label, [1, 2])
    got_image, hdr = data.read_nifti(os.path.join(fit, "case_a", "image_cropped.nii"))
    got_label, _ = data.read_nifti(os.path.join(fit, "case_a", "label_cropped.nii"))
    assert got_image.dtype == np.int16 and got_label.dtype == np.uint8                                          # dtypes kept
    assert np.array_equal(got_image, want_image) and np.array_equal(got_label, want_label)
    assert np.allclose(hdr["pixdim"], spacing)
    assert rule_ops.calls == ["select_bits", "bits_bbox", "dilate_bits", "masked_crop", "masked_crop", "select_bits", "bits_bbox"]

    # binarize reads what fit-label wrote under the .nii.gz names
    assert P.main(["binarize", fit, binz, "--select", "2", "--mask-label", "1", "2", "--mask-dilation", "5"]) == 0
    assert sorted(os.listdir(os.path.join(binz, "case_a"))) == ["image_masked.nii", "label_masked.nii"]
    want_out, want_masked = P.binarize(want_image, want_label, [2], mask_labels=[1, 2], dilation=5)
    got_out, _ = data.read_nifti(os.path.join(binz, "case_a", "label_masked.nii"))
    got_masked, _ = data.read_nifti(os.path.join(binz, "case_a", "image_masked.nii"))
    assert got_out.dtype == np.uint8 and got_masked.dtype == np.int16
    assert np.array_equal(got_out, want_out) and np.array_equal(got_masked, want_masked)

    # without --mask-label only the label is written
    assert P.main(["binarize", fit, str(tmp_path / "bin2")]) == 0
    assert sorted(os.listdir(str(tmp_path / "bin2" / "case_a"))) == ["label_masked.nii"]

    assert P.main(["partition", fit, part, "--layer", "6"]) == 0
    nz = want_label.shape[2]
    assert sorted(os.listdir(part)) == sorted("case_a_%d" % k for k, _ in P.partition(nz, 6))
    for k, n in P.partition(nz, 6):
        slab, hdr = data.read_nifti(os.path.join(part, "case_a_%d" % k, "image.nii"))
        assert np.array_equal(slab, want_image[:, :, k:k + n]) and slab.dtype == np.int16 and np.allclose(hdr["pixdim"], spacing)
        slab, _ = data.read_nifti(os.path.join(part, "case_a_%d" % k, "label.nii"))
        assert np.array_equal(slab, want_label[:, :, k:k + n])


def test_callable_form_and_flags(tmp_path, rule_ops):
    src = str(tmp_path / "src")
    os.makedirs(src)
    image, label, _ = _write_cases(src)
    tool = P.FitLabel(src, str(tmp_path / "t"), select_label=(2,), buffer=1, mask_image=False, mask_dim=(0, 2), device="cpu")
    assert tool.run() == [("case_a", "done"), ("case_empty", "skipped: empty selection")]
    got, _ = data.read_nifti(str(tmp_path / "t" / "case_a" / "image_cropped.nii"))
    assert np.array_equal(got, P.fit_label(image, label, [2], buffer=1, mask_image=False, dims=(0, 2))[0])
    assert "dilate_bits" not in rule_ops.calls
    args = P.get_parser().parse_args(["fit-label", "a", "b"])
    t = P.from_args(args)
    assert (t.select_label, t.buffer, t.mask_image, t.mask_dilation, t.mask_dim) == ([1, 2], 2, True, 2, (0, 1, 2))
    assert (t.src_img_name, t.src_label_name, t.tgt_img_name, t.tgt_label_name) == (
        "image.nii", "label.nii", "image_cropped.nii.gz", "label_cropped.nii.gz")
    b = P.from_args(P.get_parser().parse_args(["binarize", "a", "b", "--gpu", "1"]))
    assert (b.select_label, b.mask_label, b.mask_dilation, b.device) == ([2], [], 5, "cuda:1")
    assert P.from_args(P.get_parser().parse_args(["partition", "a", "b"])).layer == 64
    with pytest.raises(ValueError):
        P.FitLabel("a", "b", mask_dilation=9)

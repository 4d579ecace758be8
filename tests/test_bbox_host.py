"""The bounding-box tool without a device: the rules of vnet_tensorflow_amd/bounding_box.py (stack, plane_components, suppress,
slice_boxes, geometry, render) against the reference's recorded answers, an independent brute force and hand-written pictures; the
ledger of csrc/vnet_bbox.h; the order of the error codes; the command line."""
import ctypes
import json
import os
import struct
import zlib

import numpy as np
import pytest

from tests import guard
from vnet_tensorflow_amd import bounding_box as B

ROOT = guard.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "bbox_nms.npz")


# ---- suppress ----------------------------------------------------------------------------------------------------------------------
def test_suppress_equals_every_recorded_answer_of_the_reference():
    d = np.load(GOLDEN)
    count = int(d["count"])
    assert count >= 200
    sizes = set()
    for k in range(count):
        boxes, picks = d["boxes_%d" % k], d["picks_%d" % k]
        bottom = boxes[:, 1] + boxes[:, 3]
        assert len(set(bottom.tolist())) == len(bottom), "case %d has a tie: the reference's answer there depends on the NumPy build" % k
        got = B.suppress(boxes, float(d["thresh"]))
        assert got.dtype == np.int64 and np.array_equal(got, picks), k
        sizes.add(len(boxes))
    assert min(sizes) == 1 and max(sizes) >= 20           # (large draws rarely come without a tie)


def test_suppress_ties_follow_the_stable_order():
    """Hand-counted.  Equal y + h: the stable sort keeps input order, the pick comes from the END, so the LATER box is picked first."""
    # two disjoint boxes with the same bottom edge: both survive, the later one first
    assert B.suppress([[0, 0, 2, 5], [10, 0, 2, 5]]).tolist() == [[10, 0, 2, 5], [0, 0, 2, 5]]
    # two identical boxes: the later is picked, the earlier lies fully inside it and is dropped
    assert B.suppress([[1, 1, 4, 4], [1, 1, 4, 4]]).tolist() == [[1, 1, 4, 4]]
    # same bottom (6); box 1 (later) is picked; its intersection with box 0 is 3 x 7 = 21 of box 0's 5 x 7 = 35: 0.6 > 0.5, dropped
    assert B.suppress([[0, 0, 4, 6], [2, 0, 4, 6]]).tolist() == [[2, 0, 4, 6]]
    # the other order: box 1 = (0, 0, 4, 6) is picked and (2, 0, 4, 6) is dropped by the same count
    assert B.suppress([[2, 0, 4, 6], [0, 0, 4, 6]]).tolist() == [[0, 0, 4, 6]]
    # intersection 2 x 7 = 14 of 35 = 0.4: both stay, later first; a third box with a larger bottom goes in front of both
    assert B.suppress([[0, 0, 4, 6], [3, 0, 4, 6], [20, 20, 1, 1]]).tolist() == [[20, 20, 1, 1], [3, 0, 4, 6], [0, 0, 4, 6]]
    assert B.suppress(np.zeros((0, 4))).shape == (0, 4)


# ---- components and boxes against a brute force ------------------------------------------------------------------------------------
def _brute(stk):
    """scipy.ndimage.label (default structure: faces) per slice and value, find_objects for the boxes."""
    from scipy import ndimage
    S, V, U = stk.shape
    rows, boxes = [], {s: [] for s in range(S)}
    for s in range(S):
        for value in sorted(int(v) for v in np.unique(stk[s]) if v > 0):
            lab, k = ndimage.label(stk[s] == value)
            found = []
            for i, sl in enumerate(ndimage.find_objects(lab)):
                where = np.nonzero(lab.reshape(-1) == i + 1)[0]
                rows.append((s * V * U + int(where[0]), len(where), s, sl[0].start, sl[1].start, s, sl[0].stop - 1, sl[1].stop - 1))
                found.append((int(where[0]), [sl[1].start, sl[0].start, sl[1].stop - sl[1].start, sl[0].stop - sl[0].start]))
            found.sort()                                                   # raster order of the first voxel
            boxes[s].extend(tuple(int(v) for v in b) + (value,) for b in B.suppress([f[1] for f in found]))
    rows.sort()
    return np.asarray(rows, dtype=np.int32).reshape(-1, 8), boxes


@pytest.mark.parametrize("shape,seed", [((3, 17, 23), 0), ((2, 40, 33), 1), ((4, 1, 9), 2), ((4, 9, 1), 3), ((1, 1, 1), 4)])
def test_plane_components_and_slice_boxes_against_brute_force(shape, seed):
    rng = np.random.default_rng(seed)
    stk = rng.integers(0, 4, shape).astype(np.int32)
    n, rows = B.plane_components(stk)
    want_rows, want_boxes = _brute(stk)
    assert n == len(want_rows) and rows.dtype == np.int32 and np.array_equal(rows, want_rows)
    assert np.array_equal(rows[:, 2], rows[:, 5])
    got = B.slice_boxes(stk)
    assert sorted(got) == list(range(shape[0])) and got == want_boxes


def test_plane_components_rules():
    ones = np.ones((5, 6, 7), dtype=np.int32)
    n, rows = B.plane_components(ones)
    assert n == 5 and rows[:, 1].tolist() == [42] * 5 and rows[:, 0].tolist() == [42 * s for s in range(5)]       # slices do not merge
    v, u = np.mgrid[0:8, 0:8]
    board = np.broadcast_to(1 + (u + v) % 2, (2, 8, 8)).astype(np.int32)
    n, rows = B.plane_components(board)
    assert n == 128 and set(rows[:, 1].tolist()) == {1}                                                       # classes do not merge
    diag = np.zeros((1, 3, 3), dtype=np.int32)
    diag[0, 0, 0] = diag[0, 1, 1] = 2
    assert B.plane_components(diag)[0] == 2
    neg = np.full((1, 2, 2), -3, dtype=np.int32)
    assert B.plane_components(neg)[0] == 0 and B.slice_boxes(neg) == {0: []}


def test_slice_boxes_orders_labels_then_picks():
    stk = np.zeros((2, 6, 8), dtype=np.int32)
    stk[1, 0:2, 0:2] = 2          # class 2: one box, bottom 2
    stk[1, 0, 5] = 1              # class 1: bottom 1
    stk[1, 3:5, 3:6] = 1          # class 1: bottom 5: picked first
    assert B.slice_boxes(stk) == {0: [], 1: [(3, 3, 3, 2, 1), (5, 0, 1, 1, 1), (0, 0, 2, 2, 2)]}


# ---- stack, geometry -----------------------------------------------------------------------------------------------------------------
def test_stack_layouts():
    x = np.arange(5 * 7 * 9, dtype=np.float32).reshape(5, 7, 9)
    for axis, perm in ((2, (2, 1, 0)), (1, (1, 2, 0)), (0, (0, 2, 1))):
        got = B.stack(x, axis)
        assert got.flags["C_CONTIGUOUS"] and np.array_equal(got, np.transpose(x, perm))
    assert B.stack(x, 2)[3, 4, 1] == x[1, 4, 3] and B.stack(x, 1)[3, 4, 1] == x[1, 3, 4] and B.stack(x, 0)[3, 4, 1] == x[3, 1, 4]
    with pytest.raises(ValueError):
        B.stack(x, 3)


def test_geometry_hand_computed():
    # axial: in-plane (x, y) -> 0.5; y: ceil(1.0 * 12 / 0.5) = 24 (a product that lands on an integer), x: ceil(0.5 * 20 / 0.5) = 20
    assert B.geometry((20, 12, 6), (0.5, 1.0, 2.0), 2) == ((20, 24, 6), (0.5, 0.5, 2.0))
    # coronal: in-plane (x, z) -> 0.5; z: ceil(2.0 * 6 / 0.5) = 24
    assert B.geometry((20, 12, 6), (0.5, 1.0, 2.0), 1) == ((20, 12, 24), (0.5, 1.0, 0.5))
    # sagittal: in-plane (y, z) -> 1.0; z: ceil(2.0 * 6 / 1.0) = 12
    assert B.geometry((20, 12, 6), (0.5, 1.0, 2.0), 0) == ((20, 12, 12), (0.5, 1.0, 1.0))
    # a ratio that is no integer: ceil(0.7 * 10 / 0.3) = ceil(23.33) = 24; x: 0.3 * 7 / 0.3 is 7 or a hair above in floats
    size, spacing = B.geometry((7, 10, 3), (0.3, 0.7, 5.0), 2)
    assert spacing == (0.3, 0.3, 5.0) and size[1] == 24 and size[2] == 3
    assert size[0] == int(np.ceil(0.3 * 7 / 0.3))
    assert B.geometry((4, 4, 4), (1.0, 1.0, 1.0), 2) == ((4, 4, 4), (1.0, 1.0, 1.0))


# ---- render --------------------------------------------------------------------------------------------------------------------------
R_, C_, G_ = (255, 0, 0), (0, 255, 255), (0, 255, 0)


def _hand_case():
    """One 6 x 7 slice (V = 6 rows, U = 7 columns), window -128 .. 127: scale = 1, grey = trunc(v + 128) inside the window."""
    image = np.full((1, 6, 7), -128, dtype=np.float32)
    image[0, 0, :] = [-128, 127, 0.7, -50, 50.5, 300, -300]      # grey 0, 255, 128, 78, 178, 255, 0
    image[0, 1, 0] = np.nan                                      # 0
    image[0, 5, 6] = 20                                          # 148
    label = np.zeros((1, 6, 7), dtype=np.int32)
    label[0, 0, 2] = 1                                           # on grey 128
    label[0, 0, 4] = 2                                           # on grey 178
    label[0, 1, 0] = 3                                           # on the NaN
    label[0, 0, 3] = 9                                           # (9 - 1) mod 8 = 0: red again, on grey 78
    label[0, 0, 6] = -4                                          # background
    # box A class 1 at (1, 2) 2 x 2: outline columns 1 and 3, rows 2 and 4; box B class 2 at (2, 3) 2 x 1 drawn later: columns 2 and 4,
    # rows 3 and 4; box C class 3 at (5, 4) 3 x 4: its far edges (column 8, row 8) leave the image
    boxes = {0: [(1, 2, 2, 2, 1), (2, 3, 2, 1, 2), (5, 4, 3, 4, 3)]}
    return image, label, boxes


def _hand_picture(a):
    def mix(g, c):
        return tuple((g * (256 - a) + ch * a + 128) >> 8 for ch in c)

    def grey(g):
        return (g, g, g)
    z = grey(0)
    rows = [
        [z, grey(255), mix(128, R_), mix(78, R_), mix(178, C_), grey(255), z],
        [mix(0, G_), z, z, z, z, z, z],
        [z, R_, R_, R_, z, z, z],                       # A's top edge: columns 1 .. 3
        [z, R_, C_, C_, C_, z, z],                      # A's sides at 1 and 3; B's top edge 2 .. 4 wins at 3
        [z, R_, C_, C_, C_, G_, G_],                    # A's bottom 1 .. 3, B's bottom 2 .. 4 wins at 2, 3; C's top edge 5 .. 6
        [z, z, z, z, z, G_, grey(148)],                 # C's left side at column 5
    ]
    return np.asarray(rows, dtype=np.uint8).reshape(1, 6, 7, 3)


@pytest.mark.parametrize("opacity,a", [(0, 0), (0.37, 95), (1, 256)])
def test_render_hand_made_slice(opacity, a):
    image, label, boxes = _hand_case()
    assert B.alpha256(opacity) == a
    got = B.render(image, label, boxes, -128, 127, opacity)
    assert got.dtype == np.uint8 and got.shape == (1, 6, 7, 3)
    want = _hand_picture(a)
    assert np.array_equal(got, want), np.argwhere(got != want)
    if a == 0:
        assert tuple(got[0, 0, 2]) == (128, 128, 128)
    if a == 256:
        assert tuple(got[0, 0, 2]) == R_ and tuple(got[0, 1, 0]) == G_


def test_render_empty_window_and_grey_rule():
    image = np.asarray([[[4.0, 5.0, 6.0, np.nan, np.inf, -np.inf]]], dtype=np.float32)
    label = np.zeros((1, 1, 6), dtype=np.int32)
    got = B.render(image, label, {}, 5, 5, 0)
    assert got[0, 0, :, 0].tolist() == [0, 255, 255, 0, 255, 0] and np.array_equal(got[..., 0], got[..., 2])
    # truncation, not rounding: (v + 1024) * (255 / 2048) at v = 0 is 127.5 -> 127; one step of the window is 8.03 units
    g = B.grey(np.asarray([0.0, -1024.0, 1024.0, 1023.0, -1016.0, -1015.9], dtype=np.float32), -1024, 1024)
    assert g.tolist() == [127, 0, 255, 254, 0, 1]
    with pytest.raises(ValueError):
        B.render(image, label, {}, 0, 1, 1.5)


def test_png_bytes_decode_back():
    from vnet_tensorflow_amd import summary as S
    image, label, boxes = _hand_case()
    pic = B.render(image, label, boxes, -128, 127, 0.37)[0]
    assert np.array_equal(decode_png(S.encode_png(pic)), pic)


def decode_png(data):
    """uint8 [H, W, 3] of an 8-bit RGB PNG whose rows all carry filter type 0 (what summary.encode_png writes)."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, head = 8, b"", None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xffffffff
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    w, h, depth, colour = head[:4]
    assert depth == 8 and colour == 2
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(h, w, 3).copy()


def test_box_arrays_and_document():
    boxes = {0: [], 1: [(1, 2, 3, 4, 1), (5, 6, 7, 8, 2)], 2: [(0, 0, 1, 1, 1)]}
    flat, first = B.box_arrays(boxes, 3)
    assert flat.dtype == np.int32 and flat.tolist() == [[1, 2, 3, 4, 1], [5, 6, 7, 8, 2], [0, 0, 1, 1, 1]] and first.tolist() == [0, 0, 2, 3]
    flat, first = B.box_arrays({}, 2)
    assert flat.shape == (0, 5) and first.tolist() == [0, 0, 0]
    doc = B.boxes_document("axial", (0.5, 0.5, 2.0), (20, 24, 6), boxes, {"1": "liver"})
    assert json.loads(json.dumps(doc)) == {"direction": "axial", "spacing": [0.5, 0.5, 2.0], "size": [20, 24, 6],
                                           "boxes": {"0": [], "1": [[1, 2, 3, 4, 1, "liver"], [5, 6, 7, 8, 2, None]],
                                                     "2": [[0, 0, 1, 1, 1, "liver"]]}}


# ---- the ledger of csrc/vnet_bbox.h ------------------------------------------------------------------------------------------------
def test_bbox_header_ledger():
    """csrc/vnet_bbox.h beyond tests/test_abi_ledger.py: components.hip and bbox.hip include the union-find instead of holding copies;
    INTEGRATION.md names the header."""
    src = {n: open(os.path.join(ROOT, "vnet_tensorflow_amd", "csrc", n)).read() for n in ("components.hip", "bbox.hip", "cc_union.h")}
    assert '#include "cc_union.h"' in src["components.hip"] and '#include "cc_union.h"' in src["bbox.hip"]
    assert "cc_unite(" in src["cc_union.h"] and "void cc_unite(" not in src["components.hip"] and "void cc_unite(" not in src["bbox.hip"]
    assert "vnet_bbox.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_error_codes_need_no_device():
    """VNET_E_BADARG (-1), then VNET_E_UNSUPPORTED (-2), then VNET_E_WORKSPACE (-3): before any launch, in that order."""
    from vnet_tensorflow_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)
    big = (2048, 1024, 1024)                                     # 2^31 voxels
    for name in ("vnet_slice_stack_f32", "vnet_slice_stack_i32"):
        fn = getattr(L, name)
        assert fn(None, one, 5, 7, 9, 2, None) == -1 and fn(one, None, 5, 7, 9, 2, None) == -1
        assert fn(one, one, 5, 7, 9, 3, None) == -1 and fn(one, one, 5, 7, 9, -1, None) == -1
        for pos in range(3):
            for v in (0, -1):
                dims = [5, 7, 9]
                dims[pos] = v
                assert fn(one, one, *dims, 0, None) == -1, (name, pos, v)
        assert fn(one, one, *big, 1, None) == -2
        assert fn(one, one, *big, 3, None) == -1 and fn(None, one, *big, 1, None) == -1          # BADARG comes first
    q = L.vnet_plane_cc_table_ws_bytes
    assert q(5, 6, 7) == 8 * 210 + 16384 and q(*big) == 0 and q(0, 6, 7) == 0 and q(5, -1, 7) == 0
    fn = L.vnet_plane_cc_table
    ok = (one, one, one, 4, 5, 6, 7, one, 1 << 20, None)
    for pos in (0, 1, 2, 7):
        bad = list(ok)
        bad[pos] = None
        assert fn(*bad) == -1, pos
    assert fn(one, one, one, 4, 5, 6, 7, ctypes.c_void_p(20), 1 << 20, None) == -1               # ws not 8-byte aligned
    assert fn(one, one, one, 0, 5, 6, 7, one, 1 << 20, None) == -1 and fn(one, one, one, 4, 5, 0, 7, one, 1 << 20, None) == -1
    assert fn(one, one, one, 4, *big, one, 0, None) == -2                                        # UNSUPPORTED before WORKSPACE
    assert fn(one, one, one, 2 ** 31 - 1, 5, 6, 7, one, 0, None) == -2                           # a table an int32 cannot index
    assert fn(one, one, one, 0, *big, one, 0, None) == -1                                        # BADARG before UNSUPPORTED
    assert fn(one, one, one, 4, 5, 6, 7, one, q(5, 6, 7) - 1, None) == -3
    fn = L.vnet_bbox_render
    ok = (one, one, one, one, one, 3, 4, 5, -1024.0, 1024.0, 0.1245, 95, None)
    for pos in (0, 1, 3, 4):                                     # (boxes, position 2, may be null: nb == 0)
        bad = list(ok)
        bad[pos] = None
        assert fn(*bad) == -1, pos
    for alpha in (-1, 257):
        assert fn(*(ok[:11] + (alpha, None))) == -1
    for pos in (5, 6, 7):
        bad = list(ok)
        bad[pos] = 0
        assert fn(*bad) == -1
    assert fn(*(ok[:5] + big + ok[8:])) == -2
    assert fn(*(ok[:5] + big + ok[8:11] + (300, None))) == -1                                    # BADARG comes first


# ---- the tool's checks and the command line ------------------------------------------------------------------------------------------
def test_cli_defaults_are_the_reference_s_and_every_flag_reaches_the_object(tmp_path):
    import inspect
    a = B.get_parser().parse_args(["i.nii", "l.nii", "out"])
    assert (a.image, a.label, a.output, a.classname, a.format, a.verbose, a.opacity, a.direction, a.min, a.max, a.gpu) == (
        "i.nii", "l.nii", "out", None, "png", False, 0, "axial", -1024, 1024, None)
    sig = inspect.signature(B.BoundingBox.__init__)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[3:]] == [
        ("output_dir", "./output"), ("image_format", "png"), ("opacity", 0), ("direction", "axial"), ("min_intensity", -1024),
        ("max_intensity", 1024), ("classname_file", ""), ("device", None)]
    a = B.get_parser().parse_args(["i.nii", "l.nii", "out", "-c", "names.json", "-f", "png", "-o", "0.25", "-d", "coronal", "-m", "-200",
                                   "-M", "300", "--gpu", "1", "-v"])
    t = B.from_args(a)
    assert (t.image_path, t.label_path, t.output_dir, t.image_format, t.opacity, t.direction, t.min_intensity, t.max_intensity,
            t.classname_file, t.device) == ("i.nii", "l.nii", "out", "png", 0.25, "coronal", -200.0, 300.0, "names.json", "cuda:1")
    with pytest.raises(ValueError, match="png"):
        B.from_args(B.get_parser().parse_args(["i.nii", "l.nii", "out", "-f", "jpg"]))
    with pytest.raises(SystemExit):
        B.get_parser().parse_args(["i.nii", "l.nii", "out", "-d", "oblique"])


def test_run_checks_come_before_any_device_work(tmp_path):
    from vnet_tensorflow_amd import data
    with pytest.raises(IOError):
        B.BoundingBox(str(tmp_path / "no.nii"), str(tmp_path / "no.nii")).run()
    img, lab = str(tmp_path / "i.nii"), str(tmp_path / "l.nii")
    data.write_nifti(img, np.zeros((3, 4, 5), dtype=np.float32), (0.5, 1.0, 2.0))
    data.write_nifti(lab, np.zeros((3, 4, 5), dtype=np.int16), (0.5, 1.0, 2.0))
    with pytest.raises(ValueError, match="png"):
        B.BoundingBox(img, lab, str(tmp_path / "o"), image_format="jpg").run()
    with pytest.raises(ValueError, match="Opacity"):
        B.BoundingBox(img, lab, str(tmp_path / "o"), opacity=1.5).run()
    with pytest.raises(ValueError, match="direction"):
        B.BoundingBox(img, lab, str(tmp_path / "o"), direction="oblique").run()
    assert not (tmp_path / "o").exists()
    arr, spacing = B.read_volume(img)
    assert arr.shape == (3, 4, 5) and spacing == (0.5, 1.0, 2.0)
    np.save(str(tmp_path / "i.npy"), np.zeros((2, 2, 2), dtype=np.float32))
    assert B.read_volume(str(tmp_path / "i.npy"))[1] == (1.0, 1.0, 1.0)

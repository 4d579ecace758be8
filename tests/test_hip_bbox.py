"""-m gpu: the device side of the bounding-box tool (csrc/bbox.hip, csrc/vnet_bbox.h) against the NumPy rules of
vnet_tensorflow_amd/bounding_box.py.  Every comparison is `==`: the stack is a permutation, the table is integers, and every byte of
the picture is an exact integer rule.  The shapes are the smallest at which each failure mode can show: ragged tiles, one voxel, a
wave that holds the end of one row and the start of the next, more work than one trip of the capped grid."""
import json
import os

import numpy as np
import pytest
import torch

from tests.test_bbox_host import decode_png
from tests.util import g
from vnet_tensorflow_amd import bounding_box as B

pytestmark = pytest.mark.gpu


# ---- slice_stack ---------------------------------------------------------------------------------------------------------------------
# (2, 4100, 3): 4100 tiles for axes 1 and 2, above the launch's cap of 4096 workgroups
@pytest.mark.parametrize("shape", [(5, 7, 9), (33, 65, 17), (1, 1, 1), (70, 3, 130), (2, 4100, 3)])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_slice_stack(dev, shape, axis):
    from vnet_tensorflow_amd import ops
    rng = np.random.default_rng(axis)
    xf = rng.standard_normal(shape).astype(np.float32)
    xf.flat[0] = np.nan                                          # (a bit copy: the NaN's payload survives too)
    xi = rng.integers(-5, 2 ** 31 - 1, shape).astype(np.int32)
    got = ops.slice_stack(g(xf, dev), axis)
    assert got.dtype == torch.float32 and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy().view(np.uint32), B.stack(xf, axis).view(np.uint32))
    got = ops.slice_stack(g(xi, dev, torch.int32), axis)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), B.stack(xi, axis))


# ---- plane_component_table -------------------------------------------------------------------------------------------------------------
def _serpentine(n=33):
    """A one-voxel-wide path that fills every even row and joins consecutive even rows at alternating ends."""
    s = np.zeros((1, n, n), dtype=np.int32)
    s[0, 0::2, :] = 3
    for k, v in enumerate(range(1, n, 2)):
        s[0, v, n - 1 if k % 2 == 0 else 0] = 3
    return s


def _row_ends():
    """(3, 5, 130): in every row a run that ends exactly at u = U - 1 and a run that starts at u = 0; the value at the end of a row
    is the value at the start of the NEXT row (also across the last row of a slice and the first of the next), so the two are
    neighbours in memory -- inside one wave, since 130 is no multiple of 64 -- and never in the slice."""
    s = np.zeros((3, 5, 130), dtype=np.int32)
    for r in range(15):
        z, v = divmod(r, 5)
        s[z, v, :3] = 1 + r % 2
        s[z, v, 127:] = 1 + (r + 1) % 2
    return s


def _full_rows():
    """(3, 5, 130) of one value: every run spans its row, one component per slice."""
    return np.full((3, 5, 130), 2, dtype=np.int32)


def _random(shape, seed):
    return np.random.default_rng(seed).choice(4, size=shape, p=(0.4, 0.2, 0.2, 0.2)).astype(np.int32)


def _diagonal():
    s = np.zeros((1, 4, 4), dtype=np.int32)
    s[0, 1, 1] = s[0, 2, 2] = 1
    return s


def _board():
    v, u = np.mgrid[0:8, 0:8]
    return np.ascontiguousarray(np.broadcast_to(1 + (u + v) % 2, (2, 8, 8))).astype(np.int32)


STACKS = {
    "ones 5x6x7": lambda: np.ones((5, 6, 7), dtype=np.int32),
    "board 2x8x8": _board,
    "diagonal": _diagonal,
    "row ends 3x5x130": _row_ends,
    "full rows 3x5x130": _full_rows,
    "random 2x70x67": lambda: _random((2, 70, 67), 1),
    "random 4x1x9": lambda: _random((4, 1, 9), 2),
    "random 4x9x1": lambda: _random((4, 9, 1), 3),
    "one voxel": lambda: np.full((1, 1, 1), 7, dtype=np.int32),
    "one background voxel": lambda: np.full((1, 1, 1), -2, dtype=np.int32),
    "serpentine 33x33": _serpentine,
    "random 3x40x70": lambda: _random((3, 40, 70), 4),
    # 1 051 650 voxels: more than one trip of the 4096 x 256 grid of every pass
    "random 2x513x1025": lambda: _random((2, 513, 1025), 5),
}


@pytest.mark.parametrize("name", sorted(STACKS))
def test_plane_component_table(dev, name):
    from vnet_tensorflow_amd import ops
    stk = STACKS[name]()
    want_n, want = B.plane_components(stk)
    n, rows, classes = ops.plane_component_table(g(stk, dev, torch.int32))
    assert n == want_n and rows.dtype == np.int32 and rows.shape == (n, 8)
    assert np.array_equal(rows, want), "rows differ at %s" % (np.argwhere(rows != want)[:5].tolist(),)
    assert np.array_equal(classes, stk.reshape(-1)[want[:, 0]])
    if name == "ones 5x6x7":
        assert n == 5 and rows[:, 1].tolist() == [42] * 5                          # slices do not merge
    if name == "board 2x8x8":
        assert n == 128 and set(rows[:, 1].tolist()) == {1}                        # classes do not merge
    if name == "diagonal":
        assert n == 2
    if name == "serpentine 33x33":
        assert n == 1 and rows[0].tolist() == [0, 17 * 33 + 16, 0, 0, 0, 0, 32, 32]
    if name == "row ends 3x5x130":
        assert n == 30 and set(rows[:, 1].tolist()) == {3}
    if name == "full rows 3x5x130":
        assert n == 3 and rows[:, 1].tolist() == [650] * 3
    if stk.size < 20000:                              # (the greedy suppression of 10^5 boxes of one class takes minutes on the host)
        assert B.boxes_of_rows(stk.shape[0], rows, classes) == B.slice_boxes(stk)


def test_plane_component_table_capacity(dev):
    """n is the true count past the capacity; the rows from min(n, capacity) up are 0; the wrapper runs once more with capacity n."""
    from vnet_tensorflow_amd import _lib, ops
    stk = _random((3, 40, 70), 4)
    want_n, want = B.plane_components(stk)
    assert want_n > 64
    t = g(stk, dev, torch.int32)
    L = _lib.lib()
    need = L.vnet_plane_cc_table_ws_bytes(3, 40, 70)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = torch.full((4 * 8 + 1,), -1, dtype=torch.int32, device=dev)
    assert L.vnet_plane_cc_table(t.data_ptr(), out.data_ptr() + 4 * 32, out.data_ptr(), 4, 3, 40, 70, ws.data_ptr(), need, stream) == 0
    host = out.cpu().numpy()
    assert host[32] == want_n and np.array_equal(host[:32].reshape(4, 8), want[:4])
    few = _row_ends()[:1, :2]                                                      # 4 components
    out = torch.full((16 * 8 + 1,), -1, dtype=torch.int32, device=dev)
    need2 = L.vnet_plane_cc_table_ws_bytes(1, 2, 130)
    assert L.vnet_plane_cc_table(g(few, dev, torch.int32).data_ptr(), out.data_ptr() + 4 * 128, out.data_ptr(), 16, 1, 2, 130,
                                 ws.data_ptr(), need2, stream) == 0
    host = out.cpu().numpy()
    assert host[128] == 4 and np.array_equal(host[:32].reshape(4, 8), B.plane_components(few)[1]) and not host[32:128].any()
    n, rows, classes = ops.plane_component_table(t, max_components=4)
    assert n == want_n and np.array_equal(rows, want) and np.array_equal(classes, stk.reshape(-1)[want[:, 0]])
    with pytest.raises(Exception):
        ops.plane_component_table(t, ws=torch.empty(need - 8, dtype=torch.uint8, device=dev))


# ---- bbox_render -----------------------------------------------------------------------------------------------------------------------
def _render_case(shape, seed):
    rng = np.random.default_rng(seed)
    image = (rng.standard_normal(shape) * 700).astype(np.float32)
    image.reshape(-1)[rng.integers(0, image.size, 40)] = np.nan
    image.reshape(-1)[:4] = [-1024, 1024, np.inf, -np.inf]
    label = rng.choice(12, size=shape, p=(0.45,) + (0.05,) * 11).astype(np.int32) - 1          # -1 .. 10: background, all 8 colours, a wrap
    return image, label


def _device_render(dev, image, label, boxes, wmin, wmax, opacity):
    from vnet_tensorflow_amd import ops
    flat, first = B.box_arrays(boxes, label.shape[0])
    return ops.bbox_render(g(image, dev), g(label, dev, torch.int32), g(flat, dev, torch.int32), g(first, dev, torch.int32),
                           wmin, wmax, opacity).cpu().numpy()


@pytest.mark.parametrize("opacity", [0, 0.37, 1])
def test_bbox_render_random_stack(dev, opacity):
    image, label = _render_case((3, 19, 70), 7)
    boxes = B.slice_boxes(np.where(label > 3, 0, label))
    boxes[1] = boxes[1] + [(60, 10, 9, 8, 2), (69, 18, 5, 5, 3), (0, 0, 69, 18, 4), (0, 0, 70, 19, 5), (68, 17, 1, 1, 9)]   # the last row and column
    want = B.render(image, label, boxes, -1024, 1024, opacity)
    got = _device_render(dev, image, label, boxes, -1024, 1024, opacity)
    assert got.dtype == np.uint8 and got.shape == (3, 19, 70, 3)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()


def test_bbox_render_no_boxes_and_empty_window(dev):
    image, label = _render_case((2, 5, 9), 8)
    for wmin, wmax in ((-1024, 1024), (0, 0), (-0.3, 811.7), (50, -50)):
        got = _device_render(dev, image, label, {}, wmin, wmax, 0.37)
        assert np.array_equal(got, B.render(image, label, {}, wmin, wmax, 0.37)), (wmin, wmax)
    one = _device_render(dev, np.full((1, 1, 1), 3.5, np.float32), np.ones((1, 1, 1), np.int32), {0: [(0, 0, 1, 1, 2)]}, 0, 7, 1)
    assert one.tolist() == [[[[0, 255, 255]]]]


def test_bbox_render_more_boxes_than_one_chunk(dev):
    """600 boxes in one slice (an LDS chunk holds 256), none in the next, 300 in the last; later boxes win across chunk borders."""
    rng = np.random.default_rng(9)
    image, label = _render_case((3, 40, 50), 10)

    def draw(n):
        return [(int(x), int(y), int(w), int(h), int(c)) for x, y, w, h, c in
                np.stack([rng.integers(0, 50, n), rng.integers(0, 40, n), rng.integers(0, 12, n), rng.integers(0, 12, n),
                          rng.integers(1, 9, n)], axis=1)]
    boxes = {0: draw(600), 1: [], 2: draw(300)}
    want = B.render(image, label, boxes, -1024, 1024, 0.37)
    got = _device_render(dev, image, label, boxes, -1024, 1024, 0.37)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """A 20 x 12 x 6 pair with spacing (0.5, 1.0, 2.0).  The image holds multiples of 8: every blend weight of the three directions is
    a multiple of 1/4, so the linear resampling is exact in any arithmetic and the end-to-end comparison can be `==` (the resampling
    kernel's own rounding has its own test, tests/test_hip_resample.py)."""
    from vnet_tensorflow_amd import data
    d = tmp_path_factory.mktemp("bbox_case")
    rng = np.random.default_rng(11)
    image = (rng.integers(-150, 150, (20, 12, 6)) * 8).astype(np.float32)
    label = np.zeros((20, 12, 6), dtype=np.int16)
    label[2:9, 1:5, 0:4] = 1
    label[11:18, 6:11, 2:6] = 2
    label[4:6, 8:10, :] = 1
    label[rng.random((20, 12, 6)) < 0.05] = 2
    paths = str(d / "image.nii"), str(d / "label.nii")
    data.write_nifti(paths[0], image, (0.5, 1.0, 2.0))
    data.write_nifti(paths[1], label, (0.5, 1.0, 2.0))
    names = str(d / "names.json")
    with open(names, "w") as f:
        json.dump({"1": "liver"}, f)
    return paths + (names, image, label.astype(np.int32))


@pytest.mark.parametrize("direction", ["axial", "coronal", "sagittal"])
def test_end_to_end(dev, case, tmp_path, direction):
    from vnet_tensorflow_amd import resample as R
    image_path, label_path, names, image, label = case
    out = str(tmp_path / "out")
    tool = B.BoundingBox(image_path, label_path, out, opacity=0.37, direction=direction, min_intensity=-1024, max_intensity=1024,
                         classname_file=names, device=dev)
    got_boxes = tool.run()
    axis = B.DIRECTIONS[direction]
    spacing = (0.5, 1.0, 2.0)
    size, new_spacing = B.geometry(image.shape, spacing, axis)
    assert size == {"axial": (20, 24, 6), "coronal": (20, 12, 24), "sagittal": (20, 12, 12)}[direction]
    ratio = R.ratios(spacing, new_spacing)
    xs = B.stack(R.linear(image, size, ratio), axis)
    ls = B.stack(R.nearest(label, size, ratio), axis)
    boxes = B.slice_boxes(ls)
    assert got_boxes == boxes and sum(len(v) for v in boxes.values()) > 0
    want = B.render(xs, ls, boxes, -1024, 1024, 0.37)
    S = ls.shape[0]
    assert sorted(os.listdir(out)) == sorted(["boxes.json"] + [str(s).zfill(3) + ".png" for s in range(S)])
    for s in range(S):
        with open(os.path.join(out, str(s).zfill(3) + ".png"), "rb") as f:
            assert np.array_equal(decode_png(f.read()), want[s]), s
    with open(os.path.join(out, "boxes.json")) as f:
        doc = json.load(f)
    assert doc == json.loads(json.dumps(B.boxes_document(direction, new_spacing, size, boxes, {"1": "liver"})))
    assert any(row[5] == "liver" for rows in doc["boxes"].values() for row in rows)

"""The reference's utils/bounding_box on the device: for every slice of a case the 2-D connected components of each class, their
bounding boxes merged by a greedy non-maximum suppression, and one picture per slice -- windowed grey image, label overlay, box
outlines.  File to PNGs with one upload and one download (csrc/bbox.hip, csrc/vnet_bbox.h).

The functions in front are the RULES, NumPy restatements the kernels are held to with `==`; the product path (BoundingBox.run) never
calls them for per-voxel work -- only suppress(), a few boxes per slice, runs on the host there.

    python -m vnet_tensorflow_amd.bounding_box IMAGE LABEL OUTPUT [-c JSON] [-f png] [-o OPACITY] [-d axial|coronal|sagittal]
                                               [-m MIN] [-M MAX] [-v] [--gpu N]

Three departures from the reference, stated in DESIGN.md section 6h: boxes that share y + h are ordered by a STABLE sort; the picture
is one pixel per voxel by exact integer rules (what is pinned to the reference is the box list, not matplotlib's rendering); coronal and
sagittal, which the reference accepts and then fails on, follow the axial rule on their own in-plane pair.  No JPEG (there is no
encoder) and no text in the picture (there is no font): class names go into boxes.json."""
import argparse
import json
import math
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

DIRECTIONS = {"axial": 2, "coronal": 1, "sagittal": 0}
# classes 1 and 2 are the reference's red and cyan
PALETTE = ((255, 0, 0), (0, 255, 255), (0, 255, 0), (255, 255, 0), (255, 0, 255), (255, 128, 0), (0, 128, 255), (255, 255, 255))
CC_ROW = 8
# the rendered stack comes down in pieces of at most this many bytes (whole slices; at least one)
DOWNLOAD_BYTES = 256 << 20
_STACK_AXES = {2: (2, 1, 0), 1: (1, 2, 0), 0: (0, 2, 1)}


# ---- the rules --------------------------------------------------------------------------------------------------------------------
def stack(volume, axis):
    """[X,Y,Z] -> [S,V,U]: S the slicing axis (2 axial, 1 coronal, 0 sagittal), u the lower-numbered in-plane axis and v the higher --
    what ITK's ExtractImageFilter leaves when one axis collapses.  u is the box's x and the PNG column, v the box's y and the PNG row."""
    volume = np.asarray(volume)
    if volume.ndim != 3 or axis not in _STACK_AXES:
        raise ValueError("stack: takes [X,Y,Z] and an axis of 0, 1, 2; got %s, axis %r" % (volume.shape, axis))
    return np.ascontiguousarray(np.transpose(volume, _STACK_AXES[axis]))


def plane_components(stk):
    """(n, int32 rows [n, 8]) of an integer stack [S,V,U].  A component is a maximal set of voxels with the same value > 0, in the same
    slice, joined through u +- 1 / v +- 1 neighbours; values <= 0 are background.  Row = {representative, count, lo_s, lo_v, lo_u,
    hi_s, hi_v, hi_u}: the representative is the smallest linear index (s * V + v) * U + u of the component, hi is inclusive, rows in
    ascending representative order -- slice by slice, inside a slice in raster order with u fastest (this project's rule for the
    order ITK numbers objects in; it matters only for ties in suppress())."""
    stk = np.asarray(stk)
    if stk.ndim != 3:
        raise ValueError("plane_components: takes [S,V,U], got %s" % (stk.shape,))
    S, V, U = stk.shape
    fg = stk > 0
    big = np.int64(stk.size)
    rep = np.where(fg, np.arange(stk.size, dtype=np.int64).reshape(stk.shape), big)
    same_u = fg[:, :, 1:] & (stk[:, :, 1:] == stk[:, :, :-1])              # voxel (.., u) and (.., u - 1) belong together
    same_v = fg[:, 1:, :] & (stk[:, 1:, :] == stk[:, :-1, :])
    while True:                                                            # the smallest index spreads until nothing changes
        new = rep.copy()
        np.minimum(new[:, :, 1:], np.where(same_u, rep[:, :, :-1], big), out=new[:, :, 1:])
        np.minimum(new[:, :, :-1], np.where(same_u, rep[:, :, 1:], big), out=new[:, :, :-1])
        np.minimum(new[:, 1:, :], np.where(same_v, rep[:, :-1, :], big), out=new[:, 1:, :])
        np.minimum(new[:, :-1, :], np.where(same_v, rep[:, 1:, :], big), out=new[:, :-1, :])
        if np.array_equal(new, rep):
            break
        rep = new
    where = np.nonzero(fg.reshape(-1))[0]
    reps, inverse, counts = np.unique(rep.reshape(-1)[where], return_inverse=True, return_counts=True)
    n = int(reps.size)
    rows = np.zeros((n, CC_ROW), dtype=np.int64)
    rows[:, 0], rows[:, 1] = reps, counts
    coords = np.stack(np.unravel_index(where, stk.shape), axis=1)
    lo = np.full((n, 3), np.iinfo(np.int64).max)
    hi = np.zeros((n, 3), dtype=np.int64)
    np.minimum.at(lo, inverse.reshape(-1), coords)
    np.maximum.at(hi, inverse.reshape(-1), coords)
    rows[:, 2:5], rows[:, 5:8] = lo, hi
    return n, rows.astype(np.int32)


def suppress(boxes, thresh=0.5):
    """The greedy suppression of the reference's non_max_suppression_fast on (x, y, w, h) rows: sort by y + h with a STABLE sort, pick
    from the end, drop every remaining box whose intersection with the pick is more than `thresh` of the remaining box's own area
    (the + 1 in widths, heights and areas as in the reference).  The picks, in pick order, as int64 [k, 4]."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    left, top = b[:, 0], b[:, 1]
    right, bottom = left + b[:, 2], top + b[:, 3]
    area = (right - left + 1) * (bottom - top + 1)
    remaining = np.argsort(bottom, kind="stable")
    picks = []
    while remaining.size:
        i, remaining = remaining[-1], remaining[:-1]
        picks.append(int(i))
        w = np.maximum(0.0, np.minimum(right[i], right[remaining]) - np.maximum(left[i], left[remaining]) + 1)
        h = np.maximum(0.0, np.minimum(bottom[i], bottom[remaining]) - np.maximum(top[i], top[remaining]) + 1)
        remaining = remaining[~((w * h) / area[remaining] > thresh)]
    return b[picks].astype(np.int64).reshape(-1, 4)


def boxes_of_rows(S, rows, classes):
    """{s: [(x, y, w, h, label), ...]} for every slice 0 .. S - 1 from component rows and the class of each row: labels ascending,
    inside a label suppress()'s pick order on the rows in table order.  (x, y, w, h) = (lo_u, lo_v, hi_u - lo_u + 1, hi_v - lo_v + 1)."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, CC_ROW)
    classes = np.asarray(classes, dtype=np.int64).reshape(-1)
    out = {s: [] for s in range(int(S))}
    xywh = np.stack([rows[:, 4], rows[:, 3], rows[:, 7] - rows[:, 4] + 1, rows[:, 6] - rows[:, 3] + 1], axis=1)
    order = np.lexsort((np.arange(rows.shape[0]), classes, rows[:, 2]))        # slice, then class, then table order
    key = np.stack([rows[order, 2], classes[order]], axis=1)
    cuts = np.nonzero(np.any(key[1:] != key[:-1], axis=1))[0] + 1 if len(order) else np.zeros(0, dtype=np.int64)
    for grp in np.split(order, cuts) if len(order) else []:
        s, label = int(rows[grp[0], 2]), int(classes[grp[0]])
        out[s].extend((int(x), int(y), int(w), int(h), label) for x, y, w, h in suppress(xywh[grp]))
    return out


def slice_boxes(stk):
    """{s: [(x, y, w, h, label), ...]} of an integer stack [S,V,U], empty slices included."""
    stk = np.asarray(stk)
    _, rows = plane_components(stk)
    return boxes_of_rows(stk.shape[0], rows, stk.reshape(-1)[rows[:, 0]])


def geometry(size, spacing, axis):
    """(new_size, new_spacing): the in-plane spacing becomes the smaller of the two in-plane spacings, the through-slice spacing stays;
    new_size[i] = int(ceil(old_spacing[i] * old_size[i] / new_spacing[i])) in Python floats.  The reference defines this for axial;
    the two other directions take the same rule on their own in-plane pair."""
    if axis not in _STACK_AXES:
        raise ValueError("geometry: axis %r (0, 1, 2)" % (axis,))
    spacing = tuple(float(v) for v in spacing)
    size = tuple(int(v) for v in size)
    small = min(spacing[a] for a in range(3) if a != axis)
    new_spacing = tuple(spacing[a] if a == axis else small for a in range(3))
    new_size = tuple(int(math.ceil(spacing[i] * size[i] / new_spacing[i])) for i in range(3))
    return new_size, new_spacing


def alpha256(opacity):
    return int(round(float(opacity) * 256))


def window_scale(wmin, wmax):
    """float32(255) / (float32(wmax) - float32(wmin)), formed once on the host (inf for an empty window, which the rule never uses)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float32(255) / (np.float32(wmax) - np.float32(wmin))


def grey(image, wmin, wmax):
    """The grey byte: trunc(clamp((v - wmin) * scale, 0, 255)), each operation rounded in float32; NaN gives 0; wmax == wmin: 0 where
    v < wmin and 255 elsewhere (NaN still 0)."""
    v = np.asarray(image, dtype=np.float32)
    lo, hi = np.float32(wmin), np.float32(wmax)
    if lo == hi:
        g = np.where(v < lo, 0, 255)
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            t = ((v - lo).astype(np.float32) * window_scale(wmin, wmax)).astype(np.float32)
        g = np.where(t > 0, np.minimum(t, np.float32(255)), np.float32(0)).astype(np.int64)
    return np.where(np.isnan(v), 0, g).astype(np.int64)


def render(image_stack, label_stack, boxes, wmin, wmax, opacity):
    """uint8 [S,V,U,3]: the picture of every slice, by exact integer rules.  boxes: {s: [(x, y, w, h, label), ...]} (slice_boxes).
    Overlay: a = round(opacity * 256); where the label l > 0 each channel is (g * (256 - a) + c * a + 128) >> 8 with c of
    PALETTE[(l - 1) mod 8].  Outlines in list order, later boxes win: (u, v) is on the outline of (x, y, w, h) when (u == x or
    u == x + w) and y <= v <= y + h, or (v == y or v == y + h) and x <= u <= x + w -- matplotlib's Rectangle((x, y), w, h) through
    pixel centres; the far edge lies one pixel past the box and is not there where that is outside the image."""
    label_stack = np.asarray(label_stack)
    S, V, U = label_stack.shape
    a = alpha256(opacity)
    if not 0 <= a <= 256:
        raise ValueError("render: opacity %r outside [0, 1]" % (opacity,))
    pal = np.asarray(PALETTE, dtype=np.int64)
    g = grey(image_stack, wmin, wmax)
    out = np.repeat(g[..., None], 3, axis=3)
    colour = pal[(label_stack.astype(np.int64) - 1) % 8]
    out = np.where((label_stack > 0)[..., None], (g[..., None] * (256 - a) + colour * a + 128) >> 8, out)
    v, u = np.mgrid[0:V, 0:U]
    for s in range(S):
        for x, y, w, h, label in boxes.get(s, ()):
            edge = (((u == x) | (u == x + w)) & (y <= v) & (v <= y + h)) | (((v == y) | (v == y + h)) & (x <= u) & (u <= x + w))
            out[s][edge] = pal[(int(label) - 1) % 8]
    return out.astype(np.uint8)


def box_arrays(boxes, S):
    """The two arrays of vnet_bbox_render: int32 [nb, 5] rows {x, y, w, h, label} grouped by slice, and int32 [S + 1] offsets."""
    flat, first = [], [0]
    for s in range(int(S)):
        flat.extend(boxes.get(s, ()))
        first.append(len(flat))
    return np.asarray(flat, dtype=np.int32).reshape(-1, 5), np.asarray(first, dtype=np.int32)


def boxes_document(direction, spacing, size, boxes, classnames):
    """What boxes.json holds: {"direction", "spacing", "size", "boxes": {slice: [[x, y, w, h, label, name-or-null], ...]}}."""
    return {"direction": direction, "spacing": [float(v) for v in spacing], "size": [int(v) for v in size],
            "boxes": {str(s): [[x, y, w, h, label, classnames.get(str(label))] for x, y, w, h, label in rows]
                      for s, rows in sorted(boxes.items())}}


def read_volume(path):
    """(array [X,Y,Z], spacing) of a .nii, .nii.gz or .npy (spacing 1) file."""
    from . import data
    if path.endswith(".npy"):
        return np.load(path), (1.0, 1.0, 1.0)
    arr, hdr = data.read_nifti(path)
    return arr, tuple(float(v) for v in hdr["pixdim"])


# ---- the tool -----------------------------------------------------------------------------------------------------------------------
class BoundingBox(object):
    """Parameter names, order and defaults are the reference's; `device` is appended.  run() returns the slice_boxes dict."""

    def __init__(self, image_path, label_path, output_dir="./output", image_format="png", opacity=0, direction="axial",
                 min_intensity=-1024, max_intensity=1024, classname_file="", device=None):
        self.image_path = image_path
        self.label_path = label_path
        self.output_dir = output_dir
        self.image_format = image_format
        self.opacity = opacity
        self.direction = direction
        self.min_intensity = min_intensity
        self.max_intensity = max_intensity
        self.classname_file = classname_file
        self.classnames = {}
        self.device = device
        self.times = {}

    def check(self):
        if not (os.path.exists(self.image_path) and os.path.exists(self.label_path)):
            raise IOError("Input image/label file not exist")
        if self.image_format != "png":
            raise ValueError("Output image format can only be png (there is no %s encoder here)" % (self.image_format,))
        if not 0 <= self.opacity <= 1:
            raise ValueError("Opacity should between 0 and 1")
        if self.direction not in DIRECTIONS:
            raise ValueError("Image direction can only be axial, coronal or sagittal")

    def run(self):
        import time
        import torch
        from . import ops, resample as R, summary
        self.check()
        os.makedirs(self.output_dir, exist_ok=True)
        if self.classname_file and os.path.exists(self.classname_file):
            with open(self.classname_file, "r") as f:
                self.classnames = json.load(f)
        axis = DIRECTIONS[self.direction]
        image, spacing = read_volume(self.image_path)
        label, _ = read_volume(self.label_path)
        if image.ndim != 3 or image.shape != label.shape:
            raise ValueError("image %s and label %s are not one 3-D grid" % (image.shape, label.shape))
        dev = torch.device(self.device if self.device is not None else "cuda")
        clock = time.perf_counter

        def sync():
            torch.cuda.synchronize(dev)
            return clock()
        t0 = clock()
        # one upload
        x = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).to(dev)
        l = torch.from_numpy(np.ascontiguousarray(label).astype(np.int32)).to(dev)
        t1 = sync()
        new_size, new_spacing = geometry(image.shape, spacing, axis)
        ratio = R.ratios(spacing, new_spacing)
        if any(r != 1.0 for r in ratio) or new_size != tuple(image.shape):
            x = ops.resample(x, new_size, ratio, "linear")
            l = ops.resample(l, new_size, ratio, "nearest")
        xs, ls = ops.slice_stack(x, axis), ops.slice_stack(l, axis)
        S, V, U = (int(v) for v in ls.shape)
        _, rows, classes = ops.plane_component_table(ls)
        t2 = sync()
        boxes = boxes_of_rows(S, rows, classes)
        flat, first = box_arrays(boxes, S)
        t3 = clock()
        rgb = ops.bbox_render(xs, ls, torch.from_numpy(flat).to(dev), torch.from_numpy(first).to(dev),
                              self.min_intensity, self.max_intensity, self.opacity)
        t4 = sync()
        # one pinned copy down, in pieces of whole slices when the stack is larger than DOWNLOAD_BYTES
        per = max(1, DOWNLOAD_BYTES // (V * U * 3))
        host = torch.empty((min(per, S), V, U, 3), dtype=torch.uint8).pin_memory()
        tcopy = tpng = 0.0
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            for s0 in range(0, S, per):
                c0 = clock()
                part = host[:min(per, S - s0)]
                part.copy_(rgb[s0:s0 + part.shape[0]])
                pixels = part.numpy()
                c1 = clock()
                list(pool.map(self._write, [(s0 + k, pixels[k]) for k in range(part.shape[0])],
                              [summary.encode_png] * part.shape[0]))
                tcopy, tpng = tcopy + (c1 - c0), tpng + (clock() - c1)
        with open(os.path.join(self.output_dir, "boxes.json"), "w") as f:
            json.dump(boxes_document(self.direction, new_spacing, new_size, boxes, self.classnames), f)
        self.times = {"upload": t1 - t0, "device": (t2 - t1) + (t4 - t3), "suppress": t3 - t2, "download": tcopy, "png": tpng}
        return boxes

    def _write(self, job, encode):
        s, pixels = job
        with open(os.path.join(self.output_dir, str(s).zfill(3) + "." + self.image_format), "wb") as f:
            f.write(encode(pixels))


# ---- command line -------------------------------------------------------------------------------------------------------------------
def get_parser():
    p = argparse.ArgumentParser(prog="python -m vnet_tensorflow_amd.bounding_box",
                                description="Draw bounding boxes from NIfTI segmentation labels, slice by slice, on the device.")
    p.add_argument("image", help="Input NIfTI image", type=str, metavar="PATH")
    p.add_argument("label", help="Input NIfTI label", type=str, metavar="PATH")
    p.add_argument("output", help="Output directory", default="./output", type=str, metavar="DIR")
    p.add_argument("-c", dest="classname", help="Class name JSON file", type=str, metavar="JSON")
    p.add_argument("-f", "--format", dest="format", help="Output image format (png)", default="png", metavar="[png]")
    p.add_argument("-v", "--verbose", dest="verbose", help="Show verbose output", action="store_true")
    p.add_argument("-o", "--opacity", dest="opacity", default=0, type=float, help="Segmentation label opacity (default=0)",
                   metavar="FLOAT [0-1]")
    p.add_argument("-d", "--direction", dest="direction", help="Image series direction (default=axial)",
                   choices=["axial", "sagittal", "coronal"], default="axial", metavar="[axial sagittal coronal]")
    p.add_argument("-m", "--min", dest="min", default=-1024, type=float, help="Minimum image intensity (default=-1024)", metavar="FLOAT")
    p.add_argument("-M", "--max", dest="max", default=1024, type=float, help="Maximum image intensity (default=1024)", metavar="FLOAT")
    p.add_argument("--gpu", dest="gpu", default=None, type=int, help="Device index (default: the current device)", metavar="N")
    return p


def from_args(args):
    """Every flag reaches the object (the reference's main.py drops -f and -d)."""
    if args.format != "png":
        raise ValueError("Output image format can only be png (there is no %s encoder here)" % (args.format,))
    return BoundingBox(args.image, args.label, args.output, image_format=args.format, opacity=args.opacity, direction=args.direction,
                       min_intensity=args.min, max_intensity=args.max, classname_file=args.classname or "",
                       device=None if args.gpu is None else "cuda:%d" % args.gpu)


def main(argv=None):
    args = get_parser().parse_args(argv)
    if args.verbose:
        for key, value in sorted(vars(args).items()):
            print("{} = {}".format(key, value))
    tool = from_args(args)
    boxes = tool.run()
    if args.verbose:
        print("%d slices, %d boxes" % (len(boxes), sum(len(v) for v in boxes.values())))
        print(" ".join("%s %.3fs" % kv for kv in sorted(tool.times.items())))
    return 0


if __name__ == "__main__":
    sys.exit(main())

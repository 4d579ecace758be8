"""The reference's utils/prepare_data on the device: image_fit_label.py (mask the image by the dilated selection of its label, crop
image and label to the selection's box), binarize.py (the selection as a 0/1 label, the image masked by a dilated second selection) and
image_partition.py (a case cut into slabs along z).  The dilation by ITK's ball, the bounding box and the masked crop run on the
device on bit-packed masks (morph.py, csrc/morph.hip, csrc/vnet_tools.h); each file goes up once in its own
dtype and each result comes down once.

The functions in front are the RULES, NumPy restatements the kernels are held to with `==`; the product path (FitLabel.run,
Binarize.run) calls none of them for per-voxel work -- only fit_window(), six numbers, runs on the host there.

    python -m vnet_tensorflow_amd.prepare_data fit-label SRC TGT [--select 1 2] [--buffer 2] [--mask-dilation 2] [--mask-dim 0 1 2]
                                               [--no-mask] [--image image.nii] [--label label.nii]
                                               [--out-image image_cropped.nii.gz] [--out-label label_cropped.nii.gz] [--gpu N] [-v]
    python -m vnet_tensorflow_amd.prepare_data binarize SRC TGT [--select 2] [--mask-label ...] [--mask-dilation 5]
                                               [--image image_cropped.nii.gz] [--label label_cropped.nii.gz]
                                               [--out-image image_masked.nii.gz] [--out-label label_masked.nii.gz] [--gpu N] [-v]
    python -m vnet_tensorflow_amd.prepare_data partition SRC TGT [--layer 64] [--image image_cropped.nii] [--label label_cropped.nii]
                                               [--out-image image.nii.gz] [--out-label label.nii.gz] [-v]

The flags replace the constants the reference's scripts have edited in; the defaults are the reference's values.  Every case is a
sub-directory of SRC.  Files are written by this project's convention (data.write_nifti): uncompressed, a `.nii.gz` name written as
`.nii`, the spacing kept, no origin or direction.  A case whose selection is empty is reported and skipped (the reference raises there).
Left out: unify_header.py, check_header_consistency.py, lits.py, adam_unzip.py -- file names and header fields only."""
import argparse
import os
import sys
import time
import warnings

import numpy as np

MAX_VALUES, MAX_RADIUS = 16, 8


# ---- the rules ----------------------------------------------------------------------------------------------------------------------
def ball(r):
    """bool [2r+1]^3: offset d is in the ball iff 4 (d . d) <= (2r + 1)^2 -- ITK's non-parametric ball, an ellipsoid with axes 2r + 1
    centred on the middle voxel: what BinaryDilateImageFilter.SetKernelRadius(r) builds with the default kernel type
    (image_fit_label.py:17-19, binarize.py:64-67; stated from knowledge of ITK, SimpleITK is not available: DESIGN.md section 6i)."""
    r = int(r)
    if r < 0:
        raise ValueError("ball: radius %d" % r)
    d = np.arange(-r, r + 1, dtype=np.int64)
    return 4 * (d[:, None, None] ** 2 + d[None, :, None] ** 2 + d[None, None, :] ** 2) <= (2 * r + 1) ** 2


def select(label, values):
    """uint8 0/1 map of `label in values`: the threshold-and-add loop of the reference (image_fit_label.py:62-66, binarize.py:38-43).
    The values are distinct -- a repeated one would make the reference's sum 2 -- and at most 16."""
    label = np.asarray(label)
    values = [int(v) for v in values]
    if len(set(values)) != len(values):
        raise ValueError("select: values %r are not distinct" % (values,))
    if len(values) > MAX_VALUES:
        raise ValueError("select: at most %d values, got %d" % (MAX_VALUES, len(values)))
    out = np.zeros(label.shape, dtype=np.uint8)
    for v in values:
        out += (label == v).astype(np.uint8)
    return out


def dilate(mask, r):
    """The OR of the mask shifted by every offset of ball(r), zero outside the volume; 1 <= r <= 8.  uint8 0/1 like its input."""
    mask = np.asarray(mask)
    r = int(r)
    if mask.ndim != 3 or not 1 <= r <= MAX_RADIUS:
        raise ValueError("dilate: takes a 3-D mask and a radius of 1 .. %d; got %s, r = %d" % (MAX_RADIUS, mask.shape, r))
    A, B, C = mask.shape
    padded = np.zeros((A + 2 * r, B + 2 * r, C + 2 * r), dtype=bool)
    padded[r:r + A, r:r + B, r:r + C] = mask != 0
    out = np.zeros(mask.shape, dtype=bool)
    for da, db, dc in np.argwhere(ball(r)) - r:
        out |= padded[r - da:r - da + A, r - db:r - db + B, r - dc:r - dc + C]
    return out.astype(np.uint8)


def bounding_box(mask):
    """(lo[3], hi[3]) inclusive of the non-zero voxels, or None for an empty mask (LabelShapeStatisticsImageFilter.GetBoundingBox(1)
    gives lo and hi - lo + 1: image_fit_label.py:72-74)."""
    where = np.argwhere(np.asarray(mask) != 0)
    if where.shape[0] == 0:
        return None
    return tuple(int(v) for v in where.min(0)), tuple(int(v) for v in where.max(0))


def fit_window(lo, hi, shape, buffer=2, dims=(0, 1, 2)):
    """(start[3], size[3]) of the crop, by the reference's arithmetic kept as written (image_fit_label.py:75-113).  On an axis in
    `dims`: start = max(lo - buffer, 0); end = lo + (hi - lo + 1) + buffer, replaced by n - 1 where it is >= n.  On any other axis:
    start = 0, end = n - 1.  size = end - start -- one voxel short wherever end was set to n - 1: the reference's behaviour, kept."""
    start, size = [], []
    for axis in range(3):
        n = int(shape[axis])
        if axis in dims:
            s = max(int(lo[axis]) - int(buffer), 0)
            e = int(lo[axis]) + (int(hi[axis]) - int(lo[axis]) + 1) + int(buffer)
            if e >= n:
                e = n - 1
        else:
            s, e = 0, n - 1
        start.append(s)
        size.append(e - s)
    return tuple(start), tuple(size)


def _window(arr, start, size):
    if min(size) < 1:
        raise ValueError("the crop window start %r size %r is empty (RegionOfInterestImageFilter refuses it)" % (start, size))
    return arr[tuple(slice(s, s + n) for s, n in zip(start, size))]


def fit_label(image, label, select_values, buffer=2, mask_image=True, dilation=2, dims=(0, 1, 2)):
    """(image_cropped, label_cropped) of image_fit_label.py.  The mask is dilate(select(label), dilation) (dilation 0: the selection
    itself); the image is zeroed where the mask is 0 and keeps its dtype; the box comes from the UNDILATED selection; the masked image
    and the ORIGINAL label are cropped to fit_window().  ValueError when the selection is empty (the reference raises there too)."""
    image, label = np.asarray(image), np.asarray(label)
    sel = select(label, select_values)
    box = bounding_box(sel)
    if box is None:
        raise ValueError("fit_label: no voxel of the label is one of %r" % (list(select_values),))
    if mask_image:
        mask = dilate(sel, dilation) if dilation > 0 else sel
        image = np.where(mask != 0, image, np.zeros((), dtype=image.dtype))
    start, size = fit_window(box[0], box[1], label.shape, buffer, dims)
    return _window(image, start, size), _window(label, start, size)


def binarize(image, label, select_values, mask_labels=(), dilation=5):
    """(label_out uint8, image_masked or None) of binarize.py:38-75: label_out = select(label, select_values); with mask_labels the
    image is zeroed outside dilate(select(label, mask_labels), dilation) (dilation 0 skips the dilation), without them it is None."""
    label = np.asarray(label)
    label_out = select(label, select_values)
    if len(mask_labels) == 0:
        return label_out, None
    image = np.asarray(image)
    mask = select(label, mask_labels)
    if dilation > 0:
        mask = dilate(mask, dilation)
    return label_out, np.where(mask != 0, image, np.zeros((), dtype=image.dtype))


def partition(nz, layer):
    """[(k_start, size)] of image_partition.py:31-36: slabs of `layer` slices along z, the last one takes what is left."""
    nz, layer = int(nz), int(layer)
    if nz < 1 or layer < 1:
        raise ValueError("partition: %d slices in layers of %d" % (nz, layer))
    return [(k, layer if k + layer < nz else nz - k) for k in range(0, nz, layer)]


def pack_bits(mask):
    """The packed layout of morph.py as a rule: 0/1 array [A,B,C] -> int64 [A,B,ceil(C/64)], bit k of word w is voxel c = 64 w + k."""
    mask = np.asarray(mask) != 0
    A, B, C = mask.shape
    W = (C + 63) // 64
    padded = np.zeros((A, B, W * 64), dtype=np.uint8)
    padded[:, :, :C] = mask
    return np.packbits(padded, axis=2, bitorder="little").view("<u8").reshape(A, B, W).view(np.int64)


def unpack_bits(bits, C):
    """int64 [A,B,W] -> uint8 0/1 [A,B,C] (the inverse of pack_bits)."""
    bits = np.ascontiguousarray(bits, dtype=np.int64)
    A, B, W = bits.shape
    return np.unpackbits(bits.view(np.uint8).reshape(A, B, W * 8), axis=2, bitorder="little")[:, :, :C].copy()


# ---- the tools ----------------------------------------------------------------------------------------------------------------------
def _find(path):
    """The file to read for a name: the name itself, or -- for a `.nii.gz` name this project wrote uncompressed -- the `.nii`."""
    if not os.path.exists(path) and path.endswith(".gz") and os.path.exists(path[:-3]):
        return path[:-3]
    return path


def _out_path(path):
    return path[:-3] if path.endswith(".gz") else path


def _upload(arr, device):
    """A NIfTI array [X,Y,Z] as data.read_nifti returns it -> the device tensor [Z,Y,X] of the file's own memory order and dtype:
    arr.T is C-contiguous, so no host transpose or cast pass happens.  One copy to the device."""
    import torch
    view = arr.T
    if not view.flags["C_CONTIGUOUS"]:
        view = np.ascontiguousarray(view)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)          # (the file's buffer is read-only; it is only read)
        return torch.from_numpy(view).to(device)


def _download(t):
    """Device tensor [Z,Y,X] -> NumPy [X,Y,Z] in the file's memory order (a view; data.write_nifti writes it without a transpose)."""
    return t.cpu().numpy().T


def _cases(src_dir, names):
    """The case directories of SRC that hold every named file, sorted."""
    out = []
    for case in sorted(os.listdir(src_dir)):
        if os.path.isdir(os.path.join(src_dir, case)) and all(os.path.exists(_find(os.path.join(src_dir, case, n))) for n in names):
            out.append(case)
    return out


class _Tool(object):
    def __init__(self, src_dir, tgt_dir, device, verbose):
        self.src_dir, self.tgt_dir, self.device, self.verbose = src_dir, tgt_dir, device, verbose
        self.times = {}

    def _device(self):
        import torch
        return torch.device(self.device if self.device is not None else "cuda")

    def _read(self, case, name):
        from . import data
        t0 = time.perf_counter()
        arr, hdr = data.read_nifti(_find(os.path.join(self.src_dir, case, name)))
        self._clock("read", t0)
        if arr.ndim != 3:
            raise ValueError("%s/%s: %s is not a 3-D volume" % (case, name, arr.shape))
        return arr, tuple(float(v) for v in hdr["pixdim"])

    def _write(self, case, name, arr, spacing):
        from . import data
        t0 = time.perf_counter()
        os.makedirs(os.path.join(self.tgt_dir, case), exist_ok=True)
        data.write_nifti(_out_path(os.path.join(self.tgt_dir, case, name)), arr, spacing)
        self._clock("write", t0)

    def _clock(self, key, t0):
        self.times[key] = self.times.get(key, 0.0) + time.perf_counter() - t0

    def _up(self, arr, dev):
        t0 = time.perf_counter()
        t = _upload(arr, dev)              # (a copy from pageable memory returns when the data is on the device)
        self._clock("upload", t0)
        return t

    def _down(self, t):
        import torch
        if t.device.type == "cuda":
            torch.cuda.synchronize(t.device)          # the kernels in front of the copy are not the download's time
        t0 = time.perf_counter()
        arr = _download(t)
        self._clock("download", t0)
        return arr

    def _say(self, case, text):
        if self.verbose:
            print("%s: %s" % (case, text))

    def run(self):
        """[(case, "done" | "skipped: ...")] in case order.  self.times: seconds spent reading, uploading, downloading and writing, and
        the total (what is left of it is the device work and its seven-number read-back)."""
        self.times = {}
        t0 = time.perf_counter()
        report = [(case, self.run_case(case)) for case in _cases(self.src_dir, self.inputs())]
        self.times["total"] = time.perf_counter() - t0
        return report


class FitLabel(_Tool):
    """image_fit_label.py.  Parameter names follow the reference's constants; `device` is appended."""

    def __init__(self, src_dir, tgt_dir, select_label=(1, 2), src_img_name="image.nii", src_label_name="label.nii",
                 tgt_img_name="image_cropped.nii.gz", tgt_label_name="label_cropped.nii.gz", buffer=2, mask_image=True,
                 mask_dilation=2, mask_dim=(0, 1, 2), device=None, verbose=False):
        _Tool.__init__(self, src_dir, tgt_dir, device, verbose)
        self.select_label = [int(v) for v in select_label]
        self.src_img_name, self.src_label_name = src_img_name, src_label_name
        self.tgt_img_name, self.tgt_label_name = tgt_img_name, tgt_label_name
        self.buffer, self.mask_image, self.mask_dilation = int(buffer), bool(mask_image), int(mask_dilation)
        self.mask_dim = tuple(int(v) for v in mask_dim)
        if not 0 <= self.mask_dilation <= MAX_RADIUS or self.buffer < 0 or any(d not in (0, 1, 2) for d in self.mask_dim):
            raise ValueError("FitLabel: dilation %d (0 .. %d), buffer %d (>= 0), dims %r (of 0, 1, 2)" % (
                self.mask_dilation, MAX_RADIUS, self.buffer, self.mask_dim))

    def inputs(self):
        return (self.src_label_name, self.src_img_name)

    def run_case(self, case):
        from . import morph
        dev = self._device()
        label, _ = self._read(case, self.src_label_name)
        image, spacing = self._read(case, self.src_img_name)
        if image.shape != label.shape:
            raise ValueError("%s: image %s and label %s are not one grid" % (case, image.shape, label.shape))
        lab = self._up(label, dev)                                  # [Z,Y,X]: device axis 2 - k is the reference's axis k
        C = int(lab.shape[2])
        sel = morph.select_bits(lab, self.select_label)
        count, lo, hi = morph.bits_bbox(sel, C)
        if count == 0:
            self._say(case, "skipped: no voxel of %s is one of %r" % (self.src_label_name, self.select_label))
            return "skipped: empty selection"
        start, size = fit_window(lo[::-1], hi[::-1], label.shape, self.buffer, self.mask_dim)
        if min(size) < 1:
            self._say(case, "skipped: the crop window start %r size %r is empty" % (start, size))
            return "skipped: empty window"
        img = self._up(image, dev)
        mask = None
        if self.mask_image:
            mask = morph.dilate_bits(sel, C, self.mask_dilation) if self.mask_dilation > 0 else sel
        image_cropped = self._down(morph.masked_crop(img, mask, start[::-1], size[::-1]))
        label_cropped = self._down(morph.masked_crop(lab, None, start[::-1], size[::-1]))
        self._write(case, self.tgt_label_name, label_cropped, spacing)
        self._write(case, self.tgt_img_name, image_cropped, spacing)
        self._say(case, "%d selected voxels, window start %r size %r of %r" % (count, start, size, tuple(label.shape)))
        return "done"


class Binarize(_Tool):
    """binarize.py.  Parameter names follow the reference's constants; `device` is appended."""

    def __init__(self, src_dir, tgt_dir, select_label=(2,), mask_label=(), src_img_name="image_cropped.nii.gz",
                 src_label_name="label_cropped.nii.gz", masked_img_name="image_masked.nii.gz", tgt_label_name="label_masked.nii.gz",
                 mask_dilation=5, device=None, verbose=False):
        _Tool.__init__(self, src_dir, tgt_dir, device, verbose)
        self.select_label, self.mask_label = [int(v) for v in select_label], [int(v) for v in mask_label]
        self.src_img_name, self.src_label_name = src_img_name, src_label_name
        self.masked_img_name, self.tgt_label_name = masked_img_name, tgt_label_name
        self.mask_dilation = int(mask_dilation)
        if not 0 <= self.mask_dilation <= MAX_RADIUS:
            raise ValueError("Binarize: dilation %d (0 .. %d)" % (self.mask_dilation, MAX_RADIUS))

    def inputs(self):
        return (self.src_label_name, self.src_img_name) if self.mask_label else (self.src_label_name,)

    def run_case(self, case):
        from . import morph
        dev = self._device()
        label, spacing = self._read(case, self.src_label_name)
        lab = self._up(label, dev)
        C = int(lab.shape[2])
        sel = morph.select_bits(lab, self.select_label)
        count, _, _ = morph.bits_bbox(sel, C)
        if count == 0:
            self._say(case, "skipped: no voxel of %s is one of %r" % (self.src_label_name, self.select_label))
            return "skipped: empty selection"
        self._write(case, self.tgt_label_name, self._down(morph.unpack_bits(sel, C)), spacing)
        if self.mask_label:
            image, spacing = self._read(case, self.src_img_name)
            if image.shape != label.shape:
                raise ValueError("%s: image %s and label %s are not one grid" % (case, image.shape, label.shape))
            mask = morph.select_bits(lab, self.mask_label)
            if self.mask_dilation > 0:
                mask = morph.dilate_bits(mask, C, self.mask_dilation)
            img = self._up(image, dev)
            masked = self._down(morph.masked_crop(img, mask, (0, 0, 0), tuple(img.shape)))
            self._write(case, self.masked_img_name, masked, spacing)
        self._say(case, "%d selected voxels of %r" % (count, tuple(label.shape)))
        return "done"


class Partition(_Tool):
    """image_partition.py: host only, it slices and writes into TGT/case_kstart/."""

    def __init__(self, src_dir, tgt_dir, layer=64, src_img_name="image_cropped.nii", src_label_name="label_cropped.nii",
                 tgt_img_name="image.nii.gz", tgt_label_name="label.nii.gz", verbose=False):
        _Tool.__init__(self, src_dir, tgt_dir, None, verbose)
        self.layer = int(layer)
        self.src_img_name, self.src_label_name = src_img_name, src_label_name
        self.tgt_img_name, self.tgt_label_name = tgt_img_name, tgt_label_name
        if self.layer < 1:
            raise ValueError("Partition: layer %d" % self.layer)

    def inputs(self):
        return (self.src_label_name, self.src_img_name)

    def run_case(self, case):
        label, _ = self._read(case, self.src_label_name)
        image, spacing = self._read(case, self.src_img_name)
        if image.shape != label.shape:
            raise ValueError("%s: image %s and label %s are not one grid" % (case, image.shape, label.shape))
        slabs = partition(label.shape[2], self.layer)
        for k, n in slabs:
            self._write("%s_%d" % (case, k), self.tgt_label_name, label[:, :, k:k + n], spacing)
            self._write("%s_%d" % (case, k), self.tgt_img_name, image[:, :, k:k + n], spacing)
        self._say(case, "%d slabs of %d slices from %r" % (len(slabs), self.layer, tuple(label.shape)))
        return "done"


# ---- command line -------------------------------------------------------------------------------------------------------------------
def get_parser():
    p = argparse.ArgumentParser(prog="python -m vnet_tensorflow_amd.prepare_data",
                                description="Turn a raw download into the case directories train and evaluate read, on the device.")
    sub = p.add_subparsers(dest="tool", metavar="{fit-label,binarize,partition}")
    sub.required = True

    def common(q, image, label, out_image, out_label, gpu=True):
        q.add_argument("src", help="Source directory: one sub-directory per case", metavar="SRC")
        q.add_argument("tgt", help="Target directory", metavar="TGT")
        q.add_argument("--image", default=image, help="Image file of a case (default=%s)" % image, metavar="NAME")
        q.add_argument("--label", default=label, help="Label file of a case (default=%s)" % label, metavar="NAME")
        q.add_argument("--out-image", dest="out_image", default=out_image, help="Image file written (default=%s)" % out_image, metavar="NAME")
        q.add_argument("--out-label", dest="out_label", default=out_label, help="Label file written (default=%s)" % out_label, metavar="NAME")
        q.add_argument("-v", "--verbose", dest="verbose", action="store_true", help="One line per case")
        if gpu:
            q.add_argument("--gpu", dest="gpu", default=None, type=int, help="Device index (default: the current device)", metavar="N")

    f = sub.add_parser("fit-label", help="Mask the image by its dilated label selection and crop both to the selection's box")
    common(f, "image.nii", "label.nii", "image_cropped.nii.gz", "label_cropped.nii.gz")
    f.add_argument("--select", nargs="+", type=int, default=[1, 2], help="Label values selected (default=1 2)", metavar="V")
    f.add_argument("--buffer", type=int, default=2, help="Voxels kept around the box (default=2)", metavar="N")
    f.add_argument("--mask-dilation", dest="mask_dilation", type=int, default=2, help="Ball radius of the mask (default=2)", metavar="R")
    f.add_argument("--mask-dim", dest="mask_dim", nargs="*", type=int, default=[0, 1, 2], help="Axes cropped (default=0 1 2)", metavar="AXIS")
    f.add_argument("--no-mask", dest="no_mask", action="store_true", help="Crop only, keep the image outside the mask")

    b = sub.add_parser("binarize", help="Write the selection as a 0/1 label and the image masked by a dilated second selection")
    common(b, "image_cropped.nii.gz", "label_cropped.nii.gz", "image_masked.nii.gz", "label_masked.nii.gz")
    b.add_argument("--select", nargs="+", type=int, default=[2], help="Label values selected (default=2)", metavar="V")
    b.add_argument("--mask-label", dest="mask_label", nargs="*", type=int, default=[], help="Label values the image is masked by "
                   "(default: none, no image is written)", metavar="V")
    b.add_argument("--mask-dilation", dest="mask_dilation", type=int, default=5, help="Ball radius of the mask (default=5)", metavar="R")

    q = sub.add_parser("partition", help="Cut every case into slabs along z (host only)")
    common(q, "image_cropped.nii", "label_cropped.nii", "image.nii.gz", "label.nii.gz", gpu=False)
    q.add_argument("--layer", type=int, default=64, help="Slices per slab (default=64)", metavar="N")
    return p


def from_args(args):
    device = None if getattr(args, "gpu", None) is None else "cuda:%d" % args.gpu
    if args.tool == "fit-label":
        return FitLabel(args.src, args.tgt, select_label=args.select, src_img_name=args.image, src_label_name=args.label,
                        tgt_img_name=args.out_image, tgt_label_name=args.out_label, buffer=args.buffer, mask_image=not args.no_mask,
                        mask_dilation=args.mask_dilation, mask_dim=args.mask_dim, device=device, verbose=args.verbose)
    if args.tool == "binarize":
        return Binarize(args.src, args.tgt, select_label=args.select, mask_label=args.mask_label, src_img_name=args.image,
                        src_label_name=args.label, masked_img_name=args.out_image, tgt_label_name=args.out_label,
                        mask_dilation=args.mask_dilation, device=device, verbose=args.verbose)
    return Partition(args.src, args.tgt, layer=args.layer, src_img_name=args.image, src_label_name=args.label,
                     tgt_img_name=args.out_image, tgt_label_name=args.out_label, verbose=args.verbose)


def main(argv=None):
    args = get_parser().parse_args(argv)
    tool = from_args(args)
    report = tool.run()
    if args.verbose:
        print("%d cases, %d skipped, %.3fs" % (len(report), sum(1 for _, s in report if s != "done"), tool.times["total"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())

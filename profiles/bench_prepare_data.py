"""Run once on an MI355X: profiles/prepare_data_bench.txt (one run; device stages: medians of 5 repetitions after 2 warm-up calls,
HIP events; no spread is measured).

The data-preparation tools (csrc/vnet_tools.h) on a synthetic 512 x 512 x 256 case: int16 image, uint8 label of two
blobs (classes 1 and 2, the second inside the first).
    device stages : morph.select_bits, morph.dilate_bits (r = 2 and r = 5), morph.bits_bbox (with its read-back), morph.masked_crop
                    (the int16 image through the mask, the uint8 label plain) and morph.unpack_bits on resident tensors
    end to end    : FitLabel.run() (r = 2) and Binarize.run() (r = 5, masked by classes 1 and 2) from the files to the files, wall clock,
                    with the tools' own split: reading, upload, download, writing; the rest is the device work
    host          : scipy.ndimage.binary_dilation of the same selection with the same ball on one thread, wall clock, once each
No target is fixed for any of these figures.
Usage: python profiles/bench_prepare_data.py [outfile]   (default profiles/prepare_data_bench.txt)"""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE, SPACING = (512, 512, 256), (0.7, 0.7, 1.0)


def synthetic(size, seed=0):
    """[X,Y,Z] in the memory order of a NIfTI file (x fastest), as data.read_nifti returns it."""
    rng = np.random.default_rng(seed)
    x, y, z = np.meshgrid(*(np.linspace(-1, 1, n, dtype=np.float32) for n in size), indexing="ij", sparse=True)
    image = np.asfortranarray((600 * np.sin(5 * x) * np.cos(4 * y) + 300 * z + rng.normal(0, 40, size)).astype(np.int16))
    label = np.zeros(size, dtype=np.uint8, order="F")
    label[(x + 0.1) ** 2 + (y - 0.05) ** 2 + (z * 0.8) ** 2 < 0.45 ** 2] = 1
    label[(x - 0.05) ** 2 + (y + 0.1) ** 2 + (z - 0.1) ** 2 < 0.12 ** 2] = 2
    return image, label


def main(out_path):
    import torch
    from scipy import ndimage
    from vnet_tensorflow_amd import data, morph, prepare_data as P
    dev = torch.device("cuda", 0)
    lines = ["data-preparation tools, synthetic %dx%dx%d int16 image, uint8 label; device %s" % (SIZE + (torch.cuda.get_device_name(0),))]

    def events(fn, warm=2, reps=5):
        for _ in range(warm):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(reps):
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    image, label = synthetic(SIZE)
    lab, img = P._upload(label, dev), P._upload(image, dev)
    C = int(lab.shape[2])
    nvox = lab.numel()
    lines.append("select_bits [1, 2]    %9.3f ms  (reads %d MB of label)" % (events(lambda: morph.select_bits(lab, [1, 2])), nvox >> 20))
    sel = morph.select_bits(lab, [1, 2])
    count, lo, hi = morph.bits_bbox(sel, C)
    lines.append("selection: %d voxels, box %s .. %s of [Z,Y,X] = %s; packed mask %d KB" % (count, lo, hi, tuple(lab.shape), sel.numel() * 8 >> 10))
    for r in (2, 5):
        lines.append("dilate_bits r = %d      %9.3f ms" % (r, events(lambda: morph.dilate_bits(sel, C, r))))
    lines.append("bits_bbox             %9.3f ms  (with its read-back)" % events(lambda: morph.bits_bbox(sel, C)))
    mask = morph.dilate_bits(sel, C, 2)
    start, size = P.fit_window(lo[::-1], hi[::-1], label.shape, 2, (0, 1, 2))
    start, size = start[::-1], size[::-1]
    out_mb = size[0] * size[1] * size[2] / 2.0 ** 20
    lines.append("masked_crop int16     %9.3f ms  (window %s, %.0f M voxels, through the mask)" % (
        events(lambda: morph.masked_crop(img, mask, start, size)), size, out_mb))
    lines.append("masked_crop uint8     %9.3f ms  (the label, no mask)" % events(lambda: morph.masked_crop(lab, None, start, size)))
    lines.append("masked_crop int16 all %9.3f ms  (the whole volume through the mask, as binarize does)" % events(
        lambda: morph.masked_crop(img, mask, (0, 0, 0), tuple(img.shape))))
    lines.append("unpack_bits           %9.3f ms" % events(lambda: morph.unpack_bits(sel, C)))

    # the rule on the device's result, once, at full size: the r = 2 mask against scipy with the same ball
    sel_host = P.unpack_bits(sel.cpu().numpy(), C)
    for r in (2, 5):
        t0 = time.perf_counter()
        want = ndimage.binary_dilation(sel_host, structure=P.ball(r), border_value=0)
        t1 = time.perf_counter()
        got = P.unpack_bits(morph.dilate_bits(sel, C, r).cpu().numpy(), C)
        lines.append("scipy.ndimage.binary_dilation, ball(%d), one thread %8.3f s; the device's mask equals it: %s" % (
            r, t1 - t0, bool(np.array_equal(got, want))))
    del sel_host, want, got

    with tempfile.TemporaryDirectory() as d:
        src, fit, binz = (os.path.join(d, n) for n in ("src", "fit", "bin"))
        os.makedirs(os.path.join(src, "case"))
        data.write_nifti(os.path.join(src, "case", "image.nii"), image, SPACING)
        data.write_nifti(os.path.join(src, "case", "label.nii"), label, SPACING)
        for name, tool in (("fit-label r = 2", P.FitLabel(src, fit, device=dev)),
                           ("binarize r = 5 ", P.Binarize(fit, binz, select_label=(2,), mask_label=(1, 2), mask_dilation=5, device=dev))):
            report = tool.run()
            t = tool.times
            rest = t["total"] - sum(t.get(k, 0.0) for k in ("read", "upload", "download", "write"))
            lines.append("%s end to end %7.3f s: read %.3f, upload %.3f, download %.3f, write %.3f, device and the rest %.3f  %s" % (
                name, t["total"], t.get("read", 0.0), t.get("upload", 0.0), t.get("download", 0.0), t.get("write", 0.0), rest, report))
    text = "\n".join(lines) + "\n"
    with open(out_path, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "prepare_data_bench.txt"))

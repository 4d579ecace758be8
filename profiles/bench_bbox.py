"""Run once on an MI355X: profiles/bbox_bench.txt (one run; device stages: medians of 5 repetitions after 2 warm-up calls; no spread
is measured).

The bounding-box tool (csrc/vnet_bbox.h) on a synthetic 512 x 512 x 128 case with spacing (0.7, 0.9, 2.5), axial:
a smooth image, three blob classes plus speckle.
    device stages : ops.resample (linear, nearest), ops.slice_stack (float32, int32), ops.plane_component_table (with its read-back) and
                    ops.bbox_render on resident tensors, HIP events
    end to end    : BoundingBox.run() from the two files to the PNGs, wall clock, with its own split: upload, device, suppression on the
                    host, pinned download, PNG compression and writing on the thread pool
    host          : the restatement of the labelling, scipy.ndimage.label + find_objects per slice and class on one thread, wall clock
No target is fixed for any of these figures; PNG compression on the host is expected to dominate end to end.
Usage: python profiles/bench_bbox.py [outfile]   (default profiles/bbox_bench.txt)"""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE, SPACING = (512, 512, 128), (0.7, 0.9, 2.5)


def synthetic(size, seed=0):
    rng = np.random.default_rng(seed)
    x, y, z = np.meshgrid(*(np.linspace(-1, 1, n, dtype=np.float32) for n in size), indexing="ij", sparse=True)
    image = (600 * np.sin(5 * x) * np.cos(4 * y) + 300 * z + rng.normal(0, 40, size)).astype(np.float32)
    label = np.zeros(size, dtype=np.int16)
    for cls, (cx, cy, cz, r) in enumerate(((-0.3, -0.2, 0.0, 0.35), (0.4, 0.3, 0.1, 0.3), (0.1, -0.5, -0.3, 0.2)), start=1):
        label[(x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 < r * r] = cls
    label[rng.random(size) < 0.0002] = 2                           # speckle: many one-voxel components
    return image, label


def main(out_path):
    import torch
    from scipy import ndimage
    from vnet_tensorflow_amd import bounding_box as B, data, ops, resample as R
    dev = torch.device("cuda", 0)
    lines = ["bounding-box tool, synthetic %dx%dx%d, spacing %s, axial; device %s" % (SIZE + (SPACING, torch.cuda.get_device_name(0)))]

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
    size, spacing = B.geometry(SIZE, SPACING, 2)
    ratio = R.ratios(SPACING, spacing)
    x = torch.from_numpy(image).to(dev)
    l = torch.from_numpy(label.astype(np.int32)).to(dev)
    lines.append("resampled grid %s, spacing %s" % (size, spacing))
    lines.append("resample linear      %9.3f ms" % events(lambda: ops.resample(x, size, ratio, "linear")))
    lines.append("resample nearest     %9.3f ms" % events(lambda: ops.resample(l, size, ratio, "nearest")))
    xr, lr = ops.resample(x, size, ratio, "linear"), ops.resample(l, size, ratio, "nearest")
    lines.append("slice_stack float32  %9.3f ms" % events(lambda: ops.slice_stack(xr, 2)))
    lines.append("slice_stack int32    %9.3f ms" % events(lambda: ops.slice_stack(lr, 2)))
    xs, ls = ops.slice_stack(xr, 2), ops.slice_stack(lr, 2)
    lines.append("plane_component_table%9.3f ms (launches, class gather and read-back)" % events(lambda: ops.plane_component_table(ls)))
    n, rows, classes = ops.plane_component_table(ls)
    t0 = time.perf_counter()
    boxes = B.boxes_of_rows(ls.shape[0], rows, classes)
    lines.append("components %d, boxes after suppression %d, suppression on the host %.3f s" % (
        n, sum(len(v) for v in boxes.values()), time.perf_counter() - t0))
    flat, first = B.box_arrays(boxes, ls.shape[0])
    fb, ff = torch.from_numpy(flat).to(dev), torch.from_numpy(first).to(dev)
    lines.append("bbox_render          %9.3f ms" % events(lambda: ops.bbox_render(xs, ls, fb, ff, -1024, 1024, 0.37)))

    with tempfile.TemporaryDirectory() as d:
        paths = os.path.join(d, "image.nii"), os.path.join(d, "label.nii")
        data.write_nifti(paths[0], image, SPACING)
        data.write_nifti(paths[1], label, SPACING)
        tool = B.BoundingBox(paths[0], paths[1], os.path.join(d, "out"), opacity=0.37, device=dev)
        t0 = time.perf_counter()
        tool.run()
        total = time.perf_counter() - t0
        lines.append("end to end, file to %d PNGs: %.3f s  (%s; the rest is file reading)" % (
            ls.shape[0], total, ", ".join("%s %.3f s" % kv for kv in sorted(tool.times.items()))))

    host = ls.cpu().numpy()
    t0 = time.perf_counter()
    found = 0
    for s in range(host.shape[0]):
        for value in np.unique(host[s]):
            if value > 0:
                lab, k = ndimage.label(host[s] == value)
                found += len(ndimage.find_objects(lab))
    lines.append("host labelling (scipy.ndimage.label + find_objects per slice and class, one thread): %.3f s, %d components" % (
        time.perf_counter() - t0, found))
    assert found == n
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bbox_bench.txt"))

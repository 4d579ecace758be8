"""Run once on an MI355X: profiles/surface_bench.txt (one run; device stages: medians of 5 repetitions after 2 warm-up calls, HIP
events; no spread is measured).

The surface-distance scores (csrc/vnet_surface.h) on a synthetic 512 x 512 x 256 case: the ground truth is an
ellipsoid with a small satellite, the output the same ellipsoid moved by (3, -2, 1) voxels with a dent and a far false positive.
    device stages : surface.surface_bits, surface.edt2 (its three passes in one figure; again on a mask of ONE set voxel, where every
                    voxel walks as far as its distance on two axes), surface.gather, surface.kth (2 ranks), surface.root_sum on
                    resident tensors
    per kernel    : `rocprofv3 --kernel-trace --stats -- python profiles/bench_surface.py --kernels` in a run of its own (every op three
                    times, nothing timed by the script); its table is appended to the file by hand
    end to end    : score.surface_distances(gt, out, spacing) on device tensors, with and without the ground truth's cached half, wall
                    clock with a synchronize
    host          : scipy.ndimage.binary_erosion + distance_transform_edt of both maps on one thread, wall clock, once; the device's
                    surfaces, fields (sqrt, at unit spacing: ==) and HD are asserted equal to them
No target is fixed for any of these figures.
Usage: python profiles/bench_surface.py [outfile | --kernels]   (default profiles/surface_bench.txt)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE, SPACING = (512, 512, 256), (1.0, 1.0, 1.0)


def synthetic(size):
    x, y, z = np.meshgrid(*(np.linspace(-1, 1, n, dtype=np.float32) for n in size), indexing="ij", sparse=True)
    gt = np.zeros(size, dtype=np.int32)
    gt[(x + 0.1) ** 2 + (y - 0.05) ** 2 + (z * 0.8) ** 2 < 0.45 ** 2] = 1
    gt[(x - 0.7) ** 2 + (y + 0.6) ** 2 + (z - 0.1) ** 2 < 0.05 ** 2] = 1
    out = np.roll(np.roll(np.roll(gt, 3, axis=0), -2, axis=1), 1, axis=2)
    out[(x - 0.3) ** 2 + (y - 0.1) ** 2 + z ** 2 < 0.1 ** 2] = 0               # a dent
    out[(x - 0.7) ** 2 + (y + 0.6) ** 2 + (z - 0.1) ** 2 < 0.08 ** 2] = 0       # the satellite is missed
    out[(x + 0.8) ** 2 + (y + 0.8) ** 2 + (z + 0.5) ** 2 < 0.04 ** 2] = 1       # a far false positive
    return gt, out


def main(out_path):
    import torch
    from scipy import ndimage
    from vnet_tensorflow_amd import score as SC, surface
    dev = torch.device("cuda", 0)
    lines = ["surface distances, synthetic %dx%dx%d int32 label maps, spacing %s; device %s" % (SIZE + (SPACING, torch.cuda.get_device_name(0)))]

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

    def wall(fn, reps=3):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), r

    gt, out = synthetic(SIZE)
    tg, to = torch.from_numpy(gt).to(dev), torch.from_numpy(out).to(dev)
    Z, nvox = SIZE[2], gt.size
    if out_path == "--kernels":                  # under the profiler: every kernel of the unit three times at full size
        for _ in range(3):
            SC.surface_distances(tg, to, SPACING)
        torch.cuda.synchronize()
        return
    lines.append("surface_bits          %9.3f ms  (reads %d MB of label, five neighbours through the caches)" % (
        events(lambda: surface.surface_bits(tg)), nvox * 4 >> 20))
    sg, so = surface.surface_bits(tg), surface.surface_bits(to)
    n1, n2 = surface.popcounts([sg, so], Z)
    lines.append("surface voxels: %d of the ground truth, %d of the output; packed mask %d KB" % (n1, n2, sg.numel() * 8 >> 10))
    t_edt = events(lambda: surface.edt2(sg, Z, SPACING))
    lines.append("edt2 (z, y, x passes) %9.3f ms  (%.1f ns per voxel; writes %d MB of fp64, %d MB of scratch)" % (
        t_edt, t_edt * 1e6 / nvox, nvox * 8 >> 20, nvox * 12 >> 20))
    one = torch.zeros_like(sg)
    one[SIZE[0] // 2, SIZE[1] // 2, 0] = 1
    lines.append("edt2, one set voxel   %9.3f ms  (the long walks: a voxel at distance r walks about r indices each way, on two axes)" % events(
        lambda: surface.edt2(one, Z, SPACING), warm=1, reps=3))
    fg, fo = surface.edt2(sg, Z, SPACING), surface.edt2(so, Z, SPACING)
    lines.append("gather                %9.3f ms  (%d values into a list of %d)" % (events(lambda: surface.gather(fo, sg, Z)), n1, n1))
    both = surface.empty_list(n1 + n2, dev)
    surface.gather(fo, sg, Z, out=both, offset=0)
    surface.gather(fg, so, Z, out=both, offset=n1)
    ranks = [n1 + n2 - 1, SC.hd95_rank(n1 + n2)]
    lines.append("kth, 2 ranks          %9.3f ms  (63 counting passes over %d numbers, 127 launches)" % (events(lambda: surface.kth(both, ranks)), n1 + n2))
    lines.append("root_sum              %9.3f ms" % events(lambda: surface.root_sum(both)))
    t_all, res = wall(lambda: SC.surface_distances(tg, to, SPACING))
    lines.append("surface_distances end to end      %8.4f s  %s" % (t_all, {k: res[k] for k in ("HD", "HD95", "ASSD")}))
    field = SC.surface_field(tg, SPACING)
    t_half, res2 = wall(lambda: SC.surface_distances(tg, to, SPACING, gt_field=field))
    lines.append("  with the ground truth's half cached %8.4f s  (as Batch_Evaluate calls it; equal scores: %s)" % (t_half, res2 == res))

    # the host's way, one thread, once: erosion for the surfaces, scipy's exact transform for the fields
    t0 = time.perf_counter()
    cross = ndimage.generate_binary_structure(3, 1)
    hs = [m & ~ndimage.binary_erosion(m, cross, border_value=0) for m in (gt != 0, out != 0)]
    t1 = time.perf_counter()
    hf = [ndimage.distance_transform_edt(~s, sampling=SPACING) for s in hs]
    t2 = time.perf_counter()
    hd = max(hf[1][hs[0]].max(), hf[0][hs[1]].max())
    t3 = time.perf_counter()
    lines.append("scipy, one thread: binary_erosion x 2 %8.3f s, distance_transform_edt x 2 %8.3f s, reading HD off them %8.3f s" % (
        t1 - t0, t2 - t1, t3 - t2))
    same_s = all(np.array_equal(d.cpu().numpy(), SC.pack(h)) for d, h in ((sg, hs[0]), (so, hs[1])))
    same_f = all(np.array_equal(np.sqrt(d.cpu().numpy()), h) for d, h in ((fg, hf[0]), (fo, hf[1])))
    lines.append("the device's surfaces equal scipy's: %s; sqrt of its fields equals scipy's transform bit for bit: %s; HD equal: %s" % (
        same_s, same_f, bool(hd == res["HD"])))
    assert same_s and same_f and hd == res["HD"] and res2 == res
    lines.append("host / device, per scored case with the cached half: %.0f x" % ((t2 - t0) / 2 / t_half))
    text = "\n".join(lines) + "\n"
    with open(out_path, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "surface_bench.txt"))

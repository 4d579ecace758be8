"""Run once on an MI355X: profiles/postprocess_bench.txt (one run; device stages: medians of 5 repetitions after 2 warm-up calls, HIP
events; no spread is measured).

The post-processing pipeline of evaluate (csrc/vnet_post.h) on a synthetic 512 x 512 x 256 label of 5 classes: four
ellipsoidal organs, one with a tumour of another class inside and two background cavities, one with a pinhole channel, plus a spray of
one-voxel components of every class.
    device stages : every entry point on resident tensors -- postprocess.class_roots_device (all four classes in one labelling),
                    filter_components (keep largest, remove small), fill_holes_class, not_bits, apply_bits -- and the morphology
                    steps composed of them and morph.select_bits / dilate_bits
    the yardstick : what the library could do before: K - 1 calls of ops.component_roots(label == c, sizes=True), with and without
                    forming the masks
    pipeline      : KeepLargestComponent, RemoveSmallComponents, FillHoles, Close(2) through postprocess.run on the device tensor, wall
                    clock with a synchronize
    host          : (second argument `host`) the same pipeline through the NumPy / scipy restatements on one thread, wall clock, once,
                    step by step; the device's result is asserted equal to it
No target is fixed for any of these figures.
Usage: python profiles/bench_postprocess.py [outfile [host]]   (default profiles/postprocess_bench.txt, device stages only)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE, SPACING, K = (512, 512, 256), (0.8, 0.8, 1.5), 5


def synthetic(size):
    x, y, z = np.meshgrid(*(np.linspace(-1, 1, n, dtype=np.float32) for n in size), indexing="ij", sparse=True)

    def ball(cx, cy, cz, r, sx=1.0, sy=1.0, sz=1.0):
        return ((x - cx) / sx) ** 2 + ((y - cy) / sy) ** 2 + ((z - cz) / sz) ** 2 < r ** 2
    lab = np.zeros(size, dtype=np.int32)
    lab[ball(-0.3, 0.1, 0.0, 0.45, 1.0, 1.2, 1.5)] = 1                       # a liver
    lab[ball(-0.35, 0.2, 0.1, 0.08)] = 4                                      # its tumour: stays under FillHoles
    lab[ball(-0.1, -0.1, -0.2, 0.05)] = 0                                     # two cavities
    lab[ball(-0.5, 0.3, 0.3, 0.03)] = 0
    lab[ball(0.5, 0.4, 0.1, 0.2, 1.0, 0.7, 1.4)] = 2
    lab[ball(0.5, 0.4, 0.1, 0.04)] = 0                                        # a cavity with a one-voxel channel to the outside
    cx, cy, cz = (int(round((c + 1) / 2 * (n - 1))) for c, n in zip((0.5, 0.4, 0.1), size))
    lab[cx:, cy, cz] = np.where(lab[cx:, cy, cz] == 2, 0, lab[cx:, cy, cz])
    lab[ball(0.55, -0.5, -0.3, 0.18)] = 3
    lab[ball(0.1, -0.6, 0.5, 0.1)] = 3                                        # a second component of class 3
    rng = np.random.default_rng(0)
    spray = rng.random(size, dtype=np.float32) < 0.002
    lab[spray] = rng.integers(1, K, size=int(spray.sum()), dtype=np.int32)
    return lab


def main(out_path, host=False):
    import torch
    from vnet_tensorflow_amd import morph, ops, postprocess as PP
    dev = torch.device("cuda", 0)
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")

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

    say("post-processing, synthetic %dx%dx%d int32 label of %d classes, spacing %s; device %s" % (SIZE + (K, SPACING, torch.cuda.get_device_name(0))))
    lab = synthetic(SIZE)
    t = torch.from_numpy(lab).to(dev)
    Z, nvox, classes = SIZE[2], lab.size, list(range(1, K))
    say("voxels per class: %s" % np.bincount(lab.ravel(), minlength=K).tolist())
    vv = PP.voxel_volume(SPACING)
    volume = 50.0 * vv

    t_one = events(lambda: PP.class_roots_device(t, classes, sizes=True))
    say("class_roots, 4 classes in one pass     %9.3f ms  (%.2f ns per voxel)" % (t_one, t_one * 1e6 / nvox))
    masks = [(t == c).to(torch.int32) for c in classes]
    t_k = events(lambda: [ops.component_roots(m, sizes=True) for m in masks])
    t_km = events(lambda: [ops.component_roots((t == c), sizes=True) for c in classes])
    say("component_roots x %d on ready masks     %9.3f ms;  forming label == c as well %9.3f ms" % (K - 1, t_k, t_km))
    say("  one pass against the %d passes: %.2f x (ready masks), %.2f x (with the masks)" % (K - 1, t_k / t_one, t_km / t_one))
    roots, sizes = PP.class_roots_device(t, classes, sizes=True)
    for c, m in zip(classes, masks):
        r, s = ops.component_roots(m, sizes=True)
        sel = t == c
        assert torch.equal(roots[sel], r[sel]) and torch.equal(sizes[sel], s[sel]) and bool((r[~sel] == -1).all())
    say("  equal representatives and counts, class by class: True; components per class: %s" % [
        int(((sizes > 0) & (t == c)).sum()) for c in classes])
    say("filter_components, keep largest        %9.3f ms" % events(lambda: PP.filter_components(t, classes, 0)))
    say("filter_components, remove small        %9.3f ms" % events(lambda: PP.filter_components(t, classes, 1, volume, vv)))
    say("fill_holes_class, one class            %9.3f ms" % events(lambda: PP.fill_holes_class(t, 1)))
    bits = morph.select_bits(t, [1])
    say("select_bits %9.3f ms, dilate_bits r = 2 %9.3f ms, not_bits %9.3f ms, apply_bits %9.3f ms" % (
        events(lambda: morph.select_bits(t, [1])), events(lambda: morph.dilate_bits(bits, Z, 2)), events(lambda: PP.not_bits(bits, Z)),
        events(lambda: PP.apply_bits(t, bits, 1))))
    for step in (PP.Dilate(2, [1]), PP.Erode(2, [1]), PP.Open(2, [1]), PP.Close(2, [1])):
        say("%-38s %9.3f ms" % ("step %r" % step, events(lambda: PP.run([step], t, SPACING))))

    steps = [PP.KeepLargestComponent(), PP.RemoveSmallComponents(volume), PP.FillHoles(), PP.Close(2)]
    for _ in range(2):
        got = PP.run(steps, t, SPACING, classes=K)
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = PP.run(steps, t, SPACING, classes=K)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    t_dev = float(np.median(ts))
    got_np = got.cpu().numpy()
    say("pipeline %s on the device: %.4f s; %d voxels changed, voxels per class after: %s" % (
        steps, t_dev, int((got_np != lab).sum()), np.bincount(got_np.ravel(), minlength=K).tolist()))
    if not host:
        return
    # the restatements, one thread, once, step by step
    run, total = lab, 0.0
    for s in steps:
        t0 = time.perf_counter()
        run = PP.run([s], run, SPACING, classes=K)
        dt = time.perf_counter() - t0
        total += dt
        say("  restatement of %-40r %8.2f s" % (s, dt))
    same = bool(np.array_equal(run, got_np))
    say("restatements (NumPy / scipy, one thread): %.1f s; the device's label equals theirs: %s; host / device: %.0f x" % (total, same, total / t_dev))
    assert same


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "postprocess_bench.txt"), host=len(sys.argv) > 2 and sys.argv[2] == "host")

"""A training sample through BSplineDeformation, per sample, on prepared cases of 256^3 x 1 (patch 128^3) and 128^3 x 4 (patch 64^3) plus
label -- the pipeline [BSplineDeformation(10), ConfidenceCrop2(patch, probability 0.8), RandomNoise] on one blob plus 40 islands:
    kernels  : on the device alone (HIP events after warm-up), the fused kernel (vnet_deform_sample_patch, sigma 5) against the composition
               it replaces, vnet_bspline_deform_f32 of the whole image plus vnet_sample_patch; and the per-visit label work, the label's
               deformation and its component table;
    resident : (a) data.VolumeDataset(device_tail=...) end to end, one loader thread, wall clock per sample after the first pass (which
               uploads the cases): coefficient upload, label deformation, table, draws, fused kernel;
    loader   : (b) the parent's device path for the same pipeline, BSplineDeformation(device=...) on the loader thread (the volume up and
               down per visit), then the NumPy ConfidenceCrop2 and RandomNoise;
    numpy    : (b) the NumPy backend throughout.
Recorded: every value, whether (a) beats both paths of (b), whether (a) stays under the headline training step quoted in README.md, and
whether the fused kernel beats the composition at both sizes.
Every step is a child process under its own time limit; a step that fails or runs out of time ends the run.
Usage: python profiles/bench_deform_sample.py [outfile]   (default profiles/deform_sample_bench.txt)"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = {"256^3x1": ((256, 256, 256), 1, (128, 128, 128)), "128^3x4": ((128, 128, 128), 4, (64, 64, 64))}
SPACING = (1.0, 1.0, 1.0)
CASES = 2
HEADLINE_MS = 14.6           # the headline training step quoted in README.md
LIMIT = {"kernels": 180, "resident": 240, "loader": 300, "numpy": 560}
SAMPLES = {"resident": 24, "loader": 6, "numpy": 2}


def _case(name, seed):
    shape, C, _ = SIZES[name]
    rng = np.random.default_rng(seed)
    image = rng.normal(100.0, 40.0, size=shape + (C,)).astype(np.float32)
    g = np.ogrid[tuple(slice(0, s) for s in shape)]
    label = (sum((a - s * 0.55) ** 2 for a, s in zip(g, shape)) <= (shape[0] / 5.0) ** 2).astype(np.int32)
    for _ in range(40):
        p = [int(rng.integers(0, s - 4)) for s in shape]
        label[p[0]:p[0] + 3, p[1]:p[1] + 3, p[2]:p[2] + 3] = 1
    return image, label


def _dataset(name, device_tail=None, deform_device=None):
    from vnet_tensorflow_amd import data, transforms as T
    shape, C, patch = SIZES[name]

    class DS(data.VolumeDataset):
        def _load(self, case, keep=True):
            if case not in self.cache:
                self.cache[case] = _case(name, 100 + case)
            return self.cache[case]
    tf = [T.BSplineDeformation(10, device=deform_device), T.ConfidenceCrop2(list(patch), rand_range=patch[0] // 4, probability=0.8), T.RandomNoise()]
    kw = {"device_tail": device_tail} if device_tail is not None else {}
    return DS("synthetic", ["c%d" % i for i in range(C)], "label", [0, 1], patch, 1, train=True, seed=1,
              synthetic={"Cases": CASES, "Shape": list(shape), "Spacing": list(SPACING)}, transforms=tf, **kw)


def _timed(fn, reps=7, warm=3):
    import torch
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


def step_kernels(name):
    import torch
    from vnet_tensorflow_amd import _lib, ops
    dev = torch.device("cuda", 0)
    shape, C, patch = SIZES[name]
    image, label = _case(name, 100)
    x, lab = torch.from_numpy(image).to(dev), torch.from_numpy(label).to(dev)
    coef = torch.from_numpy(np.random.default_rng(0).random(3 * 13 ** 3) * 10).to(dev)
    start = tuple((n - p) // 2 for n, p in zip(shape, patch))
    oi, ol = torch.empty(patch + (C,), dtype=torch.float32, device=dev), torch.empty(patch + (1,), dtype=torch.int32, device=dev)
    yl = ops.bspline_deform(lab, coef, SPACING, "label")
    need = _lib.lib().vnet_cc_table_ws_bytes(*shape)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def composition():
        ops.sample_patch(ops.bspline_deform(x, coef, SPACING, "image"), yl, start, patch, 0, 5.0, 12345, oi, ol)
    res = {"fused_ms": _timed(lambda: ops.deform_sample_patch(x, yl, coef, SPACING, start, patch, 0, 5.0, 12345, oi, ol)),
           "composition_ms": _timed(composition),
           "deform_image_ms": _timed(lambda: ops.bspline_deform(x, coef, SPACING, "image")),
           "deform_label_ms": _timed(lambda: ops.bspline_deform(lab, coef, SPACING, "label")),
           "table_ms": _timed(lambda: ops.component_table(yl, 4096, ws=ws))}
    res["components"] = int(ops.component_table(yl, 4096, ws=ws)[0])
    return res


def _per_sample(ds, samples):
    """Wall clock per sample on ONE loader thread after a first pass over the cases (uploads, host cache)."""
    import torch
    from vnet_tensorflow_amd import data
    t_first = time.perf_counter()
    for _ in data.Prefetcher(ds, depth=2, workers=1):
        pass
    torch.cuda.synchronize()
    first = time.perf_counter() - t_first
    n, t0 = 0, time.perf_counter()
    while n < samples:
        for img, lab in data.Prefetcher(ds, depth=2, workers=1):
            n += int(img.shape[0])
    torch.cuda.synchronize()
    return {"ms_per_sample": 1e3 * (time.perf_counter() - t0) / n, "first_pass_s": first, "samples": n}


def step_resident(name):
    import torch
    ds = _dataset(name, device_tail=torch.device("cuda", 0))
    r = _per_sample(ds, SAMPLES["resident"])
    r.update(ds.device_stats)
    return r


def step_loader(name):
    import torch
    return _per_sample(_dataset(name, deform_device=torch.device("cuda", 0)), SAMPLES["loader"])


def step_numpy(name):
    return _per_sample(_dataset(name), SAMPLES["numpy"])


STEPS = {"kernels": step_kernels, "resident": step_resident, "loader": step_loader, "numpy": step_numpy}


def child(step, name):
    """One step in a process of its own; None when it failed or ran out of time."""
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, name], capture_output=True, text=True, timeout=LIMIT[step])
    except subprocess.TimeoutExpired:
        return None, "ran past its limit of %d s" % LIMIT[step]
    if r.returncode != 0:
        return None, "exit status %d: %s" % (r.returncode, " ".join((r.stderr or r.stdout).strip().splitlines()[-1:]))
    return json.loads(r.stdout.strip().splitlines()[-1]), None


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        print(json.dumps(STEPS[sys.argv[2]](sys.argv[3])), flush=True)
        return
    out = ["a training sample through BSplineDeformation(10) + ConfidenceCrop2(p 0.8) + RandomNoise, per sample, one loader thread: the resident "
           "path (csrc/deform_sample.hip) against the loader path"]
    done, beats, under, fused_wins = True, True, True, []
    for name in SIZES:
        res = {}
        for step in ("kernels", "resident", "loader", "numpy"):
            res[step], why = child(step, name)
            if res[step] is None:
                out.append("%-8s %s: %s -- run ended" % (name, step, why))
                done = False
                break
        print(out[-1] if not done else name + " measured", flush=True)
        if not done:
            break
        k, a, b, h = res["kernels"], res["resident"], res["loader"], res["numpy"]
        out.append("%-8s kernels: fused %.3f ms   composition %.3f ms (image deformation alone %.3f ms)   label deformation %.3f ms   "
                   "table with its read-back %.3f ms (%d components)" % (name, k["fused_ms"], k["composition_ms"], k["deform_image_ms"],
                                                                        k["deform_label_ms"], k["table_ms"], k["components"]))
        out.append("         (a) resident path %.2f ms per sample (first pass %.2f s, %d uploads, %d evictions, %d samples on the NumPy tail)   "
                   "(b) loader path with DeformOnDevice %.1f ms per sample   (b) NumPy backend %.1f ms per sample"
                   % (a["ms_per_sample"], a["first_pass_s"], a["uploads"], a["evictions"], a["host_samples"], b["ms_per_sample"], h["ms_per_sample"]))
        beats = beats and a["ms_per_sample"] < b["ms_per_sample"] and a["ms_per_sample"] < h["ms_per_sample"]
        under = under and a["ms_per_sample"] < HEADLINE_MS
        fused_wins.append((name, k["fused_ms"] < k["composition_ms"]))
    if done:
        out.append("(a) beats both paths of (b) at both sizes: %s" % ("yes" if beats else "NO"))
        out.append("(a) stays under the headline step of %.1f ms at both sizes: %s" % (HEADLINE_MS, "yes" if under else "no"))
        out.append("the fused kernel beats the composition: %s (either way it saves the transient full-size deformed image per loader thread)"
                   % ", ".join("%s %s" % (n, "yes" if w else "NO") for n, w in fused_wins))
    else:
        out.append("not measured to the end")
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "deform_sample_bench.txt")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out), flush=True)
    sys.exit(0 if done and beats else 1)


if __name__ == "__main__":
    main()

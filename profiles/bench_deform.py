"""BSplineDeformation on the device against its NumPy backend, at 256^3 x 1 and 128^3 x 4, image plus label map each:
    kernel : vnet_bspline_deform_f32 + vnet_bspline_deform_i32 alone (HIP events after warm-up; also as algorithmic bytes -- every
             element read once and written once -- over 8 TB/s);
    device : the transform's device path as a loader thread runs it (ops.side_work: pinned staging, upload of image, label and
             coefficients, the two kernels, download, stream synchronise), wall clock;
    numpy  : the transform's NumPy backend (vnet_tensorflow_amd/deform.py), one thread, wall clock.
The condition: the device path, copies included, beats the NumPy backend at both sizes -- what TrainingSetting.DeformOnDevice's default
waits for.
Every step is a child process under its own time limit; a step that fails or runs out of time ends the run.
Usage: python profiles/bench_deform.py [outfile]   (default profiles/deform_bench.txt)"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12
SIZES = {"256^3x1": ((256, 256, 256), 1), "128^3x4": ((128, 128, 128), 4)}
SPACING = (1.0, 0.8, 1.25)
LIMIT = {"kernel": 120, "device": 120, "numpy": 420}


def _sample(name):
    shape, C = SIZES[name]
    rng = np.random.default_rng(0)
    image = rng.normal(100.0, 40.0, size=shape + (C,)).astype(np.float32)
    g = np.ogrid[tuple(slice(0, s) for s in shape)]
    label = (sum((a - s / 2.0) ** 2 for a, s in zip(g, shape)) <= (shape[0] / 3.0) ** 2).astype(np.int32)
    return {'image': image, 'label': label, 'spacing': SPACING}


def step_kernel(name):
    import torch
    from vnet_tensorflow_amd import ops
    dev = torch.device("cuda", 0)
    s = _sample(name)
    x, lab = torch.from_numpy(s['image']).to(dev), torch.from_numpy(s['label']).to(dev)
    coef = torch.from_numpy(np.random.default_rng(1).random(3 * 13 ** 3) * 10).to(dev)
    res = {}
    for what, fn in (("image", lambda: ops.bspline_deform(x, coef, SPACING, "image")), ("label", lambda: ops.bspline_deform(lab, coef, SPACING, "label"))):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(7):
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        res[what + "_ms"] = float(np.median(ts))
    res["bytes"] = 8.0 * (x.numel() + lab.numel())
    return res


def step_device(name):
    import torch
    from vnet_tensorflow_amd import transforms as T
    t = T.BSplineDeformation(10, device=torch.device("cuda", 0))
    s = _sample(name)
    ts = []
    for i in range(5):                                             # (the first call allocates the staging buffers: not in the median of 5)
        t0 = time.perf_counter()
        out = t(s, np.random.default_rng(i))
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms": float(np.median(ts)), "first_ms": ts[0], "checksum": float(out['image'].astype(np.float64).sum()), "label_voxels": int(out['label'].sum())}


def step_numpy(name):
    from vnet_tensorflow_amd import transforms as T
    t = T.BSplineDeformation(10)
    s = _sample(name)
    t0 = time.perf_counter()
    out = t(s, np.random.default_rng(4))
    return {"ms": (time.perf_counter() - t0) * 1e3, "checksum": float(out['image'].astype(np.float64).sum()), "label_voxels": int(out['label'].sum())}


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
        print(json.dumps({"kernel": step_kernel, "device": step_device, "numpy": step_numpy}[sys.argv[2]](sys.argv[3])), flush=True)
        return
    out = ["BSplineDeformation: device (csrc/deform.hip) against the NumPy backend (vnet_tensorflow_amd/deform.py); image + label per sample"]
    ok, done = True, True
    for name in SIZES:
        res = {}
        for step in ("kernel", "device", "numpy"):
            res[step], why = child(step, name)
            if res[step] is None:
                out.append("%-8s %s: %s -- run ended" % (name, step, why))
                done = False
                break
        print(out[-1] if not done else name + " measured", flush=True)
        if not done:
            break
        k, d, h = res["kernel"], res["device"], res["numpy"]
        kms = k["image_ms"] + k["label_ms"]
        out.append("%-8s kernels %7.3f ms (image %.3f + label %.3f; %6.1f MB algorithmic, %4.1f %% of 8 TB/s)   device path with copies %8.1f ms "
                   "(first call %.1f ms)   NumPy 1 thread %9.1f ms   device path is %.1fx faster"
                   % (name, kms, k["image_ms"], k["label_ms"], k["bytes"] / 1e6, 100.0 * k["bytes"] / (kms * 1e-3) / PEAK, d["ms"], d["first_ms"],
                      h["ms"], h["ms"] / d["ms"]))
        out.append("         seed 4 on both paths: image sum %.9e (device) %.9e (NumPy), label voxels %d (device) %d (NumPy)"
                   % (d["checksum"], h["checksum"], d["label_voxels"], h["label_voxels"]))
        ok = ok and d["ms"] < h["ms"]
    out.append("condition (the device path, copies included, beats the NumPy backend at both sizes): %s"
               % ("not measured" if not done else "holds" if ok else "DOES NOT HOLD"))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "deform_bench.txt")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out), flush=True)
    sys.exit(0 if done and ok else 1)


if __name__ == "__main__":
    main()

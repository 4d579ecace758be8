"""The reference's train tail -- ConfidenceCrop2(128, rand_range 32, probability 0.8) + RandomNoise -- on 256^3 x 1 and 256^3 x 4 prepared
cases (one blob plus 40 islands), samples per second:
    kernels : vnet_cc_table, vnet_window_count (a 128^3 window) and vnet_sample_patch (sigma 5) alone (HIP events after warm-up; also as
              algorithmic bytes -- the table: the label map read once; the count: the window read once; the sample: the patch read once and
              written once, image and label -- over 8 TB/s);
    device  : data.VolumeDataset(device_tail=...) behind data.Prefetcher with 3 threads, 8 cases resident, wall clock over 48 samples after
              the first pass (which uploads the cases and builds their tables; reported apart);
    numpy   : the same dataset without device_tail behind the same Prefetcher with 3 threads, pinned batches, wall clock over 12 samples;
    step    : the matching leg of bench.py on the same box (256^3 x 1: fp32_split3; 256^3 x 4: bf16 storage, 4 channels, 5 classes).
The condition: the device path delivers at least the step rate of the matching bench leg -- what TrainingSetting.SampleOnDevice's default
waits for.
Every step is a child process under its own time limit; a step that fails or runs out of time ends the run.
Usage: python profiles/bench_sample.py [outfile]   (default profiles/sample_bench.txt)"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12
SIZES = {"256^3x1": ((256, 256, 256), 1), "256^3x4": ((256, 256, 256), 4)}
PATCH = (128, 128, 128)
CASES = 8
LIMIT = {"kernels": 180, "device": 300, "numpy": 900, "step": 900}
BENCH_LEG = {"256^3x1": ["--compute", "fp32_split3"], "256^3x4": ["--compute", "bf16", "--channels", "4", "--classes", "5"]}


def _case(name, seed):
    shape, C = SIZES[name]
    rng = np.random.default_rng(seed)
    image = rng.normal(100.0, 40.0, size=shape + (C,)).astype(np.float32)
    g = np.ogrid[tuple(slice(0, s) for s in shape)]
    label = (sum((a - s * 0.55) ** 2 for a, s in zip(g, shape)) <= (shape[0] / 5.0) ** 2).astype(np.int32)
    for _ in range(40):
        p = [int(rng.integers(0, s - 4)) for s in shape]
        label[p[0]:p[0] + 3, p[1]:p[1] + 3, p[2]:p[2] + 3] = 1
    return image, label


class _Cases(object):
    """VolumeDataset over generated cases: `synthetic` with this module's generator instead of data.synthetic_case."""

    @staticmethod
    def dataset(name, device):
        from vnet_tensorflow_amd import data, transforms as T

        class DS(data.VolumeDataset):
            def _load(self, case, keep=True):
                if case not in self.cache:
                    self.cache[case] = _case(name, 100 + case)
                return self.cache[case]
        tf = [T.ConfidenceCrop2(list(PATCH), rand_range=32, probability=0.8), T.RandomNoise()]
        kw = {"device_tail": device} if device is not None else {}
        return DS("synthetic", ["c%d" % i for i in range(SIZES[name][1])], "label", [0, 1], PATCH, 1, train=True, seed=1,
                  synthetic={"Cases": CASES, "Shape": list(SIZES[name][0])}, transforms=tf, **kw)


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
    shape, C = SIZES[name]
    image, label = _case(name, 100)
    x, lab = torch.from_numpy(image).to(dev), torch.from_numpy(label).to(dev)
    L = _lib.lib()
    need = L.vnet_cc_table_ws_bytes(*shape)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(4096 * 8 + 1, dtype=torch.int32, device=dev)
    cnt = torch.empty(2, dtype=torch.int64, device=dev)
    oi, ol = torch.empty(PATCH + (C,), dtype=torch.float32, device=dev), torch.empty(PATCH + (1,), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    res = {"table_ms": _timed(lambda: _lib.check(L.vnet_cc_table(lab.data_ptr(), out.data_ptr() + 4 * 4096 * 8, out.data_ptr(), 4096, *shape,
                                                                 ws.data_ptr(), need, st), "vnet_cc_table")),
           "count_ms": _timed(lambda: _lib.check(L.vnet_window_count(lab.data_ptr(), cnt.data_ptr(), *shape, 64, 64, 64, *PATCH, 1, 255, st), "vnet_window_count")),
           "sample_ms": _timed(lambda: ops.sample_patch(x, lab, (64, 64, 64), PATCH, 0, 5.0, 12345, oi, ol))}
    nv, pv = float(np.prod(shape)), float(np.prod(PATCH))
    res.update(table_bytes=4.0 * nv, count_bytes=4.0 * pv, sample_bytes=8.0 * pv * (C + 1), components=int(out[-1]))
    return res


def _rate(ds, samples, workers=3):
    from vnet_tensorflow_amd import data
    import torch
    t_first = time.perf_counter()
    for _ in data.Prefetcher(ds, depth=4, workers=workers):        # one epoch: every case visited once (uploads / host cache)
        pass
    torch.cuda.synchronize()
    first = time.perf_counter() - t_first
    n, t0 = 0, time.perf_counter()
    while n < samples:
        for img, lab in data.Prefetcher(ds, depth=4, workers=workers):
            n += int(img.shape[0])
    torch.cuda.synchronize()
    return {"samples_per_s": n / (time.perf_counter() - t0), "first_epoch_s": first, "samples": n}


def step_device(name):
    import torch
    ds = _Cases.dataset(name, torch.device("cuda", 0))
    r = _rate(ds, 48)
    r.update(ds.device_stats)
    return r


def step_numpy(name):
    return _rate(_Cases.dataset(name, None), 12)


def step_step(name):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline",
                        "--no-c5", "--no-c2", "--no-x3", "--no-sustained"] + BENCH_LEG[name], capture_output=True, text=True, timeout=LIMIT["step"] - 30)
    if r.returncode != 0:
        raise SystemExit("bench.py: exit status %d: %s" % (r.returncode, " ".join(r.stderr.strip().splitlines()[-1:])))
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    return {"patches_per_s": float(json.loads(line)["value"])}


STEPS = {"kernels": step_kernels, "device": step_device, "numpy": step_numpy, "step": step_step}


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
    out = ["train tail ConfidenceCrop2(128, rand_range 32, p 0.8) + RandomNoise on prepared cases: device (csrc/sample.hip) against NumPy, 3 loader threads"]
    ok, done = True, True
    for name in SIZES:
        res = {}
        for step in ("kernels", "device", "numpy", "step"):
            res[step], why = child(step, name)
            if res[step] is None:
                out.append("%-8s %s: %s -- run ended" % (name, step, why))
                done = False
                break
        print(out[-1] if not done else name + " measured", flush=True)
        if not done:
            break
        k, d, h, s = res["kernels"], res["device"], res["numpy"], res["step"]
        pct = lambda b, ms: 100.0 * b / (ms * 1e-3) / PEAK
        out.append("%-8s kernels: table %.3f ms (%d components, %.1f %% of 8 TB/s)  window count %.3f ms (%.1f %%)  sample %.3f ms (%.1f %%)"
                   % (name, k["table_ms"], k["components"], pct(k["table_bytes"], k["table_ms"]), k["count_ms"], pct(k["count_bytes"], k["count_ms"]),
                      k["sample_ms"], pct(k["sample_bytes"], k["sample_ms"])))
        out.append("         device path %.1f samples/s (first epoch with %d uploads %.2f s, %d evictions, %d samples on the NumPy path)   "
                   "NumPy path %.2f samples/s   step %.1f patches/s"
                   % (d["samples_per_s"], d["uploads"], d["first_epoch_s"], d["evictions"], d["host_samples"], h["samples_per_s"], s["patches_per_s"]))
        ok = ok and d["samples_per_s"] >= s["patches_per_s"]
    out.append("condition (the device path delivers at least the step rate of the matching bench leg): %s"
               % ("not measured" if not done else "holds" if ok else "DOES NOT HOLD"))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sample_bench.txt")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out), flush=True)
    sys.exit(0 if done and ok else 1)


if __name__ == "__main__":
    main()

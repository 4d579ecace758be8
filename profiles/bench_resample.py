"""Resampling on the device against the NumPy restatement, at the sizes evaluate() meets on a 256^3 scan at half the voxel size:
    way in  : 256^3 x 1 -> 512^3                     (ops.resample linear)
    way back: 512^3 x K with the count map -> 256^3 x K, K = 2 and 5   (ops.resample linear, divisor=cnt)
For each: the kernel alone (HIP events after warm-up; also as algorithmic bytes -- source + count map read once, output written once --
over 8 TB/s), the device path with its PCIe copies (way in: upload, kernel, download; way back: kernel, download of the small result),
and the host path: the NumPy restatement (vnet_tensorflow_amd/resample.py) on one thread, with its time / 16 as what sixteen threads
could reach at best, plus -- on the way back -- the download of vol and cnt it needs first.
Usage: python profiles/bench_resample.py [outfile]   (default profiles/resample_bench.txt)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vnet_tensorflow_amd import ops, resample as R  # noqa: E402

PEAK = 8.0e12
THREADS = 16


def kernel_ms(fn, warm=2, reps=5):
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


def wall_ms(fn, reps=3):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def report(out, name, k_ms, nbytes, dev_ms, host_ms, host_copy_ms):
    best = host_ms / THREADS + host_copy_ms
    out.append("%-34s kernel %8.3f ms (%6.1f MB algorithmic, %5.1f %% of 8 TB/s)   device path with copies %9.1f ms   "
               "NumPy 1 thread %9.1f ms, /%d = %8.1f ms%s   device path is %.1fx the %d-thread bound"
               % (name, k_ms, nbytes / 1e6, 100.0 * nbytes / (k_ms * 1e-3) / PEAK, dev_ms, host_ms, THREADS, host_ms / THREADS,
                  (" + %.1f ms download of vol, cnt" % host_copy_ms) if host_copy_ms else "", best / dev_ms, THREADS))
    print(out[-1], flush=True)


def main():
    dev = torch.device("cuda", 0)
    out = ["resampling: device (csrc/resample.hip) against the NumPy restatement; %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__)]
    rng = np.random.default_rng(0)
    # ---- the way in ----
    n, m = 256, 512
    x = rng.standard_normal((n, n, n, 1), dtype=np.float32)
    size, ratio = (m, m, m), (0.5, 0.5, 0.5)
    tx = torch.from_numpy(x).to(dev)
    k = kernel_ms(lambda: ops.resample(tx, size, ratio))
    pinned = torch.from_numpy(x).pin_memory()
    d = wall_ms(lambda: ops.resample(pinned.to(dev, non_blocking=True), size, ratio).cpu())
    t = time.perf_counter()
    ref = R.linear(x, size, ratio)
    h = (time.perf_counter() - t) * 1e3
    err = float(np.abs(ops.resample(tx, size, ratio).cpu().numpy().astype(np.float64) - ref).max())
    report(out, "way in 256^3x1 -> 512^3", k, 4.0 * (n ** 3 + m ** 3), d, h, 0.0)
    out.append("    max|device - NumPy| = %.3e (one float rounding of max|x| = %.3e)" % (err, 2.0 ** -23 * float(np.abs(x).max())))
    del tx, ref, pinned
    # ---- the way back ----
    size, ratio = (n, n, n), (2.0, 2.0, 2.0)
    for K in (2, 5):
        vol = torch.rand((m, m, m, K), device=dev) * 8.0
        cnt = torch.randint(1, 9, (m, m, m), device=dev).to(torch.float32)
        k = kernel_ms(lambda: ops.resample(vol, size, ratio, divisor=cnt))
        d = wall_ms(lambda: ops.resample(vol, size, ratio, divisor=cnt).cpu())
        t = time.perf_counter()
        vol_np, cnt_np = vol.cpu().numpy(), cnt.cpu().numpy()
        c = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        ref = R.linear(vol_np, size, ratio, divisor=cnt_np)
        h = (time.perf_counter() - t) * 1e3
        err = float(np.abs(ops.resample(vol, size, ratio, divisor=cnt).cpu().numpy().astype(np.float64) - ref).max())
        report(out, "way back 512^3x%d / cnt -> 256^3x%d" % (K, K), k, 4.0 * (m ** 3 * (K + 1) + n ** 3 * K), d, h, c)
        out.append("    max|device - NumPy| = %.3e" % err)
        del vol, cnt, vol_np, cnt_np, ref
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "resample_bench.txt")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
